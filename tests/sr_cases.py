"""Stochastic rounding restated in numpy (a helper module, not a conftest): Philox4x32 with a `rounds` argument, the counter layout the
kernels use, and the rounding rule on uint32 bit patterns - what csrc/ff_sr.h is held to bit for bit (tests/test_hip_stochastic_rounding.py)
and what tests/test_sr_cases.py checks against Random123's published vectors and by enumerating every r.

    key     = (seed low 32, seed high 32)
    counter = (vec low 32, vec high 32, step, stream_id << 2 | slot)      vec = element index within the tensor >> 3
    slot    = 0 parameter, 1 exp_avg, 2 exp_avg_sq
    element e takes 16 bits of output word (e & 7) >> 1: the low half if e is even, the high half if it is odd

    sr_bf16(x, r): b = bits of x.  Not finite: what round-to-nearest stores (inf as it is, a NaN quiet with its upper payload).
    Else s = b + r (32-bit add); exponent field of s all ones (a carry past the largest finite bf16): b >> 16, else s >> 16."""
import numpy as np

ROUNDS = 7                                      # what the kernels run (csrc/ff_sr.h: kSrRounds)
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
SLOT_P, SLOT_M, SLOT_V = 0, 1, 2
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=ROUNDS):
    """counter: four uint32 arrays (or scalars) that broadcast; key: two.  Returns the four output words as uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & _MASK for x in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return [x.astype(np.uint32) for x in c]


def sr_bits(n, seed, stream_id, step, slot, rounds=ROUNDS):
    """The 16 random bits of elements 0 .. n - 1 of one stored array (uint32 array of values below 65536)."""
    assert 0 <= stream_id < 2 ** 30 and 0 <= slot < 4 and 0 <= seed < 2 ** 64
    e = np.arange(n, dtype=np.uint64)
    vec = e >> np.uint64(3)
    w = philox4x32((vec & _MASK, vec >> np.uint64(32), step & 0xFFFFFFFF, (stream_id << 2) | slot), (seed & 0xFFFFFFFF, seed >> 32), rounds)
    word = np.choose(((e & np.uint64(7)) >> np.uint64(1)).astype(np.int64), w)
    return (word >> ((e & np.uint64(1)).astype(np.uint32) * np.uint32(16))) & np.uint32(0xFFFF)


def f32_bits(x):
    return np.array(x, dtype=np.float32, order="C").view(np.uint32)


def sr_bf16(b, r):
    """b: uint32 bit patterns of fp32 values; r: 16-bit random numbers (broadcast).  Returns the stored bf16 bit patterns (uint16)."""
    b = np.asarray(b, dtype=np.uint32)
    r = np.asarray(r, dtype=np.uint32)
    assert int(r.max(initial=0)) < 65536
    b, r = np.broadcast_arrays(b, r)
    exp = np.uint32(0x7F800000)
    s = (b.astype(np.uint64) + r.astype(np.uint64)).astype(np.uint32)           # (wraps like the 32-bit add; a finite b never does)
    out = np.where((s & exp) == exp, b, s) >> np.uint32(16)
    nonfinite = (b & exp) == exp
    nan = nonfinite & ((b & np.uint32(0x007FFFFF)) != 0)
    out = np.where(nonfinite, b >> np.uint32(16), out)
    out = np.where(nan, out | np.uint32(0x0040), out)
    return out.astype(np.uint16)


def bf16_to_f64(h):
    """bf16 bit patterns (uint16) as float64 values"""
    return (np.asarray(h, dtype=np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def sr_bf16_of(x, r):
    """sr_bf16 on float values (rounded to fp32 first, as the kernel's result is): the stored values as float64"""
    return bf16_to_f64(sr_bf16(f32_bits(x), r))
