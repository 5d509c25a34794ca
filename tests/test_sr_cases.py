"""The numpy restatement of stochastic rounding (tests/sr_cases.py) checked on its own, without a GPU: Philox4x32 against Random123's
published known-answer vectors, the rounding rule by enumerating all 65536 values of r, and the counter layout's element mapping."""
import numpy as np
import pytest

import sr_cases as sr

ALL_R = np.arange(65536, dtype=np.uint32)


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox4x32_10_reproduces_the_published_vectors():
    """Random123's kat_vectors for philox4x32 with 10 rounds: counter 0 / key 0, and all ones."""
    assert _hex(sr.philox4x32((0, 0, 0, 0), (0, 0), rounds=10)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(sr.philox4x32((ones,) * 4, (ones, ones), rounds=10)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    # the kernels' 7 rounds are another function of the same inputs, and arrays broadcast element by element
    assert _hex(sr.philox4x32((0, 0, 0, 0), (0, 0), rounds=7)) != "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    both = sr.philox4x32((np.array([0, ones]), np.array([0, ones]), np.array([0, ones]), np.array([0, ones])), (np.array([0, ones]), np.array([0, ones])), 10)
    assert _hex(w[0] for w in both) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and _hex(w[1] for w in both) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_element_mapping_of_the_counter_layout():
    """Element e reads word (e & 7) >> 1 of the call for vector e >> 3, low half first; step, stream, slot and seed each select other bits."""
    n, seed, sid, step = 29, 0x0123456789ABCDEF, 5, 1000
    bits = sr.sr_bits(n, seed, sid, step, sr.SLOT_M)
    for e in (0, 1, 6, 7, 8, 15, 28):
        w = sr.philox4x32((e >> 3, 0, step, sid << 2 | 1), (0x89ABCDEF, 0x01234567))
        word = int(w[(e & 7) >> 1])
        assert int(bits[e]) == ((word >> 16) if e & 1 else (word & 0xFFFF)), e
    base = sr.sr_bits(64, seed, sid, step, 0)
    for other in (sr.sr_bits(64, seed + 1, sid, step, 0), sr.sr_bits(64, seed + (1 << 32), sid, step, 0), sr.sr_bits(64, seed, sid + 1, step, 0),
                  sr.sr_bits(64, seed, sid, step + 1, 0), sr.sr_bits(64, seed, sid, step, 1), sr.sr_bits(64, seed, sid, step, 2)):
        assert (other != base).mean() > 0.9
    # an element index past 2^35 reaches the counter's second word
    assert int(sr.philox4x32((0, 1, step, sid << 2), (0x89ABCDEF, 0x01234567))[0]) != int(sr.philox4x32((0, 0, step, sid << 2), (0x89ABCDEF, 0x01234567))[0])


@pytest.mark.parametrize("x", [0.75 - 1e-4, -0.3001, 1.0 + 2.0 ** -9, 3.0e-39, -1.7e-40, 2.0 ** -133 * 1.3, 1e30, -65504.25, 0.1])
def test_exactly_the_low_bits_of_x_round_away_from_zero(x):
    """Over all 65536 r: b & 0xFFFF of them give the neighbour farther from zero, the others the nearer one - and nothing else."""
    b = sr.f32_bits(x)
    lo = int(b) >> 16
    out = sr.sr_bf16(b, ALL_R).astype(np.int64)
    assert set(np.unique(out)) <= {lo, lo + 1}
    assert int((out == lo + 1).sum()) == int(b) & 0xFFFF
    # the two results are x's bf16 neighbours in magnitude, and the mean over r is x itself (unbiased)
    near, far = sr.bf16_to_f64(np.uint16(lo)), sr.bf16_to_f64(np.uint16(lo + 1))
    x32 = float(np.float32(x))
    assert abs(near) <= abs(x32) <= abs(far) and np.sign(near) in (0, np.sign(x32)) and np.sign(far) == np.sign(x32)
    mean = float(sr.bf16_to_f64(out.astype(np.uint16)).mean())
    assert abs(mean - x32) <= 2.0 ** -40 * abs(x32) + 1e-300


def test_representable_values_zeros_and_non_finite_values():
    rep = np.array([0.75, -0.3125, 1.0, 2.0 ** -126, 2.0 ** -133, -2.0 ** -130 * 1.5, 3.3895313892515355e38], dtype=np.float32)      # the last: the largest finite bf16
    b = sr.f32_bits(rep)
    assert (b & 0xFFFF == 0).all()
    for r in (0, 1, 0x8000, 0xFFFF):
        assert (sr.sr_bf16(b, r) == (b >> 16)).all(), r
    zeros = sr.f32_bits(np.array([0.0, -0.0], dtype=np.float32))
    assert (sr.sr_bf16(zeros[:, None], ALL_R[None, :]) == np.array([[0x0000], [0x8000]], dtype=np.uint16)).all()      # -0 stays -0
    inf = np.array([0x7F800000, 0xFF800000], dtype=np.uint32)
    assert (sr.sr_bf16(inf[:, None], ALL_R[None, :]) == np.array([[0x7F80], [0xFF80]], dtype=np.uint16)).all()
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001, 0xFFA00000], dtype=np.uint32)                     # quiet, with payload, signalling
    want = np.array([0x7FC0, 0xFFC0, 0x7FC1, 0x7FC0, 0xFFE0], dtype=np.uint16)
    assert (sr.sr_bf16(nan[:, None], ALL_R[None, :]) == want[:, None]).all()


def test_no_carry_past_the_largest_finite_value():
    """Above the largest finite bf16 (0x7F7F0000) a carry would make an infinity: those r store the truncation instead, every other r adds."""
    for b in (0x7F7F0001, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF):
        out = sr.sr_bf16(np.uint32(b), ALL_R)
        assert (out == np.uint16(b >> 16)).all(), hex(b)
        assert np.isfinite(sr.bf16_to_f64(out)).all()
    # one step below, both neighbours are finite and the count holds as everywhere else
    out = sr.sr_bf16(np.uint32(0x7F7E4000), ALL_R)
    assert int((out == 0x7F7F).sum()) == 0x4000 and int((out == 0x7F7E).sum()) == 65536 - 0x4000


def test_denormal_results_are_reached_by_the_same_rule():
    """An fp32 denormal lies between two bf16 denormals (or zero and the smallest one): plain bit arithmetic, no flush."""
    b = sr.f32_bits(np.float32(1e-45))                      # the smallest fp32 denormal, bit pattern 1
    out = sr.sr_bf16(b, ALL_R)
    assert int(b) == 1 and int((out == 1).sum()) == 1 and int((out == 0).sum()) == 65535
    b = np.uint32(0x80501234)                               # -(2^-127) * 1.25..., between two negative bf16 denormals
    out = sr.sr_bf16(b, ALL_R).astype(np.int64)
    assert set(np.unique(out)) == {int(b) >> 16, (int(b) >> 16) + 1} and (out >= 0x8000).all()
