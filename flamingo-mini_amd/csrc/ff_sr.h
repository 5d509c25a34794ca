// Stochastic rounding of fp32 results to bf16 storage (stochastic rounding): the rule, the random bits and the 8-element store
// shared by the SR instantiations of adamw_kernel and by ff_stochastic_round_bf16 (csrc/ff_optim.hip).  tests/sr_cases.py restates all of
// it in numpy; the kernels are held to that restatement bit for bit.
#pragma once
#include "ff_common.h"

namespace ff {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// Philox4x32 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the round function and constants of Random123) with
// kSrRounds rounds: 7, the count the paper lists as Crush-resistant, instead of its default of 10 (the same with a safety margin) -
// a vector with bf16 moments takes three calls, each two 32 x 32 -> 64-bit multiplies per round, beside an HBM stream.
constexpr int kSrRounds = 7;
FF_DEV void philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < kSrRounds; r++) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// One call serves the 8-element vector `vec` (element index within the tensor >> 3) of one stored array: key = the seed, counter =
// (vec low, vec high, step, stream_id << 2 | slot); slot 0 = parameter, 1 = exp_avg, 2 = exp_avg_sq; stream_id < 2^30 names the tensor.
// Nothing of the launch geometry enters, so the bits do not depend on alignment, chunking, bucketing or the path that stores them.
FF_DEV void sr_words(unsigned long long seed, long long vec, unsigned step, unsigned stream_slot, unsigned (&w)[4]) {
    philox4x32((unsigned)vec, (unsigned)((unsigned long long)vec >> 32), step, stream_slot, (unsigned)seed, (unsigned)(seed >> 32), w);
}
// element e of the tensor takes 16 bits of word (e & 7) >> 1: the low half if e is even, the high half if it is odd
FF_DEV unsigned sr_r16(const unsigned (&w)[4], int e) { return (w[(e & 7) >> 1] >> ((e & 1) * 16)) & 0xFFFFu; }

// The rule.  x finite with bit pattern b, r < 2^16: s = b + r; the stored bf16 is s >> 16, or b >> 16 where the carry reached past the
// largest finite bf16 (s's exponent field all ones).  The result is one of x's two bf16 neighbours in magnitude, x itself where it is
// representable, and exactly b & 0xFFFF of the 65536 values of r round away from zero.  Non-finite x: what from_f32<bf16> stores.
FF_DEV unsigned sr_bf16(float x, unsigned r) {
    const unsigned b = __float_as_uint(x);
    if ((b & 0x7F800000u) == 0x7F800000u) return __builtin_bit_cast(unsigned short, from_f32<bf16>(x));
    const unsigned s = b + r;
    return ((s & 0x7F800000u) == 0x7F800000u ? b : s) >> 16;
}
FF_DEV bf16 sr_bf16_value(float x, unsigned r) { return __builtin_bit_cast(bf16, (unsigned short)sr_bf16(x, r)); }

// 8 consecutive elements (one 16-byte store) rounded with the four words of their vector; NT: a nontemporal store
template <bool NT> FF_DEV void sr_store8(bf16* q, const float (&o)[8], const unsigned (&w)[4]) {
    u32x4 v;
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = sr_bf16(o[2 * k], w[k] & 0xFFFFu) | sr_bf16(o[2 * k + 1], w[k] >> 16) << 16;
    if constexpr (NT) __builtin_nontemporal_store(v, (u32x4*)q);
    else *(u32x4*)q = v;
}

}  // namespace ff
