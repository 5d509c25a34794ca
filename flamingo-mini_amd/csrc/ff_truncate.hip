// Token selection under the truncation samplers: one row of logits -> one token id drawn under temperature / top-k / nucleus filtering (the
// rules of ff_sample.hip, restated here - that unit is untouched) and then min_p, typical_p, epsilon_cutoff and eta_cutoff, in transformers'
// order, in ONE launch without a sort, so that the whole chain can sit inside the captured decode step.
//   Every rule is a function of a column's VALUE given sums over the current kept set, so the kept set is always
//       { key >= thr }  intersected with  { dkey(key) <= band }
//   where thr is a running threshold on the order-preserving key of the value and `band` the typical-sampling limit on the key of the
//   non-negative fp32 distance d (all ones = no band).  With z' = (x - max x) / T, w = exp(z') and, over a kept set, Z = sum w, S1 = sum w z':
//     min_p     q_i >= min_p max q  <=>  w_i >= min_p: the smallest such key, found by a search over KEYS (w is monotone in the key) that
//               touches no column - it raises thr.
//     typical   -log r_i - H = S1 / Z - z'_i (the log Z terms cancel), so d_i = |A - z'_i| with A = S1 / Z: one pass for (Z, S1), then the
//               largest t with mass(dkey < t) < typical_p Z by bisection on the 31 value bits of dkey, two bits per pass; kept: dkey <= t.
//     epsilon   r_i >= eps  <=>  w_i >= eps Z: one pass for Z and the largest kept key (typical may have dropped the row's maximum), then
//               the key search, capped at that largest key ("or the largest value") - it raises thr.
//     eta       one pass for (Z, S1, largest kept key); eta* Z = min(eta Z, sqrt(eta) exp(A)) because exp(-H) = exp(A) / Z; the key search.
//   A stage that is off costs no pass.  A threshold cannot split equal values, so ties are kept or dropped together at every stage, and every
//   stage keeps the columns of its largest kept value: the kept set is never empty.
//   The draw is ff_sample.hip's: the inverse CDF in vocabulary order over the kept set, thread t owning the columns [t C, (t + 1) C).
// One 256-thread workgroup per row, on the row machinery of ff_row_keys.h and under its contracts: every pass compares against thr >= 1, so
// the padding keys never act; every functor is always_inline; the loops keep four loads in flight.  fp32 math.  Every sum has the fixed
// order of ff_sample.hip (thread-local in column order, xor butterfly in the wave, wave 0..3, thread 0..255): equal inputs give equal bits,
// launch after launch, eager or replayed.
#include <cmath>

#include "ff_row_keys.h"

namespace ff {

constexpr int kTruncScratch = 2112;           // part[256] floats | last[256] ints | red[16] words: the key image starts 16-byte aligned behind them

template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void truncated_draw_kernel(int V, long long ld, const T* __restrict__ logits, float inv_temperature, int top_k, float top_p,
                                                             float min_p, float typical_p, float eps_cut, float eta_cut, const float* __restrict__ u,
                                                             long long* __restrict__ token) {
    constexpr int BITS = sizeof(T) == 2 ? 16 : 32;
    constexpr unsigned kNegInf = sizeof(T) == 2 ? 0x007Fu : 0x007FFFFFu;        // key of -inf: never kept
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    pin_args(V, ld, logits, inv_temperature, top_k, top_p, min_p, typical_p, eps_cut, eta_cut, u, token);
    float* part = (float*)smem_raw;
    int* last = (int*)(smem_raw + 1024);
    float* red = (float*)(smem_raw + 2048);
    const int tid = threadIdx.x;
    const RowKeys<T, STAGED> keys(logits + (long long)blockIdx.x * ld, V, (unsigned short*)(smem_raw + kTruncScratch));

    const unsigned kmax = keys.stage((unsigned*)red);
    const float xmax = ordered_value<BITS>(kmax);
    // z' = (x - max x) / T and exp(z'): the same bits wherever a column's value or weight is needed
    auto zrel = [&](unsigned k) __attribute__((always_inline)) { return (ordered_value<BITS>(k) - xmax) * inv_temperature; };
    auto weight = [&](unsigned k) __attribute__((always_inline)) { return __expf(zrel(k)); };

    // ---- rules 1 and 2: top-k and the nucleus, as ff_sample.hip has them ----
    const unsigned tk = top_k > 0 && top_k < V ? keys.kth_largest(top_k, (int*)red) : 0;
    const unsigned lo = tk > kNegInf + 1 ? tk : kNegInf + 1;
    unsigned thr = lo;
    if (top_p < 1.f) {
        auto mass = [&](unsigned t) __attribute__((always_inline)) {
            float s = 0.f;
            keys.each([&](unsigned k) __attribute__((always_inline)) { if (k >= t) s += weight(k); });
            return block_sum<4>(s, red);
        };
        const float Z = mass(lo), want = top_p * Z;
        unsigned s = 0;
        for (int bit = BITS - 1; bit >= 0; bit--) {
            const unsigned cand = s | (1u << bit);
            const float m = cand <= lo ? Z : mass(cand);
            if (m >= want) s = cand;
        }
        thr = s > lo ? s : lo;
    }

    // ---- the kept set from here on: key >= thr and dkey <= band ----
    float A = 0.f;                             // typical sampling's centre, S1 / Z over K2
    unsigned band = 0xFFFFFFFFu;
    // the order-preserving key of the distance d = |-log r - H| >= 0 (the bits of a non-negative float): ONE expression, every pass
    auto dkey = [&](unsigned k) __attribute__((always_inline)) { return __float_as_uint(fabsf(A - zrel(k))); };
    auto kept = [&](unsigned k) __attribute__((always_inline)) { return k >= thr && dkey(k) <= band; };
    // one pass: Z = sum w, S1 = sum w z' and the largest key, over the kept set
    float Z = 0.f, S1 = 0.f;
    unsigned top = 0;
    auto stats = [&]() __attribute__((always_inline)) {
        float s = 0.f, s1 = 0.f;
        unsigned t = 0;
        keys.each([&](unsigned k) __attribute__((always_inline)) {
            if (kept(k)) {
                const float z = zrel(k), w = __expf(z);
                s += w;
                s1 += w > 0.f ? w * z : 0.f;                                       // (an underflowed weight times z' = -inf would be a NaN)
                t = k > t ? k : t;
            }
        });
        Z = block_sum<4>(s, red);
        S1 = block_sum<4>(s1, red + 4);
        top = block_max_uint(t, (unsigned*)red + 8);
    };
    // the smallest key in [thr, khi] whose weight is >= bound, khi itself counting as such ("or the largest value"): a search over keys -
    // the weight is monotone in the key - of at most 32 steps that reads no column.  khi < thr (a row without a kept column): thr.
    auto raised = [&](float bound, unsigned khi) __attribute__((always_inline)) {
        unsigned a = thr, b = khi;
        while (a < b) {
            const unsigned mid = a + ((b - a) >> 1);
            if (weight(mid) >= bound) b = mid; else a = mid + 1;
        }
        return a;
    };

    // ---- rule 3: min_p (max q is the row's maximum: weight 1) ----
    if (min_p > 0.f) thr = raised(min_p, kmax);

    // ---- rule 4: typical_p ----
    if (typical_p < 1.f) {
        stats();
        const float want = typical_p * Z;
        A = S1 / Z;
        // the largest t with mass(dkey < t) < want, over the 31 value bits of dkey (d >= 0: the sign bit is clear).  TWO bits per pass: the
        // three candidates c1 < c2 < c3 (the lower bit, the upper bit, both) are summed side by side - each sum holds, in the pass's fixed
        // order, exactly the weights a pass of its own would add, and the masses are monotone in the candidate, so the result is that of 31
        // one-bit passes, in 16 - and one exponential serves all three.  The last pass has bit 0 alone: c1 = t, c3 = c2.
        unsigned t = 0;
        for (int hi = 30; hi >= 0; hi -= 2) {
            const unsigned low = hi > 0 ? 1u << (hi - 1) : 0u;
            const unsigned c1 = t | low, c2 = t | (1u << hi), c3 = c2 | low;
            float m1 = 0.f, m2 = 0.f, m3 = 0.f;
            keys.each([&](unsigned k) __attribute__((always_inline)) {
                if (k >= thr) {
                    const unsigned dk = dkey(k);
                    if (dk < c3) {
                        const float w = weight(k);
                        m3 += w;
                        if (dk < c2) m2 += w;
                        if (dk < c1) m1 += w;
                    }
                }
            });
            m1 = block_sum<4>(m1, red);
            m2 = block_sum<4>(m2, red + 4);
            m3 = block_sum<4>(m3, red + 8);
            t = m3 < want ? c3 : (m2 < want ? c2 : (m1 < want ? c1 : t));
        }
        band = t;
    }

    // ---- rule 5: epsilon_cutoff ----
    if (eps_cut > 0.f) {
        stats();
        thr = raised(eps_cut * Z, top);
    }

    // ---- rule 6: eta_cutoff ----
    if (eta_cut > 0.f) {
        stats();
        thr = raised(fminf(eta_cut * Z, sqrtf(eta_cut) * expf(S1 / Z)), top);
    }

    // ---- rule 7: the inverse CDF in column order (ff_sample.hip's draw over the kept set; own()'s padding calls have key 0 < thr) ----
    float p = 0.f;
    int lk = -1;
    keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
        if (kept(k)) { p += weight(k); lk = c; }
        return false;
    });
    __syncthreads();
    part[tid] = p;
    last[tid] = lk;
    __syncthreads();
    float S = 0.f;
    for (int t = 0; t < 256; t++) S += part[t];
    const float target = u[blockIdx.x] * S;
    float E = 0.f, E_own = 0.f;
    int owner = -1, fallback = -1;
    for (int t = 0; t < 256; t++) {
        const float En = E + part[t];
        if (owner < 0 && En > target) { owner = t; E_own = E; }
        E = En;
        fallback = last[t] > fallback ? last[t] : fallback;                         // the last kept column of the row
    }
    // rounding (or a NaN / +inf / all -inf row, whose token is unspecified) may leave no owner, or an owner whose walk never passes the
    // target: the last kept column then - and whatever happened, a token inside [0, V)
    if (tid == (owner < 0 ? 0 : owner)) {
        int tok = owner < 0 ? fallback : lk;
        if (owner >= 0) {
            float acc = E_own;
            keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
                if (kept(k)) {
                    acc += weight(k);
                    if (acc > target) { tok = c; return true; }
                }
                return false;
            });
        }
        tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
        token[blockIdx.x] = tok;
    }
}

template <typename T, bool STAGED>
static int truncated_launch(int rows, int V, long long ld, const void* logits, float inv_t, int top_k, float top_p, float min_p, float typical_p, float eps_cut,
                            float eta_cut, const float* u, long long* token, hipStream_t st) {
    if (STAGED) FF_TRY((allow_dynamic_lds<truncated_draw_kernel<T, STAGED>>(kTruncScratch + kRowStageMax * 2, "truncated_draw")));
    truncated_draw_kernel<T, STAGED><<<dim3(rows), dim3(256), row_keys_lds<STAGED>(kTruncScratch, V), st>>>(V, ld, (const T*)logits, inv_t, top_k, top_p, min_p, typical_p,
                                                                                                            eps_cut, eta_cut, u, token);
    return check_launch("truncated_draw");
}

}  // namespace ff

extern "C" int ff_sample_token_truncated(int dtype, int rows, int vocab, long long ld, const void* logits, float temperature, int top_k, float top_p,
                                         float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff, const float* u, long long* token,
                                         ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(logits && u && token, FF_ERR_SHAPE, "ff_sample_token_truncated: null logits, u or token");
    FF_CHECK(rows > 0 && vocab > 0 && ld >= vocab, FF_ERR_SHAPE, "ff_sample_token_truncated: rows %d, vocab %d, ld %lld (need rows > 0, vocab > 0, ld >= vocab)", rows, vocab, ld);
    FF_CHECK(temperature > 0.f && std::isfinite(temperature), FF_ERR_SHAPE, "ff_sample_token_truncated: temperature %g must be positive and finite", (double)temperature);
    FF_CHECK(top_k >= 0, FF_ERR_SHAPE, "ff_sample_token_truncated: top_k %d must be >= 0 (0 = no top-k filter)", top_k);
    FF_CHECK(top_p > 0.f && top_p <= 1.f, FF_ERR_SHAPE, "ff_sample_token_truncated: top_p %g must be in (0, 1] (1 = no nucleus filter)", (double)top_p);
    FF_CHECK(min_p >= 0.f && min_p <= 1.f, FF_ERR_SHAPE, "ff_sample_token_truncated: min_p %g must be in [0, 1] (0 = off)", (double)min_p);
    FF_CHECK(typical_p > 0.f && typical_p <= 1.f, FF_ERR_SHAPE, "ff_sample_token_truncated: typical_p %g must be in (0, 1] (1 = off)", (double)typical_p);
    FF_CHECK(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.f, FF_ERR_SHAPE, "ff_sample_token_truncated: epsilon_cutoff %g must be in [0, 1) (0 = off)", (double)epsilon_cutoff);
    FF_CHECK(eta_cutoff >= 0.f && eta_cutoff < 1.f, FF_ERR_SHAPE, "ff_sample_token_truncated: eta_cutoff %g must be in [0, 1) (0 = off)", (double)eta_cutoff);
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_sample_token_truncated: dtype %d", dtype);
    const hipStream_t st = (hipStream_t)stream;
    const float inv_t = 1.f / temperature;
    return row_keys_dispatch(dtype, vocab, [&](auto t, auto staged) {
        return truncated_launch<decltype(t), decltype(staged)::value>(rows, vocab, ld, logits, inv_t, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, u,
                                                                      token, st);
    });
}
