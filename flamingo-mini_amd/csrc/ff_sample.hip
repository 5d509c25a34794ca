// Token selection for sampled decoding: one row of logits -> one token id drawn under temperature / top-k / nucleus (top-p) filtering.
// What FlamingoModel._filter_logits + softmax + torch.multinomial do with a topk, a full descending sort of the vocabulary, two softmaxes,
// a cumsum and a scatter per step, here is one launch without a sort, so that it can sit inside the captured decode step:
//   both filters are THRESHOLDS on the logit value - the k-th largest value is the largest t with  count(x >= t) >= k,  the nucleus boundary
//   the largest t with  mass(x >= t) >= top_p * mass(all kept)  - and count and mass are monotone in t, so each is found by bisection on the
//   order-preserving integer key of the value, one pass over the row per key bit (bf16: 16 bits, fp32: 32).  Ties are kept on both sides by
//   construction (a threshold cannot split equal values), so the kept set depends on no sort order.
//   The draw is the inverse CDF in vocabulary order over the kept set: thread t owns the contiguous columns [t C, (t + 1) C).
// One 256-thread workgroup per row, on the row machinery of ff_row_keys.h (keys, the staged key image, the passes and their contracts).
// fp32 math.  Every sum has a fixed order (thread-local in column order, xor butterfly in the wave, wave 0..3, thread 0..255): equal inputs
// give equal bits, launch after launch, eager or replayed.
#include <cmath>

#include "ff_row_keys.h"

namespace ff {

constexpr int kSampleScratch = 2112;          // part[256] floats | last[256] ints | red[16] words: the key image starts 16-byte aligned behind them

template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void sample_token_kernel(int V, long long ld, const T* __restrict__ logits, float inv_temperature, int top_k, float top_p,
                                                           const float* __restrict__ u, long long* __restrict__ token) {
    constexpr int BITS = sizeof(T) == 2 ? 16 : 32;
    constexpr unsigned kNegInf = sizeof(T) == 2 ? 0x007Fu : 0x007FFFFFu;        // key of -inf: never kept
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    pin_args(V, ld, logits, inv_temperature, top_k, top_p, u, token);
    float* part = (float*)smem_raw;
    int* last = (int*)(smem_raw + 1024);
    float* red = (float*)(smem_raw + 2048);
    const int tid = threadIdx.x;
    const RowKeys<T, STAGED> keys(logits + (long long)blockIdx.x * ld, V, (unsigned short*)(smem_raw + kSampleScratch));

    const float xmax = ordered_value<BITS>(keys.stage((unsigned*)red));
    // exp(z - max z), z = x / temperature: the same bits wherever a column's weight is needed
    auto weight = [&](unsigned k) __attribute__((always_inline)) { return __expf((ordered_value<BITS>(k) - xmax) * inv_temperature); };

    const unsigned tk = top_k > 0 && top_k < V ? keys.kth_largest(top_k, (int*)red) : 0;      // top-k keeps the keys >= the k-th largest
    const unsigned lo = tk > kNegInf + 1 ? tk : kNegInf + 1;
    auto mass = [&](unsigned t) __attribute__((always_inline)) {
        float s = 0.f;
        keys.each([&](unsigned k) __attribute__((always_inline)) { if (k >= t) s += weight(k); });
        return block_sum<4>(s, red);
    };
    // nucleus: column i stays iff the mass strictly above its value is < top_p, i.e. iff key_i >= the largest t with mass(key >= t) >= top_p * Z
    unsigned thr = lo;
    if (top_p < 1.f) {
        const float Z = mass(lo), want = top_p * Z;
        unsigned s = 0;
        for (int bit = BITS - 1; bit >= 0; bit--) {
            const unsigned cand = s | (1u << bit);
            const float m = cand <= lo ? Z : mass(cand);                            // below the top-k threshold nothing more is added
            if (m >= want) s = cand;
        }
        thr = s > lo ? s : lo;
    }

    // inverse CDF in column order: thread t sums its columns, everyone scans the 256 partial sums in thread order, the owner walks its columns
    // (own()'s padding calls have key 0 < thr: never kept, so lk and tok stay below V)
    float p = 0.f;
    int lk = -1;
    keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
        if (k >= thr) { p += weight(k); lk = c; }
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
                if (k >= thr) {
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
static int sample_launch(int rows, int V, long long ld, const void* logits, float inv_t, int top_k, float top_p, const float* u, long long* token,
                         hipStream_t st) {
    if (STAGED) FF_TRY((allow_dynamic_lds<sample_token_kernel<T, STAGED>>(kSampleScratch + kRowStageMax * 2, "sample_token")));
    sample_token_kernel<T, STAGED><<<dim3(rows), dim3(256), row_keys_lds<STAGED>(kSampleScratch, V), st>>>(V, ld, (const T*)logits, inv_t, top_k, top_p, u, token);
    return check_launch("sample_token");
}

}  // namespace ff

extern "C" int ff_sample_token(int dtype, int rows, int vocab, long long ld, const void* logits, float temperature, int top_k, float top_p,
                               const float* u, long long* token, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(logits && u && token, FF_ERR_SHAPE, "ff_sample_token: null logits, u or token");
    FF_CHECK(rows > 0 && vocab > 0 && ld >= vocab, FF_ERR_SHAPE, "ff_sample_token: rows %d, vocab %d, ld %lld (need rows > 0, vocab > 0, ld >= vocab)", rows, vocab, ld);
    FF_CHECK(temperature > 0.f && std::isfinite(temperature), FF_ERR_SHAPE, "ff_sample_token: temperature %g must be positive and finite", (double)temperature);
    FF_CHECK(top_k >= 0, FF_ERR_SHAPE, "ff_sample_token: top_k %d must be >= 0 (0 = no top-k filter)", top_k);
    FF_CHECK(top_p > 0.f && top_p <= 1.f, FF_ERR_SHAPE, "ff_sample_token: top_p %g must be in (0, 1] (1 = no nucleus filter)", (double)top_p);
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_sample_token: dtype %d", dtype);
    const hipStream_t st = (hipStream_t)stream;
    const float inv_t = 1.f / temperature;
    return row_keys_dispatch(dtype, vocab, [&](auto t, auto staged) {
        return sample_launch<decltype(t), decltype(staged)::value>(rows, vocab, ld, logits, inv_t, top_k, top_p, u, token, st);
    });
}
