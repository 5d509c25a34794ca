// Token selection for sampled decoding: one row of logits -> one token id drawn under temperature / top-k / nucleus (top-p) filtering.
// What FlamingoModel._filter_logits + softmax + torch.multinomial do with a topk, a full descending sort of the vocabulary, two softmaxes,
// a cumsum and a scatter per step, here is one launch without a sort, so that it can sit inside the captured decode step:
//   both filters are THRESHOLDS on the logit value - the k-th largest value is the largest t with  count(x >= t) >= k,  the nucleus boundary
//   the largest t with  mass(x >= t) >= top_p * mass(all kept)  - and count and mass are monotone in t, so each is found by bisection on the
//   order-preserving integer key of the value, one pass over the row per key bit (bf16: 16 bits, fp32: 32).  Ties are kept on both sides by
//   construction (a threshold cannot split equal values), so the kept set depends on no sort order.
//   The draw is the inverse CDF in vocabulary order over the kept set: thread t owns the contiguous columns [t C, (t + 1) C).
//   One workgroup has its CU to itself (one wave per SIMD): every loop keeps four loads in flight, nothing else would hide their latency.
// One 256-thread workgroup per row.  A bf16 row of up to 65536 columns is staged ONCE into LDS as 16-bit keys (50258 columns: 98 KiB of the
// CU's 160 KiB) and every pass reads it from there with 16-byte LDS reads; longer bf16 rows and fp32 rows are re-read through L2 every pass.
// fp32 math.  Every sum has a fixed order (thread-local in column order, xor butterfly in the wave, wave 0..3, thread 0..255): equal inputs
// give equal bits, launch after launch, eager or replayed.
#include <cmath>

#include "ff_common.h"
#include "ff_internal.h"

namespace ff {

constexpr int kSampleScratch = 2112;          // part[256] floats | last[256] ints | red[16] words: the key image starts 16-byte aligned behind them
constexpr int kSampleStageMax = 65536;        // columns of a staged row (128 KiB of keys)

// order-preserving key of a float: a > b  <=>  key(a) > key(b) for all non-NaN values (-0 is +0).  A bf16 value's key is the top 16 bits.
template <int BITS> FF_DEV unsigned sample_key(float v) {
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0;
    return ((b >> 31) ? ~b : (b | 0x80000000u)) >> (32 - BITS);
}
template <int BITS> FF_DEV float sample_value(unsigned k) {
    const unsigned k32 = k << (32 - BITS);
    return __uint_as_float((k32 >> 31) ? (k32 & 0x7FFFFFFFu) : (~k32 & (0xFFFFFFFFu << (32 - BITS))));
}

// f(column, value) for the V elements of a row whose start is only element-aligned, like for_row_vectors of ff_loss.hip (scalar head up to
// the next 16-byte boundary, 16-byte vectors, scalar tail) - but one workgroup has a whole CU to itself here, one wave per SIMD, so
// nothing hides a load's latency unless the wave itself keeps several in flight: four vectors are requested before the first is used.
// The order in which a thread sees its columns is the order of the plain loop.
template <typename T, typename F>
FF_DEV void for_row_vectors4(const T* row, int V, F&& f) {
    constexpr int N = Vec<T>::N;
    int head = (int)(((16u - (unsigned)((unsigned long long)row & 15u)) & 15u) / sizeof(T));
    head = head < V ? head : V;
    const int nvec = (V - head) / N, tail0 = head + nvec * N;
    if ((int)threadIdx.x < head) f((int)threadIdx.x, to_f32(row[threadIdx.x]));
    for (int v = threadIdx.x; v < nvec; v += 1024) {
        typename Vec<T>::raw q[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int vj = v + 256 * j;
            q[j] = *(const typename Vec<T>::raw*)(row + head + (vj < nvec ? vj : v) * N);       // (out of range: the first vector again, unused)
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int vj = v + 256 * j;
            if (vj < nvec) {
#pragma unroll
                for (int e = 0; e < N; e++) f(head + vj * N + e, (float)q[j][e]);
            }
        }
    }
    for (int c = tail0 + threadIdx.x; c < V; c += 256) f(c, to_f32(row[c]));
}

FF_DEV int block_sum_int(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
FF_DEV unsigned block_max_uint(unsigned v, unsigned* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
        v = v > w ? v : w;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}

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
    unsigned short* sk = (unsigned short*)(smem_raw + kSampleScratch);             // STAGED: keys of columns [0, 8 ceil(V / 8)), the padding 0
    const int tid = threadIdx.x;
    const T* row = logits + (long long)blockIdx.x * ld;

    // f(key) for every column, in a fixed thread / order assignment; STAGED also visits the padding keys (0: below every threshold, all >= 1)
    auto each = [&](auto&& f) {
        if constexpr (STAGED) {
            const int nvec = (V + 7) >> 3;
            for (int v = tid; v < nvec; v += 1024) {                                 // four LDS reads in flight; past the end: padding keys
                uint4 q[4];
#pragma unroll
                for (int j = 0; j < 4; j++) q[j] = v + 256 * j < nvec ? *(const uint4*)(sk + (v + 256 * j) * 8) : uint4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const unsigned w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
                    for (int e = 0; e < 4; e++) { f(w[e] & 0xFFFFu); f(w[e] >> 16); }
                }
            }
        } else {
            for_row_vectors4(row, V, [&](int, float x) { f(sample_key<BITS>(x)); });
        }
    };
    // thread t's own columns [t C, (t + 1) C) in column order, C a multiple of 8 (STAGED: 16-byte LDS reads, four in flight; a vector may
    // reach into the padding keys); f(column, key) returns true to stop the walk
    const int C = ((((V + 255) >> 8) + 7) >> 3) << 3;
    const int c0 = tid * C < V ? tid * C : V, c1 = c0 + C < V ? c0 + C : V;
    auto own = [&](auto&& f) {
        if constexpr (STAGED) {
            bool stop = false;
            for (int c = c0; c < c1 && !stop; c += 32) {
                uint4 q[4];
#pragma unroll
                for (int j = 0; j < 4; j++) q[j] = c + 8 * j < c1 ? *(const uint4*)(sk + c + 8 * j) : uint4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const unsigned w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if (!stop) stop = f(c + 8 * j + 2 * e, w[e] & 0xFFFFu);
                        if (!stop) stop = f(c + 8 * j + 2 * e + 1, w[e] >> 16);
                    }
                }
            }
        } else {
            for (int c = c0; c < c1; c++)
                if (f(c, sample_key<BITS>(to_f32(row[c])))) break;
        }
    };

    unsigned kmax = 0;
    if constexpr (STAGED) {
        for_row_vectors4(row, V, [&](int c, float x) {
            const unsigned k = sample_key<BITS>(x);
            sk[c] = (unsigned short)k;
            kmax = k > kmax ? k : kmax;
        });
        for (int c = V + tid; c < ((V + 7) & ~7); c += 256) sk[c] = 0;
    } else {
        each([&](unsigned k) { kmax = k > kmax ? k : kmax; });
    }
    kmax = block_max_uint(kmax, (unsigned*)red);                                    // (its barriers also publish the key image)
    const float xmax = sample_value<BITS>(kmax);
    // exp(z - max z), z = x / temperature: the same bits wherever a column's weight is needed
    auto weight = [&](unsigned k) { return __expf((sample_value<BITS>(k) - xmax) * inv_temperature); };

    // top-k: the k-th largest key = the largest t with count(key >= t) >= k
    unsigned tk = 0;
    if (top_k > 0 && top_k < V) {
        for (int bit = BITS - 1; bit >= 0; bit--) {
            const unsigned cand = tk | (1u << bit);
            int n = 0;
            each([&](unsigned k) { n += k >= cand ? 1 : 0; });
            if (block_sum_int(n, (int*)red) >= top_k) tk = cand;
        }
    }
    const unsigned lo = tk > kNegInf + 1 ? tk : kNegInf + 1;
    auto mass = [&](unsigned t) {
        float s = 0.f;
        each([&](unsigned k) { if (k >= t) s += weight(k); });
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
    float p = 0.f;
    int lk = -1;
    own([&](int c, unsigned k) {
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
            own([&](int c, unsigned k) {
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
    const size_t lds = kSampleScratch + (STAGED ? (size_t)((V + 7) / 8) * 16 : 0);
    if (STAGED) {                                                                  // beyond 64 KiB of dynamic LDS a kernel has to ask once per device
        static bool attr_done[64] = {};
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev < 0 || dev >= 64 || !attr_done[dev]) {
            hipError_t e = hipFuncSetAttribute((const void*)sample_token_kernel<T, STAGED>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               kSampleScratch + kSampleStageMax * 2);
            FF_CHECK(e == hipSuccess, FF_ERR_LAUNCH, "hipFuncSetAttribute(sample_token lds): %s", hipGetErrorString(e));
            if (dev >= 0 && dev < 64) attr_done[dev] = true;
        }
    }
    sample_token_kernel<T, STAGED><<<dim3(rows), dim3(256), lds, st>>>(V, ld, (const T*)logits, inv_t, top_k, top_p, u, token);
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
    const hipStream_t st = (hipStream_t)stream;
    const float inv_t = 1.f / temperature;
    if (dtype == FF_DTYPE_BF16) {
        if (vocab <= kSampleStageMax) return sample_launch<bf16, true>(rows, vocab, ld, logits, inv_t, top_k, top_p, u, token, st);
        return sample_launch<bf16, false>(rows, vocab, ld, logits, inv_t, top_k, top_p, u, token, st);
    }
    if (dtype == FF_DTYPE_F32) return sample_launch<float, false>(rows, vocab, ld, logits, inv_t, top_k, top_p, u, token, st);
    FF_CHECK(false, FF_ERR_UNSUPPORTED, "ff_sample_token: dtype %d", dtype);
    return FF_OK;
}
