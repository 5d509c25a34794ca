// Classifier-free guidance on a decode step: out = lu + g (lc - lu) with lc / lu the log-softmax of the conditional / unconditional row,
// float32, one launch inside the captured step in front of the processors, the constraints and the selection.  g is ONE float in device
// memory: the captured launch serves every guidance scale.  One 256-thread workgroup per row (a decode step has at most a few dozen rows
// on 256 CUs, so the workgroup has its CU to itself: every loop keeps four 16-byte loads in flight, for_row_vectors4 of ff_row_keys.h).
//   pass 1: each of the two rows once, on its OWN 16-byte grid (the two may start at different phases): two running (max, sum) pairs from
//           (-FLT_MAX, 0) in the max-shifted form of the loss row pass, the wave and block combine of ff_logprob.hip with contraction off,
//           lse = M + logf(S) - known to every thread.
//   pass 2: the two rows again (about 100 KB each in bf16: from L2), on the CONDITIONAL row's grid; the unconditional vectors and the
//           float32 stores are 16 bytes wide at element alignment, which global memory takes.  out = fmaf(g, lc - lu, lu).
// No scratch, 32 bytes of LDS for the combine, no atomics: equal inputs give equal bits, eager or replayed.  Occupancy floor of the plan:
// 4 waves per SIMD (at most 128 registers) - one resident workgroup needs one.  The rules are normative in include/flamingo_fusion.h.
#include <cfloat>

#include "ff_row_keys.h"

namespace ff {

template <typename T> struct VecU;            // the 16-byte vectors of Vec<T> at element alignment
template <> struct VecU<float> { typedef f32x4 raw __attribute__((aligned(4))); };
template <> struct VecU<bf16> { typedef bf16x8 raw __attribute__((aligned(2))); };
typedef f32x4 f32x4_u __attribute__((aligned(4)));

struct MaxSum {                               // (m, s) stands for s exp(m)
    float m = -FLT_MAX, s = 0.f;
    FF_DEV void add(float x) {
        if (x > m) { s = s * __expf(m - x) + 1.f; m = x; }
        else s += __expf(x - m);
    }
    // the row's logsumexp, in every thread; sm / ss: 4 floats of LDS each
    FF_DEV float lse(float* sm, float* ss) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma clang fp contract(off)
            const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
            const float mn = fmaxf(m, m2);
            s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
            m = mn;
        }
        if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = m; ss[threadIdx.x >> 6] = s; }
        __syncthreads();
        const float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        float S = 0.f;
        for (int k = 0; k < 4; k++) S += ss[k] * __expf(sm[k] - M);
        return M + logf(S);
    }
};

template <typename T>
__global__ __launch_bounds__(256) void guided_logits_kernel(int V, long long ld_c, const T* __restrict__ cond, long long ld_u, const T* __restrict__ uncond,
                                                            const float* __restrict__ scale, float* __restrict__ out, long long ld_o) {
    constexpr int N = Vec<T>::N;
    __shared__ float sm[2][4], ss[2][4];
    pin_args(V, ld_c, cond, ld_u, uncond, scale, out, ld_o);
    const T* xc = cond + (long long)blockIdx.x * ld_c;
    const T* xu = uncond + (long long)blockIdx.x * ld_u;
    float* o = out + (long long)blockIdx.x * ld_o;
    const float g = *scale;

    MaxSum c, u;
    for_row_vectors4(xc, V, [&](int, float x) __attribute__((always_inline)) { c.add(x); });
    for_row_vectors4(xu, V, [&](int, float x) __attribute__((always_inline)) { u.add(x); });
    const float lse_c = c.lse(sm[0], ss[0]), lse_u = u.lse(sm[1], ss[1]);
    // +inf or NaN anywhere in a row ends in lse = NaN (see ff_loss.hip): the whole output row is NaN then
    const bool nan_row = lse_c != lse_c || lse_u != lse_u;
    const float ninf = -__builtin_inff();

    auto guided = [&](float a, float b) __attribute__((always_inline)) {
        const float lc = a - lse_c, lu = b - lse_u;
        const float y = fmaf(g, lc - lu, lu);
        // an entry either row bans stays banned for every g: (1 - g) (-inf) must not come out as +inf or NaN
        return nan_row ? __builtin_nanf("") : ((a == ninf || b == ninf) ? ninf : y);
    };

    int head = (int)(((16u - (unsigned)((unsigned long long)xc & 15u)) & 15u) / sizeof(T));
    head = head < V ? head : V;
    const int nvec = (V - head) / N, tail0 = head + nvec * N;
    if ((int)threadIdx.x < head) o[threadIdx.x] = guided(to_f32(xc[threadIdx.x]), to_f32(xu[threadIdx.x]));
    for (int v = threadIdx.x; v < nvec; v += 1024) {
        typename Vec<T>::raw qc[4];
        typename Vec<T>::raw qu[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int vj = v + 256 * j < nvec ? v + 256 * j : v;                              // (out of range: the first vector again, unused)
            qc[j] = *(const typename Vec<T>::raw*)(xc + head + vj * N);
            qu[j] = *(const typename VecU<T>::raw*)(xu + head + vj * N);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int vj = v + 256 * j;
            if (vj < nvec) {
#pragma unroll
                for (int e = 0; e < N; e += 4) {
                    f32x4 y;
#pragma unroll
                    for (int i = 0; i < 4; i++) y[i] = guided((float)qc[j][e + i], (float)qu[j][e + i]);
                    *(f32x4_u*)(o + head + vj * N + e) = y;
                }
            }
        }
    }
    for (int col = tail0 + threadIdx.x; col < V; col += 256) o[col] = guided(to_f32(xc[col]), to_f32(xu[col]));
}

}  // namespace ff

extern "C" int ff_guided_logits(int dtype, int rows, int vocab, long long ld_cond, const void* cond, long long ld_uncond, const void* uncond,
                                const float* scale, float* out, long long ld_out, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(cond && uncond && scale && out, FF_ERR_SHAPE, "ff_guided_logits: null cond, uncond, scale or out");
    FF_CHECK(rows > 0 && vocab > 0 && ld_cond >= vocab && ld_uncond >= vocab && ld_out >= vocab, FF_ERR_SHAPE,
             "ff_guided_logits: rows %d, vocab %d, ld_cond %lld, ld_uncond %lld, ld_out %lld (need rows > 0, vocab > 0, every ld >= vocab)", rows, vocab, ld_cond, ld_uncond, ld_out);
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_guided_logits: dtype %d", dtype);
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == FF_DTYPE_BF16) guided_logits_kernel<bf16><<<dim3(rows), dim3(256), 0, st>>>(vocab, ld_cond, (const bf16*)cond, ld_uncond, (const bf16*)uncond, scale, out, ld_out);
    else guided_logits_kernel<float><<<dim3(rows), dim3(256), 0, st>>>(vocab, ld_cond, (const float*)cond, ld_uncond, (const float*)uncond, scale, out, ld_out);
    return check_launch("ff_guided_logits");
}
