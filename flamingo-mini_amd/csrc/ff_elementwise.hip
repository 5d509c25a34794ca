// CLIP's QuickGELU, y = x * sigmoid(1.702 x) (transformers QuickGELUActivation, used by openai/clip-vit-* towers), as one pass.
// Stock PyTorch spells it as three elementwise kernels (scale, sigmoid, multiply) over the (batch * 257, 4096) MLP activations
// of each of the 24 ViT-L layers: 1.4 ms of a 45 ms step at config B.  Forward + derivative (the tower is frozen in Flamingo,
// the backward exists for completeness).
#include "ff_common.h"
#include "ff_internal.h"

namespace ff {

// Which products round on their own is written out here, not left to the compiler: it contracts the same expression in one pair of a
// vector's elements and not in the next, and differently once the code around it changes.  The one fused step is the fmaf below.
#pragma clang fp contract(off)

// One element, the plain formula: right down to x = -26 and what every activation a model produces takes.
template <bool BWD> FF_DEV float quick_gelu_plain(float x, float g) {
    const float s = 1.f / (1.f + __expf(-1.702f * x));
    return BWD ? g * s * fmaf(1.702f * x, 1.f - s, 1.f) : x * s;
}

// One element below x = -26: exp(-1.702 x) is inf from x = -52 down (the sigmoid 0 where x sigmoid is still 1e-37), and before that the
// sigmoid is a denormal.  Here exp(-1.702 x) is taken 2^-64 times smaller where it exceeds 2^64, so that neither it nor the sigmoid,
// 2^64 times larger, leaves the normal range; the result is multiplied by 2^-64 last: exact, or the one rounding into a denormal.
// Where the exponential is below 2^64 this is the plain formula, bit for bit (__expf(y) is exp2(y log2 e)).
template <bool BWD> FF_DEV float quick_gelu_far(float x, float g) {
    const float w = (-1.702f * x) * 1.44269504f;
    const bool far = w > 64.f;
    const float u = far ? 0x1p-64f : 1.f;
    const float s = 1.f / (u + __builtin_amdgcn_exp2f(far ? w - 64.f : w));
    return (BWD ? g * s * fmaf(1.702f * x, 1.f - s * u, 1.f) : x * s) * u;
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void quick_gelu_kernel(long long n, const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ out) {
    pin_args(n, x, dy, out);
    constexpr int N = Vec<T>::N;
    const long long nvec = n / N;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
        float v[N], g[N];
        Vec<T>::load(x + i * N, v);
        if (BWD) Vec<T>::load(dy + i * N, g);
        float lo = v[0];
#pragma unroll
        for (int e = 1; e < N; e++) lo = fminf(lo, v[e]);
        if (lo < -26.f) {   // some element of this vector needs the scaled form (never, for activations of a trained tower)
#pragma unroll
            for (int e = 0; e < N; e++) v[e] = quick_gelu_far<BWD>(v[e], BWD ? g[e] : 0.f);
        } else {
#pragma unroll
            for (int e = 0; e < N; e++) v[e] = quick_gelu_plain<BWD>(v[e], BWD ? g[e] : 0.f);
        }
        Vec<T>::store(out + i * N, v);
    }
    if (blockIdx.x == 0) {   // ragged tail
        const long long i = nvec * N + threadIdx.x;
        if (i < n) {
            const float xv = to_f32(x[i]), gv = BWD ? to_f32(dy[i]) : 0.f;
            out[i] = from_f32<T>(xv < -26.f ? quick_gelu_far<BWD>(xv, gv) : quick_gelu_plain<BWD>(xv, gv));
        }
    }
}

template <bool BWD> static int quick_gelu_launch(int dtype, long long n, const void* x, const void* dy, void* out, hipStream_t st) {
    FF_CHECK(n >= 0 && (n == 0 || (x && out && (!BWD || dy))), FF_ERR_SHAPE, "ff_quick_gelu: bad arguments");
    FF_CHECK(((uintptr_t)x | (uintptr_t)dy | (uintptr_t)out) % 16 == 0, FF_ERR_UNSUPPORTED, "ff_quick_gelu: pointers must be 16-byte aligned");
    if (n == 0) return FF_OK;
    const int per = dtype == FF_DTYPE_BF16 ? 8 : 4;
    const int grid = (int)std::min<long long>((n / per + 255) / 256 + 1, 256 * 16);
    if (dtype == FF_DTYPE_BF16) quick_gelu_kernel<bf16, BWD><<<dim3(grid), dim3(256), 0, st>>>(n, (const bf16*)x, (const bf16*)dy, (bf16*)out);
    else if (dtype == FF_DTYPE_F32) quick_gelu_kernel<float, BWD><<<dim3(grid), dim3(256), 0, st>>>(n, (const float*)x, (const float*)dy, (float*)out);
    else FF_CHECK(false, FF_ERR_UNSUPPORTED, "ff_quick_gelu: dtype %d", dtype);
    return check_launch("quick_gelu");
}

}  // namespace ff

extern "C" int ff_quick_gelu_fwd(int dtype, long long n, const void* x, void* y, ff_stream_t stream) {
    return ff::quick_gelu_launch<false>(dtype, n, x, nullptr, y, (hipStream_t)stream);
}
extern "C" int ff_quick_gelu_bwd(int dtype, long long n, const void* x, const void* dy, void* dx, ff_stream_t stream) {
    return ff::quick_gelu_launch<true>(dtype, n, x, dy, dx, (hipStream_t)stream);
}
