// Log-probability of the chosen token of a decode step: logprob[r] = x_tok - logsumexp(x) for the row the selection just used (argmax,
// ff_sample_token), one small launch inside the captured step - no host synchronisation, no vocabulary-wide temporary.
// The row pass RESTATES the forward of shifted_ce_fwd_kernel (ff_loss.hip) operation for operation - one 256-thread workgroup per row,
// the head / vector / tail walk, (m, s) pairs from (-FLT_MAX, 0), the wave and block combine with contraction off, lse = M + logf(S) - so
// that a row at the same address gets the lse bits the loss gives and logprob == -loss_row bit for bit: the loss kernels' per-element
// bounds (tests/test_hip_loss_bounds.py) then hold here too.  It is restated and not shared through a header so that ff_loss.hip keeps
// its instructions and resource remarks.  No reduction across workgroups and no atomics: equal inputs give equal bits, eager or replayed.
// The rules are normative in include/flamingo_fusion.h.
#include <cfloat>

#include "ff_common.h"

namespace ff {

// (as in ff_loss.hip) the V elements of a row whose start is only element-aligned: scalar head up to the next 16-byte boundary, 16-byte
// vectors for the body, scalar tail
template <typename T, typename F>
FF_DEV void logprob_row_vectors(const T* row, int V, F&& f) {   // f(column, value)
    constexpr int N = Vec<T>::N;
    int head = (int)(((16u - (unsigned)((unsigned long long)row & 15u)) & 15u) / sizeof(T));
    head = head < V ? head : V;
    const int nvec = (V - head) / N, tail0 = head + nvec * N;
    if ((int)threadIdx.x < head) f((int)threadIdx.x, to_f32(row[threadIdx.x]));
    // A decode step has few rows (32 workgroups on 256 CUs), so a thread's chain of dependent (m, s) updates must not also wait for one
    // load at a time: four of a thread's vectors are requested together and then visited in the thread's own order - the order of the
    // calls, and with it every bit, is that of the plain loop below.
    int v = threadIdx.x;
    for (; v + 3 * 256 < nvec; v += 4 * 256) {
        float x[4][N];
#pragma unroll
        for (int u = 0; u < 4; u++) Vec<T>::load(row + head + (v + u * 256) * N, x[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int e = 0; e < N; e++) f(head + (v + u * 256) * N + e, x[u][e]);
        }
    }
    for (; v < nvec; v += 256) {
        float x[N];
        Vec<T>::load(row + head + v * N, x);
#pragma unroll
        for (int e = 0; e < N; e++) f(head + v * N + e, x[e]);
    }
    for (int c = tail0 + threadIdx.x; c < V; c += 256) f(c, to_f32(row[c]));
}

template <typename T>
__global__ __launch_bounds__(256) void token_logprob_kernel(int V, long long ld, const T* __restrict__ logits, const long long* __restrict__ token,
                                                            const unsigned char* __restrict__ skip, float* __restrict__ logprob, float* __restrict__ lse) {
    __shared__ float sm[4], ss[4];
    pin_args(V, ld, logits, token, skip, logprob, lse);
    const int r = blockIdx.x;
    if (skip != nullptr && skip[r] != 0) {                     // (uniform over the workgroup) a skipped row is not read at all
        if (threadIdx.x == 0) {
            logprob[r] = 0.f;
            if (lse != nullptr) lse[r] = 0.f;
        }
        return;
    }
    const T* row = logits + (long long)r * ld;
    // (m, s) stands for s exp(m), from (-FLT_MAX, 0): a -inf logit adds exp(-inf) = 0, +inf and NaN end in a NaN row (see ff_loss.hip)
    float m = -FLT_MAX, s = 0.f;
    logprob_row_vectors(row, V, [&](int, float x) {
        if (x > m) { s = s * __expf(m - x) + 1.f; m = x; }
        else s += __expf(x - m);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        // each product rounds on its own (no fma), as in the loss
#pragma clang fp contract(off)
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const float mn = fmaxf(m, m2);
        s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
        m = mn;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[w] = m; ss[w] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])), S = 0.f;
        for (int k = 0; k < 4; k++) S += ss[k] * __expf(sm[k] - M);
        const float l = M + logf(S);
        if (lse != nullptr) lse[r] = l;
        const long long t = token[r];
        // a token outside [0, V) is an error no sum can hide: NaN, and nothing is read.  x_tok = -inf gives -inf - l = -inf.
        logprob[r] = (t < 0 || t >= V) ? __builtin_nanf("") : to_f32(row[t]) - l;
    }
}

}  // namespace ff

extern "C" int ff_token_logprob(int dtype, int rows, int vocab, long long ld, const void* logits, const long long* token, const unsigned char* skip,
                                float* logprob, float* lse, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(logits && token && logprob, FF_ERR_SHAPE, "ff_token_logprob: null logits, token or logprob");
    FF_CHECK(rows > 0 && vocab > 0 && ld >= vocab, FF_ERR_SHAPE, "ff_token_logprob: rows %d, vocab %d, ld %lld (need rows > 0, vocab > 0, ld >= vocab)", rows, vocab, ld);
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_token_logprob: dtype %d", dtype);
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == FF_DTYPE_BF16) token_logprob_kernel<bf16><<<dim3(rows), dim3(256), 0, st>>>(vocab, ld, (const bf16*)logits, token, skip, logprob, lse);
    else token_logprob_kernel<float><<<dim3(rows), dim3(256), 0, st>>>(vocab, ld, (const float*)logits, token, skip, logprob, lse);
    return check_launch("ff_token_logprob");
}
