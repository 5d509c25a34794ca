// Log-probabilities of MANY queried tokens per row: out[q] = (base[r] +) x_tok[q] - logsumexp(x_r) for the queries q a CSR table gives row r -
// the edges of a candidate trie's node, read from the logits of the LM step that ran the node (decoding.score_trie).  One launch per level
// of the trie, no vocabulary-wide temporary, the logits read once in their own dtype and never written.
// The row pass RESTATES that of token_logprob (ff_logprob.hip; itself the forward of ff_loss.hip) operation for operation - one 256-thread
// workgroup per row, the head / vector / tail walk with four vectors in flight, (m, s) pairs from (-FLT_MAX, 0), the wave combine with
// contraction off, the block combine, lse = M + logf(S) - so that a row at the same address gets the lse bits ff_token_logprob stores and each out[q]
// without base equals its logprob bit for bit: the bounds held there (tests/test_hip_logprob.py) hold here too.  It is restated and not
// shared through a header so that ff_logprob.hip and ff_loss.hip keep their instructions and resource remarks.
// Unlike ff_token_logprob (32 rows on 256 CUs) a level has hundreds to thousands of rows: the launch fills the chip and is a streaming
// read of rows * vocab elements; the four loads in flight per thread are kept because they also hide the latency inside a full CU.
// lse reaches the workgroup through one LDS word; the threads then serve the row's queries strided by 256 (the root of a 1000-class trie
// has more than 256).  No reduction across workgroups and no atomics: equal inputs give equal bits, eager or replayed.
// The rules (S1 - S5) are normative in include/flamingo_fusion.h.
#include <cfloat>

#include "ff_common.h"

namespace ff {

// (as in ff_logprob.hip) the V elements of a row whose start is only element-aligned: scalar head up to the next 16-byte boundary,
// 16-byte vectors for the body, scalar tail; four of a thread's vectors are requested together and visited in the plain loop's order
template <typename T, typename F>
FF_DEV void gather_row_vectors(const T* row, int V, F&& f) {   // f(column, value)
    constexpr int N = Vec<T>::N;
    int head = (int)(((16u - (unsigned)((unsigned long long)row & 15u)) & 15u) / sizeof(T));
    head = head < V ? head : V;
    const int nvec = (V - head) / N, tail0 = head + nvec * N;
    if ((int)threadIdx.x < head) f((int)threadIdx.x, to_f32(row[threadIdx.x]));
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
__global__ __launch_bounds__(256) void logprob_gather_kernel(int V, long long ld, int n_q, const T* __restrict__ logits, const int* __restrict__ row_first,
                                                             const int* __restrict__ tok, const float* __restrict__ base, float* __restrict__ out) {
    __shared__ float sm[4], ss[4], sl;
    pin_args(V, ld, n_q, logits, row_first, tok, base, out);
    const int r = blockIdx.x;
    // S4: the bounds as given, clamped into [0, n_q] - whatever the table holds, every q below lies in [0, n_q)
    const int q0 = min(max(row_first[r], 0), n_q), q1 = min(max(row_first[r + 1], 0), n_q);
    if (q1 <= q0) return;                                      // S3 (uniform over the workgroup): a row without queries is not read
    const T* row = logits + (long long)r * ld;
    // (m, s) stands for s exp(m), from (-FLT_MAX, 0): a -inf logit adds exp(-inf) = 0, +inf and NaN end in a NaN row (see ff_loss.hip)
    float m = -FLT_MAX, s = 0.f;
    gather_row_vectors(row, V, [&](int, float x) {
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
        // ff_token_logprob's build forms this sum as a chain of fused multiply-adds; it is spelled out here so that the bits do not hang
        // on what the compiler makes of `S += a * b` in this unit (it packs the products and adds them unfused)
        for (int k = 0; k < 4; k++) S = __builtin_fmaf(ss[k], __expf(sm[k] - M), S);
        sl = M + logf(S);
    }
    __syncthreads();
    const float l = sl;
    const bool add = base != nullptr;
    const float b = add ? base[r] : 0.f;
    for (int q = q0 + (int)threadIdx.x; q < q1; q += 256) {
        const int t = tok[q];
        // S2: a token outside [0, V) is an error no sum can hide: NaN, and nothing is read.  x_tok = -inf gives -inf - l = -inf.
        float lp = (t < 0 || t >= V) ? __builtin_nanf("") : to_f32(row[t]) - l;
        if (add) {
            // the one fp32 add, rounded once, never contracted with the subtraction
#pragma clang fp contract(off)
            lp = b + lp;
        }
        out[q] = lp;
    }
}

}  // namespace ff

extern "C" int ff_logprob_gather(int dtype, int rows, int vocab, long long ld, const void* logits, const int* row_first, const int* tok, int n_q,
                                 const float* base, float* out, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(logits && row_first && tok && out, FF_ERR_SHAPE, "ff_logprob_gather: null logits, row_first, tok or out");
    FF_CHECK(rows > 0 && vocab > 0 && ld >= vocab && n_q > 0, FF_ERR_SHAPE,
             "ff_logprob_gather: rows %d, vocab %d, ld %lld, n_q %d (need rows > 0, vocab > 0, ld >= vocab, n_q > 0)", rows, vocab, ld, n_q);
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_logprob_gather: dtype %d", dtype);
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == FF_DTYPE_BF16) logprob_gather_kernel<bf16><<<dim3(rows), dim3(256), 0, st>>>(vocab, ld, n_q, (const bf16*)logits, row_first, tok, base, out);
    else logprob_gather_kernel<float><<<dim3(rows), dim3(256), 0, st>>>(vocab, ld, n_q, (const float*)logits, row_first, tok, base, out);
    return check_launch("ff_logprob_gather");
}
