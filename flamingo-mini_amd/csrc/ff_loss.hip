// Shifted next-token cross-entropy, forward and backward fused (reference modeling_flamingo.py:288-298:
// shift_logits = logits[..., :-1, :], shift_labels = labels[..., 1:], F.cross_entropy(..., reduction)).
// The reference materialises the shifted copy, a log-softmax and its backward (~10 kernels over batch*seq*vocab elements);
// here the forward reads the logits once (online max / sum-exp per row, one workgroup per token) and the backward reads them
// once more and writes d logits directly in the unshifted layout (last position = 0).  fp32 math on fp32 / bf16 logits.
// Label smoothing and z-loss (ff_shifted_ce_fwd_reg / _bwd_reg) ride on the same two passes: the same kernels with a trailing (eps, zl).
#include <cfloat>

#include "ff_common.h"
#include "ff_internal.h"

namespace ff {

// Visit the V elements of a row whose start is only element-aligned (vocab 50258: rows start 4 bytes off a 16-byte
// boundary): scalar head up to the next 16-byte boundary, 16-byte vectors for the body, scalar tail.
template <typename T, typename F>
FF_DEV void for_row_vectors(const T* row, int V, F&& f) {   // f(column, value)
    constexpr int N = Vec<T>::N;
    int head = (int)(((16u - (unsigned)((unsigned long long)row & 15u)) & 15u) / sizeof(T));
    head = head < V ? head : V;
    const int nvec = (V - head) / N, tail0 = head + nvec * N;
    if ((int)threadIdx.x < head) f((int)threadIdx.x, to_f32(row[threadIdx.x]));
    for (int v = threadIdx.x; v < nvec; v += 256) {
        float x[N];
        Vec<T>::load(row + head + v * N, x);
#pragma unroll
        for (int e = 0; e < N; e++) f(head + v * N + e, x[e]);
    }
    for (int c = tail0 + threadIdx.x; c < V; c += 256) f(c, to_f32(row[c]));
}

// loss_row[b*(L-1)+i] = logsumexp(logits[b,i,:]) - logits[b,i,labels[b,i+1]]   (0 where the label == ignore_index)
// Reg... is empty - the plain kernel, with the signature and the instructions it had before the pack existed - or (float eps, float zl),
// label smoothing and z-loss:   loss_row = lse - (1 - eps) x_t - eps mean(x) + zl lse^2   (lse stored as in the plain kernel); the row's sum
// of x is carried beside (m, s) and reduced over the wave and the four waves in a fixed order.
template <typename T, typename... Reg>
__global__ __launch_bounds__(256) void shifted_ce_fwd_kernel(int L, int V, const T* __restrict__ logits, const long long* __restrict__ labels,
                                                             long long ignore_index, float* __restrict__ loss_row, float* __restrict__ lse, Reg... reg) {
    constexpr bool REG = sizeof...(Reg) == 2;
    static_assert(REG || sizeof...(Reg) == 0, "shifted_ce_fwd_kernel: no trailing argument, or eps and zl");
    __shared__ float sm[4], ss[4], sq[REG ? 4 : 1];
    pin_args(L, V, logits, labels, ignore_index, loss_row, lse, reg...);
    const int r = blockIdx.x, b = r / (L - 1), i = r - b * (L - 1);
    const T* row = logits + ((long long)b * L + i) * V;
    // (m, s) stands for s exp(m): with s = 0 any finite m is the empty sum.  m must not start at -inf: a thread whose first logit is -inf
    // (a masked vocabulary entry) would add exp(-inf - -inf) = NaN.  From -FLT_MAX a -inf logit adds exp(-inf) = 0 and every other first
    // logit is a new maximum (or equal: + exp(0)); +inf and NaN logits still end in a NaN row, as in torch.
    float m = -FLT_MAX, s = 0.f, sx = 0.f;
    for_row_vectors(row, V, [&](int, float x) {
        if (x > m) { s = s * __expf(m - x) + 1.f; m = x; }
        else s += __expf(x - m);
        if constexpr (REG) sx += x;                            // a -inf logit makes the sum -inf: with eps > 0 that row's loss is +inf, as in torch
    });
    // combine (m, s) pairs: wave, then block
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        // each product rounds on its own (no fma): both lanes of a pair get the same bits, and finite rows keep the lse they always had
#pragma clang fp contract(off)
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const float mn = fmaxf(m, m2);
        s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
        m = mn;
        if constexpr (REG) sx += __shfl_xor(sx, o, 64);        // a + b = b + a: the same bits on both lanes of a pair
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sm[w] = m; ss[w] = s;
        if constexpr (REG) sq[w] = sx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])), S = 0.f;
        for (int k = 0; k < 4; k++) S += ss[k] * __expf(sm[k] - M);
        const float l = M + logf(S);
        lse[r] = l;
        const long long tgt = labels[(long long)b * L + i + 1];
        // a label outside [0, V) that is not ignore_index (e.g. the <EOC> id with an un-resized embedding) is an error: torch's
        // cross_entropy asserts on the device; here the row's loss becomes NaN (no out-of-bounds read), which no reduction can hide
        if constexpr (!REG) {
            loss_row[r] = tgt == ignore_index ? 0.f : ((tgt < 0 || tgt >= V) ? __builtin_nanf("") : l - to_f32(row[tgt]));
        } else if (tgt == ignore_index) {
            loss_row[r] = 0.f;
        } else if (tgt < 0 || tgt >= V) {
            loss_row[r] = __builtin_nanf("");
        } else {
            const float ez[2] = {reg...}, eps = ez[0], zl = ez[1];
            const float mean = (((sq[0] + sq[1]) + sq[2]) + sq[3]) / (float)V;
            float v = l - (1.f - eps) * to_f32(row[tgt]);
            if (eps > 0.f) v -= eps * mean;                    // (eps = 0 must not meet a -inf mean: 0 x inf)
            loss_row[r] = v + zl * l * l;
        }
    }
}

// dlogits[b,i,:] = (softmax(logits[b,i,:]) - onehot(label)) * g[b*(L-1)+i]   for i < L-1;   dlogits[b,L-1,:] = 0
// Reg... = (float eps, float zl):   (softmax (1 + 2 zl lse) - (1 - eps) onehot - eps / V) * g[b*(L-1)+i], the three factors once per row
template <typename T, typename... Reg>
__global__ __launch_bounds__(256) void shifted_ce_bwd_kernel(int L, int V, const T* __restrict__ logits, const long long* __restrict__ labels,
                                                             long long ignore_index, const float* __restrict__ lse, const float* __restrict__ g,
                                                             T* __restrict__ dlogits, Reg... reg) {
    constexpr bool REG = sizeof...(Reg) == 2;
    static_assert(REG || sizeof...(Reg) == 0, "shifted_ce_bwd_kernel: no trailing argument, or eps and zl");
    pin_args(L, V, logits, labels, ignore_index, lse, g, dlogits, reg...);
    const int b = blockIdx.x / L, i = blockIdx.x - b * L;
    const long long off = ((long long)b * L + i) * V;
    constexpr int N = Vec<T>::N;
    const T* row = logits + off;
    T* drow = dlogits + off;                                   // same element offset => same alignment phase as `row`
    const bool last = i == L - 1;
    const int r = b * (L - 1) + i;
    const long long tgt = last ? -1 : labels[(long long)b * L + i + 1];
    const float gr = (last || tgt == ignore_index) ? 0.f : ((tgt < 0 || tgt >= V) ? __builtin_nanf("") : g[r]), l = last ? 0.f : lse[r];   // bad label: NaN row
    // (with Reg only, once per row)  pk = 1 + 2 zl lse goes into the exponent, p pk = sign(pk) exp(x - (lse - log |pk|)): a product formed
    // after the exponential would lose a p below 2^-126 that v_exp_f32 flushes although p pk is a normal number (pk = 0: exp(-inf) = 0)
    const float ez[3] = {reg..., 0.f}, pk = 1.f + 2.f * ez[1] * l, sgn = pk < 0.f ? -1.f : 1.f, lk = l - logf(fabsf(pk));
    const float hot = 1.f - ez[0], eov = ez[0] / (float)V;
    auto dval = [&](int c, float x) {
        if constexpr (!REG) return gr == 0.f ? 0.f : (__expf(x - l) - (c == tgt ? 1.f : 0.f)) * gr;
        else return gr == 0.f ? 0.f : (__expf(x - lk) * sgn - (c == tgt ? hot : 0.f) - eov) * gr;      // at a -inf logit: -eps / V * g
    };
    int head = (int)(((16u - (unsigned)((unsigned long long)row & 15u)) & 15u) / sizeof(T));
    head = head < V ? head : V;
    const int nvec = (V - head) / N, tail0 = head + nvec * N;
    if ((int)threadIdx.x < head) drow[threadIdx.x] = from_f32<T>(dval(threadIdx.x, to_f32(row[threadIdx.x])));
    for (int v = threadIdx.x; v < nvec; v += 256) {
        const int c0 = head + v * N;
        float x[N];
        Vec<T>::load(row + c0, x);
#pragma unroll
        for (int e = 0; e < N; e++) x[e] = dval(c0 + e, x[e]);
        Vec<T>::store(drow + c0, x);
    }
    for (int c = tail0 + threadIdx.x; c < V; c += 256) drow[c] = from_f32<T>(dval(c, to_f32(row[c])));
}

}  // namespace ff

// eps in [0, 1], zl >= 0 and finite (the negated comparisons refuse NaN)
static bool ce_reg_ok(float eps, float zl) { return eps >= 0.f && eps <= 1.f && zl >= 0.f && zl <= FLT_MAX; }

extern "C" int ff_shifted_ce_fwd_reg(int dtype, int batch, int seq, int vocab, const void* logits, const long long* labels, long long ignore_index,
                                     float* loss_row, float* lse, float label_smoothing, float z_loss, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(batch > 0 && seq > 1 && vocab > 0 && logits && labels && loss_row && lse, FF_ERR_SHAPE, "ff_shifted_ce_fwd: bad arguments");
    FF_CHECK(ce_reg_ok(label_smoothing, z_loss), FF_ERR_UNSUPPORTED, "ff_shifted_ce_fwd_reg: label_smoothing %g must lie in [0, 1], z_loss %g be >= 0 and finite",
             (double)label_smoothing, (double)z_loss);
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_shifted_ce_fwd: dtype %d", dtype);
    const dim3 grid(batch * (seq - 1));
    hipStream_t st = (hipStream_t)stream;
    if (label_smoothing == 0.f && z_loss == 0.f) {            // nothing to add: the plain kernels, and so the plain bits
        if (dtype == FF_DTYPE_BF16) shifted_ce_fwd_kernel<bf16><<<grid, dim3(256), 0, st>>>(seq, vocab, (const bf16*)logits, labels, ignore_index, loss_row, lse);
        else shifted_ce_fwd_kernel<float><<<grid, dim3(256), 0, st>>>(seq, vocab, (const float*)logits, labels, ignore_index, loss_row, lse);
    } else if (dtype == FF_DTYPE_BF16) {
        shifted_ce_fwd_kernel<bf16><<<grid, dim3(256), 0, st>>>(seq, vocab, (const bf16*)logits, labels, ignore_index, loss_row, lse, label_smoothing, z_loss);
    } else {
        shifted_ce_fwd_kernel<float><<<grid, dim3(256), 0, st>>>(seq, vocab, (const float*)logits, labels, ignore_index, loss_row, lse, label_smoothing, z_loss);
    }
    return check_launch("shifted_ce_fwd");
}

extern "C" int ff_shifted_ce_fwd(int dtype, int batch, int seq, int vocab, const void* logits, const long long* labels, long long ignore_index,
                                 float* loss_row, float* lse, ff_stream_t stream) {
    return ff_shifted_ce_fwd_reg(dtype, batch, seq, vocab, logits, labels, ignore_index, loss_row, lse, 0.f, 0.f, stream);
}

extern "C" int ff_shifted_ce_bwd_reg(int dtype, int batch, int seq, int vocab, const void* logits, const long long* labels, long long ignore_index,
                                     const float* lse, const float* grad_row, void* dlogits, float label_smoothing, float z_loss, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(batch > 0 && seq > 1 && vocab > 0 && logits && labels && lse && grad_row && dlogits, FF_ERR_SHAPE, "ff_shifted_ce_bwd: bad arguments");
    FF_CHECK(ce_reg_ok(label_smoothing, z_loss), FF_ERR_UNSUPPORTED, "ff_shifted_ce_bwd_reg: label_smoothing %g must lie in [0, 1], z_loss %g be >= 0 and finite",
             (double)label_smoothing, (double)z_loss);
    FF_CHECK((((unsigned long long)logits ^ (unsigned long long)dlogits) & 15u) == 0, FF_ERR_UNSUPPORTED, "ff_shifted_ce_bwd: logits and dlogits must share their 16-byte alignment phase");
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_shifted_ce_bwd: dtype %d", dtype);
    const dim3 grid(batch * seq);
    hipStream_t st = (hipStream_t)stream;
    if (label_smoothing == 0.f && z_loss == 0.f) {
        if (dtype == FF_DTYPE_BF16) shifted_ce_bwd_kernel<bf16><<<grid, dim3(256), 0, st>>>(seq, vocab, (const bf16*)logits, labels, ignore_index, lse, grad_row, (bf16*)dlogits);
        else shifted_ce_bwd_kernel<float><<<grid, dim3(256), 0, st>>>(seq, vocab, (const float*)logits, labels, ignore_index, lse, grad_row, (float*)dlogits);
    } else if (dtype == FF_DTYPE_BF16) {
        shifted_ce_bwd_kernel<bf16><<<grid, dim3(256), 0, st>>>(seq, vocab, (const bf16*)logits, labels, ignore_index, lse, grad_row, (bf16*)dlogits, label_smoothing, z_loss);
    } else {
        shifted_ce_bwd_kernel<float><<<grid, dim3(256), 0, st>>>(seq, vocab, (const float*)logits, labels, ignore_index, lse, grad_row, (float*)dlogits, label_smoothing, z_loss);
    }
    return check_launch("shifted_ce_bwd");
}

extern "C" int ff_shifted_ce_bwd(int dtype, int batch, int seq, int vocab, const void* logits, const long long* labels, long long ignore_index,
                                 const float* lse, const float* grad_row, void* dlogits, ff_stream_t stream) {
    return ff_shifted_ce_bwd_reg(dtype, batch, seq, vocab, logits, labels, ignore_index, lse, grad_row, dlogits, 0.f, 0.f, stream);
}
