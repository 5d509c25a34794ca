// Fused multi-tensor AdamW for the trainable parameters (resampler, gated xattn blocks, token embedding): SURVEY.md 8f2.
// One pass over param / grad / exp_avg / exp_avg_sq per step, fp32 math, 16-byte vector streams, up to 32 tensors per launch
// (the table travels in the kernel argument).  Semantics = torch.optim.AdamW (decoupled weight decay, bias correction):
//     p *= 1 - lr * wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// Reference training recipe: `--optim adamw_torch`, lr 1e-4 (training/train.sh:10-13).  HBM-bound: 7 streams per element.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include "ff_common.h"
#include "ff_internal.h"
#include "ff_sr.h"

namespace ff {

constexpr int kAdamTensors = 32;
constexpr int kAdamChunk = 256 * 128;  // elements per workgroup (16 sweeps of 8-element vectors: the per-workgroup table lookup is amortised)
constexpr long long kGradMaxBlocks = 1 << 22;       // workgroups per launch (x 256 threads stays far below 2^32; block_start stays an int)

// What every multi-tensor kernel of this file gets as (part of) its kernel argument: up to kAdamTensors tensors, cut into chunks of
// kAdamChunk elements, one workgroup per chunk; tensor k owns workgroups block_start[k] .. block_start[k + 1] - 1 of the launch.
struct ChunkTable {
    long long n[kAdamTensors];
    int block_start[kAdamTensors + 1];
    int count;
};

// this workgroup's chunk: elements base .. end - 1 of tensor ti, which has n elements
struct Chunk {
    int ti;
    long long n, base, end;
};
FF_DEV Chunk my_chunk(const ChunkTable& c) {
    int ti = 0;
#pragma unroll 1
    while (ti + 1 < c.count && (int)blockIdx.x >= c.block_start[ti + 1]) ti++;
    const long long n = c.n[ti];
    const long long base = (long long)((int)blockIdx.x - c.block_start[ti]) * kAdamChunk;
    return {ti, n, base, min(n, base + (long long)kAdamChunk)};
}

static long long chunks_of(long long n) { return (n + kAdamChunk - 1) / kAdamChunk; }
static long long grad_slots(int n_tensors, const long long* numels) {
    long long slots = 0;
    for (int i = 0; i < n_tensors; i++)
        if (numels[i] > 0) slots += chunks_of(numels[i]);
    return slots;
}

// The non-empty tensors of one call in launches of <= kAdamTensors tensors and <= kGradMaxBlocks workgroups.  fill(cnt, i) puts tensor i
// into entry cnt of the table `c` is part of; launch(blocks, slot) enqueues the kernel on that table, slot = the workgroups of the call's
// earlier launches.  Both return FF_OK or the error that ends the call.
template <typename Fill, typename Launch>
static int chunk_launches(const char* what, ChunkTable& c, int n_tensors, const long long* numels, Fill&& fill, Launch&& launch) {
    long long slot = 0;
    int i = 0;
    while (i < n_tensors) {
        int cnt = 0;
        long long blocks = 0;
        while (i < n_tensors && cnt < kAdamTensors) {
            if (numels[i] > 0) {
                const long long b = chunks_of(numels[i]);
                FF_CHECK(b <= kGradMaxBlocks, FF_ERR_SHAPE, "%s: tensor %d has %lld elements", what, i, numels[i]);
                if (blocks + b > kGradMaxBlocks) break;
                FF_TRY(fill(cnt, i));
                c.n[cnt] = numels[i];
                c.block_start[cnt] = (int)blocks;
                blocks += b;
                cnt++;
            }
            i++;
        }
        if (!cnt) break;
        c.block_start[cnt] = (int)blocks;
        c.count = cnt;
        FF_TRY(launch((int)blocks, slot));
        slot += blocks;
    }
    return FF_OK;
}

struct AdamTable {
    void* p[kAdamTensors];
    const void* g[kAdamTensors];
    void* m[kAdamTensors];
    void* v[kAdamTensors];
    float* w[kAdamTensors];  // fp32 master copies of the parameters (mixed-precision mode), else unused
    ChunkTable chunks;
    float lr, beta1, beta2, eps, decay, bc1, bc2_sqrt, grad_scale;
    const float* step_dev;   // capturable mode: the step count lives on the device (HIP-graph replays cannot change kernel arguments)
    const float* lr_dev;     // ... and so does the learning rate, when a scheduler is to stay effective under replay
    const float* grad_coef;  // CLIP kernels: device scalar multiplying every (grad_scale'd) gradient - the max-norm clip coefficient
    const float* skip;       // GUARD kernels: device scalar, != 0 = the step is not taken (ff_grad_guard found a non-finite gradient)
    unsigned long long seed;              // SR kernels: the Philox key, ...
    unsigned stream_id[kAdamTensors];     // ... each tensor's stream (< 2^30: the two low counter bits name the stored array) ...
    unsigned step;                        // ... and the number of the step being taken where it is not read from *step_dev
};

// T: storage type of the parameters' compute copy and of the gradients; ST: storage type of the two moments; MASTER: the update
// is applied to an fp32 master copy (t.w) and the compute copy is its rounding - what `--fp16` / bf16 autocast training keeps
// (training/train.sh:24), so that steps far below bf16 resolution of a weight (lr 1e-4) are not lost.
// bf16 parameters (NT): gradients, moments and master copies, touched once per step, are streamed with nontemporal accesses so that they
// do not evict what the next kernels read (37.52 -> 37.40 ms/step at config B in a same-box A/B); fp32 parameters use plain accesses.
// CLIP: every gradient is also multiplied by *t.grad_coef (gradient clipping by global norm, ff_grad_clip_coef); the kernels without it
// are the ones the unclipped step always ran.
// GT: storage type of the gradients - T, or float where the gradients are the fp32 accumulators of ff_grad_accumulate (ff_adamw_step_acc).
// GUARD (implies CLIP; ff_adamw_step_guarded): every workgroup reads *t.skip first and returns before it touches a tensor when it is set -
// a skipped launch is a no-op (no weight decay, no moment decay, no master write).  The read and the branch are wave-uniform.
// SR (ff_adamw_step_sr; bf16 parameters without master copies): every bf16 store - the parameter, and the moments where ST is bf16 - is
// rounded stochastically (ff_sr.h) instead of to nearest, with the bits of (seed, stream id, step, slot, element index); the arithmetic
// before the store is the same.  fp32 moments are stored as they are.
template <typename T, typename ST, bool MASTER, bool CLIP = false, typename GT = T, bool GUARD = false, bool SR = false>
__global__ __launch_bounds__(256) void adamw_kernel(const AdamTable t) {
    static_assert(!GUARD || CLIP, "GUARD implies CLIP");
    static_assert(!SR || (std::is_same_v<T, bf16> && !MASTER), "SR rounds bf16 parameters that have no master copy");
    constexpr bool SR_MOMENTS = SR && std::is_same_v<ST, bf16>;
    constexpr int VEC = Vec<T>::N;
    constexpr bool NT = !std::is_same_v<T, float>;
    if constexpr (GUARD) {
        if (*t.skip != 0.f) return;
    }
    // my_chunk(t.chunks), written out: with the call hipcc pairs the moment updates of the CLIP kernels with bf16 parameters and fp32 moments
    // into four fewer packed multiply-adds, and their results change in the last bit
    int ti = 0;
#pragma unroll 1
    while (ti + 1 < t.chunks.count && (int)blockIdx.x >= t.chunks.block_start[ti + 1]) ti++;
    const long long n = t.chunks.n[ti];
    const long long base = (long long)((int)blockIdx.x - t.chunks.block_start[ti]) * kAdamChunk;
    T* p = (T*)t.p[ti];
    const GT* g = (const GT*)t.g[ti];
    ST* m = (ST*)t.m[ti];
    ST* v = (ST*)t.v[ti];
    float* w = t.w[ti];
    float bc1 = t.bc1, bc2_sqrt = t.bc2_sqrt;
    if (t.step_dev) {
        const float step = *t.step_dev;
        bc1 = 1.f - powf(t.beta1, step);
        bc2_sqrt = sqrtf(1.f - powf(t.beta2, step));
    }
    const float lr = t.lr_dev ? *t.lr_dev : t.lr;
    unsigned sr_step = 0, sr_stream = 0;
    if constexpr (SR) {
        sr_step = t.step_dev ? (unsigned)*t.step_dev : t.step;
        sr_stream = t.stream_id[ti] << 2;
    }
    // CLIP folds the coefficient into the one factor every gradient is multiplied by (the unclipped instantiations compile as before).  With
    // a coefficient of 1 the parameters and the fp32 kernel's moments are the unclipped ones bit for bit; the bf16-parameter kernels contract
    // the moments' multiply-adds differently, so those may differ in the last bit
    float clip_scale = 0.f;
    if constexpr (CLIP) clip_scale = t.grad_scale * *t.grad_coef;
    const float step_size = lr / bc1, keep = 1.f - lr * t.decay;
    bool vec = VEC > 1 && n % VEC == 0 && ((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0;
    if (MASTER) vec = vec && (uintptr_t)w % 16 == 0;
    auto ldv = [&](auto* q, long long i, float (&o)[VEC], auto stream) {      // VEC consecutive elements of any storage type as floats
        typedef std::remove_cv_t<std::remove_pointer_t<decltype(q)>> Q;
        constexpr int QN = Vec<Q>::N;
#pragma unroll
        for (int c = 0; c < VEC / QN; c++) {
            float part[QN];
            if constexpr (decltype(stream)::value && NT) Vec<Q>::load_nt(q + i + c * QN, part);
            else Vec<Q>::load(q + i + c * QN, part);
#pragma unroll
            for (int e = 0; e < QN; e++) o[c * QN + e] = part[e];
        }
    };
    auto stv = [&](auto* q, long long i, const float (&o)[VEC], auto stream) {
        typedef std::remove_pointer_t<decltype(q)> Q;
        constexpr int QN = Vec<Q>::N;
#pragma unroll
        for (int c = 0; c < VEC / QN; c++) {
            float part[QN];
#pragma unroll
            for (int e = 0; e < QN; e++) part[e] = o[c * QN + e];
            if constexpr (decltype(stream)::value && NT) Vec<Q>::store_nt(q + i + c * QN, part);
            else Vec<Q>::store(q + i + c * QN, part);
        }
    };
    const long long end = min(n, base + (long long)kAdamChunk);
    auto update = [&](float (&pf)[VEC], const float (&gf)[VEC], float (&mf)[VEC], float (&vf)[VEC]) {
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            float gr;
            if constexpr (CLIP) gr = gf[e] * clip_scale;
            else gr = gf[e] * t.grad_scale;
            pf[e] *= keep;
            mf[e] = t.beta1 * mf[e] + (1.f - t.beta1) * gr;
            vf[e] = t.beta2 * vf[e] + (1.f - t.beta2) * gr * gr;
            pf[e] -= step_size * mf[e] / (sqrtf(vf[e]) / bc2_sqrt + t.eps);
        }
    };
    if (vec) {
        constexpr std::true_type S{};
        constexpr std::false_type K{};
        auto store = [&](long long i, const float (&pf)[VEC], const float (&mf)[VEC], const float (&vf)[VEC]) {
            if constexpr (SR) {                                        // (i is a multiple of 8: one vector of the counter layout)
                unsigned r[4];
                sr_words(t.seed, i >> 3, sr_step, sr_stream, r);
                sr_store8<false>(p + i, pf, r);
                if constexpr (SR_MOMENTS) {
                    sr_words(t.seed, i >> 3, sr_step, sr_stream | 1, r);
                    sr_store8<true>(m + i, mf, r);
                    sr_words(t.seed, i >> 3, sr_step, sr_stream | 2, r);
                    sr_store8<true>(v + i, vf, r);
                } else {
                    stv(m, i, mf, S); stv(v, i, vf, S);
                }
                return;
            }
            stv(p, i, pf, K); stv(m, i, mf, S); stv(v, i, vf, S);      // the updated parameters are what the next forward reads: kept cacheable
            if (MASTER) stv(w, i, pf, S);
        };
        long long i = base + (long long)threadIdx.x * VEC;
        // two pieces per thread and pass: eight 16-byte loads are in flight before the first one is needed (the tensors may alias as far as
        // the compiler knows, so it would not hoist the second piece's loads above the first piece's stores by itself)
        for (; i + 256 * VEC < end; i += 512 * VEC) {
            const long long j = i + 256 * VEC;
            float p0[VEC], g0[VEC], m0[VEC], v0[VEC], p1[VEC], g1[VEC], m1[VEC], v1[VEC];
            if (MASTER) { ldv(w, i, p0, S); ldv(w, j, p1, S); } else { ldv(p, i, p0, K); ldv(p, j, p1, K); }
            ldv(g, i, g0, S); ldv(g, j, g1, S);
            ldv(m, i, m0, S); ldv(m, j, m1, S);
            ldv(v, i, v0, S); ldv(v, j, v1, S);
            update(p0, g0, m0, v0);
            update(p1, g1, m1, v1);
            store(i, p0, m0, v0);
            store(j, p1, m1, v1);
        }
        if (i < end) {
            float pf[VEC], gf[VEC], mf[VEC], vf[VEC];
            if (MASTER) ldv(w, i, pf, S); else ldv(p, i, pf, K);
            ldv(g, i, gf, S); ldv(m, i, mf, S); ldv(v, i, vf, S);
            update(pf, gf, mf, vf);
            store(i, pf, mf, vf);
        }
        return;
    }
    for (long long i = base + (long long)threadIdx.x * VEC; i < end; i += 256 * VEC) {
        float pf[VEC], gf[VEC], mf[VEC], vf[VEC];
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            const bool ok = i + e < n;
            pf[e] = ok ? (MASTER ? w[i + e] : to_f32(p[i + e])) : 0.f; gf[e] = ok ? to_f32(g[i + e]) : 0.f;
            mf[e] = ok ? to_f32(m[i + e]) : 0.f; vf[e] = ok ? to_f32(v[i + e]) : 0.f;
        }
        update(pf, gf, mf, vf);
        if constexpr (SR) {                                            // (i is a multiple of 8 here too: the same words as on the vector path)
            unsigned rp[4], rm[4], rv[4];
            sr_words(t.seed, i >> 3, sr_step, sr_stream, rp);
            if constexpr (SR_MOMENTS) {
                sr_words(t.seed, i >> 3, sr_step, sr_stream | 1, rm);
                sr_words(t.seed, i >> 3, sr_step, sr_stream | 2, rv);
            }
#pragma unroll
            for (int e = 0; e < VEC; e++)
                if (i + e < n) {
                    p[i + e] = sr_bf16_value(pf[e], sr_r16(rp, e));
                    if constexpr (SR_MOMENTS) {
                        m[i + e] = sr_bf16_value(mf[e], sr_r16(rm, e)); v[i + e] = sr_bf16_value(vf[e], sr_r16(rv, e));
                    } else {
                        m[i + e] = from_f32<ST>(mf[e]); v[i + e] = from_f32<ST>(vf[e]);
                    }
                }
            continue;
        }
#pragma unroll
        for (int e = 0; e < VEC; e++)
            if (i + e < n) {
                p[i + e] = from_f32<T>(pf[e]); m[i + e] = from_f32<ST>(mf[e]); v[i + e] = from_f32<ST>(vf[e]);
                if (MASTER) w[i + e] = pf[e];
            }
    }
}

// The one place a storage mode and a variant become an instantiation: (4 storage modes with gradients in the parameter's type + the 3
// bf16-parameter ones with fp32 gradients) x 3 variants = 21 kernels; sr (bf16 parameters without master copies: 2 moment storages x 2
// gradient types) x 3 variants = 12 more.
enum AdamVariant { kAdamPlain, kAdamClip, kAdamGuard };
static void adamw_dispatch(int dtype, bool master, int state_dtype, bool grads32, AdamVariant variant, bool sr, dim3 grid, hipStream_t stream,
                           const AdamTable& t) {
    auto run = [&](auto p, auto s, auto has_master, auto g, auto rounding) {      // the three variants of one (parameter, moment, master, gradient) storage
        typedef decltype(p) T;
        typedef decltype(s) ST;
        typedef decltype(g) GT;
        constexpr bool MASTER = decltype(has_master)::value, SR = decltype(rounding)::value;
        if (variant == kAdamGuard) adamw_kernel<T, ST, MASTER, true, GT, true, SR><<<grid, 256, 0, stream>>>(t);
        else if (variant == kAdamClip) adamw_kernel<T, ST, MASTER, true, GT, false, SR><<<grid, 256, 0, stream>>>(t);
        else adamw_kernel<T, ST, MASTER, false, GT, false, SR><<<grid, 256, 0, stream>>>(t);
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    const float f{};                                              // (values that only carry their types into `run`)
    const bf16 h{};
    if (sr) {
        if (state_dtype == FF_DTYPE_F32) grads32 ? run(h, f, no, f, yes) : run(h, f, no, h, yes);
        else grads32 ? run(h, h, no, f, yes) : run(h, h, no, h, yes);
        return;
    }
    if (dtype == FF_DTYPE_F32) run(f, f, no, f, no);
    else if (master) grads32 ? run(h, f, yes, f, no) : run(h, f, yes, h, no);
    else if (state_dtype == FF_DTYPE_F32) grads32 ? run(h, f, no, f, no) : run(h, f, no, h, no);
    else grads32 ? run(h, h, no, f, no) : run(h, h, no, h, no);
}

// acc_grads: the gradients are fp32 whatever d->dtype is (for fp32 parameters that is what the fp32 kernels read anyway)
// skip: the GUARD kernels (grad_coef is then given too)
static int adamw_launch(const ff_adamw_desc* d, int state_dtype, void* const* params, const void* const* grads, void* const* exp_avg,
                        void* const* exp_avg_sq, float* const* master, const float* lr_dev, const float* grad_coef, const long long* numels,
                        hipStream_t stream, bool acc_grads = false, const float* skip = nullptr, const unsigned* stream_ids = nullptr,
                        unsigned long long seed = 0) {
    FF_CHECK(d && params && grads && exp_avg && exp_avg_sq && numels, FF_ERR_SHAPE, "ff_adamw_step: null argument");
    FF_CHECK(d->dtype == FF_DTYPE_F32 || d->dtype == FF_DTYPE_BF16, FF_ERR_UNSUPPORTED, "ff_adamw_step: dtype %d", d->dtype);
    FF_CHECK(state_dtype == d->dtype || state_dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_adamw_step: moments must be stored in the parameter dtype or in fp32");
    FF_CHECK(!master || d->dtype == FF_DTYPE_BF16, FF_ERR_UNSUPPORTED, "ff_adamw_step: fp32 master copies go with bf16 parameters");
    FF_CHECK(d->n_tensors >= 0 && (d->step >= 1 || d->step_dev), FF_ERR_SHAPE, "ff_adamw_step: n_tensors=%d step=%d", d->n_tensors, d->step);
    AdamTable t;
    t.lr = d->lr; t.beta1 = d->beta1; t.beta2 = d->beta2; t.eps = d->eps; t.decay = d->weight_decay;
    t.step_dev = d->step_dev;
    t.lr_dev = lr_dev;
    t.grad_coef = grad_coef;
    t.skip = skip;
    t.bc1 = 1.f - powf(d->beta1, (float)std::max(d->step, 1));
    t.bc2_sqrt = sqrtf(1.f - powf(d->beta2, (float)std::max(d->step, 1)));
    t.grad_scale = d->grad_scale == 0.f ? 1.f : d->grad_scale;
    t.seed = seed;
    t.step = (unsigned)std::max(d->step, 1);
    const AdamVariant variant = skip ? kAdamGuard : grad_coef ? kAdamClip : kAdamPlain;
    return chunk_launches("ff_adamw_step", t.chunks, d->n_tensors, numels, [&](int cnt, int i) -> int {
        FF_CHECK(params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i] && (!master || master[i]), FF_ERR_SHAPE, "ff_adamw_step: tensor %d has a null pointer", i);
        t.p[cnt] = params[i]; t.g[cnt] = grads[i]; t.m[cnt] = exp_avg[i]; t.v[cnt] = exp_avg_sq[i];
        t.w[cnt] = master ? master[i] : nullptr;
        t.stream_id[cnt] = stream_ids ? stream_ids[i] : 0;
        return FF_OK;
    }, [&](int blocks, long long) -> int {
        if (master) FF_CHECK(state_dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_adamw_step: fp32 master copies go with fp32 moments");
        adamw_dispatch(d->dtype, master != nullptr, state_dtype, acc_grads, variant, stream_ids != nullptr, dim3(blocks), stream, t);
        return check_launch("adamw");
    });
}


// ---- gradient clipping by global L2 norm (torch.nn.utils.clip_grad_norm_, norm_type 2; HF Trainer's max_grad_norm) ----------------------
// Sum of squares over many gradient tensors in the AdamW table's chunks: workgroup b of a launch writes ONE fp32 partial, partials[b]
// (no atomics: fixed slots, so the total is reproducible bit for bit); ff_grad_sumsq_reduce adds the partials up in fp64 in a fixed
// order, ff_grad_clip_coef turns the sum into the norm and the coefficient AdamW (CLIP) or ff_scale_grads applies on the device.
struct GradTable {
    void* g[kAdamTensors];
    ChunkTable chunks;
    float scale;             // sumsq: each gradient is multiplied by it before squaring (grad_scale)
    float* partials;         // sumsq: one slot per workgroup of the launch
    const float* coef;       // scale: device scalar every gradient is multiplied by
};

template <typename T>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const GradTable t) {
    __shared__ float red[4];
    constexpr int VEC = Vec<T>::N, PIECES = 8;      // 8 independent 16-byte loads per thread in flight before the first square
    const auto [ti, n, base, end] = my_chunk(t.chunks);
    const T* g = (const T*)t.g[ti];
    const float scale = t.scale;
    float acc = 0.f;
    long long tail = base;                          // elements from here to `end` are summed one by one
    if ((uintptr_t)g % 16 == 0) {                   // (base is a multiple of the chunk, so every vector below is 16-byte aligned)
        const long long vend = base + (end - base) / VEC * VEC;
        tail = vend;
        long long i = base + (long long)threadIdx.x * VEC;
        for (; i + (PIECES - 1) * 256 * VEC < vend; i += PIECES * 256 * VEC) {
            typename Vec<T>::raw r[PIECES];
#pragma unroll
            for (int k = 0; k < PIECES; k++) r[k] = __builtin_nontemporal_load((const typename Vec<T>::raw*)(g + i + k * 256 * VEC));
#pragma unroll
            for (int k = 0; k < PIECES; k++)
#pragma unroll
                for (int e = 0; e < VEC; e++) {
                    const float x = (float)r[k][e] * scale;
                    acc = fmaf(x, x, acc);
                }
        }
        for (; i < vend; i += 256 * VEC) {          // (a tensor's last, partial chunk)
            float x[VEC];
            Vec<T>::load_nt(g + i, x);
#pragma unroll
            for (int e = 0; e < VEC; e++) {
                const float y = x[e] * scale;
                acc = fmaf(y, y, acc);
            }
        }
    }
    for (long long i = tail + threadIdx.x; i < end; i += 256) {      // ragged tail (< VEC elements), or an unaligned tensor's whole chunk
        const float x = to_f32(g[i]) * scale;
        acc = fmaf(x, x, acc);
    }
    acc = block_sum<4>(acc, red);
    if (threadIdx.x == 0) t.partials[blockIdx.x] = acc;
}

// one workgroup: sum = (accumulate ? *sum : 0) + the partials, in fp64 and in a fixed order (thread k adds slots k, k + 1024, ... in
// index order; the 16 waves combine with a fixed shuffle tree; thread 0 adds the wave sums in wave order)
__global__ __launch_bounds__(1024) void grad_sumsq_reduce_kernel(const float* partials, long long n, double* sum, int accumulate) {
    __shared__ double red[16];
    double s = 0.0;
    long long i = threadIdx.x;
    for (; i + 3 * 1024 < n; i += 4 * 1024) {
        const float a = partials[i], b = partials[i + 1024], c = partials[i + 2048], d = partials[i + 3072];
        s += (double)a; s += (double)b; s += (double)c; s += (double)d;
    }
    for (; i < n; i += 1024) s += (double)partials[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = accumulate ? *sum : 0.0;
        for (int w = 0; w < 16; w++) total += red[w];
        *sum = total;
    }
}

// torch.nn.utils.clip_grad_norm_: norm = ||g||_2 (fp32), coef = clamp(max_norm / (norm + 1e-6), max=1) - a NaN norm gives a NaN coefficient
// and an infinite one 0, as there (no step is skipped)
__global__ void grad_clip_coef_kernel(const double* sum, float max_norm, float* norm, float* coef) {
    if (threadIdx.x != 0) return;
    const float nrm = (float)sqrt(*sum);
    const float c = max_norm / (nrm + 1e-6f);
    if (norm) *norm = nrm;
    if (coef) *coef = c > 1.f ? 1.f : c;
}

// ff_grad_guard: grad_clip_coef_kernel with a verdict - the step is skipped (bad) iff the sum of squares is non-finite, an external check
// found a non-finite gradient (torch.amp.GradScaler's found_inf), or the external loss scale has no finite inverse.  Squares are
// non-negative, so a non-finite gradient always gives a non-finite sum: nothing cancels.  inv = 1 / *ext_scale unscales the gradients
// through the coefficient (they stay scaled in memory).  The intrinsics keep every operation a separately rounded one (no contraction of
// nrm + 1e-6 into a multiply-add), so that without ext_* arguments norm and coef are grad_clip_coef_kernel's bit for bit
__global__ void grad_guard_kernel(const double* sum, float max_norm, const float* ext_found_inf, const float* ext_scale, float* norm,
                                  float* coef, float* skip, float* take, long long* skipped_total) {
    if (threadIdx.x != 0) return;
    const float inv = ext_scale ? __fdiv_rn(1.f, *ext_scale) : 1.f;
    const double s = sum ? *sum : 0.0;
    const float nrm = __fmul_rn((float)sqrt(s), inv);
    const bool bad = !isfinite(s) || (ext_found_inf && *ext_found_inf != 0.f) || !isfinite(inv);
    float c = 1.f;
    if (max_norm > 0.f) {
        c = __fdiv_rn(max_norm, __fadd_rn(nrm, 1e-6f));
        c = c > 1.f ? 1.f : c;
    }
    if (norm) *norm = nrm;
    *coef = bad ? 0.f : __fmul_rn(inv, c);
    *skip = bad ? 1.f : 0.f;
    if (take) *take = bad ? 0.f : 1.f;
    if (skipped_total && bad) *skipped_total += 1;
}

template <typename T>
__global__ __launch_bounds__(256) void grad_scale_kernel(const GradTable t) {
    constexpr int VEC = Vec<T>::N;
    const auto [ti, n, base, end] = my_chunk(t.chunks);
    T* g = (T*)t.g[ti];
    const float c = *t.coef;
    long long tail = base;
    if ((uintptr_t)g % 16 == 0) {                   // vector body; a ragged tail and an unaligned tensor go element by element
        const long long vend = base + (end - base) / VEC * VEC;
        tail = vend;
        for (long long i = base + (long long)threadIdx.x * VEC; i < vend; i += 256 * VEC) {
            float x[VEC];
            Vec<T>::load(g + i, x);
#pragma unroll
            for (int e = 0; e < VEC; e++) x[e] *= c;
            Vec<T>::store(g + i, x);
        }
    }
    for (long long i = tail + threadIdx.x; i < end; i += 256) g[i] = from_f32<T>(to_f32(g[i]) * c);
}

// ---- fp32 gradient accumulation over micro-batches (HF Trainer's gradient_accumulation_steps) ---------------------------------------------
// acc = (OVERWRITE ? 0 : acc) + scale * g in the AdamW table's chunks: g in bf16 or fp32 is read once, the fp32 accumulator is read (unless
// OVERWRITE: the first micro-batch of a step never looks at what the accumulator holds) and written once - all streamed nontemporally,
// four independent 16-byte gradient loads (and their accumulator loads) per thread in flight before the first multiply-add.
// (Open: in isolation, on one 512 M-element tensor, the overwriting fold moves 3.7 TB/s with nontemporal stores and 5.3 TB/s with plain
// ones, the adding fold 5.2 against 5.4 TB/s - not adopted before it is measured inside the step, where plain stores may evict what the
// next kernels read: DESIGN.md, gradient accumulation.)
struct AccTable {
    const void* g[kAdamTensors];
    float* a[kAdamTensors];
    ChunkTable chunks;
    float scale;
};

template <typename T, bool OVERWRITE>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(const AccTable t) {
    constexpr int VEC = Vec<T>::N, PIECES = 4;
    const auto [ti, n, base, end] = my_chunk(t.chunks);
    const T* g = (const T*)t.g[ti];
    float* a = t.a[ti];
    const float s = t.scale;
    auto lda = [&](long long i, float (&o)[VEC]) {                  // VEC accumulator elements: one (fp32 gradients) or two 16-byte loads
#pragma unroll
        for (int c = 0; c < VEC / 4; c++) {
            float part[4];
            Vec<float>::load_nt(a + i + c * 4, part);
#pragma unroll
            for (int e = 0; e < 4; e++) o[c * 4 + e] = part[e];
        }
    };
    auto sta = [&](long long i, const float (&o)[VEC]) {
#pragma unroll
        for (int c = 0; c < VEC / 4; c++) {
            float part[4];
#pragma unroll
            for (int e = 0; e < 4; e++) part[e] = o[c * 4 + e];
            Vec<float>::store_nt(a + i + c * 4, part);
        }
    };
    // the first fold is the rounded product itself (a multiply, so that -0 stays -0); every later one is ONE fused multiply-add
    auto fold = [&](float gf, float af) { return OVERWRITE ? s * gf : fmaf(s, gf, af); };
    long long tail = base;                          // elements from here to `end` go one by one
    if (((uintptr_t)g | (uintptr_t)a) % 16 == 0) {  // (base is a multiple of the chunk, so every vector below is 16-byte aligned)
        const long long vend = base + (end - base) / VEC * VEC;
        tail = vend;
        long long i = base + (long long)threadIdx.x * VEC;
        for (; i + (PIECES - 1) * 256 * VEC < vend; i += PIECES * 256 * VEC) {
            float gf[PIECES][VEC], af[PIECES][VEC];
#pragma unroll
            for (int k = 0; k < PIECES; k++) Vec<T>::load_nt(g + i + k * 256 * VEC, gf[k]);
            if constexpr (!OVERWRITE) {
#pragma unroll
                for (int k = 0; k < PIECES; k++) lda(i + k * 256 * VEC, af[k]);
            }
#pragma unroll
            for (int k = 0; k < PIECES; k++) {
#pragma unroll
                for (int e = 0; e < VEC; e++) af[k][e] = fold(gf[k][e], OVERWRITE ? 0.f : af[k][e]);
                sta(i + k * 256 * VEC, af[k]);
            }
        }
        for (; i < vend; i += 256 * VEC) {          // (a tensor's last, partial chunk)
            float gf[VEC], af[VEC];
            Vec<T>::load_nt(g + i, gf);
            if constexpr (!OVERWRITE) lda(i, af);
#pragma unroll
            for (int e = 0; e < VEC; e++) af[e] = fold(gf[e], OVERWRITE ? 0.f : af[e]);
            sta(i, af);
        }
    }
    for (long long i = tail + threadIdx.x; i < end; i += 256)       // ragged tail (< VEC elements), or an unaligned tensor's whole chunk
        a[i] = fold(to_f32(g[i]), OVERWRITE ? 0.f : a[i]);
}

// ---- exponential moving average of the weights (FusedAdamW(ema_decay=...); include/flamingo_fusion.h has the rule) -------------------------
// ema += a (th - ema) in the AdamW table's chunks, right after the AdamW launch that wrote th: th = the weights in T (the parameters in bf16 or
// fp32, or their fp32 master copies) is read once, the fp32 shadow is read and written once.  All accesses are plain ones: the parameters are
// what the next forward reads and stay cacheable, as in adamw_kernel's store, and for the shadow - touched once per step like the moments -
// nontemporal loads and stores were measured and lost: the pass over config B's 684 M bf16 parameters takes 1.37 ms with plain shadow accesses
// (5.0 TB/s) and 1.60 - 1.64 ms with nontemporal ones (4.2 - 4.3 TB/s); DESIGN.md, weight averaging.  Four independent 16-byte weight loads
// (and their shadow loads: two per weight load for bf16) per thread in flight before the first subtraction.
// Its own kernel and not one more flag of adamw_kernel: fusing would save the 2-byte re-read of the parameter out of 10 bytes per element
// and double the 33 instantiations.  *t.skip and the `every` rule are wave-uniform and decided before any tensor access: a launch that does
// not average is a no-op, as a GUARD launch of adamw_kernel is.
struct EmaTable {
    const void* th[kAdamTensors];
    float* ema[kAdamTensors];
    ChunkTable chunks;
    float decay, step;       // step: the number of the step just taken where it is not read from *step_dev
    int warmup, every;
    const float* step_dev;
    const float* skip;
};

template <typename T>
__global__ __launch_bounds__(256) void ema_update_kernel(const EmaTable t) {
    constexpr int VEC = Vec<T>::N, PIECES = 4;
    const float step = t.step_dev ? *t.step_dev : t.step;
    if (t.skip && *t.skip != 0.f) return;
    if (t.every > 1 && fmodf(step, (float)t.every) != 0.f) return;
    // (the intrinsics keep every operation a separately rounded one, so that `a` is the host restatement's bit for bit)
    const float d = t.warmup ? fminf(t.decay, __fdiv_rn(__fadd_rn(1.f, step), __fadd_rn(10.f, step))) : t.decay;
    const float a = __fsub_rn(1.f, d);
    const auto [ti, n, base, end] = my_chunk(t.chunks);
    const T* th = (const T*)t.th[ti];
    float* ema = t.ema[ti];
    auto lde = [&](long long i, float (&o)[VEC]) {                  // VEC shadow elements: one (fp32 weights) or two 16-byte loads
#pragma unroll
        for (int c = 0; c < VEC / 4; c++) {
            float part[4];
            Vec<float>::load(ema + i + c * 4, part);
#pragma unroll
            for (int e = 0; e < 4; e++) o[c * 4 + e] = part[e];
        }
    };
    auto ste = [&](long long i, const float (&o)[VEC]) {
#pragma unroll
        for (int c = 0; c < VEC / 4; c++) {
            float part[4];
#pragma unroll
            for (int e = 0; e < 4; e++) part[e] = o[c * 4 + e];
            Vec<float>::store(ema + i + c * 4, part);
        }
    };
    auto avg = [&](float w, float s) { return fmaf(a, __fsub_rn(w, s), s); };      // one subtraction, one fused multiply-add
    long long tail = base;                          // elements from here to `end` go one by one
    if (((uintptr_t)th | (uintptr_t)ema) % 16 == 0) {  // (base is a multiple of the chunk, so every vector below is 16-byte aligned)
        const long long vend = base + (end - base) / VEC * VEC;
        tail = vend;
        long long i = base + (long long)threadIdx.x * VEC;
        for (; i + (PIECES - 1) * 256 * VEC < vend; i += PIECES * 256 * VEC) {
            float wf[PIECES][VEC], sf[PIECES][VEC];
#pragma unroll
            for (int k = 0; k < PIECES; k++) Vec<T>::load(th + i + k * 256 * VEC, wf[k]);
#pragma unroll
            for (int k = 0; k < PIECES; k++) lde(i + k * 256 * VEC, sf[k]);
#pragma unroll
            for (int k = 0; k < PIECES; k++) {
#pragma unroll
                for (int e = 0; e < VEC; e++) sf[k][e] = avg(wf[k][e], sf[k][e]);
                ste(i + k * 256 * VEC, sf[k]);
            }
        }
        for (; i < vend; i += 256 * VEC) {          // (a tensor's last, partial chunk)
            float wf[VEC], sf[VEC];
            Vec<T>::load(th + i, wf);
            lde(i, sf);
#pragma unroll
            for (int e = 0; e < VEC; e++) sf[e] = avg(wf[e], sf[e]);
            ste(i, sf);
        }
    }
    for (long long i = tail + threadIdx.x; i < end; i += 256)       // ragged tail (< VEC elements), or an unaligned tensor's whole chunk
        ema[i] = avg(to_f32(th[i]), ema[i]);
}

// ff_stochastic_round_bf16: dst = src rounded stochastically (ff_sr.h), element i with the bits the optimizer gives element i of a tensor:
// 16-byte stores over the whole vectors where src and dst are on the 16-byte grid, the ragged tail - or, off the grid, everything - one by one
__global__ __launch_bounds__(256) void sr_round_kernel(const float* src, bf16* dst, long long n, unsigned long long seed, unsigned step,
                                                       unsigned stream_slot) {
    const long long base = (long long)blockIdx.x * kAdamChunk, end = min(n, base + (long long)kAdamChunk);
    long long tail = base;
    if (((uintptr_t)src | (uintptr_t)dst) % 16 == 0) {             // (base is a multiple of the chunk, so every vector below is 16-byte aligned)
        const long long vend = base + (end - base) / 8 * 8;
        tail = vend;
        for (long long i = base + (long long)threadIdx.x * 8; i < vend; i += 256 * 8) {
            float lo[4], hi[4];
            Vec<float>::load_nt(src + i, lo);
            Vec<float>::load_nt(src + i + 4, hi);
            const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            unsigned r[4];
            sr_words(seed, i >> 3, step, stream_slot, r);
            sr_store8<false>(dst + i, x, r);
        }
    }
    for (long long i = tail + threadIdx.x; i < end; i += 256) {
        unsigned r[4];
        sr_words(seed, i >> 3, step, stream_slot, r);
        dst[i] = sr_bf16_value(src[i], sr_r16(r, (int)(i & 7)));
    }
}

// ff_grad_sumsq / ff_scale_grads: launch(blocks, first slot) on `t`, filled with the next tensors of the call
template <typename F>
static int grad_launches(const char* what, int n_tensors, void* const* grads, const long long* numels, GradTable& t, F&& launch) {
    FF_CHECK(n_tensors >= 0 && (n_tensors == 0 || (grads && numels)), FF_ERR_SHAPE, "%s: null argument", what);
    return chunk_launches(what, t.chunks, n_tensors, numels, [&](int cnt, int i) -> int {
        FF_CHECK(grads[i], FF_ERR_SHAPE, "%s: tensor %d has a null pointer", what, i);
        t.g[cnt] = grads[i];
        return FF_OK;
    }, [&](int blocks, long long slot) -> int {
        launch(blocks, slot);
        return check_launch(what);
    });
}

}  // namespace ff

extern "C" int ff_adamw_step(const ff_adamw_desc* d, void* const* params, const void* const* grads, void* const* exp_avg,
                             void* const* exp_avg_sq, const long long* numels, ff_stream_t stream) {
    return ff::adamw_launch(d, d ? d->dtype : 0, params, grads, exp_avg, exp_avg_sq, nullptr, nullptr, nullptr, numels, (hipStream_t)stream);
}
extern "C" int ff_adamw_step_mixed(const ff_adamw_desc* d, int state_dtype, void* const* params, const void* const* grads, void* const* exp_avg,
                                   void* const* exp_avg_sq, float* const* master, const float* lr_dev, const long long* numels,
                                   ff_stream_t stream) {
    return ff::adamw_launch(d, state_dtype, params, grads, exp_avg, exp_avg_sq, master, lr_dev, nullptr, numels, (hipStream_t)stream);
}

extern "C" int ff_adamw_step_clipped(const ff_adamw_desc* d, int state_dtype, void* const* params, const void* const* grads, void* const* exp_avg,
                                     void* const* exp_avg_sq, float* const* master, const float* lr_dev, const float* grad_coef,
                                     const long long* numels, ff_stream_t stream) {
    FF_CHECK(grad_coef, FF_ERR_SHAPE, "ff_adamw_step_clipped: grad_coef is null");
    return ff::adamw_launch(d, state_dtype, params, grads, exp_avg, exp_avg_sq, master, lr_dev, grad_coef, numels, (hipStream_t)stream);
}
extern "C" int ff_adamw_step_acc(const ff_adamw_desc* d, int state_dtype, void* const* params, const float* const* grads32, void* const* exp_avg,
                                 void* const* exp_avg_sq, float* const* master, const float* lr_dev, const float* grad_coef,
                                 const long long* numels, ff_stream_t stream) {
    return ff::adamw_launch(d, state_dtype, params, (const void* const*)grads32, exp_avg, exp_avg_sq, master, lr_dev, grad_coef, numels,
                            (hipStream_t)stream, true);
}
extern "C" int ff_adamw_step_guarded(const ff_adamw_desc* d, int state_dtype, void* const* params, const void* const* grads, int grads_fp32,
                                     void* const* exp_avg, void* const* exp_avg_sq, float* const* master, const float* lr_dev,
                                     const float* grad_coef, const float* skip, const long long* numels, ff_stream_t stream) {
    FF_CHECK(grad_coef && skip, FF_ERR_SHAPE, "ff_adamw_step_guarded: %s is null", grad_coef ? "skip" : "grad_coef");
    return ff::adamw_launch(d, state_dtype, params, grads, exp_avg, exp_avg_sq, master, lr_dev, grad_coef, numels, (hipStream_t)stream,
                            grads_fp32 != 0, skip);
}
extern "C" int ff_adamw_step_sr(const ff_adamw_desc* d, int state_dtype, void* const* params, const void* const* grads, int grads_fp32,
                                void* const* exp_avg, void* const* exp_avg_sq, const float* lr_dev, const float* grad_coef, const float* skip,
                                long long seed, const unsigned* stream_ids, const long long* numels, ff_stream_t stream) {
    FF_CHECK(d && stream_ids, FF_ERR_SHAPE, "ff_adamw_step_sr: null argument");
    FF_CHECK(d->dtype == FF_DTYPE_BF16, FF_ERR_UNSUPPORTED, "ff_adamw_step_sr: dtype %d (stochastic rounding is for bf16 parameters)", d->dtype);
    FF_CHECK(grad_coef || !skip, FF_ERR_SHAPE, "ff_adamw_step_sr: skip is given without grad_coef");
    for (int i = 0; i < d->n_tensors; i++)
        FF_CHECK(stream_ids[i] < (1u << 30), FF_ERR_SHAPE, "ff_adamw_step_sr: stream id %u of tensor %d is not below 2^30", stream_ids[i], i);
    return ff::adamw_launch(d, state_dtype, params, grads, exp_avg, exp_avg_sq, nullptr, lr_dev, grad_coef, numels, (hipStream_t)stream,
                            grads_fp32 != 0, skip, stream_ids, (unsigned long long)seed);
}
extern "C" int ff_stochastic_round_bf16(const float* src, void* dst, long long n, long long seed, unsigned stream_id, unsigned step, int slot,
                                        ff_stream_t stream) {
    using namespace ff;
    const char* what = "ff_stochastic_round_bf16";
    FF_CHECK(n >= 0 && (n == 0 || (src && dst)), FF_ERR_SHAPE, "%s: null argument", what);
    FF_CHECK(stream_id < (1u << 30) && slot >= 0 && slot <= 3, FF_ERR_SHAPE, "%s: stream_id %u (< 2^30), slot %d (0 .. 3)", what, stream_id, slot);
    if (n == 0) return FF_OK;
    const long long blocks = chunks_of(n);
    FF_CHECK(blocks <= kGradMaxBlocks, FF_ERR_SHAPE, "%s: %lld elements", what, n);
    sr_round_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>(src, (bf16*)dst, n, (unsigned long long)seed, step, stream_id << 2 | (unsigned)slot);
    return check_launch(what);
}
extern "C" int ff_ema_update(int dtype, int n_tensors, const void* const* params, const float* const* master, float* const* ema,
                             const long long* numels, float decay, int warmup, int every, int step, const float* step_dev, const float* skip,
                             ff_stream_t stream) {
    using namespace ff;
    const char* what = "ff_ema_update";
    FF_CHECK(dtype == FF_DTYPE_F32 || dtype == FF_DTYPE_BF16, FF_ERR_UNSUPPORTED, "%s: dtype %d", what, dtype);
    FF_CHECK(decay > 0.f && decay < 1.f, FF_ERR_SHAPE, "%s: decay %g is not in (0, 1)", what, (double)decay);
    FF_CHECK(every >= 1, FF_ERR_SHAPE, "%s: every=%d", what, every);
    FF_CHECK(step >= 1 || step_dev, FF_ERR_SHAPE, "%s: step=%d without step_dev", what, step);
    FF_CHECK(n_tensors >= 0 && (n_tensors == 0 || ((params || master) && ema && numels)), FF_ERR_SHAPE, "%s: null argument", what);
    EmaTable t;
    t.decay = decay; t.step = (float)std::max(step, 1);
    t.warmup = warmup != 0; t.every = every;
    t.step_dev = step_dev; t.skip = skip;
    const bool f32 = master || dtype == FF_DTYPE_F32;            // the weights are read in fp32: master copies, or fp32 parameters
    return chunk_launches(what, t.chunks, n_tensors, numels, [&](int cnt, int i) -> int {
        const void* th = master ? (const void*)master[i] : params[i];
        FF_CHECK(th && ema[i], FF_ERR_SHAPE, "%s: tensor %d has a null pointer", what, i);
        t.th[cnt] = th; t.ema[cnt] = ema[i];
        return FF_OK;
    }, [&](int blocks, long long) -> int {
        if (f32) ema_update_kernel<float><<<blocks, 256, 0, (hipStream_t)stream>>>(t);
        else ema_update_kernel<bf16><<<blocks, 256, 0, (hipStream_t)stream>>>(t);
        return check_launch(what);
    });
}
extern "C" long long ff_grad_sumsq_partials(int n_tensors, const long long* numels) {
    return n_tensors > 0 && numels ? ff::grad_slots(n_tensors, numels) : 0;
}
extern "C" int ff_grad_sumsq(int dtype, int n_tensors, const void* const* grads, const long long* numels, float scale, float* partials,
                             long long n_partials, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(dtype == FF_DTYPE_F32 || dtype == FF_DTYPE_BF16, FF_ERR_UNSUPPORTED, "ff_grad_sumsq: dtype %d", dtype);
    FF_CHECK(n_tensors >= 0 && (n_tensors == 0 || numels), FF_ERR_SHAPE, "ff_grad_sumsq: null argument");
    const long long need = n_tensors > 0 ? grad_slots(n_tensors, numels) : 0;
    FF_CHECK(need <= n_partials && (need == 0 || partials), FF_ERR_WORKSPACE, "ff_grad_sumsq: %lld partials needed, %lld given", need, n_partials);
    GradTable t;
    t.scale = scale;
    t.coef = nullptr;
    return grad_launches("ff_grad_sumsq", n_tensors, (void* const*)grads, numels, t, [&](int blocks, long long slot) {
        t.partials = partials + slot;
        if (dtype == FF_DTYPE_F32) grad_sumsq_kernel<float><<<blocks, 256, 0, (hipStream_t)stream>>>(t);
        else grad_sumsq_kernel<bf16><<<blocks, 256, 0, (hipStream_t)stream>>>(t);
    });
}
extern "C" int ff_grad_sumsq_reduce(const float* partials, long long n_partials, double* sum, int accumulate, ff_stream_t stream) {
    FF_CHECK(sum && n_partials >= 0 && (n_partials == 0 || partials), FF_ERR_SHAPE, "ff_grad_sumsq_reduce: null argument");
    ff::grad_sumsq_reduce_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(partials, n_partials, sum, accumulate);
    return ff::check_launch("ff_grad_sumsq_reduce");
}
extern "C" int ff_grad_clip_coef(const double* sum, float max_norm, float* norm, float* coef, ff_stream_t stream) {
    FF_CHECK(sum && (norm || coef), FF_ERR_SHAPE, "ff_grad_clip_coef: null argument");
    ff::grad_clip_coef_kernel<<<1, 64, 0, (hipStream_t)stream>>>(sum, max_norm, norm, coef);
    return ff::check_launch("ff_grad_clip_coef");
}
extern "C" int ff_grad_guard(const double* sum, float max_norm, const float* ext_found_inf, const float* ext_scale, float* norm, float* coef,
                             float* skip, float* take, long long* skipped_total, ff_stream_t stream) {
    FF_CHECK(coef && skip, FF_ERR_SHAPE, "ff_grad_guard: %s is null", coef ? "skip" : "coef");
    FF_CHECK(sum || ext_found_inf, FF_ERR_SHAPE, "ff_grad_guard: neither a sum nor ext_found_inf is given");
    ff::grad_guard_kernel<<<1, 64, 0, (hipStream_t)stream>>>(sum, max_norm, ext_found_inf, ext_scale, norm, coef, skip, take, skipped_total);
    return ff::check_launch("ff_grad_guard");
}
extern "C" int ff_scale_grads(int dtype, int n_tensors, void* const* grads, const long long* numels, const float* coef, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(dtype == FF_DTYPE_F32 || dtype == FF_DTYPE_BF16, FF_ERR_UNSUPPORTED, "ff_scale_grads: dtype %d", dtype);
    FF_CHECK(coef, FF_ERR_SHAPE, "ff_scale_grads: coef is null");
    GradTable t;
    t.scale = 1.f;
    t.partials = nullptr;
    t.coef = coef;
    return grad_launches("ff_scale_grads", n_tensors, grads, numels, t, [&](int blocks, long long) {
        if (dtype == FF_DTYPE_F32) grad_scale_kernel<float><<<blocks, 256, 0, (hipStream_t)stream>>>(t);
        else grad_scale_kernel<bf16><<<blocks, 256, 0, (hipStream_t)stream>>>(t);
    });
}
extern "C" int ff_grad_accumulate(int dtype, int n_tensors, const void* const* grads, float* const* acc, const long long* numels, float scale,
                                  int overwrite, ff_stream_t stream) {
    using namespace ff;
    const char* what = "ff_grad_accumulate";
    FF_CHECK(dtype == FF_DTYPE_F32 || dtype == FF_DTYPE_BF16, FF_ERR_UNSUPPORTED, "%s: dtype %d", what, dtype);
    FF_CHECK(n_tensors >= 0 && (n_tensors == 0 || (grads && acc && numels)), FF_ERR_SHAPE, "%s: null argument", what);
    AccTable t;
    t.scale = scale;
    return chunk_launches(what, t.chunks, n_tensors, numels, [&](int cnt, int i) -> int {
        FF_CHECK(grads[i] && acc[i], FF_ERR_SHAPE, "%s: tensor %d has a null pointer", what, i);
        t.g[cnt] = grads[i]; t.a[cnt] = acc[i];
        return FF_OK;
    }, [&](int blocks, long long) -> int {
        hipStream_t s = (hipStream_t)stream;
        if (dtype == FF_DTYPE_F32) {
            if (overwrite) grad_accumulate_kernel<float, true><<<blocks, 256, 0, s>>>(t);
            else grad_accumulate_kernel<float, false><<<blocks, 256, 0, s>>>(t);
        } else {
            if (overwrite) grad_accumulate_kernel<bf16, true><<<blocks, 256, 0, s>>>(t);
            else grad_accumulate_kernel<bf16, false><<<blocks, 256, 0, s>>>(t);
        }
        return check_launch(what);
    });
}
