// Contrastive search on the captured decode step (ff_topk_logprob, ff_contrastive_step; the rules T and C1 - C9 are in
// include/flamingo_fusion.h).  Two launches a step, beside the LM and ff_beam_gather:
//   contrastive_topk_kernel   rule T.  One 256-thread workgroup per row on the row machinery of ff_row_keys.h (keys, the staged key image,
//                             kth_largest, the each / own passes).  lse as beam_rows_kernel forms it.  The k largest VALUES are the k largest
//                             keys, so no bisection is needed on the usual row:
//                               pass 1  every thread keeps the largest key of its own columns.  tau = the k-th largest of the 256 thread
//                                       maxima: at least k columns have a key >= tau;
//                               pass 2  the columns with a key >= tau go into a list of 256 entries in LDS (expected: little more than k);
//                               rank    the list is ranked by counting, (key descending, column ascending) is a total order: the best k leave.
//                             A list that overflows - the thread maxima do not bound it: a row of ties, a row with fewer than k finite values
//                             - takes the exact fallback: the k-th largest key by bisection, the (fewer than k) columns above it, then the
//                             lowest columns AT it, found from the threads' counts.
//   contrastive_step_kernel   rules C2 - C7.  One 256-thread workgroup owns one sequence, so no workgroup waits for another.  It stages the
//                             sequence's k candidate vectors in LDS (k * dim elements of the dtype: 128 KiB at k = 8, dim = 4096, fp32), then
//                             streams H[s, :n] ONCE: a wave takes two rows at a time (j, j + 4), requests four 16-byte vectors of them before
//                             it uses the first, and forms from every vector the k dot products of BOTH rows - a candidate vector is read
//                             from LDS once for the two - and the rows' own squared norms.  Per row: the lane's elements in ascending
//                             order, then the xor butterfly; the maxima per wave, then over the waves 0 .. 3.  Thread 0 picks c* and does the
//                             eos bookkeeping; the workgroup copies the chosen vector to H[s, n] from LDS, bit for bit.
//                             Rows whose start or width is not a multiple of 16 bytes take the same kernel with one element per load.
// No scratch, no global atomics (the list's slots come from an LDS counter; ranking makes the result independent of the arrival order), fixed
// summation order: equal inputs give equal bits, eager or replayed.
#include <cmath>

#include "ff_row_keys.h"

namespace ff {

constexpr int kTopkList = 256;                // entries of the LDS list
// LDS header of the row kernel: cnt[256] ints | red[16] words | misc[16] ints | tmax[256] keys | list key / column [256] each | out key / column [8] each
constexpr int kTopkScratch = 1024 + 64 + 64 + 1024 + 2 * 4 * kTopkList + 2 * 32;
static_assert(kTopkScratch % 16 == 0, "the key image starts 16-byte aligned");

// tok / logp: [rows][K], rule T
template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void contrastive_topk_kernel(int V, long long ld, const T* __restrict__ logits, int K, long long* __restrict__ tok,
                                                               float* __restrict__ logp) {
    constexpr int BITS = sizeof(T) == 2 ? 16 : 32;
    constexpr unsigned kNegInf = sizeof(T) == 2 ? 0x007Fu : 0x007FFFFFu;        // key of a logit -inf: at or below it a candidate is DEAD
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    pin_args(V, ld, logits, K, tok, logp);
    int* cnt = (int*)smem_raw;
    float* red = (float*)(smem_raw + 1024);
    int* misc = (int*)(smem_raw + 1088);                                          // [0] list length, [1] tau
    unsigned* tmax = (unsigned*)(smem_raw + 1152);
    unsigned* lkey = (unsigned*)(smem_raw + 2176);
    int* lcol = (int*)(smem_raw + 2176 + 4 * kTopkList);
    unsigned* okey = (unsigned*)(smem_raw + 2176 + 8 * kTopkList);
    int* ocol = (int*)(okey + 8);
    const int tid = threadIdx.x;
    const RowKeys<T, STAGED> keys(logits + (long long)blockIdx.x * ld, V, (unsigned short*)(smem_raw + kTopkScratch));

    if (tid < FF_CONTRASTIVE_K_MAX) { okey[tid] = kNegInf; ocol[tid] = tid < V ? tid : 0; }       // what an unfilled slot leaves behind: dead, in range
    if (tid == 0) misc[0] = 0;
    const float xmax = ordered_value<BITS>(keys.stage((unsigned*)red));

    // lse = max + log(sum exp(x - max)), formed as beam_rows_kernel forms it (rules 1 - 2 of ff_beam_step; a padding key is no column)
    float s = 0.f;
    if constexpr (STAGED) keys.each([&](unsigned k) __attribute__((always_inline)) { if (k) s += expf(ordered_value<BITS>(k) - xmax); });
    else keys.each([&](unsigned k) __attribute__((always_inline)) { s += expf(ordered_value<BITS>(k) - xmax); });
    s = block_sum<4>(s, red);
    const float lse = xmax + logf(s);

    // pass 1: the largest key among this thread's columns (own()'s padding calls have key 0: they raise nothing)
    unsigned kmax = 0;
    keys.own([&](int, unsigned k) __attribute__((always_inline)) {
        kmax = k > kmax ? k : kmax;
        return false;
    });
    tmax[tid] = kmax;
    __syncthreads();
    {
        int rank = 0;
        for (int t = 0; t < 256; t++) {
            const unsigned o = tmax[t];
            rank += o > kmax || (o == kmax && t < tid) ? 1 : 0;
        }
        if (rank == K - 1) misc[1] = (int)kmax;                                    // (the ranks are a permutation: one thread writes)
    }
    __syncthreads();
    unsigned tau = (unsigned)misc[1];

    // pass 2: the list, and per thread the number of fill candidates (strict = false: key >= tau is listed;  strict = true, after the
    // bisection: key > tau is listed, the fill candidates are the columns exactly at tau).  Padding calls carry columns >= c1: no columns.
    auto collect = [&](bool strict) __attribute__((always_inline)) {
        int n_fill = 0;
        keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
            if (c < keys.c1) {
                if (k > tau || (!strict && k == tau)) {
                    const int slot = atomicAdd(&misc[0], 1);                       // an LDS counter; the ranking below does not depend on the order
                    if (slot < kTopkList) { lkey[slot] = k; lcol[slot] = c; }
                } else if (strict && k == tau) {
                    n_fill++;
                }
            }
            return false;
        });
        cnt[tid] = n_fill;
        __syncthreads();
        return misc[0];
    };
    int n_list = collect(false);
    bool fill_at_tau = false;
    if (n_list > kTopkList) {
        // the exact fallback: tau = the K-th largest key (V >= K: it exists); fewer than K columns lie above it
        tau = keys.kth_largest(K, (int*)red);
        fill_at_tau = true;
        __syncthreads();
        if (tid == 0) misc[0] = 0;
        __syncthreads();
        n_list = collect(true);
        n_list = n_list < kTopkList ? n_list : kTopkList;
    }

    // rank the list by counting: key descending, column ascending
    if (tid < n_list) {
        const unsigned ki = lkey[tid];
        const int ci = lcol[tid];
        int rank = 0;
        for (int j = 0; j < n_list; j++) {
            const unsigned kj = lkey[j];
            const int cj = lcol[j];
            rank += kj > ki || (kj == ki && cj < ci) ? 1 : 0;
        }
        if (rank < K) { okey[rank] = ki; ocol[rank] = ci; }
    }
    // fill: the lowest columns at tau take the slots behind the list (threads own ascending column ranges: the counts give every thread its first slot)
    if (fill_at_tau && n_list < K) {
        int slot = n_list;
        for (int t = 0; t < tid; t++) slot += cnt[t];
        if (slot < K && cnt[tid] > 0) {
            keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
                if (c < keys.c1 && k == tau) {
                    if (slot < K) { okey[slot] = k; ocol[slot] = c; }
                    slot++;
                }
                return slot >= K;
            });
        }
    }
    __syncthreads();
    if (tid < K) {
        const int c = ocol[tid];
        const unsigned k = okey[tid];
        tok[(long long)blockIdx.x * K + tid] = c < 0 ? 0 : (c >= V ? V - 1 : c);
        logp[(long long)blockIdx.x * K + tid] = k <= kNegInf ? -INFINITY : ordered_value<BITS>(k) - lse;
    }
}

template <typename T, bool STAGED>
static int contrastive_topk_launch(int rows, int V, long long ld, const void* logits, int K, long long* tok, float* logp, hipStream_t st) {
    if (STAGED) FF_TRY((allow_dynamic_lds<contrastive_topk_kernel<T, STAGED>>(kTopkScratch + kRowStageMax * 2, "contrastive_topk")));
    contrastive_topk_kernel<T, STAGED><<<dim3(rows), dim3(256), row_keys_lds<STAGED>(kTopkScratch, V), st>>>(V, ld, (const T*)logits, K, tok, logp);
    return check_launch("contrastive_topk");
}

// ---- the look-ahead ranking ------------------------------------------------------------------------------------------------------------
constexpr int kStepHeader = 256;              // cn[8] floats | wmax[4][8] floats | sc[8] floats | sel: the candidate image starts behind them
constexpr int kStepStageMax = FF_CONTRASTIVE_K_MAX * 4096 * 4;      // bytes of candidate vectors a workgroup stages (k = 8, dim = 4096, fp32)

struct ContrastiveArgs {
    int b, k, dim, max_len, eos, pad;
    long long ld_hidden;
    const void* hidden;
    void* hist;
    const unsigned char* mask;
    const long long* cand_tok;
    const float* cand_logp;
    unsigned char* finished;
    long long* next_tok;
    float* logprob;
    long long* sel_row;
    long long* beam_idx;
    float* score;
    const float* alpha;
    const long long* n_pos;
};

// N elements of a row per load: a 16-byte vector, or one element for rows that are only element-aligned
template <typename T, bool VEC> struct RowChunk {
    static constexpr int N = Vec<T>::N;
    typedef typename Vec<T>::raw raw;
    static FF_DEV float at(const raw& q, int e) { return (float)q[e]; }
};
template <typename T> struct RowChunk<T, false> {
    static constexpr int N = 1;
    typedef T raw;
    static FF_DEV float at(const raw& q, int) { return to_f32(q); }
};

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void contrastive_step_kernel(ContrastiveArgs a) {
    typedef RowChunk<T, VEC> Ch;
    typedef typename Ch::raw raw;
    constexpr int N = Ch::N, KM = FF_CONTRASTIVE_K_MAX;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* cn = (float*)smem_raw;                                                 // max(|h_c|, 1e-12)
    float* wmax = cn + 8;                                                         // [wave][c]
    float* sc = wmax + 32;
    int* sel = (int*)(sc + 8);
    T* cand = (T*)(smem_raw + kStepHeader);                                       // [k][dim]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, s = blockIdx.x;
    const int k = a.k, dim = a.dim, nchunk = dim / N;                             // (VEC: dim is a multiple of N)
    long long np = *a.n_pos;
    const int n = np < 0 ? 0 : (np > a.max_len ? a.max_len : (int)np);
    const T* hidden = (const T*)a.hidden + (long long)s * k * a.ld_hidden;
    T* hist = (T*)a.hist + (long long)s * a.max_len * dim;
    const unsigned char* mask = a.mask + (long long)s * a.max_len;

    // stage the k candidate vectors
    for (int i = tid; i < k * nchunk; i += 256) {
        const int c = i / nchunk, v = i - c * nchunk;
        *(raw*)(cand + (long long)c * dim + v * N) = *(const raw*)(hidden + (long long)c * a.ld_hidden + v * N);
    }
    __syncthreads();
    for (int c = wave; c < k; c += 4) {                                           // their norms: the lane's elements in order, then the butterfly
        float ss = 0.f;
        for (int v = lane; v < nchunk; v += 64) {
            const raw q = *(const raw*)(cand + (long long)c * dim + v * N);
#pragma unroll
            for (int e = 0; e < N; e++) ss = fmaf(Ch::at(q, e), Ch::at(q, e), ss);
        }
        ss = wave_sum(ss);
        if (lane == 0) cn[c] = fmaxf(sqrtf(ss), 1e-12f);
    }
    __syncthreads();

    // rules C2, C3: stream H[s, :n] once; this wave's rows are wave, wave + 4, ..., two at a time
    float mx[KM];
#pragma unroll
    for (int c = 0; c < KM; c++) mx[c] = -INFINITY;
    for (int j = wave; j < n; j += 8) {
        const int jb = j + 4 < n ? j + 4 : j;                                     // (no second row: the first again, unused)
        const bool live_a = mask[j] != 0, live_b = j + 4 < n && mask[jb] != 0;
        if (!live_a && !live_b) continue;
        const T* ra = hist + (long long)j * dim;
        const T* rb = hist + (long long)jb * dim;
        float da[KM], db[KM], na = 0.f, nb = 0.f;
#pragma unroll
        for (int c = 0; c < KM; c++) { da[c] = 0.f; db[c] = 0.f; }
        for (int v = lane; v < nchunk; v += 128) {
            const int v1 = v + 64 < nchunk ? v + 64 : v;                          // (out of range: the first chunk again, unused)
            raw qa[2], qb[2];
            qa[0] = *(const raw*)(ra + v * N);
            qb[0] = *(const raw*)(rb + v * N);
            qa[1] = *(const raw*)(ra + v1 * N);
            qb[1] = *(const raw*)(rb + v1 * N);
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int vu = v + 64 * u;
                if (vu < nchunk) {
                    float fa[N], fb[N];
#pragma unroll
                    for (int e = 0; e < N; e++) {
                        fa[e] = Ch::at(qa[u], e);
                        fb[e] = Ch::at(qb[u], e);
                        na = fmaf(fa[e], fa[e], na);
                        nb = fmaf(fb[e], fb[e], nb);
                    }
#pragma unroll
                    for (int c = 0; c < KM; c++) {
                        if (c < k) {
                            const raw qc = *(const raw*)(cand + (long long)c * dim + vu * N);
#pragma unroll
                            for (int e = 0; e < N; e++) {
                                const float fc = Ch::at(qc, e);
                                da[c] = fmaf(fa[e], fc, da[c]);
                                db[c] = fmaf(fb[e], fc, db[c]);
                            }
                        }
                    }
                }
            }
        }
        const float ha = fmaxf(sqrtf(wave_sum(na)), 1e-12f), hb = fmaxf(sqrtf(wave_sum(nb)), 1e-12f);
#pragma unroll
        for (int c = 0; c < KM; c++) {
            if (c < k) {
                const float ca = wave_sum(da[c]) / (cn[c] * ha), cb = wave_sum(db[c]) / (cn[c] * hb);
                if (live_a) mx[c] = fmaxf(mx[c], ca);
                if (live_b) mx[c] = fmaxf(mx[c], cb);
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < KM; c++) wmax[wave * 8 + c] = mx[c];
    }
    __syncthreads();

    // rules C3, C4: the score of candidate tid
    if (tid < k) {
        const float m = fmaxf(fmaxf(wmax[tid], wmax[8 + tid]), fmaxf(wmax[16 + tid], wmax[24 + tid]));
        const float pen = m > -INFINITY ? m : 0.f;                                // no live position
        const float lp = a.cand_logp[(long long)s * k + tid], al = *a.alpha;
        const float v = lp > -INFINITY ? (1.f - al) * expf(lp) - al * pen : -INFINITY;       // a dead candidate (a NaN too) never wins
        sc[tid] = v;
        if (a.score) a.score[(long long)s * k + tid] = v;
    }
    __syncthreads();
    // rules C5, C6: the smallest c of maximal score; the eos bookkeeping
    if (tid == 0) {
        int best = 0;
        float bv = -INFINITY;
        for (int c = 0; c < k; c++)
            if (sc[c] > bv) { bv = sc[c]; best = c; }
        *sel = best;
        const long long t = a.cand_tok[(long long)s * k + best];
        const bool fin = a.finished[s] != 0;
        a.next_tok[s] = fin ? (long long)a.pad : t;
        a.logprob[s] = fin ? 0.f : a.cand_logp[(long long)s * k + best];
        if (!fin && a.eos >= 0 && t == (long long)a.eos) a.finished[s] = 1;
        a.sel_row[s] = (long long)s * k + best;
    }
    __syncthreads();
    // rule C7: every row of the sequence follows the chosen one; H[s, n] <- h_c*, bit for bit
    const int best = *sel;
    if (tid < k) a.beam_idx[(long long)s * k + tid] = (long long)s * k + best;
    if (np >= 0 && np < a.max_len) {
        for (int v = tid; v < nchunk; v += 256) *(raw*)(hist + (long long)n * dim + v * N) = *(const raw*)(cand + (long long)best * dim + v * N);
    }
}

template <typename T, bool VEC>
static int contrastive_step_launch(const ContrastiveArgs& a, hipStream_t st) {
    FF_TRY((allow_dynamic_lds<contrastive_step_kernel<T, VEC>>(kStepHeader + kStepStageMax, "contrastive_step")));
    contrastive_step_kernel<T, VEC><<<dim3(a.b), dim3(256), kStepHeader + (size_t)a.k * a.dim * sizeof(T), st>>>(a);
    return check_launch("contrastive_step");
}

}  // namespace ff

extern "C" int ff_topk_logprob(int dtype, int rows, int vocab, long long ld, const void* logits, int k, long long* tok, float* logp, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(logits && tok && logp, FF_ERR_SHAPE, "ff_topk_logprob: null logits, tok or logp");
    FF_CHECK(rows > 0 && vocab > 0 && ld >= vocab, FF_ERR_SHAPE, "ff_topk_logprob: rows %d, vocab %d, ld %lld", rows, vocab, ld);
    FF_CHECK(k >= 1 && k <= FF_CONTRASTIVE_K_MAX, FF_ERR_SHAPE, "ff_topk_logprob: k %d outside [1, %d]", k, FF_CONTRASTIVE_K_MAX);
    FF_CHECK(vocab >= k, FF_ERR_SHAPE, "ff_topk_logprob: vocab %d < k %d", vocab, k);
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_topk_logprob: dtype %d (bf16 and fp32 only)", dtype);
    return row_keys_dispatch(dtype, vocab, [&](auto t, auto staged) {
        return contrastive_topk_launch<decltype(t), decltype(staged)::value>(rows, vocab, ld, logits, k, tok, logp, (hipStream_t)stream);
    });
}

extern "C" int ff_contrastive_step(const ff_contrastive_desc* d, const float* alpha, const long long* n_pos, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(d && alpha && n_pos, FF_ERR_SHAPE, "ff_contrastive_step: null descriptor, alpha or n_pos");
    FF_CHECK(d->hidden && d->hist && d->mask && d->cand_tok && d->cand_logp && d->finished && d->next_tok && d->logprob && d->sel_row && d->beam_idx,
             FF_ERR_SHAPE, "ff_contrastive_step: a null pointer in the descriptor (only score may be null)");
    FF_CHECK(d->b > 0 && d->dim > 0 && d->max_len > 0, FF_ERR_SHAPE, "ff_contrastive_step: b %d, dim %d, max_len %d must be positive", d->b, d->dim, d->max_len);
    FF_CHECK(d->k >= 1 && d->k <= FF_CONTRASTIVE_K_MAX, FF_ERR_SHAPE, "ff_contrastive_step: k %d outside [1, %d]", d->k, FF_CONTRASTIVE_K_MAX);
    FF_CHECK(d->ld_hidden >= d->dim, FF_ERR_SHAPE, "ff_contrastive_step: ld_hidden %lld < dim %d", d->ld_hidden, d->dim);
    FF_CHECK(d->dtype == FF_DTYPE_BF16 || d->dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_contrastive_step: dtype %d (bf16 and fp32 only)", d->dtype);
    const size_t es = dtype_size(d->dtype);
    FF_CHECK((size_t)d->k * d->dim * es <= (size_t)kStepStageMax, FF_ERR_UNSUPPORTED,
             "ff_contrastive_step: k %d x dim %d x %zu bytes exceed the %d bytes of candidate vectors a workgroup stages", d->k, d->dim, es, kStepStageMax);
    const ContrastiveArgs a = {d->b, d->k, d->dim, d->max_len, d->eos, d->pad, d->ld_hidden, d->hidden, d->hist, d->mask, d->cand_tok, d->cand_logp,
                               d->finished, d->next_tok, d->logprob, d->sel_row, d->beam_idx, d->score, alpha, n_pos};
    const int per16 = (int)(16 / es);
    const bool vec = d->dim % per16 == 0 && d->ld_hidden % per16 == 0 && ((unsigned long long)d->hidden & 15u) == 0 && ((unsigned long long)d->hist & 15u) == 0;
    const hipStream_t st = (hipStream_t)stream;
    if (d->dtype == FF_DTYPE_BF16) return vec ? contrastive_step_launch<bf16, true>(a, st) : contrastive_step_launch<bf16, false>(a, st);
    return vec ? contrastive_step_launch<float, true>(a, st) : contrastive_step_launch<float, false>(a, st);
}
