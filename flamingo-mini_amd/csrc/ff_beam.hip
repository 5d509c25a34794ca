// Beam search on the captured decode step: the selection with all of its bookkeeping (ff_beam_step) and the in-place reorder of the static
// LM cache by beam index (ff_beam_gather).  The rules are in include/flamingo_fusion.h; they restate FlamingoModel._beam_search.
// ff_beam_step is two launches:
//   beam_rows_kernel   one 256-thread workgroup per row (= one beam of one sequence) on the row machinery of ff_row_keys.h, which it shares
//                      with sample_token_kernel (keys, the staged key image, the passes and their contracts): lse = max + log(sum exp(x - max));
//                      the 2 nb-th largest value of the row by bisection on the key; then the row's best 2 nb candidates under the rule's order
//                      (score descending, column ascending) are collected: everything whose score  f(x) = (x - lse) + score[row]  is above
//                      f(that value), then the lowest columns with a score equal to it.  f is monotone in x, so this is the row's top 2 nb
//                      by SCORE even where two different logits round to one score.  A sequence's top 2 nb over nb V candidates lies in the
//                      union of its rows' top 2 nb.
//   beam_merge_kernel  one wave per sequence: ranks the nb x 2 nb candidates by counting (keys are integers: a total order whatever the
//                      row held), then lane 0 walks the best 2 nb as the Python loop does (beam_walk of ff_beam_walk.h, which every merge
//                      calls - beam sampling's in ff_beam_sample.hip too) and writes the state block.
// ff_group_beam_step (diverse beam search) is the same row pass and group_merge_kernel in place of beam_merge_kernel.
// Every sum has a fixed order (thread-local in column order, xor butterfly in the wave, wave 0..3): equal inputs give equal bits.
#include <cmath>

#include "ff_beam_walk.h"
#include "ff_row_keys.h"

namespace ff {

constexpr int kBeamScratch = 2304;            // n_gt[256] ints | n_eq[256] ints | red[16] words | cand score[16] | cand column[16]: the key image starts behind them

// cand_score / cand_col: [rows][K], this row's best K candidates in no particular order (the merge ranks them)
template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void beam_rows_kernel(int V, long long ld, const T* __restrict__ logits, int K, const float* __restrict__ score,
                                                        float* __restrict__ cand_score, int* __restrict__ cand_col) {
    constexpr int BITS = sizeof(T) == 2 ? 16 : 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    pin_args(V, ld, logits, K, score, cand_score, cand_col);
    int* n_gt = (int*)smem_raw;
    int* n_eq = (int*)(smem_raw + 1024);
    float* red = (float*)(smem_raw + 2048);
    float* cs = (float*)(smem_raw + 2112);
    int* cc = (int*)(smem_raw + 2176);
    const int tid = threadIdx.x;
    const RowKeys<T, STAGED> keys(logits + (long long)blockIdx.x * ld, V, (unsigned short*)(smem_raw + kBeamScratch));

    if (tid < kBeamCand) { cs[tid] = -INFINITY; cc[tid] = tid < V ? tid : 0; }     // what a row of NaN / +inf leaves behind: in range
    const float xmax = ordered_value<BITS>(keys.stage((unsigned*)red));

    // rule 1: lse = max + log(sum exp(x - max)); a padding key (0 = a NaN of the lowest order) is skipped, it is no column
    float s = 0.f;
    if constexpr (STAGED) keys.each([&](unsigned k) __attribute__((always_inline)) { if (k) s += expf(ordered_value<BITS>(k) - xmax); });
    else keys.each([&](unsigned k) __attribute__((always_inline)) { s += expf(ordered_value<BITS>(k) - xmax); });
    s = block_sum<4>(s, red);
    const float lse = xmax + logf(s);
    const float sc = score[blockIdx.x];
    auto f = [lse, sc](unsigned k) __attribute__((always_inline)) { return (ordered_value<BITS>(k) - lse) + sc; };      // rules 2 and 3: two roundings
    const float fk = f(keys.kth_largest(K, (int*)red));                            // V >= K: the K-th largest value exists

    // rule 4 inside the row: scores above fk (fewer than K: they belong to logits above the K-th largest), then the lowest columns at fk
    // (own()'s padding calls have key 0: f of it is a NaN, neither above nor equal to fk, and they touch nothing)
    int gt = 0, eq = 0;
    keys.own([&](int, unsigned k) __attribute__((always_inline)) {
        const float v = f(k);
        gt += v > fk ? 1 : 0;
        eq += v == fk ? 1 : 0;
        return false;
    });
    n_gt[tid] = gt;
    n_eq[tid] = eq;
    __syncthreads();
    int gt_before = 0, eq_before = 0, gt_all = 0;
    for (int t = 0; t < 256; t++) {
        const int g = n_gt[t], e = n_eq[t];
        if (t < tid) { gt_before += g; eq_before += e; }
        gt_all += g;
    }
    int ig = gt_before, ie = gt_all + eq_before;
    keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
        const float v = f(k);
        const bool g = v > fk, e = v == fk;
        const int slot = g ? ig : ie;
        if ((g || e) && slot < K) { cs[slot] = v; cc[slot] = c; }
        ig += g ? 1 : 0;
        ie += e ? 1 : 0;
        return false;
    });
    __syncthreads();
    if (tid < K) {
        cand_score[(long long)blockIdx.x * K + tid] = cs[tid];
        cand_col[(long long)blockIdx.x * K + tid] = cc[tid];
    }
}

// one wave per sequence: rank the nb K candidates (score descending, beam then column ascending = flat index ascending, slot last), walk
__global__ __launch_bounds__(64) void beam_merge_kernel(BeamState st, const float* __restrict__ cand_score, const int* __restrict__ cand_col) {
    __shared__ unsigned key[FF_BEAM_MAX * kBeamCand];
    __shared__ int col[FF_BEAM_MAX * kBeamCand];
    __shared__ float top_s[kBeamCand];
    __shared__ int top_beam[kBeamCand], top_col[kBeamCand];
    __shared__ float ns[FF_BEAM_MAX];
    __shared__ int nt[FF_BEAM_MAX], np[FF_BEAM_MAX];
    const int s = blockIdx.x, nb = st.nb, K = 2 * nb, n = nb * K, tid = threadIdx.x;
    const long long r0 = (long long)s * nb;
    for (int j = tid; j < n; j += 64) {
        key[j] = ordered_key<32>(cand_score[r0 * K + j]);
        int c = cand_col[r0 * K + j];
        col[j] = c < 0 ? 0 : (c >= st.vocab ? st.vocab - 1 : c);
    }
    __syncthreads();
    for (int i = tid; i < n; i += 64) {
        const unsigned ki = key[i];
        const int bi = i / K, ci = col[i];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const unsigned kj = key[j];
            const int bj = j / K, cj = col[j];
            const bool better = kj > ki || (kj == ki && (bj < bi || (bj == bi && (cj < ci || (cj == ci && j < i)))));
            rank += better ? 1 : 0;
        }
        if (rank < K) { top_s[rank] = ordered_value<32>(ki); top_beam[rank] = bi; top_col[rank] = ci; }
    }
    __syncthreads();
    if (tid != 0) return;

    const long long cur = beam_cur_len(st);
    beam_walk(st, s, nb, 0, r0, cur, st.len_norm[cur], top_s, top_beam, top_col, ns, nt, np);     // the walk all merges share (ff_beam_walk.h)
    for (int k = 0; k < nb; k++) beam_store(st, r0, cur, k, ns, nt, np);
}

// Diverse beam search: one wave per sequence walks the G groups of gs = nb / G rows in order.  A group's penalty lowers at most nb - gs columns
// of a row, so the row's best 2 gs penalised candidates lie among its best 2 gs + (nb - gs) <= 2 nb unpenalised ones: the row pass above (K =
// 2 nb, the same workspace) already delivers them.  Per group: subtract lambda * c (c = live rows of earlier groups that chose the column in
// this step; c = 0 leaves the bits alone), rank the group's gs x K candidates by counting, lane 0 walks the best 2 gs as beam_merge_kernel
// does with nb = gs, and the tokens it chose are what the next group counts.  done / n_hyp are [b][G], hyp_* are read as [b][G][gs].
__global__ __launch_bounds__(64) void group_merge_kernel(BeamState st, int G, float lambda, const float* __restrict__ cand_score,
                                                         const int* __restrict__ cand_col) {
#pragma clang fp contract(off)                                                     // rule A: the product and the difference are rounded separately
    __shared__ float raw[FF_BEAM_MAX * kBeamCand];
    __shared__ int col[FF_BEAM_MAX * kBeamCand];
    __shared__ unsigned key[FF_BEAM_MAX * kBeamCand];
    __shared__ float top_s[kBeamCand];
    __shared__ int top_beam[kBeamCand], top_col[kBeamCand];
    __shared__ float ns[FF_BEAM_MAX];
    __shared__ int nt[FF_BEAM_MAX], np[FF_BEAM_MAX], live[FF_BEAM_MAX];
    const int s = blockIdx.x, nb = st.nb, K = 2 * nb, gs = nb / G, m = gs * K, K2 = 2 * gs, tid = threadIdx.x;
    const long long r0 = (long long)s * nb;
    for (int j = tid; j < nb * K; j += 64) {
        raw[j] = cand_score[r0 * K + j];
        int c = cand_col[r0 * K + j];
        col[j] = c < 0 ? 0 : (c >= st.vocab ? st.vocab - 1 : c);
    }
    const long long cur = beam_cur_len(st);
    const float norm = st.len_norm[cur];
    __syncthreads();
    for (int g = 0; g < G; g++) {
        const int b0 = g * gs, j0 = b0 * K;                                        // the group's first row and first candidate
        for (int i = tid; i < m; i += 64) {
            const int ci = col[j0 + i];
            int c = 0;
            for (int k = 0; k < b0; k++) c += live[k] && nt[k] == ci ? 1 : 0;
            const float v = raw[j0 + i];
            key[i] = ordered_key<32>(c ? v - lambda * (float)c : v);
        }
        __syncthreads();
        for (int i = tid; i < m; i += 64) {
            const unsigned ki = key[i];
            const int bi = i / K, ci = col[j0 + i];
            int rank = 0;
            for (int j = 0; j < m; j++) {
                const unsigned kj = key[j];
                const int bj = j / K, cj = col[j0 + j];
                const bool better = kj > ki || (kj == ki && (bj < bi || (bj == bi && (cj < ci || (cj == ci && j < i)))));
                rank += better ? 1 : 0;
            }
            if (rank < K2) { top_s[rank] = ordered_value<32>(ki); top_beam[rank] = bi; top_col[rank] = ci; }
        }
        __syncthreads();
        if (tid == 0) {
            beam_walk(st, (long long)s * G + g, gs, b0, r0, cur, norm, top_s, top_beam, top_col, ns, nt, np);      // with nb = gs, on the group's rows
            for (int k = 0; k < gs; k++) live[b0 + k] = ns[b0 + k] > -INFINITY ? 1 : 0;      // (a NaN score counts nothing)
        }
        __syncthreads();
    }
    if (tid < nb) beam_store(st, r0, cur, tid, ns, nt, np);
}

template <typename T, bool STAGED>
static int beam_rows_launch(int rows, int V, long long ld, const void* logits, int K, const float* score, float* cand_score, int* cand_col, hipStream_t st) {
    if (STAGED) FF_TRY((allow_dynamic_lds<beam_rows_kernel<T, STAGED>>(kBeamScratch + kRowStageMax * 2, "beam_rows")));
    beam_rows_kernel<T, STAGED><<<dim3(rows), dim3(256), row_keys_lds<STAGED>(kBeamScratch, V), st>>>(V, ld, (const T*)logits, K, score, cand_score, cand_col);
    return check_launch("beam_rows");
}

// ---- in-place gather of cache rows --------------------------------------------------------------------------------------------------
constexpr int kGatherTensors = 48;            // pointers one launch carries in its kernel argument; longer tables are split
struct GatherTable {
    void* t[kGatherTensors];
};
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// Tensors (rows, outer, len_max, inner) seen as units U of 16, 4 or 2 bytes, `units` per (row, o, p).  One thread owns ONE unit offset of a
// sequence in all of its nb rows: it loads the nb units its rows will hold, then stores them, so no thread reads what another writes.
template <typename U, int NB>
__global__ __launch_bounds__(256) void beam_gather_kernel(GatherTable tab, long long outer, long long len_max, long long units,
                                                          const long long* __restrict__ beam_idx, const long long* __restrict__ n_pos) {
    long long np = *n_pos;
    np = np < 0 ? 0 : (np > len_max ? len_max : np);
    const long long span = np * units;                                            // live units of one (row, o)
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= outer * span) return;
    const long long r0 = (long long)blockIdx.y * NB;
    int src[NB];
    bool identity = true;
#pragma unroll
    for (int k = 0; k < NB; k++) {
        const long long g = beam_idx[r0 + k] - r0;
        src[k] = g < 0 || g >= NB ? k : (int)g;                                    // (an index outside the sequence's rows: the row stays)
        identity = identity && src[k] == k;
    }
    if (identity) return;
    const long long o = idx / span;
    const long long row_units = outer * len_max * units;
    U* base = (U*)tab.t[blockIdx.z] + r0 * row_units + o * len_max * units + (idx - o * span);
    U v[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) v[k] = base[src[k] * row_units];
#pragma unroll
    for (int k = 0; k < NB; k++)
        if (src[k] != k) base[k * row_units] = v[k];
}

template <typename U>
static int gather_launches(int n_tensors, void* const* tensors, int b, int nb, long long outer, long long len_max, long long units,
                           const long long* beam_idx, const long long* n_pos, hipStream_t st) {
    const long long blocks = (outer * len_max * units + 255) / 256;
    FF_CHECK(blocks <= 0x7FFFFFFFll && b <= 65535, FF_ERR_SHAPE, "ff_beam_gather: %lld blocks x %d sequences exceed a launch", blocks, b);
    for (int t0 = 0; t0 < n_tensors; t0 += kGatherTensors) {
        const int cnt = n_tensors - t0 < kGatherTensors ? n_tensors - t0 : kGatherTensors;
        GatherTable tab = {};
        for (int i = 0; i < cnt; i++) tab.t[i] = tensors[t0 + i];
        const dim3 grid((unsigned)blocks, b, cnt);
#define FF_GATHER_NB(NB) case NB: beam_gather_kernel<U, NB><<<grid, dim3(256), 0, st>>>(tab, outer, len_max, units, beam_idx, n_pos); break;
        switch (nb) {
            FF_GATHER_NB(1) FF_GATHER_NB(2) FF_GATHER_NB(3) FF_GATHER_NB(4) FF_GATHER_NB(5) FF_GATHER_NB(6) FF_GATHER_NB(7) FF_GATHER_NB(8)
        }
#undef FF_GATHER_NB
        FF_TRY(check_launch("beam_gather"));
    }
    return FF_OK;
}

}  // namespace ff

extern "C" size_t ff_beam_workspace_bytes(int b, int nb) {
    if (b <= 0 || nb < 1 || nb > FF_BEAM_MAX) return 0;
    return (size_t)b * nb * 2 * nb * (sizeof(float) + sizeof(int));
}

// the argument checks every beam step shares, under the caller's name
int ff::beam_step_check(const char* fn, const ff_beam_desc* d, const void* logits, const long long* cur_len, void* workspace, size_t workspace_bytes,
                        size_t workspace_need) {
    FF_CHECK(d && logits && cur_len && workspace, FF_ERR_SHAPE, "%s: null descriptor, logits, cur_len or workspace", fn);
    FF_CHECK(d->score && d->done && d->n_hyp && d->hyp_score && d->hyp_len && d->hyp_row && d->hist_tok && d->hist_parent && d->hist_score &&
                 d->next_tok && d->beam_idx && d->len_norm, FF_ERR_SHAPE, "%s: null state pointer", fn);
    FF_CHECK(d->b > 0 && d->nb >= 1 && d->nb <= FF_BEAM_MAX, FF_ERR_SHAPE, "%s: b %d, nb %d (need b > 0, 1 <= nb <= %d)", fn, d->b, d->nb, FF_BEAM_MAX);
    FF_CHECK(d->vocab >= 2 * d->nb && d->ld >= d->vocab, FF_ERR_SHAPE, "%s: vocab %d, ld %lld (need vocab >= 2 nb = %d, ld >= vocab)", fn, d->vocab, d->ld, 2 * d->nb);
    FF_CHECK(d->max_len >= 1 && (long long)d->b * d->nb <= 0x7FFFFFFF / (2 * FF_BEAM_MAX), FF_ERR_SHAPE, "%s: max_len %d, %d x %d rows", fn, d->max_len, d->b, d->nb);
    FF_CHECK(workspace_bytes >= workspace_need, FF_ERR_SHAPE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, workspace_need);
    FF_CHECK(d->dtype == FF_DTYPE_F32 || d->dtype == FF_DTYPE_BF16, FF_ERR_UNSUPPORTED, "%s: dtype %d", fn, d->dtype);
    return FF_OK;
}

// the row pass and one merge: beam_merge_kernel without groups, group_merge_kernel with them (the same candidates in the same workspace)
static int beam_step_launch(const ff_beam_desc* d, int n_groups, float diversity_penalty, const void* logits, const long long* cur_len, void* workspace,
                            ff_stream_t stream) {
    using namespace ff;
    const hipStream_t st = (hipStream_t)stream;
    const int rows = d->b * d->nb, K = 2 * d->nb, V = d->vocab;
    float* cand_score = (float*)workspace;
    int* cand_col = (int*)(cand_score + (size_t)rows * K);
    FF_TRY(row_keys_dispatch(d->dtype, V, [&](auto t, auto staged) {
        return beam_rows_launch<decltype(t), decltype(staged)::value>(rows, V, d->ld, logits, K, d->score, cand_score, cand_col, st);
    }));
    BeamState s = {d->b, d->nb, V, d->max_len, d->eos, d->pad, d->early_stopping, d->score, d->done, d->n_hyp, d->hyp_score, d->hyp_len, d->hyp_row,
                   d->hist_tok, d->hist_parent, d->hist_score, d->next_tok, d->beam_idx, d->len_norm, cur_len};
    if (n_groups == 1) {
        beam_merge_kernel<<<dim3(d->b), dim3(64), 0, st>>>(s, cand_score, cand_col);
        return check_launch("beam_merge");
    }
    group_merge_kernel<<<dim3(d->b), dim3(64), 0, st>>>(s, n_groups, diversity_penalty, cand_score, cand_col);
    return check_launch("group_merge");
}

extern "C" int ff_beam_step(const ff_beam_desc* d, const void* logits, const long long* cur_len, void* workspace, size_t workspace_bytes,
                            ff_stream_t stream) {
    FF_TRY(ff::beam_step_check("ff_beam_step", d, logits, cur_len, workspace, workspace_bytes, d ? ff_beam_workspace_bytes(d->b, d->nb) : 0));
    return beam_step_launch(d, 1, 0.f, logits, cur_len, workspace, stream);
}

extern "C" int ff_group_beam_step(const ff_beam_desc* d, int n_groups, float diversity_penalty, const void* logits, const long long* cur_len,
                                  void* workspace, size_t workspace_bytes, ff_stream_t stream) {
    FF_TRY(ff::beam_step_check("ff_group_beam_step", d, logits, cur_len, workspace, workspace_bytes, d ? ff_beam_workspace_bytes(d->b, d->nb) : 0));
    FF_CHECK(n_groups >= 1 && d->nb % n_groups == 0, FF_ERR_SHAPE, "ff_group_beam_step: n_groups %d (need n_groups >= 1 and nb %d a multiple of it)", n_groups, d->nb);
    FF_CHECK(diversity_penalty >= 0.f && std::isfinite(diversity_penalty), FF_ERR_SHAPE, "ff_group_beam_step: diversity_penalty %g (need a finite value >= 0)",
             (double)diversity_penalty);
    return beam_step_launch(d, n_groups, diversity_penalty, logits, cur_len, workspace, stream);   // one group IS ff_beam_step: the same two launches
}

extern "C" int ff_beam_gather(int n_tensors, void* const* tensors, int elem_size, int b, int nb, long long outer, long long len_max, long long inner,
                              const long long* beam_idx, const long long* n_pos, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(tensors && beam_idx && n_pos, FF_ERR_SHAPE, "ff_beam_gather: null tensor table, beam_idx or n_pos");
    FF_CHECK(n_tensors > 0 && b > 0 && nb >= 1 && nb <= FF_BEAM_MAX && outer > 0 && len_max > 0 && inner > 0, FF_ERR_SHAPE,
             "ff_beam_gather: n_tensors %d, b %d, nb %d, outer %lld, len_max %lld, inner %lld", n_tensors, b, nb, outer, len_max, inner);
    FF_CHECK(elem_size == 2 || elem_size == 4, FF_ERR_UNSUPPORTED, "ff_beam_gather: element size %d (2 or 4 bytes)", elem_size);
    bool vec = inner * elem_size % 16 == 0;
    for (int i = 0; i < n_tensors; i++) {
        FF_CHECK(tensors[i], FF_ERR_SHAPE, "ff_beam_gather: tensor %d is null", i);
        vec = vec && (uintptr_t)tensors[i] % 16 == 0;
    }
    const hipStream_t st = (hipStream_t)stream;
    if (vec) return gather_launches<u32x4>(n_tensors, tensors, b, nb, outer, len_max, inner * elem_size / 16, beam_idx, n_pos, st);
    if (elem_size == 4) return gather_launches<unsigned>(n_tensors, tensors, b, nb, outer, len_max, inner, beam_idx, n_pos, st);
    return gather_launches<unsigned short>(n_tensors, tensors, b, nb, outer, len_max, inner, beam_idx, n_pos, st);
}
