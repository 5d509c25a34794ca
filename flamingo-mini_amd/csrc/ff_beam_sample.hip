// Beam sampling on the captured decode step (ff_beam_sample_step; the rules S1 - S6 are in include/flamingo_fusion.h): ff_beam_step with
// its "2 nb best" replaced by a draw of 2 nb continuations WITHOUT replacement from the softmax over a sequence's nb V accumulated scores a,
// as a Gumbel top-k: the 2 nb largest of p = a + g, g standard Gumbel noise.  The noise is a pure function of (seed, *cur_len, row, column)
// - Philox4x32-7 of ff_sr.h -, so it is never stored: every pass that needs p recomputes it, and no (rows, V) tensor of random numbers exists.
// Two launches, like ff_beam_step:
//   gumbel_rows_kernel   one 256-thread workgroup per row on the row machinery of ff_row_keys.h (keys, the staged key image, kth_largest, the
//                        each / own passes).  lse as beam_rows_kernel forms it; the top-k and nucleus thresholds as sample_token_kernel finds
//                        them; then the row's best 2 nb columns by (p descending, column ascending).  p is not monotone in x, so no bisection
//                        on the stored keys serves.  Instead:
//                          pass 1  every thread walks its own columns and keeps the largest key of p.  tau = the 2 nb-th largest of the 256
//                                  thread maxima: at least 2 nb columns have p >= tau;
//                          pass 2  the columns with a > -inf and p >= tau go into a list of 256 entries in LDS (expected: a small multiple of
//                                  2 nb), and every thread counts its columns with a = -inf;
//                          rank    the list is ranked by counting, (key of p, column) is a total order: the best 2 nb leave;
//                          fill    only when the list is shorter than 2 nb (filtered tokens, a dead beam): the lowest columns with a = -inf,
//                                  found from the threads' counts without noise.
//                        A list that overflows (fewer than 2 nb threads hold nearly all finite columns) takes the exact fallback: the 2 nb-th
//                        largest key of p by bisection, one noise pass per bit, then pass 2 with "above it" and a fill of the lowest columns AT it.
//                        The logits are read once from memory when staged (bf16 rows up to 65536 columns); every pass reads the key image.
//   gumbel_merge_kernel  one wave per sequence: ranks the nb x 2 nb candidates by p, re-ranks the best 2 nb by a (rule S6), and lane 0 walks
//                        them with beam_walk of ff_beam_walk.h, the walk of beam_merge_kernel.
// ff_beam_sample_noise writes g for a (rows, vocab) block: the hook that ties the kernels' noise to its restatement.
// No scratch, no global atomics (the list's slots come from an LDS counter; ranking makes the result independent of the arrival order), fixed
// summation order: equal inputs and an equal seed give equal bits, eager or replayed.
#include <cmath>

#include "ff_beam_walk.h"
#include "ff_row_keys.h"
#include "ff_sr.h"

namespace ff {

constexpr int kGumbelList = 256;              // entries of the LDS list
// LDS header: cnt[256] ints | red[16] words | misc[16] ints | tmax[256] keys | list key / a / column [256] each | out p / a / column [16] each
constexpr int kGumbelScratch = 1024 + 64 + 64 + 1024 + 3 * 4 * kGumbelList + 3 * 64;
static_assert(kGumbelScratch % 16 == 0, "the key image starts 16-byte aligned");
constexpr unsigned kStreamTag = 0x42534D50u;  // counter word 3: "BSMP"
constexpr unsigned kNegInfKey32 = 0x007FFFFFu;  // ordered_key<32>(-inf): a value at or below it is -inf (or a negative NaN)

// rule S4: the standard Gumbel variate of one 32-bit word.  u = ((w >> 9) + 0.5) 2^-23 is exact in fp32 and inside [2^-24, 1 - 2^-24]
FF_DEV float gumbel_of(unsigned w) {
    const float u = ((float)(w >> 9) + 0.5f) * 0x1p-23f;
    return -logf(-logf(u));
}

// The noise of one row, column by column in ascending order: one Philox call serves the four columns 4 q .. 4 q + 3 (counter word 0 = q).
// Plain words, not an array or a reference: the state has to live in registers through the row walks.
struct GumbelRow {
    unsigned w0, w1, w2, w3;
    int q;
};
FF_DEV float gumbel_at(GumbelRow& n, int c, unsigned k0, unsigned k1, unsigned row, unsigned step) {
    if ((c >> 2) != n.q) {
        n.q = c >> 2;
        unsigned w[4];
        philox4x32((unsigned)n.q, row, step, kStreamTag, k0, k1, w);
        n.w0 = w[0]; n.w1 = w[1]; n.w2 = w[2]; n.w3 = w[3];
    }
    const int e = c & 3;
    return gumbel_of(e == 0 ? n.w0 : (e == 1 ? n.w1 : (e == 2 ? n.w2 : n.w3)));  // (selects, not an indexed register array)
}

// cand_p / cand_a / cand_col: [rows][K], this row's best K candidates by (p descending, column ascending), in that order
template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void gumbel_rows_kernel(int V, long long ld, const T* __restrict__ logits, int K, const float* __restrict__ score,
                                                          float temperature, float inv_temperature, int top_k, float top_p,
                                                          const long long* __restrict__ seed, const long long* __restrict__ cur_len,
                                                          float* __restrict__ cand_p, float* __restrict__ cand_a, int* __restrict__ cand_col) {
    constexpr int BITS = sizeof(T) == 2 ? 16 : 32;
    constexpr unsigned kNegInf = sizeof(T) == 2 ? 0x007Fu : 0x007FFFFFu;        // key of a logit -inf: never kept by a warper
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    pin_args(V, ld, logits, K, score, temperature, inv_temperature, top_k, top_p, seed, cur_len, cand_p, cand_a, cand_col);
    int* cnt = (int*)smem_raw;
    float* red = (float*)(smem_raw + 1024);
    int* misc = (int*)(smem_raw + 1088);                                          // [0] list length, [1] tau
    unsigned* tmax = (unsigned*)(smem_raw + 1152);
    unsigned* lkey = (unsigned*)(smem_raw + 2176);
    float* la = (float*)(smem_raw + 2176 + 4 * kGumbelList);
    int* lcol = (int*)(smem_raw + 2176 + 8 * kGumbelList);
    float* op = (float*)(smem_raw + 2176 + 12 * kGumbelList);
    float* oa = op + 16;
    int* oc = (int*)(oa + 16);
    const int tid = threadIdx.x;
    const RowKeys<T, STAGED> keys(logits + (long long)blockIdx.x * ld, V, (unsigned short*)(smem_raw + kGumbelScratch));

    if (tid < kBeamCand) { op[tid] = -INFINITY; oa[tid] = -INFINITY; oc[tid] = tid < V ? tid : 0; }       // what a row of NaN / +inf leaves behind: in range
    if (tid == 0) misc[0] = 0;
    const float xmax = ordered_value<BITS>(keys.stage((unsigned*)red));

    // rule S1: lse = max + log(sum exp(x - max)), formed as beam_rows_kernel forms it (a padding key is no column)
    float s = 0.f;
    if constexpr (STAGED) keys.each([&](unsigned k) __attribute__((always_inline)) { if (k) s += expf(ordered_value<BITS>(k) - xmax); });
    else keys.each([&](unsigned k) __attribute__((always_inline)) { s += expf(ordered_value<BITS>(k) - xmax); });
    s = block_sum<4>(s, red);
    const float lse = xmax + logf(s);
    const float sc = score[blockIdx.x];

    // rule S2: top-k and the nucleus are thresholds on the key, found as sample_token_kernel finds them; with both off every column is kept
    unsigned thr = 0;
    if ((top_k > 0 && top_k < V) || top_p < 1.f) {
        auto weight = [&](unsigned k) __attribute__((always_inline)) { return __expf((ordered_value<BITS>(k) - xmax) * inv_temperature); };
        const unsigned tk = top_k > 0 && top_k < V ? keys.kth_largest(top_k, (int*)red) : 0;
        const unsigned lo = tk > kNegInf + 1 ? tk : kNegInf + 1;
        thr = lo;
        if (top_p < 1.f) {
            auto mass = [&](unsigned t) __attribute__((always_inline)) {
                float m = 0.f;
                keys.each([&](unsigned k) __attribute__((always_inline)) { if (k >= t) m += weight(k); });
                return block_sum<4>(m, red);
            };
            const float Z = mass(lo), want = top_p * Z;
            unsigned t = 0;
            for (int bit = BITS - 1; bit >= 0; bit--) {
                const unsigned cand = t | (1u << bit);
                const float m = cand <= lo ? Z : mass(cand);
                if (m >= want) t = cand;
            }
            thr = t > lo ? t : lo;
        }
    }
    const bool unit_t = temperature == 1.f;
    // rules S2 and S3: a = fl(z + score), z = fl(logp / T) for a kept column and -inf otherwise (T = 1: the bits of ff_beam_step's score)
    auto acc = [&](unsigned k) __attribute__((always_inline)) {
        const float logp = ordered_value<BITS>(k) - lse;
        const float z = k >= thr ? (unit_t ? logp : logp / temperature) : -INFINITY;
        return z + sc;
    };
    auto low = [](float a) __attribute__((always_inline)) { return ordered_key<32>(a) <= kNegInfKey32; };     // a = -inf: p = -inf whatever the noise
    const long long sd = *seed;
    const unsigned k0 = (unsigned)sd, k1 = (unsigned)((unsigned long long)sd >> 32), step = (unsigned)*cur_len, row = blockIdx.x;

    // pass 1: the largest key of p among this thread's columns (own()'s padding calls carry columns >= V: they are no columns)
    unsigned kmax = 0;
    {
        GumbelRow noise = {0u, 0u, 0u, 0u, -1};
        keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
            if (c < keys.c1) {
                const unsigned kp = ordered_key<32>(acc(k) + gumbel_at(noise, c, k0, k1, row, step));
                kmax = kp > kmax ? kp : kmax;
            }
            return false;
        });
    }
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

    // pass 2: the list - a > -inf and p at / above the threshold - and, per thread, the number of fill candidates
    // (strict = false: p >= tau is listed, the fill candidates are the columns with a = -inf;  strict = true, after the bisection: p > tau
    // is listed, the fill candidates are the columns with p exactly at tau)
    auto collect = [&](bool strict) __attribute__((always_inline)) {
        int n_fill = 0;
        GumbelRow noise = {0u, 0u, 0u, 0u, -1};
        keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
            if (c < keys.c1) {
                const float a = acc(k);
                if (low(a)) {
                    n_fill += strict ? 0 : 1;
                } else {
                    const unsigned kp = ordered_key<32>(a + gumbel_at(noise, c, k0, k1, row, step));
                    if (kp > tau || (!strict && kp == tau)) {
                        const int slot = atomicAdd(&misc[0], 1);                   // an LDS counter; the ranking below does not depend on the order
                        if (slot < kGumbelList) { lkey[slot] = kp; la[slot] = a; lcol[slot] = c; }
                    } else if (strict && kp == tau) {
                        n_fill++;
                    }
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
    if (n_list > kGumbelList) {
        // the exact fallback: tau = the K-th largest key of p over the columns with a > -inf (more than 256 of them reach the bound above)
        unsigned t = 0;
        for (int bit = 31; bit >= 0; bit--) {
            const unsigned cand = t | (1u << bit);
            int n = 0;
            GumbelRow noise = {0u, 0u, 0u, 0u, -1};
            keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
                if (c < keys.c1) {
                    const float a = acc(k);
                    if (!low(a)) n += ordered_key<32>(a + gumbel_at(noise, c, k0, k1, row, step)) >= cand ? 1 : 0;
                }
                return false;
            });
            if (block_sum_int(n, (int*)red) >= K) t = cand;
        }
        tau = t;
        fill_at_tau = true;
        __syncthreads();
        if (tid == 0) misc[0] = 0;
        __syncthreads();
        n_list = collect(true);                                                    // fewer than K entries lie above the K-th largest
        n_list = n_list < kGumbelList ? n_list : kGumbelList;
    }

    // rank the list by counting: key of p descending, column ascending
    if (tid < n_list) {
        const unsigned ki = lkey[tid];
        const int ci = lcol[tid];
        int rank = 0;
        for (int j = 0; j < n_list; j++) {
            const unsigned kj = lkey[j];
            const int cj = lcol[j];
            rank += kj > ki || (kj == ki && cj < ci) ? 1 : 0;
        }
        if (rank < K) { op[rank] = ordered_value<32>(ki); oa[rank] = la[tid]; oc[rank] = ci; }
    }
    // fill: the lowest fill columns take the slots behind the list (threads own ascending column ranges: the counts give every thread its first slot)
    if (n_list < K) {
        int slot = n_list;
        for (int t = 0; t < tid; t++) slot += cnt[t];
        if (slot < K && cnt[tid] > 0) {
            if (!fill_at_tau) {
                keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
                    if (c < keys.c1) {
                        const float a = acc(k);
                        if (low(a)) {
                            if (slot < K) { op[slot] = -INFINITY; oa[slot] = a; oc[slot] = c; }
                            slot++;
                        }
                    }
                    return slot >= K;
                });
            } else {
                GumbelRow noise = {0u, 0u, 0u, 0u, -1};
                keys.own([&](int c, unsigned k) __attribute__((always_inline)) {
                    if (c < keys.c1) {
                        const float a = acc(k);
                        if (!low(a)) {
                            const float p = a + gumbel_at(noise, c, k0, k1, row, step);
                            if (ordered_key<32>(p) == tau) {
                                if (slot < K) { op[slot] = p; oa[slot] = a; oc[slot] = c; }
                                slot++;
                            }
                        }
                    }
                    return slot >= K;
                });
            }
        }
    }
    __syncthreads();
    if (tid < K) {
        const int c = oc[tid];
        cand_p[(long long)blockIdx.x * K + tid] = op[tid];
        cand_a[(long long)blockIdx.x * K + tid] = oa[tid];
        cand_col[(long long)blockIdx.x * K + tid] = c < 0 ? 0 : (c >= V ? V - 1 : c);
    }
}

// one wave per sequence: rank the nb K candidates by p (then flat index, slot last), re-rank the best K by a (rule S6), walk
__global__ __launch_bounds__(64) void gumbel_merge_kernel(BeamState st, const float* __restrict__ cand_p, const float* __restrict__ cand_a,
                                                          const int* __restrict__ cand_col) {
    __shared__ unsigned key[FF_BEAM_MAX * kBeamCand];
    __shared__ float av[FF_BEAM_MAX * kBeamCand];
    __shared__ int col[FF_BEAM_MAX * kBeamCand];
    __shared__ unsigned sel_key[kBeamCand];
    __shared__ int sel_beam[kBeamCand], sel_col[kBeamCand];
    __shared__ float top_s[kBeamCand];
    __shared__ int top_beam[kBeamCand], top_col[kBeamCand];
    __shared__ float ns[FF_BEAM_MAX];
    __shared__ int nt[FF_BEAM_MAX], np[FF_BEAM_MAX];
    const int s = blockIdx.x, nb = st.nb, K = 2 * nb, n = nb * K, tid = threadIdx.x;
    const long long r0 = (long long)s * nb;
    for (int j = tid; j < n; j += 64) {
        key[j] = ordered_key<32>(cand_p[r0 * K + j]);
        av[j] = cand_a[r0 * K + j];
        int c = cand_col[r0 * K + j];
        col[j] = c < 0 ? 0 : (c >= st.vocab ? st.vocab - 1 : c);
    }
    __syncthreads();
    for (int i = tid; i < n; i += 64) {                                            // rule S5: p descending, then beam, then column
        const unsigned ki = key[i];
        const int bi = i / K, ci = col[i];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const unsigned kj = key[j];
            const int bj = j / K, cj = col[j];
            const bool better = kj > ki || (kj == ki && (bj < bi || (bj == bi && (cj < ci || (cj == ci && j < i)))));
            rank += better ? 1 : 0;
        }
        if (rank < K) { sel_key[rank] = ordered_key<32>(av[i]); sel_beam[rank] = bi; sel_col[rank] = ci; }
    }
    __syncthreads();
    if (tid < K) {                                                                 // rule S6: a descending, then beam, then column
        const unsigned ki = sel_key[tid];
        const int bi = sel_beam[tid], ci = sel_col[tid];
        int rank = 0;
        for (int j = 0; j < K; j++) {
            const unsigned kj = sel_key[j];
            const int bj = sel_beam[j], cj = sel_col[j];
            const bool better = kj > ki || (kj == ki && (bj < bi || (bj == bi && (cj < ci || (cj == ci && j < tid)))));
            rank += better ? 1 : 0;
        }
        top_s[rank] = ordered_value<32>(ki); top_beam[rank] = bi; top_col[rank] = ci;
    }
    __syncthreads();
    if (tid != 0) return;
    const long long cur = beam_cur_len(st);
    beam_walk(st, s, nb, 0, r0, cur, st.len_norm[cur], top_s, top_beam, top_col, ns, nt, np);
    for (int k = 0; k < nb; k++) beam_store(st, r0, cur, k, ns, nt, np);
}

// g[r][v] of rule S4: one thread per Philox call, four columns
__global__ __launch_bounds__(256) void gumbel_noise_kernel(int vocab, const long long* __restrict__ seed, const long long* __restrict__ cur_len,
                                                           float* __restrict__ g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q > (vocab - 1) >> 2) return;
    const long long sd = *seed;
    unsigned w[4];
    philox4x32((unsigned)q, blockIdx.y, (unsigned)*cur_len, kStreamTag, (unsigned)sd, (unsigned)((unsigned long long)sd >> 32), w);
    float* out = g + (long long)blockIdx.y * vocab;
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (4 * q + e < vocab) out[4 * q + e] = gumbel_of(w[e]);
}

template <typename T, bool STAGED>
static int gumbel_rows_launch(int rows, int V, long long ld, const void* logits, int K, const float* score, float temperature, int top_k, float top_p,
                              const long long* seed, const long long* cur_len, float* cand_p, float* cand_a, int* cand_col, hipStream_t st) {
    if (STAGED) FF_TRY((allow_dynamic_lds<gumbel_rows_kernel<T, STAGED>>(kGumbelScratch + kRowStageMax * 2, "gumbel_rows")));
    gumbel_rows_kernel<T, STAGED><<<dim3(rows), dim3(256), row_keys_lds<STAGED>(kGumbelScratch, V), st>>>(V, ld, (const T*)logits, K, score, temperature,
                                                                                                         1.f / temperature, top_k, top_p, seed, cur_len, cand_p, cand_a, cand_col);
    return check_launch("gumbel_rows");
}

}  // namespace ff

extern "C" size_t ff_beam_sample_workspace_bytes(int b, int nb) {
    if (b <= 0 || nb < 1 || nb > FF_BEAM_MAX) return 0;
    return (size_t)b * nb * 2 * nb * (2 * sizeof(float) + sizeof(int));
}

extern "C" int ff_beam_sample_step(const ff_beam_desc* d, float temperature, int top_k, float top_p, const long long* seed, const void* logits,
                                   const long long* cur_len, void* workspace, size_t workspace_bytes, ff_stream_t stream) {
    using namespace ff;
    FF_TRY(beam_step_check("ff_beam_sample_step", d, logits, cur_len, workspace, workspace_bytes, d ? ff_beam_sample_workspace_bytes(d->b, d->nb) : 0));
    FF_CHECK(seed, FF_ERR_SHAPE, "ff_beam_sample_step: null seed");
    FF_CHECK(temperature > 0.f && std::isfinite(temperature), FF_ERR_SHAPE, "ff_beam_sample_step: temperature %g must be positive and finite", (double)temperature);
    FF_CHECK(top_k >= 0, FF_ERR_SHAPE, "ff_beam_sample_step: top_k %d must be >= 0 (0 = no top-k filter)", top_k);
    FF_CHECK(top_p > 0.f && top_p <= 1.f, FF_ERR_SHAPE, "ff_beam_sample_step: top_p %g must be in (0, 1] (1 = no nucleus filter)", (double)top_p);
    const hipStream_t st = (hipStream_t)stream;
    const int rows = d->b * d->nb, K = 2 * d->nb, V = d->vocab;
    float* cand_p = (float*)workspace;
    float* cand_a = cand_p + (size_t)rows * K;
    int* cand_col = (int*)(cand_a + (size_t)rows * K);
    FF_TRY(row_keys_dispatch(d->dtype, V, [&](auto t, auto staged) {
        return gumbel_rows_launch<decltype(t), decltype(staged)::value>(rows, V, d->ld, logits, K, d->score, temperature, top_k, top_p, seed, cur_len, cand_p, cand_a,
                                                                        cand_col, st);
    }));
    BeamState s = {d->b, d->nb, V, d->max_len, d->eos, d->pad, d->early_stopping, d->score, d->done, d->n_hyp, d->hyp_score, d->hyp_len, d->hyp_row,
                   d->hist_tok, d->hist_parent, d->hist_score, d->next_tok, d->beam_idx, d->len_norm, cur_len};
    gumbel_merge_kernel<<<dim3(d->b), dim3(64), 0, st>>>(s, cand_p, cand_a, cand_col);
    return check_launch("gumbel_merge");
}

extern "C" int ff_beam_sample_noise(int rows, int vocab, const long long* seed, const long long* cur_len, float* g, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(seed && cur_len && g, FF_ERR_SHAPE, "ff_beam_sample_noise: null seed, cur_len or g");
    FF_CHECK(rows > 0 && rows <= 65535 && vocab > 0, FF_ERR_SHAPE, "ff_beam_sample_noise: rows %d (1 .. 65535), vocab %d (> 0)", rows, vocab);
    const int calls = (vocab + 3) / 4;
    gumbel_noise_kernel<<<dim3((calls + 255) / 256, rows), dim3(256), 0, (hipStream_t)stream>>>(vocab, seed, cur_len, g);
    return check_launch("gumbel_noise");
}
