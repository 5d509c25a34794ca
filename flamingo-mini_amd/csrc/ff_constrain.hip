// Constrained decoding in generate(): a candidate trie (what transformers does with a Python callable per row and step,
// PrefixConstrainedLogitsProcessor) and a list of banned words (NoBadWordsLogitsProcessor's vocabulary-wide bias add), applied IN PLACE to the
// rows of logits a decode step is about to select from.  Both rules only ever write -inf, and everything about the constraint - the trie in
// CSR form, the word list, their live sizes - is read from device memory, so one launch inside the captured decode step serves every
// candidate set that fits the capacities it was captured with.  The rules are normative in include/flamingo_fusion.h.
// One 256-thread workgroup per row, nothing kept between steps (the row's position in the trie is re-derived from its generated tokens):
//   B1. one thread per banned word compares the word's head with the tail of the history and stores -inf at the word's last token;
//   T1. wave 0 walks the trie along the generated tokens, 64 tokens per load; a node's sorted children are searched by the whole wave, 64
//       probes per round (one round up to 64 children, two up to 4096, three beyond), found by ballot - no barrier inside the walk, and it
//       ends at the first DONE or DEAD, so it is as long as the candidate, not as the history;
//   T2. the workgroup sets one bit per child token in a vocab-bit bitmap in LDS (OR is order-independent: deterministic), and after a barrier
//       streams the row: a 16-byte group whose bits are all clear is one vector store of -inf, a mixed group is stored element by element, a
//       group whose bits are all set is skipped.  The row is never read: a kept entry keeps its bits because it is not touched.
// B1 and T2 may store to the same entry; both store -inf.  No global atomics, no reduction: equal inputs give equal bits, eager or replayed.
#include "ff_common.h"

namespace ff {

struct constrain_tables {
    const int* node_first;
    const int* edge_tok;
    const int* edge_child;
    const unsigned char* node_terminal;
    const int* n_nodes;
    int node_cap, edge_cap;
    const int* bw_off;
    const int* bw_tok;
    const int* n_bw;
    int bw_cap, bw_tok_cap;
};

enum { CN_DEAD = -1, CN_DONE = -2 };

FF_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The child of node s along token t, searched by one whole wave: edge_tok[lo .. hi) is ascending.  Returns the child node or CN_DEAD; every
// lane returns the same value.  A table entry that points outside the capacities reads nothing: it ends the walk.
FF_DEV int trie_child(const constrain_tables& c, int n_nodes, int s, long long t, int lane) {
    int lo = clampi(c.node_first[s], 0, c.edge_cap), hi = clampi(c.node_first[s + 1], 0, c.edge_cap);
    while (hi - lo > 64) {
        const int step = (hi - lo + 63) >> 6;
        const int p = lo + lane * step;
        const bool le = p < hi && (long long)c.edge_tok[p] <= t;            // ascending: the lanes that hold a token <= t are a prefix
        const int k = __popcll(__ballot(le));
        if (k == 0) return CN_DEAD;
        lo += (k - 1) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    const int p = lo + lane;
    const unsigned long long hit = __ballot(p < hi && (long long)c.edge_tok[p] == t);
    if (hit == 0) return CN_DEAD;
    const int child = c.edge_child[lo + __builtin_ctzll(hit)];
    return child >= 0 && child < n_nodes ? child : CN_DEAD;
}

template <typename T>
__global__ __launch_bounds__(256) void constrain_rows_kernel(int V, long long ld, T* __restrict__ logits, const long long* __restrict__ hist, long long hist_ld,
                                                             int hist_cap, const long long* __restrict__ hist_len, const long long* __restrict__ gen_start, int eos,
                                                             constrain_tables c) {
    extern __shared__ __attribute__((aligned(16))) unsigned int bitmap[];      // words + 2 entries: [words] is read by the 64-bit window of the last group and
                                                                                // never set, [words + 1] carries the row's node from wave 0 to the workgroup
    constexpr int G = 16 / (int)sizeof(T);                                      // elements per 16-byte group
    constexpr unsigned int NINF2 = sizeof(T) == 2 ? 0xFF80FF80u : 0xFF800000u;
    const int tid = threadIdx.x, lane = tid & 63;
    T* x = logits + (long long)blockIdx.x * ld;
    const long long* h = hist + (long long)blockIdx.x * hist_ld;
    const long long len = *hist_len, gs = *gen_start;
    const int n = len < 0 ? 0 : (len > hist_cap ? hist_cap : (int)len);
    const int n0 = gs < 0 ? 0 : (gs > n ? n : (int)gs);
    const T ninf = from_f32<T>(-INFINITY);

    if (c.bw_off != nullptr) {                                                  // B1
        const int n_bw = clampi(*c.n_bw, 0, c.bw_cap);
        for (int w = tid; w < n_bw; w += 256) {
            const int a = clampi(c.bw_off[w], 0, c.bw_tok_cap), b = clampi(c.bw_off[w + 1], 0, c.bw_tok_cap);
            const int m = b - a;
            if (m < 1 || n < m - 1) continue;
            const int last = c.bw_tok[b - 1];
            if (last < 0 || last >= V) continue;
            bool same = true;
            for (int k = 0; k < m - 1 && same; k++) same = h[n - m + 1 + k] == (long long)c.bw_tok[a + k];
            if (same) x[last] = ninf;
        }
    }
    if (c.node_first == nullptr) return;
    const int n_nodes = clampi(*c.n_nodes, 0, c.node_cap);
    if (n_nodes == 0) return;

    const int words = (V + 31) >> 5;
    for (int i = tid; i <= words; i += 256) bitmap[i] = 0u;
    if (tid < 64) {                                                             // T1, wave 0
        int s = 0;
        for (int j0 = n0; j0 < n && s >= 0; j0 += 64) {
            const long long mine = j0 + lane < n ? h[j0 + lane] : 0;
            const int cnt = n - j0 < 64 ? n - j0 : 64;
            for (int k = 0; k < cnt && s >= 0; k++) {
                const long long t = __shfl(mine, k);
                if (t == (long long)eos && c.node_terminal[s] != 0) s = CN_DONE;
                else s = trie_child(c, n_nodes, s, t, lane);
            }
        }
        if (tid == 0) bitmap[words + 1] = (unsigned int)s;
    }
    __syncthreads();
    const int s = (int)bitmap[words + 1];
    if (s < 0) return;                                                          // DONE or DEAD: the trie rule leaves the row untouched
    const int lo = clampi(c.node_first[s], 0, c.edge_cap), hi = clampi(c.node_first[s + 1], 0, c.edge_cap);
    for (int e = lo + tid; e < hi; e += 256) {                                  // T2: the allowed set
        const int t = c.edge_tok[e];
        if (t >= 0 && t < V) atomicOr(&bitmap[t >> 5], 1u << (t & 31));
    }
    if (tid == 0 && c.node_terminal[s] != 0) atomicOr(&bitmap[eos >> 5], 1u << (eos & 31));
    __syncthreads();

    // the row's 16-byte grid: `head` elements in front of it, then whole groups, then the tail
    const int mis = (int)(((unsigned long long)x / sizeof(T)) % G);
    int head = (G - mis) % G;
    head = head < V ? head : V;
    const int n_groups = (V - head) / G;
    const int tail0 = head + n_groups * G;
    if (tid < head && !((bitmap[0] >> tid) & 1u)) x[tid] = ninf;
    if (tid < V - tail0) {
        const int v = tail0 + tid;
        if (!((bitmap[v >> 5] >> (v & 31)) & 1u)) x[v] = ninf;
    }
    const uint4 ninf4 = make_uint4(NINF2, NINF2, NINF2, NINF2);
    for (int k = tid; k < n_groups; k += 256) {
        const int v0 = head + k * G;
        const unsigned long long win = (unsigned long long)bitmap[v0 >> 5] | ((unsigned long long)bitmap[(v0 >> 5) + 1] << 32);
        const unsigned int bits = (unsigned int)(win >> (v0 & 31)) & ((1u << G) - 1u);
        if (bits == 0u) {
            *(uint4*)(x + v0) = ninf4;
        } else if (bits != (1u << G) - 1u) {
#pragma unroll
            for (int j = 0; j < G; j++)
                if (!((bits >> j) & 1u)) x[v0 + j] = ninf;
        }
    }
}

}  // namespace ff

extern "C" int ff_logits_constrain(int dtype, int rows, int vocab, long long ld, void* logits, const long long* hist, long long hist_ld, long long hist_cap,
                                   const long long* hist_len, const long long* gen_start, int eos, const int* node_first, const int* edge_tok,
                                   const int* edge_child, const unsigned char* node_terminal, const int* n_nodes, int node_cap, int edge_cap,
                                   const int* bw_off, const int* bw_tok, const int* n_bw, int bw_cap, int bw_tok_cap, ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(logits && hist && hist_len && gen_start, FF_ERR_SHAPE, "ff_logits_constrain: null logits, hist, hist_len or gen_start");
    FF_CHECK(rows > 0 && vocab > 0 && ld >= vocab, FF_ERR_SHAPE, "ff_logits_constrain: rows %d, vocab %d, ld %lld (need rows > 0, vocab > 0, ld >= vocab)", rows, vocab, ld);
    FF_CHECK(hist_cap >= 1 && hist_ld >= hist_cap, FF_ERR_SHAPE, "ff_logits_constrain: hist_cap %lld, hist_ld %lld (need hist_cap >= 1, hist_ld >= hist_cap)", hist_cap, hist_ld);
    const int trie_given = (node_first != nullptr) + (edge_tok != nullptr) + (edge_child != nullptr) + (node_terminal != nullptr) + (n_nodes != nullptr);
    const int bw_given = (bw_off != nullptr) + (bw_tok != nullptr) + (n_bw != nullptr);
    FF_CHECK(trie_given == 0 || trie_given == 5, FF_ERR_SHAPE, "ff_logits_constrain: the trie is half given (%d of its 5 pointers)", trie_given);
    FF_CHECK(bw_given == 0 || bw_given == 3, FF_ERR_SHAPE, "ff_logits_constrain: the bad-word table is half given (%d of its 3 pointers)", bw_given);
    FF_CHECK(trie_given == 0 || (node_cap >= 1 && edge_cap >= 1), FF_ERR_SHAPE, "ff_logits_constrain: node_cap %d, edge_cap %d (need both >= 1)", node_cap, edge_cap);
    FF_CHECK(bw_given == 0 || (bw_cap >= 1 && bw_tok_cap >= 1), FF_ERR_SHAPE, "ff_logits_constrain: bw_cap %d, bw_tok_cap %d (need both >= 1)", bw_cap, bw_tok_cap);
    FF_CHECK(eos >= (trie_given ? 0 : -1) && eos < vocab, FF_ERR_SHAPE, "ff_logits_constrain: eos %d outside [%d, vocab %d) (a trie needs eos; -1 = none without one)", eos,
             trie_given ? 0 : -1, vocab);
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_logits_constrain: dtype %d", dtype);
    FF_CHECK(hist_cap <= FF_LOGITS_HIST_MAX, FF_ERR_UNSUPPORTED, "ff_logits_constrain: hist_cap %lld exceeds FF_LOGITS_HIST_MAX %d", hist_cap, FF_LOGITS_HIST_MAX);
    FF_CHECK(vocab <= FF_CONSTRAIN_VOCAB_MAX, FF_ERR_UNSUPPORTED, "ff_logits_constrain: vocab %d exceeds FF_CONSTRAIN_VOCAB_MAX %d", vocab, FF_CONSTRAIN_VOCAB_MAX);
    if (trie_given == 0 && bw_given == 0) return FF_OK;                        // no constraint: no launch
    const hipStream_t st = (hipStream_t)stream;
    const constrain_tables c = {node_first, edge_tok, edge_child, node_terminal, n_nodes, node_cap, edge_cap, bw_off, bw_tok, n_bw, bw_cap, bw_tok_cap};
    const size_t lds = trie_given ? ((size_t)((vocab + 31) / 32 + 2) * 4 + 15) / 16 * 16 : 0;      // <= 32 KiB + 16 at the cap
    if (dtype == FF_DTYPE_BF16)
        constrain_rows_kernel<bf16><<<dim3(rows), dim3(256), lds, st>>>(vocab, ld, (bf16*)logits, hist, hist_ld, (int)hist_cap, hist_len, gen_start, eos, c);
    else
        constrain_rows_kernel<float><<<dim3(rows), dim3(256), lds, st>>>(vocab, ld, (float*)logits, hist, hist_ld, (int)hist_cap, hist_len, gen_start, eos, c);
    return check_launch("ff_logits_constrain");
}
