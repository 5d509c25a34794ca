// The state block of the beam-search steps and the walk over a sequence's ranked candidates (rules 6 of ff_beam_step, B of ff_group_beam_step):
// what beam_merge_kernel, group_merge_kernel (csrc/ff_beam.hip) and gumbel_merge_kernel (csrc/ff_beam_sample.hip) share.  Each merge ranks its
// candidates its own way; ONE lane then calls beam_walk, which is the Python loop of FlamingoModel._beam_search for one sequence (or one group).
#pragma once
#include <cmath>

#include "ff_common.h"

namespace ff {

constexpr int kBeamCand = 2 * FF_BEAM_MAX;    // candidates a row contributes at most

struct BeamState {
    int b, nb, vocab, max_len, eos, pad, early_stopping;
    float* score; int* done; int* n_hyp; float* hyp_score; int* hyp_len; int* hyp_row;
    long long* hist_tok; int* hist_parent; float* hist_score; long long* next_tok; long long* beam_idx;
    const float* len_norm; const long long* cur_len;
};

// *cur_len inside the tables (a length outside them: no write leaves them)
FF_DEV long long beam_cur_len(const BeamState& st) {
    const long long cur = *st.cur_len;
    return cur < 1 ? 1 : (cur > st.max_len ? st.max_len : cur);
}

// One lane.  The 2 nbw ranked candidates top_* (best first; top_beam counts from the first of the nbw rows) of the rows r0 + beam0 .. + nbw - 1
// become the next beams ns / nt / np [beam0 .. beam0 + nbw) (np: the parent, counted from r0) and the hypotheses of those rows; `flag` indexes
// done / n_hyp.  Plain beam search: beam0 = 0, nbw = nb, flag = the sequence.  A group: beam0 = its first row, nbw = gs, flag = s * G + g.
FF_DEV void beam_walk(const BeamState& st, long long flag, int nbw, int beam0, long long r0, long long cur, float norm, const float* top_s,
                      const int* top_beam, const int* top_col, float* ns, int* nt, int* np) {
    float* hs = st.hyp_score + r0 + beam0;
    int* hl = st.hyp_len + r0 + beam0;
    int* hr = st.hyp_row + r0 + beam0;
    for (int k = 0; k < nbw; k++) { ns[beam0 + k] = -INFINITY; nt[beam0 + k] = st.pad; np[beam0 + k] = beam0 + k; }
    if (st.done[flag]) return;
    int nh = st.n_hyp[flag];
    nh = nh < 0 ? 0 : (nh > nbw ? nbw : nh);
    int k = 0;
    for (int rank = 0; rank < 2 * nbw && k < nbw; rank++) {
        const float v = top_s[rank];
        const int beam = top_beam[rank], tok = top_col[rank];
        if (st.eos >= 0 && tok == st.eos) {
            if (rank < nbw) {                                                    // a finished hypothesis: kept sorted, equal scores in arrival order
                const float h = v / norm;
                int p = 0;
                while (p < nh && hs[p] >= h) p++;
                if (p < nbw) {
                    for (int j = nh < nbw - 1 ? nh : nbw - 1; j > p; j--) { hs[j] = hs[j - 1]; hl[j] = hl[j - 1]; hr[j] = hr[j - 1]; }
                    hs[p] = h; hl[p] = (int)cur; hr[p] = (int)r0 + beam0 + beam;
                    nh = nh < nbw ? nh + 1 : nbw;
                }
            }
            continue;
        }
        ns[beam0 + k] = v; nt[beam0 + k] = tok; np[beam0 + k] = beam0 + beam;
        k++;
    }
    st.n_hyp[flag] = nh;
    if (nh >= nbw) {
        float best = ns[beam0];
        for (int j = 1; j < nbw; j++) best = fmaxf(best, ns[beam0 + j]);
        if (st.early_stopping || hs[nbw - 1] >= best / norm) st.done[flag] = 1;
    }
}

// the rows' results and the history row of this step, for beam k of the sequence whose first row is r0
FF_DEV void beam_store(const BeamState& st, long long r0, long long cur, int k, const float* ns, const int* nt, const int* np) {
    const long long h0 = (cur - 1) * (long long)st.b * st.nb + r0;
    st.score[r0 + k] = ns[k];
    st.next_tok[r0 + k] = nt[k];
    st.beam_idx[r0 + k] = r0 + np[k];
    st.hist_tok[h0 + k] = nt[k];
    st.hist_parent[h0 + k] = (int)r0 + np[k];
    st.hist_score[h0 + k] = ns[k];
}

// the argument checks every beam step shares, under the caller's name (workspace_need: what that step's workspace function returns)
int beam_step_check(const char* fn, const ff_beam_desc* d, const void* logits, const long long* cur_len, void* workspace, size_t workspace_bytes,
                    size_t workspace_need);

}  // namespace ff
