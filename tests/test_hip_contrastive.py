"""Contrastive search on the graph-replayed decode path, on the GPU: ff_topk_logprob (functional.topk_logprobs) and ff_contrastive_step
(functional.contrastive_step) against the numpy float64 restatement of their rules (tests/contrastive_cases.py) on designed inputs, guarded
and poisoned, eager and replayed, and the _ContrastiveSession of FlamingoModel.generate(penalty_alpha=, top_k=, static_decode=True).

SCORE_BOUND, the distance allowed between a score of rule C4 the kernel writes and the float64 value on the same inputs, follows from the
kernel's summation structure for dim <= 4096, with u = 2^-24.  A row of dim elements is spread over the 64 lanes of a wave in 16-byte
vectors, so a lane adds at most dim / 64 = 64 products one after another (fma: one rounding each), then 6 butterfly additions: a dot product
is off by <= 70 u |a| |b| (Cauchy-Schwarz bounds the sum of the |products|), a squared norm by <= 70 u relative, its root by <= 36 u.
cos = dot / (|h_c| * |H_j|): 70 u from the dot product, 36 u from each norm, one rounding each for the product of the norms and the
division: <= 144 u absolute, since |cos| <= 1.  The maximum adds nothing.  score = (1 - alpha) * expf(logp) - alpha * pen, all of
magnitude <= 1: expf <= 2 u, the two products and the two differences one rounding each: <= 6 u.  Total <= 150 u = 8.94e-6 <= SCORE_BOUND
= 1e-5, and the designed margin 1e-3 is 100 x that (>= 20 x).  Measured worst on the designed steps: see the MEASURED line (DESIGN.md
records it).  The log-probabilities of rule T are held to test_hip_beam.SCORE_BOUND, whose derivation covers rules 1 - 2.

The session test decodes test_hip_decode's GPT-2 model on make_inputs(4, 1, TAG) with k = 3: 12 LM rows, 13 decode steps.  Every step of
the eager run is recorded (the inputs and outputs of functional.topk_logprobs and functional.contrastive_step, cloned by a wrapper in this
file) and every (sequence, step) transition is compared with the float64 restatement ON THE RECORDED INPUTS wherever that step is decidable
by MARGIN; at most 5 % of the pairs may be undecidable, the cap of the beam session tests.  TAG and the two values of alpha were fixed
after the float64 twin's dynamic loop (decoding.contrastive_search on the host, these inputs, k = 3) had been run alone: it counted 0 of 52
(sequence, step) pairs with a margin below 1e-3 at alpha 0.6 (smallest margin 2.2e-3) and 0 of 52 at alpha 0.3 (smallest 2.4e-2).
Measured on the device: 0 of 52 at both."""
import contextlib

import numpy as np
import pytest
import torch

import contrastive_cases as CC
from guarded import guarded_allocations
from test_hip_beam import SCORE_BOUND as LOGP_BOUND

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SCORE_BOUND = 1e-5
MARGIN = CC.MARGIN
assert MARGIN >= 20 * SCORE_BOUND
TAG, ALPHA, K = "contrastive", 0.6, 3
DT = {"bf16": BF16, "fp32": F32}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# ---- rule T ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("V", [16, 300, 50258])
def test_topk_logprobs_designed_rows(V, dtype):
    """rows 5, k in (1, 3, 8): tokens exactly, logp within the bound, on rows offset by ld > V and by one element (an unaligned start);
    designed ties across the k-th place, a row with fewer than k finite values; outputs poisoned and guarded"""
    from flamingo_mini_amd import functional as F
    rows, worst = 5, 0.0
    for k in (1, 3, 8):
        x = CC.design_rows(rows, V, k, dtype, seed=V + k)
        tok_ref, lp_ref = CC.topk_logprobs(x, k)
        for ld, off in ((V, 0), (V + 13, 1)):
            buf = torch.full((rows * ld + off + 8,), float("nan"), dtype=DT[dtype], device="cuda")
            view = buf[off:off + rows * ld].view(rows, ld)[:, :V]
            view.copy_(dev(x))
            with guarded_allocations() as g:
                tok, lp = F.topk_logprobs(view, k)
                g.check()
            tok, lp = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64)
            fin = np.isfinite(lp_ref)
            assert np.array_equal(tok[fin], tok_ref[fin]), (V, dtype, k, ld, tok, tok_ref)
            assert ((tok >= 0) & (tok < V)).all()
            assert np.array_equal(np.isfinite(lp), fin) and (lp[~fin] == -np.inf).all()
            worst = max(worst, float(np.abs(lp[fin] - lp_ref[fin]).max()))
    print(f"MEASURED topk_logprobs logp error {worst:.3e} (bound {LOGP_BOUND:.1e}) at V={V} {dtype}")
    assert worst <= LOGP_BOUND


def test_topk_logprobs_rejects_bad_arguments():
    from flamingo_mini_amd import ffi, functional as F
    x = torch.zeros((2, 16), device="cuda")
    for k in (0, 9, True, 2.0):
        with pytest.raises(ValueError):
            F.topk_logprobs(x, k)
    with pytest.raises(ValueError):
        F.topk_logprobs(x[:, :4], 8)
    with pytest.raises(ffi.FusionLibraryError):
        F.topk_logprobs(x.half(), 2)
    tok, lp = torch.zeros((2, 2), dtype=torch.long, device="cuda"), torch.zeros((2, 2), device="cuda")
    assert ffi.lib().ff_topk_logprob(ffi.DTYPE_F32, 2, 1, 16, x.data_ptr(), 2, tok.data_ptr(), lp.data_ptr(), None) == -1      # vocab < k


# ---- rules C2 - C7 on designed steps -----------------------------------------------------------------------------------------------------
def run_step(case, ld_extra=0, score=True):
    """the kernel on a designed case: hist, the outputs and the score buffer are guarded and poisoned.  Returns (outputs, hist before, hist
    after, finished after, score)"""
    from flamingo_mini_amd import functional as F
    dt = DT[case["dtype"]]
    b, k, dim = case["b"], case["k"], case["dim"]
    hid = torch.full((b * k, dim + ld_extra), float("nan"), dtype=dt, device="cuda")
    hidden = hid[:, :dim]
    hidden.copy_(dev(case["hidden"]))
    with guarded_allocations() as g:
        hist = g.new((b, case["max_len"], dim), dt, "cuda")
        hist.copy_(dev(case["hist"]))
        before = hist.clone()
        sc = g.new((b, k), F32, "cuda") if score else None
        fin = dev(case["finished"])
        out = F.contrastive_step(hidden, hist, dev(case["mask"]), dev(case["cand_tok"]), dev(case["cand_logp"]), fin,
                                 torch.tensor([case["alpha"]], dtype=F32, device="cuda"), torch.tensor([case["n"]], device="cuda"),
                                 eos=case["eos"], pad=case["pad"], score=sc)
        g.check()
    return [t.cpu().numpy() for t in out], before, hist, fin.cpu().numpy(), None if sc is None else sc.cpu().numpy()


def check_step(case, got, where):
    (nxt, lp, sel_row, beam_idx), before, after, fin, sc = got
    ref, n, k = case["ref"], case["n"], case["k"]
    assert np.array_equal(sel_row, ref["sel_row"]), (where, sel_row, ref["sel_row"], ref["score"], sc)
    assert np.array_equal(nxt, ref["next_tok"]) and np.array_equal(beam_idx, ref["beam_idx"]) and np.array_equal(fin.astype(bool), ref["finished"]), where
    assert np.array_equal(lp.astype(np.float64), ref["logprob"]), (where, lp, ref["logprob"])       # logp_c* is copied, not computed
    chosen = dev(case["hidden"], DT[case["dtype"]])[dev(ref["sel_row"])]
    assert torch.equal(after[:, n].view(torch.uint8), chosen.view(torch.uint8)), f"{where}: hist[s, n] is not the chosen row bit for bit"
    rest = torch.ones(after.shape[1], dtype=torch.bool, device="cuda")
    rest[n] = False
    assert torch.equal(after[:, rest].view(torch.uint8), before[:, rest].view(torch.uint8)), f"{where}: hist written outside position n"
    finite = np.isfinite(ref["score"])
    assert np.array_equal(np.isfinite(sc), finite) and (sc[~finite] == -np.inf).all(), (where, sc, ref["score"])
    return float(np.abs(sc[finite].astype(np.float64) - ref["score"][finite]).max()) if finite.any() else 0.0


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    import test_hip_decode as TD
    TD._MODELS.clear()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("dim", [64, 100, 768, 4096])
def test_contrastive_step_designed(dim, dtype):
    """b = 3, k in (2, 3, 8), n in (1, 7, 40): a left-padded sequence, a dead candidate, an exact tie of candidates 0 and 1; every integer
    output exactly, hist[s, n] the chosen row bitwise and nothing else of hist written, the score within SCORE_BOUND"""
    worst = 0.0
    for k in (2, 3, 8):
        for n in (1, 7, 40):
            case = CC.design_step(3, k, dim, n, 48, dtype, seed=k * dim + n, left_pad=(1,), dead=(0,), tie=(2,))
            assert CC.decidable(case["ref"]).all()
            worst = max(worst, check_step(case, run_step(case), (k, dim, n, dtype)))
    print(f"MEASURED contrastive_step score error {worst:.3e} (bound {SCORE_BOUND:.1e}) at dim={dim} {dtype}")
    assert worst <= SCORE_BOUND


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_contrastive_step_long_history_and_bookkeeping(dtype):
    """n = 4095 of max_len = 4096 at dim = 64; ld_hidden > dim; an all-dead sequence (c* = 0); finished rows (pad, log-probability 0, the
    state still advances); eos chosen (finished is set); no score buffer"""
    case = CC.design_step(3, 3, 64, 4095, 4096, dtype, seed=11, left_pad=(0,), tie=(1,))
    worst = check_step(case, run_step(case), "n=4095")
    case = CC.design_step(3, 4, 768, 23, 32, dtype, seed=12, all_dead=(1,), finished=(0,), eos_seq=(2,), dead=(0,))
    assert case["ref"]["sel"][1] == 0 and case["ref"]["next_tok"][0] == case["pad"] and case["ref"]["logprob"][0] == 0
    assert case["ref"]["finished"][2] and case["ref"]["next_tok"][2] == case["eos"]
    worst = max(worst, check_step(case, run_step(case, ld_extra=24), "bookkeeping"))
    worst = max(worst, check_step(case, run_step(case, ld_extra=3), "bookkeeping, element-aligned rows"))
    got = run_step(case, score=False)
    assert np.array_equal(got[0][2], case["ref"]["sel_row"])
    print(f"MEASURED contrastive_step score error {worst:.3e} (bound {SCORE_BOUND:.1e}) on the long history and the bookkeeping cases, {dtype}")
    assert worst <= SCORE_BOUND


def test_contrastive_step_rejects_bad_arguments():
    from flamingo_mini_amd import ffi, functional as F
    case = CC.design_step(2, 2, 64, 3, 8, "fp32", seed=5)
    a = dict(hidden=dev(case["hidden"]), hist=dev(case["hist"]), mask=dev(case["mask"]), cand_tok=dev(case["cand_tok"]), cand_logp=dev(case["cand_logp"]),
             finished=dev(case["finished"]), alpha=torch.tensor([0.5], device="cuda"), n_pos=torch.tensor([3], device="cuda"))
    F.contrastive_step(**a)
    for name, bad in (("hidden", a["hidden"][:3]), ("hist", a["hist"].to(BF16)), ("mask", a["mask"][:, :4]), ("cand_logp", a["cand_logp"].double()),
                      ("finished", a["finished"].long()), ("alpha", a["alpha"].double()), ("n_pos", a["n_pos"].int())):
        with pytest.raises(ValueError):
            F.contrastive_step(**dict(a, **{name: bad}))
    with pytest.raises(ffi.FusionLibraryError, match="exceed"):                 # k * dim beyond what the staging holds
        F.contrastive_step(torch.zeros((16, 8192), device="cuda"), torch.zeros((2, 4, 8192), device="cuda"), torch.ones((2, 4), dtype=torch.bool, device="cuda"),
                           torch.zeros((2, 8), dtype=torch.long, device="cuda"), torch.zeros((2, 8), device="cuda"), torch.zeros(2, dtype=torch.bool, device="cuda"),
                           a["alpha"], a["n_pos"])


def test_contrastive_step_replays_with_other_alpha_and_n_pos():
    """captured once with alpha and n_pos as device scalars, replayed with other values: the eager results, bit for bit"""
    from flamingo_mini_amd import functional as F
    b, k, dim, max_len = 3, 4, 768, 48
    cases = {(al, n): CC.design_step(b, k, dim, n, max_len, "bf16", seed=77, alpha=al) for al, n in ((0.6, 9), (0.3, 9), (0.6, 30), (0.9, 17))}
    c0 = cases[(0.6, 9)]
    hidden, mask = dev(c0["hidden"], BF16), dev(c0["mask"])
    tok, lp = dev(c0["cand_tok"]), dev(c0["cand_logp"])
    hist0 = dev(c0["hist"], BF16)
    alpha, n_pos = torch.zeros(1, dtype=F32, device="cuda"), torch.zeros(1, dtype=torch.long, device="cuda")

    def fresh():
        return dict(hist=hist0.clone(), fin=torch.zeros(b, dtype=torch.bool, device="cuda"), sc=torch.zeros((b, k), device="cuda"),
                    out=(torch.zeros(b, dtype=torch.long, device="cuda"), torch.zeros(b, device="cuda"), torch.zeros(b, dtype=torch.long, device="cuda"),
                         torch.zeros(b * k, dtype=torch.long, device="cuda")))

    def call(s):
        F.contrastive_step(hidden, s["hist"], mask, tok, lp, s["fin"], alpha, n_pos, eos=c0["eos"], pad=c0["pad"], out=s["out"], score=s["sc"])

    eager = {}
    for (al, n) in cases:
        alpha.fill_(al); n_pos.fill_(n)
        s = fresh()
        call(s)
        eager[(al, n)] = s
    torch.cuda.synchronize()
    st = fresh()
    alpha.fill_(0.6); n_pos.fill_(9)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(st)
    for (al, n), e in eager.items():
        alpha.fill_(al); n_pos.fill_(n)
        st["hist"].copy_(hist0); st["fin"].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a_, b_ in zip(st["out"] + (st["sc"], st["hist"], st["fin"]), e["out"] + (e["sc"], e["hist"], e["fin"])):
            assert torch.equal(a_.view(torch.uint8), b_.view(torch.uint8)), (al, n)
        # (hidden, mask, candidates are shared: only alpha and n differ between the cases, and the float64 reference agrees where it decides)
        ref = CC.select(c0["hidden"], c0["hist"], c0["mask"], n, c0["cand_tok"], c0["cand_logp"], c0["finished"], al, c0["eos"], c0["pad"])
        ok = CC.decidable(ref)
        assert np.array_equal(st["out"][2].cpu().numpy()[ok], ref["sel_row"][ok])


# ---- the session -------------------------------------------------------------------------------------------------------------------------
class StepLog:
    """Clones what functional.topk_logprobs and functional.contrastive_step read and wrote, call by call (eager runs only)."""

    def __init__(self):
        self.topk, self.steps = [], []

    @contextlib.contextmanager
    def installed(self):
        from flamingo_mini_amd import functional as F
        orig_topk, orig_step = F.topk_logprobs, F.contrastive_step
        log = self

        def topk(logits, k, out=None):
            x = logits.clone()
            res = orig_topk(logits, k, out=out)
            log.topk.append(dict(x=x, tok=res[0].clone(), logp=res[1].clone()))
            return res

        def step(hidden, hist, mask, cand_tok, cand_logp, finished, alpha, n_pos, eos=None, pad=0, out=None, score=None):
            rec = dict(hidden=hidden.clone(), hist=hist.clone(), mask=mask.clone(), cand_tok=cand_tok.clone(), cand_logp=cand_logp.clone(),
                       finished=finished.clone(), alpha=float(alpha), n=int(n_pos), eos=-1 if eos is None else eos, pad=pad)
            res = orig_step(hidden, hist, mask, cand_tok, cand_logp, finished, alpha, n_pos, eos=eos, pad=pad, out=out, score=score)
            rec.update(next_tok=res[0].clone(), logprob=res[1].clone(), sel_row=res[2].clone(), beam_idx=res[3].clone(), hist_after=hist.clone(),
                       finished_after=finished.clone())
            log.steps.append(rec)
            return res

        F.topk_logprobs, F.contrastive_step = topk, step
        try:
            yield self
        finally:
            F.topk_logprobs, F.contrastive_step = orig_topk, orig_step


def check_transitions(log, alpha):
    """every recorded step against the float64 restatement on the recorded inputs.  Returns (undecidable pairs, all pairs)."""
    undecidable = total = 0
    for t in log.topk:
        x = t["x"].float().cpu().numpy()
        tok_ref, lp_ref = CC.topk_logprobs(x, t["tok"].shape[1])
        assert np.array_equal(t["tok"].cpu().numpy(), tok_ref)                   # values are compared as values: exact
        assert np.abs(t["logp"].cpu().numpy() - lp_ref).max() <= LOGP_BOUND
    for r in log.steps:
        assert abs(r["alpha"] - alpha) < 1e-6
        n = r["n"]
        ref = CC.select(r["hidden"].float().cpu().numpy(), r["hist"].float().cpu().numpy(), r["mask"].cpu().numpy(), n, r["cand_tok"].cpu().numpy(),
                        r["cand_logp"].cpu().numpy(), r["finished"].cpu().numpy(), r["alpha"], r["eos"], r["pad"])
        ok = ref["margin"] >= MARGIN
        total += ok.size
        undecidable += int((~ok).sum())
        assert np.array_equal(r["sel_row"].cpu().numpy()[ok], ref["sel_row"][ok]), (n, r["sel_row"], ref["sel_row"], ref["margin"])
        assert np.array_equal(r["next_tok"].cpu().numpy()[ok], ref["next_tok"][ok])
        chosen = r["hidden"][r["sel_row"]]
        assert torch.equal(r["hist_after"][:, n].view(torch.uint8), chosen.contiguous().view(torch.uint8))
        k = r["cand_tok"].shape[1]
        assert torch.equal(r["beam_idx"].view(-1, k), r["sel_row"][:, None].expand(-1, k))
    return undecidable, total


def generate(model, ids, ml, am, vf, graph, alpha=ALPHA, **kw):
    model.decode_graph = graph
    import test_hip_decode as TD
    return model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=TD.MAXLEN, penalty_alpha=alpha, top_k=K,
                          static_decode=True, **kw)


def contrastive_sessions(model):
    """the sessions that capture a graph (decode_graph=False builds one of its own: the flag is part of the key)"""
    from flamingo_mini_amd import decoding as D
    return [s for s in model._decode_sessions.values() if isinstance(s, D._ContrastiveSession) and s.graph_wanted]


def test_session_replays_follows_the_rules_and_reuses_its_graph():
    """(a) a _ContrastiveSession with 12 rows whose graph replays; (b) decode_graph=False gives the same ids; (c) every transition of the
    eager run equals the float64 restatement where decidable, at most 5 % undecidable; (d) penalty_alpha=0.3 reuses the session and the
    graph and follows the rules with 0.3"""
    import test_hip_decode as TD
    model, _ = TD.models("gpt2")
    model.reset_decode_sessions()
    ids, ml, am, vf = TD.make_inputs(4, 1, TAG)
    L0 = ids.shape[1]
    out = generate(model, ids, ml, am, vf, True)
    (sess,) = contrastive_sessions(model)
    assert sess.b == 4 * K == 12 and sess.n_seq == 4 and sess.replay is not None and not sess.capture_failed
    assert out.shape == (4, TD.MAXLEN) and torch.equal(out[:, :L0], ids)
    graph = sess.graph
    log = StepLog()
    with log.installed():
        eager = generate(model, ids, ml, am, vf, False)
    assert torch.equal(out, eager), "the replayed steps and the eager steps chose different tokens"
    assert len(log.steps) == TD.MAXLEN - L0 and len(log.topk) == TD.MAXLEN - L0 + 1
    und, total = check_transitions(log, ALPHA)
    print(f"MEASURED contrastive session: {und} of {total} (sequence, step) pairs undecidable at margin {MARGIN:g}, alpha {ALPHA}")
    assert und <= 0.05 * total
    gen = torch.stack([r["next_tok"] for r in log.steps], 1)
    assert torch.equal(gen, eager[:, L0:])
    # (d)
    out3 = generate(model, ids, ml, am, vf, True, alpha=0.3)
    assert contrastive_sessions(model) == [sess] and sess.graph is graph and float(sess.alpha) == pytest.approx(0.3)
    log3 = StepLog()
    with log3.installed():
        eager3 = generate(model, ids, ml, am, vf, False, alpha=0.3)
    assert torch.equal(out3, eager3)
    und3, total3 = check_transitions(log3, 0.3)
    print(f"MEASURED contrastive session: {und3} of {total3} pairs undecidable at alpha 0.3")
    assert und3 <= 0.05 * total3


def test_session_eos_logprobs_processors_and_bad_words():
    """(e) with eos rows stop and pad, and output_logprobs gives 0 at the pads; (f) with no_repeat_ngram_size=2 and bad_words_ids no banned
    token is ever chosen"""
    import test_hip_decode as TD
    model, _ = TD.models("gpt2")
    ids, ml, am, vf = TD.make_inputs(4, 1, TAG)
    L0 = ids.shape[1]
    base = generate(model, ids, ml, am, vf, True)
    eos = int(base[0, L0 + 3])                                                  # row 0 ends after four tokens, other rows where they reach it
    out = generate(model, ids, ml, am, vf, True, eos_token_id=eos, pad_token_id=0, return_dict_in_generate=True, output_logprobs=True)
    seq, lps = out.sequences, out.token_logprobs
    assert lps.shape == (4, seq.shape[1] - L0) and out.sequences_scores.shape == (4,)
    ended = 0
    for r in range(4):
        g = seq[r, L0:].tolist()
        if eos in g:
            e = g.index(eos)
            ended += 1
            assert g[:e + 1] == base[r, L0:L0 + e + 1].tolist() and all(t == 0 for t in g[e + 1:])
            assert bool((lps[r, e + 1:] == 0).all()) and bool((lps[r, :e + 1] < 0).all())
        else:
            assert g == base[r, L0:L0 + len(g)].tolist()
    assert ended >= 1 and 0 in seq[0, L0:].tolist()
    eager = generate(model, ids, ml, am, vf, False, eos_token_id=eos, pad_token_id=0, return_dict_in_generate=True, output_logprobs=True)
    assert torch.equal(eager.sequences, seq) and torch.equal(eager.token_logprobs, lps)
    # (f)
    bad = sorted({int(t) for t in base[:, L0].tolist()} | {int(base[1, L0 + 2])})
    out = generate(model, ids, ml, am, vf, True, no_repeat_ngram_size=2, bad_words_ids=[[t] for t in bad])
    for r in range(4):
        row = out[r].tolist()
        assert not set(row[L0:]) & set(bad), (r, row, bad)
        grams = list(zip(row, row[1:]))
        first_generated = L0 - 1
        assert all(grams[i] not in grams[:i] for i in range(first_generated, len(grams))), (r, row)
    assert not torch.equal(out, base)
    assert torch.equal(out, generate(model, ids, ml, am, vf, False, no_repeat_ngram_size=2, bad_words_ids=[[t] for t in bad]))


def test_session_opt_replays_what_it_runs_eagerly():
    """(g) an OPT-backed model: position_ids from the attention mask on b * k rows, the same ids replayed and eager"""
    import test_hip_decode as TD
    model, _ = TD.models("opt")
    model.reset_decode_sessions()
    ids, ml, am, vf = TD.make_inputs(4, 1, TAG)
    out = generate(model, ids, ml, am, vf, True)
    (sess,) = contrastive_sessions(model)
    assert sess.replay is not None and not sess.capture_failed
    log = StepLog()
    with log.installed():
        eager = generate(model, ids, ml, am, vf, False)
    assert torch.equal(out, eager)
    und, total = check_transitions(log, ALPHA)
    assert und <= 0.05 * total
