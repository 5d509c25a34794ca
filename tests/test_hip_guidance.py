"""Classifier-free guidance on the MI355X: ff_guided_logits / functional.guided_logits (csrc/ff_guidance.hip) and the decode sessions built
with guidance.

The kernel: every designed row pair of tests/guidance_cases.py in both dtypes, inside the sentinel arenas of tests/test_hip_loss_bounds.py -
cond, uncond and out each with a row stride and a start phase of its own; the inputs and their surroundings keep their bits, the
surroundings of out and the gaps between its rows keep theirs - against float64 from the stored values under
    |out - out*| <= |1 - g| B(lu) + g B(lc) + 4 2^-24 (g |lc* - lu*| + |lu*| + |out*|),   B = CE_C_F 2^-24 (|lse*| + |x| + 1)
(guidance_cases.bound: the kernel evaluates out = fmaf(g, lc - lu, lu), whose two roundings the last term covers; the float32 restatement
stays inside it on the CPU, tests/test_guidance_cases.py); the edge rules G3; g = 1 and g = 0 against the log-softmax of one input, their
lse against ff_token_logprob's; graph replay with the scale rewritten on the device.

The sessions (G1 geometry of tests/test_hip_decode.py; batch 4 = 8 LM rows on the decode feed-forward kernels, batch 17 = 34 rows beyond
the 32-row switch): the raw 2 R-row logits and the guided buffer of every step are recorded inside the session (device copies, so they
are captured and run under replay); the guided buffer lies within the kernel bound of float64 from THOSE logits and the greedy token is
its argmax; eager and replayed steps give the same bits; g = 0 is the ordinary static decode without media; static and dynamic guided
decoding agree for greedy and beam search wherever the float64 guided scores decide by more than the margin; sampling; session reuse.

The margin of the static-against-dynamic comparison.  A path chooses entry j over the float64 winner t only if its own difference
score[t] - score[j] has the wrong sign, i.e. if the float64 gap between the two is smaller than the path's error of that DIFFERENCE (what
the two entries share - the error of lse, a common offset of the bf16 logits - cancels in it).  Against the float64 teacher-forced guided
scores, the differences of either path from the winner to the TOP_K highest float64 entries are off by at most TOL_GUIDED_GAP, and single
entries anywhere in the row by at most TOL_GUIDED_ROW (both measured on an MI355X, see the constants).  A decision is compared where the
float64 top-two gap is at least MARGIN = TOL_GUIDED_GAP and entry TOP_K + 1 lies at least 2 TOL_GUIDED_ROW below the first: there neither
path can choose another token."""
import contextlib

import pytest
import torch

import guidance_cases as GC
import logprob_cases as LP
import loss_cases as lc
from util import CE_C_F

pytestmark = pytest.mark.gpu
BF16, F32 = GC.BF16, GC.F32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])

# errors of a step's guided scores (g = 1.5, bf16 model) against the float64 teacher-forced guided scores, measured on an MI355X (the
# MEASURED guided-f64-* lines of this file; FF_TOL_REPORT=<file>, tools/tol_report.py) and set with the project's 1.3 - 2 x margin:
#   TOL_GUIDED_ROW  max-abs of an entry anywhere in the row: the session's guided buffer 1.31e-1 (batch 4), 1.48e-1 (batch 17); the
#                   dynamic form (two uncached bf16 forwards, guided_logits_torch) 1.39e-1, 1.51e-1
#   TOL_GUIDED_GAP  max-abs of (winner - entry j) over the TOP_K float64 entries: the session's guided buffer 1.34e-1 (batch 4), 1.38e-1
#                   (batch 17); the dynamic form 1.25e-1, 1.36e-1
TOP_K = 8
TOL_GUIDED_ROW = 0.2
TOL_GUIDED_GAP = 0.2
MARGIN = TOL_GUIDED_GAP


def scale_tensor(g):
    return torch.tensor([g], dtype=torch.float32, device="cuda")


def run_case(case, g):
    """functional.guided_logits on the case's rows inside arenas; returns out (rows, V) on the CPU after checking that nothing but
    out[r, 0:V] was written"""
    from flamingo_mini_amd import functional as F
    from test_hip_loss_bounds import Arena
    c, u = case["cond"], case["uncond"]
    rows, V = c.shape
    dtype = c.dtype

    def place(x, ld, off):
        a = Arena((rows * ld,), dtype, off)
        view = a.body.view(rows, 2, V)[:, -1] if ld == 2 * V else a.body.view(rows, ld)[:, :V]
        view.copy_(x)
        assert [(view[r].data_ptr() % 16) for r in range(rows)] == LP.row_starts(rows, ld, dtype, LP.start_off(V, ld, off)), "row starts"
        return a, view

    ca, cv = place(c, case["ld_c"], case["off_c"])
    ua, uv = place(u, case["ld_u"], case["off_u"])
    oa = Arena((rows * case["ld_o"],), F32, case["off_o"])
    ov = oa.body.view(rows, case["ld_o"])[:, :V]
    assert [(ov[r].data_ptr() % 16) for r in range(rows)] == LP.row_starts(rows, case["ld_o"], F32, case["off_o"])
    before_c, before_u, before_o = ca.bits.clone(), ua.bits.clone(), oa.bits.clone()
    scale = scale_tensor(g)
    res = F.guided_logits(cv, uv, scale, out=ov)
    torch.cuda.synchronize()
    assert res is ov and float(scale) == g
    assert torch.equal(ca.bits, before_c) and torch.equal(ua.bits, before_u), "an input (or its surroundings, or a gap between its rows) was written"
    assert oa.intact(), "a write outside out"
    if case["ld_o"] > V:
        gaps = lambda bits: bits[oa.lo:oa.hi].view(rows, case["ld_o"])[:, V:]
        assert torch.equal(gaps(oa.bits), gaps(before_o)), "a gap between two rows of out was written"
    return ov.cpu()


@DTYPES
def test_kernel_within_the_bound_of_float64_on_every_designed_row(dtype):
    worst, n = 0.0, 0
    for case in GC.cases(dtype):
        for g in case["scales"]:
            out = run_case(case, g)
            ok, w = GC.within_bound(out, case["cond"], case["uncond"], g, CE_C_F)
            worst, n = max(worst, w), n + 1
            assert ok, f"{case['name']} g={g}: at {w:.4g} of the bound"
    print(f"MEASURED {str(dtype).replace('torch.', '')}: worst element at {worst:.3f} of its bound over {n} (case, scale) pairs")
    assert n >= 200


@DTYPES
def test_edge_rules(dtype):
    """G3: -inf in cond, in uncond, in both is exactly -inf at every scale (0 included), a NaN / +inf anywhere in either row makes the row
    NaN, a row of nothing but -inf is all -inf; the untouched rows keep the bits they have without any of it"""
    V = 2057 if dtype == BF16 else 1029
    c0, u0 = GC.pair(V, dtype, seed=4, rows=7)
    case = dict(ld_c=LP.odd_ld(V), off_c=1, ld_u=V, off_u=0, ld_o=V + 4, off_o=3)
    for g in (0.0, 0.5, 1.0, 3.0, 7.5):
        base = run_case(dict(case, cond=c0, uncond=u0), g)
        c, u = c0.clone(), u0.clone()
        c[0, 5] = u[0, V - 1] = GC.NINF
        c[1, 300] = u[1, 300] = GC.NINF
        c[2, 9] = float("nan")
        u[3, V // 2] = float("inf")
        u[4] = GC.NINF
        c[5, 0] = float("nan"); c[5, 1] = GC.NINF
        out = run_case(dict(case, cond=c, uncond=u), g)
        assert out[0, 5] == GC.NINF and out[0, V - 1] == GC.NINF and out[1, 300] == GC.NINF and int(torch.isinf(out[0]).sum()) == 2
        assert bool((out[4] == GC.NINF).all()) and bool(out[2].isnan().all()) and bool(out[3].isnan().all()) and bool(out[5].isnan().all())
        assert not bool((out == float("inf")).any())
        assert torch.equal(out[6].view(torch.int32), base[6].view(torch.int32))
        assert GC.within_bound(out[:2], c[:2], u[:2], g, CE_C_F)[0]


@DTYPES
def test_scale_one_and_zero_are_the_log_softmax_of_one_input(dtype):
    """g = 1: log_softmax(cond), g = 0: log_softmax(uncond), each within B of float64 - the other input, however different, leaves at most
    the roundings the bound's last term states; and x - out recovers an lse that agrees with ff_token_logprob's within that kernel's bound"""
    from flamingo_mini_amd import functional as F
    V = lc.V_GPT2[1]
    c, u = GC.pair(V, dtype, seed=5, rows=4)
    cd, ud = c.cuda(), u.cuda()
    tok = torch.zeros(4, dtype=torch.long, device="cuda")
    for g, x, xd in ((1.0, c, cd), (0.0, u, ud)):
        out = F.guided_logits(cd, ud, scale_tensor(g)).cpu().double()
        ref = x.double().log_softmax(-1)
        lse_ref = torch.logsumexp(x.double(), -1, keepdim=True)
        B = CE_C_F * 2.0 ** -24 * (lse_ref.abs() + x.double().abs() + 1.0)
        extra = 4 * 2.0 ** -24 * ((GC.reference(c, u, g)["d"].abs() * g) + 2 * ref.abs())
        ratio = float(((out - ref).abs() / (B + extra)).max())
        print(f"MEASURED g={g} {str(dtype).replace('torch.', '')}: at {ratio:.3f} of B")
        assert ratio <= 1.0
        lse = torch.zeros(4, device="cuda")
        F.token_logprobs(xd, tok, lse=lse)
        j = x.double().argmax(-1, keepdim=True)                          # at the row's largest logit: x_j - out_j = lse up to the roundings of out_j
        mine = (x.double().gather(1, j) - out.gather(1, j))[:, 0]
        slack = CE_C_F * 2.0 ** -24 * (lse_ref[:, 0].abs() + 1.0) + (B + extra).gather(1, j)[:, 0]
        assert float(((mine - lse.cpu().double()).abs() / slack).max()) <= 1.0


def test_wrapper_validation():
    from flamingo_mini_amd import functional as F
    x = torch.zeros((4, 64), dtype=BF16, device="cuda")
    s = scale_tensor(1.5)
    for bad in (dict(cond=x[:3]), dict(cond=x.float()), dict(cond=x.t()), dict(cond=x[0]), dict(scale=s.double()), dict(scale=torch.ones(2, device="cuda")),
                dict(out=torch.zeros((4, 64), dtype=BF16, device="cuda")), dict(out=torch.zeros((4, 63), device="cuda")), dict(out=torch.zeros((64, 4), device="cuda").t())):
        with pytest.raises(ValueError, match="guided_logits"):
            F.guided_logits(**dict(dict(cond=x, uncond=x, scale=s), **bad))
    wide = torch.zeros((8, 3, 64), dtype=BF16, device="cuda")                # row views are read in place
    out = F.guided_logits(wide[:4, -1], wide[4:, -1], s)
    assert out.shape == (4, 64) and out.dtype == torch.float32 and torch.allclose(out, torch.full_like(out, -4.158883), atol=1e-5)


def test_replay_follows_the_scale_on_the_device():
    """captured once; then the scale (and the logits) are rewritten on the device and every replay equals the eager call bit for bit"""
    from flamingo_mini_amd import functional as F
    rows, V = 5, 2049
    both = torch.zeros((2 * rows, 2, V), dtype=BF16, device="cuda")
    cond, uncond = both[:rows, -1], both[rows:, -1]
    scale, out = scale_tensor(1.0), torch.zeros((rows, V), device="cuda")
    call = lambda: F.guided_logits(cond, uncond, scale, out=out)
    call()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        call()
    seen = []
    c, u = GC.pair(V, BF16, seed=6, rows=rows)
    cond.copy_(c); uncond.copy_(u)
    for g in GC.SCALES:
        scale.fill_(g)
        out.fill_(float("nan"))
        graph.replay()
        got = out.clone()
        want = F.guided_logits(cond, uncond, scale_tensor(g))
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), g
        assert GC.within_bound(got.cpu(), c, u, g, CE_C_F)[0]
        seen.append(got.cpu())
    assert all(not torch.equal(a, b) for a, b in zip(seen, seen[1:]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the decode sessions
# ---------------------------------------------------------------------------------------------------------------------------------------
TAG = "guide"
G = 1.5


class Recorder:
    """records, inside the session, every step's raw 2 R-row logits (`_rec_raw`) and the guided buffer as functional.guided_logits leaves it
    (`_rec_g`), by device copies next to the session's own work: a step captured while this is installed records under replay too"""

    def __init__(self):
        self.session = None

    @contextlib.contextmanager
    def installed(self):
        from flamingo_mini_amd import decoding as Dec
        S, F = Dec._DecodeSession, Dec.F
        orig_append, orig_run, orig_guided = S._append, S.run, F.guided_logits
        rec = self

        def _append(sess, logits):
            if sess.guidance:
                if getattr(sess, "_rec_raw", None) is None:                    # (the first prompt step: eager)
                    sess._rec_raw = torch.full((logits.shape[0], sess.max_length, logits.shape[-1]), float("nan"), dtype=logits.dtype, device=logits.device)
                    sess._rec_g = torch.full((sess.b, sess.max_length, logits.shape[-1]), float("nan"), device=logits.device)
                sess._rec_raw.index_copy_(1, sess.pos, logits[:, None])
            orig_append(sess, logits)

        def guided(cond, uncond, scale, out=None):
            res = orig_guided(cond, uncond, scale, out=out)
            rec.session._rec_g.index_copy_(1, rec.session.pos, res[:, None])
            return res

        def run(sess, *a, **k):
            rec.session = sess
            for name in ("_rec_raw", "_rec_g"):
                if getattr(sess, name, None) is not None:
                    getattr(sess, name).fill_(float("nan"))
            return orig_run(sess, *a, **k)

        S._append, S.run, F.guided_logits = _append, run, guided
        try:
            yield self
        finally:
            S._append, S.run, F.guided_logits = orig_append, orig_run, orig_guided


def generate(model, inputs, max_length, graph=True, rec=None, **kw):
    ids, ml, am, vf = inputs
    model.decode_graph = graph
    try:
        with (rec.installed() if rec is not None else contextlib.nullcontext()):
            return model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=max_length, **kw)
    finally:
        model.decode_graph = True


@pytest.fixture(scope="module")
def g1():
    import test_hip_decode as D
    model, model64 = D.models("gpt2")
    model.reset_decode_sessions()
    yield D, model, model64
    model.decode_graph = True
    model.reset_decode_sessions()
    D._MODELS.clear()


def guided_f64(D, model64, seq, inputs, g):
    """float64 teacher-forced guided scores (b, L, V) on the host: two uncached forwards, with the media and without"""
    ids, ml, am, vf = inputs
    c = D.teacher_forced_f64(model64, seq, ml, am, vf)
    u = D.teacher_forced_f64(model64, seq, torch.zeros_like(ml), am, vf)
    return GC.reference(c.reshape(-1, c.shape[-1]), u.reshape(-1, c.shape[-1]), g)["out"].reshape(c.shape)


def errors_f64(got, ref):
    """(max-abs error of an entry, max-abs error of the differences winner - entry over the TOP_K entries that are highest in `ref`) of
    guided rows (..., V) against float64"""
    idx = ref.topk(TOP_K, dim=-1).indices
    g, r = got.double().gather(-1, idx), ref.gather(-1, idx)
    return float((got.double() - ref).abs().max()), float(((g[..., :1] - g) - (r[..., :1] - r)).abs().max())


def compared_prefix(a, b, ref, L0, margin):
    """the (row, step) pairs up to each row's first decision that the float64 scores do not decide - a top-two gap below the margin, or
    entry TOP_K + 1 less than 2 TOL_GUIDED_ROW below the first -, along a; asserts a == b there.  Returns the fraction of pairs compared."""
    a, b = a.cpu(), b.cpu()
    n_cmp, n_all = 0, 0
    for r in range(a.shape[0]):
        n_all += a.shape[1] - L0
        for pos in range(L0, a.shape[1]):
            top = ref[r, pos - 1].topk(TOP_K + 1).values
            if float(top[0] - top[1]) < margin or float(top[0] - top[TOP_K]) < 2 * TOL_GUIDED_ROW:
                break
            assert pos < b.shape[1] and int(a[r, pos]) == int(b[r, pos]), f"row {r} position {pos}: {int(a[r, pos])} against {int(b[r, pos])} at a float64 gap of {float(top[0] - top[1]):.3f}"
            n_cmp += 1
    return n_cmp / n_all


@pytest.mark.parametrize("batch", [4, 17])
def test_sessions_record_the_guided_scores_and_choose_their_argmax(g1, batch):
    D, model, model64 = g1
    inputs = D.make_inputs(batch, 1, TAG)
    L0, R = D.L0, batch
    model.reset_decode_sessions()
    rec = Recorder()
    out = generate(model, inputs, D.MAXLEN, rec=rec, guidance_scale=G)
    sess = rec.session
    (key,) = [k for k, s in model._decode_sessions.items() if s is sess]
    assert key[-1] == "guidance" and key[:10] == (batch, D.MAXLEN, 1, "cuda:0", None, None, True, None, None, None) and len(key) == 11
    assert sess.guidance and sess.replay is not None and not sess.capture_failed
    raw_v = model.flamingo.lm_head.weight.shape[0]                            # (the vocabulary plus <EOC>)
    assert sess.am_buf.shape[0] == sess.tt_step.shape[0] == sess.lm_tok.shape[0] == 2 * R and sess.ids_buf.shape[0] == sess.tok.shape[0] == R
    assert sess.guided.shape == (R, raw_v) and all(k.shape[0] == 2 * R for k, v in sess.xattn_past) and float(sess.scale) == G
    assert bool((sess.tt_step[R:] == 0).all()) and int((sess.tt_step[:R] != 0).sum()) >= R - 1
    raw, guided = sess._rec_raw.clone(), sess._rec_g.clone()
    assert out.shape == (R, D.MAXLEN) and bool(torch.isfinite(guided[:, L0:]).all()) and bool(torch.isfinite(raw[:, L0:].float()).all())
    worst = 0.0
    for pos in range(L0, D.MAXLEN):
        c, u = raw[:R, pos].cpu(), raw[R:, pos].cpu()
        ok, w = GC.within_bound(guided[:, pos].cpu(), c, u, G, CE_C_F)
        worst = max(worst, w)
        assert ok, f"position {pos}: the guided buffer at {w:.4g} of the kernel bound of its own logits"
        assert torch.equal(guided[:, pos].argmax(-1), out[:, pos]), f"position {pos}: the token is not the argmax of the guided buffer"
    assert not torch.equal(raw[:R, L0:], raw[R:, L0:]), "the two halves are equal: the media change nothing here"
    # eager steps: the same bits
    eager_rec = Recorder()
    eager = generate(model, inputs, D.MAXLEN, graph=False, rec=eager_rec, guidance_scale=G)
    es = eager_rec.session
    assert es is not sess and es.replay is None and torch.equal(eager, out)
    assert torch.equal(es._rec_raw[:, L0:].view(torch.int16), raw[:, L0:].view(torch.int16)) and torch.equal(es._rec_g[:, L0:].view(torch.int32), guided[:, L0:].view(torch.int32))
    # against the float64 teacher-forced guided scores: the error the margin of the static-against-dynamic test is set from
    ref = guided_f64(D, model64, out, inputs, G)
    err, err_top = errors_f64(guided[:, L0:].cpu(), ref[:, L0 - 1:-1])
    D._report(f"guided-f64-row-b{batch}", err)
    D._report(f"guided-f64-gap-b{batch}", err_top)
    print(f"MEASURED batch {batch}: guided buffer at most {worst:.3f} of the kernel bound; |guided - float64 teacher forced| {err:.3e} in the row, {err_top:.3e} in the differences to the top {TOP_K}")
    # the dynamic form on the same sequences: two uncached bf16 forwards on the GPU, combined by guided_logits_torch
    from flamingo_mini_amd.decoding import guided_logits_torch
    ids, ml, am, vf = inputs
    mlf, amf = D.extend(ml, am, out.shape[1])
    with torch.no_grad():
        c = model(input_ids=out, attention_mask=amf, media_locations=mlf, visual_features=vf).logits[:, L0 - 1:-1]
        u = model(input_ids=out, attention_mask=amf, media_locations=torch.zeros_like(mlf), visual_features=vf).logits[:, L0 - 1:-1]
    dyn_scores = guided_logits_torch(c.reshape(-1, c.shape[-1]).float(), u.reshape(-1, c.shape[-1]).float(), G).reshape(c.shape)
    err_d, err_top_d = errors_f64(dyn_scores.cpu(), ref[:, L0 - 1:-1])
    D._report(f"guided-f64-row-dynamic-b{batch}", err_d)
    D._report(f"guided-f64-gap-dynamic-b{batch}", err_top_d)
    print(f"MEASURED batch {batch}: the dynamic form {err_d:.3e} in the row, {err_top_d:.3e} in the differences to the top {TOP_K}")
    # static against dynamic, greedy
    dyn = generate(model, inputs, D.MAXLEN, static_decode=False, guidance_scale=G)
    frac = compared_prefix(out, dyn, ref, L0, MARGIN)
    print(f"MEASURED batch {batch}: static against dynamic greedy, {frac:.2%} of the (row, step) pairs compared")
    assert max(err, err_d) <= TOL_GUIDED_ROW and max(err_top, err_top_d) <= TOL_GUIDED_GAP and frac >= 0.8


def test_scale_zero_is_the_ordinary_static_decode_without_media(g1):
    D, model, model64 = g1
    inputs = D.make_inputs(4, 1, TAG)
    ids, ml, am, vf = inputs
    model.reset_decode_sessions()
    plain_rec = D._Recorder()
    plain, plain_logits = D.decode(model, plain_rec, ids, torch.zeros_like(ml), am, vf)
    rec = Recorder()
    out = generate(model, inputs, D.MAXLEN, rec=rec, guidance_scale=0.0)
    guided = rec.session._rec_g[:, D.L0:].cpu()
    ref = plain_logits[:, D.L0:].cpu().double().log_softmax(-1)
    if torch.equal(out, plain):                                              # the same tokens: the guided rows are the log-softmax of the plain rows
        D.chosen_consistent(out, ref, guided, D.L0)
    frac = compared_prefix(out, plain, guided_f64(D, model64, out, inputs, 0.0), D.L0, MARGIN)
    print(f"MEASURED g = 0 against the plain decode without media: equal {torch.equal(out, plain)}, {frac:.2%} compared")
    assert frac >= 0.8


@pytest.mark.parametrize("groups", [{}, dict(num_beam_groups=3, diversity_penalty=0.5)], ids=["beams", "groups"])
def test_static_and_dynamic_beam_search_agree(g1, groups):
    D, model, model64 = g1
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    kw = dict(num_beams=3, guidance_scale=G, **groups)
    static = generate(model, inputs, D.MAXLEN, static_decode=True, **kw)
    sess = [s for s in model._decode_sessions.values() if s.beams is not None][-1]
    assert sess.guidance and sess.replay is not None and not sess.capture_failed and sess.lm_beam_idx.shape == (24,) and sess.b == 12
    assert sess.am_buf.shape[0] == 24 and sess.guided.shape == (12, model.flamingo.lm_head.weight.shape[0])
    assert torch.equal(sess.lm_beam_idx[12:], sess.lm_beam_idx[:12] + 12)
    assert torch.equal(generate(model, inputs, D.MAXLEN, static_decode=True, graph=False, **kw), static), "eager and replayed steps differ"
    dyn = generate(model, inputs, D.MAXLEN, **kw)
    ref = guided_f64(D, model64, static, inputs, G)
    frac = compared_prefix(static, dyn, ref, D.L0, MARGIN)
    print(f"MEASURED beam search {groups or ''}: static against dynamic, {frac:.2%} of the (row, step) pairs compared; equal {torch.equal(static, dyn)}")
    assert frac >= 0.8


def test_sampling_sessions(g1):
    """the same seed gives the same tokens eagerly and under replay; token_logprobs are within the loss bound of the log-softmax of the
    recorded guided rows"""
    D, model, _ = g1
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    gen = lambda: torch.Generator(device="cuda").manual_seed(3)
    kw = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, static_decode=True, guidance_scale=G)
    rec = Recorder()
    out = generate(model, inputs, D.MAXLEN, rec=rec, return_dict_in_generate=True, output_logprobs=True, generator=gen(), **kw)
    sess = rec.session
    assert sess.sampling is not None and sess.logprobs and sess.replay is not None and not sess.capture_failed
    again = generate(model, inputs, D.MAXLEN, return_dict_in_generate=True, output_logprobs=True, generator=gen(), **kw)
    eager = generate(model, inputs, D.MAXLEN, graph=False, return_dict_in_generate=True, output_logprobs=True, generator=gen(), **kw)
    assert torch.equal(again.sequences, out.sequences) and torch.equal(eager.sequences, out.sequences)
    assert torch.equal(eager.token_logprobs.view(torch.int32), out.token_logprobs.view(torch.int32))
    assert torch.equal(generate(model, inputs, D.MAXLEN, generator=gen(), **kw), out.sequences)
    assert not torch.equal(generate(model, inputs, D.MAXLEN, generator=gen(), **dict(kw, guidance_scale=1.0)), out.sequences)
    worst = 0.0
    for pos in range(D.L0, D.MAXLEN):
        x, tok = sess._rec_g[:, pos].cpu(), out.sequences[:, pos].cpu()
        lp_ref, lse_ref, xt = LP.reference(x, tok)
        w = float(((out.token_logprobs[:, pos - D.L0].cpu().double() - lp_ref).abs() / (CE_C_F * 2.0 ** -24 * (lse_ref.abs() + xt.abs() + 1.0))).max())
        worst = max(worst, w)
        assert w <= 1.0, f"position {pos}: a log-probability at {w:.4g} of its bound"
    print(f"MEASURED sampling: worst log-probability at {worst:.3f} of the loss bound of the guided rows")


def test_another_scale_reuses_the_session_and_scale_one_builds_the_unguided_key(g1):
    D, model, _ = g1
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    a = generate(model, inputs, D.MAXLEN, guidance_scale=1.5)
    (sess,) = model._decode_sessions.values()
    graph = sess.graph
    b = generate(model, inputs, D.MAXLEN, guidance_scale=7.5)
    zero = generate(model, inputs, D.MAXLEN, guidance_scale=0.0)
    assert len(model._decode_sessions) == 1 and next(iter(model._decode_sessions.values())) is sess and sess.graph is graph and float(sess.scale) == 0.0
    assert not torch.equal(a, b) and not torch.equal(b, zero)
    assert torch.equal(generate(model, inputs, D.MAXLEN, guidance_scale=1.5), a) and torch.equal(generate(model, inputs, D.MAXLEN, guidance_scale=1.5, graph=False), a)
    plain = generate(model, inputs, D.MAXLEN, guidance_scale=1.0)
    keys = list(model._decode_sessions)
    assert any(len(k) == 10 for k in keys) and sum(k[-1] == "guidance" for k in keys) == 2          # (the replayed and the eager guided session)
    unguided = [s for k, s in model._decode_sessions.items() if len(k) == 10][0]
    assert unguided.guidance is False and not hasattr(unguided, "lm_tok") and unguided.am_buf.shape[0] == 4
    assert torch.equal(plain, generate(model, inputs, D.MAXLEN)) and not torch.equal(plain, b)
