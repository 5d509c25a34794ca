"""Token log-probabilities on the MI355X: ff_token_logprob / functional.token_logprobs (csrc/ff_logprob.hip) and the decode sessions that
record them.

The kernel: every designed row of tests/logprob_cases.py in both dtypes, through arenas whose surroundings hold a sentinel (the arenas of
tests/test_hip_loss_bounds.py), at ld == V, ld == 2 V (the [:, -1] view, through the wrapper) and an odd ld > V, against float64 from the
stored values under the project's loss bound (tests/util.py CE_C_F):
    |lp - lp*| <= CE_C_F 2^-24 (|lse*| + |x_tok| + 1),    |lse - lse*| <= CE_C_F 2^-24 (|lse*| + 1);
the edge rules; bit equality with ff_shifted_ce_fwd on contiguous (3, 9, V) tensors and, on and off the grid, at GPT-2's vocabularies (the
only ones at which the kernel's four-vectors-at-once loop makes several trips and leaves a remainder); graph replay with device-side changes.
The sessions (G1 geometry of tests/test_hip_decode.py, batch 4): greedy and sampling with output_logprobs=True return the tokens of the
call without it, eager and replayed steps give the same bits, every value is within the loss bound of float64 from that step's logits as
the selection saw them (recorded in the eager run), 0 after eos; num_return_sequences for sampling and beam search; the routing."""
import contextlib

import pytest
import torch

import logprob_cases as LP
import loss_cases as lc
from util import CE_C_F

pytestmark = pytest.mark.gpu
BF16, F32 = LP.BF16, LP.F32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
BITS = {F32: torch.int32, BF16: torch.int16}


def run_case(x, tok, ld, off, skip=None, want_lse=True, wrapper=False):
    """ff_token_logprob on x's rows laid out with row stride ld, the first `off` elements off the 16-byte grid, inside an arena; the gaps
    between the rows hold NaN.  Returns (logprob, lse) on the CPU after checking that nothing but the two outputs' bodies was written.
    wrapper=True (ld == 2 V): through functional.token_logprobs on the [:, -1] view of a (rows, 2, V) tensor."""
    from flamingo_mini_amd import ffi, functional as F
    from test_hip_loss_bounds import Arena
    rows, V = x.shape
    dtype = x.dtype
    xa = Arena((rows * ld,), dtype, off)
    if wrapper:
        assert ld == 2 * V
        view = xa.body.view(rows, 2, V)[:, -1]
    else:
        view = xa.body.view(rows, ld)[:, :V]
    view.copy_(x)
    es = x.element_size()                                   # the rows start where the cases' bookkeeping (LP.start_off, LP.row_starts) says
    assert [(view[r].data_ptr() % 16) for r in range(rows)] == LP.row_starts(rows, ld, dtype, LP.start_off(V, ld, off)), "row starts"
    assert es == 16 // lc.NVEC[dtype]
    lpa, lsa = Arena((rows,), F32), Arena((rows,), F32)
    tokd = tok.cuda()
    skipd = None if skip is None else skip.cuda()
    before = xa.bits.clone()
    if wrapper:
        out = F.token_logprobs(view, tokd, skip=skipd, out=lpa.body, lse=lsa.body if want_lse else None)
        assert out is lpa.body
    else:
        ffi.check(ffi.lib().ff_token_logprob(ffi.dtype_code(dtype), rows, V, ld, view.data_ptr(), tokd.data_ptr(), ffi.ptr(skipd), lpa.body.data_ptr(),
                                             lsa.body.data_ptr() if want_lse else None, ffi.stream_handle(view.device)), "ff_token_logprob")
    torch.cuda.synchronize()
    assert torch.equal(xa.bits, before), "the logits (or their surroundings, or the gaps between the rows) were written"
    assert lpa.intact() and lsa.intact(), "a write outside an output"
    assert torch.equal(tokd.cpu(), tok) and (skip is None or torch.equal(skipd.cpu(), skip))
    if not want_lse:
        assert bool(torch.isnan(lsa.body).all()), "lse was written although null"
    return lpa.body.cpu(), lsa.body.cpu()


@DTYPES
@pytest.mark.parametrize("group", LP.GROUPS)
def test_kernel_within_the_loss_bound_of_float64_on_every_designed_row(dtype, group):
    n, worst, regions, phases = 0, [0.0, 0.0], set(), set()
    es = 16 // lc.NVEC[dtype]
    for name, x, tok, ld, off in LP.cases(dtype, (group,)):
        V = x.shape[1]
        lp, lse = run_case(x, tok, ld, off, wrapper=ld == 2 * V)
        start_off = LP.start_off(V, ld, off)
        ok, w_lp, w_lse = LP.within_bounds(lp, lse, x, tok, CE_C_F)
        print(f"{str(dtype).replace('torch.', '')} {name}: logprob at {w_lp:.3f}, lse at {w_lse:.3f} of their bounds")
        worst = [max(worst[0], w_lp), max(worst[1], w_lse)]
        assert ok, f"{name}: logprob at {w_lp:.4g}, lse at {w_lse:.4g} of their bounds"
        regions |= LP.token_regions(V, dtype, tok, ld, start_off)
        if V >= 9:
            phases |= {s // es for s in LP.row_starts(len(tok), ld, dtype, start_off)}
        n += 1
    print(f"worst over {n} {group} cases: logprob {worst[0]:.3f}, lse {worst[1]:.3f}")
    assert n >= 8 and {"body", "tail"} <= regions          # (head as well, over all groups: the next test)
    assert phases == set(range(lc.NVEC[dtype])), phases


@DTYPES
def test_tokens_fall_in_head_body_and_tail_at_the_starts_the_kernel_sees(dtype):
    """over all groups, with every row's start taken as run_case lays it out (and checks against the data pointers): the chosen tokens
    fall in the scalar head, the vector body and the scalar tail, in every group"""
    for group in LP.GROUPS:
        regions = set()
        for name, x, tok, ld, off in LP.cases(dtype, (group,)):
            regions |= LP.token_regions(x.shape[1], dtype, tok, ld, LP.start_off(x.shape[1], ld, off))
        assert regions == {"head", "body", "tail"}, (group, regions)


@DTYPES
def test_edge_rules(dtype):
    """skipped rows are exactly 0.0 in both outputs and are not read (they hold NaN); a token outside [0, V) gives NaN; x_tok = -inf
    gives -inf; a row holding NaN or +inf gives NaN; a null lse is not written; the other rows keep the bits they have without any of it"""
    V = lc.V_LARGE
    x0 = lc.logits(V, dtype, seed=7)[0].reshape(LP.R, V)[:4].clone()
    tok0 = LP.tokens(V, 2, rows=4)
    base_lp, base_lse = run_case(x0, tok0, LP.odd_ld(V), 1)
    assert LP.within_bounds(base_lp, base_lse, x0, tok0, CE_C_F)[0]
    same = lambda a, b, rows: torch.equal(a[rows].view(torch.int32), b[rows].view(torch.int32))
    # skip flags, as bool and as uint8
    for flags in (torch.tensor([False, True, False, True]), torch.tensor([0, 0, 7, 0], dtype=torch.uint8)):
        x = x0.clone()
        x[flags != 0] = float("nan")
        lp, lse = run_case(x, tok0, LP.odd_ld(V), 1, skip=flags)
        on = flags != 0
        assert lp[on].view(torch.int32).tolist() == [0] * int(on.sum()) and lse[on].view(torch.int32).tolist() == [0] * int(on.sum())
        assert same(lp, base_lp, ~on) and same(lse, base_lse, ~on)
    # tokens out of range: NaN, lse still the row's
    tok = tok0.clone()
    tok[0], tok[1], tok[3] = -1, V, 1 << 40
    lp, lse = run_case(x0, tok, LP.odd_ld(V), 1)
    assert bool(torch.isnan(lp[[0, 1, 3]]).all()) and same(lp, base_lp, [2]) and same(lse, base_lse, [0, 1, 2, 3])
    # x_tok = -inf; -inf elsewhere; NaN / +inf in a row
    x = x0.clone()
    x[0, tok0[0]] = float("-inf")
    x[1, (int(tok0[1]) + 5) % V] = float("nan")
    x[2, (int(tok0[2]) + 5) % V] = float("inf")
    lp, lse = run_case(x, tok0, LP.odd_ld(V), 1, want_lse=False)
    assert float(lp[0]) == float("-inf") and bool(torch.isnan(lp[1])) and bool(torch.isnan(lp[2])) and same(lp, base_lp, [3])


EQ_SHAPES = [(3, 9, 33, 0), (3, 9, 2049, 0), (3, 9, 4099, 0)] + [(2, 4, V, off) for V in lc.V_GPT2 for off in (0, 1)]


@DTYPES
@pytest.mark.parametrize("b,L,V,off", EQ_SHAPES, ids=lambda v: str(v))
def test_bit_equality_with_the_loss_forward(dtype, b, L, V, off):
    """a contiguous (b, L, V) tensor whose first element is `off` elements off the 16-byte grid, token[b, i] = labels[b, i + 1]: on the
    b (L - 1) scored rows lse has ff_shifted_ce_fwd's bits and logprob == -loss_row bit for bit.  (3, 9, V) at V = 33, 2049, 4099; and
    (2, 4, V) at GPT-2's vocabularies, on and off the grid, where every thread of token_logprob_kernel makes several trips through its
    four-vectors-at-once loop and finishes in the plain one (24 - 25 vectors per thread in bf16, 49 - 50 in fp32) - the loss kernel, whose
    loop is the plain one throughout, is what holds that loop's indexing and order to the bit."""
    from flamingo_mini_amd import ffi
    N = lc.NVEC[dtype]
    nvec = (V - N) // N                                                          # at least this many vectors in every row
    assert V < 5000 or nvec // 256 >= 4 * 2 + 1, "the large shapes must reach several unrolled trips and a remainder"
    x = lc.logits(V, dtype, b=b, L_=L, seed=8)[0]
    lab = lc.labels(V, b=b, L_=L, start=5)
    lab[lab == lc.IGNORE] = V // 3
    flat = torch.empty(x.numel() + 16, dtype=dtype, device="cuda")
    xd = flat[off:off + x.numel()].view(x.shape)
    xd.copy_(x)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == off * x.element_size()
    labd = lab.cuda()
    lib, code, st = ffi.lib(), ffi.dtype_code(dtype), ffi.stream_handle(xd.device)
    loss, lse = torch.full((b * (L - 1),), float("nan"), device="cuda"), torch.full((b * (L - 1),), float("nan"), device="cuda")
    ffi.check(lib.ff_shifted_ce_fwd(code, b, L, V, xd.data_ptr(), labd.data_ptr(), lc.IGNORE, loss.data_ptr(), lse.data_ptr(), st), "ff_shifted_ce_fwd")
    tok = torch.zeros((b, L), dtype=torch.long)
    tok[:, :-1] = lab[:, 1:]
    tokd = tok.reshape(-1).cuda()
    lp, lse2 = torch.full((b * L,), float("nan"), device="cuda"), torch.full((b * L,), float("nan"), device="cuda")
    ffi.check(lib.ff_token_logprob(code, b * L, V, V, xd.data_ptr(), tokd.data_ptr(), None, lp.data_ptr(), lse2.data_ptr(), st), "ff_token_logprob")
    torch.cuda.synchronize()
    scored = torch.tensor([s * L + i for s in range(b) for i in range(L - 1)], device="cuda")
    assert scored.numel() == b * (L - 1) and (scored.numel() == 24 or V > 5000) and bool(torch.isfinite(loss).all())
    assert torch.equal(lse2[scored].view(torch.int32), lse.view(torch.int32))
    assert torch.equal(lp[scored].view(torch.int32), (-loss).view(torch.int32))


def test_replay_follows_device_side_logits_tokens_and_flags():
    """captured once; then the logits, the tokens and the skip flags change on the device and every replay equals the eager call bit for bit"""
    from flamingo_mini_amd import functional as F
    rows, V = 5, 2049
    wide = torch.zeros((rows, 2, V), dtype=BF16, device="cuda")
    logits = wide[:, -1]
    tok = torch.zeros(rows, dtype=torch.long, device="cuda")
    skip = torch.zeros(rows, dtype=torch.bool, device="cuda")
    out, lse = torch.zeros(rows, device="cuda"), torch.zeros(rows, device="cuda")
    call = lambda: F.token_logprobs(logits, tok, skip=skip, out=out, lse=lse)
    call()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        call()
    seen = set()
    for seed in range(4):
        x = lc.logits(V, BF16, b=1, L_=rows, seed=20 + seed)[0][0]
        logits.copy_(x)
        tok.copy_(LP.tokens(V, 3 * seed, rows=rows))
        skip.copy_(torch.tensor([(r + seed) % 3 == 0 for r in range(rows)]))
        out.fill_(float("nan")); lse.fill_(float("nan"))
        graph.replay()
        got = (out.clone(), lse.clone())
        want = (torch.full_like(out, float("nan")), torch.full_like(lse, float("nan")))
        F.token_logprobs(logits, tok, skip=skip, out=want[0], lse=want[1])
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), seed
        keep = ~skip.cpu()
        assert LP.within_bounds(got[0].cpu()[keep], got[1].cpu()[keep], x[keep], tok.cpu()[keep], CE_C_F)[0]
        assert got[0].cpu()[~keep].tolist() == [0.0] * int((~keep).sum())
        seen.add(tuple(got[0].cpu().tolist()))
    assert len(seen) == 4


# ---------------------------------------------------------------------------------------------------------------------------------------
# the decode sessions (G1 geometry of tests/test_hip_decode.py, batch 4)
# ---------------------------------------------------------------------------------------------------------------------------------------
TAG = "scores"                    # (greedy decoding of this small model soon repeats one token; with these inputs the four rows repeat different ones)
LOGP = dict(static_decode=True, return_dict_in_generate=True, output_logprobs=True)
SAMPLING = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9)


@pytest.fixture(scope="module")
def g1():
    import test_hip_decode as D
    model, _ = D.models("gpt2")
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    yield D, model, inputs
    model.decode_graph = True
    model.reset_decode_sessions()
    D._MODELS.clear()


@contextlib.contextmanager
def selections_recorded(store):
    """wraps _TokenSession._select in an EAGER run: the logits the selection sees (after the processors), per position; `raw` of _append"""
    from flamingo_mini_amd import decoding
    S, B = decoding._TokenSession, decoding._DecodeSession          # each method is wrapped on the class that defines it, and put back there
    orig_select, orig_append = S._select, B._append

    def _append(sess, logits):
        store.setdefault("raw", {})[int(sess.pos)] = logits.detach().clone()
        orig_append(sess, logits)

    def _select(sess, logits):
        store.setdefault("seen", {})[int(sess.pos)] = logits.detach().clone()
        store["session"] = sess
        orig_select(sess, logits)

    S._select, B._append = _select, _append
    try:
        yield store
    finally:
        S._select, B._append = orig_select, orig_append


def generate(model, inputs, max_length, graph=True, store=None, **kw):
    ids, ml, am, vf = inputs
    model.decode_graph = graph
    try:
        with (selections_recorded(store) if store is not None else contextlib.nullcontext()):
            return model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=max_length, **kw)
    finally:
        model.decode_graph = True


def gen(seed=1):
    return torch.Generator(device="cuda").manual_seed(seed)


def mid_way_eos(plain, L0):
    """an eos that some rows emit and others do not (as tests/test_hip_decode.py::test_decode_eos_under_replay forces one), so that rows
    stop while others go on: among such tokens the one first emitted latest, at least two steps before the end"""
    g = plain[:, L0:].cpu()
    first = {int(t): min(int((g[r] == t).nonzero()[0, 0]) for r in range(g.shape[0]) if bool((g[r] == t).any())) for t in g.flatten().unique()}
    cands = [t for t, j in first.items() if 0 < int((g == t).any(1).sum()) < g.shape[0] and j <= g.shape[1] - 3]
    assert cands, g.tolist()
    return max(cands, key=lambda t: (first[t], t))


def held_to_the_recorded_logits(out, seen, L0, eos, pad):
    """every token_logprobs value against float64 from the logits the selection saw at that step; exactly 0 for a row that had finished"""
    seqs, lps = out.sequences.cpu(), out.token_logprobs.cpu()
    finished = torch.zeros(seqs.shape[0], dtype=torch.bool)
    worst, zeros, eos_seen = 0.0, 0, 0
    for pos in range(L0, seqs.shape[1]):
        x = seen[pos].float().cpu()
        tok = seqs[:, pos]
        live = ~finished
        if bool(finished.any()):
            assert lps[finished, pos - L0].view(torch.int32).tolist() == [0] * int(finished.sum()) and bool((tok[finished] == pad).all())
            zeros += int(finished.sum())
        lp_ref, lse_ref, xt = LP.reference(x[live], tok[live])
        ratio = (lps[live, pos - L0].double() - lp_ref).abs() / (CE_C_F * 2.0 ** -24 * (lse_ref.abs() + xt.abs() + 1.0))
        w = float(torch.nan_to_num(ratio, nan=float("inf")).max())
        worst = max(worst, w)
        assert w <= 1.0, f"position {pos}: a log-probability at {w:.4g} of its bound"
        if eos is not None:
            hit = live & (tok == eos)                      # the eos token itself carries its log-probability: the skip flags the kernel
            assert bool((lps[hit, pos - L0] != 0).all())   # reads are `finished` BEFORE this step's eos rule, not after it
            eos_seen += int(hit.sum())
            finished = finished | (tok == eos)
    assert eos is None or eos_seen > 0
    return worst, zeros


@pytest.mark.parametrize("mode", ["greedy", "sampling"])
def test_sessions_record_log_probabilities(g1, mode):
    from flamingo_mini_amd import GenerateOutput
    D, model, inputs = g1
    L0 = D.L0
    extra = dict(SAMPLING) if mode == "sampling" else {}
    g = (lambda: dict(generator=gen())) if mode == "sampling" else (lambda: {})
    free = generate(model, inputs, D.MAXLEN, static_decode=True, **extra, **g())
    eos = mid_way_eos(free, L0)
    pad = 0 if eos != 0 else 1
    kw = dict(extra, eos_token_id=eos, pad_token_id=pad)
    plain = generate(model, inputs, D.MAXLEN, static_decode=True, **kw, **g())
    out = generate(model, inputs, D.MAXLEN, **LOGP, **kw, **g())
    assert isinstance(out, GenerateOutput) and torch.equal(out.sequences, plain)
    assert out.token_logprobs.dtype == torch.float32 and out.token_logprobs.shape == (4, plain.shape[1] - L0)
    key, sess = [(k, s) for k, s in model._decode_sessions.items() if len(k) == 11 and k[-1] == "logprobs" and k[4] == eos][-1]
    assert sess.logprobs and sess.replay is not None and not sess.capture_failed and key[:10] == (4, D.MAXLEN, 1, "cuda:0", eos, pad, True, sess.sampling, None, None)
    store = {}
    eager = generate(model, inputs, D.MAXLEN, graph=False, store=store, **LOGP, **kw, **g())
    assert store["session"].replay is None and store["session"].logprobs
    assert torch.equal(eager.sequences, plain)
    assert torch.equal(eager.token_logprobs.view(torch.int32), out.token_logprobs.view(torch.int32)), "eager and replayed steps differ"
    worst, zeros = held_to_the_recorded_logits(out, store["seen"], L0, eos, pad)
    print(f"MEASURED {mode}: worst log-probability at {worst:.3f} of its bound; {zeros} positions after eos")
    assert zeros > 0
    n_gen = [(row.index(eos) + 1 if eos in row else len(row)) for row in plain[:, L0:].tolist()]      # the scores: the stated formula
    norm = torch.tensor([float(L0 + k) for k in n_gen], dtype=torch.float32, device="cuda")
    assert out.sequences_scores.shape == (4,) and torch.allclose(out.sequences_scores, out.token_logprobs.sum(1) / norm, rtol=1e-6, atol=0)
    # a default call afterwards: a ten-element key, today's tokens
    again = generate(model, inputs, D.MAXLEN, static_decode=True, **kw, **g())
    assert torch.equal(again, plain) and any(len(k) == 10 and k[4] == eos for k in model._decode_sessions)
    assert len(model._decode_sessions) <= 4


def test_values_are_taken_after_the_processors(g1):
    """repetition_penalty 1.3, no_repeat_ngram_size 2: every value is within the bound of float64 from the PROCESSED logits, and at some
    positions it is outside the bound of the raw ones"""
    D, model, inputs = g1
    L0 = D.L0
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    plain = generate(model, inputs, D.MAXLEN, static_decode=True, **kw)
    out = generate(model, inputs, D.MAXLEN, **LOGP, **kw)
    sess = [s for k, s in model._decode_sessions.items() if len(k) == 11 and k[9] == (1.3, 2, 0, 0)][-1]
    assert torch.equal(out.sequences, plain) and sess.replay is not None and not sess.capture_failed
    store = {}
    eager = generate(model, inputs, D.MAXLEN, graph=False, store=store, **LOGP, **kw)
    assert torch.equal(eager.sequences, plain) and torch.equal(eager.token_logprobs.view(torch.int32), out.token_logprobs.view(torch.int32))
    worst, _ = held_to_the_recorded_logits(out, store["seen"], L0, None, None)
    seqs, lps, off_raw = out.sequences.cpu(), out.token_logprobs.cpu(), 0
    for pos in range(L0, seqs.shape[1]):
        raw = store["raw"][pos].float().cpu()
        lp_ref, lse_ref, xt = LP.reference(raw, seqs[:, pos])
        off_raw += int(((lps[:, pos - L0].double() - lp_ref).abs() > CE_C_F * 2.0 ** -24 * (lse_ref.abs() + xt.abs() + 1.0)).sum())
    print(f"MEASURED processors: worst at {worst:.3f} of the bound on the processed logits; {off_raw} values outside the raw logits' bound")
    assert off_raw > 0


def test_num_return_sequences_sampling(g1):
    D, model, inputs = g1
    ids, ml, am, vf = inputs
    out = generate(model, inputs, D.MAXLEN, static_decode=True, num_return_sequences=3, **SAMPLING, generator=gen(4))
    assert out.shape == (12, D.MAXLEN) and all(torch.equal(out[r, :D.L0], ids[r // 3]) for r in range(12))
    rep = tuple(t.repeat_interleave(3, dim=0) for t in inputs)
    assert torch.equal(out, generate(model, rep, D.MAXLEN, static_decode=True, **SAMPLING, generator=gen(4)))
    assert len({tuple(r) for r in out[:3].tolist()}) > 1, "the three samples of a sequence are identical"
    boxed = generate(model, inputs, D.MAXLEN, num_return_sequences=3, **LOGP, **SAMPLING, generator=gen(4))
    assert torch.equal(boxed.sequences, out) and boxed.token_logprobs.shape == (12, D.MAXLEN - D.L0) and boxed.sequences_scores.shape == (12,)


@pytest.mark.parametrize("static", [True, None], ids=["static", "dynamic"])
def test_num_return_sequences_beam_search(g1, static):
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    D, model, inputs = g1
    kw = dict(num_beams=3, static_decode=static)
    single = generate(model, inputs, D.MAXLEN, **kw)
    out = generate(model, inputs, D.MAXLEN, num_return_sequences=3, return_dict_in_generate=True, **kw)
    assert out.sequences.shape[0] == 12 and out.sequences_scores.shape == (12,) and out.sequences_scores.dtype == torch.float32 and out.token_logprobs is None
    first = out.sequences[::3]
    assert torch.equal(first[:, :single.shape[1]], single) and bool(torch.isfinite(out.sequences_scores).all())
    scores = out.sequences_scores.view(4, 3)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), scores
    assert torch.equal(generate(model, inputs, D.MAXLEN, num_return_sequences=3, **kw), out.sequences)
    one = generate(model, inputs, D.MAXLEN, return_dict_in_generate=True, **kw)
    assert torch.equal(one.sequences, single) and torch.equal(one.sequences_scores, out.sequences_scores[::3])
    if static:
        sess = [s for s in model._decode_sessions.values() if s.beams is not None][-1]
        assert sess.replay is not None and not sess.capture_failed
        host = sess.state.to_host()
        host["length"] = D.MAXLEN
        ids1, s1 = _beam_finalize(host, D.L0, inputs[0].cpu(), 3, sess.fill, n_return=1)
        assert torch.equal(ids1.cuda(), single) and torch.equal(s1.cuda(), out.sequences_scores[::3])
    else:
        assert not any(s.beams is not None and len(k) == 11 for k, s in model._decode_sessions.items())


def test_routing_with_cpu_tensors():
    """CPU tensors: static_decode=True with output_logprobs=True raises what ffi.require_cuda raises; static_decode=None decodes dynamically
    and returns the output object (the tiny host model on the oracle backend)"""
    import oracle_backend
    from flamingo_mini_amd import GenerateOutput, ffi
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", "gpt2")
        model.eval()
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        kw = dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=torch.from_numpy(z["px"]).double(), max_length=8)
        with pytest.raises(ffi.FusionLibraryError, match="no CPU fallback"):
            model.generate(ids, static_decode=True, return_dict_in_generate=True, output_logprobs=True, **kw)
        out = model.generate(ids, return_dict_in_generate=True, output_logprobs=True, **kw)
        assert isinstance(out, GenerateOutput) and len(model._decode_sessions) == 0
        assert torch.equal(out.sequences, model.generate(ids, **kw)) and out.token_logprobs.shape == (ids.shape[0], 4)
    finally:
        oracle_backend.uninstall()
