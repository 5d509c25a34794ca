"""bf16 cached caption decoding of whole models against a float64 reference.

greedy_generate on the GPU runs through modeling_flamingo._DecodeSession (StaticCache, cross-attention K/V copied into persistent buffers,
one decode step captured into a HIP graph and replayed).  At <= 32 rows in bf16 the feed-forward half of every gated block runs the decode
kernels of csrc/ff_decode.hip (LayerNorm + up-projection, then a down-projection whose K slices are combined inside the launch through
tickets), and the cross-attention reads cached K/V with n_q = 1 through the resident-operand kernel (dim <= 1536, <= 64 keys) or the general
fused kernel (dim 2048, or 128 keys).  The models here are random-init two-layer LMs at real fusion widths, so those branches really run:

    case    LM     dim   heads   images  batch        pins
    G1      GPT-2  1280  8 x 64  1       1, 7, 32     resident cached-K/V forward; decode FFW, 4 K slices (ffi 5120); M = 1 / 7 / 32
    G2      GPT-2  1280  8 x 64  2       5            general fused kernel with cached K/V (128 keys); no-image row, tag on the last prompt token
    O1      OPT    2048  8 x 64  1       16           general fused kernel (dim > 1536); decode FFW at its dim limit (ffi 8192, 4 slices)
    C1      GPT-2  1280  8 x 64  1       33           control: M > 32, the decode kernels are off, the training GEMMs run

Per-step logits are recorded on the device inside the session (_Recorder: an index_copy_ next to the session's own token write, so it is
captured into the graph and runs under replay) and compared with a teacher-forced UNCACHED float64 forward of the same bf16 weights on the
host (tests/oracle_backend.py for the fused entry points, stock PyTorch for the LM).  The CPU test at the end shows that this harness lines
positions up exactly before it is trusted on the GPU."""
import contextlib
import os

import numpy as np
import pytest
import torch

from util import TOL_FULL_BF16, rel_rows

BF16 = torch.bfloat16
DV = 256            # dim_visual (CLIP is never run: visual features are handed over directly)
NV = 64             # latents per image = keys per image
L0 = 10             # prompt length
MAXLEN = L0 + 13    # the prompt step and 12 decode steps
VOCAB = 320
ALPHA_ATTN, ALPHA_FFW = 0.625, -0.375      # non-zero gates (bf16-exact): fresh blocks have alpha = 0 and the cross-attention would add nothing

# Tolerances, relative L2 error of the worst (sample, position) logit row / block-output row, set from the errors measured on an MI355X
# (FF_TOL_REPORT=<file> pytest tests/test_hip_decode.py -m gpu; tools/tol_report.py) with the project's 1.3-2x margin:
#   TOL_LOGITS_F64      check 1, recorded bf16 decode logits vs the float64 teacher-forced forward.  The stock LM runs in bf16 too, so
#                       this is the whole-model class (util.TOL_FULL_BF16): measured worst row 7.8e-3 (G2), 6.5e-3 .. 7.6e-3 elsewhere.
#   TOL_LOGITS_UNCACHED check 3, recorded logits vs the same bf16 model's uncached GPU forward (training GEMMs, no cache): only the cached
#                       path's own rounding differs.  Measured worst row 7.3e-3 (G1 b7).
#   TOL_BLOCK           check 4, one gated block's decode-step output vs the oracle on exactly the recorded inputs: measured 3.3e-3.
#   TOL_LOGPROB         check 8, |per-token log-probability| difference of the uncached bf16 GPU forward from float64: measured 3.4e-2.
# Closing every gate changes each generated logit row by >= 0.74 relative (the vacuity guard asks for > 5 x TOL_LOGITS_F64).
TOL_LOGITS_F64 = TOL_FULL_BF16["out"]
TOL_LOGITS_UNCACHED = 1.1e-2
TOL_BLOCK = 5e-3
TOL_LOGPROB = 5e-2

CASES = {   # name: (LM family, batch, images per sample)
    "G1-b1": ("gpt2", 1, 1), "G1-b7": ("gpt2", 7, 1), "G1-b32": ("gpt2", 32, 1),
    "G2-b5": ("gpt2", 5, 2), "O1-b16": ("opt", 16, 1), "C1-b33": ("gpt2", 33, 1),
}
LM = {
    "gpt2": dict(lm="gpt2-decode", dim=1280, lm_kw=dict(n_embd=1280, n_layer=2, n_head=20, vocab_size=VOCAB, n_positions=64,
                                                        resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)),
    "opt": dict(lm="facebook/opt-decode", dim=2048, lm_kw=dict(hidden_size=2048, num_hidden_layers=2, num_attention_heads=32, ffn_dim=8192,
                                                               word_embed_proj_dim=2048, do_layer_norm_before=True, vocab_size=VOCAB,
                                                               max_position_embeddings=64, dropout=0.0)),
}


def _report(label, v):
    """measured error next to the test id (tools/tol_report.py), and on stdout"""
    print(f"MEASURED {label} {v:.3e}")
    if os.environ.get("FF_TOL_REPORT"):
        with open(os.environ["FF_TOL_REPORT"], "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}[{label}]\t{v:.3e}\n")


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-step logit recorder of the decode session (test side: the product code has no hook for it)
# ---------------------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Wraps _DecodeSession._append / .run.  Every _append also copies the logits it chooses from into `session._rec[:, pos]` - a device
    op on a buffer allocated on the eager prompt step, so a captured decode step records under replay as well.  `on_prompt(session)` runs
    once per run() at the prompt step's _append, i.e. after the session loaded K/V, text_time and the buffers and before any decode step
    (the tests use it to plant stale state)."""

    def __init__(self):
        self.session = None
        self.on_prompt = None

    @contextlib.contextmanager
    def installed(self):
        from flamingo_mini_amd import modeling_flamingo as MF
        S = MF._DecodeSession
        orig_append, orig_run = S._append, S.run
        rec = self

        def _append(sess, logits):
            if getattr(sess, "_rec_prompt", False):
                sess._rec_prompt = False
                if getattr(sess, "_rec", None) is None:
                    dt = torch.float64 if logits.dtype == torch.float64 else torch.float32
                    sess._rec = torch.full((sess.b, sess.max_length, logits.shape[-1]), float("nan"), dtype=dt, device=logits.device)
                if rec.on_prompt is not None:
                    rec.on_prompt(sess)
            sess._rec.index_copy_(1, sess.pos, logits[:, None].to(sess._rec.dtype))
            orig_append(sess, logits)

        def run(sess, *a, **k):
            rec.session = sess
            if getattr(sess, "_rec", None) is not None:
                sess._rec.fill_(float("nan"))
            sess._rec_prompt = True
            return orig_run(sess, *a, **k)

        S._append, S.run = _append, run
        try:
            yield self
        finally:
            S._append, S.run = orig_append, orig_run

    def logits(self):
        return self.session._rec.clone()


def decode(model, rec, ids, ml, am, vf, graph=True, eos=None, max_length=MAXLEN):
    """greedy_generate through the static session with the recorder installed: (tokens, recorded logits (b, max_length, V))"""
    model.decode_graph = graph
    with rec.installed():
        if ids.is_cuda:
            out = model.greedy_generate(ids, ml, am, visual_features=vf, max_length=max_length, eos_token_id=eos)
        else:
            out = model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=max_length, eos_token_id=eos,
                                 static_decode=True)
    if ids.is_cuda:
        assert (rec.session.replay is not None) == graph and not rec.session.capture_failed
    return out, rec.logits()


def extend(ml, am, L):
    n = L - ml.shape[1]
    return torch.cat([ml, torch.zeros_like(ml[:, :1]).expand(-1, n)], 1), torch.cat([am, torch.ones_like(am[:, :1]).expand(-1, n)], 1)


def teacher_forced_f64(model64, seq, ml, am, vf):
    """uncached float64 forward on the host over the whole sequence (fused entry points on the numpy oracle): logits (b, L, V)"""
    import oracle_backend
    mlf, amf = extend(ml.cpu(), am.cpu(), seq.shape[1])
    oracle_backend.install()
    try:
        with torch.no_grad():
            return model64(input_ids=seq.cpu(), attention_mask=amf, media_locations=mlf, visual_features=vf.cpu().double()).logits
    finally:
        oracle_backend.uninstall()


def generated(logits_seq, rec, L0_):
    """(the teacher-forced logits that predict positions L0 .. L-1, the recorded ones at those positions)"""
    L = rec.shape[1]
    return logits_seq[:, L0_ - 1:L - 1], rec[:, L0_:L]


def chosen_consistent(seq, ref, got, L0_):
    """check 2: every chosen token is the argmax of its recorded row, and within twice that row's measured max-abs logit error of the
    reference's maximum (a token written at the wrong position or taken from the wrong row fails this)"""
    ch = seq[:, L0_:].cpu()
    got64, ref64 = got.double().cpu(), ref.double().cpu()
    assert torch.equal(got64.argmax(-1), ch), "a recorded row's argmax is not the token at its position"
    err = (got64 - ref64).abs().amax(-1)
    slack = ref64.amax(-1) - ref64.gather(-1, ch[..., None])[..., 0] - 2 * err
    bad = (slack > 1e-9 * ref64.abs().amax(-1)).nonzero().tolist()
    assert not bad, f"(sample, step) rows whose chosen token is not near the reference maximum: {bad[:8]}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# models and inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def build_models(family):
    """(bf16 model on the GPU, float64 copy on the host): the same bf16-representable weights (detgen.det_state), gates opened"""
    import copy
    from detgen import det_state
    from flamingo_mini_amd import FlamingoConfig, FlamingoModel
    spec = LM[family]
    cfg = FlamingoConfig(lm=spec["lm"], clip_model_type="openai/clip-vit-tiny", dim=spec["dim"], dim_visual=DV, xattn_every=1,
                         xattn_dim_head=64, xattn_heads=8, xattn_ff_mult=4, xattn_act="gelu", resampler_depth=1, resampler_dim_head=32,
                         resampler_heads=2, resampler_num_latents=NV, resampler_num_time_embeds=2, resampler_ff_mult=1,
                         random_init_backbones=True,
                         backbone_overrides={"lm": spec["lm_kw"], "clip": dict(hidden_size=DV, num_hidden_layers=1, num_attention_heads=4,
                                                                                intermediate_size=2 * DV, patch_size=16, image_size=32)})
    model = FlamingoModel(cfg)
    sd = {k: torch.from_numpy(det_state(k, v.shape, tag="decode")) for k, v in model.state_dict().items()}
    emb = model.flamingo.lm.get_input_embeddings().weight
    for k, v in model.state_dict().items():        # the tied lm_head holds the token embedding's values
        if v.data_ptr() == emb.data_ptr():
            sd[k] = sd["flamingo.lm." + ("wte.weight" if family == "gpt2" else "decoder.embed_tokens.weight")]
    for k in sd:
        if k.endswith("alpha_attn"):
            sd[k] = torch.tensor([ALPHA_ATTN])
        elif k.endswith("alpha_ffw"):
            sd[k] = torch.tensor([ALPHA_FFW])
    model.load_state_dict(sd)
    assert torch.equal(model.flamingo.lm_head.weight, emb)
    model.eval()
    model64 = copy.deepcopy(model).double()
    return model.to(device="cuda", dtype=BF16), model64


_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _MODELS.clear()


def models(family):
    if family not in _MODELS:
        _MODELS.clear()                      # one family at a time (the OPT pair holds ~2 GB on the host)
        _MODELS[family] = build_models(family)
    return _MODELS[family]


def make_inputs(b, T, tag, L0_=L0, device="cuda"):
    """prompt ids / media_locations / attention_mask / visual features.  T = 1: every sample has one tag except sample 3 (text_time 0 for
    every generated token); sample 5 is left-padded.  T = 2: sample 0 has no tag, sample 1's second tag is the last prompt token, sample 2
    is left-padded."""
    from detgen import bf16_round, det
    g = np.random.default_rng(sum(map(ord, tag)) * 7919 + b)
    ids = torch.from_numpy(g.integers(1, VOCAB - 20, (b, L0_)))
    ml = torch.zeros((b, L0_), dtype=torch.long)
    am = torch.ones((b, L0_), dtype=torch.long)
    for i in range(b):
        if T == 1:
            if i != 3:
                ml[i, (2 * i + len(tag)) % (L0_ - 1)] = 1
        else:
            if i == 1:
                ml[i, [1, L0_ - 1]] = 1
            elif i != 0:
                a = int(g.integers(0, L0_ // 2))
                ml[i, [a, a + 2 + int(g.integers(0, L0_ // 2 - 1))]] = 1
    pad = 5 if T == 1 else 2
    if b > pad:
        am[pad, :3] = 0
        ml[pad] = 0
        ml[pad, [4] if T == 1 else [3, 6]] = 1
    vf = torch.from_numpy(bf16_round(det((b, T, NV, DV), tag + "-vf")))
    return ids.to(device), ml.to(device), am.to(device), vf.to(device=device, dtype=BF16)


def decode_step_records(model, ids, ml, am, vf):
    """launch log (ff_gemm_profile_*) of ONE eager cached decode step after a prompt step: [(tile, split_k, b_layout)] of the fused /
    decode launches (tile <= -4)"""
    from flamingo_mini_amd import ffi
    lib = ffi.lib()
    with torch.no_grad():
        o = model.flamingo(input_ids=ids, attention_mask=am, media_locations=ml, visual_features=vf, use_cache=True)
        nxt = o.logits[:, -1].argmax(-1, keepdim=True)
        ml2, am2 = extend(ml, am, ids.shape[1] + 1)
        torch.cuda.synchronize()
        lib.ff_gemm_profile_enable(512)
        try:
            model.flamingo(input_ids=nxt, attention_mask=am2, media_locations=ml2, past_key_values=o.past_key_values, use_cache=True)
            torch.cuda.synchronize()
            recs = (ffi.GemmProfileRecord * 512)()
            n = lib.ff_gemm_profile_read(recs, 512)
        finally:
            lib.ff_gemm_profile_enable(0)
    return [(recs[i].tile, recs[i].split_k, recs[i].b_layout) for i in range(n) if recs[i].tile <= -4]


@contextlib.contextmanager
def gates(model, attn=None, ffw=None, blocks=None):
    """temporarily set the gates of the model's cross-attention blocks (in place: the parameters keep their addresses)"""
    hooks = model.flamingo.get_modified_layers()
    chosen = [h.xattn_block for i, h in enumerate(hooks) if blocks is None or i in blocks]
    saved = [(b.alpha_attn.detach().clone(), b.alpha_ffw.detach().clone()) for b in chosen]
    try:
        with torch.no_grad():
            for b in chosen:
                if attn is not None:
                    b.alpha_attn.fill_(attn)
                if ffw is not None:
                    b.alpha_ffw.fill_(ffw)
        yield
    finally:
        with torch.no_grad():
            for b, (a, f) in zip(chosen, saved):
                b.alpha_attn.copy_(a)
                b.alpha_ffw.copy_(f)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_cached_decode_logits_vs_f64_reference(case):
    """Checks 1, 2, 3 and 5 plus the launch log and the vacuity guard, for one geometry."""
    family, b, T = CASES[case]
    model, model64 = models(family)
    ids, ml, am, vf = make_inputs(b, T, case)

    # the branches this case exists for really run (one eager cached decode step; two gated blocks)
    recs = decode_step_records(model, ids, ml, am, vf)
    up = [r for r in recs if r[0] == -10]
    down = [r for r in recs if r[0] == -11]
    fwd = [r for r in recs if r[0] in (-4, -6, -8)]
    assert len(fwd) == 2, recs
    if case.startswith("C1"):
        assert not up and not down, recs                             # M = 33 > 32: the training GEMMs
    else:
        assert len(up) == 2 and len(down) == 2 and all(r[1] == 4 for r in down), recs        # ffi 5120 / 8192: four K slices
        assert all(r[0] == -4 for r in fwd), recs
        if case.startswith("G1"):
            assert all(r[2] > 0 for r in fwd), recs                  # resident-operand kernel (ring depth)
        else:
            assert all(r[2] == 0 for r in fwd), recs                 # general fused kernel: 128 keys (G2) / dim 2048 (O1)

    rec = _Recorder()
    model.reset_decode_sessions()
    seq, logits = decode(model, rec, ids, ml, am, vf, graph=True)
    assert seq.shape == (b, MAXLEN) and torch.equal(seq[:, :L0], ids)
    assert torch.isfinite(logits[:, L0:]).all()

    # check 5: graph replay == eager steps, bitwise (the kernels are deterministic)
    seq_e, logits_e = decode(model, rec, ids, ml, am, vf, graph=False)
    assert torch.equal(seq_e, seq) and torch.equal(logits_e[:, L0:], logits[:, L0:]), "HIP-graph replay differs from the eager decode steps"

    # check 1: every generated position of every row against the float64 teacher-forced forward
    ref64 = teacher_forced_f64(model64, seq, ml, am, vf)
    ref, got = generated(ref64, logits.cpu(), L0)
    worst, where = rel_rows(got, ref, (0, 1))
    _report("f64", worst)
    # check 2: chosen tokens consistent with the reference
    chosen_consistent(seq, ref, got, L0)
    # check 3: the same bf16 model's UNCACHED forward on the GPU (isolates the cached path from the LM's bf16 rounding)
    mlf, amf = extend(ml, am, MAXLEN)
    with torch.no_grad():
        unc = model(input_ids=seq, attention_mask=amf, media_locations=mlf, visual_features=vf).logits
    worst_u, where_u = rel_rows(got, unc[:, L0 - 1:MAXLEN - 1].float().cpu(), (0, 1))
    _report("uncached", worst_u)
    # vacuity guard: closing every gate changes the reference's logits by far more than the tolerance, in every row
    with gates(model64, 0.0, 0.0):
        ref0 = generated(teacher_forced_f64(model64, seq, ml, am, vf), logits, L0)[0]
    change = ((ref0 - ref).norm(dim=-1) / ref.norm(dim=-1)).min().item()
    _report("gates-closed-change(min row)", change)
    assert worst < TOL_LOGITS_F64, f"{case}: worst (sample, step) {where}: {worst:.3e} vs float64"
    assert worst_u < TOL_LOGITS_UNCACHED, f"{case}: worst (sample, step) {where_u}: {worst_u:.3e} vs the uncached bf16 forward"
    assert change > 5 * TOL_LOGITS_F64, f"{case}: closing the gates changes a logit row by only {change:.3e}: the check would be vacuous"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["G1-b7", "G2-b5", "O1-b16"])
def test_decode_block_outputs_vs_oracle(case):
    """Check 4: every gated block of every decode step of an eager session against the oracle's cached-K/V forward on exactly the inputs
    the block saw (y, the cached (k, v), text_time).  With alpha_ffw = 0 on one block, rows whose text_time is 0 leave it bit-identical."""
    from oracle import flamingo_oracle as O
    family, b, T = CASES[case]
    model, _ = models(family)
    ids, ml, am, vf = make_inputs(b, T, case)
    blocks = [h.xattn_block for h in model.flamingo.get_modified_layers()]
    seen = {i: [] for i in range(len(blocks))}

    def hook(i):
        def fn(mod, args, kwargs, output):
            if kwargs.get("previous_kv") is not None:
                k, v = kwargs["previous_kv"]
                seen[i].append(dict(y=kwargs["y"].detach().clone(), k=k.detach().clone(), v=v.detach().clone(),
                                    tt=kwargs["text_time"].detach().clone(), out=output[0].detach().clone()))
        return fn

    handles = [blk.register_forward_hook(hook(i), with_kwargs=True) for i, blk in enumerate(blocks)]
    rec = _Recorder()
    try:
        model.reset_decode_sessions()
        decode(model, rec, ids, ml, am, vf, graph=False)
        steps = MAXLEN - L0 - 1
        assert all(len(s) == steps for s in seen.values()), {i: len(s) for i, s in seen.items()}
        tt_want = ml.cumsum(-1)[:, -1:].int()
        worst = 0.0
        for i, blk in enumerate(blocks):
            p64 = {k: v.double().cpu().numpy() for k, v in blk.state_dict().items()}
            heads, dh, _, act = blk.cfg
            for s, r in enumerate(seen[i]):
                assert torch.equal(r["tt"].int(), tt_want), "decode step's text_time is not the prompt's last value"
                f = lambda t: t.double().cpu().numpy()
                ref, _, _ = O.gated_xattn_block_fwd(f(r["y"]), None, r["tt"].long().cpu().numpy(), p64, heads=heads, dim_head=dh, act=act,
                                                    n_visual=NV, previous_kv=(f(r["k"]), f(r["v"])))
                err, where = rel_rows(r["out"], ref, (0, 1))
                worst = max(worst, err)
                assert err < TOL_BLOCK, f"{case}: block {i}, decode step {s}, sample {where[0]}: {err:.3e}"
        _report("block", worst)

        # alpha_ffw = 0 on the last block: rows without media (text_time 0) come out bit-identical to their input
        last = len(blocks) - 1
        for s in seen.values():
            s.clear()
        with gates(model, ffw=0.0, blocks=[last]):
            decode(model, rec, ids, ml, am, vf, graph=False)
        no_media = (tt_want[:, 0] == 0).nonzero()[:, 0]
        assert no_media.numel() > 0
        for r in seen[last]:
            assert torch.equal(r["out"][no_media], r["y"][no_media]), "a closed feed-forward gate and no media did not leave the rows unchanged"
    finally:
        for h in handles:
            h.remove()


@pytest.mark.gpu
def test_decode_session_reuse_equals_fresh_session():
    """Check 6: a second prompt through the SAME session (same key; another prompt length, other media positions, other visual features)
    equals, bitwise, the same prompt through a fresh session.  Stale K/V or a stale text_time planted after the prompt step must break
    that equality - the check sees the state a reused session carries over."""
    model, _ = models("gpt2")
    b = 7
    A = make_inputs(b, 1, "reuse-A")
    ids, ml, am, vf = make_inputs(b, 1, "reuse-B", L0_=L0 - 2)
    ml = ml.clone(); ml[3, 1] = 1; ml[1] = 0             # the no-image sample moves: text_time of samples 1 and 3 differs from prompt A
    assert not torch.equal(ml.cumsum(-1)[:, -1], A[1].cumsum(-1)[:, -1])
    rec = _Recorder()
    model.reset_decode_sessions()
    decode(model, rec, *A)
    reused, lg_reused = decode(model, rec, ids, ml, am, vf)
    assert len(model._decode_sessions) == 1
    model.reset_decode_sessions()
    fresh, lg_fresh = decode(model, rec, ids, ml, am, vf)
    assert torch.equal(reused, fresh) and torch.equal(lg_reused[:, L0 - 2:], lg_fresh[:, L0 - 2:]), "a reused session differs from a fresh one"

    def plant(what):
        def fn(sess):
            if what == "kv":
                for (kb, vb), (k, v) in zip(sess.xattn_past, state["kv"]):
                    kb.copy_(k); vb.copy_(v)
            else:
                sess.tt_step.copy_(state["tt"])
        return fn

    for what in ("kv", "tt"):
        model.reset_decode_sessions()
        decode(model, rec, *A)
        sess = rec.session
        state = dict(kv=[(k.clone(), v.clone()) for k, v in sess.xattn_past], tt=sess.tt_step.clone())
        rec.on_prompt = plant(what)
        try:
            stale, lg_stale = decode(model, rec, ids, ml, am, vf)
        finally:
            rec.on_prompt = None
        assert not torch.equal(lg_stale[:, L0 - 2:], lg_fresh[:, L0 - 2:]), f"stale {what} of the previous prompt went unnoticed"


@pytest.mark.gpu
def test_decode_eos_under_replay():
    """Check 7: an eos some samples emit mid-way.  The graph session and the eager session agree bitwise on tokens and trimmed length, both
    equal the un-stopped decode cut at each sample's first eos (pad = eos after it), and the recorded logits up to each sample's stop are
    the bits of the un-stopped run (which check 1 holds to float64)."""
    model, _ = models("gpt2")
    ids, ml, am, vf = make_inputs(7, 1, "G1-b7")
    rec = _Recorder()
    model.reset_decode_sessions()
    full, lg_full = decode(model, rec, ids, ml, am, vf)
    gen = full[:, L0:]
    cands = [int(t) for t in gen[:, 3:9].flatten().unique() if not bool((gen[:, 0] == t).any())]
    counts = {t: int((gen == t).any(1).sum()) for t in cands}
    eos = max(cands, key=lambda t: (0 < counts[t] < gen.shape[0], counts[t]))          # emitted by some samples, mid-way
    assert 0 < counts[eos] < gen.shape[0]
    stop = [int((gen[i] == eos).nonzero()[0, 0]) + L0 if bool((gen[i] == eos).any()) else MAXLEN - 1 for i in range(gen.shape[0])]
    want = full.clone()
    for i, s in enumerate(stop):
        want[i, s + 1:] = eos
    want = want[:, :max(stop) + 1]
    got_g, lg_g = decode(model, rec, ids, ml, am, vf, graph=True, eos=eos)
    got_e, lg_e = decode(model, rec, ids, ml, am, vf, graph=False, eos=eos)
    assert got_g.shape == got_e.shape == want.shape and torch.equal(got_g, got_e) and torch.equal(got_g, want), (eos, got_g, want)
    for i, s in enumerate(stop):
        assert torch.equal(lg_g[i, L0:s + 1], lg_full[i, L0:s + 1]) and torch.equal(lg_e[i, L0:s + 1], lg_full[i, L0:s + 1])


@pytest.mark.gpu
def test_beam_search_on_gpu():
    """Check 8 (G1 geometry, batch 4, 3 beams: 12 rows through the decode kernels).  _reorder_cache gathers the cross-attention K/V rows
    (and the LM cache) by beam_idx, bitwise; the returned beams' float64 teacher-forced log-probability is at least greedy's."""
    model, model64 = models("gpt2")
    ids, ml, am, vf = make_inputs(4, 1, "beam")
    with torch.no_grad():
        o = model.flamingo(input_ids=ids, attention_mask=am, media_locations=ml, visual_features=vf, use_cache=True)
    xa, lm = o.past_key_values
    before = [(k.clone(), v.clone()) for k, v in xa]
    lm_before = [(l.keys.clone(), l.values.clone()) for l in lm.layers]
    beam_idx = torch.tensor([2, 0, 3, 1], device="cuda")
    xa_new, lm_new = model._reorder_cache((xa, lm), beam_idx)
    for (k, v), (k0, v0) in zip(xa_new, before):
        assert torch.equal(k, k0[beam_idx]) and torch.equal(v, v0[beam_idx])
    for l, (k0, v0) in zip(lm_new.layers, lm_before):
        assert torch.equal(l.keys, k0[beam_idx]) and torch.equal(l.values, v0[beam_idx])

    greedy = model.greedy_generate(ids, ml, am, visual_features=vf, max_length=MAXLEN)
    beams = model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=MAXLEN, num_beams=3)
    assert beams.shape == greedy.shape

    def logprobs(seq):      # (per-token log-probabilities of the generated suffix: float64 host, bf16 uncached GPU)
        lp64 = teacher_forced_f64(model64, seq, ml, am, vf).log_softmax(-1)[:, L0 - 1:-1].gather(-1, seq[:, L0:, None].cpu())[..., 0]
        mlf, amf = extend(ml, am, seq.shape[1])
        with torch.no_grad():
            lg = model(input_ids=seq, attention_mask=amf, media_locations=mlf, visual_features=vf).logits.float().log_softmax(-1)
        return lp64, lg[:, L0 - 1:-1].gather(-1, seq[:, L0:, None])[..., 0].double().cpu()

    lb64, lbg = logprobs(beams)
    lg64, lgg = logprobs(greedy)
    tok_err = max(float((lb64 - lbg).abs().max()), float((lg64 - lgg).abs().max()))
    _report("logprob-token", tok_err)
    assert tok_err < TOL_LOGPROB
    margin = float((lb64.sum(1) - lg64.sum(1)).min())
    _report("beam-minus-greedy(min)", margin)
    # beam search ranks by bf16 log-probabilities: it may lose to greedy in float64 by at most the two sequences' summed rounding
    slack = ((lb64 - lbg).abs().sum(1) + (lg64 - lgg).abs().sum(1))
    assert bool((lb64.sum(1) >= lg64.sum(1) - slack).all()), (lb64.sum(1), lg64.sum(1), slack)


FALLBACKS = {   # calls the static path cannot serve: more beams than ff_beam_step has, or a prompt within one token of max_length
    "beams-9": dict(num_beams=9, static_decode=True, max_length=10),
    "beams-3-short": dict(num_beams=3, static_decode=True, max_length=5),
    "sample-short": dict(do_sample=True, static_decode=True, max_length=5),
    "greedy-short": dict(max_length=5),
}


@pytest.fixture(scope="module", params=["gpt2", "opt"])
def tiny_on_gpu(request):
    from test_model_plumbing import build
    model, z = build(torch.float32, "cuda", request.param)
    model.eval()
    ids, ml = torch.from_numpy(z["ids"])[:, :4].cuda(), torch.from_numpy(z["ml"])[:, :4].cuda()
    return model, ids, dict(media_locations=ml, attention_mask=torch.ones_like(ids), pixel_values=torch.from_numpy(z["px"]).float().cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FALLBACKS))
def test_static_requests_the_sessions_cannot_serve_run_the_dynamic_path(tiny_on_gpu, case):
    """The tiny fp32 models on the device, b = 2, L0 = 4: each call returns exactly what the same call with static_decode=False returns
    (the same seed where it samples) and builds no session."""
    model, ids, kw = tiny_on_gpu
    args = FALLBACKS[case]
    assert ids.shape == (2, 4) and len(model._decode_sessions) == 0

    def call(**over):
        g = torch.Generator(device="cuda").manual_seed(1234) if args.get("do_sample") else None
        return model.generate(ids, **kw, **dict(args, **over), generator=g)

    got, want = call(), call(static_decode=False)
    assert got.shape == want.shape and torch.equal(got, want), (got.tolist(), want.tolist())
    assert got.shape[0] == 2 and 4 < got.shape[1] <= args["max_length"]
    assert len(model._decode_sessions) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the harness itself
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["opt", "gpt2"])
def test_recorder_and_teacher_forcing_line_up_on_cpu(family):
    """The recorder + teacher-forced reference, on the tiny fixtures with the fused entry points on the float64 oracle: the session's tokens
    are the existing CPU generate's, and every recorded logit row equals the float64 teacher-forced row it is compared with to ~1e-12 -
    positions line up exactly (an off-by-one would compare logits of different tokens)."""
    import oracle_backend
    from test_model_plumbing import build
    oracle_backend.install()
    try:
        model, z = build(torch.float64, "cpu", family)
        model.eval()
        vf = model.flamingo.encode_resample_visuals(torch.from_numpy(z["px"]).double()).detach()
        ids, ml = torch.from_numpy(z["ids"])[:, :4], torch.from_numpy(z["ml"])[:, :4]
        am = torch.ones_like(ids)
        am[1, 0] = 0                                                     # a left-padded prompt
        want = model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=10, static_decode=False)
        rec = _Recorder()
        seq, logits = decode(model, rec, ids, ml, am, vf, max_length=10)
    finally:
        oracle_backend.uninstall()
    assert torch.equal(seq, want)
    ref, got = generated(teacher_forced_f64(model, seq, ml, am, vf), logits, 4)
    assert torch.isfinite(got).all()
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12
    chosen_consistent(seq, ref, got, 4)
    # one position off is far outside that
    assert float((logits[:, 5:10] - ref[:, :5]).abs().max() / ref.abs().max()) > 1e-3
