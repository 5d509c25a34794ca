"""Label smoothing and z-loss in the fused shifted cross-entropy (ff_shifted_ce_fwd_reg / ff_shifted_ce_bwd_reg), on the MI355X.

Every element of lse, loss and d logits is held to float64 from what the kernel saw (loss_reg_cases.shifted_ce_reg_ref, reg_bound_ok) at
every (eps, zeta) of loss_reg_cases.GRID over all inputs of loss_cases.ce_cases - the vocabularies from 1 to GPT-2's, rows at every phase
of the 16-byte grid, sorted rows, dominant logits, offsets, -inf columns -, through direct C-ABI calls on buffers that lie between sentinels;
then the properties that do not change (exact zero rows, NaN for a bad label, the plain bits when both values are 0, the same bits on every
run and in a replayed graph), the wrapper through autograd and the model-level route through the config keys."""
import copy

import pytest
import torch

import loss_cases as lc
import loss_reg_cases as lr
from guarded import SENTINEL, guarded_allocations

pytestmark = pytest.mark.gpu
BF16, F32 = lc.BF16, lc.F32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
BITS = {F32: torch.int32, BF16: torch.int16}
PAD = 64                                         # sentinel elements on either side of a body (a multiple of 16 bytes in both dtypes)


class Arena:
    """A device buffer whose body starts `off` elements past the 16-byte grid, PAD or more sentinel elements around it
    (the helper of tests/test_hip_loss_bounds.py)"""

    def __init__(self, shape, dtype, off=0, values=None):
        n = 1
        for s in shape:
            n *= s
        self.flat = torch.empty(n + 2 * PAD + 8, dtype=dtype, device="cuda")
        self.bits = self.flat.view(BITS[dtype])
        self.bits.fill_(SENTINEL[dtype])
        self.lo, self.hi = PAD + off, PAD + off + n
        self.body = self.flat[self.lo:self.hi].view(shape)
        self.body.fill_(float("nan"))                 # an element the kernel never writes reaches the comparison as NaN
        if values is not None:
            self.body.copy_(values)
        assert self.flat.data_ptr() % 16 == 0 and self.body.data_ptr() % 16 == off * self.flat.element_size()

    def intact(self):
        sentinel = SENTINEL[self.flat.dtype]
        return bool((self.bits[:self.lo] == sentinel).all()) and bool((self.bits[self.hi:] == sentinel).all())


class Buffers:
    """the arenas of one input set: logits (and their bits as uploaded), d logits, loss rows, lse; labels and row gradients"""

    def __init__(self, x, lab, g, off=0):
        b, L, V = x.shape
        self.shape, self.dtype = (b, L, V), x.dtype
        self.xa, self.da = Arena(x.shape, x.dtype, off, x), Arena(x.shape, x.dtype, off)
        self.rows, self.lse = Arena((b * (L - 1),), F32), Arena((b * (L - 1),), F32)
        self.labels, self.g = lab.cuda(), g.cuda()
        self.before = self.xa.bits.clone()

    def launch(self, eps, zeta, plain=False, check=True):
        """forward and backward on the current stream; plain=True: ff_shifted_ce_fwd / _bwd.  Returns the two return codes."""
        from flamingo_mini_amd import ffi
        lib, code = ffi.lib(), ffi.dtype_code(self.dtype)
        b, L, V = self.shape
        stream = ffi.stream_handle(self.xa.flat.device)
        head = (code, b, L, V, self.xa.body.data_ptr(), self.labels.data_ptr(), lc.IGNORE)
        if plain:
            rc = (lib.ff_shifted_ce_fwd(*head, self.rows.body.data_ptr(), self.lse.body.data_ptr(), stream),
                  lib.ff_shifted_ce_bwd(*head, self.lse.body.data_ptr(), self.g.data_ptr(), self.da.body.data_ptr(), stream))
        else:
            rc = (lib.ff_shifted_ce_fwd_reg(*head, self.rows.body.data_ptr(), self.lse.body.data_ptr(), eps, zeta, stream),
                  lib.ff_shifted_ce_bwd_reg(*head, self.lse.body.data_ptr(), self.g.data_ptr(), self.da.body.data_ptr(), eps, zeta, stream))
        if check:
            ffi.check(rc[0], "ff_shifted_ce_fwd"), ffi.check(rc[1], "ff_shifted_ce_bwd")
        return rc

    def results(self):
        """(loss, lse, d) on the CPU; nothing around any buffer is written, the logits are not written"""
        torch.cuda.synchronize()
        assert torch.equal(self.xa.bits, self.before), "the logits (or their surroundings) were written"
        assert self.da.intact() and self.rows.intact() and self.lse.intact(), "a write outside an output"
        return self.rows.body.cpu(), self.lse.body.cpu(), self.da.body.cpu()

    def bits(self):
        loss, lse, d = self.results()
        return loss.view(torch.int32), lse.view(torch.int32), d.view(BITS[self.dtype])


def held(name, x, lab, g, eps, zeta, got, worst):
    """(loss, lse or None, d) against the float64 reference by reg_bound_ok; prints and collects every figure, then asserts"""
    ref = lr.shifted_ce_reg_ref(x, lab, g, eps, zeta, lc.IGNORE)
    res = {what: lr.reg_bound_ok(what, t, ref, x.dtype) for what, t in zip(("loss", "lse", "d"), got) if t is not None}
    for what, (ok, w, idx) in res.items():
        print(f"{str(x.dtype).replace('torch.', '')} {name} eps {eps} zeta {zeta} {what}: worst element at {w:.3f} of its bound")
        worst[what] = max(worst.get(what, 0.0), w)
    for what, (ok, w, idx) in res.items():
        where = idx if what != "d" else (idx // (x.shape[1] * x.shape[2]), idx // x.shape[2] % x.shape[1], idx % x.shape[2])
        assert ok, f"{name} eps {eps} zeta {zeta}: {what} element {where} is {w:.4g} x its bound"
    last, ignored = got[2][:, -1], got[2][:, :-1][lab[:, 1:] == lc.IGNORE]
    assert int((last != 0).sum()) == 0 and int((ignored != 0).sum()) == 0 and ignored.numel() > 0
    assert int((got[0][(lab[:, 1:] == lc.IGNORE).reshape(-1)] != 0).sum()) == 0
    return ref


@DTYPES
@pytest.mark.parametrize("group", lc.GROUPS)
def test_every_element_within_its_bound_at_every_eps_and_zeta(dtype, group):
    """shapes: b = 4, L = 5 at every vocabulary of loss_cases.vocabularies (1, 3, 7, 8, 9, ... 4099), the 256-vector-boundary ones also one
    element off the grid, targets in the scalar head, the vector body and the scalar tail;  patterns: sorted rows, one logit 80 above the
    rest, a common offset;  neg-inf: -inf at non-target columns - the loss +inf exactly where eps > 0 and the row holds one, d finite,
    -eps / V g there (inside the bound: the reference has it);  gpt2: V = 50257, 50258 with b = 2."""
    worst, regions = {}, set()
    with guarded_allocations() as gd:
        for name, x, lab, g, off in lc.ce_cases(dtype, (group,)):
            assert x.shape[:2] == ((2, lc.L) if group == "gpt2" else (lc.B, lc.L))
            regions |= lc.target_regions(x.shape[2], dtype, lab, off)
            buf = Buffers(x, lab, g, off)
            for eps, zeta in lr.GRID:
                buf.launch(eps, zeta)
                loss, lse, d = buf.results()
                ref = held(name, x, lab, g, eps, zeta, (loss, lse, d), worst)
                if group == "neg-inf":
                    masked = torch.isinf(x)
                    holds = masked[:, :-1].any(dim=-1).reshape(-1) & (lab[:, 1:] != lc.IGNORE).reshape(-1)
                    assert torch.equal(torch.isposinf(loss), holds if eps > 0 else torch.zeros_like(holds)), (name, eps, loss.tolist())
                    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(lse).all()) and not bool(torch.isnan(loss).any())
                    assert torch.equal(d[masked] != 0, ref["d"][masked] != 0)
                else:
                    assert bool(torch.isfinite(loss).all())
        gd.check()
    if group == "shapes":
        assert regions == {"head", "body", "tail"}, regions
    print(f"worst over {group}: {worst}")


@DTYPES
def test_a_negative_and_a_vanishing_factor_of_the_softmax(dtype):
    """1 + 2 zeta lse, the factor of p in d, is negative where lse < -1 / (2 zeta) and 0 where they are equal - no case of the grid has
    either: logits lowered by 32 (lse about -22) at zeta = 0.5, and zeta = -1 / (2 lse) of the first scored row, as nearly as float32 has it"""
    V = lc.V_SMALL[6]
    x = (lc.logits(V, dtype, seed=8)[0].float() - 32.0).to(dtype)
    lab, g = lc.labels(V, start=2), lc.grad_rows()
    r = int((lab[:, 1:].reshape(-1) != lc.IGNORE).nonzero()[0])
    lse_r = float(lr.shifted_ce_reg_ref(x, lab, g, 0.0, 0.0)["lse"][r])
    assert lse_r < -15
    worst = {}
    for eps, zeta in ((0.1, 0.5), (0.0, -0.5 / lse_r)):
        buf = Buffers(x, lab, g)
        buf.launch(eps, zeta)
        ref = held(f"V={V} - 32", x, lab, g, eps, zeta, buf.results(), worst)
        factor = 1.0 + 2.0 * lr.as_launched(eps, zeta)[1] * ref["lse"]
        assert bool((factor < 0).all()) if zeta == 0.5 else abs(float(factor[r])) < 1e-6


@DTYPES
def test_both_values_0_give_the_bits_of_the_plain_entry_points(dtype):
    for name, x, lab, g, off in lc.ce_cases(dtype, ("shapes",)):
        buf = Buffers(x, lab, g, off)
        buf.launch(0.0, 0.0, plain=True)
        plain = buf.bits()
        buf = Buffers(x, lab, g, off)
        buf.launch(0.0, 0.0)
        for a, b in zip(plain, buf.bits()):
            assert torch.equal(a, b), name


@DTYPES
def test_a_bad_label_is_nan_and_a_bad_value_an_error_code_that_writes_nothing(dtype):
    V = lc.V_PATTERN[dtype][1]
    x, _ = lc.logits(V, dtype)
    lab, g = lc.labels(V, start=2), lc.grad_rows()
    good = Buffers(x, lab, g)
    good.launch(0.1, 1e-4)
    base = good.bits()
    bad_lab = lab.clone()
    s, i = 1, 2
    assert int(lab[s, i + 1]) != lc.IGNORE
    for value in (V, -1, 2 ** 40):
        bad_lab[s, i + 1] = value
        buf = Buffers(x, bad_lab, g)
        buf.launch(0.1, 1e-4)
        loss, lse, d = buf.results()
        r = s * (lc.L - 1) + i
        assert bool(torch.isnan(loss[r])) and int(torch.isnan(loss).sum()) == 1 and bool(torch.isfinite(lse).all()), value
        assert bool(torch.isnan(d[s, i]).all()) and int(torch.isnan(d).sum()) == V, value
        keep = torch.ones(x.shape[:2], dtype=torch.bool)
        keep[s, i] = False
        assert torch.equal(buf.bits()[2].view(x.shape)[keep], base[2].view(x.shape)[keep]), value
    for eps, zeta in ((-0.5, 0.0), (1.0001, 0.0), (float("nan"), 0.0), (0.1, -1e-6), (0.1, float("inf")), (0.1, float("nan"))):
        buf = Buffers(x, lab, g)
        untouched = [a.bits.clone() for a in (buf.da, buf.rows, buf.lse)]
        assert buf.launch(eps, zeta, check=False) == (-2, -2), (eps, zeta)
        torch.cuda.synchronize()
        assert all(torch.equal(a.bits, u) for a, u in zip((buf.da, buf.rows, buf.lse), untouched)) and torch.equal(buf.xa.bits, buf.before)


@DTYPES
def test_two_runs_give_the_same_bits(dtype):
    for V in lc.V_GPT2[1:] + [lc.V_BOUNDARY[dtype][3]]:
        b = 2 if V > lc.V_LARGE else lc.B
        x, lab, g = lc.logits(V, dtype, b=b, seed=6)[0], lc.labels(V, b=b, start=5), lc.grad_rows(b=b)
        buf = Buffers(x, lab, g, 1)
        buf.launch(0.1, 1e-4)
        first = buf.bits()
        buf.da.body.fill_(float("nan")), buf.rows.body.fill_(float("nan")), buf.lse.body.fill_(float("nan"))
        buf.launch(0.1, 1e-4)
        for a, c in zip(first, buf.bits()):
            assert torch.equal(a, c), V


@DTYPES
def test_a_captured_forward_and_backward_replays_to_the_eager_bits(dtype):
    """one torch.cuda.graph capture of the two launches (one stream, no branches), replayed on two further sets of logits"""
    V = lc.V_BOUNDARY[dtype][3]
    lab, g = lc.labels(V, start=7), lc.grad_rows()
    xs = [lc.logits(V, dtype, seed=20 + k)[0] for k in range(3)]
    eager = []
    for x in xs:
        buf = Buffers(x, lab, g, 1)
        buf.launch(0.1, 1e-4)
        eager.append(buf.bits())
    buf = Buffers(xs[0], lab, g, 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.launch(0.1, 1e-4)
    for k in (1, 2):
        buf.xa.body.copy_(xs[k])
        buf.before = buf.xa.bits.clone()
        for a in (buf.da, buf.rows, buf.lse):
            a.body.fill_(float("nan"))
        graph.replay()
        for a, c in zip(eager[k], buf.bits()):
            assert torch.equal(a, c), k
    assert not torch.equal(eager[1][0], eager[2][0])


@DTYPES
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off-grid"])
def test_the_wrapper_matches_the_reference_through_autograd(dtype, off):
    """functional.shifted_cross_entropy(label_smoothing=, z_loss=) under all three reductions; off-grid: the logits are a contiguous view one
    element off the 16-byte grid.  reduction='none': every element by reg_bound_ok.  'sum' / 'mean': d logits by the same bound with the
    row gradient 1 or 1 / count, the scalar within the sum of its rows' bounds plus the float32 summation of n rows, n 2^-24 sum |row|."""
    from flamingo_mini_amd import functional as F
    eps, zeta = 0.1, 1e-4
    worst = {}
    for V in (lc.V_SMALL[4], lc.V_BOUNDARY[dtype][2], lc.V_LARGE):
        x, _ = lc.logits(V, dtype, seed=4)
        lab = lc.labels(V, start=6)
        count = int((lab[:, 1:] != lc.IGNORE).sum())
        n = lab.shape[0] * (lab.shape[1] - 1)
        for reduction in ("none", "sum", "mean"):
            g = {"none": lc.grad_rows(), "sum": torch.ones(n), "mean": torch.full((n,), 1.0 / count).float()}[reduction]
            flat = torch.empty(x.numel() + 16, dtype=dtype, device="cuda")
            logits = flat[off:off + x.numel()].view(x.shape)
            logits.copy_(x)
            assert logits.is_contiguous() and logits.data_ptr() % 16 == off * x.element_size()
            logits.requires_grad_(True)
            with guarded_allocations() as gd:
                out = F.shifted_cross_entropy(logits, lab.cuda(), reduction=reduction, label_smoothing=eps, z_loss=zeta)
                ((out * g.cuda()).sum() if reduction == "none" else out).backward()
                gd.check()
            if reduction == "none":
                held(f"wrapper V={V}", x, lab, g, eps, zeta, (out.detach().cpu(), None, logits.grad.cpu()), worst)
            else:
                ref = lr.shifted_ce_reg_ref(x, lab, g, eps, zeta, lc.IGNORE)
                ok, w, idx = lr.reg_bound_ok("d", logits.grad.cpu(), ref, dtype)
                assert ok, f"V={V} {reduction}: d element {idx} is {w:.4g} x its bound"
                unit = lr.shifted_ce_reg_ref(x, lab, torch.ones(n), eps, zeta, lc.IGNORE)
                scale = 1.0 if reduction == "sum" else 1.0 / count
                want = float(unit["loss"].sum()) * scale
                bound = (lr.CE_REG_C_F * 2.0 ** -24 * float(unit["t_loss"].sum()) + (n + 1) * 2.0 ** -24 * float(unit["loss"].abs().sum())) * scale
                print(f"wrapper V={V} {reduction}: loss {float(out):.8g} reference {want:.8g} bound {bound:.3g}")
                assert abs(float(out) - want) <= bound, (V, reduction, float(out), want, bound)
            assert torch.equal(logits.detach().cpu().view(BITS[dtype]), x.view(BITS[dtype]))


def stock_attention_pinned():
    """The frozen GPT-2's attention pinned to torch's MATH scaled-dot-product backend, for BOTH arms of the two tests below.  The backend
    torch picks by itself for these float32 shapes, memory-efficient attention, gives the model other bits in a captured graph than in eager
    launches - with the plain loss on the commit before this feature just as with the keys set: all 39 trainable gradients differ by a few
    ulp from the first LM block's attention output on, found by comparing every module's output and incoming gradient between an eager run
    and a replay; under the MATH backend the loss and all 39 gradients are bit-equal.  The arms compare eager launches with a replay of
    the library's kernels and of the route from the config keys to them; a stock kernel that is not reproducible across the two would hide
    exactly that.  (Measured on the MI355X, 2026-10-20.)"""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    return sdpa_kernel(SDPBackend.MATH)


def _h64_arms(eps, zeta):
    """the h64 fixture model (float32) with the two config keys set, a deep copy of it, the batch, and a copy without the keys"""
    from test_model_plumbing import build_h64
    base, z, batch = build_h64(torch.float32, "cuda")
    plain = copy.deepcopy(base)
    base.config.label_smoothing, base.config.z_loss = eps, zeta
    assert base.flamingo.config is base.config and not hasattr(plain.config, "label_smoothing")
    return base, copy.deepcopy(base), plain, batch


def _eager_steps(model, batch, n):
    from test_model_plumbing import H64
    from flamingo_mini_amd import FusedAdamW
    opt = FusedAdamW([p for p in model.parameters_trainable()], capturable=True, **H64["adamw"])
    losses = []
    for _ in range(n):
        model.zero_grad(set_to_none=True)
        loss = model(**batch).loss
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def _graphed_step(model, batch):
    from test_model_plumbing import H64
    from flamingo_mini_amd import FusedAdamW, GraphedTrainStep
    opt = FusedAdamW([p for p in model.parameters_trainable()], capturable=True, **H64["adamw"])
    return GraphedTrainStep(model, opt, batch, warmup=1)              # (the constructor's warm-up is training step 1)


def test_the_config_keys_reach_the_kernels_through_eager_and_graphed_steps():
    """A tiny GPT-2-backed model (the h64 fixture's geometry, float32) carrying config.label_smoothing and config.z_loss, driven only by
    model(**batch): the loss is the definition applied to the model's own logits and differs from the loss of the same model without the
    keys; two eager training steps against GraphedTrainStep's warm-up step plus one replay give the same loss, bit for bit; and a replay
    keeps the values the capture saw (launch constants)."""
    eps, zeta = 0.1, 1e-2
    eager, graphed, plain, batch = _h64_arms(eps, zeta)
    with stock_attention_pinned():
        with torch.no_grad():
            out = eager(**batch)
            loss_plain = float(plain(**batch).loss)
        n = batch["labels"].shape[0] * (batch["labels"].shape[1] - 1)
        unit = lr.shifted_ce_reg_ref(out.logits.cpu(), batch["labels"].cpu(), torch.ones(n), eps, zeta)
        want = float(unit["loss"].sum()) / n
        bound = (lr.CE_REG_C_F * 2.0 ** -24 * float(unit["t_loss"].sum()) + (n + 1) * 2.0 ** -24 * float(unit["loss"].abs().sum())) / n
        print(f"model loss {float(out.loss):.8g} definition {want:.8g} bound {bound:.3g} plain {loss_plain:.8g}")
        assert abs(float(out.loss) - want) <= bound and abs(float(out.loss) - loss_plain) > 100 * bound
        with torch.no_grad():
            assert abs(float(eager(**batch, label_smoothing=0.0, z_loss=0.0).loss) - loss_plain) <= bound        # an explicit 0 overrides the keys
        losses_e = _eager_steps(eager, batch, 2)
        step = _graphed_step(graphed, batch)
        loss_g = float(step())
        torch.cuda.synchronize()
        print(f"eager losses {losses_e} replayed {loss_g}")
        assert losses_e[0] == float(out.loss) and loss_g == losses_e[1], (losses_e, loss_g)
        graphed.config.label_smoothing, graphed.config.z_loss = 0.0, 0.0      # launch constants: the captured step keeps what it was captured with
        loss_g3 = float(step())
        assert loss_g3 == _eager_steps(eager, batch, 1)[0]                      # (the eager arm still has the keys; the plain loss is 0.25 away)


def test_eager_and_replayed_steps_leave_equal_parameter_bits():
    """The same two arms after the second training step - two eager steps; the warm-up step of GraphedTrainStep and one replay -: equal
    losses and every trainable parameter bit for bit, with the config keys set and, for comparison, without them."""
    for eps, zeta in ((0.1, 1e-2), (0.0, 0.0)):
        eager, graphed, plain, batch = _h64_arms(eps, zeta)
        with stock_attention_pinned():
            losses_e = _eager_steps(eager, batch, 2)
            step = _graphed_step(graphed, batch)
            loss_g = float(step())
            torch.cuda.synchronize()
        assert loss_g == losses_e[1], (eps, zeta, losses_e, loss_g)
        differ = {k: float((pe - pg).abs().max()) for (k, pe), (_, pg) in zip(eager.named_parameters(), graphed.named_parameters()) if not torch.equal(pe, pg)}
        print(f"eps {eps} zeta {zeta}: parameters that differ after the step: {len(differ)}", differ)
        assert not differ, differ
        assert sum(p.requires_grad for p in eager.parameters()) == 39
