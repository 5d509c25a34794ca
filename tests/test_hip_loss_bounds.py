"""The kernels of csrc/ff_loss.hip and csrc/ff_elementwise.hip held to per-element bounds, on the MI355X.

test_hip_loss.py compares d logits with one whole-tensor rel() (8e-3 in bf16 over 3 x 9 x 50258 elements, the onehot element of every row
dominating the norm) at one even vocabulary, and never looks at lse.  Here every element of lse, loss and d logits is held to float64 from
what the kernel saw (util.shifted_ce_ref, util.ce_bound_ok), and every element of QuickGELU and of its derivative (util.quick_gelu_ref,
util.quick_gelu_bound_ok), at the inputs of tests/loss_cases.py: vocabularies below the head length, below one vector, around the
256-vector boundary and odd (so the rows run through every start phase relative to the 16-byte grid), targets in the scalar head, the
vector body and the scalar tail, ignored positions and an all-ignored sample, sorted rows, one dominant logit, a common offset, -inf at
non-target columns, logits one element off the grid; QuickGELU sizes around one vector and one workgroup and one that needs a second
grid-stride pass, with inputs out to +-60.  The C ABI is called directly where a test wants lse or a chosen base pointer - its buffers
lie in arenas whose surroundings hold a sentinel that must survive -, the wrappers of functional.py elsewhere."""
import pytest
import torch

import loss_cases as lc
from guarded import SENTINEL, guarded_allocations
from util import ce_bound_ok, quick_gelu_bound_ok, quick_gelu_ref, shifted_ce_ref

pytestmark = pytest.mark.gpu
BF16, F32 = lc.BF16, lc.F32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
BITS = {F32: torch.int32, BF16: torch.int16}
PAD = 64                                         # sentinel elements on either side of a body (a multiple of 16 bytes in both dtypes)


class Arena:
    """A device buffer whose body starts `off` elements past the 16-byte grid, PAD or more sentinel elements around it"""

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


def ce_cabi(x, lab, g, off=0):
    """ff_shifted_ce_fwd and ff_shifted_ce_bwd on logits whose first element is `off` elements off the 16-byte grid: (loss, lse, d) on the
    CPU.  Nothing around any buffer is written, the logits are not written."""
    from flamingo_mini_amd import ffi
    lib, code = ffi.lib(), ffi.dtype_code(x.dtype)
    b, L, V = x.shape
    xa = Arena(x.shape, x.dtype, off, x)
    da = Arena(x.shape, x.dtype, off)
    rows, lse = Arena((b * (L - 1),), F32), Arena((b * (L - 1),), F32)
    labels, gd = lab.cuda(), g.cuda()
    before = xa.bits.clone()
    stream = ffi.stream_handle(xa.flat.device)
    ffi.check(lib.ff_shifted_ce_fwd(code, b, L, V, xa.body.data_ptr(), labels.data_ptr(), lc.IGNORE, rows.body.data_ptr(), lse.body.data_ptr(),
                                    stream), "ff_shifted_ce_fwd")
    ffi.check(lib.ff_shifted_ce_bwd(code, b, L, V, xa.body.data_ptr(), labels.data_ptr(), lc.IGNORE, lse.body.data_ptr(), gd.data_ptr(),
                                    da.body.data_ptr(), stream), "ff_shifted_ce_bwd")
    torch.cuda.synchronize()
    assert torch.equal(xa.bits, before), "the logits (or their surroundings) were written"
    assert da.intact() and rows.intact() and lse.intact(), "a write outside an output"
    assert torch.equal(labels.cpu(), lab) and torch.equal(gd.cpu(), g)
    return rows.body.cpu(), lse.body.cpu(), da.body.cpu()


def held(name, x, lab, g, got, worst):
    """(loss, lse or None, d) against the float64 reference by ce_bound_ok; prints and collects every figure, then asserts"""
    ref = shifted_ce_ref(x, lab, g, lc.IGNORE)
    res = {what: ce_bound_ok(what, t, ref, x.dtype) for what, t in zip(("loss", "lse", "d"), got) if t is not None}
    for what, (ok, w, idx) in res.items():
        print(f"{str(x.dtype).replace('torch.', '')} {name} {what}: worst element at {w:.3f} of its bound")
        worst[what] = max(worst.get(what, 0.0), w)
    for what, (ok, w, idx) in res.items():
        where = idx if what != "d" else (idx // (x.shape[1] * x.shape[2]), idx // x.shape[2] % x.shape[1], idx % x.shape[2])
        assert ok, f"{name}: {what} element {where} is {w:.4g} x its bound"
    last, ignored = got[2][:, -1], got[2][:, :-1][lab[:, 1:] == lc.IGNORE]
    assert int((last != 0).sum()) == 0 and int((ignored != 0).sum()) == 0 and ignored.numel() > 0
    return ref


def check_labels(lab):
    """one ignored target per sample; the last sample of three or more all ignored"""
    b = lab.shape[0]
    per_sample = (lab[:, 1:] == lc.IGNORE).sum(dim=1).tolist()
    assert per_sample == [1] * (b - 1) + [lab.shape[1] - 1] if b >= 3 else per_sample == [1] * b, per_sample


@DTYPES
def test_ce_every_vocabulary_within_the_element_bounds(dtype):
    """b = 4, L = 5 at every vocabulary of loss_cases.vocabularies, the 256-vector-boundary ones also one element off the grid: lse, loss and
    d logits element by element.  At every odd V >= 9 every start phase of the dtype occurs on a row that has a loss (from the data
    pointers); over the cases the targets fall in the scalar head, the vector body and the scalar tail."""
    worst, regions, es = {}, set(), 16 // lc.NVEC[dtype]
    with guarded_allocations() as gd:
        for name, x, lab, g, off in lc.ce_cases(dtype, ("shapes",)):
            b, L, V = x.shape
            assert (b, L) == (lc.B, lc.L)
            check_labels(lab)
            if V % 2 == 1 and V >= 9:
                a = Arena(x.shape, dtype, off)
                phases = {(a.body[s, i].data_ptr() % 16) // es for s in range(b) for i in range(L - 1)}
                assert phases == set(range(lc.NVEC[dtype])), (V, phases)
                assert [a.body[r // L, r % L].data_ptr() % 16 for r in range(b * L)] == lc.row_starts(b, L, V, dtype, off)
            regions |= lc.target_regions(V, dtype, lab, off)
            held(name, x, lab, g, ce_cabi(x, lab, g, off), worst)
        gd.check()
    assert regions == {"head", "body", "tail"}, regions
    print(f"worst over the vocabularies: {worst}")


@DTYPES
def test_ce_value_patterns_within_the_element_bounds(dtype):
    """Sorted rows (ascending: every element a new maximum, descending: none but the first), one logit 80 above the rest at the target and
    away from it, a common offset of 1000 (fp32) / 64 (bf16), at V = 4099 and at one vector per thread + 1."""
    worst = {}
    with guarded_allocations() as gd:
        for name, x, lab, g, off in lc.ce_cases(dtype, ("patterns",)):
            ref = held(name, x, lab, g, ce_cabi(x, lab, g, off), worst)
            if "spike-target" in name:                                    # the softmax is the onehot: a loss of (almost) nothing
                assert float(ref["loss"].abs().max()) < 1e-30 and int((lab == lc.spike_column(x.shape[2])).sum()) >= 9
        gd.check()
    print(f"worst over the patterns: {worst}")


@DTYPES
def test_ce_neg_inf_at_non_target_columns(dtype):
    """-inf logits (masked vocabulary entries) at column 0, at the first body column of each row's phase, in the first 300 columns and in
    the last column, aligned and one element off the grid: loss and lse finite and within their bounds as F.cross_entropy's are, d logits
    exactly 0 at those columns.  (Before the forward started its maximum at -FLT_MAX, a thread whose first logit was -inf made the row NaN.)"""
    worst = {}
    with guarded_allocations() as gd:
        for name, x, lab, g, off in lc.ce_cases(dtype, ("neg-inf",)):
            masked = torch.isinf(x)
            assert int(masked.sum()) >= (299 * 20 if "first300" in name else 12) and not bool(torch.isposinf(x).any())
            loss, lse, d = ce_cabi(x, lab, g, off)
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(lse).all()), f"{name}: loss {loss.tolist()} lse {lse.tolist()}"
            held(name, x, lab, g, (loss, lse, d), worst)
            assert int((d[masked] != 0).sum()) == 0, name
        gd.check()
    print(f"worst over the -inf cases: {worst}")


@DTYPES
@pytest.mark.parametrize("V", lc.V_GPT2)
def test_ce_gpt2_vocabularies_within_the_element_bounds(dtype, V):
    worst = {}
    with guarded_allocations() as gd:
        (name, x, lab, g, off), = [c for c in lc.ce_cases(dtype, ("gpt2",)) if c[1].shape[2] == V]
        assert x.shape == (2, lc.L, V)
        check_labels(lab)
        held(name, x, lab, g, ce_cabi(x, lab, g, off), worst)
        gd.check()


@DTYPES
def test_ce_nonfinite_rows_are_nan_for_that_row_only(dtype):
    """Pinned, as torch has it: a row of all -inf, a row holding +inf and a row holding a NaN each give a NaN loss for that row, and every
    other row's loss, lse and gradient are bit for bit what they are without it."""
    V = lc.V_PATTERN[dtype][1]
    x0, _ = lc.logits(V, dtype)
    lab, g = lc.labels(V, start=2), lc.grad_rows()
    with guarded_allocations() as gd:
        base = ce_cabi(x0, lab, g)
        assert bool(torch.isfinite(base[0]).all())
        for what, (s, i) in (("all -inf", (0, 1)), ("+inf", (1, 0)), ("nan", (2, 3))):
            assert int(lab[s, i + 1]) != lc.IGNORE
            x = x0.clone()
            if what == "all -inf":
                x[s, i] = float("-inf")
            else:
                x[s, i, V // 3] = float("inf") if what == "+inf" else float("nan")
            loss, lse, d = ce_cabi(x, lab, g)
            r = s * (lc.L - 1) + i
            others = torch.arange(loss.numel()) != r
            assert bool(torch.isnan(loss[r])) and int(torch.isnan(loss).sum()) == 1, (what, loss.tolist())
            assert torch.equal(loss[others], base[0][others]) and torch.equal(lse[others], base[1][others]), what
            keep = torch.ones(x.shape[:2], dtype=torch.bool)
            keep[s, i] = False
            assert torch.equal(d[keep].view(BITS[dtype]), base[2][keep].view(BITS[dtype])), what
            ref = torch.nn.functional.cross_entropy(x.double()[:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1), reduction="none")
            assert bool(torch.isnan(ref[r])) and int(torch.isnan(ref).sum()) == 1, what
        gd.check()


@DTYPES
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off-grid"])
def test_shifted_cross_entropy_wrapper_within_the_element_bounds(dtype, off):
    """F.shifted_cross_entropy(reduction='none') forward and backward, its outputs guarded allocations; off-grid: the logits are a
    contiguous view one element off the 16-byte grid (flat[1:1 + n].view(b, L, V)), which the wrapper has to take like any other."""
    from flamingo_mini_amd import functional as F
    worst = {}
    for V in (lc.V_SMALL[4], lc.V_BOUNDARY[dtype][2], lc.V_LARGE):
        x, _ = lc.logits(V, dtype, seed=4)
        lab, g = lc.labels(V, start=6), lc.grad_rows()
        flat = torch.empty(x.numel() + 16, dtype=dtype, device="cuda")
        logits = flat[off:off + x.numel()].view(x.shape)
        logits.copy_(x)
        assert logits.is_contiguous() and logits.data_ptr() % 16 == off * x.element_size()
        logits.requires_grad_(True)
        with guarded_allocations() as gd:
            rows = F.shifted_cross_entropy(logits, lab.cuda(), reduction="none")
            (rows * g.cuda()).sum().backward()
            gd.check()
        held(f"wrapper V={V}", x, lab, g, (rows.detach().cpu(), None, logits.grad.cpu()), worst)
        assert torch.equal(logits.detach().cpu().view(BITS[dtype]), x.view(BITS[dtype]))


@DTYPES
def test_quick_gelu_within_the_element_bound(dtype):
    """F.quick_gelu and its derivative element by element, from an empty tensor over sizes around one vector and one workgroup to one that
    takes a second grid-stride pass (the grid is capped at 4096 workgroups) plus three workgroups and a ragged tail; inputs normal x 4 with a
    ramp from -60 to 60 at the end."""
    from flamingo_mini_amd import functional as F
    worst = [0.0, 0.0]
    sizes = lc.gelu_sizes(dtype)
    assert sizes[-1] > lc.GRID_PASS[dtype] + 256 * lc.NVEC[dtype] and sizes[-1] % lc.NVEC[dtype] == lc.NVEC[dtype] - 1
    for n in sizes:
        x, dy = lc.gelu_inputs(n, dtype)
        xd = x.cuda().requires_grad_(True)
        with guarded_allocations() as gd:
            y = F.quick_gelu(xd)
            y.backward(dy.cuda())
            gd.check()
        for k, (what, got, w) in enumerate((("forward", y.detach(), None), ("derivative", xd.grad, dy))):
            ok, ratio, idx = quick_gelu_bound_ok(got.cpu(), *quick_gelu_ref(x, w), dtype)
            print(f"{str(dtype).replace('torch.', '')} quick_gelu n = {n} {what}: worst element at {ratio:.3f} of its bound")
            worst[k] = max(worst[k], ratio)
            assert ok, f"n = {n} {what}: element {idx} (x = {float(x[idx])!r}) is {ratio:.4g} x its bound"
    print(f"worst over the sizes: forward {worst[0]:.3f} derivative {worst[1]:.3f}")


@DTYPES
def test_quick_gelu_off_the_grid(dtype):
    """x (and dy) contiguous views one element off the 16-byte grid: the wrapper takes them like any other tensor"""
    from flamingo_mini_amd import functional as F
    n = 256 * lc.NVEC[dtype] + 1
    x, dy = lc.gelu_inputs(n, dtype, seed=12)
    xd = torch.empty(n + 16, dtype=dtype, device="cuda")[1:1 + n].copy_(x).requires_grad_(True)
    dyd = torch.empty(n + 16, dtype=dtype, device="cuda")[1:1 + n].copy_(dy)
    assert xd.data_ptr() % 16 == x.element_size() == dyd.data_ptr() % 16
    with guarded_allocations() as gd:
        y = F.quick_gelu(xd)
        y.backward(dyd)
        gd.check()
    for what, got, w in (("forward", y.detach(), None), ("derivative", xd.grad, dy)):
        ok, ratio, idx = quick_gelu_bound_ok(got.cpu(), *quick_gelu_ref(x, w), dtype)
        assert ok, f"{what}: element {idx} is {ratio:.4g} x its bound"
