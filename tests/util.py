"""Shared helpers for the parity tests."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Tolerances (relative L2 error against the fp64 oracle / reference vectors), set from MEASURED errors (tools/tol_report.py over a
# `FF_TOL_REPORT=... pytest -m gpu` run on an MI355X, round 2) with a 1.3-2x margin - the kernels are bitwise deterministic, so the
# margin only has to absorb a different tile / split-K plan:
#   fp32 path (MFMA fp32 FMA chains + __expf): measured <= 2.7e-6 everywhere (BASELINE.json's logits target is 1e-3)  -> 5e-6 / 1e-5
#   bf16 path (inputs / activations rounded to bf16 at every kernel boundary): primitives <= 2.7e-3, modules at real geometry
#              <= 6.7e-3 on outputs (six stacked resampler layers, config D) and <= 9.7e-3 on gradients                -> 8e-3 / 1.2e-2
#              The reference's own bf16-vs-fp32 deviation is 6.6e-3 (resampler) / 2.9e-3 (xattn block).
TOL = {torch.float32: dict(out=5e-6, grad=1e-5), torch.bfloat16: dict(out=8e-3, grad=1.2e-2)}
# A THIRD class: the WHOLE drop-in model in bf16 against the reference's float64 vectors - the stock CLIP and GPT-2 stacks run in
# bf16 on PyTorch-ROCm here too, so every stock op rounds on top of the fusion path's own error and the module tolerances above do not apply.
# Measured on an MI355X (rounds 2 and 4): logits 8.9e-3 (tiny GPT-2 fixture) / 6.5e-3 (h64 fixture, step 1), worst parameter gradient
# 1.5e-2 / 1.1e-2, loss |difference| <= 1.2e-2; step 2 of the h64 fixture (weights have left the bf16 grid) is held to twice these bounds,
# measured 2.0e-2 / 3.6e-2.  Used by tests/test_model_plumbing.py::test_full_gpt2_model_bf16_on_hip and ::test_h64_bf16_two_steps_...
TOL_FULL_BF16 = dict(out=1.5e-2, grad=2.5e-2, loss=3e-2)


def gate_grad_ok(got, ref, tol, scale) -> bool:
    """THE rule for the scalar tanh-gate gradients (alpha_attn, alpha_ffw), used by every test that checks one:
            |got - ref| <= tol * (scale + |ref|)
    A gate gradient is a dot product over all b * L * dim elements, (1 - tanh^2 alpha) * sum(d branch_sum .* branch): `scale` is the
    natural size of such a sum of rounded products, (1 - tanh^2 alpha) * || d branch_sum .* branch ||_2 (what it would be if the terms
    did not cancel), |ref| covers relative errors common to all terms.  The golden fixtures carry the scale next to every gate gradient
    (`gs.<name>`, tests/golden/make_golden.py: GateProbe); oracle-based tests compute it from the oracle's cache."""
    return abs(float(np.asarray(got, np.float64).reshape(-1)[0]) - float(np.asarray(ref, np.float64).reshape(-1)[0])) <= \
        tol * (float(np.asarray(scale).reshape(-1)[0]) + abs(float(np.asarray(ref, np.float64).reshape(-1)[0])))


def rel(a, b) -> float:
    a = np.asarray(a.detach().double().cpu().numpy() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().double().cpu().numpy() if torch.is_tensor(b) else b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    r = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
    if os.environ.get("FF_TOL_REPORT"):      # tools/tol_report.py: the measured errors the tolerances above are set from
        with open(os.environ["FF_TOL_REPORT"], "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{r:.3e}\n")
    return r


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a, np.float64)).to(dtype).cuda()


def rnd(shape, seed, scale=1.0):
    g = np.random.default_rng(seed)
    return (g.standard_normal(shape) * scale).astype(np.float32)


def as64(t):
    """what the kernel actually saw (after rounding to its dtype), as float64 numpy"""
    return t.detach().double().cpu().numpy()


def build_cu_hog() -> str:
    """Compile tests/helpers/cu_hog.hip -> libcu_hog.so if stale (hipcc cross-compiles without a GPU; __graft_entry__.build() calls this so
    that the helper travels to the GPU box prebuilt)."""
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
    src, so = os.path.join(here, "cu_hog.hip"), os.path.join(here, "libcu_hog.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        hipcc = next(c for c in ("/opt/rocm/bin/hipcc", "hipcc") if c == "hipcc" or os.path.exists(c))
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", "-o", so, src], check=True, capture_output=True)
    return so


def cu_hog():
    """ctypes handle of tests/helpers/libcu_hog.so (a kernel that holds CUs for a given time - a test helper, not part of the product
    library).  `lib.cu_hog_launch(blocks, lds_bytes, milliseconds, sink_ptr, stream)` returns a hipError_t."""
    import ctypes
    lib = ctypes.CDLL(build_cu_hog())
    lib.cu_hog_launch.restype = ctypes.c_int
    lib.cu_hog_launch.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def hog_stream():
    """The stream to launch cu_hog on: it must run BESIDE the current stream's launches, not ahead of them.  HIP maps streams onto a small,
    fixed pool of hardware queues and, once the pool is full, hands a new stream the least-used queue - late in
    a test session, after many streams were created, that can be the current stream's own queue, and then every launch the test makes
    waits behind the hog in that queue.  High-priority streams draw from a pool of their own, apart from the normal-priority queues the
    test's launches go to."""
    return torch.cuda.Stream(priority=-1)


# ---- row-level and element-level checks (tests/test_hip_bounds.py; the checkers' own tests: tests/test_guarded_checks.py) ----
# rel() above is ONE number over a whole tensor: an error confined to a few rows or one tile is diluted by everything else.  These two
# look at the worst row / the worst element instead.
def _np64(a):
    return np.asarray(a.detach().double().cpu().numpy() if torch.is_tensor(a) else a, np.float64)


def _report(tag, v):
    if os.environ.get("FF_TOL_REPORT"):      # the same report as rel(), the test id tagged [rows] / [elem]
        with open(os.environ["FF_TOL_REPORT"], "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}[{tag}]\t{v:.3e}\n")


def rel_rows(got, ref, row_axes, floor=1e-2):
    """(worst row's relative L2 error, that row's index) - a row is the set of elements that share the indices on `row_axes`, e.g. (0, 1)
    = (sample, token) of a (b, n, d) block output, (0, 2, 1) = (b, h, q) of a (b, nq, h, d) attention output.
    Rows whose reference norm is below `floor` x the median row norm are compared absolutely (their error is divided by that floor
    instead of by their own norm).  Rows the reference holds as exactly zero must be exactly zero: any other value gives inf.  A NaN in
    `got` (an element a kernel never wrote, under tests/guarded.py's poison) gives inf for its row."""
    g, r = _np64(got), _np64(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    row_axes = tuple(a % r.ndim for a in (row_axes if isinstance(row_axes, (tuple, list)) else (row_axes,)))
    rest = tuple(a for a in range(r.ndim) if a not in row_axes)
    rows_shape = tuple(r.shape[a] for a in row_axes)
    g2 = np.transpose(g, row_axes + rest).reshape(int(np.prod(rows_shape)), -1)
    r2 = np.transpose(r, row_axes + rest).reshape(int(np.prod(rows_shape)), -1)
    rn = np.linalg.norm(r2, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        en = np.linalg.norm(g2 - r2, axis=1)
    nz = rn[rn > 0]
    den = np.maximum(rn, floor * (float(np.median(nz)) if nz.size else 1.0))
    err = en / den
    zero_rows = ~np.any(r2 != 0, axis=1)
    err[zero_rows] = np.where(np.any(g2[zero_rows] != 0, axis=1), np.inf, 0.0)
    err[~np.isfinite(err)] = np.inf
    i = int(np.argmax(err))
    worst = float(err[i])
    _report("rows", worst)
    return worst, tuple(int(x) for x in np.unravel_index(i, rows_shape))


def gemm_ref(A, B, a_layout=0, b_layout=0, scale=1.0):
    """(scale . op(A) op(B), |scale| . |op(A)| |op(B)|) in float64 from what the kernel saw - the product and the size of its terms."""
    a, b = _np64(A), _np64(B)
    a = a if a_layout == 0 else a.T
    b = b.T if b_layout == 0 else b
    return scale * (a @ b), abs(scale) * (np.abs(a) @ np.abs(b))


def gemm_bound_ok(C, A, B, a_layout=0, b_layout=0, scale=1.0, epilogue=None, u_out=None, u_mid=0.0, c=2.0):
    """Element-wise bound for a bf16 / fp32 GEMM with fp32 accumulation:
            |C - f(C*)| <= u_out |f(C*)| + |f'(C*)| (c K 2^-24 (|A| |B|) + u_mid |C*|)
    C* = scale op(A) op(B) in float64, f the epilogue: `epilogue(acc) -> (f(acc), |f'(acc)|)` (None: identity).  u_out is the output's
    rounding (default 2^-7 for bf16: one ulp at the bottom of a binade, twice the round-to-nearest worst case - measured on an MI355X,
    tests/test_hip_bounds.py: <= 0.96 of the bound at 2^-8, so <= 0.48 at 2^-7; 2^-22 for fp32); c K 2^-24 |A||B| the worst-case error of a K-term fp32 sum (c = 2:
    a split-K combine on top); u_mid the rounding of an intermediate the epilogue starts from (0: the epilogue sees the fp32 accumulator).
    A single dropped k-step, or one wrong element in any one tile, exceeds it by orders of magnitude.
    Returns (ok, worst error / bound, index of that element)."""
    got = _np64(C)
    acc, absprod = gemm_ref(A, B, a_layout, b_layout, scale)
    K = (A.shape[1] if a_layout == 0 else A.shape[0])
    ref, deriv = (acc, np.ones_like(acc)) if epilogue is None else epilogue(acc)
    if u_out is None:
        u_out = 2.0 ** -7 if C.dtype == torch.bfloat16 else 2.0 ** -22
    bound = u_out * np.abs(ref) + np.abs(deriv) * (c * K * 2.0 ** -24 * absprod + u_mid * np.abs(acc)) + 1e-30
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.abs(got - ref) / bound
    ratio[~np.isfinite(ratio)] = np.inf
    i = int(np.argmax(ratio))
    worst = float(ratio.reshape(-1)[i])
    _report("elem", worst)
    return worst <= 1.0, worst, tuple(int(x) for x in np.unravel_index(i, ratio.shape))


# ---- AdamW, element by element and step by step (tests/test_hip_optim_bounds.py; the checker's own tests: tests/test_guarded_checks.py) ----
# A whole-tensor rel() on the parameters after a few steps cannot see the parameter rule at all in bf16: four steps of lr 3e-3 move a
# weight by less than the 1e-2 the parity tests allow.  These two check ONE step from the state the kernel itself stored, per element.
def _t64(a):
    return a.detach().double().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float64))


def adamw_ref_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0, coef=1.0):
    """One AdamW step in float64 from the given state (torch.optim.AdamW's rule; g' = g * grad_scale * coef).  The hyper-parameters are
    rounded to float32 first and then used as float64 - the kernel receives them as `float`, and 1 - 0.9f is not 0.1; `coef` (the clip
    coefficient) is used as given.  Returns ((p, m, v), (terms_p, terms_m, terms_v)): the new state and, for each of the three, the size
    of the terms that were added to give it, |p| + |update|, |b1 m| + |(1 - b1) g'|, v_new - what a rounding error of the fp32
    arithmetic is proportional to (adamw_bound_ok).  float64 CPU tensors."""
    p, g, m, v = (_t64(x).reshape(-1) for x in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (float(np.float32(x)) for x in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    gp = g * (gs * float(coef))
    m_new = b1 * m + (1.0 - b1) * gp
    v_new = b2 * v + (1.0 - b2) * gp * gp
    bc1, bc2 = 1.0 - b1 ** float(step), 1.0 - b2 ** float(step)
    upd = (lr / bc1) * m_new / (v_new.sqrt() / float(np.sqrt(bc2)) + eps)
    p_new = p * (1.0 - lr * wd) - upd
    return (p_new, m_new, v_new), (p.abs() + upd.abs(), (b1 * m).abs() + ((1.0 - b1) * gp).abs(), v_new)


def _ulp(ref, dtype):
    """spacing of `dtype` (bf16: 8 significant bits, fp32: 24) at each element of the float64 tensor `ref`"""
    bits = {torch.bfloat16: 8, torch.float32: 24}[dtype]
    e = torch.where(ref == 0, torch.full_like(ref, -126.0), torch.frexp(ref)[1].double() - 1.0).clamp(min=-126.0)
    return torch.exp2(e - (bits - 1))


def adamw_excess(got, ref, terms, storage_dtype):
    """max over the elements of (|got - ref| - 0.5 ulp_storage(ref)) / (2^-24 terms): what is left of the error after the one rounding to
    the storage type, in units of one fp32 rounding of the terms - the quantity adamw_bound_ok's c bounds."""
    got, ref, terms = _t64(got).reshape(-1), _t64(ref).reshape(-1), _t64(terms).reshape(-1)
    ex = ((got - ref).abs() - 0.5 * _ulp(ref, storage_dtype)) / (2.0 ** -24 * terms + 1e-300)
    return float(torch.nan_to_num(ex, nan=float("inf")).max())


# c, measured and not derived (tools/adamw_c.py, on the CPU): the worst adamw_excess of a float32 restatement of the kernel's formula, in the
# operation order of `update` in csrc/ff_optim.hip (tests/optim_cases.py: adamw_f32_step), against adamw_ref_step at the inputs of
# tests/test_hip_optim_bounds.py - all four storage modes, both hyper-parameter sets, unclipped and clipped, steps 1-3, 1000 and the graph
# test's four.  Worst excess 5.13 (exp_avg_sq of the clipped fp32 kernel, set B step 2: the fp32 coefficient on top of three roundings
# of g'^2); p <= 4.04 (set B: lr / eps = 10 carries the rounding of m into the update), exp_avg <= 2.58.  c = 4 x 5.13: the factor 4
# is for what the CPU cannot show - the device's powf in capturable mode, its FMA contraction, the fp32 sum of squares behind the
# clip coefficient.  ONE constant for both storage types: a bf16 result is the fp32 result rounded once more, so the fp32 error is
# what decides on which side of a rounding tie it falls (in bf16 the excess shows only at elements next to a tie: measured <= 2.85).
# The bound is only this sharp because those inputs keep |p| >= 0.125 (optim_cases.HP explains why).
# On the MI355X: not measured yet - a `FF_TOL_REPORT=... pytest -m gpu` run writes every call's worst error / bound as an [elem] entry
# (tools/tol_report.py), and tests/test_hip_optim_bounds.py prints it per step and stored tensor.
# ADAMW_C_PARITY, for the per-step checks inside the two parity tests, whose parameters are normal and so come arbitrarily close to zero:
# there the rounding of a cancelling m_new reaches an update that is all of |p| + |update|, amplified by (|b1 m| + |(1 - b1) g'|) / |m_new|,
# and the excess of p is the maximum of a heavy-tailed quantity over 6.5 M elements.  Measured the same way at those tests' inputs:
# p 133.7 (clipped fp32 kernel), moments <= 5.27; 4 x 133.7.  Still 20 times below what any of the defects tests/test_guarded_checks.py
# injects does to an fp32 result.
ADAMW_C = 20.5
ADAMW_C_PARITY = 535.0


def adamw_bound_ok(got, ref, terms, storage_dtype, c=None):
    """Element by element:   |got - ref| <= 0.5 ulp_storage(ref) + c 2^-24 terms
    got: what the kernel stored (bf16 or fp32 = storage_dtype); ref, terms: adamw_ref_step's.  The first term is the one rounding to the
    storage type of an exact result, the second the fp32 arithmetic before it (and what lets a result close to a rounding tie fall to the
    other side).  A NaN in `got` counts as inf.  Returns (ok, worst error / bound, flat index of that element)."""
    c = ADAMW_C if c is None else c
    got, ref, terms = _t64(got).reshape(-1), _t64(ref).reshape(-1), _t64(terms).reshape(-1)
    assert got.shape == ref.shape == terms.shape, (got.shape, ref.shape, terms.shape)
    if got.numel() == 0:
        return True, 0.0, 0
    ratio = (got - ref).abs() / (0.5 * _ulp(ref, storage_dtype) + c * 2.0 ** -24 * terms)
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    i = int(torch.argmax(ratio))
    worst = float(ratio[i])
    _report("elem", worst)
    return worst <= 1.0, worst, i


def adamw_state(opt, p):
    """((w, m, v) as stored now - clones; w = the fp32 master copy where there is one, else p; zero moments before the first step -,
    their storage dtypes)"""
    st = opt.state.get(p, {})
    w = st["master"] if "master" in st else p.detach()
    m, v = (st[k] if k in st else torch.zeros_like(w) for k in ("exp_avg", "exp_avg_sq"))
    return (w.clone(), m.clone(), v.clone()), (w.dtype, m.dtype, v.dtype)


def adamw_step_ok(old, new, g, storages, step, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0, coef=1.0, c=None):
    """One step's stored results new = (w, m, v) against adamw_ref_step from old = (w, m, v) and the gradient g, each by adamw_bound_ok
    in its storage dtype.  Returns (ok, what failed: "name: element i is r x its bound", ...)."""
    refs, terms = adamw_ref_step(old[0], g, old[1], old[2], step, lr, beta1, beta2, eps, weight_decay, grad_scale, coef)
    bad = []
    for name, got, ref, t, sd in zip(("p", "exp_avg", "exp_avg_sq"), new, refs, terms, storages):
        ok, worst, idx = adamw_bound_ok(got, ref, t, sd, c)
        if not ok:
            bad.append(f"{name}: element {idx} is {worst:.4g} x its bound")
    return not bad, "; ".join(bad)


# ---- shifted cross-entropy and QuickGELU, element by element (tests/test_hip_loss_bounds.py; the checkers' own tests: test_guarded_checks.py) ----
# rel() over d logits is dominated by the onehot element (about -g) of every row: the softmax part, the scalar head and tail columns of a row
# and any single row are held far more loosely than its figure suggests.  These compare every element with float64 from what the kernel saw.
def shifted_ce_ref(logits, labels, g, ignore_index=-100):
    """Shifted next-token cross-entropy in float64 from the logits as stored (b, L, V), labels (b, L), g (b (L - 1),) the gradient of each
    loss row.  A dict of float64 CPU tensors:
      lse, loss (b (L - 1),): logsumexp of row (b, i) and lse - x[label[b, i + 1]], 0 for an ignored label;
      d (b, L, V): (exp(x - lse) - onehot) g, exactly 0 for the last position and for ignored rows;
      t_lse = |lse| + 1, t_loss = |lse| + |x_t| + 1 (0 for an ignored label: its loss is exactly 0),
      t_d = |g| (p (1 + |x - lse| + |lse|) + onehot): what a float32 rounding error of each is proportional to - the sum and its logarithm,
      the subtraction, and for d the rounding of x - lse (and of lse itself) in the exponent; flush = 2^-126 |g|, a flushed denormal p."""
    x, g = _t64(logits), _t64(g).reshape(-1)
    lab = labels.detach().cpu().long()
    b, L, V = x.shape
    xs, tgt = x[:, :-1], lab[:, 1:]
    valid = tgt != ignore_index
    lse = torch.logsumexp(xs, dim=-1)
    xt = xs.gather(-1, tgt.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    loss = torch.where(valid, lse - xt, torch.zeros_like(lse))
    p = (xs - lse.unsqueeze(-1)).exp()
    onehot = torch.zeros_like(xs).scatter_(-1, tgt.clamp(0, V - 1).unsqueeze(-1), 1.0) * valid.unsqueeze(-1)
    gr = (g.reshape(b, L - 1) * valid).unsqueeze(-1)
    zero = torch.zeros_like(xs)
    d, t_d, flush = (torch.zeros_like(x) for _ in range(3))
    d[:, :-1] = torch.where(valid.unsqueeze(-1), (p - onehot) * gr, zero)
    size = torch.where(p == 0, zero, p * (1.0 + (xs - lse.unsqueeze(-1)).abs() + lse.abs().unsqueeze(-1)))      # p = 0 at a -inf logit
    t_d[:, :-1] = torch.where(valid.unsqueeze(-1), gr.abs() * (size + onehot), zero)
    flush[:, :-1] = (2.0 ** -126 * gr.abs()).expand_as(xs)
    return dict(lse=lse.reshape(-1), loss=loss.reshape(-1), d=d, t_lse=(lse.abs() + 1.0).reshape(-1),
                t_loss=torch.where(valid, lse.abs() + xt.abs() + 1.0, torch.zeros_like(lse)).reshape(-1), t_d=t_d, flush=flush)


def _elem_ratio(got, ref, bound):
    """(worst |got - ref| / bound, its flat index): nothing excluded, NaN counts as inf, an exact match is 0 whatever the bound"""
    got, ref, bound = _t64(got).reshape(-1), _t64(ref).reshape(-1), _t64(bound).reshape(-1)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.numel() == 0:
        return 0.0, 0
    err = (got - ref).abs()
    ratio = torch.where((err == 0) | (got == ref), torch.zeros_like(err), torch.nan_to_num(err / bound, nan=float("inf"), posinf=float("inf")))
    i = int(torch.argmax(ratio))
    return float(ratio[i]), i


def _excess(got, ref, terms, fixed):
    """max of (|got - ref| - fixed) / (2^-24 terms): the error left after the allowance that does not scale with the constant, in units of
    one float32 rounding of the terms (what the constants below bound); an error within `fixed` alone counts as 0"""
    got, ref, terms, fixed = (_t64(a).reshape(-1) for a in (got, ref, terms, fixed))
    if got.numel() == 0:
        return 0.0
    over = (got - ref).abs() - fixed
    ex = torch.where(~(over > 0) & ~torch.isnan(over), torch.zeros_like(over), over / (2.0 ** -24 * terms))
    return float(torch.nan_to_num(ex, nan=float("inf"), posinf=float("inf")).max())


# c_f, c_b, c_q: measured, not derived (tools/loss_c.py, on the CPU): the worst excess of the float32 restatements of the kernels in their
# operation order (tests/loss_cases.py: ce_fwd_f32 - per-thread online (m, s) over head, vectors and tail, xor-shuffle combine, four-wave
# combine -, ce_bwd_f32, quick_gelu_f32) over the float64 references, at exactly the inputs of tests/test_hip_loss_bounds.py, both dtypes;
# times 4, the factor and the reasons of ADAMW_C: the device's __expf / logf and its FMA contraction cannot be shown on the CPU.
# Worst excess: lse 1.06 (bf16 V = 3), loss 1.24 (bf16 V = 4099 with -inf in the last column) -> c_f = 4 x 1.24; d 0.95 (fp32 V = 1025,
# -inf in the last column, off the grid; in bf16 half a storage ulp covers nearly everything: <= 0.53) -> c_b = 4 x 0.95; QuickGELU
# 2.87 (the fp32 derivative at the largest size; forward 2.07; bf16 <= 0.27) -> c_q = 4 x 2.87.
# On the MI355X (worst error / bound per checker, the [elem] entries of an FF_TOL_REPORT run of tests/test_hip_loss_bounds.py):
#   lse 0.20 (fp32) / 0.21 (bf16), loss 0.22 / 0.25;
#   d logits 0.39 in fp32 apart from the two one-dominant-logit patterns, 0.999: there every other p is below 2^-126, v_exp_f32 returns 0,
#   and the error is p |g| against the 2^-126 |g| the bound's last term allows for exactly that; 0.999 in bf16: an exact result next to a
#   rounding tie, where half a storage ulp is nearly all of the bound;
#   QuickGELU forward 0.956 / derivative 0.942 in fp32, both at x = -59.76 and -59.70 on the ramp: results of 4e-43, denormals with eight
#   significant bits, whose rounding is half a storage ulp - the restatement gives the same two figures at the same elements; 1.000 in
#   bf16, rounding ties again.  No device figure is above 1.
CE_C_F = 5.0
CE_C_B = 3.8
QGELU_C = 11.5


def ce_bound_ok(what, got, ref, storage_dtype=torch.float32, c=None):
    """One output of the shifted cross-entropy against shifted_ce_ref's dict, element by element, nothing excluded, NaN = inf:
      what = "lse":   |lse - lse*| <= c_f 2^-24 (|lse*| + 1)
             "loss":  |loss - loss*| <= c_f 2^-24 (|lse*| + |x_t| + 1)
             "d":     |d - d*| <= 0.5 ulp_storage(d*) + c_b 2^-24 |g| (p (1 + |x - lse*| + |lse*|) + onehot) + 2^-126 |g|
    Returns (ok, worst error / bound, flat index of that element)."""
    if what == "d":
        bound = 0.5 * _ulp(ref["d"], storage_dtype) + (CE_C_B if c is None else c) * 2.0 ** -24 * ref["t_d"] + ref["flush"]
        bound = torch.where(ref["t_d"] + ref["flush"] == 0, torch.zeros_like(bound), bound)          # last position, ignored rows: exactly 0
    else:
        bound = (CE_C_F if c is None else c) * 2.0 ** -24 * ref["t_" + what]
    worst, i = _elem_ratio(got, ref[what], bound)
    _report("elem", worst)
    return worst <= 1.0, worst, i


def ce_excess(what, got, ref, storage_dtype=torch.float32):
    if what == "d":
        return _excess(got, ref["d"], ref["t_d"], torch.where(ref["t_d"] + ref["flush"] == 0, torch.zeros_like(ref["d"]),
                                                              0.5 * _ulp(ref["d"], storage_dtype) + ref["flush"]))
    return _excess(got, ref[what], ref["t_" + what], torch.zeros_like(ref[what]))


QGELU_A = float(np.float32(1.702))


def quick_gelu_ref(x, dy=None):
    """(value, terms) in float64 from x (and dy) as stored, 1.702 rounded to float32 first as the kernel has it: x s with s = sigmoid(1.702 x),
    or the derivative dy s (1 + 1.702 x (1 - s)).  terms = |value| (1 + 1.702 |x|), where for the derivative |value| is taken as the size of
    its two terms, |dy| s (1 + 1.702 |x| (1 - s)): the same for x >= 0, but around x = -0.75, where the derivative changes sign, the two
    cancel, and no float32 evaluation keeps an error proportional to the difference (among 4 M normal inputs some fall within 1e-6 of it)."""
    x = _t64(x).reshape(-1)
    s = torch.sigmoid(QGELU_A * x)
    if dy is None:
        value = x * s
        return value, value.abs() * (1.0 + QGELU_A * x.abs())
    dy = _t64(dy).reshape(-1)
    return dy * s * (1.0 + QGELU_A * x * (1.0 - s)), dy.abs() * s * (1.0 + QGELU_A * x.abs() * (1.0 - s)) * (1.0 + QGELU_A * x.abs())


def quick_gelu_bound_ok(got, ref, terms, storage_dtype, c=None):
    """Element by element, nothing excluded, NaN = inf:   |got - ref| <= 0.5 ulp_storage(ref) + c_q 2^-24 terms      (quick_gelu_ref's)
    Returns (ok, worst error / bound, flat index of that element)."""
    worst, i = _elem_ratio(got, ref, 0.5 * _ulp(_t64(ref).reshape(-1), storage_dtype) + (QGELU_C if c is None else c) * 2.0 ** -24 * _t64(terms).reshape(-1))
    _report("elem", worst)
    return worst <= 1.0, worst, i


def quick_gelu_excess(got, ref, terms, storage_dtype):
    return _excess(got, ref, terms, 0.5 * _ulp(_t64(ref).reshape(-1), storage_dtype))


# ---- the attention core, element by element (tests/test_hip_attention_bounds.py; the checkers' own tests: tests/test_attn_cases.py) ----
# rel() and rel_rows() at 5e-6 / 8e-3 hold a row's L2 norm: one wrong key tile of one row, an lse that is off, a zero row that holds 1e-30
# or a stride used for the wrong tensor in one head all hide inside them.  attn_cases.attention_ref gives every output of the three kernels
# in float64 from what they saw, with the size of the terms each rounding error is proportional to; attn_bound_ok holds every element:
#   lse:  |lse - lse*| <= c_l 2^-24 (1 + |lse*| + sum_j p_ij a_ij)                     a_ij = sum_d |q_id| |k_jd|, the size of a score's terms
#   o:    1/2 ulp_T(o*) + u_P sum_j p_ij |v_jd| + c_o 2^-24 (sum_j w_ij |v_jd| + |o*_id| sum_j w_ij) + 2^-126 sum_j |v_jd|
#   dV:   1/2 ulp_T + u_P sum_i p_ij |dO_id| + c_g 2^-24 sum_i w_ij |dO_id| + 2^-126 sum_i |dO_id|
#   dQ:   1/2 ulp_T + u_P sum_j |ds_ij| |k_jd| + (1 + u_P) u_T (sum_d |dO_id o*_id|) sum_j p_ij |k_jd| + c_g 2^-24 sum_j g_ij |k_jd|
#         + 2^-126 sum_j (1 + |dp_ij| + |D_i|) |k_jd|
#   dK:   the dQ bound with q for k and the sums over i
# w_ij = p_ij (1 + a_ij + |s_ij - lse*_i|): the rounding of the score and of the exponent's argument reach p in proportion to it;
# g_ij = p_ij (|dp_ij| + |D_i|)(1 + a_ij + |s_ij - lse*_i|) + p_ij (b_ij + sum_d |dO_id o*_id|), b_ij = sum_d |dO_id| |v_jd|: the same for
# ds = p (dp - D), plus the rounding of dp and of D.  The sums run over the keys a row may see (over the rows that may see a key).
# u_P: P and dS are rounded to bf16 before the second product (0 in fp32); u_T: D = rowsum(dO . O) is taken from the STORED O (2^-24 in
# fp32), and dS is rounded after that D went in (the 1 + u_P).  Both are 2^-8 in bf16, the format's unit roundoff (8 significant bits: half
# a spacing of 2^-7 at the bottom of a binade).  With 2^-9 the bf16 restatement itself is up to 1.15 x its bound (d v of bf16-dh32-64x130-scales:
# error 0.119 = half an ulp of the result, 0.0625, + 0.057 from the rounded P, where 2^-9 sum p |dO| allows 0.042).
# The 2^-126 terms: __expf is v_exp_f32, which returns 0 below 2^-126, so a probability (or a rescale factor alpha) that small is lost
# whole - an absolute error of up to 2^-126 per key (query) of the sum, however small the sum itself is; in bf16 a dS below 2^-126 has
# fewer than eight bits left: the "1 +".  The sharp cases put the second-best score 95 below the best, p = 5e-42: d v and d k of a key
# no row favours are 1e-41 exactly and 0 from the kernel.  Without the terms the fp32 restatement is 85138 (d v) and 82137 (d k) roundings
# over at f32-dh128-130x200-sharp-rows; with them no case is above 6.81.
# Where every term is zero - a text_time = 0 row's o and dq, a uniform row's dq, the dk of an image no token looks at - the bound is 0:
# the kernel must store an exact zero.  A zero row's lse must be the kernel's sentinel 1e30 (exp(s - 1e30) = 0 whatever the score).
# c_l, c_o, c_g: measured, not derived (tools/attn_c.py, on the CPU): 4 x the worst excess of the float32 / bf16 restatements of the kernels
# (attn_cases.attn_fwd_f32, attn_bwd_f32: 64-row tiles, block_range's tile skipping, the running (m, lsum) per lane with the alpha
# rescale, acc * (1 / lsum), exp(s - L) from the stored lse, D from the rounded O) over attention_ref, at exactly the inputs of
# tests/test_hip_attention_bounds.py; the factor 4 as for ADAMW_C: the device's __expf / __logf, the MFMA accumulation order and FMA
# contraction cannot be shown on the CPU.  Worst excess: lse 5.77 (f32-dh128-130x200-sharp-rows: scores of 300, a_ij the whole of the
# bound) -> c_l = 4 x 5.77; o 5.48 (f32-dh128-64x130-tied) -> c_o = 4 x 5.48; d v 6.81 (f32-dh64-media-nv72x3-sharp-rows), d k 5.35
# (f32-dh128-64x130-offset+), d q 4.41 (f32-dh128-65x63-offset+) -> c_g = 4 x 6.81.  In bf16 the fixed terms cover everything but lse
# (<= 3.3).
# On the MI355X (worst error / bound per checker, the [elem] entries of an FF_TOL_REPORT run of tests/test_hip_attention_bounds.py):
#   fp32: lse 0.26 (f32-dh128-64x130-sharp-rows), o 0.25 (f32-dh128-65x63-tied), d q 0.15, d k 0.20, d v 0.19 (the offset cases at dim_head
#   128) - the same cases that give the restatement's worst figures, at the 1 / 4 the factor leaves;
#   bf16: lse 0.11, o 0.81 (bf16-dh128-65x63-tied), d q 0.51, d k 0.77, d v 0.86 (the scales cases at 64x130): results beside a rounding tie,
#   where half a storage ulp and the rounded P are nearly all of the bound.  No device figure is above 1; the kernels needed no change.
# The fused block (tests/test_hip_xattn_bounds.py: every stage of ff_xattn_block_fwd / ff_xattn_block_bwd_kv_data judged from what the kernel
# stored for the stage before, inputs and stage references in tests/xattn_cases.py).  The kernels form d O = tanh(alpha) d y1 Wo themselves
# and never store it, so d Qs, d K and d V are compared with attention_ref at dO* (float64 from the stored d y1) and the bounds gain, with
# e_id = gemm_bound_ok's own bound of that product: sum_i p_ij e_id (d V), sum_j p_ij h_ij |k_jd| (d Q), sum_i p_ij h_ij |q_id| (d K),
# h_ij = sum_d e_id (|v_jd| + |o_id|) - attention_ref(e_do=), attn_bound_ok(extra=True); fixed terms, outside the constants.
# Measured again at those inputs (tools/xattn_c.py: attn_fwd_f32 / attn_bwd_f32 with the fused kernels' tiling - 32 or 64 queries per
# workgroup, one key tile and no rescale in the resident kernels, d O taken in float32 and rounded to T before D and both passes use it;
# reading the kernels showed no other difference in operation order that matters: they share attn_fwd_loop / attn_dq_loop /
# attn_dkv_step with csrc/ff_attention.hip).  Worst excess: lse 3.28, o 3.70 (both general-f32-dh128-offset), d v 1.26
# (general-f32-dh64-sharp-rows), d q and d k 0.00 (the fixed terms cover them); bf16: lse 1.96 (general-bf16-dh128-sharp-rows), all else
# 0.00.  4 x 3.28 = 13.1 < c_l, 4 x 3.70 = 14.8 < c_o, 4 x 1.26 = 5.1 < c_g: the constants stay.
# On the MI355X (worst error / bound per checker and the case that set it, from the tests' own print-out):
#   bf16: Qs 0.493 (general-bf16-multitile-offset), lse 0.060 (res-ring4-ragged-flat), O 0.789 (general-bf16-multitile-scales), attn_out
#   0.490, y1 0.497 (general-bf16-bm64-scales), Hpre 0.492, Aact 0.369, ffw_out 0.488, y_out 0.496 (general-bf16-dh128-offset), d H 0.329,
#   d Qs 0.145 (res-ring6-scales), d K 0.216 (res-ring4-ragged-scales), d V 0.569 (decode-flat);
#   fp32: Qs 0.015, lse 0.145, O 0.198, d V 0.147 (all general-f32-dh128-offset), attn_out 0.031, y1 0.056 (general-f32-dh16-offset), Hpre
#   0.016, ffw_out 0.014, y_out 0.014, d Qs 0.023, d K 0.116 (general-f32-dh64-sharp-rows).
# The fp32 defect: Aact = h (1 + erf(h / sqrt 2)) / 2 cancels in its negative tail.  Before: Aact 31.28 x its bound at general-f32-dh32-flat
# (sample 2, token 2, column 224), 6.08 at general-f32-dh16-offset, 1.69 at general-f32-dh16-scales, 1.21 at general-f32-dh128-scales, and
# d H 1.246 at general-f32-dh16-offset (the same element as its Aact) - the float32 restatement with torch.erf gives all five figures to
# three digits at the same elements.  csrc/ff_common.h now takes the cdf as erfc(-h / sqrt 2) / 2 (fp32 epilogues; the bf16 ones already
# used an erfc form).  After (the restatement in the kernel's new form): Aact <= 0.063, d H <= 0.016 over the fp32 cases.
# d H in fp32: the bound scales |cdf| + |h pdf|, not |cdf + h pdf| - the two cancel at h = -0.752, and with |factor| the restatement itself
# is 1.3 to 124 x over at exactly that h in every fp32 case, in either form of the cdf (xattn_cases.stage_checks says why).
ATTN_C_L = 23.1
ATTN_C_O = 21.9
ATTN_C_G = 27.2
ATTN_U_P = {torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
ATTN_U_T = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
_ATTN_C = {"lse": "ATTN_C_L", "o": "ATTN_C_O", "dq": "ATTN_C_G", "dk": "ATTN_C_G", "dv": "ATTN_C_G"}


def _attn_parts(what, ref, storage_dtype, extra=False):
    """(fixed, scaled): the part of the bound that does not carry the constant and the terms one float32 rounding is proportional to;
    both exactly 0 where no term reaches the element.  extra: the reference's e_<what> (attention_ref(e_do=...): dO is a result of the
    launch under test, known only to within e_do) joins the fixed part; it is 0 wherever the other terms are."""
    r = _t64(ref[what])
    if what == "lse":
        return torch.zeros_like(r), _t64(ref["t_lse"])
    t, pu, fl = _t64(ref["t_" + what]), _t64(ref["pu_" + what]), _t64(ref["fl_" + what])
    fixed = 0.5 * _ulp(r, storage_dtype) + ATTN_U_P[storage_dtype] * pu + 2.0 ** -126 * fl
    if what in ("dq", "dk"):
        fixed = fixed + (1.0 + ATTN_U_P[storage_dtype]) * ATTN_U_T[storage_dtype] * _t64(ref["ut_" + what])     # dS is rounded after D went in
    if extra and what != "lse" and ("e_" + what) in ref:
        fixed = fixed + _t64(ref["e_" + what])
    return torch.where(t + pu + fl == 0, torch.zeros_like(fixed), fixed), t


def attn_bound_ok(what, got, ref, storage_dtype, c=None, extra=False):
    """One output (what = "lse", "o", "dq", "dk", "dv") of the attention kernels against attn_cases.attention_ref's dict, element by
    element, nothing excluded, NaN = inf.  extra: add the reference's e_dq / e_dk / e_dv (_attn_parts).
    Returns (ok, worst error / bound, index of that element in the output's own shape)."""
    c = globals()[_ATTN_C[what]] if c is None else c
    fixed, t = _attn_parts(what, ref, storage_dtype, extra)
    worst, i = _elem_ratio(got, ref[what], fixed + c * 2.0 ** -24 * t)
    _report("elem", worst)
    return worst <= 1.0, worst, tuple(int(x) for x in np.unravel_index(i, tuple(np.shape(ref[what]))))


def attn_excess(what, got, ref, storage_dtype, extra=False):
    fixed, t = _attn_parts(what, ref, storage_dtype, extra)
    return _excess(got, ref[what], t, fixed)


# ---- LayerNorm, element by element (tests/test_hip_layernorm_bounds.py; the checkers' own tests: tests/test_ln_cases.py) ----
# The project has five LayerNorm implementations that compute row statistics (csrc/ff_rowwise.hip: two passes, one wave per row; the general
# fused kernel, the resident kernel and the decode feed-forward kernel: ONE pass, sums shifted by the mean of the row's first 4 / 8 / 16
# elements; phase 3 of the resident kernel: two passes per head slice and a Chan combine).  rel() / rel_rows() at 5e-6 / 8e-3 on N(0, 2^2)
# rows cannot tell a shifted from an unshifted one-pass variance, a wrong divisor, a missing piece of a sum or two swapped rows.
# ln_cases.ln_ref gives every output in float64 from what the kernel saw; y, dx, dgamma and dbeta are computed from the statistics the kernel
# STORED, so the normalising step is judged apart from them.  u = 2^-24, T the storage type, nothing excluded, NaN = inf:
#   mean:    |mean - mean*| <= c_m u (|s0| + mean_c |x_c - s0|)        s0 = 0 (two-pass), the row's shift s* (one-pass)
#   rstd:    |rstd - rstd*| <= rstd* u (c_r + c_v kappa)               kappa = (var* + 2 (mean* - s*)^2) / (var* + eps): what the rounding of
#            the one-pass sums (relative to sum (x - s)^2 = n (var + (mean - s)^2), and of its correction (mean - s)^2) is to var + eps
#   y:       1/2 ulp_T(y) + c_y u (|x - mean| rstd |g| + |b|)          (+ u |mean rstd| |g| for the decode kernel: it forms x rs - mean rs)
#   dx:      1/2 ulp_T + c_x u rstd (|dy g| + mean|dy g| + |xh| mean|dy g xh|) + 1/2 ulp_T(residual) where a residual is added
#   dgamma, dbeta, rows_reduce:   1/2 ulp_T + c_p u sum |terms|;        gate_grad:  1/2 ulp_T + c_p u (1 - tanh^2 alpha) sum |a b|
# Where every term is zero (an all-zero dy row without residual, an all-zero row's mean) the kernel must store an exact zero.
# The constants: measured, not derived (tools/ln_c.py, on the CPU): 4 x the worst excess of the float32 restatements of the kernels in their
# operation order (tests/ln_cases.py) over ln_ref, at exactly the inputs of tests/test_hip_layernorm_bounds.py; the factor 4 as for ADAMW_C:
# the device's rsqrtf, its FMA contraction and its reduction order cannot be shown on the CPU.  c_r comes from the two-pass restatements
# (kappa <= 1 there: the excess is |d rstd| / (u rstd*)), c_v from the one-pass ones (|d rstd| / (u rstd* max(kappa, 1))).
# Worst excess, and the case that set it: c_m 13.30 (mean_a of general-bf16: the bf16 general kernel at dim 512, a massive-head row - each
# thread adds 64 deviations of -250 one after the other) -> 53.3; c_r 8.36 (rstd of bf16-1025x4096: 64 squares per lane in one chain) ->
# 33.5; c_v 5.45 (rstd_a of general-bf16, massive-head, kappa 62) -> 21.9; c_y 2.58 (y of f32-1025x4096-add) -> 10.4; c_x 3.21 (dx of
# f32-1025x2048) -> 12.9; c_p 2.02 (dgamma of f32-5x256; rows_reduce <= 1.40, gate_grad <= 0.27) -> 8.1.
# The decode kernel's y: 1/2 ulp_T is taken at |y| + u |mean rstd| |g|, not at |y|.  The kernel forms x rs - mean rs, so the float32 value it
# rounds to bf16 is off by up to u |mean rstd| |g| whatever |y| is, and may lie in the binade above y's: with 1/2 ulp_T(y) the restatement
# itself is 1.4 % over at decode-dim128 (a const row, mean rstd = 1028, beta = 4.7e-4 just below 2^-11: error 4.196e-5, bound 4.139e-5).
# Two conditions that are not measurements (tests/test_ln_cases.py asserts both): kappa <= 512 on every designed row of every block case
# (largest: 192.4, head-off and massive-head- rows at dim 1536) and <= 2 on every row of at least four families; on every fp32 case
# |rstd - rstd*| / rstd* <= TOL[float32]["out"] = 5e-6 whatever kappa is (the GPU test asserts that one on the device as well).
# On the MI355X (worst error / bound per checker, the [elem] entries of an FF_TOL_REPORT run of tests/test_hip_layernorm_bounds.py):
#   fp32: mean 0.121 (general-f32-bm64-reload), rstd 0.097 (general-f32-widest), y 0.246 (general-f32-multitile), dx 0.651 (f32-1025x4096-add: ln_bwd_dx_kernel),
#   dgamma 0.328, dbeta 0.244, rows_reduce 0.194, gate_grad 0.011; the block kernels' mean_f 0.040, rstd_f 0.037, xn_f 0.216;
#   bf16: mean 0.250, rstd 0.224 (both general-bf16: the restatement's worst case at the 1 / 4 the factor leaves), mean_f 0.038, rstd_f
#   0.066 (phase3-dim1280), gate_grad 0.693; y, dx, dgamma, dbeta, rows_reduce 1.000: results on a rounding tie, where half a storage ulp is
#   all of the error.  No device figure is above 1.  Relative rstd error of the bf16 one-pass kernels: up to 9.0e-6 (separate-ln-dim1536,
#   a head-off row, kappa 184), 5.3e-6 in the bf16 general kernel (massive-head, kappa 62).
# The fp32 defect (the one-pass general kernel with its 4-element shift): CONFIRMED on the device and fixed.  Before: rstd_a of
# general-f32-widest (dim 1536) off by 1.647e-5 relative on a massive-head- row (kappa 192.4; the restatement: 1.70e-5, head-off 1.12e-5),
# 2.72e-6 at dim 256, 1.26e-6 at dim 128 - above the 5e-6 the fp32 parity tests promise.  A 16-element shift would not have helped the
# head-off rows (their first 16 columns ARE the shift: kappa stays 184), so the fp32 kernel now takes the variance by a second pass around
# the mean (csrc/ff_xattn_fused.hip; the bf16 instantiations are unchanged).  After: 3.20e-7 at dim 1536 (massive-head), 1.58e-7 at dim
# 256, 1.71e-7 at dim 128.  Worst |rstd - rstd*| / rstd* per family over the fp32 block cases, on the device, after the fix:
#   plain 1.29e-7, offset+ 1.01e-7, offset- 1.06e-7, massive-head 3.20e-7, massive-head- 2.14e-7, massive-body 2.44e-7, massive-tail 1.09e-7,
#   head-off 1.30e-7, const 5.5e-8, zero 5.5e-8, tiny-var 7.6e-8, big 9.3e-8, small 7.7e-8.
# LN_CONSTANTS_BEGIN (tools/ln_c.py prints these lines)
LN_C_M = 53.3
LN_C_R = 33.5
LN_C_V = 21.9
LN_C_Y = 10.4
LN_C_X = 12.9
LN_C_P = 8.1
# LN_CONSTANTS_END
_LN_C = {"y": "LN_C_Y", "dx": "LN_C_X", "dgamma": "LN_C_P", "dbeta": "LN_C_P", "rows_reduce": "LN_C_P", "gate_grad": "LN_C_P"}


def _ln_parts(what, ref, storage_dtype, decode=False):
    """(fixed, scaled): the part of the bound that carries no constant and the terms one float32 rounding is proportional to"""
    r, t = _t64(ref[what]), _t64(ref["t_" + what])
    fixed = 0.5 * _ulp(r, storage_dtype)
    if what == "y" and decode:      # the storage rounding is taken where the fp32 value may lie: |y| + u |mean rstd| |g| can be in the next binade
        dec = 2.0 ** -24 * _t64(ref["t_y_dec"])
        fixed = 0.5 * _ulp(r.abs() + dec, storage_dtype) + dec
    if what == "dx":
        if ref.get("residual") is not None:
            fixed = fixed + 0.5 * _ulp(_t64(ref["residual"]), storage_dtype)
        else:
            fixed = torch.where(t == 0, torch.zeros_like(fixed), fixed)
    return fixed, t


def ln_bound_ok(what, got, ref, storage_dtype=torch.float32, c=None, decode=False):
    """One output of a LayerNorm kernel (what = "mean", "rstd", "y", "dx", "dgamma", "dbeta", "rows_reduce", "gate_grad") against
    ln_cases.ln_ref's dict (rows_reduce_ref's, gate_grad_ref's), element by element.  c: the constant (rstd: the pair (c_r, c_v)).
    Returns (ok, worst error / bound, index of that element in the output's own shape)."""
    u = 2.0 ** -24
    if what == "mean":
        bound = (LN_C_M if c is None else c) * u * _t64(ref["t_mean"])
    elif what == "rstd":
        cr, cv = (LN_C_R, LN_C_V) if c is None else c
        bound = _t64(ref["rstd"]) * u * (cr + cv * _t64(ref["kappa"]))
    else:
        fixed, t = _ln_parts(what, ref, storage_dtype, decode)
        bound = fixed + (globals()[_LN_C[what]] if c is None else c) * u * t
    worst, i = _elem_ratio(got, ref[what], bound)
    _report("elem", worst)
    return worst <= 1.0, worst, tuple(int(x) for x in np.unravel_index(i, tuple(np.shape(ref[what]))))


def ln_excess(what, got, ref, storage_dtype=torch.float32, decode=False):
    """the quantity the constants bound: mean - |err| / (u t_mean); rstd - |err| / (u rstd* max(kappa, 1)); else (|err| - fixed) / (u terms)"""
    if what == "mean":
        return _excess(got, ref["mean"], ref["t_mean"], torch.zeros_like(_t64(ref["mean"])))
    if what == "rstd":
        return _excess(got, ref["rstd"], _t64(ref["rstd"]) * _t64(ref["kappa"]).clamp(min=1.0), torch.zeros_like(_t64(ref["rstd"])))
    fixed, t = _ln_parts(what, ref, storage_dtype, decode)
    return _excess(got, ref[what], t, fixed)
