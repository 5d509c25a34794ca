"""The constant of tests/util.py's adamw_bound_ok, measured on the CPU: the float32 restatement of the AdamW kernel (tests/optim_cases.py:
adamw_f32_step) against the float64 step (util.adamw_ref_step) at the inputs of tests/test_hip_optim_bounds.py - every storage mode,
both hyper-parameter sets, unclipped and clipped, steps 1 to 3 from zero state, step 1000 from the loaded state, and the graph test's
four steps with its learning rates; then the same at the inputs of the two parity tests that check every step too
(test_hip_optim.py::test_fused_adamw_matches_oracle_and_torch, test_hip_grad_clip.py::test_fused_adamw_clipped_matches_oracle_and_torch:
normal parameters, four steps), whose constant is util.ADAMW_C_PARITY.  Prints the worst excess (util.adamw_excess) per case and overall, and the smallest fraction of
elements per tensor (>= 64 elements) whose reference result differs from the stored old value (the tests' non-vacuity condition, >= 0.25).
    python tools/adamw_c.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import optim_cases as oc  # noqa: E402
from util import adamw_excess, adamw_ref_step, rnd  # noqa: E402

OWN, SEG = oc.owned(), oc.segments()


def run(mode, hpn, clipped, first, lrs):
    hp = dict(oc.HP[hpn])
    T, ST, master = oc.MODES[mode]
    p = torch.from_numpy(oc.p_values(1))[OWN].to(T)
    if first > 1:
        m, v = (torch.from_numpy(x).to(ST) for x in oc.injected_state(hp, p.numel()))
    else:
        m, v = torch.zeros(p.numel(), dtype=ST), torch.zeros(p.numel(), dtype=ST)
    w = p.float() if master else None
    worst, least = {}, 1.0
    for k, lr in enumerate(lrs):
        step = first + k
        hp["lr"] = lr
        g = torch.from_numpy(oc.values(100 + step, hp["g_scale"]))[OWN].to(T)
        coef = oc.clip_coef64(g, hp)[1] if clipped else 1.0
        refs, terms = adamw_ref_step(w if master else p, g, m, v, step, lr, *hp["betas"], hp["eps"], hp["weight_decay"], hp["grad_scale"], coef)
        new = oc.adamw_f32_step(p, g, m, v, w, step, hp, mode, clipped)
        for name, got, old, ref, t, sd in (("p", new[3] if master else new[0], w if master else p, refs[0], terms[0], torch.float32 if master else T),
                                           ("m", new[1], m, refs[1], terms[1], ST), ("v", new[2], v, refs[2], terms[2], ST)):
            worst[name] = max(worst.get(name, 0.0), adamw_excess(got, ref, t, sd))
            changed = ref.to(sd).double() != old.double()
            least = min([least] + [float(changed[a:b].double().mean()) for a, b in SEG if b - a >= 64])
        p, m, v, w = new
    return worst, least


def parity(shapes, mode, max_grad_norm):
    """the parity tests' inputs: rnd(shape, 10 + i) parameters, rnd(shape, 100 * step + i, 0.5) gradients, steps 1 to 4"""
    T, ST, master = oc.MODES[mode]
    hp = dict(lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05, grad_scale=1.0, max_grad_norm=max_grad_norm)
    clipped = max_grad_norm is not None
    p = torch.cat([torch.from_numpy(rnd(s, 10 + i)).reshape(-1) for i, s in enumerate(shapes)]).to(T)
    m = torch.zeros(p.numel(), dtype=ST)
    v, w = m.clone(), (p.float() if master else None)
    worst = {}
    for step in range(1, 5):
        g = torch.cat([torch.from_numpy(rnd(s, 100 * step + i, 0.5)).reshape(-1) for i, s in enumerate(shapes)]).to(T)
        coef = oc.clip_coef64(g, hp)[1] if clipped else 1.0
        refs, terms = adamw_ref_step(w if master else p, g, m, v, step, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], 1.0, coef)
        new = oc.adamw_f32_step(p, g, m, v, w, step, hp, mode, clipped)
        for name, got, ref, t, sd in (("p", new[3] if master else new[0], refs[0], terms[0], torch.float32 if master else T),
                                      ("m", new[1], refs[1], terms[1], ST), ("v", new[2], refs[2], terms[2], ST)):
            worst[name] = max(worst.get(name, 0.0), adamw_excess(got, ref, t, sd))
        p, m, v, w = new
    return worst


if __name__ == "__main__":
    top, low = 0.0, 1.0
    for mode in oc.MODES:
        for clipped in (False, True):
            cases = [(hpn, first, [oc.HP[hpn]["lr"]] * n) for hpn in oc.HP for first, n in ((1, 3), (1000, 1))] + [("A", 1, [oc.HP["A"]["lr"], 2e-3, 6e-3, 4e-3])]
            for hpn, first, lrs in cases:
                worst, least = run(mode, hpn, clipped, first, lrs)
                top, low = max(top, *worst.values()), min(low, least)
                print(f"{mode:14s} {'clipped  ' if clipped else 'unclipped'} set {hpn} steps {first}..{first + len(lrs) - 1}: excess "
                      + " ".join(f"{k} {x:6.2f}" for k, x in worst.items()) + f"   least changed fraction {least:.2f}")
    print(f"worst excess {top:.2f} -> c = 4 x = {4 * top:.1f}; least changed fraction {low:.2f}")
    top = 0.0
    cases = [("test_hip_optim", [(1,), (1280,), (513, 7), (5120, 1280), (64, 1024), (3,)], mode, None) for mode in ("f32", "bf16")] + \
            [("test_hip_grad_clip", [(1,), (3,), (513, 7), (8191,), (5120, 1280)], mode, c) for mode in ("f32", "bf16", "bf16-master") for c in (100.0, 1e5)]
    for name, shapes, mode, c in cases:
        worst = parity(shapes, mode, c)
        top = max(top, *worst.values())
        print(f"{name:18s} {mode:12s} max_grad_norm {c}: excess " + " ".join(f"{k} {x:7.2f}" for k, x in worst.items()))
    print(f"parity inputs: worst excess {top:.2f} -> c = 4 x = {4 * top:.1f}")
