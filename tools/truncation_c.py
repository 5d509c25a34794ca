"""The constants of tests/truncation_cases.py (REL_MARGIN, DELTA_H), measured on the CPU: the float32 restatement of what
csrc/ff_truncate.hip computes over a kept set - z' = (x - max x) * (1 / T), the fast exponential, Z = sum w and S1 = sum w z' in the kernel's
summation order (thread-local in column order, xor butterfly, wave 0..3), A = S1 / Z, d = |A - z'| - against float64, over every row of
every designed case of tests/test_hip_truncation.py and every kept set a stage of the kernel sums over (K1 for min_p's weights, K2 for
typical_p, K3 for epsilon_cutoff, K4 for eta_cutoff).  Prints per case and overall
    rel    the largest relative error of a compared probability (w for min_p, w / Z for epsilon and eta), columns with r >= 1e-8
    dH     the largest error of the entropy centre A (= log Z - H) and of a column's distance d, in nats
REL_MARGIN and DELTA_H are 8 x the overall figures.
    python tools/truncation_c.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import truncation_cases as tc  # noqa: E402


def row_order(shape, r):
    """the summation order of row r of the shape as the test lays it out (rows are element-aligned only: the scalar head differs per row)"""
    rows, V, dtype, layout = tc.SHAPES[shape]
    size = 2 if dtype == tc.BF16 else 4
    staged = dtype == tc.BF16 and V <= 65536
    start = ((3 * r + 2) * V if layout == "last-of-3" else r * V) * size
    return tc.thread_order(V, 16 // size, staged, head=((16 - start % 16) % 16) // size)


def case_errors(shape, setting):
    T, k, _, rules = tc.SETTINGS[setting]
    x64 = tc.shape_logits(shape).double().numpy()
    rel = dh = 0.0
    for r, p, tr, _ in tc.designed_case(shape, setting):
        x, order = x64[r], row_order(shape, r)
        c = tc.Chain(x, T, k).nucleus(p)
        if "min_p" in rules:                                             # the weight alone is compared
            z, w = tc.kernel_terms_f32(x, T)
            big = c.K & (c.e >= 1e-8)
            rel = max(rel, float(np.abs(w[big].astype(np.float64) / c.e[big] - 1).max()))
        c.min_p(tr["min_p"])
        for name, apply in (("typical_p", c.typical), ("epsilon_cutoff", c.epsilon), ("eta_cutoff", c.eta)):
            if name in rules:
                e_rel, e_a, e_d = tc.stage_errors(x, T, c.K, order)
                if name != "typical_p":
                    rel = max(rel, e_rel)
                if name != "epsilon_cutoff":
                    dh = max(dh, e_a, e_d)
            apply(tr[name])
    return rel, dh


if __name__ == "__main__":
    top_rel = top_dh = 0.0
    for shape in tc.SHAPES:
        for setting in tc.SETTINGS:
            rel, dh = case_errors(shape, setting)
            top_rel, top_dh = max(top_rel, rel), max(top_dh, dh)
            print(f"{shape:26s} {setting:22s} rel {rel:.2e}  dH {dh:.2e}")
    print(f"largest relative probability error {top_rel:.2e}; largest |dH| {top_dh:.2e} nats")
    print(f"REL_MARGIN = 8 x {top_rel:.2e} = {8 * top_rel:.2e}; DELTA_H = 8 x {top_dh:.2e} = {8 * top_dh:.2e}")
