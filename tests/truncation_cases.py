"""The truncation samplers' reference and the cases the tests share: a float64 numpy restatement of rules 1 - 7 of ff_sample_token_truncated
(include/flamingo_fusion.h), applied to the logits exactly as stored (bf16 values are widened, never re-rounded); the placement helpers; the
designed cases of tests/test_hip_truncation.py; and a float32 restatement of what csrc/ff_truncate.hip computes over a kept set, in the
kernel's summation order (tools/truncation_c.py measures the constants below with it).

A sampled token is a discontinuous function of its inputs, so the tests never compare near a decision.  There are three kinds of decision:
  mass      the nucleus and the typical band compare a partial mass with top_p / typical_p.  As in tests/test_hip_sampling.py the parameter is
            PLACED in the middle of the mass interval of a distinct-value group of mass >= GROUP_MASS, so every decision is >= 1e-3 away
            (an fp32 sum of V <= 70001 positive terms carries about 1.7e-5).
  relative  min_p, epsilon and eta compare a column's probability with a threshold.  The threshold is placed between two adjacent distinct
            probabilities, and no compared probability may lie within REL_MARGIN (relative) of it.
  entropy   typical_p orders the columns by |-log r - H| and eta's threshold is sqrt(eta) exp(-H): the kept set must be IDENTICAL when H is
            replaced by H + DELTA_H and by H - DELTA_H (and every other margin must hold in all three evaluations).
REL_MARGIN and DELTA_H are 8 x what tools/truncation_c.py measures (the float32 restatement against float64 over all designed cases):
    largest relative probability error 1.83e-6  (mostly the fast exponential's argument, z' log2 e rounded to float32, at z' near -18)
    largest |dH| (entropy centre and a column's distance d) 1.53e-6 nats
(the estimate before the measurement was 2e-5 and a few 1e-4 - worst-case bounds; the errors of the measured sums largely cancel)."""
import numpy as np
import torch

BF16, F32 = torch.bfloat16, torch.float32
GROUP_MASS = 2e-3        # least mass of the distinct-value group top_p / typical_p is placed in
TOKEN_MASS = 2e-3        # least kept-normalised probability of a token u is placed on
REL_MARGIN = 8 * 1.83e-6  # measured 1.83e-6 (tools/truncation_c.py)
DELTA_H = 8 * 1.53e-6     # measured 1.53e-6 nats (tools/truncation_c.py)
OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
RULES = tuple(OFF)
f32 = lambda v: float(np.float32(v))


def _groups(key, w):
    """distinct values of `key`, ascending: (index of each element's group, mass per group, mass of the groups in front of each group)"""
    vals, inv = np.unique(key, return_inverse=True)
    gm = np.bincount(inv.reshape(-1), weights=w, minlength=vals.size)
    return inv.reshape(-1), gm, np.concatenate([[0.0], np.cumsum(gm)[:-1]])


class Chain:
    """One row x (float64, as stored) under (T, k): K = the kept set so far (K0 after the constructor), e = exp(z - max z).  Every stage
    method applies one rule to K and appends (stage, kind, margin) to `margins`; `dH` is added to the entropy wherever one is used."""

    def __init__(self, x, T=1.0, k=0, dH=0.0):
        x = np.asarray(x, dtype=np.float64)
        self.x, self.V, self.T, self.dH, self.margins = x, x.size, T, dH, []
        finite = x > -np.inf
        self.K = (x >= np.sort(x)[self.V - k]) & finite if 0 < k < self.V else finite.copy()
        z = x / T
        with np.errstate(invalid="ignore", over="ignore"):
            self.e = np.where(finite, np.exp(z - z[self.K].max()), 0.0)
        self.z = z

    # ---- what the stages share ----
    def r(self):
        """q renormalised over K (0 outside)"""
        w = np.where(self.K, self.e, 0.0)
        return w / w.sum()

    def entropy(self):
        r = self.r()[self.K]
        return float(-(r[r > 0] * np.log(r[r > 0])).sum()) + self.dH

    def _mass_groups(self, key):
        idx = np.nonzero(self.K)[0]
        return (idx,) + _groups(key[idx], self.r()[idx])

    def _mass_rule(self, stage, key, p):
        """keeps the columns whose groups in front (smaller key) hold a mass < p"""
        idx, inv, gm, above = self._mass_groups(key)
        self.margins.append((stage, "mass", float(np.abs(above - p).min())))
        K = np.zeros(self.V, dtype=bool)
        K[idx[above[inv] < p]] = True
        self.K = K

    def _place_mass(self, key, near, accept=lambda p: True):
        idx, inv, gm, above = self._mass_groups(key)
        mid = above + 0.5 * gm
        ok = np.nonzero(gm >= GROUP_MASS)[0]
        assert ok.size > 0, "no distinct-value group heavy enough to place the parameter in"
        for g in ok[np.argsort(np.abs(mid[ok] - near))]:
            p = f32(mid[g])
            if 0 < p < 1 and np.abs(above - p).min() >= 0.5 * GROUP_MASS * (1 - 1e-6) and accept(p):
                return p
        raise AssertionError("no distinct-value group to place the parameter in")

    def _prob_rule(self, stage, prob, thr, keep_top):
        idx = np.nonzero(self.K)[0]
        keep = prob[idx] >= thr
        if keep_top:
            keep |= self.x[idx] == self.x[idx].max()
        self.margins.append((stage, "relative", float(np.abs(prob[idx] / thr - 1).min())))
        K = np.zeros(self.V, dtype=bool)
        K[idx[keep]] = True
        self.K = K

    def _place_prob(self, prob, near, accept=lambda t: True):
        """a threshold between two adjacent distinct probabilities of K that are at least (1 + 4 REL_MARGIN)^2 apart: the one nearest `near`
        (None: nearest the lower quartile of the distinct probabilities, so that about a quarter of the distinct values is cut) that `accept`
        takes"""
        pv = np.unique(prob[self.K])
        pv = pv[pv > 0]
        if pv.size < 2:
            return 0.5 * float(pv[0])
        mids, gap = np.sqrt(pv[1:] * pv[:-1]), pv[1:] / pv[:-1]
        want = np.log(near) if near is not None else np.log(mids[mids.size // 4])
        for j in np.argsort(np.abs(np.log(mids) - want)):
            if gap[j] >= (1 + 4 * REL_MARGIN) ** 2 and accept(float(mids[j])):
                return float(mids[j])
        raise AssertionError("no gap between adjacent probabilities wide enough to place a threshold in")

    def _stable(self, rule, value):
        """the rule gives the same kept set at H, H + DELTA_H and H - DELTA_H, its margin held in all three"""
        Ks = []
        for s in (0, 1, -1):
            c = Chain.__new__(Chain)
            c.__dict__.update(self.__dict__, dH=s * DELTA_H, margins=[])
            getattr(c, rule)(value)
            if any(m < (0.5 * GROUP_MASS * (1 - 1e-6) if kind == "mass" else REL_MARGIN) for _, kind, m in c.margins):
                return False
            Ks.append(c.K)
        return all(np.array_equal(K, Ks[0]) for K in Ks[1:])

    # ---- the rules ----
    def nucleus(self, p):
        if p < 1:
            self._mass_rule("top_p", -self.x, p)
        return self

    def place_p(self, near=0.7):
        return self._place_mass(-self.x, near)

    def min_p(self, m):
        if m > 0:
            self._prob_rule("min_p", self.e, m, False)
        return self

    def place_min_p(self, near=0.05):
        return f32(min(self._place_prob(self.e, near), 1.0))

    def _d(self):
        with np.errstate(divide="ignore"):
            return np.abs(-np.log(self.r()) - self.entropy())

    def typical(self, tp):
        if tp < 1:
            self._mass_rule("typical_p", self._d(), tp)
        return self

    def place_typical(self, near=0.7):
        return self._place_mass(self._d(), near, accept=lambda p: self._stable("typical", p))

    def epsilon(self, eps):
        if eps > 0:
            self._prob_rule("epsilon_cutoff", self.r(), eps, True)
        return self

    def place_epsilon(self, near=3e-4):
        return f32(self._place_prob(self.r(), near, accept=lambda t: t < 0.999))

    def eta_star(self, eta):
        return min(eta, np.sqrt(eta) * np.exp(-self.entropy()))

    def eta(self, eta):
        if eta > 0:
            self._prob_rule("eta_cutoff", self.r(), self.eta_star(eta), True)
        return self

    def place_eta(self, near=2e-3):
        """eta whose eta* = min(eta, sqrt(eta) exp(-H)) is the placed threshold t: eta = t where sqrt(t) <= exp(-H), else (t exp(H))^2"""
        eH = np.exp(-self.entropy())
        inv = lambda t: t if np.sqrt(t) <= eH else (t / eH) ** 2
        return f32(inv(self._place_prob(self.r(), near, accept=lambda t: inv(t) < 0.999 and self._stable("eta", f32(inv(t))))))

    # ---- rule 7 ----
    def cdf(self):
        r = self.r()
        return self.K, r, np.cumsum(r)

    def token(self, u):
        P, r, c = self.cdf()
        hit = np.nonzero(P & (c > u))[0]
        return int(hit[0]) if hit.size else int(np.nonzero(P)[0][-1])

    def place_u(self):
        """[(u, token)]: u in the middle of the CDF interval of the first, the heaviest and the last (in index order) kept token whose
        kept-normalised probability is >= TOKEN_MASS (tests/test_hip_sampling.py's Ref.place_u over K5)"""
        P, r, c = self.cdf()
        heavy = np.nonzero(P & (r >= TOKEN_MASS))[0]
        assert heavy.size > 0, "no kept token heavy enough to place u on"
        out = []
        for i in (heavy[0], heavy[np.argmax(r[heavy])], heavy[-1]):
            u = f32(c[i] - 0.5 * r[i])
            assert r[i] >= TOKEN_MASS and c[i] - r[i] + 0.25 * r[i] < u < c[i] - 0.25 * r[i] and 0 <= u < 1
            assert self.token(u) == i
            out.append((u, int(i)))
        return out


def chain(x, T, k, p, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, dH=0.0):
    """rules 1 - 6 on one row: the Chain whose K is K5"""
    return Chain(x, T, k, dH).nucleus(p).min_p(min_p).typical(typical_p).epsilon(epsilon_cutoff).eta(eta_cutoff)


def decidable(x, T, k, p, tr, mass_edge=0.5 * GROUP_MASS * (1 - 1e-6), u=None):
    """(ok, the Chain at dH = 0).  ok: every mass decision is >= mass_edge and every probability decision >= REL_MARGIN (relative) away, at
    H, H + DELTA_H and H - DELTA_H, the three kept sets are identical, and - with `u` - u is >= mass_edge from every end of a CDF interval."""
    base = chain(x, T, k, p, **tr)
    runs = [base] + ([chain(x, T, k, p, dH=s * DELTA_H, **tr) for s in (1, -1)] if tr["typical_p"] < 1 or tr["eta_cutoff"] > 0 else [])
    ok = all(m >= (mass_edge if kind == "mass" else REL_MARGIN) for c in runs for _, kind, m in c.margins)
    ok = ok and all(np.array_equal(c.K, base.K) for c in runs[1:])
    if ok and u is not None:
        P, _, c = base.cdf()
        ok = np.abs(np.concatenate([[0.0], c[P]]) - u).min() >= mass_edge
    return bool(ok), base


def place(x, T, k, p, rules, near=None):
    """(top_p, {the four parameters}): top_p placed when `p` is None, then every rule named in `rules` placed in turn on the set the earlier
    ones leave (`near`: rule or "top_p" -> target; with more than one rule the epsilon and eta thresholds default to the lower quartile of
    what is left, so that every stage cuts and leaves something to cut).  The parameters are float32 values, and the chain they were placed on used those."""
    near = dict(near or {})
    c = Chain(x, T, k)
    if p is None:
        p = c.place_p(near.get("top_p", 0.95 if rules else 0.7))          # (a wide nucleus: the rules behind it need something to cut)
    c.nucleus(p)
    tr = dict(OFF)
    many = len(rules) > 1
    for name, placer, apply, one, chained in (("min_p", c.place_min_p, c.min_p, 0.05, 0.05), ("typical_p", c.place_typical, c.typical, 0.7, 0.9),
                                              ("epsilon_cutoff", c.place_epsilon, c.epsilon, 3e-4, None), ("eta_cutoff", c.place_eta, c.eta, 2e-3, None)):
        if name in rules:
            tr[name] = placer(near.get(name, chained if many else one))
            apply(tr[name])
    return p, tr


# ---------------------------------------------------------------------------------------------------------------------------------------
# the designed cases of tests/test_hip_truncation.py
# ---------------------------------------------------------------------------------------------------------------------------------------
SHAPES = {
    "b32-V50258-bf16": (32, 50258, BF16, "contiguous"),
    "b7-V50258-bf16-last-of-3": (7, 50258, BF16, "last-of-3"),
    "b1-V65536-bf16": (1, 65536, BF16, "contiguous"),
    "b2-V70001-bf16": (2, 70001, BF16, "contiguous"),
    "b5-V1000-f32": (5, 1000, F32, "contiguous"),
    "b2-V7-f32": (2, 7, F32, "contiguous"),
    "b1-V1-f32": (1, 1, F32, "contiguous"),
}
# name -> (T, top_k, top_p (None: placed per row), the rules that are on)
SETTINGS = {
    "min_p": (1.0, 0, 1.0, ("min_p",)),
    "typical_p": (1.0, 0, 1.0, ("typical_p",)),
    "epsilon_cutoff": (1.0, 0, 1.0, ("epsilon_cutoff",)),
    "eta_cutoff": (1.0, 0, 1.0, ("eta_cutoff",)),
    "all-four": (1.0, 0, 1.0, RULES),
    "all-four-T0.7-k50-p": (0.7, 50, None, RULES),
}


def make_logits(rows, V, dtype, seed, scale=4.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, V), generator=g, dtype=torch.float32) * scale).to(dtype)


def shape_logits(shape):
    rows, V, dtype, _ = SHAPES[shape]
    return make_logits(rows, V, dtype, seed=2000 + V + rows)


def designed_case(shape, setting):
    """[(row, top_p, {parameters}, [(u, token) x 3])] for every row of the shape under the setting, preconditions asserted"""
    T, k, p_set, rules = SETTINGS[setting]
    x64 = shape_logits(shape).double().numpy()
    out = []
    for r in range(x64.shape[0]):
        p, tr = place(x64[r], T, k, p_set, rules)
        ok, c = decidable(x64[r], T, k, p, tr)
        assert ok, (shape, setting, r, p, tr, c.margins)
        out.append((r, p, tr, c.place_u()))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# float32 restatement of the kernel's sums (tools/truncation_c.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
def thread_order(V, elems, staged, head=0):
    """(256, L) column indices, -1 = none: the columns thread t of RowKeys::each adds up, in its order.  staged: 16-byte vectors of 8 keys,
    thread t takes the vectors t, t + 256, ...; otherwise for_row_vectors4: `head` scalar columns, vectors of `elems`, the scalar tail."""
    n = elems if not staged else 8
    head = 0 if staged else min(head, V)
    nvec = (V + 7) // 8 if staged else (V - head) // n
    M = (nvec + 255) // 256
    vec = (np.arange(M)[None, :, None] * 256 + np.arange(256)[:, None, None]) * n + np.arange(n)[None, None, :] + head      # (256, M, n)
    vec = np.where((vec < head + nvec * n) & (vec < V), vec, -1).reshape(256, M * n)
    tail0 = head + nvec * n
    Lt = (max(V - tail0, 0) + 255) // 256
    tail = tail0 + np.arange(256)[:, None] + 256 * np.arange(Lt)[None, :]
    tail = np.where(tail < V, tail, -1)
    hd = np.where(np.arange(256) < head, np.arange(256), -1)[:, None]
    return np.concatenate([hd, vec, tail], axis=1)


def block_sum_f32(vals, order):
    """the kernel's sum of `vals` (V,) float32: thread-local in column order, xor butterfly in each wave, wave 0..3"""
    v = np.concatenate([vals.astype(np.float32), np.zeros(1, np.float32)])[order]          # (index -1: the appended 0)
    s = np.zeros(256, np.float32)
    for i in range(v.shape[1]):
        s = s + v[:, i]
    lane = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[lane ^ o]
    out = np.float32(0)
    for w in range(4):
        out = out + s[64 * w]
    return out


def kernel_terms_f32(x, T):
    """(z', w) as the kernel forms them from the stored values: z' = (x - max x) * (1 / T) and the fast exponential exp2(z' * log2 e), every
    step rounded to float32"""
    x32 = np.asarray(x, np.float32)
    inv_t = np.float32(1) / np.float32(T)
    with np.errstate(invalid="ignore"):
        z = (x32 - x32.max()) * inv_t
        w = np.exp2((z * np.float32(1.4426950408889634)).astype(np.float64)).astype(np.float32)
    return z, w


def stage_errors(x, T, K, order):
    """over the kept set K: (largest relative error of w / Z among the columns with r >= 1e-8, |A32 - A64|, the largest |d32 - d64| among
    them), A = sum w z' / Z the entropy centre, d = |A - z'|"""
    x = np.asarray(x, np.float64)
    z64 = np.where(K, (x - x.max()) / T, 0.0)                         # (both sides measure z' from the ROW's maximum, kept or not)
    w64 = np.where(K, np.exp(z64), 0.0)
    Z64 = w64.sum()
    A64 = (w64[K] * z64[K]).sum() / Z64
    z, w = kernel_terms_f32(x, T)
    z, w = np.where(K, z, np.float32(0)), np.where(K, w, np.float32(0))
    Z32 = block_sum_f32(w, order)
    A32 = block_sum_f32(w * z, order) / Z32
    big = K & (w64 / Z64 >= 1e-8)
    rel = np.abs((w[big].astype(np.float64) / float(Z32)) / (w64[big] / Z64) - 1).max()
    dd = np.abs(np.abs(A32 - z[big]).astype(np.float64) - np.abs(A64 - z64[big])).max()
    return float(rel), float(abs(float(A32) - A64)), float(dd)
