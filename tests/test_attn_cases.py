"""The attention checkers' own tests, on the CPU: the case table of tests/attn_cases.py has the properties the GPU tests rely on, the
restatements of the kernels pass util.attn_bound_ok at every case, and each of eight injected defects fails its bound, in fp32 and in
bf16, by a wide margin, at the element where it was injected.  Smallest margin over all of them: 35.6 x the bound (bf16, D left at 0 for one query, d q),
then 39.4 x (bf16, a key tile skipped for one row); in fp32 1675 x and more."""
import numpy as np
import pytest
import torch

import attn_cases as ac
from util import ATTN_C_G, ATTN_C_L, ATTN_C_O, attn_bound_ok

BF16, F32 = ac.BF16, ac.F32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
OUTPUTS = ("lse", "o", "dq", "dk", "dv")
_REF = {}


def restated(case, mutate=None, **kw):
    fwd = mutate if mutate in ("skip-tile", "no-rescale", "lse-log2", "range-shift", "zero-1e-30") else None
    bwd = mutate if mutate in ("D-zero", "dk-miss-qtile", "uniform-dq", "range-shift") else None
    o, lse = ac.attn_fwd_f32(case.q, case.k, case.v, case.tt, case.n_visual, mutate=fwd, **kw)
    dq, dk, dv = ac.attn_bwd_f32(case.q, case.k, case.v, o, case.do, lse, case.tt, case.n_visual, mutate=bwd, **kw)
    return dict(zip(OUTPUTS, (lse, o, dq, dk, dv)))


def ref_of(case):
    """one float64 reference per case, shared by the tests of this module and left unchanged"""
    if case.name not in _REF:
        _REF[case.name] = case.ref()
    return _REF[case.name]


def dense(dtype, pattern, dh=64, shape=(130, 200)):
    return ac.make_case(dtype, dh, shape[0], shape[1], pattern)


def media(dtype, pattern, nv=40, n_media=4, dh=64):
    return ac.make_case(dtype, dh, ac.MEDIA_NQ, nv * n_media, pattern, ac.media_text_time(ac.MEDIA_NQ, n_media), nv)


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_four_times_the_measured_excess():
    """tools/attn_c.py's figures (the comment above ATTN_C_L in util.py): lse 5.77, o 5.48, gradients 6.81"""
    assert (ATTN_C_L, ATTN_C_O, ATTN_C_G) == (23.1, 21.9, 27.2)


@pytest.mark.parametrize("dtype,dh", ac.DENSE_INST, ids=[f"{ac.name_of(t)}-{d}" for t, d in ac.DENSE_INST])
def test_sharp_tied_and_offset_cases_are_what_they_claim(dtype, dh):
    n_q, n_kv = 130, 200
    for pattern in ac.SHARP:
        case = dense(dtype, pattern, dh)
        p = ref_of(case)["p"]
        top = p.max(-1)
        rest = np.where(p == top[..., None], 0.0, p).max()
        assert top.min() > 1 - 2.0 ** -20 and rest < 2.0 ** -126, (case.name, top.min(), rest)
        assert np.abs(ref_of(case)["s"]).max() < 4000, case.name
        j = p.argmax(-1)
        want = ac.dominant_keys(pattern, n_q, np.zeros((ac.B, n_q), int), np.full((ac.B, n_q), n_kv))
        assert (j == want[:, None, :]).all(), case.name
    rows = ac.dominant_keys("sharp-rows", n_q, np.zeros((1, n_q), int), np.full((1, n_q), n_kv))[0]
    assert ac.dominant_keys("sharp-first", n_q, np.zeros((1, n_q), int), np.full((1, n_q), n_kv)).max() == 0
    assert set(ac.dominant_keys("sharp-mid", n_q, np.zeros((1, n_q), int), np.full((1, n_q), n_kv))[0] // ac.TILE) == {1}
    assert set(ac.dominant_keys("sharp-last", n_q, np.zeros((1, n_q), int), np.full((1, n_q), n_kv))[0]) == {n_kv - 1}
    for w in range(0, n_q - 15, 16):                 # every wave: 16 different keys, in three or all four of the key tiles (the last holds 8 keys)
        assert len(set(rows[w:w + 16])) == 16 and {0, 1, 2} <= set(rows[w:w + 16] // ac.TILE)
    case = dense(dtype, "tied", dh)
    p = np.sort(ref_of(case)["p"], axis=-1)
    assert (p[..., -1] + p[..., -2]).min() > 1 - 2.0 ** -20 and p[..., -3].max() < 2.0 ** -126
    j = np.argsort(ref_of(case)["p"], axis=-1)[..., -2:]
    assert (np.sort(j, axis=-1) == np.array([3, n_kv - 2])).all() and 3 // ac.TILE != (n_kv - 2) // ac.TILE
    near = p[..., -2] > 0.05                         # the smaller of the two still carries weight: on all rows in fp32; the bf16 grid of q
    assert near.mean() > (0.99 if dtype == F32 else 0.3), near.mean()           # moves a score of 300 by about 1
    for pattern, sign in (("offset+", 1), ("offset-", -1)):
        s = ref_of(dense(dtype, pattern, dh))["s"]
        assert (sign * s).min() > 100 and (sign * s).max() < 300 and ref_of(dense(dtype, pattern, dh))["p"].max() < 0.9
    case = dense(dtype, "scales", dh)
    qn, dn = case.q.double().norm(dim=-1)[0, :64, 0].numpy(), case.do.double().norm(dim=-1)[0, :64, 0].numpy()
    assert (qn == 0).sum() >= 12 and (qn > 15).sum() >= 12 and ((qn > 0) & (qn < 0.01)).sum() >= 12 and (dn > 100).sum() >= 20
    p = ref_of(case)["p"][0, 0, :5]
    assert np.allclose(p[0], 1.0 / n_kv, rtol=1e-12, atol=0) and p[4].max() > 0.5 and p[2].max() < 0.2


@pytest.mark.parametrize("nv,n_media", ac.MEDIA_KEYS)
def test_media_text_time_mixes_all_row_kinds_in_one_block(nv, n_media):
    n_q, n_kv = ac.MEDIA_NQ, nv * n_media
    tt = ac.media_text_time(n_q, n_media)
    lo, hi, sm, un = ac.row_ranges(tt, n_q, n_kv, nv)
    kinds = ref_of(media(F32, "flat", nv, n_media, 16))["kinds"]
    assert n_q > 2 * ac.TILE and n_q % ac.TILE != 0
    for s in range(ac.B):
        assert {n_media + 1, n_media + 3} <= set(tt[s, :64].tolist())
        for w in range(0, 64, 16):                   # every wave of the first workgroup: zero rows, uniform rows and every image
            t = tt[s, w:w + 16]
            assert (t == 0).any() and (t > n_media).any() and set(range(1, n_media + 1)) <= set(t.tolist()), (s, w, t)
        assert set(kinds[s, :64].tolist()) == {0, 1, 2}
        assert (kinds[s, 64:128] == 0).all() and (tt[s, 128:] == n_media).all() and (kinds[s, 128:] == 1).all()
        assert ((kinds[s] == 1) == (sm[s] == 1)).all() and ((kinds[s] == 2) == (un[s] == 1)).all()
        seen = ref_of(media(F32, "flat", nv, n_media, 16))["seen"][s, 0]
        key = np.arange(n_kv)[None, :]
        assert (seen == ((key >= lo[s][:, None]) & (key < hi[s][:, None]))).all()          # the kernel's ranges are the oracle's masks
    ranges = {(int(a), int(b)) for a, b in zip(lo[sm == 1], hi[sm == 1])}
    assert len(ranges) == n_media
    if nv == 8:
        assert all(a // 16 == (b - 1) // 16 for a, b in ranges)                                # inside one MFMA sub-block
    if nv == 40:
        assert any(a // 64 != (b - 1) // 64 for a, b in ranges) and all(a // 16 != (b - 1) // 16 for a, b in ranges)
    if nv == 72:
        assert all(b - a > 64 for a, b in ranges) and all((b - 1) // 64 - a // 64 == 1 for a, b in ranges)    # longer than a tile, over two tiles


def test_media_sharp_rows_are_sharp_inside_their_image():
    for dtype in (F32, BF16):
        case = media(dtype, "sharp-rows")
        r = ref_of(case)
        p = r["p"][np.broadcast_to((r["kinds"] == 1)[:, None], r["p"].shape[:3])]
        top = p.max(-1)
        assert top.min() > 1 - 2.0 ** -20 and np.where(p == top[:, None], 0.0, p).max() < 2.0 ** -126


# ---- the restatement passes --------------------------------------------------------------------------------------------------------------
def _all_hold(case):
    ref, got = ref_of(case), restated(case)
    for what in OUTPUTS:
        ok, worst, idx = attn_bound_ok(what, got[what], ref, case.dtype)
        assert ok, f"{case.name}: {what} element {idx} is {worst:.4g} x its bound"


@pytest.mark.parametrize("dtype,dh", ac.DENSE_INST, ids=[f"{ac.name_of(t)}-{d}" for t, d in ac.DENSE_INST])
def test_restatement_within_the_bounds_dense(dtype, dh):
    for case in ac.dense_cases(dtype, dh):
        _all_hold(case)


@pytest.mark.parametrize("dtype,dh", ac.MEDIA_INST, ids=[f"{ac.name_of(t)}-{d}" for t, d in ac.MEDIA_INST])
def test_restatement_within_the_bounds_media(dtype, dh):
    for case in ac.media_cases(dtype, dh):
        _all_hold(case)
        ref, got = ref_of(case), restated(case)
        zero, uni = torch.from_numpy(ref["kinds"] == 0), torch.from_numpy(ref["kinds"] == 2)
        assert int((got["o"][zero] != 0).sum()) == 0 and int((got["dq"][zero] != 0).sum()) == 0 and int((got["dq"][uni] != 0).sum()) == 0
        assert bool((got["lse"].permute(0, 2, 1)[zero] == float(ac.POS_BIG)).all())


# ---- injected defects ---------------------------------------------------------------------------------------------------------------------
def _first(kinds, kind, sample=1):
    return int(np.nonzero(kinds[sample] == kind)[0][0])


DEFECTS = [
    # (defect, case, what must fail, keyword arguments, which element must be named: a function of (index, reference))
    ("skip-tile", lambda t: dense(t, "flat"), "o", dict(at=(1, 2, 70), tile=2), lambda i, r: i[:3] == (1, 70, 2)),
    ("no-rescale", lambda t: dense(t, "sharp-last"), "o", {}, lambda i, r: True),
    ("lse-log2", lambda t: dense(t, "flat"), "lse", dict(at=(1, 2, 70)), lambda i, r: i == (1, 2, 70)),
    ("range-shift", lambda t: media(t, "flat"), "o", {}, lambda i, r: r["kinds"][i[0], i[1]] == 1),
    ("D-zero", lambda t: dense(t, "tied"), "dq", dict(at=(1, 2, 70)), lambda i, r: i[:3] == (1, 70, 2)),
    ("dk-miss-qtile", lambda t: dense(t, "flat"), "dk", dict(tile=1), lambda i, r: True),
    ("uniform-dq", lambda t: media(t, "flat"), "dq", {}, lambda i, r: r["kinds"][i[0], i[1]] == 2),
    ("zero-1e-30", lambda t: media(t, "flat"), "o", dict(at=(1, 0, 0)), lambda i, r: i[:2] == (1, _first(r["kinds"], 0))),
]
MARGINS = {}


@DTYPES
@pytest.mark.parametrize("defect,make,what,kw,named", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_injected_defect_fails_its_bound(dtype, defect, make, what, kw, named):
    case = make(dtype)
    ref = ref_of(case)
    good, bad = restated(case), restated(case, defect, **kw)
    assert attn_bound_ok(what, good[what], ref, dtype)[0]
    ok, worst, idx = attn_bound_ok(what, bad[what], ref, dtype)
    print(f"{ac.name_of(dtype)} {defect}: {what} element {idx} is {worst:.4g} x its bound")
    MARGINS[(ac.name_of(dtype), defect)] = worst
    assert not ok and worst >= 10.0, (defect, worst)
    assert named(idx, ref), (defect, idx)
    if defect in ("skip-tile", "D-zero", "lse-log2"):          # one row was touched: every other row of that output is bit for bit as before
        a, b = good[what].clone(), bad[what].clone()
        row = kw["at"] if what == "lse" else (kw["at"][0], kw["at"][2], kw["at"][1])
        a[row], b[row] = 0, 0
        assert torch.equal(a, b)
