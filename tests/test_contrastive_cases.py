"""The numpy float64 restatement of contrastive search (tests/contrastive_cases.py) on hand-computed cases, against
decoding.contrastive_select_torch / topk_logprobs_torch on the designed cases, and under injected defects: every wrong reading of the rules
listed in contrastive_cases.DEFECTS changes the outcome of at least one designed case, so the GPU tests that compare the kernel with the
restatement on those cases would catch a kernel that has it.  Every designed case is decidable - the best score leads the second by at
least MARGIN, or they are an exact designed tie -, asserted here, without a GPU."""
import numpy as np
import pytest
import torch

import contrastive_cases as CC

E = np.eye(4)


def hand_case(**over):
    """b = 1, k = 3, dim = 4, n = 3.  H = e0, e1, (e0 + e1) / sqrt 2 (unnormalised: 3 e0 + 3 e1).  Candidates: h0 = e0 (cos 1 with position 0),
    h1 = e2 (cos 0 with all), h2 = e0 + e2 (cos 1 / sqrt 2 with position 0, 1 / 2 with position 2).  p = 0.5, 0.3, 0.2."""
    c = dict(hidden=np.stack([E[0], E[2], E[0] + E[2]]), hist=np.stack([E[0], 2 * E[1], 3 * E[0] + 3 * E[1], 9 * E[3]])[None], mask=np.ones((1, 4), np.uint8),
             n=3, cand_tok=np.array([[11, 12, 13]]), cand_logp=np.log(np.array([[0.5, 0.3, 0.2]])), finished=np.array([False]), alpha=0.6, eos=12, pad=7)
    c.update(over)
    return c


def run(c, defect=None):
    return CC.select(c["hidden"], c["hist"], c["mask"], c["n"], c["cand_tok"], c["cand_logp"], c["finished"], c["alpha"], c["eos"], c["pad"], defect=defect)


def test_hand_computed_step():
    r = run(hand_case())
    want = np.array([0.4 * 0.5 - 0.6 * 1.0, 0.4 * 0.3 - 0.0, 0.4 * 0.2 - 0.6 / np.sqrt(2)])
    assert np.allclose(r["score"][0], want, atol=1e-15)
    assert r["sel"][0] == 1 and r["sel_row"][0] == 1 and r["next_tok"][0] == 12 and r["beam_idx"].tolist() == [1, 1, 1]
    assert np.isclose(r["logprob"][0], np.log(0.3)) and r["finished"][0]          # token 12 is eos
    assert np.array_equal(r["hist_row"][0], E[2]) and r["hist_pos"] == 3
    assert np.isclose(r["margin"][0], 0.12 - (0.08 - 0.6 / np.sqrt(2))) and not r["tie"][0]
    # the unread position 3 (n = 3) does not count: e3 would give candidate 1 no penalty either, but h = e3 shows it
    r = run(hand_case(hidden=np.stack([E[3], E[2], E[0]])))
    assert np.allclose(r["score"][0, 0], 0.4 * 0.5)
    # alpha = 0 is greedy over the candidates, alpha = 1 the least similar one (smallest c on a tie)
    assert run(hand_case(alpha=0.0))["sel"][0] == 0 and run(hand_case(alpha=1.0))["sel"][0] == 1
    # no live position: pen = 0
    assert np.allclose(run(hand_case(mask=np.zeros((1, 4), np.uint8)))["score"][0], [0.2, 0.12, 0.08])
    assert np.allclose(run(hand_case(n=0))["score"][0], [0.2, 0.12, 0.08])
    # a zero vector is clamped, not NaN
    assert np.allclose(run(hand_case(hidden=np.stack([0 * E[0], E[2], E[0]])))["score"][0, 0], 0.2)
    # a finished sequence: pad, 0, and the state still advances
    r = run(hand_case(finished=np.array([True])))
    assert r["next_tok"][0] == 7 and r["logprob"][0] == 0 and r["sel"][0] == 1 and np.array_equal(r["hist_row"][0], E[2]) and r["finished"][0]
    # dead candidates never win; all dead: c* = 0
    r = run(hand_case(cand_logp=np.array([[np.log(0.5), -np.inf, np.log(0.2)]])))
    assert r["score"][0, 1] == -np.inf and r["sel"][0] == 2
    r = run(hand_case(cand_logp=np.full((1, 3), -np.inf)))
    assert r["sel"][0] == 0 and r["logprob"][0] == -np.inf and r["margin"][0] == np.inf


def test_hand_computed_topk():
    x = np.array([[0.0, 2.0, 2.0, -np.inf, 1.0], [-np.inf, -np.inf, 3.0, -np.inf, -np.inf], [1.0, 1.0, 1.0, 1.0, 1.0]])
    tok, lp = CC.topk_logprobs(x, 3)
    assert tok[0].tolist() == [1, 2, 4] and tok[2].tolist() == [0, 1, 2] and tok[1, 0] == 2
    lse0 = np.log(1 + 2 * np.exp(2) + np.exp(1))
    assert np.allclose(lp[0], [2 - lse0, 2 - lse0, 1 - lse0]) and np.allclose(lp[2], -np.log(5))
    assert lp[1, 0] == 0 and (lp[1, 1:] == -np.inf).all() and ((tok >= 0) & (tok < 5)).all()
    t2, l2 = (t.numpy() for t in __import__("flamingo_mini_amd").decoding.topk_logprobs_torch(torch.from_numpy(x), 3))
    assert np.array_equal(t2[np.isfinite(lp)], tok[np.isfinite(lp)]) and np.allclose(l2[np.isfinite(lp)], lp[np.isfinite(lp)]) and (l2[~np.isfinite(lp)] == -np.inf).all()


# ---- designed cases: decidable, and equal to the torch restatement --------------------------------------------------------------------
DESIGNED = [dict(b=3, k=k, dim=dim, n=n, max_len=48, dtype=dtype, seed=k * dim + n, left_pad=(1,), dead=(0,), tie=(2,))
            for dtype in ("bf16", "fp32") for k in (2, 3, 8) for dim in (64, 100, 768) for n in (1, 7, 40)] + \
           [dict(b=3, k=3, dim=64, n=4095, max_len=4096, dtype="bf16", seed=11, left_pad=(0,), tie=(1,)),
            dict(b=3, k=4, dim=768, n=23, max_len=32, dtype="fp32", seed=12, all_dead=(1,), finished=(0,), eos_seq=(2,), dead=(0,))]


@pytest.fixture(scope="module")
def designed():
    return [CC.design_step(**kw) for kw in DESIGNED]


def test_designed_cases_are_decidable_and_equal_the_torch_restatement(designed):
    from flamingo_mini_amd import decoding as D
    for kw, c in zip(DESIGNED, designed):
        ref, n = c["ref"], c["n"]
        for s in range(c["b"]):
            if s in kw.get("all_dead", ()):
                continue
            assert ref["margin"][s] >= CC.MARGIN or (s in kw.get("tie", ()) and ref["tie"][s] and ref["sel"][s] == 0 and ref["margin"][s] == 0), (kw, s)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        nxt, lp, sel, done, score = D.contrastive_select_torch(t(c["hidden"]), t(c["hist"][:, :n]), t(c["mask"][:, :n]), t(c["cand_tok"]), t(c["cand_logp"]),
                                                               t(c["finished"]), c["alpha"], c["eos"], c["pad"])
        assert np.array_equal(sel.numpy(), ref["sel"]) and np.array_equal(nxt.numpy(), ref["next_tok"]) and np.array_equal(done.numpy(), ref["finished"]), kw
        assert np.array_equal(lp.double().numpy(), ref["logprob"])
        fin = np.isfinite(ref["score"])
        assert np.array_equal(np.isfinite(score.numpy()), fin) and np.abs(score.double().numpy()[fin] - ref["score"][fin]).max() < 1e-5
    for V in (16, 300, 5000):
        for k in (1, 3, 8):
            x = CC.design_rows(5, V, k, "bf16", seed=V + k)
            tok, lp = CC.topk_logprobs(x, k)
            t2, l2 = D.topk_logprobs_torch(torch.from_numpy(x), k)
            fin = np.isfinite(lp)
            assert np.array_equal(t2.numpy()[fin], tok[fin]) and np.abs(l2.double().numpy()[fin] - lp[fin]).max() < 1e-4 and (l2.numpy()[~fin] == -np.inf).all()
            assert fin[1].all() and len(set(np.round(lp[1], 12))) == 1 and not fin[2].all()      # the tie row and the row with fewer than k finite values


# ---- injected defects -------------------------------------------------------------------------------------------------------------------
def outcome(r):
    return (r["sel"].tolist(), r["next_tok"].tolist(), r["finished"].tolist(), [round(float(x), 9) for x in r["logprob"]], r["hist_pos"])


def pointed_cases():
    """hand-built steps, one per defect, on which that defect changes the choice (the designed random cases catch most of them too; these
    make it certain)"""
    h = hand_case
    return {
        # only position 1 is live: candidate 0 (cos 1 with position 0) pays nothing and wins; over the masked positions it pays 1 and loses
        "masked_positions": h(mask=np.array([[0, 1, 0, 1]], np.uint8), cand_logp=np.log(np.array([[0.6, 0.3, 0.1]]))),
        # max against mean: candidates e0 (cos 1, 0, 0.71) and e0 + e1 (0.71, 0.71, 1) both have max 1; their means are 0.57 and 0.80
        "mean": h(cand_logp=np.log(np.array([[0.4, 0.5, 0.1]])), hidden=np.stack([E[0], E[0] + E[1], E[1]])),
        # the last position n - 1 carries the only similarity of candidate 0
        "last_missing": h(hist=np.stack([E[1], 2 * E[1], 3 * E[0], 9 * E[3]])[None], cand_logp=np.log(np.array([[0.5, 0.3, 0.2]]))),
        "alpha_swapped": h(alpha=0.2, cand_logp=np.log(np.array([[0.7, 0.2, 0.1]]))),
        "logp_for_p": h(cand_logp=np.log(np.array([[0.5, 0.1, 0.05]])), alpha=0.3),
        # the dead candidate has no similarity at all: with a probability of 0 it would still win on the penalty
        "dead_wins": h(cand_logp=np.array([[np.log(0.1), -np.inf, np.log(0.1)]]), hidden=np.stack([E[0], E[2], E[0] + E[1]])),
        "tie_to_larger": h(hidden=np.stack([E[2], E[2], E[0]]), cand_logp=np.log(np.array([[0.3, 0.3, 0.2]]))),
        "finished_not_padded": h(finished=np.array([True])),
        "append_at_n_minus_1": h(),
    }


@pytest.mark.parametrize("defect", CC.DEFECTS)
def test_every_injected_defect_fails(defect, designed):
    c = pointed_cases()[defect]
    assert outcome(run(c)) != outcome(run(c, defect)), defect
    assert run(c)["margin"][0] >= CC.MARGIN or run(c)["tie"][0]
    changed = sum(outcome(CC.select(d["hidden"], d["hist"], d["mask"], d["n"], d["cand_tok"], d["cand_logp"], d["finished"], d["alpha"], d["eos"], d["pad"], defect=defect))
                  != outcome(d["ref"]) for d in designed)
    assert changed >= 1, f"no designed case notices the defect {defect}"


def test_bf16_round_is_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -2.5, 3.0e38, 1.0 + 2 ** -9, 1.0 + 3 * 2 ** -9], np.float32)
    assert np.array_equal(CC.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
