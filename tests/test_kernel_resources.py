"""Register budgets the launch plans rely on, read from the compiler's own remarks (build.py keeps `-Rpass-analysis=kernel-resource-usage`
per translation unit under csrc/_obj/*.resources.txt; tools/kernel_resources.py prints the table).

Why this is a test: `gemm_bf16_pc_kernel<128, 128, ...>` is planned as TWO 8-wave workgroups per CU (4 waves per SIMD, <= 128 registers per
lane).  In round 4 an edit of the tile-coordinate function moved the weight-gradient instantiation from 124 to 140 registers; nothing failed,
the 12-block launches just ran with one workgroup per CU: 189 -> 289 us, dominant-kernel fraction 0.29 -> 0.21."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ROWS = kernel_resources.load()
pytestmark = pytest.mark.skipif(not ROWS, reason="library not built in this tree (no csrc/_obj/*.resources.txt)")


def test_every_translation_unit_reported():
    units = {r["unit"] for r in ROWS}
    assert {"ff_gemm", "ff_attention", "ff_xattn_fused", "ff_rowwise", "ff_optim", "ff_decode", "ff_loss", "ff_elementwise", "ff_sample", "ff_beam"} <= units, units


def test_producer_consumer_gemm_instantiations_keep_their_planned_co_residency():
    seen = 0
    for r in ROWS:
        m = re.search(r"gemm_bf16_pc_kernel(?:<|ILi)(\d+)(?:, |ELi)(\d+)(?:, |ELi)(\d)(?:, |ELi)(\d)(?:, |ELi)(\d)(?:, |ELi)(\d)(?:, |ELi)(\d)(?:, |ELi)(\d)", r["name"] + r["mangled"])
        if not m:
            continue
        bm, bn, al, bl, ns, wpc, npw, ncw = (int(v) for v in m.groups())
        need = wpc * (npw + ncw) // 4                 # waves per SIMD for `wpc` workgroups of npw + ncw waves on a CU's four SIMDs
        assert r["occupancy"] >= need and r["scratch"] == 0, (r["name"], r["vgprs"], r["occupancy"], need)
        if wpc == 2:
            assert r["vgprs"] + r.get("agprs", 0) <= 128, (r["name"], r["vgprs"])
        seen += 1
    assert seen >= 20


def test_no_bfloat16_kernel_spills():
    """(the fp32 verification kernels at 128-wide heads are allowed their scratch: they exist for parity runs, not for speed)"""
    spilling = [r["name"] for r in ROWS if r.get("scratch", 0) > 0 and "float" not in r["name"]]
    assert not spilling, spilling


def test_one_workgroup_per_cu_kernels_fit_their_waves():
    """decode_rows32_kernel and the resident fused cross-attention kernels: 8 resp. 4-6 waves per workgroup, one workgroup per CU"""
    for r in ROWS:
        if "decode_rows32_kernel" in r["mangled"]:
            assert r["occupancy"] >= 2 and r["scratch"] == 0, r
        if "xa_qattn_fwd_res_kernel" in r["mangled"] or "xa_dattn_bwd_res_kernel" in r["mangled"]:
            assert r["occupancy"] >= 2 and r["scratch"] == 0, r


def test_optimizer_kernels_keep_their_occupancy_without_scratch():
    """ff_optim's kernels are HBM-bound streams that hide latency with resident waves.  Floors in waves per SIMD: 4 for every adamw_kernel
    instantiation (5 only for bf16 moments with bf16 gradients), 7 for the sum-of-squares and accumulate kernels, 8 for grad_scale_kernel."""
    floors = {"adamw_kernel": 4, "grad_sumsq_kernel": 7, "grad_accumulate_kernel": 7, "grad_scale_kernel": 8}
    seen = dict.fromkeys(floors, 0)
    for r in ROWS:
        if r["unit"] != "ff_optim":
            continue
        assert r["scratch"] == 0, (r["name"], r["scratch"])
        for family, floor in floors.items():
            if family in r["mangled"]:
                assert r["occupancy"] >= floor, (r["name"], r["vgprs"], r["occupancy"], floor)
                seen[family] += 1
    assert all(seen.values()), seen


def test_selection_kernels_keep_their_functors_out_of_scratch():
    """sample_token_kernel and beam_rows_kernel hand functors to the row walks of csrc/ff_row_keys.h.  A functor that is not inlined puts its
    captured counters in scratch memory, in a kernel that runs 16 to 32 passes over the row: every instantiation (bf16 staged, bf16
    unstaged, fp32 - three of each kernel) uses none."""
    seen = {"sample_token_kernel": 0, "beam_rows_kernel": 0}
    for r in ROWS:
        for family in seen:
            if family in r["mangled"]:
                assert r["scratch"] == 0, (r["name"], r["scratch"])
                seen[family] += 1
    assert seen == {"sample_token_kernel": 3, "beam_rows_kernel": 3}, seen


@pytest.mark.parametrize("unit, kernel, others", [
    ("ff_logits", "logits_process_kernel", ("sample_token_kernel", "beam_rows_kernel")),
    ("ff_logprob", "token_logprob_kernel", ("sample_token_kernel", "beam_rows_kernel", "logits_process_kernel", "shifted_ce_")),
], ids=["ff_logits", "ff_logprob"])
def test_the_unit_is_reported_and_its_kernels_use_no_scratch(unit, kernel, others):
    """ff_logits sits in front of every replayed decode step's selection, ff_logprob inside every step of a session that records
    log-probabilities (at the occupancy of the loss forward whose row pass it restates): a spill would put a memory round trip into a
    launch that does a handful of loads and stores.  Both instantiations are there, and their names stay clear of the kernels other
    resource tests count by name."""
    mine = [r for r in ROWS if r["unit"] == unit]
    assert len(mine) == 2 and all(kernel in r["mangled"] for r in mine), [r["name"] for r in mine]
    assert len({r["mangled"] for r in mine}) == 2
    for r in mine:
        assert r["scratch"] == 0 and r["occupancy"] >= 8, (r["name"], r["scratch"], r["vgprs"], r["occupancy"])
        for other in others:
            assert other not in r["mangled"], r["mangled"]


def test_the_regularised_loss_kernels_are_reported_without_scratch_at_the_plain_occupancy():
    """The regularised instantiations of the two loss kernels - the ones with the trailing (float, float) pack - ride on passes that stream
    the logits: a spill or a lost wave against the plain instantiation of the same kernel and type would cost those passes their bandwidth."""
    mine = [r for r in ROWS if r["unit"] == "ff_loss"]
    assert len(mine) == 8 and all("shifted_ce_" in r["mangled"] for r in mine), [r["name"] for r in mine]
    for kernel in ("shifted_ce_fwd_kernel", "shifted_ce_bwd_kernel"):
        for dtype in ("DF16b", "f"):                                     # the Itanium codes of __bf16 and float
            plain = [r for r in mine if f"{kernel}I{dtype}JEE" in r["mangled"]]
            reg = [r for r in mine if f"{kernel}I{dtype}JffEE" in r["mangled"]]
            assert len(plain) == 1 and len(reg) == 1, (kernel, dtype, [r["mangled"] for r in mine])
            for r in plain + reg:
                assert r["scratch"] == 0, (r["name"], r["scratch"])
            assert reg[0]["occupancy"] >= plain[0]["occupancy"] >= 8, (kernel, dtype, reg[0]["vgprs"], reg[0]["occupancy"], plain[0]["occupancy"])


def test_the_ema_kernel_is_reported_without_scratch_at_the_accumulate_kernels_occupancy():
    """ema_update_kernel, for bf16 and for fp32 weights, is held to the floor of grad_accumulate_kernel, its nearest relative (one stream
    in, one fp32 read-modify-write stream): 7 waves per SIMD, no scratch, no LDS."""
    unit = [r for r in ROWS if r["unit"] == "ff_optim"]
    mine = [r for r in unit if "ema_update_kernel" in r["mangled"]]
    assert len(mine) == 2 and not any("adamw_kernel" in r["mangled"] for r in mine), [r["mangled"] for r in mine]
    for dtype in ("DF16b", "f"):                                         # the Itanium codes of __bf16 and float
        row = [r for r in mine if f"ema_update_kernelI{dtype}E" in r["mangled"]]
        assert len(row) == 1, (dtype, [r["mangled"] for r in mine])
        assert row[0]["scratch"] == 0 and row[0].get("lds", 0) == 0, row[0]
        assert row[0]["occupancy"] >= 7, (row[0]["name"], row[0]["vgprs"], row[0]["occupancy"])


def test_the_adamw_instantiations_are_the_33_there_were():
    """The weight average came as a kernel of its own: the unit keeps its 33 adamw_kernel instantiations (21 round-to-nearest, 12
    stochastic-rounding)."""
    assert sum("adamw_kernel" in r["mangled"] for r in ROWS if r["unit"] == "ff_optim") == 33
