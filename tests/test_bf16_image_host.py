"""CPU side of test_gpu_bf16_image: the shapes reach the kernel states the cases module claims, the
CPU float32 evaluation of every NT case passes the per-element bound (so the bound is not tighter
than f32 accumulation itself), its misrounded counts are the recorded ones, and the checker sees
the two kinds of damage the old max-against-max assertion let through.  No device, no library.
"""
import math

import pytest
import torch

import bf16_image_cases as bc

CUS = bc.HOST_CUS


def test_nt_shapes_reach_the_ring_states():
    rows = bc.nt_rows(CUS)
    assert [bc.nt_sweep(M, CUS)[:3] for M in rows] == [(256, 1, 2), (256, 2, 3), (256, 3, 4), (256, 6, 7)]
    assert [-(-M // 32) for M in rows] == [259, 640, 769, 1613]
    assert rows[bc.DEEP] % 32 == 13
    block, pos = bc.nt_sweep(rows[bc.DEEP], CUS)[3]
    assert (block, pos) == (76, 6)  # the tail tile is the 7th of its block: every ring buffer reused before it
    for cus in (64, 256, 304):  # any CU count: whole tiles of the deepest shape, at most one tile per block
        M = bc.nt_rows(cus)[bc.DEEP]
        rg = bc.nt_ranges(cus)
        assert all(r0 % 32 == 0 and 0 <= r0 < r1 <= M and r1 - r0 <= 32 * cus for r0, r1 in rg)
        assert rg[-1][1] == M
    # at 256 CUs the ranges hold tiles of every later sweep position
    assert {(r // 32) // CUS for r0, r1 in bc.nt_ranges(CUS) for r in (r0, r1 - 1)} == {1, 2, 3, 4, 5, 6}


def test_nt_cases_cover_the_issue():
    cases = bc.NT_CASES
    assert len(cases) == len(set(cases)) and 20 <= len(cases) <= 32
    for ld in (256, 336):  # every epilogue at the deepest shape, at both widths
        assert {c[4] for c in cases if c[0] == bc.DEEP and bc.image_ld(c[1], c[2])[1] == ld} == set(bc.EPIS)
    for s in range(3):
        for ld in (256, 336):
            assert {c[4] for c in cases if c[0] == s and bc.image_ld(c[1], c[2])[1] == ld} >= {"plain", "drop_proj"}
    assert {(c[1], c[2]) for c in cases} == {(128, 128), (100, 150), (166, 166), (150, 180)}
    assert bc.image_ld(100, 150) == (104, 256) and bc.image_ld(150, 180) == (152, 336)  # a zero gap after k1
    assert {c[3] for c in cases} == {128, 72, 8}
    assert {bc.image_ld(c[1], c[2])[1] for c in bc.RANGE_CASES} == {256, 336}
    assert {c[4] for c in bc.RANGE_CASES} == {"plain", "bias", "bias_relu", "proj"}


def test_tn_plan_figures():
    for M, fig in bc.TN_PLAN.items():
        assert bc.tn_plan(M) == fig
    nch = {n for M in bc.TN_M for n in bc.tn_plan(M)[3:]}
    assert nch == {1, 3, 4, 5, 6, 7, 8}
    # the 5-row last block loads rows M - 16 .. M: 11 of them its neighbour's
    blocks, rows, last = bc.tn_plan(12_741)[:3]
    assert (blocks - 1) * rows - (12_741 - 16) == 11 and last == 5


def test_tn_cases_cover_the_issue():
    cases = bc.TN_CASES
    assert len(cases) == len(set(cases))
    assert {(c[0], bc.image_ld(c[1], c[2])[1]) for c in cases} == {(M, ld) for M in bc.TN_M for ld in (256, 336)}
    assert {(c[4], c[5]) for c in cases} == {(f, g) for f in bc.TN_FORMS for g in (True, False)}
    assert {(c[4], c[6]) for c in cases} == {(f, d) for f in bc.TN_FORMS for d in ("f32", "bf16")}
    assert {(c[4], c[3]) for c in cases} == {(f, n) for f in bc.TN_FORMS for n in (128, 72, 8)}
    assert {(c[0], c[3] < 128) for c in cases} == {(M, b) for M in bc.TN_M for b in (True, False)}


def test_rne_bf16_is_one_rounding():
    x = torch.tensor([1.0, 1.00390625, 1.005859375, 1.00390625 + 2.0 ** -40, 1.01171875 - 2.0 ** -40, -0.3, 0.0],
                     dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0078125, 1.0078125, 1.0078125, -0.30078125, 0.0],
                        dtype=torch.float64)
    assert torch.equal(bc.rne_bf16(x), want)
    y = torch.randn(4096, dtype=torch.float32)
    assert torch.equal(bc.rne_bf16(y.double()), y.to(torch.bfloat16).double())  # from float32: torch's own RNE


@pytest.mark.parametrize("case", bc.NT_CASES, ids=bc.nt_id)
def test_cpu_f32_evaluation_passes_and_share_is_recorded(case):
    r = bc.nt_reference(case, CUS)
    res = bc.nt_check(r, r.cpu)
    rec = bc.recorded_shares()[bc.nt_id(case)]
    print(bc.nt_id(case), f"worst ratio {res.worst:.3f} misrounded {res.misrounded} / {res.n} recorded {rec['cpu']}")
    assert res.bound_bad == 0 and res.zero_bad == 0, (res.worst, res.worst_at)
    assert res.worst < 1.0
    assert rec["n"] == res.n
    # the count is a property of the BLAS summation order: the same build reproduces it exactly,
    # another sgemm kernel lands within the sampling noise of a count (4 sigma of a Poisson count)
    assert abs(res.misrounded - rec["cpu"]) <= 4.0 * math.sqrt(max(rec["cpu"], 1)) + 1
    if r.proj is not None:
        z = (r.cpu.float() @ r.proj.t())
        assert bc.nt_check_z(r, r.cpu, z) == 0


def _ulp_bf16(v):
    return 2.0 ** (math.floor(math.log2(abs(v))) - 7)


@pytest.mark.parametrize("case", [c for c in bc.NT_CASES if c[4] == "plain" and c[0] in (0, bc.DEEP)], ids=bc.nt_id)
def test_checker_sees_what_max_against_max_missed(case):
    r = bc.nt_reference(case, CUS)
    base = bc.nt_check(r, r.cpu)
    assert base.bound_bad == 0 and bc.old_max_check(r.cpu, r.ref)
    # one small element two bf16 ulps off
    cand = ((r.ref.abs() < 0.05) & (r.ref.abs() > 0.02)).nonzero()
    i, j = (int(v) for v in cand[len(cand) // 2])
    c = r.cpu.clone()
    v = float(c[i, j])
    c[i, j] = v + 2 * _ulp_bf16(v) * (1 if v > 0 else -1)
    assert float(c[i, j]) != v and abs(float(c[i, j]) - v) <= 2.001 * _ulp_bf16(v) * 2
    res = bc.nt_check(r, c)
    assert res.bound_bad == 1 and res.worst_at == (i, j), (res.bound_bad, res.worst_at, (i, j))
    assert res.misrounded == base.misrounded + 1
    assert bc.old_max_check(c, r.ref)  # the old expression passes it
    # one output row swapped with its neighbour: two rows of the smallest input scale
    c = r.cpu.clone()
    row = 32 * 7 + 6
    assert bc.ROW_EXPS[row % 8] == bc.ROW_EXPS[(row + 1) % 8] == max(bc.ROW_EXPS)
    c[[row, row + 1]] = c[[row + 1, row]]
    res = bc.nt_check(r, c)
    assert res.bound_bad > c.size(1) and res.misrounded > base.misrounded + c.size(1)
    assert bc.old_max_check(c, r.ref)


def test_row_misses_sees_one_lost_row_and_column():
    ref = torch.randn(8, 40, dtype=torch.float64)
    got = ref.float().clone()
    assert bc.row_misses(got, ref) == []
    got[5] = 0
    got[2, 17] = 0
    assert bc.row_misses(got, ref) == [2, 5]
