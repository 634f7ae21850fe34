"""CPU side of test_gpu_x3_ws: the case table covers what x3_ws_cases claims (through the dispatch as
restated there), the checkers pass the CPU float32 product and the six-term emulation of the
kernel's arithmetic and fail the damage they are there for, and the recorded yardstick is the
computed one.  No device, no library.

Which checker reports which seeded defect (test_checkers_report_seeded_defects):
  rows 8j + 6, 8j + 7 swapped (both of the smallest input scale) ........ ceiling, tile (and row)
  one tile replaced by the tile ``grid`` positions earlier ................ ceiling, tile
  a row's last two columns taken from the next row (the straddling quad) .. ceiling (another row's
      sums: off by the size of the sum itself, of order D / sqrt(K), the ceiling being about 5e-4 D)
  one element off by 32 units of 2^-24 (D + |b|), plain ................... row only: inside the
      ceiling (hundreds of units), lost in a tile's 4,096 elements, 2.8 on the row's scale against 1.9
  an element that should be kept, stored as zero ........................... zeros
"""
import pytest
import torch

import x3_ws_cases as xc

CUS = xc.HOST_CUS
EMU_M = 32 * 4 + 13  # the reduced M of the emulation: five tiles, the last a 13-row tail
ALL_NKS = (8, 11, 16, 21)


def test_shapes_reach_the_sweep_states():
    M = xc.rows(CUS)
    assert [xc.nt_sweep(m, CUS)[:3] for m in M] == [(256, 1, 2), (256, 2, 3), (256, 3, 4), (256, 6, 7),
                                                    (1, 1, 1), (2, 1, 1), (2, 1, 1)]
    assert M[0] % 32 == 0 and M[xc.DEEP] % 32 == 13  # a full copy as the tail tile; a 13-row tail
    ntiles = -(-M[xc.DEEP] // 32)
    assert xc.nt_sweep(M[xc.DEEP], CUS)[3] == (76, 6)  # the tail is the 7th tile of block 76
    # both exits of the two-tiles-per-trip loop: blocks with 7 tiles leave at the first, with 6 at the second
    assert {-(-(ntiles - b) // CUS) for b in range(CUS)} == {6, 7}
    assert {(r // 32) // CUS for r0, r1 in xc.nt_ranges(CUS) for r in (r0, r1 - 1)} == {1, 2, 3, 4, 5, 6}
    for cus in (64, 256, 304):
        rg = xc.nt_ranges(cus)
        assert all(r0 % 32 == 0 and r1 - r0 <= 32 * cus for r0, r1 in rg) and rg[-1][1] == xc.rows(cus)[xc.DEEP]


def test_cases_cover_the_table():
    cases = xc.NT_CASES
    assert len(cases) == len(set(cases)) == 48
    flags = {xc.epi_flags(e) for e in xc.EPIS}
    assert flags == {0, 1, 3, 7, 11, 15}
    deep = {xc.instantiation(c) for c in cases if c[0] == xc.DEEP}
    assert deep == {(nks, e, 1 if nks == 21 else 2) for nks in ALL_NKS for e in flags} and len(deep) == 24
    for s in (0, 1, 2, 4, 5, 6):  # one case per NKS at every shallower shape and tiny M, mixed epilogues
        here = [c for c in cases if c[0] == s]
        assert sorted(xc.nks_of(c[1], c[2]) for c in here) == list(ALL_NKS)
        assert len({c[4] for c in here}) == 4
    assert {c[4] for c in cases if c[0] != xc.DEEP} == set(xc.EPIS)
    for nks, pairs in xc.K_PAIRS.items():
        assert all(xc.nks_of(*p) == nks for p in pairs)
        assert any(k % 4 == 2 for p in pairs for k in p)              # quads straddle two rows
        assert any(p[1] and p[0] % 16 for p in pairs)                 # segment 2 starts inside a k-step
        assert any(xc.pad_cols(*p) == 0 for p in pairs) and any(xc.pad_cols(*p) > 0 for p in pairs)
        assert any(p[1] == 0 for p in pairs)
        for s in (xc.DEEP,):
            assert {(c[1], c[2]) for c in cases if c[0] == s and xc.nks_of(c[1], c[2]) == nks} == set(pairs)
    assert {(c[1], c[2]) for c in cases} == {p for v in xc.K_PAIRS.values() for p in v}
    assert {c[3] for c in cases} == {128, 100, 68}
    for nks in ALL_NKS:
        assert {c[3] for c in cases if c[0] == xc.DEEP and xc.nks_of(c[1], c[2]) == nks} == {128, 100, 68}
    for c in cases:  # adjacent cases share operands; every case is one the weight-stationary kernel takes
        assert xc.nt_ws_ok(xc.rows(CUS)[c[0]], c[1], c[2], c[3], c[4], ldc=c[3] + 4, ldz=8), c
    groups = [c[:4] for c in cases]
    assert len([g for i, g in enumerate(groups) if i == 0 or g != groups[i - 1]]) == len(set(groups))
    assert xc.SEED_CASE in cases and xc.NO_C_CASE in cases and xc.EPIS[xc.SEED_CASE[4]][2]
    assert {xc.instantiation(c)[0] for c in xc.RANGE_CASES} == set(ALL_NKS) and len(xc.RANGE_CASES) == 16
    # the slice runs of the range check stay weight-stationary calls; the classic cases are declined
    assert all(xc.nt_ws_ok(r1 - r0, 166, 166, 128, "plain") for r0, r1 in xc.nt_ranges(CUS))
    assert not any(xc.nt_ws_ok(xc.X3_M, k1, k2, nc, e) for k1, k2, nc, e in xc.X3_CASES)
    assert not xc.nt_ws_ok(31, 64, 64, 128, "plain") and not xc.nt_ws_ok(64, 64, 64, 128, "bias_relu", ldc=130)
    assert not xc.nt_ws_ok(64, 65, 63, 128, "plain") and not xc.nt_ws_ok(64, 64, 0, 128, "plain")


@pytest.mark.parametrize("case", xc.NT_CASES[24:], ids=xc.nt_id)
def test_cpu_f32_product_passes_and_band_is_small(case):
    """Every shallow and tiny case at 256 CUs: the CPU float32 evaluation passes the four checkers and
    at most 1 % of the elements sit in the band the zero test leaves out."""
    r = xc.reference(case, CUS)
    bad, res = xc.failures(r, r.cpu, xc.s_cpu_of(case, CUS))
    print(xc.nt_id(case), f"worst ceiling ratio {res.worst:.4f}, tile S max {float(res.tile_s.max()):.3f}, "
                          f"row S max {float(res.row_s.max()) if res.row_s is not None else float('nan'):.3f}, band {r.band:.5f}")
    assert bad == [] and res.min_live > 0
    assert r.band <= xc.BAND_CAP
    if r.proj is not None:
        assert xc.check_z(r, r.cpu, r.cpu @ r.proj.t()) == 0


@pytest.mark.parametrize("s,k1,k2,nc", [k for k in xc.stat_keys() if k[0] == xc.DEEP], ids=lambda v: str(v))
def test_band_cap_at_the_deepest_shape(s, k1, k2, nc):
    M = xc.rows(CUS)[s]
    for epi in {c[4] for c in xc.NT_CASES if c[:4] == (s, k1, k2, nc)}:
        assert xc.reference_of(M, k1, k2, nc, epi).band <= xc.BAND_CAP, epi


EMU = [(64, 64, 128), (50, 70, 68), (166, 0, 128), (86, 84, 100), (6, 246, 100), (128, 128, 68), (166, 166, 128),
       (336, 0, 100)]


@pytest.mark.parametrize("k1,k2,nc", EMU, ids=lambda v: str(v))
def test_emulation_passes_and_one_lost_term_fails(k1, k2, nc):
    op = xc.operands(EMU_M, k1, k2, nc)
    full = xc.emulate(op)
    for epi in xc.EPIS:
        r = xc.reference_of(EMU_M, k1, k2, nc, epi)
        for name, c in (("emulation", full), ("cpu32", op.cpu32)):
            c = xc.apply_epilogue(c, op, epi, r.keep)
            bad, res = xc.failures(r, c, op.s_cpu)
            assert bad == [], (name, epi, bad, res.worst, float(res.tile_s.max()))
            if r.proj is not None:
                assert xc.check_z(r, c, c @ r.proj.t()) == 0
    r = xc.reference_of(EMU_M, k1, k2, nc, "plain")
    print((k1, k2, nc), f"S_cpu {op.s_cpu:.3f}, emulation tile S max {float(xc.check(r, full).tile_s.max()):.3f}")
    for term in xc.TERMS:  # one of the six plane products missing: every tile is past the allowance
        res = xc.check(r, xc.emulate(op, drop_term=term))
        print("  without", term, f"tile S min {float(res.tile_s.min()):.2f}")
        assert bool((res.tile_s > xc.STAT_FACTOR * op.s_cpu).all()), (term, res.tile_s)
    for step in (0, op.nks - 1):  # a lost k-step is past the ceiling
        bad, res = xc.failures(r, xc.emulate(op, skip_step=step), op.s_cpu)
        assert "ceiling" in bad and res.ceil_bad > op.nc, (step, res.ceil_bad)


def test_checkers_report_seeded_defects():
    M, k1, k2, nc, grid = 32 * 6 + 13, 166, 166, 128, 2
    op = xc.operands(M, k1, k2, nc)
    r = xc.reference_of(M, k1, k2, nc, "plain")
    good = xc.emulate(op)
    assert xc.failures(r, good, op.s_cpu)[0] == []
    # the two tiny rows of a group of eight, swapped
    c = good.clone()
    row = 32 * 3 + 8 + 6
    assert xc.ROW_EXPS[row % 8] == xc.ROW_EXPS[(row + 1) % 8] == max(xc.ROW_EXPS)
    c[[row, row + 1]] = c[[row + 1, row]]
    bad, res = xc.failures(r, c, op.s_cpu)
    assert {"ceiling", "tile", "row"} <= set(bad) and res.ceil_bad > nc
    # tile 4 is tile 4 - grid again (a stale LDS buffer)
    c = good.clone()
    c[32 * 4:32 * 5] = good[32 * (4 - grid):32 * (5 - grid)]
    bad, res = xc.failures(r, c, op.s_cpu)
    assert {"ceiling", "tile"} <= set(bad) and res.ceil_bad > 16 * nc
    assert [i for i, s in enumerate(res.tile_s.tolist()) if s > xc.STAT_FACTOR * op.s_cpu] == [4]
    # the last two columns of a row from the next row, at every scale step of the eight rows
    for row in (40, 45, 46):
        c = good.clone()
        c[row, -2:] = good[row + 1, -2:]
        bad, res = xc.failures(r, c, op.s_cpu)
        assert "ceiling" in bad and res.ceil_bad == 2, (row, bad, res.ceil_bad)  # (46, 47: one scale, other sums)
    # one element 32 units off: the row statistic alone
    c = good.clone()
    c[77, 5] += float(32 * r.unit[77, 5])
    bad, res = xc.failures(r, c, op.s_cpu)
    assert bad == ["row"] and int((res.row_s > xc.STAT_FACTOR * op.s_cpu).sum()) == 1
    # a kept element stored as zero
    rd = xc.reference_of(M, k1, k2, nc, "drop")
    cd = xc.apply_epilogue(good, op, "drop", rd.keep)
    assert xc.failures(rd, cd, op.s_cpu)[0] == []
    i, j = (int(v) for v in rd.nonzero.nonzero()[1234])
    cd[i, j] = 0.0
    bad, res = xc.failures(rd, cd, op.s_cpu)
    assert "zeros" in bad and res.nonzero_bad == 1 and res.zero_bad == 0
    # ... and a dropped element that came through
    cd = xc.apply_epilogue(good, op, "drop", rd.keep)
    i, j = (int(v) for v in (~rd.keep).nonzero()[77])
    cd[i, j] = 1e-30
    bad, res = xc.failures(rd, cd, op.s_cpu)
    assert bad == ["zeros"] and res.zero_bad == 1


def test_recorded_yardstick_is_the_computed_one():
    rec = xc.recorded_stats()
    assert set(rec) == {xc.stat_id(*k) for k in xc.stat_keys()}
    assert all(0.4 < v < 0.55 for v in rec.values())  # half an ulp's uniform error is 0.29; BLAS order adds to it
    for key in ((0, 166, 166, 128), (6, 128, 128, 68)):
        got = xc.compute_stats(CUS, [key])[xc.stat_id(*key)]
        # The same sgemm reproduces it.  Another one sums each element's K products in another number of
        # independent partial sums (vector width x unrolling), and the rounding error of a sum grows
        # with the square root of its length: a factor 4 in that number, either way, is a factor 2
        # here (measured on two hosts with different CPUs: 0.47 and 0.34, sqrt(2) apart).
        assert rec[xc.stat_id(*key)] / 2 <= got <= 2 * rec[xc.stat_id(*key)], (key, got)
