"""The weight-stationary split-bf16 NT (gemm_ws.hip gemm_nt_ws_kernel) past one tile per block,
element by element (cases, references and checkers: x3_ws_cases; what they claim is checked on the
CPU by test_x3_ws_host).

Every call goes through fused.gemm_nt with w1 / w2, math="split_bf16" and dense 16-byte operands.
M comes from the device's CU count, so blocks sweep 1-2, 2-3, 3-4 and 6-7 tiles (the steady state
of the two LDS buffers and staging register sets, both exits of the loop, a 13-row tail as a block's
7th tile), with M = 32, 33 and 45 for grids of one and two blocks; the K pairs reach every k-step
count (8, 11, 16 with K split over a wave pair, 21 without), straddling staging quads, a second
segment starting inside a k-step and 0 to 14 pad columns; Nc 128, 100 and 68.

Per case: the four checkers of x3_ws_cases (ceiling, exact zeros, the tile / row statistic against
four times the CPU float32 product's, z against the stored C); C written into a view (ldc = Nc + 4,
guard rows) of a NaN-filled buffer and z into a padded one, no byte outside the views changed; the
inputs unchanged; a second run bit-equal; and the epilogue equal, bit for bit, to the same float32
operations applied to the plain run of the same operands (bias add, ReLU, the oracle's keep mask
and f32(1 / (1 - p))) - which pins the kernel's own dropout hash at every sweep position.
At the deepest shape the rows of three ranges are bit-equal to a one-tile-per-block run over those
rows alone.  The classic gemm_nt_x3_kernel gets the checkers at the N = 64 shapes nt_ws_ok declines.
"""
import functools

import pytest
import torch

import x3_ws_cases as xc

pytestmark = pytest.mark.gpu

SENT32 = 0x7FC12345    # a float32 NaN payload


@pytest.fixture(scope="module")
def cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def _fill(buf):
    buf.view(torch.int32).fill_(SENT32)
    return buf


def _outside_untouched(buf, r0, r1, c0, c1):
    v = buf.view(torch.int32).clone()
    v[r0:r1, c0:c1] = SENT32
    return bool((v == SENT32).all())


DEV_KEYS = ("a1", "a2", "w1", "w2", "bias", "proj")


@functools.lru_cache(maxsize=1)
def _device_operands(M, k1, k2, nc, device):
    op = xc.operands(M, k1, k2, nc)
    return {k: getattr(op, k).to(device) if getattr(op, k) is not None else None for k in DEV_KEYS}


def _run(t, nc, epi, out=None, z=None, seed=xc.DROP_SEED, seed_ptr=None, want_c=True, a=None):
    from elliptic_gnn_project_amd.fused import gemm_nt

    a1, a2 = a if a is not None else (t["a1"], t["a2"])
    bias, relu, drop, proj = xc.EPIS[epi]
    kw = dict(a2=a2, w1=t["w1"], w2=t["w2"], math="split_bf16", out=out, want_c=want_c)
    if bias:
        kw["bias"] = t["bias"]
    if relu:
        kw["relu"] = True
    if drop:
        kw.update(dropout_p=xc.DROP_P, seed=seed, seed_ptr=seed_ptr)
    if proj:
        kw.update(proj=t["proj"], z=z)
    c = gemm_nt(a1, None, nc, **kw)
    if want_c:
        assert c.dtype == torch.float32 and (out is None or c.data_ptr() == out.data_ptr())
    return c


def _guarded_run(device, t, M, nc, epi, **kw):
    """One run into guarded destinations: C a [2:M + 2, :Nc] view of a NaN-filled (M + 4, Nc + 4)
    buffer (two rows above and below M, four columns between rows), z a [1:M + 1, :4] view of an
    (M + 2, 8) one.  Returns the views after asserting nothing else changed."""
    proj = bool(xc.EPIS[epi][3])
    buf = _fill(torch.empty((M + 4, nc + 4), device=device))
    out = buf[2:M + 2, :nc]
    zb = _fill(torch.empty((M + 2, 8), device=device)) if proj else None
    z = zb[1:M + 1, :4] if proj else None
    assert out.data_ptr() % 16 == 0 and out.stride(0) == nc + 4
    _run(t, nc, epi, out, z, **kw)
    torch.cuda.synchronize()
    assert _outside_untouched(buf, 2, M + 2, 0, nc), "C guard"
    if proj:
        assert _outside_untouched(zb, 1, M + 1, 0, 4), "z guard"
    return out, z


def _chain(t, plain, epi, keep, device):
    """The epilogue in float32 on the device's own plain output: what the kernel must store, bit for bit."""
    bias, relu, drop, proj = xc.EPIS[epi]
    c = plain
    if bias:
        c = c + t["bias"]
    if relu:
        c = torch.relu(c)
    if drop:
        c = torch.where(keep.to(device), c * xc.drop_scale32().to(device), torch.zeros((), device=device))
    return c


def _assert_checkers(r, c, z, s_cpu, name, tile=32):
    bad, res = xc.failures(r, c, s_cpu, tile)
    row = float(res.row_s.max()) if res.row_s is not None else float("nan")
    print(name, f"NKS {r.nks}: worst ceiling ratio {res.worst:.4f} at {res.worst_at}, tile S max {float(res.tile_s.max()):.3f}, "
                f"row S max {row:.3f}, allowed {xc.STAT_FACTOR * s_cpu:.3f}, band {r.band:.5f}, zero misses "
                f"{res.zero_bad} + {res.nonzero_bad}")
    assert res.ceil_bad == 0, (res.ceil_bad, res.worst, res.worst_at)
    assert res.zero_bad == 0 and res.nonzero_bad == 0 and r.band <= xc.BAND_CAP
    assert "tile" not in bad, [(i, s) for i, s in enumerate(res.tile_s.tolist()) if not s <= xc.STAT_FACTOR * s_cpu][:8]
    assert "row" not in bad, [(i, s) for i, s in enumerate(res.row_s.tolist()) if not s <= xc.STAT_FACTOR * s_cpu][:8]
    assert res.min_live > 0
    if r.proj is not None:
        assert xc.check_z(r, c, z) == 0
    return res


def _case(device, cus, case, seed=xc.DROP_SEED, seed_ptr=None, eff_seed=None):
    s, k1, k2, nc, epi = case
    M = xc.rows(cus)[s]
    assert xc.nt_ws_ok(M, k1, k2, nc, epi, ldc=nc + 4, ldz=8)
    if s <= xc.DEEP:
        assert xc.nt_sweep(M, cus)[2] >= 2  # more tiles than blocks
    r = xc.reference(case, cus, seed=seed if eff_seed is None else eff_seed)
    t = _device_operands(M, k1, k2, nc, device)
    out, z = _guarded_run(device, t, M, nc, epi, seed=seed, seed_ptr=seed_ptr)
    out2, z2 = _guarded_run(device, t, M, nc, epi, seed=seed, seed_ptr=seed_ptr)
    assert torch.equal(out, out2) and (z is None or torch.equal(z, z2))  # bit-equal repeat
    for k in DEV_KEYS:  # inputs untouched
        assert t[k] is None or torch.equal(t[k].cpu(), getattr(r.op, k)), k
    plain = _run(t, nc, "plain")
    assert torch.equal(out, _chain(t, plain, epi, r.keep, device)), "epilogue chain"
    _assert_checkers(r, out.cpu(), z.cpu() if z is not None else None, xc.s_cpu_of(case, cus), xc.nt_id(case))
    return out, z, t, r


@pytest.mark.parametrize("case", xc.NT_CASES, ids=xc.nt_id)
def test_ws_nt_past_one_tile_per_block(device, cus, case):
    _case(device, cus, case)


def test_ws_nt_seed_counter(device, cus):
    """With seed_ptr set the mask is the oracle's under seed = *seed_ptr * phi + seed (mod 2^64), at
    every tile of a block's sweep."""
    counter = 0x1_0000_0005  # past 32 bits: the product wraps in 64
    eff = xc.effective_seed(xc.DROP_SEED, counter)
    assert eff != xc.DROP_SEED and eff >> 32 and eff & 0xFFFFFFFF
    assert not torch.equal(xc.reference(xc.SEED_CASE, cus, seed=eff).keep, xc.reference(xc.SEED_CASE, cus).keep)
    ctr = torch.tensor([counter], dtype=torch.int64, device=device)
    out, z, t, r = _case(device, cus, xc.SEED_CASE, seed_ptr=ctr, eff_seed=eff)
    sure = r.nonzero | ~r.keep  # all but what ReLU may cut
    assert torch.equal((out.cpu() != 0)[sure], r.keep[sure])


def test_ws_nt_z_without_c(device, cus):
    s, k1, k2, nc, epi = xc.NO_C_CASE
    M = xc.rows(cus)[s]
    t = _device_operands(M, k1, k2, nc, device)
    _, z = _guarded_run(device, t, M, nc, epi)
    zb = _fill(torch.empty((M + 2, 8), device=device))
    assert _run(t, nc, epi, None, zb[1:M + 1, :4], want_c=False) is None
    torch.cuda.synchronize()
    assert _outside_untouched(zb, 1, M + 1, 0, 4)
    assert torch.equal(zb[1:M + 1, :4], z)


@pytest.mark.parametrize("case", xc.RANGE_CASES, ids=xc.nt_id)
def test_ws_nt_sweep_position_changes_no_bit(device, cus, case):
    """A tile's arithmetic does not depend on where in a block's sweep it runs: rows [r0, r1) of the
    deepest shape's output equal, bit for bit, gemm_nt over that row slice alone (one tile per block:
    prologue loads only), which itself passes the checkers.  A stale LDS buffer or staging register
    set shows here even where it stays inside the float64 bounds."""
    s, k1, k2, nc, epi = case
    M = xc.rows(cus)[s]
    assert xc.nt_sweep(M, cus)[1:3] == (6, 7) or cus < 77
    r = xc.reference(case, cus)
    t = _device_operands(M, k1, k2, nc, device)
    proj = r.proj is not None
    big = torch.empty((M, nc), device=device)
    zbig = torch.empty((M, 4), device=device) if proj else None
    _run(t, nc, epi, big, zbig)
    for r0, r1 in xc.nt_ranges(cus):
        assert xc.nt_sweep(r1 - r0, cus)[2] == 1 and r0 % 32 == 0
        assert xc.nt_ws_ok(r1 - r0, k1, k2, nc, epi)
        a = (t["a1"][r0:r1], t["a2"][r0:r1] if k2 else None)
        assert a[0].is_contiguous() and a[0].data_ptr() % 16 == 0
        out = torch.empty((r1 - r0, nc), device=device)
        zs = torch.empty((r1 - r0, 4), device=device) if proj else None
        _run(t, nc, epi, out, zs, a=a)
        assert torch.equal(big[r0:r1], out), (r0, r1)
        if proj:
            assert torch.equal(zbig[r0:r1], zs), (r0, r1)
        _assert_checkers(xc.row_slice(r, r0, r1), out.cpu(), zs.cpu() if proj else None, xc.s_cpu_of(case, cus),
                         f"{xc.nt_id(case)} rows {r0}:{r1}")


@pytest.mark.parametrize("k1,k2,nc,epi", xc.X3_CASES, ids=lambda v: str(v))
def test_classic_x3_nt_tile_statistic(device, k1, k2, nc, epi):
    """gemm_nt_x3_kernel (128-row tiles) at the N = 64 shapes of the default GCN / GAT layer 1 and the
    hidden-64 SAGE, which nt_ws_ok declines: the same checkers, the statistic per 128-row tile."""
    M = xc.X3_M
    assert not xc.nt_ws_ok(M, k1, k2, nc, epi)
    r = xc.reference_of(M, k1, k2, nc, epi)
    t = _device_operands(M, k1, k2, nc, device)
    z = torch.empty((M, 4), device=device) if r.proj is not None else None
    c = _run(t, nc, epi, None, z)
    _assert_checkers(r, c.cpu(), z.cpu() if z is not None else None, r.op.s_cpu, f"classic {k1}+{k2}-n{nc}-{epi}", tile=128)
