"""GPU: K12 (csrc/bn.hip) at every block geometry against the float64 reference of tests/bn_ref.py, and
K13's edges.

bn.hip lays a block out as cols = min(C, 256) columns by lanes = 256 / cols row lanes and derives the
column passes (C > 256), the idle threads (256 % C != 0), the reduction block height R and the apply
grid min(ceil(N / lanes), 2048) from it.  bn_ref.case_table() walks them: 11 widths at N = 2 and one
row on either side of a reduction unit (the clamped "load row r0, then drop it" lanes), and at four
widths the first grid-stride trip of the apply kernels and the first N at which R doubles.  Every
case applies the bounds derived in bn_ref's docstring (u = 2^-24; forward 12 u·mag_out, sums
(K + 4) u·Σ|terms|, dz (K + 12) u·mag_dz, running statistics 2 float32 ulps, num_batches_tracked
exact); the integer probes need no tolerance at all (Σdy of integers is exact in any order, so
bias.grad must be the reference's integer bit for bit, and with momentum 1 running_mean must be
float32(mean64)).  Further: the colsum form of the backward apply, four training steps on one module
(the cumulative average with nbt = 1, 2, 3), the device seed counter, two unequal SyncBN shards on
one GPU (a stub process group adds the other shard's float64 contribution), the one-pass variance at
mean / spread up to 1e5, a constant column, statistics of an empty shard, and K13 at N = 1, 2, 7,
Fin = 1, 63, 256, dim = 1, 64, 600, T = 2, timesteps of ±2^40 and x as a column slice.

Largest errors seen on the MI355X, in the units each bound is stated in (bound in brackets):

    family                      forward [12]   dweight / dbias [K + 4]   dz [K + 12]   running [2 ulps]
    table, N <= unit + 1        2.76           3.17 / 1.68  [>= 26]      4.96 [>= 34]  1.06
    table, 2048·lanes + 1       3.74           0.43 / 0.24  [>= 26]      3.64 [>= 34]  0.91
    table, 2048·unit + 1        3.77           0.18 / 0.10  [>= 30]      3.90 [>= 38]  0.96
    p = 0 / no r / momentum None / no running stats
                                2.76           2.30 / 1.74  [>= 26]      4.73 [>= 34]  1.15
    device seed counter         3.12           1.10 / 0.85  [29]         3.34 [37]     -
    two shards (K + 1)          3.84           2.07 / 1.46  [>= 27]      3.87 [>= 35]  0.97
    four steps                  -              -                         -             1.23
    dz column sums: 1.03 u·Σ|dz| at (17, 100) [12]; at 2048·lanes + 1 rows at most 0.23 [>= 2051]
    one-pass variance: 0.022 (running_var) and 0.053 (1 / invstd²) of the float64 summation bound

Every derived bound held as first derived; none was re-derived.  The integer probes, the constant
columns, the seed counter's kept set and K13's x columns are exact comparisons.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu

SEED = 1234567
CROSS = [(R.unit(64) + 1, 64), (R.unit(257) + 1, 257)]


def _bn(device, C, a=None, momentum=0.1, track=True, nbt0=0, cls=torch.nn.BatchNorm1d):
    bn = cls(C, momentum=momentum, track_running_stats=track).to(device).train()
    if a is not None:
        with torch.no_grad():
            bn.weight.copy_(a.w)
            bn.bias.copy_(a.b)
            if track:
                bn.running_mean.copy_(a.rm)
                bn.running_var.copy_(a.rv)
                bn.num_batches_tracked.fill_(nbt0)
    return bn


def _device_pos(device, z, a):
    """The device's ReLU decisions: a K12 forward of the same z with p = 0 and no residual."""
    from elliptic_gnn_project_amd.fused import bn_relu_dropout_residual

    with torch.no_grad():
        out = bn_relu_dropout_residual(z.to(device), None, _bn(device, z.size(1), a, track=False), 0.0, 0, None)
    return (out > 0).cpu()


def _run(device, bn, z, r, dh, p, seed, ctr=None):
    from elliptic_gnn_project_amd.fused import bn_relu_dropout_residual

    z = z.to(device).requires_grad_(True)
    r = r.to(device).requires_grad_(True) if r is not None else None
    bn.weight.grad = bn.bias.grad = None
    out = bn_relu_dropout_residual(z, r, bn, p, seed, ctr)
    out.backward(dh.to(device))
    return SimpleNamespace(out=out.detach(), dz=z.grad, dweight=bn.weight.grad, dbias=bn.bias.grad,
                           dr=r.grad if r is not None else None)


def _report(tag, N, C, e):
    print(f"K12-UNITS {tag} N={N} C={C} " + " ".join(f"{k}={v:.3f}" for k, v in e.items()))


def _bounds_case(device, N, C, p=0.5, with_r=True, momentum=0.1, track=True, nbt0=0, tag="table"):
    a = R.make_inputs(N, C)
    r = a.r if with_r else None
    ref = R.tail(a.z, r, a.w, a.b, p, SEED, a.dh, device_pos=_device_pos(device, a.z, a))
    assert ref.ties <= R.TIE_CAP * N * C
    bn = _bn(device, C, a, momentum, track, nbt0)
    res = _run(device, bn, a.z, r, a.dh, p, SEED)
    e = R.check_all(res, ref)
    if track:
        e["rmean_ulp"], e["rvar_ulp"] = R.check_running(bn, a.rm, a.rv, nbt0, ref, momentum)
    else:
        assert bn.running_mean is None and bn.running_var is None
    _report(tag, N, C, e)


@pytest.mark.parametrize("N,C", R.case_table())
def test_tail_meets_the_derived_bounds(device, N, C):
    """p = 0.5, a residual, fixed momentum, forward and backward, at every case of the table."""
    _bounds_case(device, N, C)


@pytest.mark.parametrize("N,C", CROSS)
@pytest.mark.parametrize("variant", ["p0", "no_residual", "momentum_none", "no_running_stats"])
def test_tail_branches_meet_the_derived_bounds(device, N, C, variant):
    kw = dict(p0=dict(p=0.0), no_residual=dict(with_r=False), momentum_none=dict(momentum=None, nbt0=2),
              no_running_stats=dict(track=False))[variant]
    _bounds_case(device, N, C, tag=variant, **kw)


@pytest.mark.parametrize("N,C", R.case_table())
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_integer_probe_counts_every_row_once(device, N, C, p):
    """Integer z and dh, w = 1, b = 0: bias.grad is the reference's integer sum bit for bit and, with
    momentum 1, running_mean is float32 of the float64 mean: a dropped, repeated or mis-masked row at
    any geometry fails outright."""
    z, dh = R.integer_inputs(N, C)
    assert R.integer_precondition(z, dh)
    ref = R.tail(z, None, torch.ones(C), torch.zeros(C), p, SEED, dh)
    assert ref.ties == 0
    bn = _bn(device, C, momentum=1.0)
    res = _run(device, bn, z, None, dh, p, SEED)
    assert torch.equal(res.dbias.cpu().double(), ref.dbias)
    assert torch.equal(bn.running_mean.cpu(), ref.mean.float())
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("C", [1, 3, 64, 100, 256])
@pytest.mark.parametrize("long", [False, True])
def test_dz_column_sums_are_the_bias_gradient_below(device, C, long):
    """gnn_bn_act_bwd_colsum_f32's per-block column sums of dz, finished by colsum_of, against a float64
    column sum of the device's own dz; dz bit-identical to gnn_bn_act_bwd_f32's.  At 2048·lanes + 1 rows
    block 0 sums two row groups (the only size of the table where a block sums more than one)."""
    from elliptic_gnn_project_amd import fused
    from elliptic_gnn_project_amd.aggregation import colsum_of

    N = R.BLOCKS * R.lanes(C) + 1 if long else R.unit(C) + 1
    a = R.make_inputs(N, C)
    z0, r0, dh = a.z.to(device), a.r.to(device), a.dh.to(device)
    res = []
    for on in (True, False):
        fused._BN_COLSUM = on
        try:
            bn = _bn(device, C, a)
            z = z0.clone().requires_grad_(True)
            out = fused.bn_relu_dropout_residual(z, r0, bn, 0.5, SEED, None)
            seen = {}
            h = z.register_hook(lambda gr: seen.setdefault("g", gr))
            out.backward(dh)
            h.remove()
            gr = seen["g"]
            assert (getattr(gr, "_gnnmp_colsum", None) is not None) == on
            if on:
                assert gr._gnnmp_colsum.numel() == R.grid(N, C) * C
            res.append((gr.clone(), colsum_of(gr)))
        finally:
            fused._BN_COLSUM = True
    (ga, da), (gb, db) = res
    assert torch.equal(ga, gb)
    ref = ga.double().sum(0).cpu()
    mag = ga.double().abs().sum(0).cpu()
    nblocks = R.grid(N, C)
    adds = R.ceil_div(N, nblocks * R.lanes(C)) + R.lanes(C) + nblocks
    e = R._units(da, ref, mag)
    assert e <= adds, (e, adds)
    print(f"K12-UNITS colsum N={N} C={C} colsum={e:.3f} bound={adds}")


@pytest.mark.parametrize("C", [64, 257])
@pytest.mark.parametrize("momentum", [None, 0.1])
def test_running_statistics_over_four_steps(device, C, momentum):
    """Four training-mode calls on one module, fresh z each: the running statistics after every call
    (from the module's own state before it) and num_batches_tracked: 1 / (nbt + 1) with nbt = 0..3."""
    a = R.make_inputs(100, C)
    bn = _bn(device, C, a, momentum)
    worst = 0.0
    for step in range(4):
        b = R.make_inputs(100 + 31 * step, C, seed=step + 1)
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        assert int(bn.num_batches_tracked) == step
        ref = R.tail(b.z, b.r, a.w, a.b, 0.5, SEED + step, b.dh)
        _run(device, bn, b.z, b.r, b.dh, 0.5, SEED + step)
        worst = max(worst, *R.check_running(bn, rm0, rv0, step, ref, momentum))
    assert int(bn.num_batches_tracked) == 4
    print(f"K12-UNITS steps C={C} momentum={momentum} running_ulp={worst:.3f}")


@pytest.mark.parametrize("ctr", [0, 1, 5])
def test_device_seed_counter(device, ctr):
    """seed_ptr: the mask is the oracle's for (ctr · 0x9E3779B97F4A7C15 + seed) mod 2^64, forward and
    backward (every bound, and the kept elements themselves)."""
    N, C = 100, 64
    a = R.make_inputs(N, C)
    seed = 2 ** 62 + 12345
    eff = R.effective_seed(seed, ctr)
    ref = R.tail(a.z, a.r, a.w, a.b, 0.5, eff, a.dh, device_pos=_device_pos(device, a.z, a))
    bn = _bn(device, C, a)
    res = _run(device, bn, a.z, a.r, a.dh, 0.5, seed, torch.tensor([ctr], dtype=torch.int64, device=device))
    e = R.check_all(res, ref)
    live = ref.out != a.r.double()  # relu(y) > 0 and kept
    assert torch.equal((res.out.cpu() != a.r), live)
    if ctr:
        other = R.tail(a.z, a.r, a.w, a.b, 0.5, R.effective_seed(seed), a.dh)
        assert not torch.equal(other.out != a.r.double(), live)
    _report("seed_ctr", N, C, e)


class _OtherShard:
    """A process group of two on one GPU: all_reduce adds the other shard's contribution."""

    def __init__(self):
        self.adds = []

    def is_initialized(self):
        return True

    def all_reduce(self, t):
        t.add_(self.adds.pop(0).to(device=t.device, dtype=t.dtype))


@pytest.mark.parametrize("rows", [(700, 77), (8193, 1)])
@pytest.mark.parametrize("C", [64, 257])
@pytest.mark.parametrize("momentum,nbt0", [(0.1, 0), (None, 1)])
def test_two_shards_on_one_gpu(device, rows, C, momentum, nbt0):
    """gnn_bn_stats_f32(finalize = 0) -> all-reduce -> gnn_bn_finalize_f32 with n_total != N, and the
    backward apply with inv_n = 1 / n_total on local rows: each shard's out and dz are its rows of the
    full batch's, weight.grad / bias.grad the local sums, the running statistics the full batch's."""
    from elliptic_gnn_project_amd.distributed import SyncBatchNorm1d
    from elliptic_gnn_project_amd.fused import _bn_group

    N = sum(rows)
    a = R.make_inputs(N, C)
    pos = _device_pos(device, a.z, a)
    lo, hi = slice(0, rows[0]), slice(rows[0], N)
    for me, ot in ((lo, hi), (hi, lo)):
        ref = R.tail(a.z[me], a.r[me], a.w, a.b, 0.5, SEED, a.dh[me], other=(a.z[ot], a.dh[ot]), device_pos=pos[me])
        assert ref.n == N and ref.K == R.chain(ref.N, C) + 1
        bn = _bn(device, C, a, momentum, nbt0=nbt0, cls=SyncBatchNorm1d)
        bn.dist = _OtherShard()
        bn.dist.adds = [ref.stats2, ref.sums2]
        assert _bn_group(bn) is bn.dist
        res = _run(device, bn, a.z[me], a.r[me], a.dh[me], 0.5, SEED)
        assert not bn.dist.adds
        e = R.check_all(res, ref)
        e["rmean_ulp"], e["rvar_ulp"] = R.check_running(bn, a.rm, a.rv, nbt0, ref, momentum)
        _report("shard", ref.N, C, e)


def test_one_pass_variance_conditioning(device):
    """Columns with mean / spread of 1e3, 1e4 and 1e5: the variance the device forms from float64
    Σz² / n − m² against the two-pass float64 one, within the worst case of sequential float64
    summation, N·2^-53·(1 + mean² / var) relative (plus the float32 roundings of what is read back: one
    for running_var, six for 1 / invstd² = var + eps).  Float32 partials would miss it by 1e5 and more."""
    from elliptic_gnn_project_amd.fused import bn_relu_dropout_residual

    N, C = 20000, 16
    g = torch.Generator().manual_seed(17)
    centre = torch.tensor([1e3, 1e4, 1e5], dtype=torch.float64).repeat(6)[:C]
    z = (centre + torch.randn(N, C, generator=g, dtype=torch.float64)).float()
    zd = z.double()
    mean = zd.sum(0) / N  # (Σz of these float32 values is exact in float64 in any order)
    var = ((zd - mean) ** 2).sum(0) / N
    bound = N * 2.0 ** -53 * (1 + mean ** 2 / var)
    bn = _bn(device, C, momentum=1.0)
    out = bn_relu_dropout_residual(z.to(device).requires_grad_(True), None, bn, 0.0, 0, None)
    unb = var * N / (N - 1)
    e_run = ((bn.running_var.cpu().double() - unb).abs() / unb)
    assert bool((e_run <= bound + R.U).all()), (e_run / bound).max()
    invstd = out.grad_fn.saved_tensors[2].cpu().double()
    implied = 1.0 / invstd ** 2 - R.EPS
    e_inv = (implied - var).abs() / var
    six = ((1 + R.U) ** 6 - 1) * (1 + R.EPS / var)
    assert bool((e_inv <= bound + six).all()), (e_inv / (bound + six)).max()
    assert torch.equal(bn.running_mean.cpu(), mean.float())
    print(f"K12-UNITS conditioning running_var={float((e_run / (bound + R.U)).max()):.4f} "
          f"invstd={float((e_inv / (bound + six)).max()):.4f} (fractions of the bound)")


def test_constant_columns(device):
    """var = 0 exactly (Σz and Σz² of small integers are exact): y = bias, so out = relu(bias)·scale
    exactly where kept and 0 where dropped; with a per-column constant dh, p = 0 and N a power of two
    dz = 0 exactly; running_var decays by (1 − momentum) in float32."""
    from oracle.dropout_hash import keep_mask

    N, C = 4096, 24
    z = torch.arange(C, dtype=torch.float32).sub(11).repeat(N, 1)
    bias = torch.linspace(-1, 1, C)
    dh = torch.tensor([0.5, -2.0, 1.0]).repeat(8)[:C].repeat(N, 1)
    a = SimpleNamespace(w=torch.rand(C) + 0.5, b=bias, rm=torch.zeros(C), rv=torch.rand(C) + 0.5)
    bn = _bn(device, C, a)
    res = _run(device, bn, z, None, dh, 0.5, SEED)
    keep = torch.from_numpy(keep_mask(SEED, N, C, 0.5))
    assert torch.equal(res.out.cpu(), torch.where(keep, torch.relu(bias) * 2, torch.zeros(())).expand(N, C))
    decay = torch.from_numpy((np.float32(1) - np.float32(0.1)) * a.rv.numpy())
    assert torch.equal(bn.running_var.cpu(), decay)
    res = _run(device, _bn(device, C, a), z, None, dh, 0.0, SEED)
    assert torch.equal(res.dz.cpu(), torch.zeros(N, C))
    assert torch.equal(res.dweight.cpu(), torch.zeros(C))  # x^ = 0
    assert torch.equal(res.dbias.cpu(), torch.where(bias > 0, dh[0] * N, torch.zeros(())))


def test_statistics_of_an_empty_shard(device):
    """gnn_bn_stats_f32 with N = 0: finalize = 0 writes [Σz | Σz² | n] = 0 (an empty shard's share of
    the all-reduce, z may be null); finalize = 1 is an argument error (no batch mean)."""
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.fused import _bn_ws_bytes

    C = 70
    stats = torch.full((2 * C + 2,), 7.0, dtype=torch.float64, device=device)
    ws = torch.empty(_bn_ws_bytes(C) // 4, dtype=torch.float32, device=device)
    mean = torch.full((C,), 3.0, device=device)
    invstd = torch.full((C,), 3.0, device=device)
    st = _lib.stream_handle(device)
    _lib.call("gnn_bn_stats_f32", None, C, 0, C, stats.data_ptr(), 0, 1e-5, 0.1, None, None, None, None, None,
              ws.data_ptr(), ws.numel() * 4, st)
    assert torch.equal(stats.cpu(), torch.tensor([0.0] * (2 * C + 1) + [7.0], dtype=torch.float64))
    stats.fill_(7.0)
    with pytest.raises(ValueError):
        _lib.call("gnn_bn_stats_f32", None, C, 0, C, stats.data_ptr(), 1, 1e-5, 0.1, mean.data_ptr(), invstd.data_ptr(),
                  None, None, None, ws.data_ptr(), ws.numel() * 4, st)
    torch.cuda.synchronize(device)
    assert float(stats.min()) == 7.0 and float(mean.min()) == 3.0 and float(invstd.max()) == 3.0


# ---------------------------------------------------------------------------------------------- K13
@pytest.mark.parametrize("N", [1, 2, 7])
@pytest.mark.parametrize("Fin", [1, 63, 256])
@pytest.mark.parametrize("dim", [1, 64, 600])
def test_time_inject_sin_edges(device, N, Fin, dim):
    """K13 at the two-rows-per-wave clamp (N = 1, 2, 7), the `c < F ? c : F − 1` clamp and a pass
    boundary exactly on F (Fin = 1, 63, 256), no sin / cos pair at all and time columns crossing a
    256-column pass (dim = 1, 64, 600), T = 2, timesteps of ±2^40 (the int64 clamp), x contiguous and as
    a column slice of a wider tensor (ldx > F).  Against the model's torch path at 1e-6, and against a
    float64 sinusoid within 2 u (1 + 2π k t): sinf's own error and, on the angle, the two float32
    roundings of (float)k · (float)2π (T = 2 makes t itself exactly 0 or 1)."""
    import math

    from elliptic_gnn_project_amd.fused import time_inject_sin
    from elliptic_gnn_project_amd.gnn import SAGEResBNNet

    T = 2
    g = torch.Generator().manual_seed(100 * N + Fin + dim)
    wide = torch.randn(N, Fin + 5, generator=g).to(device)
    t = torch.tensor([2, 1, -(2 ** 40), 2 ** 40, 0, 3, 2][:N], dtype=torch.int64, device=device)
    m = SAGEResBNNet(Fin, 16, layers=2, time_embed_dim=dim, time_embed_type="sin", max_timestep=T).to(device)
    half = dim // 2
    tc = (t.cpu() - 1).clamp(0, T - 1).double()[:, None]
    k = torch.arange(1, half + 1, dtype=torch.float64)[None, :]
    ang = 2 * math.pi * k * tc
    feat = torch.cat([torch.sin(ang), torch.cos(ang), torch.zeros(N, dim - 2 * half, dtype=torch.float64)], 1)
    bound = 2 * R.U * (1 + torch.cat([ang, ang, torch.zeros(N, dim - 2 * half, dtype=torch.float64)], 1))
    for x in (wide[:, 3:3 + Fin], wide[:, 3:3 + Fin].contiguous()):
        out = time_inject_sin(x, t, dim, T)
        assert out.shape == (N, Fin + dim)
        torch.testing.assert_close(out, torch.cat([x, m._sinusoid(t)], dim=1), rtol=1e-6, atol=1e-6)
        assert torch.equal(out[:, :Fin], x)
        assert bool(((out[:, Fin:].cpu().double() - feat).abs() <= bound).all())
        if dim % 2:
            assert torch.equal(out[:, -1], torch.zeros(N, device=device))
