"""Float64 CPU restatement of K12, the SAGE-ResBN layer tail h = dropout(relu(BatchNorm1d(z))) + r
(csrc/bn.hip), written for the tests (test infrastructure, not a test module): the whole forward and
backward, the nn.BatchNorm1d running-stat update, an optional second shard (SyncBN), the kernel's
block geometry in Python, the case table, and the derived error bounds (u = 2^-24 throughout).

Bounds (each checker returns the largest error in units of u times the magnitude it names, and
asserts it under the count of roundings derived here, never under a measured figure):

* forward, |out - ref| <= 12 u mag_out, mag_out = (|x^ w| + |b| + |mean| invstd |w|) scale + |r|:
  11 roundings (stored mean 1; stored invstd 4: cast, add, sqrt, divide; sub, mul, mul, add 4; the
  drop scale 1; the residual add 1).  |mean| invstd |w| is the float32 rounding of the stored mean.
* sums, |S_dev - S_ref| <= (K + 4) u Σ|terms|: K(N, C) = 4 ceil(ceil(N / 2048) / (8 lanes)) + lanes + 17
  is the longest chain of additions an addend passes through in bn_bwd_partial_kernel followed by
  bn_merge_kernel (4 per unrolled iteration in each of the two interleaved chains, 1 for their sum,
  `lanes` for the row-lane sum, at most 8 strided merge terms, the 8-level tree); terms |dy| for
  dbias and |dy x^| + |dy| |mean| invstd for dweight.  SyncBN adds one (the all-reduce): K + 1.
* dz, |dz - ref| <= (K + 12) u mag_dz, mag_dz = |w| invstd (|dy| + Σ|dy| / n + (|x^| + |mean| invstd) Σ|dy x^| / n).
* running statistics within 2 float32 ulps: new = (1 - m) old + m stat is formed in float32 from
  m (1 rounding; 1 / (nbt + 1) for the cumulative average), 1 - m (1), float32(stat) (1), the two
  products (1 each) and the sum (1): at most 3 u on either addend and u on the sum, 4 u = 2 ulps
  (2^-23) of (1 - m) |old| + m |stat|, which is the result's own magnitude wherever the addends do not
  cancel.

ReLU ties: where |y64| < 16 u mag_out the device and float64 may decide the ReLU either way, so the
reference takes the device's decision there (``device_pos``, read from a K12 forward of the same z
with p = 0 and no residual), as tests/relu_ties.py does for the model.  At most 1e-5 of a case's
elements may lie in that window (TIE_CAP, a condition on the inputs checked on the CPU).
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle.dropout_hash import keep_mask

U = 2.0 ** -24
EPS = 1e-5
TIE_CAP = 1e-5
GOLDEN = 0x9E3779B97F4A7C15
BLOCKS = 2048   # kBnBlocks
THREADS = 256   # kBnThreads
UNROLL = 8      # kBnU
FWD_ROUNDINGS = 12
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------ geometry (csrc/bn.hip, restated)
def lanes(C):
    return THREADS // min(C, THREADS)


def unit(C):
    return UNROLL * lanes(C)


def ceil_div(a, b):
    return -(-a // b)


def rows_per_block(N, C):
    return ceil_div(ceil_div(N, BLOCKS), unit(C)) * unit(C)


def grid(N, C):
    return min(max(ceil_div(N, lanes(C)), 1), BLOCKS)


def passes(C):
    return ceil_div(C, min(C, THREADS))


def chain(N, C):
    """K(N, C): the longest chain of float32 additions under one addend of the backward sums."""
    return 4 * ceil_div(ceil_div(N, BLOCKS), unit(C)) + lanes(C) + 17


WIDTHS = (1, 3, 8, 64, 100, 128, 129, 255, 256, 257, 600)
LONG_WIDTHS = (1, 64, 100, 257)


def case_table():
    """(N, C): N = 2 and one row on either side of a reduction unit at every width; at four widths
    also the apply kernels' first grid-stride trip and the first N at which the block height doubles."""
    cases = []
    for C in WIDTHS:
        ns = [2, unit(C) - 1, unit(C) + 1]
        if C in LONG_WIDTHS:
            ns += [BLOCKS * lanes(C) + 1, BLOCKS * unit(C) + 1]
        cases += [(n, C) for n in ns]
    return cases


SMALL_CASES = [(n, c) for n, c in case_table() if n * c <= 1 << 20]


def effective_seed(seed, ctr=None):
    """bn_seed: the seed a device counter turns ``seed`` into."""
    return (seed & MASK64) if ctr is None else ((ctr * GOLDEN + seed) & MASK64)


def drop_scale(p):
    """float32(1 / (1 - p)) as bn_args forms it from the float32 p."""
    return float(np.float32(1.0 / (1.0 - float(np.float32(p))))) if p > 0 else 1.0


# ------------------------------------------------------------------ inputs
def make_inputs(N, C, seed=0):
    """Seeded z = randn·2 + 0.3, r, dh, weight in [0.5, 1.5), small bias, running statistics."""
    g = torch.Generator().manual_seed(1000003 * C + N + seed)
    z = torch.randn(N, C, generator=g) * 2 + 0.3
    r = torch.randn(N, C, generator=g)
    dh = torch.randn(N, C, generator=g)
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g) * 0.1
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    return SimpleNamespace(z=z, r=r, dh=dh, w=w, b=b, rm=rm, rv=rv)


def integer_inputs(N, C, seed=0):
    """z in {-2..3}, dh in {-3..3} (exact in every float format), repaired so that no column's mean
    lies within 1e-3 of an integer: then no z - mean is a ReLU tie, dy is an integer (or twice one) and
    Σdy is exact in float32 in any order.  A draw alone cannot reach the precondition at N = 2 with
    hundreds of columns (every column's two values would have to differ in parity), so an offending
    column has one element moved by one, which shifts its mean by 1 / N."""
    g = torch.Generator().manual_seed(7000003 * C + N + seed)
    z = torch.randint(-2, 4, (N, C), generator=g).double()
    dh = torch.randint(-3, 4, (N, C), generator=g).float()
    for row in range(min(N, 4)):
        m = z.mean(0)
        bad = (m - m.round()).abs() < 1e-3
        if not bool(bad.any()):
            break
        z[row, bad] = torch.where(z[row, bad] < 3, z[row, bad] + 1, z[row, bad] - 1)
    return z.float(), dh


def integer_precondition(z, dh):
    m = z.double().mean(0)
    ok = bool(((m - m.round()).abs() >= 1e-3).all())
    return ok and float(dh.double().abs().sum(0).max()) * 2 < 2 ** 24  # every partial sum exact in float32


# ------------------------------------------------------------------ the reference
def _shard(z, r, dh, w, b, mean, invstd, p, seed, device_pos):
    N, C = z.shape
    scale = drop_scale(p)
    xh = (z - mean) * invstd
    y = xh * w + b
    mag = ((xh * w).abs() + b.abs() + mean.abs() * invstd * w.abs()) * scale
    if r is not None:
        mag = mag + r.abs()
    window = y.abs() < 16 * U * mag
    pos = y > 0
    if device_pos is not None:
        pos = torch.where(window, device_pos, pos)
    ks = torch.from_numpy(keep_mask(seed, N, C, p)).double() * scale if p > 0 else torch.ones((), dtype=torch.float64)
    out = torch.where(pos, y, torch.zeros((), dtype=torch.float64)) * ks
    if r is not None:
        out = out + r
    s = SimpleNamespace(xh=xh, out=out, mag_out=mag, ties=int(window.sum()), keep=ks)
    if dh is not None:
        s.dy = dh * ks * pos
        s.sum_dy, s.sum_dyx = s.dy.sum(0), (s.dy * xh).sum(0)
        s.abs_dy, s.abs_dyx = s.dy.abs().sum(0), (s.dy * xh).abs().sum(0)
    return s


def tail(z, r, w, b, p, seed, dh=None, other=None, device_pos=None, eps=EPS):
    """The float64 tail of one shard.  ``other`` = (z2, dh2): a second shard whose rows join the batch
    statistics and the backward sums (its dropout mask is keep_mask(seed, N2, C, p): each shard numbers
    its own elements).  Returns out, dz, dweight, dbias (local sums), the batch statistics and the
    magnitudes of the bounds; ``stats2`` / ``sums2`` are the other shard's all-reduce contributions."""
    d = lambda t: None if t is None else t.detach().cpu().double()
    z, r, w, b, dh = d(z), d(r), d(w), d(b), d(dh)
    N, C = z.shape
    z2, dh2 = (d(other[0]), d(other[1])) if other is not None else (None, None)
    n = N + (z2.size(0) if z2 is not None else 0)
    tot = z.sum(0) + (z2.sum(0) if z2 is not None else 0)
    mean = tot / n
    var = (((z - mean) ** 2).sum(0) + (((z2 - mean) ** 2).sum(0) if z2 is not None else 0)) / n
    invstd = 1.0 / torch.sqrt(var + eps)
    s = _shard(z, r, dh, w, b, mean, invstd, p, seed, device_pos)
    ref = SimpleNamespace(N=N, C=C, n=n, mean=mean, var=var, invstd=invstd, out=s.out, mag_out=s.mag_out,
                          ties=s.ties, xh=s.xh, keep=s.keep, K=chain(N, C) + (1 if other is not None else 0))
    if z2 is not None:
        ref.stats2 = torch.cat([z2.sum(0), (z2 * z2).sum(0), torch.tensor([float(z2.size(0))], dtype=torch.float64)])
    if dh is None:
        return ref
    sdy, sdyx, ady, adyx = s.sum_dy, s.sum_dyx, s.abs_dy, s.abs_dyx
    if z2 is not None:
        o = _shard(z2, None, dh2, w, b, mean, invstd, p, seed, None)
        ref.sums2 = torch.cat([o.sum_dy, o.sum_dyx])
        sdy, sdyx, ady, adyx = sdy + o.sum_dy, sdyx + o.sum_dyx, ady + o.abs_dy, adyx + o.abs_dyx
    k = w * invstd
    ref.dy = s.dy
    ref.dz = k * (s.dy - sdy / n - s.xh * sdyx / n)
    ref.mag_dz = k.abs() * (s.dy.abs() + ady / n + (s.xh.abs() + mean.abs() * invstd) * adyx / n)
    ref.dbias, ref.dweight = s.sum_dy, s.sum_dyx
    ref.mag_dbias = s.abs_dy
    ref.mag_dweight = s.abs_dyx + s.abs_dy * mean.abs() * invstd
    ref.dr = dh
    return ref


def running_update(rm, rv, nbt, mean, var, n, momentum):
    """nn.BatchNorm1d's update in float64: unbiased variance, fixed momentum or (None) the cumulative
    average.  Returns (running_mean, running_var, num_batches_tracked, their two magnitudes)."""
    rm, rv = rm.detach().cpu().double(), rv.detach().cpu().double()
    m = momentum if momentum is not None else 1.0 / (nbt + 1)
    unb = var * (n / max(n - 1.0, 1.0))
    return ((1 - m) * rm + m * mean, (1 - m) * rv + m * unb, nbt + 1,
            (1 - m) * rm.abs() + m * mean.abs(), (1 - m) * rv.abs() + m * unb)


# ------------------------------------------------------------------ checkers (shared by host and GPU tests)
def _units(dev, ref, mag):
    err = (dev.detach().cpu().double() - ref).abs()
    bad = (mag == 0) & (err > 0)
    if bool(bad.any()):
        return math.inf
    return float((err / torch.where(mag > 0, mag, torch.ones_like(mag))).max()) / U


def check_forward(out, ref):
    e = _units(out, ref.out, ref.mag_out)
    assert e <= FWD_ROUNDINGS, f"forward: {e:.2f} u·mag_out > {FWD_ROUNDINGS}"
    return e


def check_sums(dweight, dbias, ref):
    ew = _units(dweight, ref.dweight, ref.mag_dweight)
    eb = _units(dbias, ref.dbias, ref.mag_dbias)
    assert ew <= ref.K + 4, f"dweight: {ew:.2f} u·Σ|terms| > K + 4 = {ref.K + 4}"
    assert eb <= ref.K + 4, f"dbias: {eb:.2f} u·Σ|terms| > K + 4 = {ref.K + 4}"
    return ew, eb


def check_dz(dz, ref):
    e = _units(dz, ref.dz, ref.mag_dz)
    assert e <= ref.K + 12, f"dz: {e:.2f} u·mag_dz > K + 12 = {ref.K + 12}"
    return e


def check_running(bn, rm0, rv0, nbt0, ref, momentum):
    """bn's buffers after one call against the update of (rm0, rv0, nbt0): 2 float32 ulps, nbt exact."""
    rm, rv, nbt, mag_m, mag_v = running_update(rm0, rv0, nbt0, ref.mean, ref.var, float(ref.n), momentum)
    em = _units(bn.running_mean, rm, mag_m) / 2  # in ulps (2^-23)
    ev = _units(bn.running_var, rv, mag_v) / 2
    assert em <= 2 and ev <= 2, f"running stats: {em:.2f} / {ev:.2f} ulps > 2"
    assert int(bn.num_batches_tracked) == nbt
    return em, ev


def check_all(res, ref):
    """res: out, dz, dweight, dbias (and dr) of the code under test."""
    e = dict(fwd=check_forward(res.out, ref))
    e["dw"], e["db"] = check_sums(res.dweight, res.dbias, ref)
    e["dz"] = check_dz(res.dz, ref)
    if getattr(res, "dr", None) is not None:
        assert torch.equal(res.dr.detach().cpu().double(), ref.dr)
    return e


# ------------------------------------------------------------------ float32 emulation of the kernel formulas
def emulate_f32(z, r, w, b, p, seed, dh, other=None, mutate=None, eps=EPS):
    """K12's formulas in float32 on the CPU (statistics in float64 as on the device, elementwise work
    and sums in float32; torch's summation order, not the kernel's).  ``mutate`` plants the bugs the
    tests must reject: "drop_row" leaves the last row out of Σdy and Σdy·x^, "other_n" divides by the
    other shard's n, "mask_shift" hashes element i + 1."""
    f = torch.float32
    N, C = z.shape
    zd = z.double()
    z2 = other[0].double() if other is not None else None
    n = N + (z2.size(0) if z2 is not None else 0)
    n_used = z2.size(0) if mutate == "other_n" else n
    s1 = zd.sum(0) + (z2.sum(0) if z2 is not None else 0)
    s2 = (zd * zd).sum(0) + ((z2 * z2).sum(0) if z2 is not None else 0)
    m64 = s1 / n_used
    var64 = (s2 / n_used - m64 * m64).clamp_min(0)
    mean = m64.to(f)
    invstd = 1.0 / torch.sqrt(var64.to(f) + torch.tensor(eps, dtype=f))
    scale = torch.tensor(drop_scale(p), dtype=f)

    def shard(zz, rr, dd):
        rows = zz.size(0)
        xh = (zz - mean) * invstd
        y = xh * w + b
        if p > 0:
            if mutate == "mask_shift":
                keep = torch.from_numpy(keep_mask(seed, rows * C + 1, 1, p).reshape(-1)[1:].reshape(rows, C).copy())
            else:
                keep = torch.from_numpy(keep_mask(seed, rows, C, p))
        else:
            keep = torch.ones(rows, C, dtype=torch.bool)
        out = torch.where(keep, torch.relu(y) * scale, torch.zeros((), dtype=f))
        if rr is not None:
            out = out + rr
        dy = torch.where(keep & (y > 0), dd * scale, torch.zeros((), dtype=f))
        return xh, out, dy

    xh, out, dy = shard(z, r, dh)
    rows = slice(0, N - 1) if mutate == "drop_row" else slice(0, N)
    sdy, sdyx = dy[rows].sum(0), (dy[rows] * xh[rows]).sum(0)
    tdy, tdyx = sdy, sdyx
    if other is not None:
        xh2, _, dy2 = shard(other[0], None, other[1])
        tdy, tdyx = sdy + dy2.sum(0), sdyx + (dy2 * xh2).sum(0)
    inv_n = torch.tensor(1.0 / n_used, dtype=f)
    dz = (w * invstd) * (dy - tdy * inv_n - xh * (tdyx * inv_n))
    return SimpleNamespace(out=out, dz=dz, dweight=sdyx, dbias=sdy, dr=dh, mean=m64, var=var64, n=n_used)
