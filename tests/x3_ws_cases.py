"""Cases, inputs, float64 references and checkers of the weight-stationary split-bf16 NT tests
(test_gpu_x3_ws on the device, test_x3_ws_host for what the cases and the checkers claim).  Plain
helper module: no test lives here.

The kernel (gemm_ws.hip gemm_nt_ws_kernel<NKS, EPI, KS>): f32 A1 | A2 and f32 W1 | W2, each split
into hi / mid / lo bf16 planes, six plane products per 16-deep k-step accumulated in f32 by MFMAs.
One block per CU sweeps the 32-row tiles t = block, block + grid, ...; two LDS A buffers and two
staging register sets alternate, the prologue loads the block's first three tiles, and a tile's
loads are first issued inside the loop at the block's 4th tile: the steady state is a block's 4th
and 5th tile on.  ``nt_rows(cus)`` (bf16_image_cases) gives blocks of 1-2, 2-3, 3-4 and 6-7 tiles,
the last with a 13-row tail as the 7th tile of its block; ``TINY_M`` adds grids of 1 and 2 blocks.

The dispatch, restated from gemm_ws.hip as read (``nt_ws_ok``, ``nks_of``, ``ks_of``, ``epi_flags``):
nt_ws_ok takes f32 operands with dense even-k segments, 16-byte C rows, Nc % 4 == 0, 64 < Nc <= 128,
M >= 32, ceil((k1 + k2) / 16) in {8, 11, 16, 21} and an epilogue among plain | bias | bias + ReLU |
bias + ReLU + dropout, the last two with or without the projection; launch_nt_ws splits K over a
wave pair (KS = 2) except at 21 k-steps; with_nt_epi (shared by the four
weight-stationary NT launchers) picks EPI from (proj, dropout, relu, bias).

The checkers (``check``, ``check_z``), u = 2^-24, D = |A| |W|^T and b the bias:
 1. ceiling: |c - ref| <= (96 NKS + 4) 2^-23 1.01 (D + |b|) / (1 - p).  At most 96 NKS accumulations
    inside the MFMAs (6 instructions x 16 products per k-step), the K-half add, the bias add and the
    dropout scale, each wrong by at most one f32 ulp of a magnitude <= (1 + 2^-8)^2 D (whichever way
    the unit rounds inside an instruction), plus the dropped mid x lo, lo x mid, lo x lo terms at
    2^-26 D.  The net for gross errors: a wrong row, a stale buffer, a lost k-step or hi / mid product.
 2. exact zeros: c == 0 where the keep mask (oracle.dropout_hash) is off and where ReLU sees
    ref + b < -ceiling; c != 0 where ref + b > ceiling and the element is kept.  The band
    |ref + b| <= ceiling is left out of this test only, and may hold 1 % of a case's elements.
 3. the statistic S(X) = sqrt(mean(((c - ref) / (u (D + |b|) / (1 - p)))^2)) over the live elements
    (kept, and not cut by ReLU in the reference) of X: at most 4 S_cpu for every 32-row tile, and
    in the plain and bias epilogues for every row, S_cpu the statistic of the CPU float32 product
    of the same operands over the whole matrix (the factor bf16_image_cases grants MFMA order against
    BLAS order).  One dropped plane product of the six moves it past that.
 4. z against the stored C: |z - c P^T| <= (Nc + 2) 2^-24 |c| |P|^T (an f32 dot of Nc terms in any
    order).
"""
import functools
import json
from pathlib import Path
from types import SimpleNamespace

import torch

from bf16_image_cases import (DEEP, DROP_P, DROP_SEED, EPIS, HOST_CUS, ROW_EXPS, U24, _seed, effective_seed, nt_ranges,
                              nt_rows, nt_sweep, nt_tiles)
from oracle.dropout_hash import keep_mask

__all__ = ["DEEP", "DROP_P", "DROP_SEED", "EPIS", "HOST_CUS", "ROW_EXPS", "effective_seed", "nt_ranges", "nt_rows",
           "nt_sweep", "nt_tiles"]

STATS_FILE = Path(__file__).resolve().parent / "golden" / "x3_ws_cpu_stats.json"
TINY_M = (32, 33, 45)          # shapes 4, 5, 6: one full tile, a 1-row and a 13-row tail (grid 1, 2, 2)
STAT_FACTOR = 4.0
BAND_CAP = 0.01
WS_BIAS, WS_RELU, WS_DROP, WS_PROJ = 1, 2, 4, 8


def rows(cus):
    """M of the shapes 0 .. 6."""
    return nt_rows(cus) + TINY_M


# ------------------------------------------------------------------------- the dispatch, restated
def nks_of(k1, k2):
    return (k1 + k2 + 15) // 16


def ks_of(nks):
    """launch_nt_ws: K parts per column group."""
    return 1 if nks == 21 else 2


def epi_flags(epi):
    """with_nt_epi (gemm_ws.hip): the EPI template argument of an epilogue (bias, relu, dropout, proj)."""
    bias, relu, drop, proj = EPIS[epi]
    if proj and drop:
        return WS_BIAS | WS_RELU | WS_DROP | WS_PROJ
    if proj:
        return WS_BIAS | WS_RELU | WS_PROJ
    if drop:
        return WS_BIAS | WS_RELU | WS_DROP
    if relu:
        return WS_BIAS | WS_RELU
    return WS_BIAS if bias else 0


def nt_ws_ok(M, k1, k2, nc, epi, ldc=None, ldz=4):
    """nt_ws_ok for f32 A and C, dense 16-byte aligned operands (lda == k) and the w1/w2 form."""
    bias, relu, drop, proj = EPIS[epi]
    ldc = nc if ldc is None else ldc
    if nc > 128 or nc < 1 or k1 % 2 or k2 % 2:
        return False
    if ldc % 4 or M * ldc * 4 >= 2 ** 31 or nc % 4 or (proj and M * ldz * 4 >= 2 ** 31):
        return False
    if nks_of(k1, k2) not in (8, 11, 16, 21) or M < 32 or M * max(k1, k2) >= 2 ** 40 or nc <= 64:
        return False
    return not ((drop or proj or relu) and not (relu and bias))


def instantiation(case):
    """(NKS, EPI, KS) of gemm_nt_ws_kernel a case launches."""
    s, k1, k2, nc, epi = case
    nks = nks_of(k1, k2)
    return nks, epi_flags(epi), ks_of(nks)


def pad_cols(k1, k2):
    return 16 * nks_of(k1, k2) - k1 - k2


# ------------------------------------------------------------------------------------ the cases
# K pairs per NKS: every NKS has a segment with k % 4 == 2 (staging quads straddle two rows), a k1
# inside a k-step, a pair without pad columns and a single-segment call
K_PAIRS = {8: ((64, 64), (114, 0), (50, 70)), 11: ((166, 0), (86, 84), (90, 86)),
           16: ((128, 128), (250, 0), (6, 246)), 21: ((166, 166), (150, 180), (336, 0))}
# (shape index, k1, k2, Nc, epilogue).  Cases of one (shape, k1, k2, Nc) are adjacent: they share
# their products.  Nc 68: column group 3 dead, group 2 partly dead.
NT_CASES = [
    (DEEP, 64, 64, 128, "plain"), (DEEP, 64, 64, 128, "drop_proj"), (DEEP, 114, 0, 100, "bias"), (DEEP, 114, 0, 100, "proj"),
    (DEEP, 50, 70, 68, "bias_relu"), (DEEP, 50, 70, 68, "drop"),
    (DEEP, 166, 0, 128, "plain"), (DEEP, 166, 0, 128, "drop"), (DEEP, 86, 84, 68, "bias"), (DEEP, 86, 84, 68, "drop_proj"),
    (DEEP, 90, 86, 100, "bias_relu"), (DEEP, 90, 86, 100, "proj"),
    (DEEP, 128, 128, 100, "plain"), (DEEP, 128, 128, 100, "proj"), (DEEP, 250, 0, 68, "bias_relu"), (DEEP, 250, 0, 68, "drop_proj"),
    (DEEP, 6, 246, 128, "bias"), (DEEP, 6, 246, 128, "drop"),
    (DEEP, 166, 166, 128, "plain"), (DEEP, 166, 166, 128, "drop_proj"), (DEEP, 150, 180, 100, "bias"), (DEEP, 150, 180, 100, "drop"),
    (DEEP, 336, 0, 68, "bias_relu"), (DEEP, 336, 0, 68, "proj"),
    (0, 114, 0, 128, "drop"), (0, 86, 84, 100, "plain"), (0, 6, 246, 68, "proj"), (0, 166, 166, 128, "bias"),
    (1, 50, 70, 100, "proj"), (1, 166, 0, 68, "bias_relu"), (1, 128, 128, 128, "drop_proj"), (1, 336, 0, 100, "plain"),
    (2, 64, 64, 68, "bias"), (2, 90, 86, 128, "drop_proj"), (2, 250, 0, 100, "plain"), (2, 150, 180, 68, "drop"),
    (4, 64, 64, 128, "plain"), (4, 166, 0, 100, "drop_proj"), (4, 6, 246, 128, "bias_relu"), (4, 166, 166, 68, "proj"),
    (5, 114, 0, 68, "drop_proj"), (5, 86, 84, 128, "bias"), (5, 250, 0, 128, "drop"), (5, 150, 180, 128, "plain"),
    (6, 50, 70, 128, "bias_relu"), (6, 90, 86, 100, "drop"), (6, 128, 128, 68, "plain"), (6, 336, 0, 128, "drop_proj"),
]
RANGE_CASES = [c for c in NT_CASES if c[0] == DEEP and not EPIS[c[4]][2]]  # the bitwise row-range check
SEED_CASE = (1, 128, 128, 128, "drop_proj")   # run once more through seed_ptr
NO_C_CASE = (DEEP, 128, 128, 100, "proj")     # run once more with want_c=False
# the classic gemm_nt_x3_kernel (128-row tiles): what the default GCN / GAT and hidden-64 SAGE send
X3_M = 128 * 3 + 13
X3_CASES = [(k1, k2, 64, epi) for k1, k2 in ((166, 0), (64, 64)) for epi in ("plain", "bias_relu", "drop", "proj")]


def nt_id(case):
    s, k1, k2, nc, epi = case
    return f"s{s}-{k1}+{k2}-n{nc}-{epi}"


def stat_id(s, k1, k2, nc):
    return f"s{s}-{k1}+{k2}-n{nc}"


# ----------------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=2)
def operands(M, k1, k2, nc):
    """f32 inputs (full 24-bit significands: every bf16 plane carries bits) and the products every
    epilogue of (M, k1, k2, Nc) shares; never modified.  A row r is scaled by 2^-ROW_EXPS[r % 8], W row
    n by 0.1 2^-(n % 3), so a small output comes with a small D."""
    g = torch.Generator().manual_seed(_seed(M, k1, k2, nc, 3))
    rs = (2.0 ** -torch.tensor(ROW_EXPS)[torch.arange(M) % len(ROW_EXPS)].float())[:, None]
    cs = (0.1 * 2.0 ** -(torch.arange(nc) % 3).float())[:, None]
    a1 = torch.randn(M, k1, generator=g) * rs
    a2 = torch.randn(M, k2, generator=g) * rs if k2 else None
    w1 = torch.randn(nc, k1, generator=g) * cs
    w2 = torch.randn(nc, k2, generator=g) * cs if k2 else None
    bias = torch.randn(nc, generator=g) * 0.2
    proj = torch.randn(4, nc, generator=g)
    A = torch.cat([a1, a2], 1) if k2 else a1
    W = torch.cat([w1, w2], 1) if k2 else w1
    A64, W64 = A.double(), W.double()
    op = SimpleNamespace(M=M, k1=k1, k2=k2, nc=nc, nks=nks_of(k1, k2), a1=a1, a2=a2, w1=w1, w2=w2, bias=bias, proj=proj,
                         A=A, W=W, s64=A64 @ W64.t(), D=A64.abs() @ W64.abs().t(), cpu32=A @ W.t())
    op.s_cpu = float(((op.cpu32.double() - op.s64) / (U24 * op.D)).square().mean().sqrt())
    return op


def drop_scale32():
    """NTArgs::drop_scale: (float)(1 / (1 - (double)p)), p the float32 probability."""
    return torch.tensor(1.0 / (1.0 - float(torch.tensor(DROP_P, dtype=torch.float32))), dtype=torch.float32)


def apply_epilogue(c, op, epi, keep):
    """The epilogue in float32 on a float32 product c, operation by operation as the kernel's."""
    bias, relu, drop, proj = EPIS[epi]
    if bias:
        c = c + op.bias
    if relu:
        c = torch.relu(c)
    if drop:
        c = torch.where(keep, c * drop_scale32(), torch.zeros(()))
    return c


def reference_of(M, k1, k2, nc, epi, seed=DROP_SEED, nks=None):
    """float64 reference of one call: ref, the ceiling, the sets that must (not) be exactly zero, the
    live set and unit of the statistic, the keep mask and the CPU float32 evaluation (``cpu``)."""
    op = operands(M, k1, k2, nc)
    bias, relu, drop, proj = EPIS[epi]
    nks = nks or op.nks
    mag = op.D + (op.bias.double().abs() if bias else 0.0)
    pre = op.s64 + (op.bias.double() if bias else 0.0)
    ceil0 = (96 * nks + 4) * 2.0 ** -23 * 1.01 * mag
    keep = torch.from_numpy(keep_mask(seed, M, nc, DROP_P)) if drop else None
    kept = keep if drop else torch.ones(pre.shape, dtype=torch.bool)
    ps = 1.0 / (1.0 - float(torch.tensor(DROP_P, dtype=torch.float32))) if drop else 1.0
    ref = (torch.relu(pre) if relu else pre) * kept * ps
    zero = ~kept | ((pre < -ceil0) if relu else torch.zeros_like(kept))
    nonzero = kept & ((pre > ceil0) if relu else (pre.abs() > ceil0))
    live = kept & ((pre > 0) if relu else torch.ones_like(kept))
    return SimpleNamespace(op=op, M=M, nc=nc, epi=epi, nks=nks, ref=ref, ceil=ceil0 * ps, unit=U24 * mag * ps, zero=zero,
                           nonzero=nonzero, live=live, keep=keep, band=float((~zero & ~nonzero).double().mean()),
                           rows_live=not relu and not drop, cpu=apply_epilogue(op.cpu32, op, epi, keep),
                           proj=op.proj if proj else None)


def reference(case, cus, seed=DROP_SEED):
    s, k1, k2, nc, epi = case
    return reference_of(rows(cus)[s], k1, k2, nc, epi, seed)


def row_slice(r, r0, r1):
    """The reference of rows [r0, r1) alone (r0 a multiple of the tile)."""
    out = SimpleNamespace(**vars(r))
    for k in ("ref", "ceil", "unit", "zero", "nonzero", "live"):
        setattr(out, k, getattr(r, k)[r0:r1])
    out.M = r1 - r0
    out.band = float((~out.zero & ~out.nonzero).double().mean())
    return out


def check(r, c, tile=32):
    """An output c (float32, CPU) against a reference: the counts of elements past the ceiling, of
    nonzero elements that must be exactly zero and of zeros that must not be, the statistic of every
    ``tile``-row tile and (plain, bias) of every row, the worst ceiling ratio and its place."""
    c64 = c.double()
    err = (c64 - r.ref).abs()
    bad = ~(err <= r.ceil)  # a NaN is bad
    ratio = torch.nan_to_num(err / r.ceil.clamp_min(1e-300), nan=float("inf"))
    at = int(ratio.argmax())
    q = torch.where(r.live, (err / r.unit).square(), torch.zeros((), dtype=torch.float64))
    nt = -(-r.M // tile)
    tid = torch.arange(r.M) // tile
    num = torch.zeros(nt, dtype=torch.float64).index_add_(0, tid, q.sum(1))
    cnt = torch.zeros(nt, dtype=torch.float64).index_add_(0, tid, r.live.sum(1).double())
    tile_s = (num / cnt.clamp_min(1.0)).sqrt()
    row_s = (q.sum(1) / r.live.sum(1).clamp_min(1)).sqrt() if r.rows_live else None
    return SimpleNamespace(n=c64.numel(), ceil_bad=int(bad.sum()), zero_bad=int((r.zero & (c64 != 0)).sum()),
                           nonzero_bad=int((r.nonzero & (c64 == 0)).sum()), worst=float(ratio.flatten()[at]),
                           worst_at=divmod(at, c64.size(1)), tile_s=tile_s, row_s=row_s, min_live=int(cnt.min()))


def failures(r, c, s_cpu, tile=32):
    """The names of the checkers an output fails (empty: it passes), for the tests to assert on."""
    res = check(r, c, tile)
    allow = STAT_FACTOR * s_cpu
    out = []
    if res.ceil_bad:
        out.append("ceiling")
    if res.zero_bad or res.nonzero_bad:
        out.append("zeros")
    if not bool((res.tile_s <= allow).all()):
        out.append("tile")
    if res.row_s is not None and not bool((res.row_s <= allow).all()):
        out.append("row")
    return out, res


def check_z(r, c, z):
    """z = c P^T of the stored c per row: the number of elements past (Nc + 2) 2^-24 |c| |P|^T."""
    c64, P = c.double(), r.proj.double()
    zb = (c64.size(1) + 2) * U24 * (c64.abs() @ P.abs().t())
    return int((~((z.double() - c64 @ P.t()).abs() <= zb)).sum())


# ------------------------------------------------------------------------------ the yardstick
def recorded_stats():
    return json.loads(STATS_FILE.read_text())


def stat_keys():
    return sorted({(s, k1, k2, nc) for s, k1, k2, nc, _ in NT_CASES})


def compute_stats(cus=HOST_CUS, keys=None):
    """{stat_id: S_cpu}: the table golden/make_x3_ws_stats.py writes."""
    return {stat_id(*k): round(operands(rows(cus)[k[0]], *k[1:]).s_cpu, 6) for k in (keys or stat_keys())}


def s_cpu_of(case, cus):
    """The yardstick of a case: the recorded one at the 256 CUs the table was made for (and at the
    tiny M, which no CU count changes), evaluated on the spot on any other device (other M)."""
    s, k1, k2, nc, _ = case
    if cus == HOST_CUS or s > DEEP:
        return recorded_stats()[stat_id(s, k1, k2, nc)]
    return operands(rows(cus)[s], k1, k2, nc).s_cpu


# ----------------------------------------------------------------- the six-term emulation (host)
def split3(x):
    """hi, mid, lo bf16 planes of a float32 tensor (RNE, exact remainders), as float32."""
    hi = x.to(torch.bfloat16).float()
    mid = (x - hi).to(torch.bfloat16).float()
    lo = (x - hi - mid).to(torch.bfloat16).float()
    return hi, mid, lo


TERMS = ("lh", "mm", "mh", "hl", "hm", "hh")  # (A plane, W plane) in the kernel's order: small terms first


def emulate(op, drop_term=None, skip_step=None):
    """The kernel's arithmetic on the CPU: per 16-deep k-step the six plane products accumulated in
    float32 (exact bf16 x bf16 products, float32 sums), the K parts of KS = 2 added last.
    ``drop_term``: one of TERMS left out; ``skip_step``: one k-step left out."""
    pa = dict(zip("hml", split3(op.A)))
    pw = dict(zip("hml", split3(op.W)))
    K, nks = op.A.size(1), op.nks
    kh0 = -(-nks // ks_of(nks))
    parts = [torch.zeros(op.M, op.nc), torch.zeros(op.M, op.nc)]
    for s in range(nks):
        if s == skip_step:
            continue
        k0, k1 = 16 * s, min(16 * s + 16, K)
        for t in TERMS:
            if t != drop_term:
                parts[s >= kh0] += pa[t[0]][:, k0:k1] @ pw[t[1]][:, k0:k1].t()
    return parts[0] + parts[1]
