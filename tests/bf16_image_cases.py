"""Cases, inputs, float64 references and checkers of the bf16 image GEMM tests (test_gpu_bf16_image
on the device, test_bf16_image_host for what the cases and the checkers claim).  Plain helper
module: no test lives here.

NT (gemm_ws.hip gemm_nt_img16_kernel): one block per CU sweeps the 32-row tiles t = block,
block + grid, ... through a 4-buffer LDS-DMA ring with counted waits that differ at a block's
first, second and later tiles.  ``nt_rows(cus)`` gives the smallest M at which a block runs 2, 3, 4
and 7 tiles (the last with a 13-row tail tile as the 7th tile of its block); ``NT_CASES`` crosses
them with both image widths, a gapped and an ungapped operand pair each, three output widths and
the six epilogues.

TN (gemm_planes.hip gemm_tn_img16_kernel): ``TN_M`` are the M whose row blocks hold 4, 6 and 8
16-row chunks with a short last block of 3, 5, 7 and 1 chunks (the last one reached through the
M - 16 clamp), the plan of gemm_dispatch.hip's tn_rows restated in ``tn_rows`` and asserted below.
Forms: "dz_mask" (dz, proj, h), "g_mask" (g, h), "g" (g alone), "dz" (dz, proj, no h), each with
and without gout, with f32 and bf16 g / gout.  gemm_tn(check_planes=True) accepts every one of
them over a BfImage (Nr % 4 == 0, bf16 h, g and gout of one dtype); none is left out.

The NT bound.  The kernel stores c = RNE_bf16(epi(s)), s the f32-accumulated sum of exact bf16
products, so |s - ref| <= delta = K 2^-24 (|A| |RNE(W)|^T) per element (K the image width: at most
K - 1 roundings of partial sums no larger than the sum of the terms' magnitudes), scaled by
1 / (1 - p) under dropout.  Rounding adds half a bf16 ulp of a value within delta of ref:
    |c - ref| <= 2^-8 (|ref| + delta) + delta         on every element,
    c == 0 exactly where the keep mask is off or ReLU sees ref + b < -delta.
Inputs carry a power-of-two scale per A row and per W row, so small outputs come with a small
delta and the bound stays a few bf16 ulps of the element itself across 2^-11 .. 1 of magnitude.

delta is a worst case.  ``misrounded`` counts the elements with c != RNE_bf16(ref); the allowance
is four times the count of the same operation evaluated in float32 on the CPU (``cpu``: the same
error scale, another summation order; MFMA's blocked order against BLAS's is the factor), at least
one element.  The CPU counts at 256 CUs are recorded in golden/bf16_image_cpu_shares.json.
"""
import functools
import json
import math
from pathlib import Path
from types import SimpleNamespace

import torch

from oracle.dropout_hash import keep_mask

U24 = 2.0 ** -24
BF_ULP = 2.0 ** -8
HOST_CUS = 256
PHI64 = 0x9E3779B97F4A7C15
DROP_P = 0.3
DROP_SEED = 0x0BAD_5EED_1234_ABCD   # both 32-bit halves of the seed take part in the hash
SHARES_FILE = Path(__file__).resolve().parent / "golden" / "bf16_image_cpu_shares.json"


def _seed(*parts):
    return int(sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts))) % (2 ** 31)


def rb(t):
    """Round to bf16 (RNE), back to the computing dtype (float32 inputs only: one rounding)."""
    return t.to(torch.bfloat16).to(t.dtype)


def rne_bf16(x):
    """RNE of a float64 tensor to bf16's 8-bit significand, in one rounding, as float64 (torch's
    double -> bfloat16 cast rounds through float32 first: a double rounding at 2^-16 of the
    values, as many as the share measured here)."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def image_ld(k1, k2):
    """planes.BfImage's layout restated: (col2, ld)."""
    col2 = (k1 + 7) // 8 * 8
    return col2, (col2 + (k2 + 7) // 8 * 8 + 15) // 16 * 16


# ------------------------------------------------------------------------------------------ NT
def nt_tiles(cus):
    return (cus + 3, 2 * cus + cus // 2, 3 * cus + 1, 6 * cus + 77)


def nt_rows(cus):
    t = nt_tiles(cus)
    return (32 * t[0], 32 * t[1], 32 * t[2], 32 * (t[3] - 1) + 13)


def nt_sweep(M, cus):
    """launch_nt_img16_k restated: (grid, fewest and most tiles of a block, (block, position) of
    the last tile)."""
    ntiles = -(-M // 32)
    grid = min(ntiles, cus)
    last = ntiles - 1
    return grid, ntiles // grid, -(-ntiles // grid), (last % grid, last // grid)


EPIS = {  # name -> (bias, relu, dropout, proj): the six instantiations of launch_nt_img16_k
    "plain": (0, 0, 0, 0), "bias": (1, 0, 0, 0), "bias_relu": (1, 1, 0, 0),
    "drop": (1, 1, 1, 0), "proj": (1, 1, 0, 1), "drop_proj": (1, 1, 1, 1),
}
DEEP = 3
ROW_EXPS = (0, 1, 2, 3, 4, 6, 9, 9)  # A row r is scaled by 2^-ROW_EXPS[r % 8]: rows 8j + 6, 8j + 7 are both tiny
# (shape index, k1, k2, Nc, epilogue); ld 256: (128, 128) and the gapped (100, 150) (col2 104);
# ld 336: (166, 166) and (150, 180) (col2 152).  Cases of one (shape, k1, k2, Nc) are adjacent: they
# share their products.
NT_CASES = [
    (DEEP, 128, 128, 128, "plain"), (DEEP, 128, 128, 128, "proj"), (DEEP, 128, 128, 72, "bias_relu"),
    (DEEP, 100, 150, 128, "bias"), (DEEP, 100, 150, 128, "drop"), (DEEP, 100, 150, 8, "drop_proj"),
    (DEEP, 166, 166, 128, "plain"), (DEEP, 166, 166, 128, "bias_relu"), (DEEP, 166, 166, 8, "proj"),
    (DEEP, 150, 180, 128, "drop"), (DEEP, 150, 180, 128, "drop_proj"), (DEEP, 150, 180, 72, "bias"),
    (0, 128, 128, 128, "plain"), (0, 100, 150, 72, "drop_proj"), (0, 166, 166, 72, "plain"), (0, 150, 180, 128, "drop_proj"),
    (1, 100, 150, 128, "plain"), (1, 128, 128, 128, "drop_proj"), (1, 150, 180, 8, "plain"), (1, 166, 166, 72, "drop_proj"),
    (2, 128, 128, 8, "plain"), (2, 100, 150, 128, "drop_proj"), (2, 166, 166, 128, "plain"), (2, 150, 180, 72, "drop_proj"),
]
RANGE_CASES = [c for c in NT_CASES if c[0] == DEEP and not EPIS[c[4]][2]]  # the bitwise range check


def nt_id(case):
    s, k1, k2, nc, epi = case
    return f"s{s}-{k1}+{k2}-n{nc}-{epi}"


def nt_ranges(cus):
    """Row ranges of the deepest shape, each at most 32 cus rows from a multiple of 32: tiles at
    sweep positions 1-2, 3-4 and 5-6 of their blocks, the last range ending in the tail tile."""
    T, M = nt_tiles(cus)[DEEP], nt_rows(cus)[DEEP]
    return [(32 * (cus + 5), 32 * (2 * cus + 5)), (32 * (3 * cus + cus // 2), 32 * (4 * cus + cus // 2)),
            (32 * (T - cus), M)]


@functools.lru_cache(maxsize=2)
def nt_operands(M, k1, k2, nc):
    """Inputs and the three products every epilogue of (M, k1, k2, Nc) shares; never modified."""
    g = torch.Generator().manual_seed(_seed(M, k1, k2, nc))
    rs = (2.0 ** -torch.tensor(ROW_EXPS)[torch.arange(M) % len(ROW_EXPS)].float())[:, None]
    cs = (0.1 * 2.0 ** -(torch.arange(nc) % 3).float())[:, None]
    a1 = (torch.randn(M, k1, generator=g) * rs).to(torch.bfloat16)
    a2 = (torch.randn(M, k2, generator=g) * rs).to(torch.bfloat16)
    w1 = torch.randn(nc, k1, generator=g) * cs
    w2 = torch.randn(nc, k2, generator=g) * cs
    bias = torch.randn(nc, generator=g) * 0.2
    proj = torch.randn(4, nc, generator=g)
    A = torch.cat([a1, a2], 1)
    Wb = rb(torch.cat([w1, w2], 1))
    A64, W64 = A.double(), Wb.double()
    return SimpleNamespace(M=M, k1=k1, k2=k2, nc=nc, K=image_ld(k1, k2)[1], a1=a1, a2=a2, w1=w1, w2=w2, bias=bias,
                           proj=proj, s64=A64 @ W64.t(), absdot=A64.abs() @ W64.abs().t(), s32=A.float() @ Wb.float().t())


def effective_seed(seed, counter=None):
    """gemm_nt's seed with the device counter seed_ptr set: *seed_ptr * phi + seed (mod 2^64)."""
    return seed if counter is None else (counter * PHI64 + seed) & 0xFFFFFFFFFFFFFFFF


def nt_reference(case, cus, seed=DROP_SEED):
    """float64 reference, delta, the exact-zero set, the keep mask and the CPU float32 evaluation
    (``cpu``, bf16) of one case."""
    s, k1, k2, nc, epi = case
    op = nt_operands(nt_rows(cus)[s], k1, k2, nc)
    bias, relu, drop, proj = EPIS[epi]
    ref, delta, c32 = op.s64, op.K * U24 * op.absdot, op.s32
    zero = torch.zeros(ref.shape, dtype=torch.bool)
    keep = None
    if bias:
        ref = ref + op.bias.double()
        c32 = c32 + op.bias
    if relu:
        zero = ref < -delta
        ref, c32 = torch.relu(ref), torch.relu(c32)
    if drop:
        keep = torch.from_numpy(keep_mask(seed, op.M, nc, DROP_P))
        p32 = float(torch.tensor(DROP_P, dtype=torch.float32))
        ref = ref * keep / (1.0 - p32)
        delta = delta / (1.0 - p32)
        c32 = torch.where(keep, c32 * torch.tensor(1.0 / (1.0 - p32), dtype=torch.float32), torch.zeros(()))
        zero = zero | ~keep
    return SimpleNamespace(op=op, ref=ref, delta=delta, zero=zero, keep=keep, cpu=c32.to(torch.bfloat16),
                           proj=op.proj if proj else None)


def nt_check(r, c):
    """The three per-element findings of an output c (bf16, CPU) against nt_reference's r: counts
    of elements outside the bound, of nonzero elements that must be exactly zero, and of
    misrounded ones, with the worst bound ratio and its place."""
    c64 = c.double()
    bound = BF_ULP * (r.ref.abs() + r.delta) + r.delta
    err = (c64 - r.ref).abs()
    bad = ~(err <= bound)  # a NaN is bad
    ratio = err / bound.clamp_min(1e-300)
    at = int(torch.nan_to_num(ratio, nan=math.inf).argmax())
    return SimpleNamespace(n=c64.numel(), bound_bad=int(bad.sum()), zero_bad=int((r.zero & (c64 != 0)).sum()),
                           misrounded=int((c64 != rne_bf16(r.ref)).sum()), worst=float(ratio.flatten()[at]),
                           worst_at=divmod(at, c64.size(1)))


def nt_bound_misses(c, ref, absdot, K, scale=1.0):
    """Elements of c outside 2^-8 (|ref| + delta) + delta, delta = K 2^-24 absdot scale (module
    docstring), for a caller with its own inputs: absdot = |A| |RNE(W)|^T in float64, K the depth
    of the sum, scale the dropout's 1 / (1 - p)."""
    delta = K * U24 * absdot * scale
    return int((~((c.double() - ref).abs() <= BF_ULP * (ref.abs() + delta) + delta)).sum())


def nt_check_z(r, c, z):
    """z = h P^T of the stored h per row: |z - c P^T| <= Nc 2^-24 |c| |P|^T; the number of misses."""
    c64, P = c.double(), r.proj.double()
    zb = c64.size(1) * U24 * (c64.abs() @ P.abs().t())
    return int((~((z.double() - c64 @ P.t()).abs() <= zb)).sum())


def old_max_check(c, ref):
    """What test_gpu_bf16 asserted before: the largest error against the largest tolerance."""
    d = (c.double() - ref).abs()
    return float(d.max()) <= float((BF_ULP * ref.abs() + 1e-5).max())


def misround_allowance(cpu_count):
    return max(4 * int(cpu_count), 1)


def recorded_shares():
    return json.loads(SHARES_FILE.read_text())


def cpu_misrounded(case, cus, r=None):
    """The CPU float32 evaluation's misrounded count: the recorded one at the 256 CUs the table
    was made for, evaluated on the spot on any other device (other M)."""
    if cus == HOST_CUS:
        return recorded_shares()[nt_id(case)]["cpu"]
    r = r or nt_reference(case, cus)
    return nt_check(r, r.cpu).misrounded


# ------------------------------------------------------------------------------------------ TN
TN_BLOCKS = 256
TN_M = (12_776, 20_134, 29_412, 12_741)
# M -> (blocks, rows per block, rows of the last block, 16-row chunks of a full block, of the last)
TN_PLAN = {12_776: (200, 64, 40, 4, 3), 20_134: (210, 96, 70, 6, 5), 29_412: (230, 128, 100, 8, 7),
           12_741: (200, 64, 5, 4, 1)}


def tn_rows(M, cap=TN_BLOCKS):
    """gemm_dispatch.hip tn_rows restated: (blocks, rows per block)."""
    chunks = -(-M // 32)
    per = -(-chunks // cap)
    return -(-chunks // per), per * 32


def tn_plan(M):
    blocks, rows = tn_rows(M)
    last = M - (blocks - 1) * rows
    return blocks, rows, last, -(-rows // 16), -(-last // 16)


for _m in TN_M:  # a changed plan must not silently void the cases
    assert tn_plan(_m) == TN_PLAN[_m], (_m, tn_plan(_m))

TN_FORMS = ("dz_mask", "g_mask", "g", "dz")
TN_GEOM = ((128, 128), (166, 166), (100, 150), (150, 180))
HSCALE = 2.0   # a power of two: the g forms' G = g * hscale is exact


def _tn_cases():
    out = []
    for i, M in enumerate(TN_M):
        for w in range(2):  # ld 256, ld 336; the gapped pairs at every other M
            k1, k2 = TN_GEOM[w + 2 * (i % 2)]
            for f, form in enumerate(TN_FORMS):
                j = 2 * i + w + f
                out.append((M, k1, k2, (128, 72, 8)[j % 3], form, (j // 3 + f) % 2 == 0, ("f32", "bf16")[(i + w + f // 2) % 2]))
    return out


TN_CASES = _tn_cases()  # (M, k1, k2, Nr, form, gout, g / gout dtype)


def tn_id(case):
    M, k1, k2, nr, form, gout, gdt = case
    return f"M{M}-{k1}+{k2}-n{nr}-{form}-{'gout' if gout else 'nogout'}-{gdt}"


@functools.lru_cache(maxsize=2)
def tn_operands(M, k1, k2):
    g = torch.Generator().manual_seed(_seed(M, k1, k2, 3))
    a1 = torch.randn(M, k1, generator=g).to(torch.bfloat16)
    a2 = torch.randn(M, k2, generator=g).to(torch.bfloat16)
    h = torch.relu(torch.randn(M, 128, generator=g)).to(torch.bfloat16)
    dz = torch.randn(M, 4, generator=g) * 1e-3
    proj = torch.randn(4, 128, generator=g)
    gg = torch.randn(M, 128, generator=g) * 1e-3
    return SimpleNamespace(a1=a1, a2=a2, h=h, dz=dz, proj=proj, g=gg, A64=torch.cat([a1, a2], 1).double())


def tn_reference(case):
    """Inputs of one case (Nr-wide contiguous copies) and its float64 construction: G (masked,
    scaled), eps = the f32 formation error of G (0 for the g forms: exact), db, dz^T h, sum dz."""
    M, k1, k2, nr, form, gout, gdt = case
    op = tn_operands(M, k1, k2)
    proj_form, masked = form.startswith("dz"), form.endswith("mask")
    h = op.h[:, :nr].contiguous() if masked else None
    proj = op.proj[:, :nr].contiguous()
    hs = HSCALE if masked else 1.0
    if proj_form:
        g_in = None
        G = op.dz.double() @ proj.double()
        # e = z0 p0, then three fmas, then * hscale (exact): four roundings of partial sums
        eps = 4.01 * U24 * (op.dz.double().abs() @ proj.double().abs()) * hs
    else:
        g_in = op.g[:, :nr].contiguous()
        if gdt == "bf16":
            g_in = g_in.to(torch.bfloat16)
        G = g_in.double()
        eps = torch.zeros_like(G)
    if masked:
        on = h.float() > 0
        G = torch.where(on, G * hs, torch.zeros_like(G))
        eps = torch.where(on, eps, torch.zeros_like(eps))
    r = SimpleNamespace(op=op, M=M, nr=nr, form=form, h=h, proj=proj, g_in=g_in, hs=hs, G=G, eps=eps, db=G.sum(0))
    if proj_form:
        r.dzs = op.dz.double().sum(0)
        r.dw2 = op.dz.double().t() @ h.double() if masked else torch.zeros(4, nr, dtype=torch.float64)
    return r


ROW_TOL = 1e-5


def tn_operand(r, gout=None):
    """(the MFMA's G operand, per-row slack of dW) of a run: RNE_bf16 of the G the kernel wrote
    when it wrote one; else RNE_bf16 of the float64 G, and for the elements whose rounding the f32
    formation error eps can flip, the flip's size times |A| row by row."""
    nr, K = r.nr, r.op.A64.size(1)
    if gout is not None:
        return rne_bf16(gout.double()), torch.zeros(nr, dtype=torch.float64)
    lo, hi = rne_bf16(r.G - r.eps), rne_bf16(r.G + r.eps)
    idx = (lo != hi).nonzero()
    extra = torch.zeros(nr, K, dtype=torch.float64)
    if idx.numel():
        extra.index_add_(0, idx[:, 1], (hi - lo)[idx[:, 0], idx[:, 1]].abs()[:, None] * r.op.A64[idx[:, 0]].abs())
    return rne_bf16(r.G), extra.norm(dim=1)


def row_misses(got, ref, slack=None):
    """Rows n with |got[n] - ref[n]|_2 > ROW_TOL |ref[n]|_2 + slack[n].  The outputs are sums of M
    random-sign terms accumulated in f32 in pieces (16 rows per MFMA, up to 8 chunks per block, up
    to 256 slabs): a rounding error of order sqrt(depth) 2^-24 of a row's norm, about 1e-6; the
    files' whole-tensor figure, 1e-5, asked of every row."""
    d = (got.double() - ref).norm(dim=1)
    tol = ROW_TOL * ref.norm(dim=1) + (slack if slack is not None else 0.0)
    return (~(d <= tol)).nonzero().flatten().tolist()


def compute_shares(cus=HOST_CUS):
    """{case id: {"n": elements, "cpu": misrounded elements of the CPU float32 evaluation}}: the
    table golden/make_bf16_image_shares.py writes and test_bf16_image_host regenerates."""
    out = {}
    for case in NT_CASES:
        r = nt_reference(case, cus)
        out[nt_id(case)] = {"n": r.ref.numel(), "cpu": nt_check(r, r.cpu).misrounded}
    return out
