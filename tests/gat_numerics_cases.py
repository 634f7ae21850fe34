"""Cases, inputs, the float64 / float32 oracle pair and the error metrics of the GAT numerics tests
(test_gpu_gat_numerics on the device, test_gat_numerics_host for the conditions the inputs must
meet).  Plain helper module: no test lives here.

The op under test is the attention after ``lin`` (lin = identity in the oracle, as in
test_gpu_dispatch_model.test_gat_attention_xh_alignment).  Every quantity of a run is compared with
``oracle.pyg_ref.gat_conv`` on the same float32 inputs cast to float64; the same oracle run in
float32 gives e_32, the error a plain f32 evaluation makes, which scales the bound.
"""
import functools
import math
from types import SimpleNamespace

import torch

from oracle import pyg_ref
from oracle.dropout_hash import keep_mask
from test_gpu_parity import GRAPHS, _split_graph, rand_graph

GRAPH_NAMES = ("small", "hub", "split")
HUB_ROW = {"hub": 7, "split": 5}       # the 3,000- and the 1,000-slot row
WINDOW = 512                           # twice the narrow kernel's staging window (gat.hip CAP = 256):
                                       # past any window alignment, and past every lane-group phase

# (C, H, concat) -> the kernel family gat.hip's dispatch picks for aligned, contiguous operands
SHAPES = {
    (8, 4, True): "group",      # lane-group v4
    (64, 4, True): "group",     # lane-group v4, FL = 64: the last fast width
    (6, 2, True): "group",      # lane-group v2, FL = 6 padded to 8
    (5, 8, True): "group",      # lane-group v1, FL = 40
    (4, 2, False): "group",     # lane-group head mean
    (3, 2, False): "generic",   # L = 3 is not a power of two
    (130, 1, True): "generic",  # F / v = 65 > 64
    (2, 1, False): "narrow",    # the narrow output kernel (lane-group with _GAT_NARROW off)
    (1, 1, False): "narrow",
}
GEOM = {(8, 4, True): (4, 8), (64, 4, True): (4, 64), (6, 2, True): (2, 6), (5, 8, True): (1, 40),
        (4, 2, False): (4, 2), (2, 1, False): (2, 1), (1, 1, False): (1, 1)}  # lane-group (v, FL)
# every shape, the narrow ones a second time in their lane-group form
RUNS = [(s, True) for s in SHAPES] + [(s, False) for s, f in SHAPES.items() if f == "narrow"]
SLOPES = (0.0, 0.5, 1.0, -0.5)
RANGE_SCALES = (8, 32)
RANGE_SLOPES = (0.2, 0.0, -0.5)
KINK_SHAPES = ((8, 4, True), (3, 2, False), (2, 1, False))
KINK_SLOPES = (0.0, 0.5, -0.5)
MIN_SPREAD = 40.0   # exp(-40) = 4e-18: far below float32's resolution of a row sum
KINK_SHARE = 0.10
DROP_P, DROP_SEED = 0.5, 0x1234_5678_9ABC
# slope 0.5 through the other three backward entry points: (graph, shape, form)
EPILOGUE_CASES = [(g, s, f) for g in ("small", "hub") for s, f in (
    ((8, 4, True), "post"), ((130, 1, True), "post"),         # gnn_gat_bwd_act_f32: lane-group, generic
    ((8, 4, True), "proj"),                                    # gnn_gat_bwd_act_proj_f32
    ((8, 4, True), "explain"), ((4, 2, False), "explain"))]    # gnn_gat_bwd_ew_f32

QUANTITIES = ("out", "alpha", "dxh", "datt_src", "datt_dst", "dbias", "dew")
FLOOR = {q: 1e-5 for q in QUANTITIES}
FLOOR["alpha"] = 2.0 ** -20  # 16 ulp of 1.0


def gat_family(C, H, concat, narrow=True, post=False, edge_w=False):
    """gat.hip's choice restated (gat_geom, gnn_gat_fwd_fused_f32, _GATAttention.forward) for
    contiguous 16-byte aligned operands: (family, v, FL)."""
    if H == 1 and C <= 2 and not concat and narrow and not post and not edge_w:
        return "narrow", None, None
    v = next(v for v in (4, 2, 1) if C % v == 0)
    FL, L = H * C // v, C // v
    if edge_w or FL > 64 or (not concat and L & (L - 1)):
        return "generic", v, FL
    return "group", v, FL


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "split":
        return _split_graph()
    return rand_graph(**GRAPHS[name]), GRAPHS[name]["n"]


def _seed(*parts):
    return int(sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts))) % (2 ** 31)


def _finish(gname, C, H, concat, g, xh, att_src, att_dst):
    ei, n = graph(gname)
    Fo = H * C if concat else C
    return SimpleNamespace(gname=gname, C=C, H=H, concat=concat, xh=xh, att_src=att_src, att_dst=att_dst,
                           bias=torch.randn(Fo, generator=g), dy=torch.randn(n, Fo, generator=g),
                           edge_w=torch.rand(ei.size(1), generator=g),
                           w_out=torch.randn(2, H * C, generator=g) * 0.1, dz=torch.randn(n, 2, generator=g))


def _draw(gname, C, H, concat, scale, salt):
    _, n = graph(gname)
    g = torch.Generator().manual_seed(_seed(GRAPH_NAMES.index(gname), C, H, concat, scale, salt))
    xh = torch.randn(n, H * C, generator=g)
    att_src = torch.randn(1, H, C, generator=g) * (scale / math.sqrt(C))
    att_dst = torch.randn(1, H, C, generator=g) * (scale / math.sqrt(C))
    return _finish(gname, C, H, concat, g, xh, att_src, att_dst)


@functools.lru_cache(maxsize=None)
def randn_inputs(gname, C, H, concat, scale=1):
    """xh ~ randn, att ~ randn * scale / sqrt(C) (scores of standard deviation ~ scale * sqrt(2)).
    At scale > 1, on the graphs with a hub, the draw is the first that does what the score-range
    test is for, under every slope of RANGE_SLOPES: some row's scores span more than MIN_SPREAD and
    the hub row's running maximum still grows past WINDOW slots (score_stats: properties of the
    inputs alone, read from float64 scores)."""
    for salt in range(64):
        inp = _draw(gname, C, H, concat, scale, salt)
        if scale == 1 or gname not in HUB_ROW:
            return inp
        st = [score_stats(inp, s) for s in RANGE_SLOPES]
        if all(t.hub_late_max and t.spread > MIN_SPREAD for t in st):
            return inp
    raise AssertionError("no draw with a wide row and a late hub maximum")


@functools.lru_cache(maxsize=None)
def kink_inputs(gname, C, H, concat):
    """Integer inputs: xh in {-2..2}, att in {-1, 0, 1} with at most two nonzero channels per head
    and vector, so every a_src[j] + a_dst[i] is a small exact integer and z == 0 is common.  The
    first draw with at least KINK_SHARE of the slots at z == 0 and a tenth on either side (one hub
    row of one head can otherwise put most slots on one side)."""
    _, n = graph(gname)
    for salt in range(64):
        g = torch.Generator().manual_seed(_seed(GRAPH_NAMES.index(gname), C, H, concat, 991, salt))
        xh = torch.randint(-2, 3, (n, H * C), generator=g).float()
        att = []
        for _ in range(2):
            a = torch.zeros(H, C)
            for h in range(H):
                ch = torch.randperm(C, generator=g)[:2]
                a[h, ch] = (torch.randint(0, 2, (ch.numel(),), generator=g) * 2 - 1).float()
            att.append(a.view(1, H, C))
        inp = _finish(gname, C, H, concat, g, xh, att[0], att[1])
        st = score_stats(inp, 0.5)
        if st.zero >= KINK_SHARE and min(st.pos, st.neg) >= 0.1:
            return inp
    raise AssertionError("no draw on the kink")


def replaced_edges(gname):
    """The oracle's edge list: non-loop input edges in input order, then one loop per node."""
    ei, n = graph(gname)
    return pyg_ref.add_self_loops(pyg_ref.remove_self_loops(ei), n)


def score_stats(inp, slope):
    """From the float64 scores of ``inp`` alone: the share of slots with z == 0 and of z > 0 / z < 0,
    the largest max - min of the score z = a_src[j] + a_dst[i] over a (row, head) (and, espread, of
    the softmax argument e = leaky(z)), and whether the hub row's running maximum of e still grows
    after its first WINDOW slots (for some head)."""
    _, n = graph(inp.gname)
    e2 = replaced_edges(inp.gname)
    xh = inp.xh.double().view(n, inp.H, inp.C)
    z = (xh * inp.att_src.double()).sum(-1)[e2[0]] + (xh * inp.att_dst.double()).sum(-1)[e2[1]]
    e = torch.nn.functional.leaky_relu(z, slope)
    idx = e2[1].view(-1, 1).expand_as(e)

    def spread(t):
        hi = torch.full((n, inp.H), -math.inf, dtype=torch.float64).scatter_reduce_(0, idx, t, "amax")
        lo = torch.full((n, inp.H), math.inf, dtype=torch.float64).scatter_reduce_(0, idx, t, "amin")
        return float((hi - lo).max())

    late = False
    if inp.gname in HUB_ROW:
        eh = e[e2[1] == HUB_ROW[inp.gname]]  # CSR slot order: stable in the edge list
        late = bool((eh[WINDOW:].max(0).values > eh[:WINDOW].max(0).values).any())
    return SimpleNamespace(zero=float((z == 0).double().mean()), pos=float((z > 0).double().mean()),
                           neg=float((z < 0).double().mean()), spread=spread(z), espread=spread(e), hub_late_max=late)


def reference(inp, slope, dtype, form="conv"):
    """The oracle on ``inp`` in ``dtype``, forward and autograd with the fixed dy.  form: "conv";
    "post" (dropout(elu(.)) under the counter-hash mask); "proj" (post, then · w_outᵀ, dy = dz);
    "explain" (messages scaled by edge_w)."""
    ei, n = graph(inp.gname)
    H, C, concat = inp.H, inp.C, inp.concat
    F = H * C
    xh, a_s, a_d, b = (t.detach().to(dtype, copy=True).requires_grad_(True)
                       for t in (inp.xh, inp.att_src, inp.att_dst, inp.bias))
    eye = torch.eye(F, dtype=dtype)
    ew = None
    with torch.no_grad():
        _, alpha, _ = pyg_ref.gat_conv(xh, ei, eye, a_s, a_d, b, H, C, concat=concat, negative_slope=slope,
                                       return_alpha=True)
    if form == "explain":
        ew = inp.edge_w.detach().to(dtype, copy=True).requires_grad_(True)
        out = pyg_ref.gat_conv_explain(xh, ei, ew, eye, a_s, a_d, b, H, C, concat=concat, negative_slope=slope,
                                       apply_sigmoid=False)
    else:
        out = pyg_ref.gat_conv(xh, ei, eye, a_s, a_d, b, H, C, concat=concat, negative_slope=slope)
    dy = inp.dy
    if form in ("post", "proj"):
        keep = torch.from_numpy(keep_mask(DROP_SEED, n, out.size(1), DROP_P)).to(dtype)
        out = torch.nn.functional.elu(out) * (keep / (1.0 - DROP_P))
    if form == "proj":
        out = out @ inp.w_out.to(dtype).t()
        dy = inp.dz
    out.backward(dy.to(dtype))
    res = dict(out=out.detach(), alpha=alpha, dxh=xh.grad, datt_src=a_s.grad, datt_dst=a_d.grad, dbias=b.grad)
    if ew is not None:
        res["dew"] = ew.grad
    return res


@functools.lru_cache(maxsize=None)
def _oracle_pair(kind, gname, C, H, concat, scale, slope, form):
    inp = kink_inputs(gname, C, H, concat) if kind == "kink" else randn_inputs(gname, C, H, concat, scale)
    r64 = reference(inp, slope, torch.float64, form)
    r32 = reference(inp, slope, torch.float32, form)
    return inp, r64, errors(r32, r64)


def oracle_pair(kind, gname, shape, scale, slope, form="conv"):
    """(inputs, float64 results, e_32) of one case; computed once and shared, never modified."""
    return _oracle_pair(kind, gname, *shape, scale, slope, form)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def errors(got, r64):
    """Error of every quantity of ``got`` against the float64 results: relative L2 for out, d xh,
    d bias and d edge_w; max |diff| for alpha; for d att_src and d att_dst the L2 error over the
    larger of the two float64 norms (d att_dst is zero at slope 1 and cancellation-dominated
    elsewhere).  Every element takes part."""
    e = {q: _rel(got[q].reshape(r64[q].shape), r64[q]) for q in ("out", "dxh", "dbias", "dew") if q in r64}
    e["alpha"] = float((got["alpha"].detach().double().cpu() - r64["alpha"]).abs().max())
    scale = max(float(r64["datt_src"].norm()), float(r64["datt_dst"].norm()), 1e-300)
    for q in ("datt_src", "datt_dst"):
        e[q] = float((got[q].detach().double().cpu().reshape(r64[q].shape) - r64[q]).norm()) / scale
    return e
