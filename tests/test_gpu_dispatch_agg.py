"""gnn_aggregate_f32 / gnn_aggregate_bf16 at every vector width and lane geometry their
dispatchers pick, reached by width, by pointer alignment and by row pitch.

The dispatcher (aggregate.hip, gnn_aggregate_f32 -> launch_mode / launch_mode_split) reads
  vec    = the widest of 4 / 2 / 1 with F, every pitch (x, y, addend, addend2) and, for EDGE_W, the
           per-head width divisible by it and every pointer 4*vec-byte aligned (ok_vec);
  nchunk = F / vec, and from it the form:
             F <= 4 SUM / MEAN / MEAN_BWD, F <= 2 GCN     agg_narrow_lds_kernel<2|4>
             F <= 8 otherwise                               agg_group_kernel<2|4|8>
             nchunk <= 8 / 16 / 32                          agg_flat_kernel<V, 8|16|32, 1>
             nchunk 33..128                                 agg_wave_kernel<V, 2>
             nchunk 129..256                                agg_flat_kernel<V, 64, 4>
             nchunk > 256                                   refused (GNN_ERR_UNSUPPORTED)
  and, on a plan with long segments (8 < F <= 128, F / vec <= 32, not EDGE_W), the split:
             main pass agg_flat_kernel<V, 8|32, 1> over the truncated segments in degree order,
             agg_piece_wide_kernel<V, 1> and agg_combine_kernel<V, 1>; 16-lane groups take the
             pieces into the main pass's launch (agg_flat_pieces_kernel<V, 16, 1>) + the combine.
agg_flat_kernel<*, 1, 8, 1> is not instantiated (F > 8 at vec 1 is nchunk >= 9), nor are the split's
NCH = 2 / 4 piece and combine forms (the split runs only for nchunk <= 32).

KERNEL and CASES below are that reading written out: the kernels each (F, vec) must select, unsplit
and split, and one row per (F, operand layout) with the vec that layout gives.  ``expected`` restates the dispatcher and the test
asserts that the table, the restatement and the operands' real pointers and pitches agree, so a
case cannot silently drift to another instantiation; profiles/dispatch_lattice_kernels.txt records
the kernels a traced run of this file launched.

Bit equality between layouts of one (graph, F, mode), decided from the code: aggregate.hip builds
without FMA contraction; agg_flat_kernel, agg_wave_kernel and the piece kernels all start a
column's accumulator at 0 and add the row's slots one at a time in slot order (the U rows in
flight are loaded together but added in order), whatever VEC or lane holds the column, and their
epilogues apply / deg, + addend, + addend2, + bias, ReLU, dropout in the same order on the same
element index.  So every unsplit wide form is bit-equal to every other ("seq"), and every split
form to every other ("split": main-pass partial, pieces in slot order, combine in piece order,
independent of VEC).  Split and unsplit associate differently: f64 bound only.  The narrow and
group kernels (F <= 8) never read vec: all layouts run one instantiation.
"""
import functools

import pytest
import torch

from dispatch_operands import Carved, align_bytes, ld_of
from test_gpu_parity import ATOL, GRAPHS, RTOL, _split_graph, rand_graph

pytestmark = pytest.mark.gpu

A0 = ("flat", 0)
# operand layouts by name: x, y, add, add2 (see dispatch_operands.Carved)
VARIANTS = {
    "aligned": dict(),
    "x+2": dict(x=("flat", 2)),                 # by pointer: x 8-byte aligned
    "x+1": dict(x=("flat", 1)),                 # by pointer: x 4-byte aligned
    "x+3": dict(x=("flat", 3)),
    "y+2": dict(y=("flat", 2)),
    "y+1": dict(y=("flat", 1)),
    "add+2": dict(add=("flat", 2)),
    "add+1": dict(add=("flat", 1)),
    "add2+2": dict(add2=("flat", 2)),
    "add2+1": dict(add2=("flat", 1)),
    "xpitch+2": dict(x=("pad", 0, 2)),          # by pitch: every pointer 16-byte aligned
    "xpitch+1": dict(x=("pad", 0, 1)),
    "ypitch+2": dict(y=("pad", 0, 2)),
    "ypitch+1": dict(y=("pad", 0, 1)),
    "addpitch+2": dict(add=("pad", 0, 2)),
    "add2pitch+1": dict(add2=("pad", 0, 1)),
    # padded pitches and column offsets that keep 16 bytes: the widest vec over pitch != F
    "pad4": dict(x=("pad", 4, 8), y=("pad", 4, 8), add=("pad", 0, 4), add2=("pad", 8, 12)),
    "pad2": dict(x=("pad", 2, 4), y=("pad", 4, 8), add=("pad", 0, 4), add2=("pad", 8, 12)),
    "pad1": dict(x=("pad", 4, 8), y=("pad", 3, 5), add=("pad", 0, 4), add2=("pad", 8, 12)),
}


def layouts(variant):
    return {k: VARIANTS[variant].get(k, A0) for k in ("x", "y", "add", "add2")}


def vec_of(F, lay, use, chan=None):
    """ok_vec: the operands in ``use`` (names of x / y / add / add2 actually passed)."""
    for v in (4, 2):
        if F % v or (chan is not None and chan % v):
            continue
        if all(ld_of(lay[k], F) % v == 0 and align_bytes(lay[k]) >= 4 * v for k in use):
            return v
    return 1


def expected(mode, F, vec, split):
    """launch_mode / launch_mode_split restated: the kernels one call launches."""
    if F <= 8:
        if (F <= 4 and mode in ("sum", "mean", "mean_bwd")) or (F <= 2 and mode == "gcn"):
            return f"narrow<{2 if F <= 2 else 4}>"
        return f"group<{2 if F <= 2 else 4 if F <= 4 else 8}>"
    nchunk = F // vec
    if nchunk > 256:
        return "refused"
    lps = 8 if nchunk <= 8 else 16 if nchunk <= 16 else 32 if nchunk <= 32 else 64
    if split and mode != "edge_w" and F <= 128 and nchunk <= 32:
        if lps == 16:
            return f"split: flat_pieces<{vec},16,1> + combine<{vec},1>"
        return f"split: flat<{vec},{lps},1> + piece_wide<{vec},1> + combine<{vec},1>"
    if lps == 64 and nchunk <= 128:
        return f"wave<{vec},2>"
    return f"flat<{vec},{lps},{4 if lps == 64 else 1}>"


# Which operands each mode of the test passes (they all feed ok_vec), and its epilogue:
#   sum       no addend, no bias                    (null addends must not lower vec)
#   mean      + addend + addend2 + bias
#   mean_bwd  + addend                              (transposed: CSC, the backward's direction)
#   gcn       + addend + bias, ReLU, dropout 0.25
USE = {"sum": ("x", "y"), "mean": ("x", "y", "add", "add2"), "mean_bwd": ("x", "y", "add"),
       "gcn": ("x", "y", "add"), "edge_w": ("x", "y", "add")}
MODES = ("sum", "mean", "mean_bwd", "gcn")
DROP_P, DROP_SEED = 0.25, 0x5EED1234

# The lattice for F > 8, read off launch_mode / launch_mode_split: (F, vec) -> (kernel of an unsplit
# call, kernels of a call over a direction with long segments; None: the split does not apply, the
# unsplit kernel runs).  F <= 8 is NARROW below.  Generated once from ``expected`` and committed;
# test_table_is_the_dispatcher keeps the two in step.
KERNEL = {
    (9, 1): ('flat<1,16,1>', 'split: flat_pieces<1,16,1> + combine<1,1>'),
    (10, 2): ('flat<2,8,1>', 'split: flat<2,8,1> + piece_wide<2,1> + combine<2,1>'),
    (12, 4): ('flat<4,8,1>', 'split: flat<4,8,1> + piece_wide<4,1> + combine<4,1>'),
    (16, 1): ('flat<1,16,1>', 'split: flat_pieces<1,16,1> + combine<1,1>'),
    (16, 2): ('flat<2,8,1>', 'split: flat<2,8,1> + piece_wide<2,1> + combine<2,1>'),
    (16, 4): ('flat<4,8,1>', 'split: flat<4,8,1> + piece_wide<4,1> + combine<4,1>'),
    (17, 1): ('flat<1,32,1>', 'split: flat<1,32,1> + piece_wide<1,1> + combine<1,1>'),
    (18, 2): ('flat<2,16,1>', 'split: flat_pieces<2,16,1> + combine<2,1>'),
    (20, 4): ('flat<4,8,1>', 'split: flat<4,8,1> + piece_wide<4,1> + combine<4,1>'),
    (32, 1): ('flat<1,32,1>', 'split: flat<1,32,1> + piece_wide<1,1> + combine<1,1>'),
    (32, 2): ('flat<2,16,1>', 'split: flat_pieces<2,16,1> + combine<2,1>'),
    (32, 4): ('flat<4,8,1>', 'split: flat<4,8,1> + piece_wide<4,1> + combine<4,1>'),
    (33, 1): ('wave<1,2>', None),
    (34, 2): ('flat<2,32,1>', 'split: flat<2,32,1> + piece_wide<2,1> + combine<2,1>'),
    (36, 4): ('flat<4,16,1>', 'split: flat_pieces<4,16,1> + combine<4,1>'),
    (64, 1): ('wave<1,2>', None),
    (64, 2): ('flat<2,32,1>', 'split: flat<2,32,1> + piece_wide<2,1> + combine<2,1>'),
    (64, 4): ('flat<4,16,1>', 'split: flat_pieces<4,16,1> + combine<4,1>'),
    (68, 4): ('flat<4,32,1>', 'split: flat<4,32,1> + piece_wide<4,1> + combine<4,1>'),
    (127, 1): ('wave<1,2>', None),
    (128, 1): ('wave<1,2>', None),
    (128, 2): ('wave<2,2>', None),
    (128, 4): ('flat<4,32,1>', 'split: flat<4,32,1> + piece_wide<4,1> + combine<4,1>'),
    (131, 1): ('flat<1,64,4>', None),
    (132, 4): ('wave<4,2>', None),
    (166, 1): ('flat<1,64,4>', None),
    (166, 2): ('wave<2,2>', None),
    (256, 1): ('flat<1,64,4>', None),
    (256, 2): ('wave<2,2>', None),
    (256, 4): ('wave<4,2>', None),
    (257, 1): ('refused', None),
    (258, 2): ('flat<2,64,4>', None),
    (512, 1): ('refused', None),
    (512, 2): ('flat<2,64,4>', None),
    (512, 4): ('wave<4,2>', None),
    (516, 4): ('flat<4,64,4>', None),
    (1024, 2): ('refused', None),
    (1024, 4): ('flat<4,64,4>', None),
    (1028, 4): ('refused', None),
}

# F <= 8 never reads vec: (F, mode) -> kernel, every layout.
NARROW = {(F, m): expected(m, F, 1, False) for F in range(1, 9) for m in MODES + ("edge_w",)}
assert NARROW[(2, "gcn")] == "narrow<2>" and NARROW[(3, "gcn")] == "group<4>" and NARROW[(4, "mean")] == "narrow<4>"
assert NARROW[(2, "edge_w")] == "group<2>" and NARROW[(4, "edge_w")] == "group<4>" and NARROW[(5, "sum")] == "group<8>"

# (F, layout, vec): vec as ok_vec gives it for that layout; a triple where the addends' layout
# matters: (sum: x, y only | mean: + addend + addend2 | mean_bwd, gcn: + addend).
CASES = [
    (1, 'aligned', 1),
    (1, 'x+1', 1),
    (1, 'pad1', 1),
    (2, 'aligned', 2),
    (2, 'x+1', 1),
    (2, 'pad1', 1),
    (3, 'aligned', 1),
    (3, 'x+1', 1),
    (3, 'pad1', 1),
    (4, 'aligned', 4),
    (4, 'x+1', 1),
    (4, 'pad1', 1),
    (5, 'aligned', 1),
    (5, 'x+1', 1),
    (5, 'pad1', 1),
    (7, 'aligned', 1),
    (7, 'x+1', 1),
    (7, 'pad1', 1),
    (8, 'aligned', 4),
    (8, 'x+1', 1),
    (8, 'pad1', 1),
    (9, 'aligned', 1),
    (9, 'pad4', 1),
    (10, 'aligned', 2),
    (10, 'pad4', 2),
    (12, 'aligned', 4),
    (12, 'pad4', 4),
    (16, 'aligned', 4),
    (16, 'x+2', 2),
    (16, 'x+1', 1),
    (16, 'xpitch+2', 2),
    (16, 'xpitch+1', 1),
    (16, 'pad4', 4),
    (16, 'pad2', 2),
    (16, 'pad1', 1),
    (17, 'aligned', 1),
    (17, 'pad4', 1),
    (18, 'aligned', 2),
    (18, 'pad4', 2),
    (20, 'aligned', 4),
    (20, 'pad4', 4),
    (32, 'aligned', 4),
    (32, 'x+2', 2),
    (32, 'x+1', 1),
    (32, 'xpitch+2', 2),
    (32, 'xpitch+1', 1),
    (32, 'pad4', 4),
    (32, 'pad2', 2),
    (32, 'pad1', 1),
    (33, 'aligned', 1),
    (33, 'pad4', 1),
    (34, 'aligned', 2),
    (34, 'pad4', 2),
    (36, 'aligned', 4),
    (36, 'pad4', 4),
    (64, 'aligned', 4),
    (64, 'x+2', 2),
    (64, 'x+1', 1),
    (64, 'xpitch+2', 2),
    (64, 'xpitch+1', 1),
    (64, 'pad4', 4),
    (64, 'pad2', 2),
    (64, 'pad1', 1),
    (64, 'x+3', 1),
    (64, 'y+2', 2),
    (64, 'y+1', 1),
    (64, 'add+2', (4, 2, 2)),
    (64, 'add+1', (4, 1, 1)),
    (64, 'add2+2', (4, 2, 4)),
    (64, 'add2+1', (4, 1, 4)),
    (64, 'ypitch+2', 2),
    (64, 'ypitch+1', 1),
    (64, 'addpitch+2', (4, 2, 2)),
    (64, 'add2pitch+1', (4, 1, 4)),
    (68, 'aligned', 4),
    (68, 'pad4', 4),
    (127, 'aligned', 1),
    (127, 'pad4', 1),
    (128, 'aligned', 4),
    (128, 'x+2', 2),
    (128, 'x+1', 1),
    (128, 'xpitch+2', 2),
    (128, 'xpitch+1', 1),
    (128, 'pad4', 4),
    (128, 'pad2', 2),
    (128, 'pad1', 1),
    (131, 'aligned', 1),
    (131, 'pad4', 1),
    (132, 'aligned', 4),
    (132, 'pad4', 4),
    (166, 'aligned', 2),
    (166, 'x+2', 2),
    (166, 'x+1', 1),
    (166, 'xpitch+2', 2),
    (166, 'xpitch+1', 1),
    (166, 'pad4', 2),
    (166, 'pad2', 2),
    (166, 'pad1', 1),
    (256, 'aligned', 4),
    (256, 'x+2', 2),
    (256, 'x+1', 1),
    (256, 'xpitch+2', 2),
    (256, 'xpitch+1', 1),
    (256, 'pad4', 4),
    (256, 'pad2', 2),
    (256, 'pad1', 1),
    (256, 'x+3', 1),
    (256, 'y+2', 2),
    (256, 'y+1', 1),
    (256, 'add+2', (4, 2, 2)),
    (256, 'add+1', (4, 1, 1)),
    (256, 'add2+2', (4, 2, 4)),
    (256, 'add2+1', (4, 1, 4)),
    (256, 'ypitch+2', 2),
    (256, 'ypitch+1', 1),
    (256, 'addpitch+2', (4, 2, 2)),
    (256, 'add2pitch+1', (4, 1, 4)),
    (257, 'aligned', 1),
    (258, 'aligned', 2),
    (258, 'pad4', 2),
    (512, 'aligned', 4),
    (512, 'x+2', 2),
    (512, 'x+1', 1),
    (512, 'xpitch+2', 2),
    (512, 'xpitch+1', 1),
    (512, 'pad4', 4),
    (512, 'pad2', 2),
    (512, 'pad1', 1),
    (516, 'aligned', 4),
    (516, 'pad4', 4),
    (1024, 'aligned', 4),
    (1024, 'pad4', 4),
    (1024, 'xpitch+2', 2),
    (1028, 'aligned', 4),
]


# Where each row runs.  "small" (37 nodes, no long segment: unsplit), "hub" (300 nodes, one CSR row
# of 3000 slots: split forward, unsplit transpose) and "split" (_split_graph: long segments both
# ways, rows of 32 / 33 / 64 / 65 slots).  N is 37 / 300 / 600: no multiple of 16 rows per wave
# (300, 600), nor of the 7 / 2 / 8 rows per lane group (37).  "one" is a single node with two
# self loops, "alone" 19 nodes without an edge.
_SPLIT_F = (9, 10, 12, 16, 17, 18, 20, 32, 34, 36, 64, 68, 128)
_SPLIT_V = ("aligned", "x+2", "x+1", "xpitch+2", "pad4", "y+1", "add+2")


def _graphs_of(F, variant):
    gs = ["small"]
    if (F in _SPLIT_F and variant in _SPLIT_V) or (F in (3, 5, 166, 256) and variant == "aligned"):
        gs += ["hub", "split"]
    if (F, variant) in ((3, "x+1"), (7, "pad1"), (16, "x+2"), (64, "x+1"), (64, "pad4"), (166, "aligned"),
                        (166, "x+1"), (256, "aligned")):
        gs += ["one", "alone"]
    return gs


# one test per (graph, F): its layouts run inside it, so the bit-equality check between them is
# self-contained whichever cases are selected
GROUPS = {}
for _F, _variant, _vecs in CASES:
    for _g in _graphs_of(_F, _variant):
        GROUPS.setdefault((_g, _F), []).append((_variant, _vecs))


@functools.lru_cache(maxsize=None)
def _edges(graph):
    if graph == "split":
        return _split_graph()
    if graph == "one":
        return torch.zeros((2, 2), dtype=torch.long), 1
    if graph == "alone":
        return torch.zeros((2, 0), dtype=torch.long), 19
    return rand_graph(**GRAPHS[graph]), GRAPHS[graph]["n"]


_PLANS = {}


def _plan(device, graph, replace):
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.graph import GraphPlan

    key = (graph, replace)
    if key not in _PLANS:
        ei, n = _edges(graph)
        _PLANS[key] = GraphPlan(ei.to(device), n, _lib.LOOPS_REPLACE if replace else _lib.LOOPS_KEEP)
    return _PLANS[key]


def _grid(t, bits):
    """t rounded to multiples of 2^-bits.  The bound of this file is 1e-5 against float64, and the
    hub rows sum 1000 to 3000 slots: an f32 sum of that many unit-variance terms is itself off by
    more than 1e-5 in whatever order (n * 2^-24 * sum |x_i| at worst, 3e-5 seen), which would
    measure f32 addition and not the kernel.  With x on a 2^-6 grid (and EDGE_W's weights on a
    2^-3 grid) every partial sum of SUM, MEAN and EDGE_W is exact in f32 (|partial| < 2^15 needs
    15 + 9 bits), so those modes are held to the bound by the kernel's indexing alone; MEAN_BWD
    and GCN round each slot's term (x / deg, w * x) and keep their order-dependent rounding."""
    return (t * 2.0 ** bits).round() / 2.0 ** bits


@functools.lru_cache(maxsize=None)
def _inputs(graph, F):
    n = _edges(graph)[1]
    g = torch.Generator().manual_seed(1000 + F)
    x, add, add2 = (torch.randn(n, F, generator=g, dtype=torch.float64).float() for _ in range(3))
    return (_grid(x, 6), add, add2, torch.randn(F, generator=g, dtype=torch.float64).float())


@functools.lru_cache(maxsize=None)
def _reference(graph, F, mode):
    """float64 scatter of the operation over the f32 inputs, with the mode's epilogue (USE)."""
    from oracle.dropout_hash import keep_mask

    ei, n = _edges(graph)
    x, add, add2, bias = (t.double() for t in _inputs(graph, F))
    s, d = ei[0], ei[1]
    if mode == "gcn":
        keep = s != d
        s = torch.cat([s[keep], torch.arange(n)])
        d = torch.cat([d[keep], torch.arange(n)])
    deg = torch.bincount(d, minlength=n).double()
    z = torch.zeros(n, F, dtype=torch.float64)
    if mode == "sum":
        return z.index_add_(0, d, x[s])
    if mode == "mean":
        return z.index_add_(0, d, x[s]) / deg.clamp(min=1)[:, None] + add + add2 + bias
    if mode == "mean_bwd":
        return z.index_add_(0, s, x[d] / deg.clamp(min=1)[d][:, None]) + add
    dinv = deg.pow(-0.5)
    ref = torch.relu(z.index_add_(0, d, x[s] * (dinv[s] * dinv[d])[:, None]) + add + bias)
    return ref * torch.from_numpy(keep_mask(DROP_SEED, n, F, DROP_P)).double() / (1.0 - DROP_P)


def _call(device, graph, F, lay, mode):
    """One aggregate call of ``mode`` with its operands carved as ``lay``; returns the operands."""
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.aggregation import aggregate

    plan = _plan(device, graph, mode == "gcn")
    n = plan.num_nodes
    x, add, add2, bias = _inputs(graph, F)
    ops = {"x": Carved(n, F, lay["x"], device, data=x), "y": Carved(n, F, lay["y"], device)}
    if "add" in USE[mode]:
        ops["add"] = Carved(n, F, lay["add"], device, data=add)
    if "add2" in USE[mode]:
        ops["add2"] = Carved(n, F, lay["add2"], device, data=add2)
    b = bias.to(device)
    kw = dict(out=ops["y"].view)
    if mode == "sum":
        m = _lib.AGG_SUM
    elif mode == "mean":
        m = _lib.AGG_MEAN
        kw.update(nodew=plan.deg, addend=ops["add"].view, addend2=ops["add2"].view, bias=b)
    elif mode == "mean_bwd":
        m = _lib.AGG_MEAN_BWD
        kw.update(nodew=plan.deg, transpose=True, addend=ops["add"].view)
    else:
        m = _lib.AGG_GCN
        kw.update(nodew=plan.dinv, addend=ops["add"].view, bias=b, relu=True, dropout_p=DROP_P, seed=DROP_SEED)
    for k, o in ops.items():  # what reaches the C entry point is the carved operand itself
        assert o.view.stride(1) == 1 and (o.view.stride(0) == o.ld or n <= 1), k
    return ops, (lambda: aggregate(plan, ops["x"].view, m, **kw))


_VEC_SLOT = {"sum": 0, "mean": 1, "mean_bwd": 2, "gcn": 2}  # CASES' triple: (x, y | + add + add2 | + add)


def _vec_for(vecs, mode):
    return vecs if isinstance(vecs, int) else vecs[_VEC_SLOT[mode]]


def _kernel_for(device, graph, F, vec, mode):
    if F <= 8:
        return NARROW[(F, mode)]
    unsplit, split = KERNEL[(F, vec)]
    long_rows = _plan(device, graph, mode == "gcn").split_pieces(mode == "mean_bwd") > 0
    return split if (long_rows and split is not None) else unsplit


def test_table_is_the_dispatcher():
    """CASES / KERNEL agree with the dispatcher's restatement (``vec_of``, ``expected``), and between
    them name every reachable form at every vec."""
    for F, variant, vecs in CASES:
        lay = layouts(variant)
        for mode in MODES:
            vec = _vec_for(vecs, mode)
            assert vec == vec_of(F, lay, USE[mode]), (F, variant, mode)
            if F > 8:
                assert KERNEL[(F, vec)][0] == expected(mode, F, vec, False)
                sp = expected(mode, F, vec, True)
                assert KERNEL[(F, vec)][1] == (sp if sp != KERNEL[(F, vec)][0] else None)
    named = {k for pair in KERNEL.values() for k in pair if k} | set(NARROW.values())
    want = {"narrow<2>", "narrow<4>", "group<2>", "group<4>", "group<8>", "refused"}
    for v in (1, 2, 4):
        want |= {f"flat<{v},{l},1>" for l in (8, 16, 32) if (v, l) != (1, 8)}
        want |= {f"wave<{v},2>", f"flat<{v},64,4>", f"split: flat_pieces<{v},16,1> + combine<{v},1>"}
        want |= {f"split: flat<{v},{l},1> + piece_wide<{v},1> + combine<{v},1>" for l in (8, 32) if (v, l) != (1, 8)}
    assert want <= named, want - named
    # each vec by width, by pointer and by pitch
    by = {(vecs if isinstance(vecs, int) else vecs[1], variant) for F, variant, vecs in CASES if F > 8}
    for need in ((4, "aligned"), (2, "aligned"), (1, "aligned"), (2, "x+2"), (1, "x+1"), (2, "xpitch+2"),
                 (1, "xpitch+1"), (4, "pad4")):
        assert need in by, need


def test_graphs_are_what_the_table_assumes(device):
    assert _plan(device, "small", False).split_pieces(False) == 0 and _plan(device, "small", False).split_pieces(True) == 0
    assert _plan(device, "small", True).split_pieces(False) == 0
    for replace in (False, True):
        assert _plan(device, "hub", replace).split_pieces(False) > 0
        assert _plan(device, "split", replace).split_pieces(False) > 0
    assert _plan(device, "split", False).split_pieces(True) > 0  # mean_bwd walks the CSC direction
    assert _plan(device, "alone", False).num_slots == 0 and _plan(device, "one", False).num_nodes == 1


def _one_layout(device, graph, F, variant, vecs, first):
    """Every mode at this (F, layout): f64 bound, sentinels, and bit equality with the layouts of
    the same association class that ran before it in this test (``first``)."""
    lay = layouts(variant)
    for mode in MODES:
        vec = _vec_for(vecs, mode)
        kernel = _kernel_for(device, graph, F, vec, mode)
        where = f"{variant} {mode} {kernel}"
        ops, run = _call(device, graph, F, lay, mode)
        if kernel == "refused":
            with pytest.raises(NotImplementedError, match="F too wide for the gather kernel"):
                run()
            torch.cuda.synchronize()
            for o in ops.values():
                o.check_unchanged()
            continue
        out = run()
        assert out.data_ptr() == ops["y"].view.data_ptr(), where
        ops["y"].check_outside()
        for k, o in ops.items():
            if k != "y":
                o.check_unchanged()
        ref = _reference(graph, F, mode)
        torch.testing.assert_close(out.cpu().double(), ref, rtol=RTOL, atol=ATOL, msg=lambda m: f"{where}: {m}")
        cls = "split" if kernel.startswith("split") else "seq" if F > 8 else kernel
        ref_variant, ref_out = first.setdefault((mode, cls), (variant, out.clone()))
        assert torch.equal(ref_out, out), f"{where}: differs bitwise from layout {ref_variant}"


@pytest.mark.parametrize("graph,F", list(GROUPS), ids=[f"{g}-F{F}" for g, F in GROUPS])
def test_aggregate_f32_lattice(device, graph, F):
    first = {}  # (mode, association class) -> (layout, result) of the first layout that ran it
    for variant, vecs in GROUPS[(graph, F)]:
        _one_layout(device, graph, F, variant, vecs, first)


# EDGE_W (per-slot weights, ``heads`` of them per slot): chan = F / heads joins ok_vec; never split.
# (F, heads, layout, transpose, vec, kernel)
EDGE_W = [
    (2, 2, "aligned", False, 1, "group<2>"),
    (2, 1, "x+1", True, 1, "group<2>"),
    (4, 2, "aligned", False, 2, "group<4>"),
    (3, 3, "pad1", True, 1, "group<4>"),
    (8, 4, "x+1", False, 1, "group<8>"),
    (6, 2, "aligned", True, 1, "group<8>"),
    (12, 4, "aligned", False, 1, "flat<1,16,1>"),    # chan 3: vec 1 by the head width alone
    (24, 4, "aligned", True, 2, "flat<2,16,1>"),     # chan 6
    (24, 4, "pad2", False, 2, "flat<2,16,1>"),
    (24, 4, "x+1", False, 1, "flat<1,32,1>"),
    (64, 4, "aligned", False, 4, "flat<4,16,1>"),
    (64, 4, "x+2", True, 2, "flat<2,32,1>"),
    (64, 4, "add+1", False, 1, "wave<1,2>"),
    (64, 32, "aligned", True, 2, "flat<2,32,1>"),    # chan 2
    (64, 64, "pad4", False, 1, "wave<1,2>"),         # chan 1
    (166, 2, "aligned", False, 1, "flat<1,64,4>"),   # chan 83
    (166, 1, "aligned", True, 2, "wave<2,2>"),
    (256, 4, "ypitch+1", False, 1, "flat<1,64,4>"),
    (512, 8, "pad4", True, 4, "wave<4,2>"),
    (512, 8, "x+2", False, 2, "flat<2,64,4>"),
    (512, 8, "aligned", False, 4, "wave<4,2>"),
    (166, 1, "x+1", True, 1, "flat<1,64,4>"),
    (12, 2, "pad4", True, 2, "flat<2,8,1>"),         # chan 6
    (32, 2, "aligned", False, 4, "flat<4,8,1>"),
    (68, 1, "aligned", False, 4, "flat<4,32,1>"),
    (17, 1, "aligned", True, 1, "flat<1,32,1>"),
    (132, 3, "aligned", False, 4, "wave<4,2>"),      # chan 44
    (516, 1, "aligned", True, 4, "flat<4,64,4>"),
]


EDGE_W_GROUPS = {}
for _c in EDGE_W:
    EDGE_W_GROUPS.setdefault(_c[:2], []).append(_c[2:])


@pytest.mark.parametrize("graph", ["small", "hub"])
@pytest.mark.parametrize("F,heads", list(EDGE_W_GROUPS), ids=[f"F{F}h{h}" for F, h in EDGE_W_GROUPS])
def test_aggregate_edge_w_lattice(device, graph, F, heads):
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.aggregation import aggregate

    plan = _plan(device, graph, False)
    n, S = plan.num_nodes, plan.num_slots
    x, add, _, bias = _inputs(graph, F)
    g = torch.Generator().manual_seed(F * 64 + heads)
    ew = _grid(torch.randn(S, heads, generator=g), 3)
    rowptr, col, _ = (t.cpu().long() for t in plan.csr())
    seg = torch.repeat_interleave(torch.arange(n), rowptr.diff())
    w = ew.double().repeat_interleave(F // heads, dim=1)  # slot s, feature f: ew[s, f // chan]
    first = {}  # (transpose, association class) -> (layout, result)
    for variant, transpose, vec, kernel in EDGE_W_GROUPS[(F, heads)]:
        lay = layouts(variant)
        assert vec == vec_of(F, lay, USE["edge_w"], chan=F // heads), variant
        assert kernel == expected("edge_w", F, vec, True), variant
        ops = {"x": Carved(n, F, lay["x"], device, data=x), "y": Carved(n, F, lay["y"], device),
               "add": Carved(n, F, lay["add"], device, data=add)}
        out = aggregate(plan, ops["x"].view, _lib.AGG_EDGE_W, transpose=transpose, ew=ew.to(device), heads=heads,
                        addend=ops["add"].view, bias=bias.to(device), out=ops["y"].view)
        ops["y"].check_outside()
        ops["x"].check_unchanged()
        ops["add"].check_unchanged()
        src, dst = (seg, col) if transpose else (col, seg)
        ref = torch.zeros(n, F, dtype=torch.float64).index_add_(0, dst, w * x.double()[src]) + add.double() + bias.double()
        torch.testing.assert_close(out.cpu().double(), ref, rtol=RTOL, atol=ATOL, msg=lambda m: f"{variant} {kernel}: {m}")
        ref_variant, ref_out = first.setdefault((transpose, "seq" if F > 8 else kernel), (variant, out.clone()))
        assert torch.equal(ref_out, out), f"{variant} {kernel}: differs bitwise from layout {ref_variant}"


# ---------------------------------------------------------------------------------- bf16 storage
# gnn_aggregate_bf16: vec = the widest of 4 / 2 / 1 with F and the pitches of x, y and the f32
# addend divisible by it, x and y 2*vec-byte and the addend 4*vec-byte aligned; then
#   SUM / MEAN / MEAN_BWD at vec 4 with F / 4 <= 32      agg_wave_group_bf16_kernel<4, 2>
#   F / vec <= 64                                         agg_wave_kernel<V, 1, bf16>
#   F / vec <= 128                                        agg_wave_kernel<V, 2, bf16>
#   F / vec > 128                                         refused (GNN_ERR_UNSUPPORTED)
# The 8-wide form (agg_wave_group_bf16_kernel<8, 4, 4>) runs only under GNNMP_BF_GROUPS=4, an A/B
# switch read once per process: test_aggregate_bf16_eight_wide runs it in a child process.
# (F, x layout, y layout, addend layout, vec, kernel of sum / mean / mean_bwd, kernel of gcn)
_G, _W = "wave_group_bf16<4,2>", "wave<%d,%d,bf16>"
BF16 = [
    (128, ("flat", 0), A0, A0, 4, _G, _W % (4, 1)),
    (128, ("flat", 1), A0, A0, 1, _W % (1, 2), _W % (1, 2)),       # 2-byte aligned
    (128, ("flat", 2), A0, A0, 2, _W % (2, 1), _W % (2, 1)),       # 4-byte aligned
    (128, ("flat", 3), A0, A0, 1, _W % (1, 2), _W % (1, 2)),
    (128, ("flat", 4), A0, A0, 4, _G, _W % (4, 1)),                # 8-byte aligned: still vec 4
    (128, ("flat", 5), A0, A0, 1, _W % (1, 2), _W % (1, 2)),
    (128, ("flat", 6), A0, A0, 2, _W % (2, 1), _W % (2, 1)),
    (128, ("flat", 7), A0, A0, 1, _W % (1, 2), _W % (1, 2)),
    (128, A0, ("flat", 2), A0, 2, _W % (2, 1), _W % (2, 1)),       # by y's pointer
    (128, A0, A0, ("flat", 1), 1, _W % (1, 2), _W % (1, 2)),       # by the f32 addend's pointer (4 bytes)
    (128, A0, A0, ("flat", 2), 2, _W % (2, 1), _W % (2, 1)),       # (8 bytes: vec 2)
    (128, ("pad", 0, 2), A0, A0, 2, _W % (2, 1), _W % (2, 1)),     # by pitch
    (128, A0, ("pad", 0, 1), A0, 1, _W % (1, 2), _W % (1, 2)),
    (128, A0, A0, ("pad", 0, 2), 2, _W % (2, 1), _W % (2, 1)),
    (128, ("pad", 4, 8), ("pad", 8, 12), ("pad", 4, 4), 4, _G, _W % (4, 1)),  # vec 4 over padded pitches
    (64, A0, A0, A0, 4, _G, _W % (4, 1)),
    (64, ("flat", 1), A0, A0, 1, _W % (1, 1), _W % (1, 1)),
    (7, A0, A0, A0, 1, _W % (1, 1), _W % (1, 1)),
    (10, A0, A0, A0, 2, _W % (2, 1), _W % (2, 1)),
    (136, A0, A0, A0, 4, _W % (4, 1), _W % (4, 1)),                # 34 chunks: past the lane-group form
    (166, A0, A0, A0, 2, _W % (2, 2), _W % (2, 2)),
    (166, ("flat", 1), A0, A0, 1, "refused", "refused"),           # 166 chunks of 1
    (256, A0, A0, A0, 4, _W % (4, 1), _W % (4, 1)),
    (256, ("flat", 2), A0, A0, 2, _W % (2, 2), _W % (2, 2)),
    (256, A0, ("flat", 1), A0, 1, "refused", "refused"),
    (512, ("pad", 4, 4), A0, A0, 4, _W % (4, 2), _W % (4, 2)),
    (516, A0, A0, A0, 4, "refused", "refused"),
]


def _bf16_expected(F, lx, ly, la, groups=2):
    """gnn_aggregate_bf16's ok_vec and launch_bf16 restated (groups: GNNMP_BF_GROUPS)."""
    def ok(v):
        return F % v == 0 and all(ld_of(l, F) % v == 0 for l in (lx, ly, la)) and \
            align_bytes(lx, 2) >= min(2 * v, 16) and align_bytes(ly, 2) >= min(2 * v, 16) and \
            align_bytes(la, 4) >= min(4 * v, 16)  # (Carved states alignment up to 16 bytes; buffers are 32-byte aligned)
    vec = 4 if ok(4) else 2 if ok(2) else 1
    n = F // vec
    wave = "refused" if n > 128 else _W % (vec, 1 if n <= 64 else 2)
    if n > 128:
        return vec, wave, wave
    if groups == 4 and ok(8) and F // 8 <= 16:
        return vec, "wave_group_bf16<8,4,4>", wave
    return vec, (_G if vec == 4 and n <= 32 else wave), wave


def _bf16_id(c):
    return "F%d-x%s-y%s-a%s-%s" % (c[0], *("".join(map(str, l)) for l in c[1:4]), c[5])


@pytest.mark.parametrize("graph", ["small", "hub"])
@pytest.mark.parametrize("case", BF16, ids=_bf16_id)
def test_aggregate_bf16_lattice(device, graph, case):
    """f64 over the bf16 inputs, the output rounded once: test_gpu_bf16's bound for sums over hub
    rows (two bf16 ulps of the larger magnitude plus the f32 sum's own error where terms cancel;
    99.9 % within one ulp of the reference)."""
    _bf16_case(device, graph, case)


# GNNMP_BF_GROUPS=4 (an A/B switch of the shipped library, read once per process): the 8-wide
# four-group form agg_wave_group_bf16_kernel<8, 4, 4> for SUM / MEAN / MEAN_BWD when F % 8 == 0,
# F / 8 <= 16, every pitch % 8 == 0, x and y 16-byte and the addend 32-byte aligned.
BF16_GROUPS4 = [
    (128, A0, A0, A0, 4, "wave_group_bf16<8,4,4>", _W % (4, 1)),
    (64, A0, A0, A0, 4, "wave_group_bf16<8,4,4>", _W % (4, 1)),
    (8, A0, A0, A0, 4, "wave_group_bf16<8,4,4>", _W % (4, 1)),
    (128, ("pad", 8, 8), ("pad", 8, 16), ("pad", 8, 8), 4, "wave_group_bf16<8,4,4>", _W % (4, 1)),  # padded pitches
    (128, ("flat", 4), A0, A0, 4, _G, _W % (4, 1)),           # x 8-byte aligned: not 8-wide, the two-group form
    (128, A0, ("pad", 0, 4), A0, 4, _G, _W % (4, 1)),         # ldy % 8 != 0
    (136, A0, A0, A0, 4, _W % (4, 1), _W % (4, 1)),           # 17 pieces of 8 > 16
]


def _bf16_groups4_child():
    """Body of test_aggregate_bf16_eight_wide's child process (GNNMP_BF_GROUPS=4 in its environment)."""
    dev = torch.device("cuda:0")
    for case in BF16_GROUPS4:
        for graph in ("small", "hub"):
            _bf16_case(dev, graph, case, groups=4)


def test_aggregate_bf16_eight_wide(device):
    """The switch is read once per process, so the cases run in one fresh child (this test is about
    that process: nothing else in the suite can launch these three instantiations)."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, GNNMP_BF_GROUPS="4")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_dispatch_agg as t; t._bf16_groups4_child(); print('ok')"
            % (here, os.path.dirname(here)))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def _bf16_case(device, graph, case, groups=2):
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.aggregation import aggregate
    from test_gpu_bf16 import BF_ULP

    F, lx, ly, la, vec, kernel, kernel_gcn = case
    assert (vec, kernel, kernel_gcn) == _bf16_expected(F, lx, ly, la, groups), case
    x32, add, _, bias = _inputs(graph, F)
    xb = x32.to(torch.bfloat16)
    for mode in MODES:
        plan = _plan(device, graph, mode == "gcn")
        n = plan.num_nodes
        ops = {"x": Carved(n, F, lx, device, dtype=torch.bfloat16, data=xb),
               "y": Carved(n, F, ly, device, dtype=torch.bfloat16), "add": Carved(n, F, la, device, data=add)}
        if mode == "sum":
            m, kw = _lib.AGG_SUM, {}
        elif mode == "mean":
            m, kw = _lib.AGG_MEAN, dict(nodew=plan.deg, bias=bias.to(device))
        elif mode == "mean_bwd":
            m, kw = _lib.AGG_MEAN_BWD, dict(nodew=plan.deg, transpose=True)
        else:
            m, kw = _lib.AGG_GCN, dict(nodew=plan.dinv, bias=bias.to(device), relu=True)
        if kernel.startswith("wave_group_bf16<8"):  # the 8-wide form needs a 32-byte addend
            assert ops["add"].view.data_ptr() % 32 == 0
        run = lambda: aggregate(plan, ops["x"].view, m, addend=ops["add"].view, out=ops["y"].view, **kw)
        if kernel == "refused":
            with pytest.raises(NotImplementedError, match="F too wide for the bf16 gather"):
                run()
            torch.cuda.synchronize()
            for o in ops.values():
                o.check_unchanged()
            continue
        out = run()
        assert out.dtype == torch.bfloat16 and out.data_ptr() == ops["y"].view.data_ptr()
        ops["y"].check_outside()
        ops["x"].check_unchanged()
        ops["add"].check_unchanged()
        ei, _ = _edges(graph)
        s, d = ei[0], ei[1]
        if mode == "gcn":
            keep = s != d
            s, d = torch.cat([s[keep], torch.arange(n)]), torch.cat([d[keep], torch.arange(n)])
        deg = torch.bincount(d, minlength=n).double()
        xd = xb.double()
        if mode == "sum":
            msg, to = xd[s], d
        elif mode == "mean":
            msg, to = xd[s] / deg.clamp(min=1)[d][:, None], d
        elif mode == "mean_bwd":
            msg, to = xd[d] / deg.clamp(min=1)[d][:, None], s
        else:
            msg, to = xd[s] * (deg.pow(-0.5)[s] * deg.pow(-0.5)[d])[:, None], d
        z = torch.zeros(n, F, dtype=torch.float64)
        ref = z.clone().index_add_(0, to, msg) + add.double()
        terms = z.clone().index_add_(0, to, msg.abs()) + add.double().abs()
        if mode in ("mean", "gcn"):
            ref, terms = ref + bias.double(), terms + bias.double().abs()
        if mode == "gcn":
            ref = torch.relu(ref)
        got = out.double().cpu()
        dlt = (got - ref).abs()
        mag = torch.maximum(ref.abs(), got.abs())
        assert bool((dlt <= 2 * BF_ULP * mag + 2.0 ** -20 * terms).all()), (mode, float(dlt.max()))
        assert float((dlt <= BF_ULP * ref.abs() + 1e-30).double().mean()) > 0.999, mode
