"""The GEMM dispatch's decision table: what the side-effect-free entries of libgnnmp answer over a
lattice of NT / TN calls (gnn_gemm_nt_planes_ok, gnn_gemm_tn_planes_ok, gnn_gemm_nt_workspace_size,
gnn_gemm_tn_workspace_size, gnn_gemm_nt_colsum_blocks, gnn_gemm_tn_sq_blocks, gnn_gemm_tn_active_pays).
No launch, no device: the pointers in the params are never read.

    GNNMP_LIB=<a libgnnmp.so> python tests/golden/make_gemm_dispatch_golden.py          # writes the JSON
    GNNMP_LIB=<a libgnnmp.so> python tests/golden/make_gemm_dispatch_golden.py --print  # to stdout

tests/golden/gemm_dispatch_golden.json was written from a build of the commit BEFORE the dispatch
moved into csrc/gemm_dispatch.hip; tests/test_gemm_dispatch_host.py replays the lattice against the
built library (in a child process without the GNNMP_TN_* A/B switches) and requires the same rows.
Regenerate it only with a change that means to move a routing rule.

The lattice crosses the edges the rules turn on — fully over the shapes, one option at a time off a
base call, and a seeded sample of the full product of options.
"""
import ctypes
import itertools
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_dispatch_golden.json")
FAKE = 1 << 20  # an aligned address that is never read

NT_M = [0, 1, 31, 32, 1000]
NT_N = [1, 8, 9, 64, 128, 129]
NT_K = [(166, 166), (128, 128), (16, 0), (8, 0), (165, 0)]
# image kinds: 0 none, 1 split, 2 half-pair, 3 bf16; (ld, col2) with the (k1, k2) that fill it
IMG_GEOM = [(336, 168, 166, 166), (256, 128, 128, 128), (176, 168, 166, 0)]
NT_SHAPES = [(k1, k2, 0, 0, 0) for k1, k2 in NT_K] + [(k1, k2, img, ld, col2) for img in (1, 2, 3)
                                                      for ld, col2, k1, k2 in IMG_GEOM]  # k1, k2, img, ld, col2
NT_FIELDS = ["M", "N", "shape", "math", "mask", "dropout", "nproj", "c_bf16", "planes_exp",
             "a1", "epi", "a_bf16"]
TN_M = [1, 15, 16, 1000, 27196, 32768, 32769, 114688, 114689, 203769]
TN_NR = [1, 8, 9, 64, 65, 128, 129]
TN_SHAPES = NT_SHAPES[len(NT_K):]
TN_FIELDS = ["M", "Nr", "shape", "dz", "h", "gout", "math", "g4", "graph", "dz_cols",
             "nodes_off", "a1"]
TN_SIZES = [(128, 332, 4), (64, 128, 0), (8, 332, 0), (128, 384, 0)]


def nt_rows():
    rows = set()
    base = dict(math=0, mask=0, dropout=0, nproj=0, c_bf16=0, planes_exp=0, a1=0, epi=1, a_bf16=0)

    def add(M, N, shape, **kw):
        r = dict(base, M=M, N=N, shape=shape, **kw)
        if NT_SHAPES[shape][2] == 3:
            r["a_bf16"] = 1
        rows.add(tuple(r[f] for f in NT_FIELDS))

    shapes = range(len(NT_SHAPES))
    opts = dict(math=[0, 1, 2], mask=[0, 1], dropout=[0, 1], nproj=[0, 2, 4], c_bf16=[0, 1], planes_exp=[0, 3, 101],
                a1=[0, 1], epi=[0, 1], a_bf16=[0, 1])
    for M, N, shape in itertools.product(NT_M, NT_N, shapes):
        add(M, N, shape)  # every shape on the base call
    for (M, N), shape in itertools.product([(1000, 128), (32, 64)], shapes):
        for name, vals in opts.items():  # one option at a time
            for v in vals:
                add(M, N, shape, **{name: v})
    rng = random.Random(7)
    for _ in range(400):  # the full product, sampled
        add(rng.choice(NT_M), rng.choice(NT_N), rng.choice(shapes), **{n: rng.choice(v) for n, v in opts.items()})
    return sorted(rows)


def nt_params(_lib, row):
    r = dict(zip(NT_FIELDS, row))
    r["k1"], r["k2"], r["img"], r["ld"], r["col2"] = NT_SHAPES[r["shape"]]
    p = _lib.GnnGemmNTParams()
    p.M, p.N, p.k1, p.k2 = r["M"], r["N"], r["k1"], r["k2"]
    if r["a1"] or not r["img"]:
        p.a1, p.lda1 = FAKE, r["k1"]
        if r["k2"]:
            p.a2, p.lda2 = FAKE, r["k2"]
    p.w1, p.ldw1 = FAKE, r["k1"]
    if r["k2"]:
        p.w2, p.ldw2 = FAKE, r["k2"]
    p.c, p.ldc = FAKE, r["N"]
    if r["epi"]:
        p.bias, p.relu = FAKE, 1
    if r["dropout"]:
        p.dropout_p, p.seed = 0.5, 1
    if r["nproj"]:
        p.proj, p.nproj, p.z, p.ldz = FAKE, r["nproj"], FAKE, 4
    p.math = r["math"]
    p.a_dtype, p.c_dtype = r["a_bf16"], r["c_bf16"]
    if r["mask"]:
        p.mask, p.ldmask, p.mask_scale = FAKE, r["N"], 1.0
    if r["img"]:
        p.a_planes, p.planes_ld, p.planes_col2 = FAKE, r["ld"], r["col2"]
        p.planes_stride = max(r["M"], 1) * r["ld"]
        p.planes_format = _lib.PLANES_HALF_PAIR if r["img"] == 2 else _lib.PLANES_SPLIT_BF16
        p.planes_exp = r["planes_exp"]
    return p


def tn_rows():
    rows = set()
    base = dict(dz=0, h=0, gout=0, math=0, g4=0, graph=0, dz_cols=0, nodes_off=0, a1=0)

    def add(M, Nr, shape, **kw):
        r = dict(base, M=M, Nr=Nr, shape=shape, **kw)
        if not r["graph"]:
            r["dz_cols"] = r["nodes_off"] = 0
        rows.add(tuple(r[f] for f in TN_FIELDS))

    shapes = range(len(TN_SHAPES))
    wide = [s for s in shapes if TN_SHAPES[s][3] == 336 or TN_SHAPES[s][2] == 2]  # 336-wide, and every half-pair image
    forms = [dict(dz=0), dict(dz=1, h=1), dict(dz=1, h=1, gout=1), dict(dz=1), dict(dz=0, h=1), dict(dz=0, gout=1)]
    for M, Nr, shape in itertools.product(TN_M, TN_NR, wide):
        add(M, Nr, shape)                 # the g form
        add(M, Nr, shape, dz=1, h=1)      # the dz form with h
    for M, shape, form in itertools.product([16, 1000, 114689], wide, forms):
        for math, g4, a1 in [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 0, 1)]:  # one option at a time
            add(M, 128, shape, math=math, g4=g4, a1=a1, **form)
    for M, shape, form in itertools.product(TN_M, wide[:3], forms[:3]):
        for dz_cols, nodes_off in itertools.product([1, 2, 3], [0, 1]):  # dz_graph
            add(M, 128, shape, graph=1, dz_cols=dz_cols, nodes_off=nodes_off, **form)
    rng = random.Random(11)
    for _ in range(300):
        add(rng.choice(TN_M), rng.choice(TN_NR), rng.choice(shapes), math=rng.choice([0, 1, 2]),
            g4=rng.choice([0, 1]), a1=rng.choice([0, 1]), graph=rng.choice([0, 0, 1]), dz_cols=rng.choice([1, 2, 3]),
            nodes_off=rng.choice([0, 0, 1]), **rng.choice(forms))
    return sorted(rows)


def tn_params(_lib, row, keep):
    r = dict(zip(TN_FIELDS, row))
    r["k1"], r["k2"], r["img"], r["ld"], r["col2"] = TN_SHAPES[r["shape"]]
    p = _lib.GnnGemmTNParams()
    p.M, p.Nr, p.k1, p.k2 = r["M"], r["Nr"], r["k1"], r["k2"]
    if r["dz"]:
        p.dz, p.lddz, p.proj, p.nproj = FAKE, 4, FAKE, 4
    else:
        p.g, p.ldg = FAKE + 4 * r["g4"], r["Nr"]
    bf = r["img"] == 3
    if r["h"]:
        p.h, p.ldh, p.hscale, p.h_dtype = FAKE, r["Nr"], 2.0, int(bf)
    if r["gout"]:
        p.gout, p.ldgout = FAKE, r["Nr"]
    if r["a1"]:
        p.a1, p.lda1 = FAKE, r["k1"]
        if r["k2"]:
            p.a2, p.lda2 = FAKE, r["k2"]
    p.math, p.a_dtype = r["math"], int(bf)
    p.a_planes, p.planes_ld, p.planes_col2, p.planes_stride = FAKE, r["ld"], r["col2"], r["M"] * r["ld"]
    p.planes_format = _lib.PLANES_HALF_PAIR if r["img"] == 2 else _lib.PLANES_SPLIT_BF16
    if r["graph"]:
        g = _lib.GnnGraph(r["M"] + r["nodes_off"], 4 * r["M"], FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
        keep.append(g)
        p.dz_graph, p.dz_u, p.ldu, p.dz_cols = ctypes.addressof(g), FAKE, 2, r["dz_cols"]
    return p


def sweep():
    """{table: rows}; a row is its inputs followed by the library's answers."""
    for name in ("GNNMP_TN_KSPLIT_MAXM", "GNNMP_TN_CSC_INKERNEL"):
        if name in os.environ:
            raise SystemExit(f"{name} is set: the table is the default routing")
    sys.path.insert(0, ROOT)
    from elliptic_gnn_project_amd import _lib

    lib = _lib.load()
    out = {"nt_fields": NT_FIELDS + ["planes_ok", "colsum_blocks"], "tn_fields": TN_FIELDS + ["planes_ok"],
           "nt_shapes": NT_SHAPES, "tn_shapes": TN_SHAPES, "shape_fields": ["k1", "k2", "img", "ld", "col2"]}
    nt = []
    for row in nt_rows():
        p, nb = nt_params(_lib, row), _lib.c_i32(-1)
        _lib.check(lib.gnn_gemm_nt_colsum_blocks(p, ctypes.byref(nb)), "colsum_blocks")
        nt.append(list(row) + [lib.gnn_gemm_nt_planes_ok(p), nb.value])
    out["nt"] = nt
    keep = []
    out["tn"] = [list(row) + [lib.gnn_gemm_tn_planes_ok(tn_params(_lib, row, keep))] for row in tn_rows()]
    n = _lib.c_size(0)
    sizes = []
    for M, (Nr, Kc, nproj) in itertools.product([0] + TN_M, TN_SIZES):
        _lib.check(lib.gnn_gemm_tn_workspace_size(M, Nr, Kc, nproj, ctypes.byref(n)), "tn_workspace_size")
        sizes.append([M, Nr, Kc, nproj, n.value])
    out["tn_workspace_size"] = sizes
    sizes = []
    for N, (k1, k2) in itertools.product(NT_N, NT_K):
        _lib.check(lib.gnn_gemm_nt_workspace_size(N, k1, k2, ctypes.byref(n)), "nt_workspace_size")
        sizes.append([N, k1, k2, n.value])
    out["nt_workspace_size"] = sizes
    nb = _lib.c_i32(0)
    out["tn_sq_blocks"] = []
    for n_out in (1, 63, 64, 65, 2 * 16 + 2, 128 * 332 + 128 + 4 * 128 + 4, 128 * 384 + 128):
        _lib.check(lib.gnn_gemm_tn_sq_blocks(n_out, ctypes.byref(nb)), "sq_blocks")
        out["tn_sq_blocks"].append([n_out, nb.value])
    out["tn_active_pays"] = [[M, lib.gnn_gemm_tn_active_pays(M)]
                             for M in sorted(set([0] + TN_M + [32 * 256 * k + d for k in (1, 7, 13, 14, 15, 56, 57)
                                                               for d in (0, 1)]))]
    return out


if __name__ == "__main__":
    table = sweep()
    if "--print" in sys.argv:
        json.dump(table, sys.stdout, separators=(",", ":"))
    else:
        with open(OUT, "w") as fh:
            json.dump(table, fh, separators=(",", ":"))
        print("wrote", OUT, {k: len(v) for k, v in table.items()})
