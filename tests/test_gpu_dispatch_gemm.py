"""fused.gemm_nt / fused.gemm_tn at the pitch and alignment branches of their dispatchers.

test_gpu_fused.py covers the dispatchers by shape with allocator-aligned, dense operands.  Here
one operand at a time sits at an 8- or 4-byte aligned pointer or on a padded pitch
(dispatch_operands.Carved), so each predicate's other outcome runs:

  gemm_skinny.hip  launch_nt_skinny   Nc <= 8:  VEC = v_ok over k1, k2, lda1, lda2, a1, a2;
                                                nt_skinny_n_kernel<VEC, NC = 1|2|4|8>
                                      K <= 8:   VEC = skk_vec over Nc, ldc and C's pointer;
                                                nt_skinny_k_kernel<VEC, KK = 1|2|4|8>
                   tn_skinny_ok       Nr <= 8:  VEC = tn_vec over the A operands; declined when
                                                K / VEC > 256 lanes: the generic TN takes the call
  gemm_f32.hip     gemm_nt_dispatch   v4 / v2 / scalar A loads, wvec (w1 / w2), bvec4 (bt)
                   gemm_tn_kernel     v2 / scalar A loads, the dz form's 16-byte dz row load
  gemm_x3.hip      launch_nt_x3       nt_ws_ok (gemm_ws.hip: dense 16-byte A, 16-byte C) or the
                                      classic kernel at av = 4 | 2 | 1
                   launch_nt_h2s      v4 / v2 / scalar A staging (math="half_pair")
                   tn_h2s_ok          16-byte g with ldg % 4 == 0, else the split-bf16 TN
  gemm_planes.hip  tn_h2_ok (g form)  16-byte g with ldg % 4 == 0, else the split-bf16 image TN
                   tn_planes_ok       any g (scalar loads)

Every case checks the result against float64 at the bound the aligned test of the same kernel
and math mode uses (test_gpu_fused.py, test_gpu_h2s.py), that inputs are untouched, and that no
byte outside an ``out=`` view changed.  Whichever kernel takes a call must meet that bound.
"""
import pytest
import torch

from dispatch_operands import Carved, align_bytes, ld_of

pytestmark = pytest.mark.gpu

A0 = ("flat", 0)
# name -> layout; the widest vector a row pitch / pointer allows is noted per use
LAY = {"a16": A0, "p8": ("flat", 2), "p4": ("flat", 1), "p12": ("flat", 3), "ld+2": ("pad", 0, 2),
       "ld+1": ("pad", 0, 1), "pad16": ("pad", 4, 8), "pad8": ("pad", 2, 4)}


def _vec(parts):
    """v_ok / tn_vec / skk_vec: parts = [(width, layout)]: the widest of 4 / 2 / 1 every part allows."""
    for v in (4, 2):
        if all(w % v == 0 and ld_of(l, w) % v == 0 and align_bytes(l) >= 4 * v for w, l in parts):
            return v
    return 1


def rel_l2(a, b, floor=1e-7):  # test_gpu_fused.rel_l2
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), floor / 1e-5))


def _operands(M, k1, k2, n, seed):
    g = torch.Generator().manual_seed(seed)
    a1 = torch.randn(M, k1, generator=g)
    a2 = torch.randn(M, k2, generator=g) if k2 else None
    W = torch.randn(n, k1 + k2, generator=g) / (k1 + k2) ** 0.5
    bias = torch.randn(n, generator=g)
    A = torch.cat([a1, a2], 1) if k2 else a1
    return a1, a2, W, bias, A


def _carve(t, layout, device):
    return None if t is None else Carved(t.size(0), t.size(1), layout, device, data=t)


def _done(ins, out=None):
    for o in ins:
        if o is not None:
            o.check_unchanged()
    if out is not None:
        out.check_outside()


# ------------------------------------------------------------------------------- skinny NT, Nc <= 8
# (M, k1, k2, a1 layout, a2 layout, VEC)
SKINNY_N = [
    (257, 64, 64, "a16", "a16", 4),
    (257, 64, 64, "p8", "a16", 2),     # one operand 8-byte aligned: the lower VEC for both
    (257, 64, 64, "a16", "p4", 1),
    (257, 64, 64, "p12", "p8", 1),
    (257, 64, 64, "ld+2", "a16", 2),   # by pitch
    (257, 64, 64, "a16", "ld+1", 1),
    (257, 64, 64, "pad16", "pad16", 4),
    (257, 64, 64, "pad8", "pad16", 2),
    (33, 6, 0, "a16", None, 2),        # by width
    (33, 7, 9, "a16", "a16", 1),
    (1000, 166, 166, "a16", "a16", 2),
    (1000, 166, 166, "a16", "p4", 1),
    (33, 384, 0, "p8", None, 2),
]


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("M,k1,k2,l1,l2,vec", SKINNY_N,
                         ids=[f"M{c[0]}-k{c[1]}+{c[2]}-{c[3]}-{c[4]}-v{c[5]}" for c in SKINNY_N])
def test_nt_skinny_n(device, M, k1, k2, l1, l2, vec, n):
    """nt_skinny_n_kernel<vec, NC>: bt and w1 / w2 forms, bias + ReLU, C stored into a 4-byte
    aligned padded view (scalar stores)."""
    from elliptic_gnn_project_amd.fused import gemm_nt

    assert vec == _vec([(k1, LAY[l1])] + ([(k2, LAY[l2])] if k2 else []))
    a1, a2, W, bias, A = _operands(M, k1, k2, n, M + k1 + n)
    ref = torch.relu(A.double() @ W.double().t() + bias.double())
    c1, c2 = _carve(a1, LAY[l1], device), _carve(a2, LAY[l2] if l2 else None, device)
    b = bias.to(device)
    for wform in (False, True):
        out = Carved(M, n, ("pad", 1, 3), device)
        kw = dict(w1=W[:, :k1].contiguous().to(device), w2=W[:, k1:].contiguous().to(device) if k2 else None) \
            if wform else {}
        for math in ("split_bf16", "f32"):  # the skinny kernels serve both modes
            c = gemm_nt(c1.view, None if wform else W.t().contiguous().to(device), n,
                        a2=c2.view if c2 is not None else None, bias=b, relu=True, out=out.view, math=math, **kw)
            _done([c1, c2], out)
            torch.testing.assert_close(c.cpu().double(), ref, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------- skinny NT, K <= 8
# (M, Nc, out layout, VEC)
SKINNY_K = [
    (257, 64, "a16", 4),
    (257, 64, "p8", 2),       # by C's pointer
    (257, 64, "p4", 1),
    (257, 64, "ld+2", 2),     # by ldc
    (257, 64, "ld+1", 1),
    (257, 64, "pad16", 4),
    (257, 64, "pad8", 2),
    (33, 33, "a16", 1),       # by Nc
    (33, 34, "a16", 2),
    (33, 36, "a16", 4),
    (1000, 256, "a16", 4),
    (1000, 255, "a16", 1),    # 255 lanes of one column
]


@pytest.mark.parametrize("k1", [1, 2, 3, 8])
@pytest.mark.parametrize("M,n,lo,vec", SKINNY_K, ids=[f"M{c[0]}-N{c[1]}-{c[2]}-v{c[3]}" for c in SKINNY_K])
def test_nt_skinny_k(device, M, n, lo, vec, k1):
    """nt_skinny_k_kernel<vec, KK>: VEC from Nc, ldc and the pointer of a padded ``out=`` view; A at
    a 4-byte aligned pointer (scalar loads); with the column sums on the 16-byte and 4-byte cases."""
    from elliptic_gnn_project_amd.fused import gemm_nt

    assert vec == _vec([(n, LAY[lo])])
    a1, _, W, bias, A = _operands(M, k1, 0, n, M + 3 * k1 + n)
    ref = A.double() @ W.double().t() + bias.double()
    c1 = _carve(a1, LAY["p4"], device)
    out = Carved(M, n, LAY[lo], device)
    colsum = lo in ("a16", "p4", "ld+2")
    got = gemm_nt(c1.view, W.t().contiguous().to(device), n, bias=bias.to(device), out=out.view, colsum=colsum)
    c, cs = got if colsum else (got, None)
    _done([c1], out)
    torch.testing.assert_close(c.cpu().double(), ref, rtol=1e-5, atol=1e-5)
    if colsum:
        assert rel_l2(cs, ref.sum(0)) < 1e-5


# ------------------------------------------------------------------------------- skinny TN, Nr <= 8
# (M, k1, k2, a1 layout, a2 layout, VEC or None: tn_skinny_ok declines)
SKINNY_TN = [
    (257, 64, 64, "a16", "a16", 4),
    (257, 64, 64, "p8", "a16", 2),
    (257, 64, 64, "a16", "p4", 1),
    (257, 64, 64, "ld+2", "a16", 2),
    (257, 64, 64, "a16", "ld+1", 1),
    (257, 64, 64, "pad16", "pad8", 2),
    (33, 7, 9, "a16", "a16", 1),
    (1000, 166, 166, "a16", "a16", 2),
    (1000, 128, 128, "p4", "a16", 1),     # 256 chunks of 1: the last K the skinny form takes
    (257, 300, 0, "p8", None, 2),         # 150 chunks of 2
    (257, 258, 0, "p4", None, None),      # 258 chunks of 1 > 256 lanes: declined, the generic TN
    (257, 384, 0, "ld+1", None, None),
    (257, 384, 0, "a16", None, 4),
]


@pytest.mark.parametrize("nr", [1, 2, 3, 8])
@pytest.mark.parametrize("M,k1,k2,l1,l2,vec", SKINNY_TN,
                         ids=[f"M{c[0]}-k{c[1]}+{c[2]}-{c[3]}-{c[4]}-v{c[5]}" for c in SKINNY_TN])
def test_tn_skinny(device, M, k1, k2, l1, l2, vec, nr):
    """tn_skinny_kernel<vec, NR>, and the generic TN where tn_skinny_ok declines (in both math
    modes: the split-bf16 MFMA TN and gemm_tn_kernel's scalar A loads).  G at a 4-byte pointer."""
    from elliptic_gnn_project_amd.fused import gemm_tn

    v = _vec([(k1, LAY[l1])] + ([(k2, LAY[l2])] if k2 else []))
    took = (k1 + k2) // v <= 256
    assert vec == (v if took else None)
    a1, a2, _, _, A = _operands(M, k1, k2, 1, M + k1 + 7 * nr)
    G = torch.randn(M, nr, generator=torch.Generator().manual_seed(nr))
    c1, c2, cg = _carve(a1, LAY[l1], device), _carve(a2, LAY[l2] if l2 else None, device), _carve(G, LAY["p4"], device)
    for math in ("split_bf16", "f32"):
        dW, db, _, _ = gemm_tn(nr, c1.view, c2.view if c2 is not None else None, g=cg.view, math=math)
        _done([c1, c2, cg])
        dWfull = torch.cat([dW[0], dW[1]], 1) if dW[1] is not None else dW[0]
        bound = 1e-6 if took else 1e-5  # test_gemm_tn_skinny's / test_gemm_tn's
        assert rel_l2(dWfull, G.double().t() @ A.double()) < bound
        assert rel_l2(db, G.double().sum(0)) < bound


# ------------------------------------------------------------------------------- gemm_f32 (math="f32")
F32_A = [("a16", "a16", 4), ("p8", "a16", 2), ("a16", "p4", 1), ("ld+2", "a16", 2), ("a16", "ld+1", 1),
         ("pad16", "pad16", 4)]


@pytest.mark.parametrize("lb", ["a16", "p4", "p8", "ld+2", "pad16"])   # bvec4: 16-byte bt with ldb % 4 == 0
@pytest.mark.parametrize("l1,l2,vec", F32_A, ids=[f"{c[0]}-{c[1]}-v{c[2]}" for c in F32_A])
@pytest.mark.parametrize("M,k1,k2,n", [(257, 64, 64, 64), (33, 20, 12, 33)])
def test_gemm_f32_nt_bt(device, M, k1, k2, n, l1, l2, vec, lb):
    from elliptic_gnn_project_amd.fused import gemm_nt

    assert vec == _vec([(k1, LAY[l1]), (k2, LAY[l2])])
    a1, a2, W, bias, A = _operands(M, k1, k2, n, M + n)
    c1, c2, cb = _carve(a1, LAY[l1], device), _carve(a2, LAY[l2], device), _carve(W.t().contiguous(), LAY[lb], device)
    out = Carved(M, n, ("pad", 1, 3), device)
    c = gemm_nt(c1.view, cb.view, n, a2=c2.view, bias=bias.to(device), out=out.view, math="f32")
    _done([c1, c2, cb], out)
    torch.testing.assert_close(c.cpu().double(), A.double() @ W.double().t() + bias.double(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("math", ["f32", "split_bf16"])
@pytest.mark.parametrize("lw1,lw2,wvec", [("a16", "a16", 4), ("p8", "a16", 2), ("a16", "p4", 1), ("ld+2", "a16", 2),
                                          ("a16", "ld+1", 1), ("pad16", "pad8", 2)])
@pytest.mark.parametrize("M,k1,k2,n", [(257, 64, 64, 64), (33, 20, 12, 33)])
def test_gemm_nt_weight_alignment(device, M, k1, k2, n, lw1, lw2, wvec, math):
    """wvec / wvec2: Linear weights read in place from 8- and 4-byte aligned views and padded
    pitches (GradBucket-style flat parameter storage), the f32 kernel and the split-bf16 B prep."""
    from elliptic_gnn_project_amd.fused import gemm_nt

    assert wvec == _vec([(k1, LAY[lw1]), (k2, LAY[lw2])])
    a1, a2, W, bias, A = _operands(M, k1, k2, n, M + n + 1)
    w1, w2 = _carve(W[:, :k1], LAY[lw1], device), _carve(W[:, k1:], LAY[lw2], device)
    c = gemm_nt(a1.to(device), None, n, a2=a2.to(device), w1=w1.view, w2=w2.view, bias=bias.to(device), math=math)
    _done([w1, w2])
    torch.testing.assert_close(c.cpu().double(), A.double() @ W.double().t() + bias.double(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("math", ["f32", "split_bf16"])
@pytest.mark.parametrize("form", ["g", "g_mask", "dz_mask"])
@pytest.mark.parametrize("l1,l2,lg", [("a16", "a16", "a16"), ("p8", "a16", "a16"), ("a16", "p4", "p4"),
                                      ("ld+1", "a16", "p8"), ("pad16", "ld+2", "ld+1")])
@pytest.mark.parametrize("M,nr,k1,k2", [(257, 64, 64, 64), (33, 33, 20, 12)])
def test_gemm_tn_alignment(device, M, nr, k1, k2, l1, l2, lg, form, math):
    """The generic TNs (gemm_tn_kernel v2 / scalar A loads; the split-bf16 MFMA TN) with A, and
    g / dz / h, off 16 bytes.  dz is [M, 4] with nproj = 4: at a 4- or 8-byte pointer its rows may
    not be read as one 16-byte load."""
    from elliptic_gnn_project_amd.fused import gemm_tn

    a1, a2, _, _, A = _operands(M, k1, k2, 1, M + nr)
    g_ = torch.Generator().manual_seed(M + nr + 1)
    h = torch.relu(torch.randn(M, nr, generator=g_))
    dz = torch.randn(M, 4, generator=g_)
    proj = torch.randn(4, nr, generator=g_)
    G = torch.randn(M, nr, generator=g_)
    c1, c2 = _carve(a1, LAY[l1], device), _carve(a2, LAY[l2], device)
    ins = [c1, c2]
    if form == "dz_mask":
        G = dz.double() @ proj.double()
        cz = _carve(dz, LAY[lg], device)
        kw = dict(dz=cz.view, proj=proj.to(device))
        ins.append(cz)
    else:
        cg = _carve(G, LAY[lg], device)
        kw = dict(g=cg.view)
        ins.append(cg)
    G = G.double()
    if form != "g":
        ch = _carve(h, LAY[lg], device)
        G = torch.where(h > 0, G * 2.0, torch.zeros_like(G))
        kw.update(h=ch.view, hscale=2.0)
        ins.append(ch)
    gout = Carved(M, nr, ("pad", 1, 3), device)
    dW, db, dW2, dzs = gemm_tn(nr, c1.view, c2.view, gout=gout.view, math=math, **kw)
    _done(ins, gout)
    torch.testing.assert_close(gout.view.cpu().double(), G, rtol=1e-5, atol=1e-5)
    assert rel_l2(torch.cat([dW[0], dW[1]], 1), G.t() @ A.double()) < 1e-5
    assert rel_l2(db, G.sum(0)) < 1e-5
    if form == "dz_mask":
        assert rel_l2(dW2, dz.double().t() @ h.double()) < 1e-5
        assert rel_l2(dzs, dz.double().sum(0)) < 1e-5


# ------------------------------------------------------------------------------- MFMA shapes
MFMA_SHAPES = [(203, 64, 0, 128), (128, 16, 16, 128), (1000, 166, 166, 128), (257, 64, 64, 64)]
MFMA_LAY = [("a16", "a16", "a16"),      # the aligned call: gemm_ws / the half-pair v4 staging
            ("p8", "a16", "a16"),       # A1 8-byte aligned: gemm_ws declines; av = 2 / v2
            ("a16", "p4", "a16"),       # A2 (A1 when k2 = 0) 4-byte aligned: av = 1 / scalar
            ("ld+2", "a16", "a16"),     # lda1 != k1: gemm_ws declines
            ("a16", "ld+1", "a16"),
            ("a16", "a16", "p4"),       # C off 16 bytes: gemm_ws declines, scalar C stores
            ("a16", "a16", "ld+2"),     # ldc % 4 != 0
            ("pad16", "pad16", "pad16")]


@pytest.mark.parametrize("math", ["split_bf16", "half_pair"])
@pytest.mark.parametrize("l1,l2,lo", MFMA_LAY, ids=["-".join(c) for c in MFMA_LAY])
@pytest.mark.parametrize("M,k1,k2,n", MFMA_SHAPES)
def test_gemm_nt_mfma_alignment(device, M, k1, k2, n, l1, l2, lo, math):
    """Shapes that take gemm_ws / gemm_x3 when aligned, with one operand misaligned: whichever
    kernel takes the call meets the math mode's bound (split-bf16: test_gemm_nt's 1e-5; half-pair:
    test_h2s_nt_vs_f64's relL2 1e-6 and 2e-6 of the row scale)."""
    from elliptic_gnn_project_amd.fused import gemm_nt, h2s_nt_ok

    if k2 == 0:
        l1 = l1 if l1 != "a16" else l2  # the one A operand takes whichever layout the case varies
    a1, a2, W, bias, A = _operands(M, k1, k2, n, M + n + 2)
    c1, c2 = _carve(a1, LAY[l1], device), _carve(a2, LAY[l2], device)
    out = Carved(M, n, LAY[lo], device)
    c = gemm_nt(c1.view, None, n, a2=c2.view if c2 is not None else None, w1=W[:, :k1].contiguous().to(device),
                w2=W[:, k1:].contiguous().to(device) if k2 else None, bias=bias.to(device), out=out.view, math=math)
    _done([c1, c2], out)
    ref = A.double() @ W.double().t() + bias.double()
    torch.testing.assert_close(c.cpu().double(), ref, rtol=1e-5, atol=1e-5)
    if math == "half_pair" and h2s_nt_ok(n, k1, k2):
        scale = (A.double().abs() @ W.double().abs().t()).amax(1, keepdim=True) + bias.double().abs().max()
        assert float(((c.cpu().double() - ref).abs() / scale).max()) < 2e-6
        assert rel_l2(c, ref) < 1e-6


@pytest.mark.parametrize("l1,l2,lg", [("a16", "a16", "a16"), ("p4", "a16", "a16"), ("a16", "ld+1", "a16"),
                                      ("a16", "a16", "p8"), ("a16", "a16", "ld+2"), ("pad16", "pad16", "pad16")])
@pytest.mark.parametrize("M,k1,k2,nr", [(257, 64, 64, 64), (1000, 96, 0, 128), (33, 32, 32, 64)])
def test_gemm_tn_half_pair_alignment(device, M, k1, k2, nr, l1, l2, lg):
    """The half-pair TN (row_exp from the forward NT) reads g in 16-byte pieces: tn_h2s_ok declines
    a g off 16 bytes or with ldg % 4 != 0 and the split-bf16 TN serves; A is staged by scalar
    loads at any alignment.  test_h2s_tn_vs_f64's bound either way."""
    from elliptic_gnn_project_amd.fused import gemm_nt, gemm_tn

    if k2 == 0:
        l1 = l1 if l1 != "a16" else l2
    a1, a2, _, _, A = _operands(M, k1, k2, 1, M + nr + 3)
    g_ = torch.Generator().manual_seed(M + nr)
    G = torch.randn(M, nr, generator=g_)
    w = torch.randn(16, k1 + k2, generator=g_).to(device)
    c1, c2, cg = _carve(a1, LAY[l1], device), _carve(a2, LAY[l2], device), _carve(G, LAY[lg], device)
    rexp = torch.empty(M, dtype=torch.int32, device=device)
    gemm_nt(c1.view, None, 16, a2=c2.view if c2 is not None else None, w1=w[:, :k1].contiguous(),
            w2=w[:, k1:].contiguous() if k2 else None, math="half_pair", row_exp=rexp)
    dW, db, _, _ = gemm_tn(nr, c1.view, c2.view if c2 is not None else None, g=cg.view, math="half_pair", row_exp=rexp)
    _done([c1, c2, cg])
    dWfull = torch.cat([dW[0], dW[1]], 1) if dW[1] is not None else dW[0]
    assert rel_l2(dWfull, G.double().t() @ A.double()) < 1e-6
    assert rel_l2(db, G.double().sum(0)) < 1e-6


# ------------------------------------------------------------------------------- image-A TN gates
@pytest.mark.parametrize("lg,h2_takes", [("a16", True), ("p8", False), ("p4", False), ("ld+2", False), ("pad16", True)])
@pytest.mark.parametrize("nr", [64, 128])
def test_gemm_tn_image_g_alignment(device, nr, lg, h2_takes):
    """dW = gᵀ·x over x's cached images (gemm_planes.hip): tn_h2_ok's g form reads g in 16-byte
    pieces (a 16-byte g with ldg % 4 == 0, else it declines); tn_planes_ok's split-bf16 image TN
    loads g by scalars and takes any g.  gemm_tn_input then serves the call either way, at
    test_gemm_tn's bound."""
    from elliptic_gnn_project_amd.fused import gemm_tn, gemm_tn_input
    from elliptic_gnn_project_amd.planes import HalfPairImage, register_input, x_only_image

    M, F = 1000, 166
    gen = torch.Generator().manual_seed(nr)
    x = register_input(torch.randn(M, F, generator=gen).to(device))
    G = torch.randn(M, nr, generator=gen)
    cg = _carve(G, LAY[lg], device)
    ref = G.double().t() @ x.double().cpu()
    im_h2, im_sp = x_only_image(x, HalfPairImage), x_only_image(x)
    assert gemm_tn(nr, None, g=cg.view, planes=im_h2, check_planes=True) == h2_takes
    assert gemm_tn(nr, None, g=cg.view, planes=im_sp, check_planes=True)
    (dW, _), db, _, _ = gemm_tn_input(nr, x, cg.view)
    (dWs, _), dbs, _, _ = gemm_tn(nr, None, g=cg.view, planes=im_sp)
    _done([cg])
    for w, b in ((dW, db), (dWs, dbs)):
        assert rel_l2(w, ref) < 1e-5
        assert rel_l2(b, G.double().sum(0)) < 1e-5
