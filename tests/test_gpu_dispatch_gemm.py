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
                                      classic gemm_nt_x3_kernel<AV, BV, ABF, CBF> at AV = 4 | 2 | 1
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
# (nr, k1 + k2, KT): every rung of tn_kt_ladder (gemm_x3.hip), which launch_tn_x3 and launch_tn_h2s
# share.  nkt = ceil(K / 32) k-tiles; nr > 64: KT = the first of 6 / 8 / 11 / 12 >= nkt; nr <= 64 (the
# half-N mapping): KT = the first of 2 / 3 / 4 / 6 >= ceil(nkt / 2)
KT_RUNGS = [(128, 192, 6), (128, 256, 8), (128, 352, 11), (128, 384, 12),
            (64, 128, 2), (64, 192, 3), (64, 256, 4), (64, 384, 6)]


@pytest.mark.parametrize("math", ["split_bf16", "half_pair"])
@pytest.mark.parametrize("nr,K,kt", KT_RUNGS, ids=[f"N{c[0]}-K{c[1]}-KT{c[2]}" for c in KT_RUNGS])
def test_gemm_tn_kt_rungs(device, nr, K, kt, math):
    """gemm_tn_x3_kernel / gemm_tn_h2s_kernel (the plain g form) at each k-tile count their shared
    ladder picks, 80 rows.  test_gemm_tn_alignment's bound for the split-bf16 TN, and
    test_gemm_tn_half_pair_alignment's for the half-pair one (its row_exp formed here as the NT
    defines it: max |A[r, :]| < 2^E_r)."""
    from elliptic_gnn_project_amd.fused import gemm_tn

    nkt = -(-K // 32)
    assert kt == next(v for v in ((2, 3, 4, 6) if nr <= 64 else (6, 8, 11, 12)) if v >= (-(-nkt // 2) if nr <= 64 else nkt))
    M, k2 = 80, 64
    a1, a2, _, _, A = _operands(M, K - k2, k2, 1, nr + K)
    G = torch.randn(M, nr, generator=torch.Generator().manual_seed(nr + K + 1))
    kw = {}
    if math == "half_pair":
        kw["row_exp"] = torch.frexp(A.abs().amax(1)).exponent.to(torch.int32).to(device)
    dW, db, _, _ = gemm_tn(nr, a1.to(device), a2.to(device), g=G.to(device), math=math, **kw)
    bound = 1e-5 if math == "split_bf16" else 1e-6
    assert rel_l2(torch.cat([dW[0], dW[1]], 1), G.double().t() @ A.double()) < bound
    assert rel_l2(db, G.double().sum(0)) < bound


# ------------------------------------------------------------------------------- ladder rungs
# The launchers share their ladders (gemm_common.hpp with_rung / tn_forms, gemm_ws.hip with_nt_epi);
# the cases below are the rungs no other GEMM test launches, each at the bound the test it cites
# applies to the same kernel.

@pytest.mark.parametrize("math", ["f32", "split_bf16"])
@pytest.mark.parametrize("with_gout", [False, True])
def test_gemm_tn_dz_form_without_mask(device, with_gout, math):
    """tn_forms' PROJ, no MASK rungs on the generic TNs (gemm_tn_kernel<true, false, ..>,
    gemm_tn_x3_kernel<true, false, .., GOUT, ..>): G = dz·P with no h.  test_gemm_tn_alignment's bounds."""
    from elliptic_gnn_project_amd.fused import gemm_tn

    M, nr, k1, k2 = 80, 64, 64, 64
    a1, a2, _, _, A = _operands(M, k1, k2, 1, 71)
    g_ = torch.Generator().manual_seed(72)
    dz = torch.randn(M, 4, generator=g_)
    proj = torch.randn(4, nr, generator=g_)
    G = dz.double() @ proj.double()
    gout = torch.empty(M, nr, device=device) if with_gout else None
    dW, db, _, dzs = gemm_tn(nr, a1.to(device), a2.to(device), dz=dz.to(device), proj=proj.to(device), gout=gout,
                             math=math)
    if with_gout:
        torch.testing.assert_close(gout.cpu().double(), G, rtol=1e-5, atol=1e-5)
    assert rel_l2(torch.cat([dW[0], dW[1]], 1), G.t() @ A.double()) < 1e-5
    assert rel_l2(db, G.sum(0)) < 1e-5
    assert rel_l2(dzs, dz.double().sum(0)) < 1e-5


def _split_image(a, x, device, half_pair=False):  # test_gpu_planes._image / test_gpu_h2._image
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.planes import HalfPairImage, SplitImage

    im = (HalfPairImage if half_pair else SplitImage)(a.size(0), a.size(1), x.size(1), device)
    im.fill_x(x.to(device))
    _lib.call("gnn_split_h2_f32" if half_pair else "gnn_split_planes_f32", a.to(device).data_ptr(), a.size(1), im.n,
              im.k1, im.ptr, im.ld, im.ps, 0, im.col2, *((im.exp,) if half_pair else ()), _lib.stream_handle(device))
    return im


# (k per operand, nr, form, gout): image rows of 128 (KT = 4) and 240 (KT = 8) bf16, the forms of
# tn_forms that test_gpu_planes.py leaves out, and the N <= 64 split-K mapping with gout
TN_PLANES_RUNGS = [(60, 128, "dz", False), (120, 128, "dz", True), (120, 64, "g", True), (60, 128, "dz_mask", True)]


@pytest.mark.parametrize("k,nr,form,with_gout", TN_PLANES_RUNGS,
                         ids=[f"k{c[0]}-N{c[1]}-{c[2]}-{'gout' if c[3] else 'nogout'}" for c in TN_PLANES_RUNGS])
def test_gemm_tn_planes_rungs(device, k, nr, form, with_gout):
    """gemm_tn_planes_kernel at KT = 4 / 8 (launch_tn_planes' ladder over the image width) and at the
    PROJ / MASK / GOUT forms test_gpu_planes.py does not launch.  test_tn_planes_vs_f64's bounds."""
    from elliptic_gnn_project_amd.fused import gemm_tn

    M = 80
    g_ = torch.Generator().manual_seed(k + nr)
    a1, a2 = torch.randn(M, k, generator=g_), torch.randn(M, k, generator=g_)
    h = torch.relu(torch.randn(M, nr, generator=g_))
    dz = torch.randn(M, 4, generator=g_) * 1e-3
    proj = torch.randn(4, nr, generator=g_)
    G = torch.randn(M, nr, generator=g_) * 1e-3
    if form == "g":
        kw = dict(g=G.to(device))
    else:
        G = dz @ proj
        kw = dict(dz=dz.to(device), proj=proj.to(device))
    if form == "dz_mask":
        G = torch.where(h > 0, G * 2.0, torch.zeros_like(G))
        kw.update(h=h.to(device), hscale=2.0)
    gout = torch.empty(M, nr, device=device) if with_gout else None
    im = _split_image(a1, a2, device)
    assert (im.ld + 31) // 32 == (4 if k == 60 else 8)
    assert gemm_tn(nr, None, None, planes=im, check_planes=True, gout=gout, **kw)
    dW, db, dW2, dzs = gemm_tn(nr, None, None, planes=im, gout=gout, **kw)
    assert rel_l2(torch.cat([dW[0], dW[1]], 1), G.double().t() @ torch.cat([a1, a2], 1).double()) < 1e-6
    assert rel_l2(db, G.double().sum(0)) < 1e-6
    if form != "g":
        assert rel_l2(dzs, dz.double().sum(0)) < 1e-6
    if form == "dz_mask":
        assert rel_l2(dW2, dz.double().t() @ h.double()) < 1e-6
    if with_gout:
        torch.testing.assert_close(gout.cpu(), G, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("image,epi", [("split", "bias_relu"), ("half_pair", "bias_relu"), ("half_pair", "keep_bits")])
def test_gemm_nt_image_epilogue_rungs(device, image, epi):
    """with_nt_epi's rungs the image NT tests leave out: bias + ReLU alone on gemm_nt_planes_kernel and
    gemm_nt_h2_kernel, and the half-pair form's dropout from precomputed keep bits without the
    projection.  test_nt_planes_vs_f64's / test_nt_h2_vs_f64's bound."""
    from oracle.dropout_hash import keep_mask
    from elliptic_gnn_project_amd.fused import gemm_nt

    M, F, n, p, seed = 80, 166, 128, 0.5, 99
    g_ = torch.Generator().manual_seed(len(image) + len(epi))
    agg, x = torch.randn(M, F, generator=g_) * 0.7, torch.randn(M, F, generator=g_)
    w1, w2 = torch.randn(n, F, generator=g_) * 0.08, torch.randn(n, F, generator=g_) * 0.08
    bias = torch.randn(n, generator=g_) * 0.1
    ref = torch.relu(torch.cat([agg, x], 1).double() @ torch.cat([w1, w2], 1).double().t() + bias.double())
    kw = dict(w1=w1.to(device), w2=w2.to(device), bias=bias.to(device), relu=True)
    if epi == "keep_bits":
        keep = torch.from_numpy(keep_mask(seed, M, n, p)).to(torch.int64)
        ref = ref * keep.double() * 2.0
        # bit c of word c / 32 of a row (NTArgs::kmask)
        words = (keep.view(M, 4, 32) << torch.arange(32)).sum(2)
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
        kw.update(dropout_p=p, seed=seed, keep_mask=words.to(device))
    im = _split_image(agg, x, device, half_pair=image == "half_pair")
    assert gemm_nt(None, None, n, planes=im, check_planes=True, **kw)
    c = gemm_nt(None, None, n, planes=im, **kw)
    assert rel_l2(c, ref) < 1e-6


@pytest.mark.parametrize("lw1,lw2,wvec", [("a16", "a16", 4), ("p8", "a16", 2), ("a16", "p4", 1)])
def test_gemm_nt_x3_without_b_image(device, lw1, lw2, wvec):
    """gemm_nt_x3_kernel<AV, BV = 4 | 2 | 1, ..>: with a workspace too small for the B image the kernel
    splits W in place, at the widest vector its rows allow.  test_gemm_nt_weight_alignment's bound."""
    from elliptic_gnn_project_amd.fused import gemm_nt

    M, k1, k2, n = 80, 64, 64, 64
    assert wvec == _vec([(k1, LAY[lw1]), (k2, LAY[lw2])])
    a1, a2, W, bias, A = _operands(M, k1, k2, n, 73)
    w1, w2 = _carve(W[:, :k1], LAY[lw1], device), _carve(W[:, k1:], LAY[lw2], device)
    c = gemm_nt(a1.to(device), None, n, a2=a2.to(device), w1=w1.view, w2=w2.view, bias=bias.to(device),
                math="split_bf16", workspace=torch.empty(1, device=device))
    _done([w1, w2])
    torch.testing.assert_close(c.cpu().double(), A.double() @ W.double().t() + bias.double(), rtol=1e-5, atol=1e-5)


def _rb(t):  # test_gpu_bf16.rb
    return t.to(torch.bfloat16).to(t.dtype)


# (A one element off 4 bytes, B image, w1 layout, C dtype): AV = 1 | 2, BV = 0 | 2 | 1, CBF
NT_BF16_RUNGS = [(True, True, "a16", "bf16"), (False, True, "a16", "f32"), (False, False, "a16", "f32"),
                 (False, False, "p4", "bf16"), (True, False, "p4", "f32")]


@pytest.mark.parametrize("odd,image,lw,cdt", NT_BF16_RUNGS,
                         ids=[f"av{1 if c[0] else 2}-{'img' if c[1] else 'w'}-{c[2]}-{c[3]}" for c in NT_BF16_RUNGS])
def test_gemm_nt_bf16_rungs(device, odd, image, lw, cdt):
    """The bf16-storage gemm_nt_x3_kernel<AV, BV, true, CBF> off test_gemm_nt_bf16's one form (AV = 2, the
    B image, bf16 C): A at a 2-byte aligned pointer, W split in place, f32 C.  test_gemm_nt_bf16's
    global ceiling and relative L2 bound."""
    from elliptic_gnn_project_amd.fused import gemm_nt

    M, k1, k2, n = 80, 64, 64, 64
    a1, a2, W, bias, _ = _operands(M, k1, k2, n, 74)
    a1, a2 = a1.to(torch.bfloat16), a2.to(torch.bfloat16)

    def place(t):  # bf16 rows at a 4-byte (flat allocation) or a 2-byte aligned pointer
        buf = torch.empty(t.numel() + 2, dtype=torch.bfloat16, device=device)
        v = buf[1 if odd else 2:][:t.numel()].view_as(t)
        v.copy_(t)
        return v

    w1, w2 = _carve(W[:, :k1], LAY[lw], device), _carve(W[:, k1:], LAY["a16"], device)
    out = torch.empty(M, n, dtype=torch.bfloat16 if cdt == "bf16" else torch.float32, device=device)
    c = gemm_nt(place(a1), None, n, a2=place(a2), w1=w1.view, w2=w2.view, bias=bias.to(device), out=out,
                **({} if image else dict(workspace=torch.empty(1, device=device))))
    _done([w1, w2])
    ref = torch.cat([a1, a2], 1).double() @ _rb(W).double().t() + bias.double()
    d = (c.double().cpu() - ref).abs()
    assert float(d.max()) <= float((2.0 ** -8 * ref.abs() + 1e-5).max()), float(d.max())
    assert rel_l2(c, ref) < 3e-3


@pytest.mark.parametrize("form", ["g", "g_mask"])
@pytest.mark.parametrize("k", [128, 166], ids=["KT8", "KT12"])
def test_gemm_tn_bf16_rungs(device, k, form):
    """The bf16-storage gemm_tn_x3_kernel<.., KT = 8 | 12, true, HBF = false, ..>: no h, and an f32 h
    (test_gemm_tn_bf16 gives a bf16 h).  Its bounds: G rounded to bf16 is the MFMA operand."""
    from elliptic_gnn_project_amd.fused import gemm_tn

    M, nr = 80, 128
    g_ = torch.Generator().manual_seed(k)
    a1 = torch.randn(M, k, generator=g_).to(torch.bfloat16)
    a2 = torch.randn(M, k, generator=g_).to(torch.bfloat16)
    h = torch.relu(torch.randn(M, nr, generator=g_))
    g = torch.randn(M, nr, generator=g_) * 1e-3
    G, kw = g, {}
    if form == "g_mask":
        kw = dict(h=h.to(device), hscale=2.0)
        G = torch.where(h > 0, g * 2.0, torch.zeros_like(g))
    gout = torch.empty(M, nr, device=device)
    dW, db, _, _ = gemm_tn(nr, a1.to(device), a2.to(device), g=g.to(device), gout=gout, **kw)
    torch.testing.assert_close(gout.cpu(), G, rtol=1e-5, atol=1e-8)
    assert rel_l2(torch.cat([dW[0], dW[1]], 1), _rb(G).double().t() @ torch.cat([a1, a2], 1).double()) < 1e-5
    assert rel_l2(db, G.sum(0)) < 1e-5


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
