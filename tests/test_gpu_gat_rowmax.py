"""(ABI 25) The g form of the half-pair TN with its per-row-block scale taken from the producer's
row-group maxima (gnn_gemm_tn_params.g_rowmax, GNN_ROWMAX_ROWS = 16 rows per group) instead of its
own pass over G — GATNet's lin weight gradient dW = dxhᵀ · x, the maxima written by the hidden
attention backward as it stores dxh (gnn_gat_bwd_act_proj_f32 dxh_rowmax).  Exact maxima give the
scan's power-of-two scale, so the TN is bit for bit the scanning TN; an upper bound keeps fp32-class
accuracy; an in-place edit of G voids the tag."""
import pytest
import torch

pytestmark = pytest.mark.gpu

R = 16


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _rowmax(G):
    M = G.size(0)
    pad = (-M) % R
    a = torch.nn.functional.pad(G.abs(), (0, 0, 0, pad)).view(-1, R * G.size(1)).amax(1)
    return a.contiguous().view(torch.int32)  # float bits (non-negative: int order = float order)


@pytest.mark.parametrize("M,F,nr", [(20011, 166, 64), (4099, 166, 128), (777, 40, 16)])
@pytest.mark.parametrize("prof", ["rand", "ramp", "late"])
def test_tn_g_form_rowmax_equals_scan(device, M, F, nr, prof):
    from elliptic_gnn_project_amd.aggregation import tag_rowmax
    from elliptic_gnn_project_amd.fused import gemm_tn
    from elliptic_gnn_project_amd.planes import HalfPairImage, register_input, x_only_image

    g_ = torch.Generator().manual_seed(M + nr)
    x = register_input(torch.randn(M, F, generator=g_).to(device))
    G = torch.randn(M, nr, generator=g_) * torch.exp(torch.randn(M, 1, generator=g_) * 2) * 1e-3
    if prof == "ramp":
        G = G * torch.logspace(-4, 4, M).view(M, 1)
    elif prof == "late":
        G = G * (torch.arange(M).view(M, 1) % 800 == 799)
    im = x_only_image(x, HalfPairImage)
    Gd = G.to(device)
    (dW0, _), db0, _, _ = gemm_tn(nr, None, g=Gd, planes=im)  # the scanning TN
    Gt = Gd.clone()
    tag_rowmax(Gt, _rowmax(Gt))
    (dW1, _), db1, _, _ = gemm_tn(nr, None, g=Gt, planes=im)
    assert torch.equal(dW0, dW1) and torch.equal(db0, db1)
    # an upper bound (8x, 64x the true maxima): a coarser but valid scale
    for k in (8.0, 64.0):
        Gu = Gd.clone()
        tag_rowmax(Gu, (_rowmax(Gu).view(torch.float32) * k).contiguous().view(torch.int32))
        (dW2, _), _, _, _ = gemm_tn(nr, None, g=Gu, planes=im)
        ref = G.double().t() @ x.double().cpu()
        assert _rel(dW2, ref) < 2e-6, (k, _rel(dW2, ref))


def test_rowmax_tag_voided_by_inplace_edit(device):
    from elliptic_gnn_project_amd.aggregation import rowmax_of, tag_rowmax

    G = torch.randn(100, 8, device=device)
    rm = _rowmax(G)
    tag_rowmax(G, rm)
    assert rowmax_of(G) is rm
    G.mul_(2.0)  # its maxima are stale now
    assert rowmax_of(G) is None


def test_gat_producer_rowmax_is_exact(device):
    """The attention backward's dxh_rowmax equals the per-16-row max |dxh| it stored."""
    from elliptic_gnn_project_amd import aggregation, gnn
    from elliptic_gnn_project_amd.planes import register_input

    seen = {}
    real = aggregation.tag_rowmax

    def spy(g, rm):
        seen["g"], seen["rm"] = g, rm
        real(g, rm)

    aggregation.tag_rowmax = spy
    try:
        g_ = torch.Generator().manual_seed(5)
        N, E, F = 5000, 12000, 166
        x = register_input(torch.randn(N, F, generator=g_).to(device))
        ei = torch.randint(0, N, (2, E), generator=g_).to(device)
        y = torch.randint(0, 2, (N,), generator=g_).to(device)
        torch.manual_seed(0)
        m = gnn.GATNet(F, hidden_dim=64, layers=2, dropout=0.3, heads=4).to(device).train()
        torch.nn.functional.cross_entropy(m(x, ei), y).backward()
        torch.cuda.synchronize()
    finally:
        aggregation.tag_rowmax = real
    assert "g" in seen
    assert torch.equal(seen["rm"], _rowmax(seen["g"]))


@pytest.mark.parametrize("graph", ["small", "hub"])
def test_gat_generic_route_rowmax_is_exact(device, graph):
    """The generic one-wave-per-row backward forms dxh_rowmax in a pass of its own (gat.hip
    rowmax_group_kernel).  xh [n, 256] carved 4 bytes past a 16-byte boundary lowers the vector width
    to 1, 256 slots > 64, so gat_route answers generic; n = 37 (two full 16-row groups and one of 5)
    and n = 300 (a last group of 12, one degree-3000 row).  The tag equals the per-16-row max |dxh|."""
    from dispatch_operands import Carved
    from test_gpu_parity import GRAPHS, rand_graph

    from elliptic_gnn_project_amd import _lib, aggregation

    seen = {}
    real = aggregation.tag_rowmax

    def spy(g, rm):
        seen["g"], seen["rm"] = g, rm
        real(g, rm)

    H, C, n = 4, 64, GRAPHS[graph]["n"]
    F = H * C
    ei = rand_graph(**GRAPHS[graph]).to(device)
    g_ = torch.Generator().manual_seed(11)
    cx = Carved(n, F, ("flat", 1), device, data=torch.randn(n, F, generator=g_))
    xh = cx.view.detach().requires_grad_(True)
    assert xh.data_ptr() % 8 == 4 and xh.stride(0) == F
    att_s, att_d = (torch.randn(1, H, C, generator=g_).to(device) for _ in range(2))
    bias = torch.randn(F, generator=g_).to(device)
    w_out = (torch.randn(2, F, generator=g_) * 0.1).to(device).requires_grad_(True)
    dz = torch.randn(n, 2, generator=g_).to(device)
    aggregation.tag_rowmax = spy
    try:
        z = aggregation.gat_attention_proj(xh, att_s, att_d, bias, w_out, ei, H, C, 0.2, _lib.ACT_ELU, 0.5,
                                           0x1234_5678_9ABC, None)
        z.backward(dz)
        torch.cuda.synchronize()
    finally:
        aggregation.tag_rowmax = real
    assert "g" in seen and seen["g"].shape == (n, F)
    assert seen["rm"].numel() == (n + R - 1) // R
    assert torch.equal(seen["rm"], _rowmax(seen["g"]))
    assert torch.equal(xh.grad, seen["g"]) and bool(seen["g"].abs().amax() > 0)


@pytest.mark.parametrize("layers,heads,hidden", [(2, 4, 64), (3, 4, 64)])
def test_gat_step_rowmax_bit_identical(device, layers, heads, hidden):
    """The GAT train step with the producer's maxima == the step with the TN's own scan, bit for bit
    (registered input: layer 1's lin on x's half-pair image)."""
    from elliptic_gnn_project_amd import aggregation, gnn
    from elliptic_gnn_project_amd.planes import register_input

    g_ = torch.Generator().manual_seed(3)
    N, E, F = 6000, 15000, 166
    x = register_input(torch.randn(N, F, generator=g_).to(device))
    ei = torch.randint(0, N, (2, E), generator=g_).to(device)
    y = torch.randint(0, 2, (N,), generator=g_).to(device)
    res = {}
    for on in (True, False):
        aggregation._GAT_ROWMAX = on
        try:
            torch.manual_seed(0)
            m = gnn.GATNet(F, hidden_dim=hidden, layers=layers, dropout=0.3, heads=heads).to(device).train()
            torch.manual_seed(5)
            logits = m(x, ei)
            torch.nn.functional.cross_entropy(logits, y).backward()
            res[on] = (logits.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()})
        finally:
            aggregation._GAT_ROWMAX = True
    assert torch.equal(res[True][0], res[False][0])
    for k, g in res[False][1].items():
        assert torch.equal(res[True][1][k], g), k
