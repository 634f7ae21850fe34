"""GPU: the SAGE layer-1 weight-gradient TN over the row chunks whose dz can be nonzero (ABI 28).

gnn_aggregate_active_f32 — the CSC-sum launch that finishes dz = [Σ_CSC u | dlogits] — writes one
byte per 16 rows of dz (nonzero iff the group holds a nonzero), and in gnn_gemm_tn_active_f32 each
row block of the dense call walks only its flagged chunks.  Here: the kernel against the dense call
(bit for bit, with every flag set and for flag patterns that leave blocks empty, short or scattered)
and against float64; the producer's flags against the finished dz; and the train step's routing
(flags where gnn_gemm_tn_active_pays, the same logits and gradients bit for bit).
"""
import functools

import pytest
import torch

from oracle import pyg_ref

pytestmark = pytest.mark.gpu

F, NR, NPROJ = 166, 128, 4
SIZES = [16, 25, 121, 4105, 9600]  # one chunk; a tail base shifted back; 257 chunks in 65 row blocks


def rel_l2(a, b, floor=1e-30):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), floor))


def _nchunks(M):
    return (M + 15) // 16


@functools.lru_cache(maxsize=None)
def _case(M):
    """The operands of one size, built once: A = [agg | x] on a half-pair image, h, dz, P."""
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.planes import HalfPairImage

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 + M)
    agg = torch.randn(M, F, generator=g) * 0.7
    x = torch.randn(M, F, generator=g)
    h = torch.relu(torch.randn(M, NR, generator=g))
    dz = torch.randn(M, NPROJ, generator=g) * 1e-3
    proj = torch.randn(NPROJ, NR, generator=g)
    im = HalfPairImage(M, F, F, dev)
    im.fill_x(x.to(dev))
    _lib.call("gnn_split_h2_f32", agg.to(dev).data_ptr(), F, im.n, im.k1, im.ptr, im.ld, im.ps, 0, im.col2, im.exp,
              _lib.stream_handle(dev))
    return dict(A=torch.cat([agg, x], 1).double(), h=h, dz=dz, proj=proj, im=im, h_d=h.to(dev), proj_d=proj.to(dev))


def _patterns(M):
    """name -> (chunks with nonzero dz, chunks flagged), bool [nchunks] each."""
    n = _nchunks(M)
    g = torch.Generator().manual_seed(77 + M)
    z = torch.zeros(n, dtype=torch.bool)
    pats = {"none": (z.clone(), z.clone())}
    first = z.clone()
    first[0] = True
    last = z.clone()
    last[-1] = True
    alt = z.clone()
    alt[::2] = True
    rnd = torch.rand(n, generator=g) < 0.2
    span = z.clone()
    span[n // 3: max(n // 3 + 1, n // 3 + n // 5)] = True
    pats.update(first=(first, first), last=(last, last), alternating=(alt, alt), random20=(rnd, rnd), span=(span, span))
    sup = rnd | (torch.rand(n, generator=g) < 0.3)  # zero chunks flagged too: a superset is legal
    pats["superset"] = (rnd, sup)
    if M == 9600:  # 5 active chunks in 100 row blocks of 6: one block with two, three with one, the rest empty
        five = z.clone()
        five[[3, 4, 200, 431, 599]] = True
        pats["n_act5"] = (five, five)
    return pats


PATTERN_CASES = [(M, name) for M in SIZES for name in ("none", "first", "last", "alternating", "random20", "span",
                                                       "superset")] + [(9600, "n_act5")]


def _run(M, dz, flags, h=None):
    from elliptic_gnn_project_amd.fused import gemm_tn

    c = _case(M)
    dev = c["h_d"].device
    kw = dict(dz=dz.to(dev), proj=c["proj_d"], h=c["h_d"] if h is None else h, hscale=2.0, planes=c["im"])
    act = None if flags is None else flags.to(torch.uint8).to(dev)
    dW, db, dW2, dzs = gemm_tn(NR, None, None, dz_active=act, **kw)
    torch.cuda.synchronize()
    return torch.cat([dW[0], dW[1]], 1), db, dW2, dzs


@pytest.mark.parametrize("M", SIZES)
def test_all_flags_is_the_dense_partition(M):
    """Every flag set: the dense kernel's row blocks, base rows and tail included — every output bit
    for bit the call without flags."""
    c = _case(M)
    dense = _run(M, c["dz"], None)
    flagged = _run(M, c["dz"], torch.ones(_nchunks(M), dtype=torch.bool))
    for a, b in zip(dense, flagged):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,name", PATTERN_CASES)
def test_flag_patterns_vs_f64(M, name):
    """dz zero outside the pattern's chunks: within test_tn_h2_vs_f64's relL2 1e-6 of float64 (its
    reference expression), bit for bit the dense call on the same operands (a skipped chunk adds exact
    zeros there), deterministic, and the h rows of unflagged chunks never read (NaN there changes no
    bit)."""
    c = _case(M)
    nz, flags = _patterns(M)[name]
    rows_nz = nz.repeat_interleave(16)[:M]
    dz = torch.where(rows_nz[:, None], c["dz"], torch.zeros_like(c["dz"]))
    out = _run(M, dz, flags)
    if not bool(nz.any()):
        for t in out:
            assert not bool(t.any())  # exactly zero
    else:
        Gd = torch.where(c["h"] > 0, (dz.double() @ c["proj"].double()) * 2.0, torch.zeros(M, NR, dtype=torch.float64))
        refs = (Gd.t() @ c["A"], Gd.sum(0), dz.double().t() @ c["h"].double(), dz.double().sum(0))
        for k, (t, r) in enumerate(zip(out, refs)):
            e = rel_l2(t, r)
            print(f"M={M} {name} output {k}: relL2 {e:.3e}")
            assert e < 1e-6, (k, e)
    again = _run(M, dz, flags)
    dense = _run(M, dz, None)
    for a, b, d in zip(out, again, dense):
        assert torch.equal(a, b) and torch.equal(a, d)
    rows_off = ~flags.repeat_interleave(16)[:M]
    h_nan = c["h_d"].clone()
    h_nan[rows_off.to(h_nan.device)] = float("nan")
    poisoned = _run(M, dz, flags, h=h_nan)
    for a, b in zip(out, poisoned):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


# ------------------------------------------------------------------ the producer
def _elliptic(n, e, seed=9):
    from elliptic_gnn_project_amd.dataset_elliptic import prepare_inputs, synthetic_elliptic

    return prepare_inputs(synthetic_elliptic(num_nodes=n, num_edges=e, seed=seed),
                          dict(use_time_scalar=True, symmetrize_edges=True, train_window_k=10))


def _hub_edges(n=3000, seed=4):
    """A random graph plus hub sources with 40 / 300 / 1500 out-edges (CSC columns past a lane's
    32-slot walk and past one 256-slot pass) and a run of isolated nodes."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n - 100, (4 * n,), generator=g)
    dst = torch.randint(0, n - 100, (4 * n,), generator=g)
    hubs = [torch.stack([torch.full((d,), hb), torch.randint(0, n, (d,), generator=g)])
            for hb, d in ((7, 40), (700, 300), (1901, 1500))]
    return torch.cat([torch.stack([src, dst])] + hubs, dim=1), n


def _graphs(which):
    if which == "hub":
        return _hub_edges()
    d = _elliptic(4000 if which == "elliptic" else 4009, 5000)
    return d.edge_index, d.x.size(0)


@pytest.mark.parametrize("which", ["elliptic", "hub", "tail9"])
def test_producer_flags_are_the_nonzero_groups(device, which):
    """The CSC sum of u into dz[:, :2] with dz[:, 2:] as the other columns: the same sums as the plain
    launch, and flags exactly the 16-row groups of the finished dz that hold a nonzero (NaN counts) —
    the narrow form has no long-segment rows, so nothing is flagged beyond them."""
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.aggregation import aggregate
    from elliptic_gnn_project_amd.graph import get_plan

    ei, N = _graphs(which)
    plan = get_plan(ei.to(device), N)
    g = torch.Generator().manual_seed(5)
    u = torch.randn(N, 2, generator=g) * (torch.rand(N, 1, generator=g) < 0.04)
    u[N // 2, 1] = float("nan")
    right = torch.randn(N, 2, generator=g) * (torch.rand(N, 1, generator=g) < 0.02)
    if which == "tail9":
        right[-1, 1] = 1.0  # the partial last group, flagged through the other columns alone
    dz = torch.zeros(N, 4, device=device)
    dz[:, 2:] = right.to(device)
    plain = aggregate(plan, u.to(device), _lib.AGG_SUM, transpose=True)
    n = (N + 15) // 16
    flags = torch.full((n + 16,), 7, dtype=torch.uint8, device=device)
    aggregate(plan, u.to(device), _lib.AGG_SUM, transpose=True, out=dz[:, :2], active=(flags, dz[:, 2:]))
    torch.cuda.synchronize()
    assert torch.equal(dz[:, :2].isnan(), plain.isnan())
    assert torch.equal(dz[:, :2].nan_to_num(1.0), plain.nan_to_num(1.0))
    want = torch.zeros(n * 16, dtype=torch.bool, device=device)
    want[:N] = (dz != 0).any(1)  # (NaN != 0)
    want = want.view(n, 16).any(1)
    assert bool(want.any()) and not bool(want.all())
    assert torch.equal(flags[:n] != 0, want)
    assert bool((flags[n:] == 7).all())  # nothing written past the last group


def test_producer_refuses_wide_rows(device):
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.aggregation import aggregate
    from elliptic_gnn_project_amd.graph import get_plan

    ei, N = _graphs("elliptic")
    plan = get_plan(ei.to(device), N)
    flags = torch.zeros((N + 15) // 16, dtype=torch.uint8, device=device)
    with pytest.raises(NotImplementedError):
        aggregate(plan, torch.randn(N, 8, device=device), _lib.AGG_SUM, transpose=True, active=(flags, None))


# ------------------------------------------------------------------ the train step's routing
def _step(device, data, monkeypatch, active):
    from elliptic_gnn_project_amd import fused
    from elliptic_gnn_project_amd.planes import register_input
    from elliptic_gnn_project_amd.train_gnn import _make_loss_fn, build_model
    from elliptic_gnn_project_amd.train_ops import unit_gradient

    seen = []
    real = fused.gemm_tn

    def spy(*a, **k):
        if not k.get("check_planes") and k.get("dz") is not None:
            seen.append((k.get("dz_active"), k["dz"]))
        return real(*a, **k)

    monkeypatch.setattr(fused, "_TN_ACTIVE", active)
    monkeypatch.setattr(fused, "gemm_tn", spy)
    x, ei, y, mask = (t.to(device) for t in (data.x, data.edge_index, data.y, data.train_mask))
    cw = pyg_ref.class_weight(y[mask].cpu())
    denom = float(mask.sum())
    torch.manual_seed(11)
    model = build_model("sage", x.size(1), dict(hidden_dim=128, layers=2, dropout=0.5)).to(device)
    loss_fn = _make_loss_fn({}, cw, model, 1, 34)
    model.train()
    torch.manual_seed(5)
    xr = register_input(x)
    with loss_fn.target(y, mask, denom):
        logits = model(xr, ei)
    loss = loss_fn.full(logits, y, mask, denom=denom)
    loss.backward(unit_gradient(device))
    torch.cuda.synchronize()
    assert len(seen) == 1
    return logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}, seen[0]


def test_routing_flags_where_they_pay(device, monkeypatch):
    """115,000 nodes (row blocks of 480 rows: past the in-kernel fold): the TN receives flags that
    cover dz's nonzero rows, chunk by chunk; with the switch off, the same logits and the same
    gradients bit for bit (the row blocks and their order are the dense call's)."""
    data = _elliptic(115_000, 130_000, seed=1)
    lo, go, (flags, dz) = _step(device, data, monkeypatch, True)
    assert flags is not None and flags.dtype == torch.uint8
    N = dz.size(0)
    n = (N + 15) // 16
    nzrow = torch.zeros(n * 16, dtype=torch.bool, device=device)
    nzrow[:N] = (dz != 0).any(1)
    nzc = nzrow.view(n, 16).any(1)
    assert bool(((flags[:n] != 0) | ~nzc).all())
    frac = float((flags[:n] != 0).float().mean())
    print(f"active chunks: {frac:.3f}")
    assert 0.0 < frac < 0.5  # the rolling train window: a fraction of the timesteps
    lf, gf, (none, _) = _step(device, data, monkeypatch, False)
    assert none is None
    assert torch.equal(lo, lf)
    for k in go:
        assert torch.equal(go[k], gf[k]), k


def test_routing_no_flags_below_the_threshold(device, monkeypatch):
    data = _elliptic(100_000, 113_000, seed=1)
    _, _, (flags, _) = _step(device, data, monkeypatch, True)
    assert flags is None
