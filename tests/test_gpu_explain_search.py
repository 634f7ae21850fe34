"""GPU: the GNNExplainer search (elliptic_gnn_project_amd/explain.py) and its fused mask step K16
(csrc/explain.hip gnn_explain_mask_step_f32).

* K16 against the float64 mirror ``host_mask_step`` at every access width, with partial last groups,
  epoch 0 and a later step, one and three blocks (one of them empty): mask, exp_avg, exp_avg_sq and h
  at relative L2 <= 1e-5 (the project's bar against f64), mask at max abs <= 1e-6, hard_out exact,
  two calls bitwise equal, a bad block id reported and skipped.
* ``explain_nodes`` end to end against the CPU f64 restatement tests/explainer_ref.py: sigmoided masks
  within 1e-5 max abs, hard masks equal.  1e-5 is the project's bar; the restatement's own f32-vs-f64
  divergence after 20 epochs is about 25x smaller (asserted <= 1e-6 in explainer_ref.case).
* The subgraph run equals the full-graph run (this fails if GCN is given L hops), the batch equals
  single runs, the fused step equals the torch step, the model is left as it was, and the CLI.
Parity with PyG itself is unpinned (PyG is not installed), as for tests/test_gpu_explain.py.
"""
import json

import numpy as np
import pytest
import torch

import explainer_ref as R

pytestmark = pytest.mark.gpu

LR = 0.01


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ----------------------------------------------------------------------------- K16 vs the mirror
def _place(a, layout, ld, device):
    """The CPU array ``a`` ([n] or [rows, F]) on the device in one of the layouts: contiguous, rows of a
    [rows, ld] buffer, or such rows starting one element into the allocation (4-byte offset for f32)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if layout == "contiguous":
        return t.to(device)
    if t.dim() == 1:  # plain form: only the offset layout differs
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=device)
        buf[1:] = t.to(device)
        return buf[1:]
    rows, F = t.shape
    off = 1 if layout == "offset" else 0
    buf = torch.zeros(rows * ld + off, dtype=t.dtype, device=device)
    v = buf.as_strided((rows, F), (ld, 1), off)
    v.copy_(t.to(device))
    return v


def _inputs(shape, B, seed):
    g = np.random.default_rng(seed)
    n = shape[0]
    logit = (2.0 * g.standard_normal(shape)).astype(np.float32)
    flat = logit.reshape(-1)
    flat[::5] = 12.0
    flat[2::7] = -12.0
    grad = (g.standard_normal(shape) * (g.random(shape) < 0.7)).astype(np.float32)
    x = g.standard_normal(shape).astype(np.float32)
    m1 = (0.01 * g.standard_normal(shape)).astype(np.float32)
    m2 = (1e-4 * g.random(shape)).astype(np.float32)
    hard = (g.random(shape) < 0.6).astype(np.uint8)
    # blocks in runs of rows; with B = 3 block 1 stays empty
    blk = (np.sort(g.integers(0, B, n)) if B == 1 else np.where(np.arange(n) < (n + 1) // 2, 0, 2)).astype(np.int32)
    cnt = np.zeros(B)
    np.add.at(cnt, blk, hard.reshape(n, -1).sum(1))
    inv = np.where(cnt > 0, 1.0 / np.maximum(cnt, 1), 0.0)
    return logit, grad, x, m1, m2, hard, blk, inv.astype(np.float32)


def _check_step(device, shape, ld, layout, epoch0, B, gate):
    from elliptic_gnn_project_amd import explain as X

    logit, grad, x, m1, m2, hard, blk, inv = _inputs(shape, B, seed=shape[0] * 7 + B)
    t = 1 if epoch0 else 6
    if epoch0:
        m1, m2 = np.zeros_like(m1), np.zeros_like(m2)
    ss = (1.0 * inv if gate else np.where(inv > 0, 0.005, 0.0)).astype(np.float32)
    es = ((0.1 if gate else 1.0) * inv).astype(np.float32)
    kw = dict(dh=grad, x=x) if gate else dict(grad=grad)
    if not epoch0:
        kw.update(hard=hard, size_scale=ss, ent_scale=es)
    want = X.host_mask_step(logit, m1, m2, blk, t, num_blocks=B, lr=LR, **kw)

    def run():
        put = lambda a: _place(a, layout, ld, device)  # noqa: E731
        d = dict(mask=put(logit), m1=put(m1), m2=put(m2), status=torch.zeros(1, dtype=torch.int32, device=device))
        args = dict(dh=put(grad), x=put(x), h=put(np.zeros_like(x))) if gate else dict(grad=put(grad))
        if epoch0:
            args["hard_out"] = put(np.full(shape, 7, dtype=np.uint8))
        else:
            args.update(hard=put(hard), size_scale=torch.from_numpy(ss).to(device), ent_scale=torch.from_numpy(es).to(device))
        X.mask_step(d["mask"], d["m1"], d["m2"], torch.from_numpy(blk).to(device), B, t, d["status"], lr=LR, **args)
        d.update(args)
        return d

    got, again = run(), run()
    assert int(got["status"].item()) == 0
    tag = f"K16 {'gate' if gate else 'plain'} {shape} ld {ld} {layout} epoch0={epoch0} B={B}"
    for name, key in (("mask", "mask"), ("exp_avg", "m1"), ("exp_avg_sq", "m2")) + ((("h", "h"),) if gate else ()):
        g = got[key].cpu().numpy()
        err = rel_l2(g, want[name])
        print(f"{tag} {name}: rel L2 {err:.2e}" + (f", max abs {np.abs(g - want[name]).max():.2e}" if name == "mask" else ""))
        assert err <= 1e-5, (tag, name)
        assert torch.equal(got[key], again[key]), (tag, name, "not bitwise reproducible")
    assert float(np.abs(got["mask"].cpu().numpy() - want["mask"]).max()) <= 1e-6, tag
    if epoch0:
        assert np.array_equal(got["hard_out"].cpu().numpy() != 0, want["hard_out"]), tag
        assert torch.equal(got["hard_out"], again["hard_out"])


@pytest.mark.parametrize("n", [1, 3, 64, 257, 1025])
@pytest.mark.parametrize("layout", ["contiguous", "offset"])
def test_mask_step_plain(device, n, layout):
    for epoch0 in (True, False):
        for B in (1, 3):
            _check_step(device, (n,), 0, layout, epoch0, B, gate=False)


@pytest.mark.parametrize("rows,F,ld", [(1, 1, 1), (5, 3, 4), (130, 166, 168), (130, 167, 168), (70, 9, 12), (257, 4, 4)])
@pytest.mark.parametrize("layout", ["contiguous", "sliced", "offset"])
def test_mask_step_gate(device, rows, F, ld, layout):
    for epoch0 in (True, False):
        for B in (1, 3):
            _check_step(device, (rows, F), ld, layout, epoch0, B, gate=True)


def test_mask_step_bad_block_and_gate_only(device):
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd import explain as X

    logit, grad, x, m1, m2, hard, blk, inv = _inputs((40, 6), 3, seed=1)
    blk[3], blk[20] = 3, -1
    d = lambda a: torch.from_numpy(a.copy()).to(device)  # noqa: E731
    mask, a1, a2, h, st = d(logit), d(m1), d(m2), torch.full((40, 6), 5.0, device=device), torch.zeros(1, dtype=torch.int32, device=device)
    X.mask_step(mask, a1, a2, d(blk), 3, 2, st, dh=d(grad), x=d(x), h=h, hard=d(hard), size_scale=d(inv), ent_scale=d(inv))
    assert int(st.item()) == _lib.EXPLAIN_STATUS_BLOCK
    for r in (3, 20):  # untouched, h included
        assert torch.equal(mask[r].cpu(), torch.from_numpy(logit[r])) and torch.equal(a1[r].cpu(), torch.from_numpy(m1[r]))
        assert bool((h[r] == 5.0).all())
    assert not torch.equal(mask[4].cpu(), torch.from_numpy(logit[4])) and not bool((h[4] == 5.0).any())
    # plain form: a bad element inside a 16-byte group leaves only itself untouched
    n = 64
    lg, gr, _, b1, b2, hd, bk, iv = _inputs((n,), 1, seed=2)
    bk[5] = 9
    pm, st2 = d(lg), torch.zeros(1, dtype=torch.int32, device=device)
    X.mask_step(pm, d(b1), d(b2), d(bk), 1, 4, st2, grad=d(np.ones(n, dtype=np.float32)), hard=d(hd), size_scale=d(iv), ent_scale=d(iv))
    assert int(st2.item()) == _lib.EXPLAIN_STATUS_BLOCK
    changed = (pm.cpu() != torch.from_numpy(lg)).numpy()
    assert not changed[5] and changed[np.arange(n) != 5].all()
    # t = 0: only the gate, the logits stay
    st3 = torch.zeros(1, dtype=torch.int32, device=device)
    mask0, h0 = d(logit), torch.zeros((40, 6), device=device)
    X.mask_step(mask0, a1, a2, d(np.zeros(40, dtype=np.int32)), 1, 0, st3, x=d(x), h=h0)
    assert torch.equal(mask0.cpu(), torch.from_numpy(logit)) and int(st3.item()) == 0
    assert rel_l2(h0.cpu().numpy(), x.astype(np.float64) / (1.0 + np.exp(-logit.astype(np.float64)))) <= 1e-5
    with pytest.raises(ValueError):
        X.mask_step(mask0, a1, a2, d(np.zeros(40, dtype=np.int32)), 0, 1, st3, dh=d(grad), x=d(x), hard_out=d(hard))


# ----------------------------------------------------------------------------- the search
def _model(arch, device, params=None, **kw):
    from elliptic_gnn_project_amd.gnn import GATNet, GCNNet, SAGENet, SAGEResBNNet

    cfg = dict(hidden_dim=16, layers=2, dropout=0.0)
    cfg.update(kw)
    in_dim = cfg.pop("in_dim", 8)
    m = {"sage": lambda: SAGENet(in_dim, **cfg), "gcn": lambda: GCNNet(in_dim, **cfg),
         "gat": lambda: GATNet(in_dim, heads=R.HEADS, **cfg), "sage_resbn": lambda: SAGEResBNNet(in_dim, **cfg)}[arch]()
    if params is not None:
        m.load_state_dict(params)
    return m.to(device).eval()


def _data(x, ei, device):
    from elliptic_gnn_project_amd.dataset_elliptic import GraphData

    return GraphData(x=x.to(device), edge_index=ei.to(device))


@pytest.mark.parametrize("arch", ["sage", "gcn", "gat"])
def test_end_to_end_against_the_f64_restatement(device, arch):
    from elliptic_gnn_project_amd.explain import explain_nodes

    params, x, ei, node, (ref_M, ref_m, hard_M, hard_m) = R.case(arch, 0)
    model = _model(arch, device, params)
    ex = explain_nodes(model, _data(x, ei, device), [node], epochs=20, lr=LR, seed=0)[0]
    assert ex.node_id == node and int(ex.n_id[0]) == node
    nm, em = ex.to_full(x.size(0), ei.size(1))
    full_hM = torch.zeros(x.shape, dtype=torch.bool).index_put_((ex.n_id.cpu(),), ex.node_hard.cpu())
    full_hm = torch.zeros(ei.size(1), dtype=torch.bool).index_put_((ex.e_id.cpu(),), ex.edge_hard.cpu())
    dM = float((nm.cpu().double() - ref_M).abs().max())
    dm = float((em.cpu().double() - ref_m).abs().max())
    print(f"explain {arch}: max abs vs f64 {dM:.2e} (features) {dm:.2e} (edges); hard {int(full_hM.sum())} / {int(full_hm.sum())}")
    assert torch.equal(full_hM, hard_M) and torch.equal(full_hm, hard_m)
    assert dM <= 1e-5 and dm <= 1e-5


SUB_ARCHS = ["sage", "gcn", "gat", "sage_resbn", "sage_resbn_time"]


def _sub_case(arch, device):
    torch.manual_seed(7)
    ei = R.sparse_graph(0)
    x = torch.randn(80, 8, generator=torch.Generator().manual_seed(8))
    t_idx = None
    if arch == "sage_resbn_time":
        model = _model("sage_resbn", device, time_embed_dim=4, time_embed_type="learned", max_timestep=10)
        t_idx = (torch.arange(80) % 10 + 1).to(device)
    else:
        model = _model(arch, device)
    if arch.startswith("sage_resbn"):  # eval-mode BatchNorm with running statistics that are not the identity
        with torch.no_grad():
            for bn in model.bns:
                bn.running_mean.normal_(0, 0.2)
                bn.running_var.uniform_(0.5, 1.5)
    return model, _data(x, ei, device), t_idx


@pytest.mark.parametrize("arch", SUB_ARCHS)
def test_subgraph_run_equals_full_graph_run(device, arch):
    from elliptic_gnn_project_amd.explain import explain_full_graph, explain_nodes

    model, data, t_idx = _sub_case(arch, device)
    node = 24  # the end of the chain 20 -> ... -> 24 of sparse_graph
    sub = explain_nodes(model, data, [node], epochs=20, lr=LR, seed=3, t_idx=t_idx)[0]
    full = explain_full_graph(model, data, node, epochs=20, lr=LR, seed=3, t_idx=t_idx, fused_step=False)
    N, E = data.x.size(0), data.edge_index.size(1)
    assert 1 < sub.n_id.numel() < N and 0 < sub.e_id.numel() < E  # a strict subgraph
    dM = float((sub.node_mask - full.node_mask[sub.n_id]).abs().max())
    dm = float((sub.edge_mask - full.edge_mask[sub.e_id]).abs().max())
    print(f"subgraph vs full graph {arch}: {sub.n_id.numel()}/{N} rows, {sub.e_id.numel()}/{E} edges, max abs {dM:.2e} / {dm:.2e}")
    assert dM <= 1e-5 and dm <= 1e-5
    nm, em = sub.to_full(N, E)
    outside_n = torch.ones(N, dtype=torch.bool, device=device).index_fill_(0, sub.n_id, False)
    outside_e = torch.ones(E, dtype=torch.bool, device=device).index_fill_(0, sub.e_id, False)
    assert float(full.node_mask[outside_n].abs().max()) == 0.0 and float(full.edge_mask[outside_e].abs().max()) == 0.0
    assert float((nm - full.node_mask).abs().max()) <= 1e-5 and float((em - full.edge_mask).abs().max()) <= 1e-5
    assert bool(sub.node_hard.any()) and bool(sub.edge_hard.any())
    assert sub.target == full.target and sub.probability_illicit == pytest.approx(full.probability_illicit, abs=1e-6)


@pytest.mark.parametrize("arch", ["sage", "gcn", "gat"])
def test_batch_equals_single_runs_and_fused_equals_torch(device, arch):
    from elliptic_gnn_project_amd.explain import explain_nodes

    model, data, _ = _sub_case(arch, device)
    nodes = [24, 23, 79]  # 23 and 24 share neighbours; 79 is isolated
    batch = explain_nodes(model, data, nodes, epochs=20, lr=LR, seed=1)
    torch_step = explain_nodes(model, data, nodes, epochs=20, lr=LR, seed=1, fused_step=False)
    split = explain_nodes(model, data, nodes, epochs=20, lr=LR, seed=1, max_rows=1)  # one target per run
    assert set(batch[0].n_id.tolist()) & set(batch[1].n_id.tolist())
    for b, v in zip(batch, nodes):
        one = explain_nodes(model, data, [v], epochs=20, lr=LR, seed=1)[0]
        for other, what in ((one, "single"), (torch_step[nodes.index(v)], "torch step"), (split[nodes.index(v)], "max_rows")):
            assert torch.equal(b.n_id, other.n_id) and torch.equal(b.e_id, other.e_id)
            dM = float((b.node_mask - other.node_mask).abs().max())
            dm = float((b.edge_mask - other.edge_mask).abs().max()) if b.e_id.numel() else 0.0
            print(f"batch vs {what} {arch} node {v}: max abs {dM:.2e} / {dm:.2e}")
            assert dM <= 1e-5 and dm <= 1e-5, (what, v)
            assert torch.equal(b.node_hard, other.node_hard) and torch.equal(b.edge_hard, other.edge_hard)
    iso = batch[2]
    assert iso.n_id.tolist() == [79] and iso.e_id.numel() == 0 and iso.edge_mask.numel() == 0
    assert bool(torch.isfinite(iso.node_mask).all()) and not bool(iso.edge_hard.any())
    assert all(bool(torch.isfinite(b.node_mask).all()) and bool(torch.isfinite(b.edge_mask).all()) for b in batch)


def test_model_is_left_as_it_was(device, monkeypatch):
    from elliptic_gnn_project_amd import explain as X

    model, data, _ = _sub_case("sage", device)
    with torch.no_grad():
        before = model(data.x, data.edge_index)
    X.explain_nodes(model, data, [24], epochs=3)
    assert not any(getattr(c, "explain", False) or c._edge_mask is not None for c in model.convs)
    assert all(p.grad is None for p in model.parameters())
    with torch.no_grad():
        assert torch.equal(model(data.x, data.edge_index), before)
    calls = []

    def boom(*a, **k):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("boom")
        return real(*a, **k)

    real = X.mask_step
    monkeypatch.setattr(X, "mask_step", boom)
    with pytest.raises(RuntimeError, match="boom"):
        X.explain_nodes(model, data, [24], epochs=3)
    assert not any(getattr(c, "explain", False) or c._edge_mask is not None for c in model.convs)
    with torch.no_grad():
        assert torch.equal(model(data.x, data.edge_index), before)
    model.train()
    with pytest.raises(ValueError, match="eval"):
        X.explain_nodes(model, data, [24], epochs=1)


def test_cli_on_a_tiny_run(device, tmp_path, capsys):
    from elliptic_gnn_project_amd import explain as X
    from elliptic_gnn_project_amd.robustness import Run
    from elliptic_gnn_project_amd.train_gnn import main as train_main

    cfg = dict(run_name="xp", output_root=str(tmp_path), arch="sage", hidden_dim=16, layers=2, dropout=0.2, lr=0.01,
               weight_decay=1e-4, max_epochs=2, patience=10, grad_clip=1.0, amp=False, symmetrize_edges=True,
               use_time_scalar=True, train_window_k=10, calibrate_temperature=True, topk=50,
               processed_dir=str(tmp_path / "none"), synthetic=dict(num_nodes=3000, num_edges=4500, seed=5))
    train_main(cfg)
    run_dir = tmp_path / "gnn" / "xp"
    keys = ["node_id", "selection", "probability_illicit", "feature_importance", "edge_importance"]
    X.main(["gnn", "--run_dir", str(run_dir), "--epochs", "5"])
    one = json.loads((run_dir / "gnn_explainer_importance.json").read_text())
    assert list(one) == keys and one["selection"]["selection"].startswith("auto_")
    X.main(["gnn", "--run_dir", str(run_dir), "--epochs", "5", "--top", "3"])
    many = json.loads((run_dir / "gnn_explainer_importance_batch.json").read_text())
    assert isinstance(many, list) and 1 <= len(many) <= 3 and all(list(r) == keys for r in many)
    r = Run(run_dir)
    with torch.no_grad():
        probs = torch.softmax(r.model(r.data.x, r.data.edge_index, r.t_idx).float(), dim=-1)[:, 1]
    ei = r.data.edge_index.cpu()
    for rec in [one] + many:
        assert rec["probability_illicit"] == float(probs[rec["node_id"]])
        feats = rec["feature_importance"]
        assert len(feats) == 20 and all(f["importance"] >= 0 for f in feats)
        assert [f["importance"] for f in feats] == sorted((f["importance"] for f in feats), reverse=True)
        assert all(f["feature"] == "time_scalar" or f["feature"].startswith("f") for f in feats)
        for e in rec["edge_importance"]:
            assert bool(((ei[0] == e["source"]) & (ei[1] == e["target"])).any()) and 0 < e["importance"] < 1
    assert [r["node_id"] for r in many] == [v for v, _ in X.pick_nodes(run_dir, top=3)]
