"""GPU end to end: the hub ablation tool (elliptic_gnn_project_amd/hub_ablation.py, the reference's
src/analysis/hub_ablation.py) on runs trained by train_gnn.main with ``ablate_hubs_frac = 0.005`` on the
seeded synthetic graph of tests/test_gpu_robustness.py.

At 0.005 the graph's hub boundary is untied (h = 40), so the tool removes main's edges in main's order
and recomputes ``metrics_hub_removed.json`` with the same kernels from the same inputs; at 0.01 (h = 80,
tied) it is checked against the host mirror, the CPU oracle and host-recomputed metrics; a sweep against
the single runs it is made of; the device evaluation against rank_metrics.evaluation_record.
"""
import json
import math

import pytest
import torch

from oracle import pyg_ref

pytestmark = pytest.mark.gpu

ARCHS = ("sage", "gat", "sage_resbn")
SHARED = ("pr_auc_illicit", "roc_auc", "f1_illicit_at_thr", "threshold", "precision_at_k", "recall_at_precision",
          "ece", "n_test")
KEYS = set(SHARED) | {"n_hubs", "hub_fraction", "n_edges_remaining"}  # the reference's (hub_ablation.py:186-200)
SWEEP_FRACS = (0.0005625, 0.005, 0.01)  # h = 4, 40, 80 of N = 8000
_RUNS, _SINGLE = {}, {}


@pytest.fixture(scope="module")
def trained(device, tmp_path_factory):
    """arch -> (run directory, config): trained once per module, 3 epochs, with main's own hub ablation."""
    from elliptic_gnn_project_amd.train_gnn import main

    def get(arch):
        if arch not in _RUNS:
            root = tmp_path_factory.mktemp(f"hub_{arch}")
            cfg = dict(run_name=f"hub_{arch}", output_root=str(root), arch=arch, hidden_dim=32, layers=2, heads=4,
                       dropout=0.2, lr=0.005, weight_decay=1e-4, max_epochs=3, patience=10, grad_clip=1.0, amp=False,
                       symmetrize_edges=True, use_time_scalar=True, train_window_k=10, calibrate_temperature=True,
                       topk=50, synthetic=dict(num_nodes=8000, num_edges=12000, seed=5), ablate_hubs_frac=0.005)
            if arch == "sage_resbn":
                cfg.update(time_embed_dim=2, time_embed_type="learned", use_time_scalar=False, layers=3)
            main(cfg)
            _RUNS[arch] = (root / "gnn" / cfg["run_name"], cfg)
        return _RUNS[arch]

    yield get
    _RUNS.clear()
    _SINGLE.clear()


def _single(trained, arch, frac):
    """(record, details) of hub_ablation.run for one fraction: run once per module."""
    from elliptic_gnn_project_amd import hub_ablation as H

    if (arch, frac) not in _SINGLE:
        det = {}
        _SINGLE[arch, frac] = (H.run(trained(arch)[0], frac, details=det), det)
    return _SINGLE[arch, frac]


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("arch", ARCHS)
def test_untied_fraction_reproduces_mains_hub_metrics(trained, arch):
    run_dir, _ = trained(arch)
    base = json.loads((run_dir / "metrics_hub_removed.json").read_text())
    rec, _ = _single(trained, arch, 0.005)
    assert set(rec) == KEYS == set(base)
    for k in SHARED:
        assert rec[k] == pytest.approx(base[k], abs=1e-12, nan_ok=True), k
    assert rec["n_hubs"] == base["n_hubs"] == 40 and rec["n_edges_remaining"] == base["n_edges_remaining"]
    assert rec["hub_fraction"] == 0.005
    path = run_dir / "metrics_hub_removed_0p005.json"
    assert path.exists() and json.dumps(json.loads(path.read_text())) == json.dumps(rec)  # (NaN prints as NaN)


@pytest.mark.parametrize("arch", ARCHS)
def test_no_hub_reproduces_metrics_json(trained, arch):
    run_dir, _ = trained(arch)
    base = json.loads((run_dir / "metrics.json").read_text())
    rec, det = _single(trained, arch, 0.0)
    assert set(rec) == KEYS
    for k in SHARED:
        assert rec[k] == pytest.approx(base[k], abs=1e-12, nan_ok=True), k
    assert det["n_hubs"] == 0  # (the threshold above is recomputed from the base probabilities, not read)
    assert rec["n_hubs"] == 0 and rec["n_edges_remaining"] == 2 * 12000 and rec["hub_fraction"] == 0.0
    assert (run_dir / "metrics_hub_removed_0p0.json").exists()


@pytest.mark.parametrize("arch", ARCHS)
def test_tied_fraction_against_mirror_oracle_and_host_metrics(trained, arch):
    """frac = 0.01 (h = 80, a tied boundary): the ablated edge_index is the host mirror's, the logits match
    the CPU oracle on it at the project's 1e-5 bar, and the record is _metrics of the returned probabilities."""
    from elliptic_gnn_project_amd import hub_ablation as H, robustness as R
    from elliptic_gnn_project_amd.train_gnn import _metrics

    run_dir, cfg = trained(arch)
    rec, det = _single(trained, arch, 0.01)
    r = R.Run(run_dir)
    N = int(r.data.x.size(0))
    ei_cpu, n_cpu = H.ablate_hubs(r.data.edge_index.cpu(), N, 0.01)
    assert n_cpu == rec["n_hubs"] == 80 and H.HubRanking(r.data.edge_index.cpu(), N).boundary_tied(80)
    assert torch.equal(det["edge_index"].cpu(), ei_cpu) and rec["n_edges_remaining"] == ei_cpu.size(1)
    params = {k: v.detach().cpu() for k, v in r.model.state_dict().items()}
    kw = dict(layers=cfg["layers"])
    if arch == "gat":
        kw["heads"] = cfg["heads"]
    if arch == "sage_resbn":
        kw.update(t_idx=r.data.timestep.cpu(), time_embed_dim=2, time_embed_type="learned",
                  max_timestep=r.model.max_timestep,
                  bn_state={k: v.clone() for k, v in params.items() if "running" in k})
    ref = pyg_ref.model_forward(arch, params, r.data.x.cpu(), ei_cpu, **kw)
    torch.testing.assert_close(det["logits"].cpu(), ref, rtol=1e-5, atol=1e-5)
    y = r.data.y.cpu().numpy()
    tm = r.data.test_mask.cpu().numpy().astype(bool)
    want = _metrics((y[tm] == 1).astype(int), det["probs"][tm], rec["threshold"], cfg)
    assert set(want) == set(SHARED)
    for k, v in want.items():
        assert _same(rec[k], v), k
    base_thr = json.loads((run_dir / "metrics.json").read_text())["threshold"]
    assert rec["threshold"] == pytest.approx(base_thr, abs=1e-12)


@pytest.mark.parametrize("arch", ARCHS)
def test_sweep_records_are_the_single_runs(trained, arch):
    from elliptic_gnn_project_amd import hub_ablation as H

    run_dir, _ = trained(arch)
    out = H.sweep(run_dir, SWEEP_FRACS)
    assert json.dumps(json.loads((run_dir / "hub_ablation_sweep.json").read_text())) == json.dumps(out)
    assert len(out["records"]) == 3
    assert [rec["boundary_tied"] for rec in out["records"]] == [False, False, True]
    assert [rec["n_hubs"] for rec in out["records"]] == [4, 40, 80]
    for frac, rec in zip(SWEEP_FRACS + (0.0,), out["records"] + [out["base"]]):
        single, _ = _single(trained, arch, frac)
        assert set(rec) == KEYS | {"min_hub_degree", "boundary_tied"}
        for k in KEYS:
            assert _same(rec[k], single[k]), (frac, k)
    assert out["base"]["min_hub_degree"] is None and out["base"]["boundary_tied"] is False
    degs = [rec["min_hub_degree"] for rec in out["records"]]
    assert degs == sorted(degs, reverse=True) and degs[-1] >= 1
    left = [out["base"]["n_edges_remaining"]] + [rec["n_edges_remaining"] for rec in out["records"]]
    assert left == sorted(left, reverse=True) and left[0] == 2 * 12000


@pytest.mark.parametrize("arch", ARCHS)
def test_device_eval_record(trained, arch):
    """Under device_eval the record is rank_metrics.evaluation_record of the same device probabilities
    at the tool's threshold, and run() returns and writes that record."""
    from elliptic_gnn_project_amd import hub_ablation as H, rank_metrics as RM

    run_dir, cfg = trained(arch)
    tool = H.Tool(run_dir, device_eval=True)
    det = {}
    rec = tool.record(0.01, details=det)
    d = tool.run.data
    want = RM.evaluation_record(det["probs_device"], d.y, d.test_mask, tool.threshold, cfg["topk"], 0.90)
    assert set(rec) == KEYS and set(want) == set(SHARED)
    for k, v in want.items():
        assert _same(rec[k], v), k
    assert rec["n_hubs"] == 80 and rec["n_edges_remaining"] == _single(trained, arch, 0.01)[0]["n_edges_remaining"]
    again = H.run(run_dir, 0.01, device_eval=True)
    for k in KEYS:
        assert _same(again[k], rec[k]), k
