"""GPU end to end: the robustness tool (elliptic_gnn_project_amd/robustness.py, the reference's
src/analysis/robustness.py) on runs trained by train_gnn.main on the seeded synthetic graph of
tests/test_gpu_train_main.py.

Unperturbed, the tool recomputes metrics.json (same kernels, same LBFGS, same inputs); a perturbed
trial is checked for its file, key set, counts, repeatability, host-recomputed metrics and against
the CPU oracle on mirror-perturbed inputs; a sweep against the single runs it is made of.
"""
import json
import math

import numpy as np
import pytest
import torch

from oracle import pyg_ref

pytestmark = pytest.mark.gpu

ARCHS = ("sage", "gat", "sage_resbn")
KEYS = {"pr_auc_illicit", "roc_auc", "f1_illicit_at_thr", "threshold", "precision_at_k", "recall_at_precision", "ece",
        "n_test", "drop_frac_requested", "drop_frac_effective", "edges_dropped", "n_edges_original",
        "n_edges_after_drop", "noise_std", "temperature", "seed"}
SHARED = ("pr_auc_illicit", "roc_auc", "f1_illicit_at_thr", "threshold", "precision_at_k", "recall_at_precision",
          "ece", "n_test")
_RUNS = {}


@pytest.fixture(scope="module")
def trained(device, tmp_path_factory):
    """arch -> (run directory, config): trained once per module, 3 epochs."""
    from elliptic_gnn_project_amd.train_gnn import main

    def get(arch):
        if arch not in _RUNS:
            root = tmp_path_factory.mktemp(f"rob_{arch}")
            cfg = dict(run_name=f"rob_{arch}", output_root=str(root), arch=arch, hidden_dim=32, layers=2, heads=4,
                       dropout=0.2, lr=0.005, weight_decay=1e-4, max_epochs=3, patience=10, grad_clip=1.0, amp=False,
                       symmetrize_edges=True, use_time_scalar=True, train_window_k=10, calibrate_temperature=True,
                       topk=50, synthetic=dict(num_nodes=8000, num_edges=12000, seed=5))
            if arch == "sage_resbn":
                cfg.update(time_embed_dim=2, time_embed_type="learned", use_time_scalar=False, layers=3)
            main(cfg)
            _RUNS[arch] = (root / "gnn" / cfg["run_name"], cfg)
        return _RUNS[arch]

    yield get
    _RUNS.clear()


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("arch", ARCHS)
def test_unperturbed_run_reproduces_metrics_json(trained, arch):
    from elliptic_gnn_project_amd import robustness as R

    run_dir, _ = trained(arch)
    base = json.loads((run_dir / "metrics.json").read_text())
    rec = R.run(run_dir, 0.0, 0.0, 42)
    for k in SHARED:
        assert rec[k] == pytest.approx(base[k], abs=1e-12, nan_ok=True), k
    assert rec["edges_dropped"] == 0 and rec["n_edges_after_drop"] == rec["n_edges_original"]
    assert rec["drop_frac_effective"] == 0.0 and rec["noise_std"] == 0.0 and rec["seed"] == 42
    assert (run_dir / "robustness_drop0.0_noise0.0.json").exists()


@pytest.mark.parametrize("arch", ARCHS)
def test_perturbed_run(trained, arch):
    from elliptic_gnn_project_amd import robustness as R
    from elliptic_gnn_project_amd.train_gnn import _metrics

    run_dir, cfg = trained(arch)
    rec = R.run(run_dir, 0.1, 0.01, 42)
    path = run_dir / "robustness_drop0.1_noise0.01.json"
    text = path.read_text()
    assert set(rec) == KEYS and set(json.loads(text)) == KEYS
    E = rec["n_edges_original"]
    assert E == 2 * 12000  # symmetrize_edges
    assert rec["edges_dropped"] == round(0.1 * E) and rec["n_edges_after_drop"] == E - rec["edges_dropped"]
    assert rec["drop_frac_requested"] == 0.1 and rec["drop_frac_effective"] == rec["edges_dropped"] / E
    assert rec["noise_std"] == 0.01 and rec["seed"] == 42 and rec["temperature"] > 0
    assert rec["threshold"] == json.loads((run_dir / "metrics.json").read_text())["threshold"]
    rec2 = R.run(run_dir, 0.1, 0.01, 42)
    assert path.read_text() == text and all(_same(rec[k], rec2[k]) for k in KEYS)
    # the metrics are those of the trial's probabilities, recomputed on the host
    r = R.Run(run_dir)
    det = {}
    rec3 = r.trial(0.1, 0.01, 42, details=det)
    y = r.data.y.cpu().numpy()
    tm = r.data.test_mask.cpu().numpy().astype(bool)
    want = _metrics((y[tm] == 1).astype(int), det["probs"][tm], rec["threshold"], cfg)
    for k, v in want.items():
        assert _same(rec[k], v) and _same(rec3[k], v), k
    # another seed is another trial
    assert not torch.equal(det["x"], R.add_noise(r.data.x, 0.01, 43))


@pytest.mark.parametrize("arch", ARCHS)
def test_trial_matches_the_cpu_oracle(trained, arch):
    """The trial's logits on the GPU against the CPU oracle on inputs perturbed by the host mirror, at
    the project's 1e-5 bar; the kept edge_index and the count are identical."""
    from elliptic_gnn_project_amd import robustness as R

    run_dir, cfg = trained(arch)
    r = R.Run(run_dir)
    det = {}
    rec = r.trial(0.1, 0.01, 42, details=det)
    ei_cpu, n_cpu = R.drop_edges(r.data.edge_index.cpu(), 0.1, 42)
    assert n_cpu == rec["edges_dropped"] and torch.equal(det["edge_index"].cpu(), ei_cpu)
    x_cpu = R.add_noise(r.data.x.cpu(), 0.01, 42)  # (the kernel against this mirror: tests/test_gpu_perturb.py)
    params = {k: v.detach().cpu() for k, v in r.model.state_dict().items()}
    kw = dict(layers=cfg["layers"])
    if arch == "gat":
        kw["heads"] = cfg["heads"]
    if arch == "sage_resbn":
        kw.update(t_idx=r.data.timestep.cpu(), time_embed_dim=2, time_embed_type="learned",
                  max_timestep=r.model.max_timestep,
                  bn_state={k: v.clone() for k, v in params.items() if "running" in k})
    ref = pyg_ref.model_forward(arch, params, x_cpu, ei_cpu, **kw)
    torch.testing.assert_close(det["logits"].cpu(), ref, rtol=1e-5, atol=1e-5)


DROPS, NOISES, SWEEP_SEEDS = (0.0, 0.1), (0.0, 0.05), (0, 1)
_SWEEPS = {}


@pytest.fixture(scope="module")
def swept(trained):
    """arch -> the sweep's result: one sweep per arch and module."""
    from elliptic_gnn_project_amd import robustness as R

    def get(arch):
        if arch not in _SWEEPS:
            _SWEEPS[arch] = R.sweep(trained(arch)[0], DROPS, NOISES, SWEEP_SEEDS)
        return _SWEEPS[arch]

    yield get
    _SWEEPS.clear()


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
@pytest.mark.parametrize("arch", ARCHS)
def test_sweep_records_are_the_single_runs(trained, swept, arch, seed):
    """Eight records, one per (drop_frac, noise_std, seed); each equals the single run of its trial (the
    runs of one seed per case: a trial's time is its temperature fit, profiles/robustness.json)."""
    from elliptic_gnn_project_amd import robustness as R

    run_dir, _ = trained(arch)
    out = swept(arch)
    recs = out["records"]
    assert len(recs) == 8
    assert {(r["drop_frac_requested"], r["noise_std"], r["seed"]) for r in recs} == \
        {(d, n, s) for d in DROPS for n in NOISES for s in SWEEP_SEEDS}
    mine = [r for r in recs if r["seed"] == seed]
    assert len(mine) == 4
    for rec in mine:
        key = (rec["drop_frac_requested"], rec["noise_std"], rec["seed"])
        single = R.run(run_dir, *key)
        assert set(rec) == KEYS
        for k in KEYS:
            assert _same(rec[k], single[k]), (key, k)


@pytest.mark.parametrize("arch", ARCHS)
def test_sweep_summary(trained, swept, arch):
    """Per (drop_frac, noise_std): mean and sample standard deviation over the seeds of the records (which
    test_sweep_records_are_the_single_runs ties to the single runs), as returned and as written."""
    from elliptic_gnn_project_amd import robustness as R

    run_dir, _ = trained(arch)
    out = swept(arch)
    assert json.loads((run_dir / "robustness_sweep.json").read_text())["summary"] == out["summary"]
    assert [(c["drop_frac"], c["noise_std"]) for c in out["summary"]] == [(d, n) for d in DROPS for n in NOISES]
    for cell in out["summary"]:
        vals = [r for r in out["records"]
                if (r["drop_frac_requested"], r["noise_std"]) == (cell["drop_frac"], cell["noise_std"])]
        assert cell["n_seeds"] == len(vals) == 2
        for k in R.SUMMARY_KEYS:
            a = np.array([v[k] for v in vals], dtype=np.float64)
            assert cell["mean"][k] == pytest.approx(float(a.mean()), abs=1e-15, nan_ok=True), k
            assert cell["std"][k] == pytest.approx(float(a.std(ddof=1)), abs=1e-15, nan_ok=True), k
