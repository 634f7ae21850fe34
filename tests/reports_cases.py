"""Inputs shared by tests/test_reports_host.py and tests/test_gpu_reports.py: the reference's golden
vectors (tests/golden/reports_golden.json), run directories built from them, and the bounds the two
files assert for the logit ensemble."""
import json
from pathlib import Path

import numpy as np

from device_eval_cases import ap_tol

# numpy's pairwise f32 mean inside the reference (tests/test_device_eval_host.py:19): 32 roundings of 2^-24
ECE_F32_TOL = 32 * 2.0 ** -24
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "reports_golden.json").read_text())
LO, HI = np.float32(1e-6), np.float32(1.0 - 1e-6)


def f32(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def closed_form_f64(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """sigma((logit a + logit b) / 2) = r / (r + q) in f64 on the f32-clipped inputs."""
    da, db = np.clip(a, LO, HI).astype(np.float64), np.clip(b, LO, HI).astype(np.float64)
    r, q = np.sqrt(da * db), np.sqrt((1.0 - da) * (1.0 - db))
    return r / (r + q)


def check_logit_bounds(ours: np.ndarray, a: np.ndarray, b: np.ndarray, ref: np.ndarray) -> None:
    """Every score within one f32 ulp of the f64 closed form, and no further from it than the reference
    is, up to one ulp: |ours - ref| <= |ref - f64| + 1 ulp."""
    assert ours.dtype == np.float32
    exact = closed_form_f64(a, b)
    ulp = np.spacing(exact.astype(np.float32)).astype(np.float64)
    o, r = ours.astype(np.float64), ref.astype(np.float64)
    print(f"max |ours - f64| {np.abs(o - exact).max():.3g} ({(np.abs(o - exact) / ulp).max():.3g} ulp), "
          f"max |ref - f64| {np.abs(r - exact).max():.3g} ({(np.abs(r - exact) / ulp).max():.3g} ulp)")
    assert (np.abs(o - exact) <= ulp).all()
    assert (np.abs(o - r) <= np.abs(r - exact) + ulp).all()


def check_ensemble_metrics(m: dict) -> None:
    """The ensemble's test record against the reference's of the logit golden."""
    g = GOLDEN["ensemble_logit"]
    want, n = g["metrics"], len(g["test"]["y_b"])
    for key in ("pr_auc_illicit", "roc_auc", "pr_auc_last1", "pr_auc_last3", "pr_auc_last5"):
        print(key, m[key], want[key])
        assert abs(m[key] - want[key]) <= ap_tol(n), key
    assert len(m["test_pr_auc_by_time"]) == len(want["test_pr_auc_by_time"]) == 8
    assert np.abs(np.asarray(m["test_pr_auc_by_time"]) - np.asarray(want["test_pr_auc_by_time"])).max() <= ap_tol(n)
    for key in ("precision_at_k", "f1_illicit_at_thr", "recall_at_precision", "n_test"):
        assert m[key] == want[key], key
    print("threshold", m["threshold"], want["threshold"], "ece", m["ece"], want["ece"], "ref_dev", g["ref_dev"])
    assert abs(m["threshold"] - want["threshold"]) <= g["ref_dev"]
    assert abs(m["ece"] - want["ece"]) <= g["ref_dev"] + ECE_F32_TOL


def ensemble_runs():
    """(run A, run B) of the logit golden as evaluate_ensemble.load_run lays them out."""
    g = GOLDEN["ensemble_logit"]
    run_a, run_b = {}, {}
    for split in ("val", "test"):
        s = g[split]
        run_a.update({f"scores_{split}": f32(s["a"]), f"y_{split}": np.asarray(s["y_a"], dtype=np.int64),
                      f"node_idx_{split}": np.asarray(s["ids_a"], dtype=np.int64)})
        run_b.update({f"scores_{split}": f32(s["b"]), f"y_{split}": np.asarray(s["y_b"], dtype=np.int64),
                      f"node_idx_{split}": np.asarray(s["ids_b"], dtype=np.int64)})
    run_b["timestep_test"] = np.asarray(g["timestep_test"], dtype=np.int64)
    run_b["timestep_val"] = np.full(len(g["val"]["y_b"]), 41, dtype=np.int64)
    return run_a, run_b


def write_run(path: Path, run: dict, metrics: dict) -> Path:
    path.mkdir(parents=True, exist_ok=True)
    for name, value in run.items():
        np.save(path / f"{name}.npy", value)
    (path / "metrics.json").write_text(json.dumps(metrics, indent=2))
    return path


def by_time_run(path: Path, name: str = "ties") -> Path:
    """A run directory holding the test split of one by-time golden case."""
    c = next(c for c in GOLDEN["by_time"] if c["name"] == name)
    run = {"scores_test": f32(c["scores"]), "y_test": np.asarray(c["y"], dtype=np.int64),
           "timestep_test": np.asarray(c["timestep"], dtype=np.int64),
           "node_idx_test": np.arange(len(c["y"]), dtype=np.int64)}
    return write_run(path, run, {"threshold": c["threshold"]})
