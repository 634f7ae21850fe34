"""Feature-only baseline of a run comparison (src/train_baselines.py, same config keys and files):
standardise + logistic regression on the node features alone, optional isotonic / Platt calibration on
the validation split, the decision threshold and ``metrics.json`` as train_gnn.main writes them.

    python -m elliptic_gnn_project_amd.train_baselines --config configs/baseline_lr.yaml

Config keys (the reference's): ``run_name, seed, processed_dir / graph_file / synthetic, model,
calibration {none, isotonic, platt}, C, max_iter, class_weight, train_window_k, use_val_for_thresholds,
precision_target, topk, device``; ``n_jobs`` is accepted and ignored; ``output_root`` as in train_gnn.
``model: xgboost`` is not rebuilt.  ``device: cpu`` (or no GPU) runs the numpy mirrors of
logreg.py / calibrate.py / rank_metrics.py, anything else the kernels (libgnnmp K20, K14, K17).

The fit is the minimiser of sklearn's objective (logreg.py), not lbfgs's stopping point; scores are f32
(the project's score dtype): the f64 probability rounded once, then the calibrator's f64 output rounded
once.  Under ``outputs/baselines/<run_name>/``: ``scores_{val,test}.npy`` (calibrated), ``y_*``,
``node_idx_*``, ``timestep_*``, the uncalibrated ``scores_raw_{val,test}.npy``, ``metrics.json`` (the eight
keys of train_gnn's) and ``model.npz`` (mu, sd, w, b and the calibrator) in place of model.pkl.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict

import numpy as np
import torch
import yaml

from . import calibrate, logreg, rank_metrics
from .dataset_elliptic import prepare_inputs
from .train_gnn import load_data, set_seed

CALIBRATIONS = ("none", "isotonic", "platt")


def pick_device(cfg: Dict) -> torch.device:
    forced = str(cfg.get("device", "auto") or "auto")
    if forced == "cpu":
        return torch.device("cpu")
    if torch.cuda.is_available():
        return torch.device("cuda", torch.cuda.current_device())
    if forced != "auto":
        raise RuntimeError(f"train_baselines: device={forced!r} but no GPU is available")
    return torch.device("cpu")


def fit_calibrator(kind: str, scores, y) -> calibrate.Calibrator:
    if kind == "isotonic":
        return calibrate.fit_isotonic(scores, y)
    if kind == "platt":
        return calibrate.fit_platt(scores, y)
    return calibrate.Calibrator("identity")


def main(cfg: Dict) -> Dict:
    set_seed(cfg.get("seed", 42))
    model_name = cfg["model"]
    if model_name == "xgboost":
        raise NotImplementedError("train_baselines: model 'xgboost' is not rebuilt — gradient-boosted trees have no "
                                  "place in this library (DESIGN.md §7); use model: logistic_regression")
    if model_name != "logistic_regression":
        raise ValueError(f"Unknown baseline model: {model_name}")
    kind = str(cfg.get("calibration", "none") or "none").lower()
    if kind not in CALIBRATIONS:
        raise ValueError(f"train_baselines: calibration {kind!r} (one of {CALIBRATIONS})")
    device = pick_device(cfg)
    outdir = os.path.join(cfg.get("output_root", "outputs"), "baselines", cfg["run_name"])
    os.makedirs(outdir, exist_ok=True)

    # labelled nodes of the temporal split: no time scalar, no symmetrising (get_split_arrays)
    data = prepare_inputs(load_data(cfg), {"train_window_k": cfg.get("train_window_k")})
    idx = {s: getattr(data, f"{s}_idx") for s in ("train", "val", "test")}
    if idx["train"].numel() == 0:
        raise RuntimeError("Train mask is empty; cannot fit the baseline.")
    on_gpu = device.type == "cuda"
    x = data.x.to(device) if on_gpu else data.x.numpy()
    y_all = data.y.to(device) if on_gpu else data.y.numpy()
    rows = {s: (v.to(device) if on_gpu else v.numpy()) for s, v in idx.items()}
    y_of = {s: y_all[rows[s]] for s in rows}

    y_tr = data.y[idx["train"]]
    pos, neg = int((y_tr == 1).sum()), int((y_tr == 0).sum())
    print(f"[BAL] train positives={pos}, negatives={neg}, pos_rate={pos / (pos + neg + 1e-9):.4f}")
    model = logreg.fit(x, y_all, rows["train"], C=float(cfg.get("C", 1.0)), class_weight=cfg.get("class_weight", None),
                       max_iter=int(cfg.get("max_iter", 2000)))
    print(f"[FIT] newton updates={model.iterations}, status={model.status}, F={model.F:.9g}")

    raw = {s: logreg.predict_proba(model, x, rows[s], np.float32) for s in ("val", "test")}
    print(f"[CAL] calibration={kind}")
    cal = fit_calibrator(kind, raw["val"], y_of["val"])
    scores = {s: calibrate.apply_calibrator(cal, raw[s]) for s in ("val", "test")}

    if cfg.get("use_val_for_thresholds", True):
        thr = rank_metrics.select_threshold(scores["val"], y_of["val"], None, cfg.get("precision_target", 0.0))[0]
    else:
        thr = rank_metrics.select_threshold(scores["test"], y_of["test"])[0]
    everything = torch.ones_like(y_of["test"], dtype=torch.bool) if on_gpu else np.ones(len(y_of["test"]), dtype=bool)
    metrics = rank_metrics.evaluation_record(scores["test"], y_of["test"], everything, thr, int(cfg.get("topk", 100)),
                                             float(cfg.get("precision_target", 0.90)))

    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
    ts = data.timestep.numpy()
    for s in ("val", "test"):
        np.save(os.path.join(outdir, f"scores_{s}.npy"), host(scores[s]).astype(np.float32))
        np.save(os.path.join(outdir, f"scores_raw_{s}.npy"), host(raw[s]).astype(np.float32))
        np.save(os.path.join(outdir, f"y_{s}.npy"), host(y_of[s]))
        np.save(os.path.join(outdir, f"node_idx_{s}.npy"), idx[s].numpy())
        np.save(os.path.join(outdir, f"timestep_{s}.npy"), ts[idx[s].numpy()])
    np.savez(os.path.join(outdir, "model.npz"), mu=model.mu, sd=model.sd, w=model.w, b=np.array([model.b]),
             iterations=np.array([model.iterations]), status=np.array([model.status]),
             calibration=np.array(cal.kind), cal_xs=cal.xs, cal_ys=cal.ys, cal_w=np.array([cal.w]),
             cal_b=np.array([cal.b]))
    with open(os.path.join(outdir, "metrics.json"), "w", encoding="utf-8") as fh:
        json.dump(metrics, fh, indent=2)
    print(json.dumps(metrics, indent=2))
    return metrics


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, required=True)
    args = parser.parse_args()
    with open(args.config, "r", encoding="utf-8") as f:
        main(yaml.safe_load(f))
