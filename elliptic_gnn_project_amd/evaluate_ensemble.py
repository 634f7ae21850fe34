"""Ensemble two finished runs into a complete run directory (src/analysis/evaluate_ensemble.py, same CLI
and files).

    python -m elliptic_gnn_project_amd.evaluate_ensemble --run_a outputs/gnn/a --run_b outputs/gnn/b \
        [--out_dir DIR] [--mode {prob,logit}] [--precision_target 0.0] [--topk 100]

Run A's validation and test scores are joined onto run B's node order by node id, averaged with run B's
(probabilities, or logits in the closed form of rank_metrics.ensemble_pair), the decision threshold is
chosen on the validation ensemble and the test record is written as train_gnn.main writes a run:
``scores_{val,test}.npy`` (f32), ``y_*``, ``node_idx_*``, ``timestep_*``, ``metrics.json`` and a four-line
``config_used.yaml`` — so eval_by_time, workload_curves, calibration_plots and bootstrap_compare accept
the output directory.  Join, ensemble, threshold and record run on the GPU (rank_metrics, libgnnmp K14 /
K17 / K19) when one is present, else in numpy with the same arithmetic.  Two runs only, as the reference.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import rank_metrics
from .eval_by_time import on_device, pick_device

RECALL_PRECISION = 0.90  # the reference's _metrics_for_test hard-codes train_gnn's default


def load_run(run_dir: Path) -> Dict[str, np.ndarray]:
    """scores / y / node_idx / timestep (when present) of both splits, keyed ``<name>_<split>``."""
    run_dir = Path(run_dir)
    run = {}
    for split in ("val", "test"):
        for name in ("scores", "y", "node_idx"):
            run[f"{name}_{split}"] = np.load(run_dir / f"{name}_{split}.npy")
        if (run_dir / f"timestep_{split}.npy").exists():
            run[f"timestep_{split}"] = np.load(run_dir / f"timestep_{split}.npy")
    return run


def _ensemble_split(run_a: Dict, run_b: Dict, split: str, mode: str, device: torch.device):
    """(ensemble scores, labels == 1 as int64) of one split in run B's order, on ``device``."""
    what = split.upper()
    perm = rank_metrics.join_by_id(on_device(run_b[f"node_idx_{split}"].astype(np.int64), device),
                                   on_device(run_a[f"node_idx_{split}"].astype(np.int64), device), what)
    ya, yb = np.asarray(run_a[f"y_{split}"]).astype(np.int64), np.asarray(run_b[f"y_{split}"]).astype(np.int64)
    if device.type == "cpu":
        same = np.array_equal(ya[perm.numpy()], yb)
    else:
        same = torch.equal(torch.from_numpy(ya).to(device)[perm.long()], torch.from_numpy(yb).to(device))
    if not same:
        raise RuntimeError(f"{what} labels differ after alignment.")
    scores = rank_metrics.ensemble_pair(on_device(np.asarray(run_a[f"scores_{split}"], dtype=np.float32), device),
                                        on_device(np.asarray(run_b[f"scores_{split}"], dtype=np.float32), device),
                                        mode, perm)
    return scores, on_device(yb, device)


def ensemble(run_a: Dict, run_b: Dict, mode: str = "logit", precision_target: float = 0.0, topk: int = 100,
             device: Optional[torch.device] = None) -> Tuple[Dict[str, np.ndarray], Dict]:
    """(the ensemble's arrays keyed as ``load_run`` keys them, its test metrics) for two loaded runs."""
    from .train_gnn import _by_time_summary

    device = pick_device(device)
    pv, yv = _ensemble_split(run_a, run_b, "val", mode, device)
    pt, yt = _ensemble_split(run_a, run_b, "test", mode, device)
    thr, _ = rank_metrics.select_threshold(pv, yv, on_device(np.ones(len(yv), dtype=bool), device), precision_target)
    everything = on_device(np.ones(len(yt), dtype=bool), device)
    metrics = rank_metrics.evaluation_record(pt, yt, everything, thr, int(topk), RECALL_PRECISION, device_order=True)
    ts = run_b.get("timestep_test")
    if ts is not None and ts.size > 0:
        _, ap, _ = rank_metrics.average_precision_by_group(pt, yt, on_device(np.asarray(ts).astype(np.int64), device),
                                                           mask=everything, device_order=True)
        _by_time_summary(metrics, [float(v) for v in ap.cpu().tolist()])
    out = {k: v for k, v in run_b.items() if not k.startswith("scores_")}
    out["scores_val"] = pv.cpu().numpy().astype(np.float32)
    out["scores_test"] = pt.cpu().numpy().astype(np.float32)
    return out, metrics


def main(argv=None, device: Optional[torch.device] = None) -> Dict:
    ap = argparse.ArgumentParser(description="Ensemble two trained runs and write metrics/artifacts.")
    ap.add_argument("--run_a", type=Path, required=True)
    ap.add_argument("--run_b", type=Path, required=True)
    ap.add_argument("--out_dir", type=Path, default=None,
                    help="Where to write ensemble outputs (default: <run_b>/ensemble)")
    ap.add_argument("--mode", type=str, default="logit", choices=["prob", "logit"],
                    help="Average probabilities or logits")
    ap.add_argument("--precision_target", type=float, default=0.0,
                    help="If >0, pick threshold to hit this precision on val")
    ap.add_argument("--topk", type=int, default=100)
    args = ap.parse_args(argv)

    run_a, run_b = args.run_a.resolve(), args.run_b.resolve()
    out_dir = (args.out_dir if args.out_dir is not None else run_b / "ensemble").resolve()
    arrays, metrics = ensemble(load_run(run_a), load_run(run_b), args.mode, args.precision_target, args.topk, device)
    metrics["ensemble_sources"] = {"run_a": str(run_a), "run_b": str(run_b), "mode": args.mode}
    best = []
    for src in (run_a, run_b):
        try:
            with open(src / "metrics.json", "r", encoding="utf-8") as fh:
                best.append(float(json.load(fh)["best_val_pr_auc"]))
        except (OSError, KeyError, TypeError, ValueError):
            pass
    if best:
        metrics["best_val_pr_auc"] = max(best)

    out_dir.mkdir(parents=True, exist_ok=True)
    for name, value in arrays.items():
        np.save(out_dir / f"{name}.npy", value)
    with open(out_dir / "metrics.json", "w", encoding="utf-8") as fh:
        json.dump(metrics, fh, indent=2)
    echo = {"run_name": f"ensemble_of_{run_a.name}_and_{run_b.name}", "precision_target": float(args.precision_target),
            "topk": int(args.topk), "ensemble_mode": args.mode}
    (out_dir / "config_used.yaml").write_text("\n".join(f"{k}: {v}" for k, v in echo.items()), encoding="utf-8")
    print(json.dumps(metrics, indent=2))
    print(f"[DONE] Ensemble written to: {out_dir}")
    return metrics


if __name__ == "__main__":
    main()
