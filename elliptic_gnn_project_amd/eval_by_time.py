"""Per-timestep PR-AUC and F1 of a finished run (src/analysis/eval_by_time.py, same CLI and file).

    python -m elliptic_gnn_project_amd.eval_by_time --run_dir outputs/gnn/<run>

Reads ``scores_test.npy`` / ``y_test.npy`` / ``timestep_test.npy`` and the ``threshold`` of
``metrics.json`` as train_gnn.main writes them and writes ``by_time.csv`` (no plot: DESIGN.md §7, every
plotted number is in the file).  One segmented average precision and one counting pass on the GPU
(rank_metrics, libgnnmp K14 / K19) when one is present, else the same arithmetic in numpy.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

from . import rank_metrics

HEADER = "timestep,pr_auc_illicit,f1_illicit_at_thr,n"


def pick_device(device: Optional[torch.device]) -> torch.device:
    if device is None:
        return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(device)


def on_device(a: np.ndarray, device: torch.device):
    """The array as it is for the host path, as a tensor on ``device`` for the device path."""
    return np.ascontiguousarray(a) if device.type == "cpu" else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def by_time(scores: np.ndarray, y: np.ndarray, timestep: np.ndarray, threshold: float,
            device: Optional[torch.device] = None) -> List[Dict]:
    """The reference's rows {timestep, pr_auc_illicit, f1_illicit_at_thr, n}, every test sample scored
    (positives are ``y == 1``).  ``threshold`` is the f32 score metrics.json holds as a JSON double."""
    device = pick_device(device)
    n = len(y)
    everything = on_device(np.ones(n, dtype=bool), device)
    return rank_metrics.by_time_table(on_device(np.asarray(scores, dtype=np.float32), device),
                                      on_device(np.asarray(y).astype(np.int64), device),
                                      on_device(np.asarray(timestep).astype(np.int64), device),
                                      rank_metrics._f32_threshold(threshold), everything)


def write_csv(path: Path, rows: List[Dict]) -> None:
    lines = [HEADER] + [f"{r['timestep']},{r['pr_auc_illicit']},{r['f1_illicit_at_thr']},{r['n']}" for r in rows]
    Path(path).write_text("\n".join(lines) + "\n", encoding="utf-8")


def main(argv=None, device: Optional[torch.device] = None) -> List[Dict]:
    ap = argparse.ArgumentParser(description="Evaluate metrics by timestep")
    ap.add_argument("--run_dir", type=Path, required=True, help="Directory containing evaluation artifacts")
    args = ap.parse_args(argv)
    run = args.run_dir
    with open(run / "metrics.json", "r", encoding="utf-8") as fh:
        threshold = float(json.load(fh).get("threshold"))
    rows = by_time(np.load(run / "scores_test.npy"), np.load(run / "y_test.npy").astype(int),
                   np.load(run / "timestep_test.npy"), threshold, device)
    write_csv(run / "by_time.csv", rows)
    return rows


if __name__ == "__main__":
    main()
