"""Precision of the k highest-scored test samples over a grid of k (src/analysis/workload_curves.py, same
CLI and file).

    python -m elliptic_gnn_project_amd.workload_curves --run_dir outputs/gnn/<run> [--k_max 5000]

Reads ``scores_test.npy`` / ``y_test.npy`` and writes ``workload_curve.csv`` (no plot: DESIGN.md §7).  One
rank plan and one scan answer every k (rank_metrics.precision_curve, libgnnmp K19) on the GPU when one is
present, else the same arithmetic in numpy.

Ties follow this project's order: score descending, equal scores by ascending index.  The reference sorts
with numpy's unstable argsort, which leaves a k inside a tie group of mixed labels undefined; wherever the
reference's value is defined (distinct scores, or ties of one label around k) this is it.
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import rank_metrics
from .eval_by_time import on_device, pick_device

HEADER = "k,precision_at_k"


def build_k_values(n: int, k_max: int) -> List[int]:
    """The reference's grid: nothing for n = 0; with limit = min(k_max, n), [limit] below 10, else
    10, 20, ... up to limit, and limit itself when it is no multiple of 10."""
    if n == 0:
        return []
    limit = min(int(k_max), int(n))
    if limit < 10:
        return [limit]
    values = list(range(10, limit + 1, 10))
    if values[-1] != limit:
        values.append(limit)
    return values


def workload_curve(scores: np.ndarray, y: np.ndarray, k_max: int = 5000,
                   device: Optional[torch.device] = None) -> Tuple[List[int], List[float]]:
    """(k values, precision at each) with every test sample scored (positives are ``y == 1``)."""
    device = pick_device(device)
    ks = build_k_values(len(y), k_max)
    if not ks:
        return [], []
    everything = on_device(np.ones(len(y), dtype=bool), device)
    _, _, prec = rank_metrics.precision_curve(on_device(np.asarray(scores, dtype=np.float32), device),
                                              on_device(np.asarray(y).astype(np.int64), device), ks, everything)
    return ks, [float(v) for v in prec.cpu().tolist()]


def write_csv(path: Path, ks: List[int], precisions: List[float]) -> None:
    lines = [HEADER] + [f"{k},{p}" for k, p in zip(ks, precisions)]
    Path(path).write_text("\n".join(lines) + "\n", encoding="utf-8")


def main(argv=None, device: Optional[torch.device] = None) -> Tuple[List[int], List[float]]:
    ap = argparse.ArgumentParser(description="Workload precision curves")
    ap.add_argument("--run_dir", type=Path, required=True, help="Directory containing evaluation artifacts")
    ap.add_argument("--k_max", type=int, default=5000, help="Maximum k to evaluate")
    args = ap.parse_args(argv)
    ks, precisions = workload_curve(np.load(args.run_dir / "scores_test.npy"),
                                    np.load(args.run_dir / "y_test.npy").astype(int), args.k_max, device)
    write_csv(args.run_dir / "workload_curve.csv", ks, precisions)
    return ks, precisions


if __name__ == "__main__":
    main()
