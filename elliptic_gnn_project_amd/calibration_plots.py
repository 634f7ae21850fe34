"""The reliability table and ECE of a finished run (src/analysis/calibration_plots.py, same CLI).

    python -m elliptic_gnn_project_amd.calibration_plots --run_dir outputs/gnn/<run>

Reads ``scores_test.npy`` / ``y_test.npy``, writes ``calibration_curve.csv`` — the numbers behind the
reference's calibration_curve.png, which this project does not draw — and prints the ECE.
The 15 equal-width bins come from one counting pass on the GPU (rank_metrics.reliability_table, libgnnmp
K17) when one is present, else from the same arithmetic in numpy.
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch

from . import rank_metrics
from .eval_by_time import on_device, pick_device

HEADER = "bin_center,accuracy,confidence,count"
BINS = 15


def reliability(scores: np.ndarray, y: np.ndarray, bins: int = BINS, device: Optional[torch.device] = None) -> Dict:
    """rank_metrics.reliability_table with every test sample scored (positives are ``y == 1``)."""
    device = pick_device(device)
    everything = on_device(np.ones(len(y), dtype=bool), device)
    return rank_metrics.reliability_table(on_device(np.asarray(scores, dtype=np.float32), device),
                                          on_device(np.asarray(y).astype(np.int64), device), everything, bins)


def write_csv(path: Path, table: Dict) -> None:
    rows = zip(table["bin_center"].tolist(), table["accuracy"].tolist(), table["confidence"].tolist(),
               table["count"].tolist())
    lines = [HEADER] + [f"{c},{a},{f},{int(k)}" for c, a, f, k in rows]
    Path(path).write_text("\n".join(lines) + "\n", encoding="utf-8")


def main(argv=None, device: Optional[torch.device] = None) -> Dict:
    ap = argparse.ArgumentParser(description="Calibration plots")
    ap.add_argument("--run_dir", type=Path, required=True, help="Directory containing evaluation artifacts")
    args = ap.parse_args(argv)
    table = reliability(np.load(args.run_dir / "scores_test.npy"), np.load(args.run_dir / "y_test.npy").astype(int),
                        BINS, device)
    write_csv(args.run_dir / "calibration_curve.csv", table)
    print(f"ECE={table['ece']:.4f}")
    return table


if __name__ == "__main__":
    main()
