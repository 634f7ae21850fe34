"""Writes golden/x3_ws_cpu_stats.json: per (shape, k1, k2, Nc) of tests/x3_ws_cases.py (at 256 CUs)
S_cpu, the RMS over the whole matrix of the CPU float32 product's error against float64 in units of
2^-24 |A| |W|^T, the yardstick of the tile and row statistic.
Run from the repository root: python tests/golden/make_x3_ws_stats.py"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parents[1]), str(HERE.parent)]

import x3_ws_cases as xc  # noqa: E402

if __name__ == "__main__":
    xc.STATS_FILE.write_text(json.dumps(xc.compute_stats(), indent=1) + "\n")
    print(xc.STATS_FILE.read_text())
