"""Paired bootstrap comparison between two runs (src/analysis/bootstrap_compare.py, same CLI and files).

    python -m elliptic_gnn_project_amd.bootstrap_compare --run_a outputs/gnn/a --run_b outputs/gnn/b

Reads ``y_test.npy`` / ``scores_test.npy`` / ``node_idx_test.npy`` as train_gnn.main writes them, aligns
the runs by node index and writes ``bootstrap_compare.json`` into run_b plus the two symmetric
``bootstrap_compare_<other run>.json`` files (and a copy under --out_dir).  The replicates run on the
GPU (rank_metrics, libgnnmp K14) when one is present, else in numpy.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import rank_metrics


def load_run(run_dir: Path) -> Dict[str, np.ndarray]:
    run_dir = Path(run_dir)
    y = np.load(run_dir / "y_test.npy").astype(int)
    scores = np.load(run_dir / "scores_test.npy")
    p = run_dir / "node_idx_test.npy"
    node_idx = np.load(p).astype(int) if p.exists() else np.arange(len(y), dtype=int)
    return {"y": y, "scores": scores, "node_idx": node_idx}


def align_runs(run_a: Dict[str, np.ndarray], run_b: Dict[str, np.ndarray]) -> Tuple[Dict, Dict]:
    """Both runs over their common nodes, in ascending node order (identical node lists pass through)."""
    ia, ib = run_a["node_idx"], run_b["node_idx"]
    if ia.shape == ib.shape and np.array_equal(ia, ib):
        return run_a, run_b
    common, a_idx, b_idx = np.intersect1d(ia, ib, assume_unique=False, return_indices=True)
    if common.size == 0:
        raise ValueError("No overlapping nodes between the provided runs.")
    pick = lambda r, i: {"y": r["y"][i], "scores": r["scores"][i], "node_idx": r["node_idx"][i]}  # noqa: E731
    return pick(run_a, a_idx), pick(run_b, b_idx)


def compare(run_a: Dict[str, np.ndarray], run_b: Dict[str, np.ndarray], topk: int, n_boot: int,
            seed: Optional[int] = 42, device: Optional[torch.device] = None) -> Dict:
    """The reference's output dict (without the run paths) for two aligned runs."""
    y = run_a["y"]
    if not np.array_equal(y, run_b["y"]):
        raise ValueError("the aligned runs disagree on the labels: not the same test set")
    n = int(len(y))
    k = int(min(int(topk), n))
    if device is None:
        device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    yt = torch.from_numpy(np.ascontiguousarray(y)).to(device)
    sa = torch.from_numpy(np.ascontiguousarray(run_a["scores"], dtype=np.float32)).to(device)
    sb = torch.from_numpy(np.ascontiguousarray(run_b["scores"], dtype=np.float32)).to(device)
    everything = torch.ones(n, dtype=torch.bool, device=device)  # the reference scores every aligned sample
    pos = (yt == 1).to(torch.int64)
    boots = rank_metrics.paired_bootstrap(pos, sa, sb, k, n_boot, seed)
    m = {name: {"run_a": float(fn(sa)), "run_b": float(fn(sb))} for name, fn in (
        ("pr_auc", lambda s: rank_metrics.average_precision(s, pos, everything)),
        ("precision_at_k", lambda s: rank_metrics.precision_at_k(s, pos, k, everything)))}
    return {"n_samples": n, "n_bootstrap": int(n_boot), "top_k": k, **boots, **m}


def main(argv=None) -> Dict:
    ap = argparse.ArgumentParser(description="Paired bootstrap comparison between two runs")
    ap.add_argument("--run_a", type=Path, required=True, help="Baseline run directory")
    ap.add_argument("--run_b", type=Path, required=True, help="Comparison run directory")
    ap.add_argument("--topk", type=int, default=100, help="Top-k for precision")
    ap.add_argument("--n_boot", type=int, default=1000, help="Number of bootstrap samples")
    ap.add_argument("--seed", type=int, default=42, help="Random seed")
    ap.add_argument("--out_dir", type=Path, default=None, help="Optional extra output directory")
    args = ap.parse_args(argv)

    run_a, run_b = align_runs(load_run(args.run_a), load_run(args.run_b))
    output = {"run_a": str(args.run_a), "run_b": str(args.run_b),
              **compare(run_a, run_b, args.topk, args.n_boot, args.seed)}
    text = json.dumps(output, indent=2)
    args.run_a.mkdir(parents=True, exist_ok=True)
    args.run_b.mkdir(parents=True, exist_ok=True)
    (args.run_b / "bootstrap_compare.json").write_text(text, encoding="utf-8")
    (args.run_b / f"bootstrap_compare_{args.run_a.name}.json").write_text(text, encoding="utf-8")
    (args.run_a / f"bootstrap_compare_{args.run_b.name}.json").write_text(text, encoding="utf-8")
    if args.out_dir is not None:
        args.out_dir.mkdir(parents=True, exist_ok=True)
        (args.out_dir / "bootstrap_compare.json").write_text(text, encoding="utf-8")
    print(text)
    return output


if __name__ == "__main__":
    main()
