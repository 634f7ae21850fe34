"""What the device ranking metrics (rank_metrics, libgnnmp K14) are worth, on the GPU:

(a) the wall time of one iteration of train_gnn.main's epoch loop (train step, evaluation forward,
    validation PR-AUC, log line, best-state copy) with ``device_metrics`` off and on, on the full
    synthetic Elliptic-shape graph.  The time between consecutive RunLogger.log_epoch calls is one
    iteration (the loop ends every iteration with a host read, so the clock sees finished work);
    the two settings run interleaved, REPS times each, and every repetition's median is kept so the
    run-to-run spread stands next to the difference;
(b) rank_metrics.paired_bootstrap at n_boot = 1000 over the test split's scores (n = its labelled
    count), host path against device path, interleaved, plus the time of the index draws both share.

    python profiles/rank_metrics_time.py            # writes profiles/rank_metrics.json

Not a test and not the benchmark (bench.py measures the train step).  Needs the GPU: no fallback.
"""
import argparse
import json
import statistics
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]


def epoch_times(cfg):
    """main(cfg) with the clock read at every log_epoch: the iterations' wall times (first two dropped: warm-up)."""
    from elliptic_gnn_project_amd import train_gnn

    stamps = []
    orig = train_gnn.RunLogger.log_epoch

    def log_epoch(self, *a, **k):
        orig(self, *a, **k)
        stamps.append(time.perf_counter())

    train_gnn.RunLogger.log_epoch = log_epoch
    try:
        train_gnn.main(cfg)
    finally:
        train_gnn.RunLogger.log_epoch = orig
    return np.diff(np.asarray(stamps))[2:]


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=list(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=80)
    ap.add_argument("--n_boot", type=int, default=1000)
    ap.add_argument("--boot_reps", type=int, default=3)
    ap.add_argument("--synthetic", type=json.loads, default={}, help="synthetic_elliptic kwargs (default: full shape)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "rank_metrics.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_metrics_time.py measures on the GPU; none found")
    import sys

    sys.path.insert(0, str(ROOT))
    from elliptic_gnn_project_amd import rank_metrics

    res = {"device": torch.cuda.get_device_name(0), "epochs": args.epochs, "reps": args.reps}
    with tempfile.TemporaryDirectory() as tmp:
        base = dict(output_root=tmp, arch="sage", hidden_dim=128, layers=2, dropout=0.3, lr=0.005, weight_decay=5e-4,
                    max_epochs=args.epochs, patience=10 ** 6, grad_clip=1.0, amp=False, symmetrize_edges=True,
                    use_time_scalar=True, train_window_k=10, calibrate_temperature=False, topk=100,
                    synthetic=args.synthetic)
        per = {"off": [], "on": []}
        for r in range(args.reps):  # interleaved: off, on, off, on, ...
            for mode in ("off", "on"):
                t = epoch_times(dict(base, run_name=f"{mode}{r}", device_metrics=mode == "on"))
                per[mode].append(float(np.median(t)) * 1e3)
                print(f"rep {r} device_metrics {mode}: median epoch {per[mode][-1]:.3f} ms over {len(t)} epochs", flush=True)
        res["epoch_ms"] = {m: spread(v) for m, v in per.items()}
        res["epoch_ratio_on_over_off"] = res["epoch_ms"]["on"]["median"] / res["epoch_ms"]["off"]["median"]
        run = Path(tmp) / "gnn" / "off0"
        y = (np.load(run / "y_test.npy") == 1).astype(np.int64)
        s_a = np.load(run / "scores_test.npy").astype(np.float32)
    rng = np.random.default_rng(0)
    s_b = np.clip(s_a + 0.05 * rng.standard_normal(len(s_a)).astype(np.float32), 0, 1).astype(np.float32)
    n = len(y)
    res["bootstrap"] = {"n": n, "n_boot": args.n_boot, "topk": 100}
    dev = torch.device("cuda")
    sa_d, sb_d = torch.from_numpy(s_a).to(dev), torch.from_numpy(s_b).to(dev)
    rank_metrics.paired_bootstrap(y, sa_d, sb_d, 100, 8)  # warm-up: buffers, code objects
    tim = {"host": [], "device": [], "draws": []}
    out = {}
    for _ in range(args.boot_reps):
        for mode in ("host", "device"):
            t0 = time.perf_counter()
            out[mode] = rank_metrics.paired_bootstrap(y, *((s_a, s_b) if mode == "host" else (sa_d, sb_d)), 100,
                                                      args.n_boot)  # (ends in host reads of the results)
            tim[mode].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        g = np.random.default_rng(42)
        for _ in range(args.n_boot):
            g.choice(n, size=n, replace=True)
        tim["draws"].append(time.perf_counter() - t0)
    res["bootstrap"]["seconds"] = {m: spread(v) for m, v in tim.items()}
    res["bootstrap"]["host_over_device"] = res["bootstrap"]["seconds"]["host"]["median"] / \
        res["bootstrap"]["seconds"]["device"]["median"]
    res["bootstrap"]["max_abs_result_difference"] = max(
        abs(out["host"][k][f] - out["device"][k][f]) for k in out["host"] for f in out["host"][k])
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(res, indent=2) + "\n")
    print(json.dumps(res, indent=2))


if __name__ == "__main__":
    main()
