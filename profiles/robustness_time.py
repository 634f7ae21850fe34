"""Where a robustness trial's time goes (elliptic_gnn_project_amd/robustness.py), on the GPU:

(a) the wall time of one trial on the full synthetic Elliptic-shape graph (SAGE preset), split into
    edge drop, graph-plan build, feature noise, forward, temperature fit and host metrics — every
    phase ends in a device synchronise (or a host read), TRIALS warmed trials with seeds of their own,
    median and spread per phase;
(b) the noise kernel (libgnnmp K15, gnn_feature_noise_f32) against the expression it replaces,
    ``x + torch.randn_like(x) * std``, interleaved, device events around CALLS calls each, with the
    kernel's achieved bytes/s (one read and one write of [N, F] f32 over its time) next to the 6.3 TB/s
    a device copy reaches on this part.

    python profiles/robustness_time.py            # writes profiles/robustness.json

Not a test and not the benchmark.  Needs the GPU: no fallback.
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
COPY_CEILING = 6.3e12  # bytes/s of a device-to-device copy (MI355X_MICROARCH: achieved HBM copy rate)


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=list(v))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def trial_phases(r, drop_frac, noise_std, seed):
    """One trial of Run.trial / Run.evaluate, phase by phase (ms)."""
    from elliptic_gnn_project_amd import _lib, robustness as R
    from elliptic_gnn_project_amd.graph import get_plan
    from elliptic_gnn_project_amd.train_gnn import _metrics

    ph = {}
    (ei, n), ph["edge_drop"] = timed(lambda: R.drop_edges(r.data.edge_index, drop_frac, seed))
    _, ph["plan_build"] = timed(lambda: get_plan(ei, r.data.x.size(0), _lib.LOOPS_KEEP))
    x, ph["noise"] = timed(lambda: R.add_noise(r.data.x, noise_std, seed))

    def fwd():
        with torch.no_grad():
            return r.model(x, ei, r.t_idx).float()

    logits, ph["forward"] = timed(fwd)
    vm = r.data.val_mask
    T, ph["temperature_fit"] = timed(lambda: R.fit_temperature(logits[vm], r.data.y[vm]))

    def host():
        p = torch.softmax(logits / T, dim=1)[:, 1].cpu().numpy()
        return _metrics(r.y_test_bin, p[r.test_np], r.threshold, r.cfg)

    _, ph["host_metrics"] = timed(host)
    ph["total"] = sum(ph.values())
    return ph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--drop_frac", type=float, default=0.1)
    ap.add_argument("--noise_std", type=float, default=0.01)
    ap.add_argument("--synthetic", type=json.loads, default={}, help="synthetic_elliptic kwargs (default: full shape)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "robustness.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robustness_time.py measures on the GPU; none found")
    sys.path.insert(0, str(ROOT))
    from elliptic_gnn_project_amd import robustness as R, train_gnn

    res = {"device": torch.cuda.get_device_name(0), "drop_frac": args.drop_frac, "noise_std": args.noise_std}
    with tempfile.TemporaryDirectory() as tmp:
        cfg = dict(run_name="rob", output_root=tmp, arch="sage", hidden_dim=128, layers=2, dropout=0.3, lr=0.005,
                   weight_decay=5e-4, max_epochs=args.epochs, patience=10 ** 6, grad_clip=1.0, amp=False,
                   symmetrize_edges=True, use_time_scalar=True, train_window_k=10, calibrate_temperature=True,
                   topk=100, synthetic=args.synthetic)
        train_gnn.main(cfg)
        r = R.Run(Path(tmp) / "gnn" / "rob")
    N, F = r.data.x.shape
    res.update(num_nodes=int(N), num_features=int(F), num_edges=int(r.data.edge_index.size(1)), trials=args.trials)
    for seed in (1000, 1001):  # warm-up: code objects, allocator, LBFGS state
        trial_phases(r, args.drop_frac, args.noise_std, seed)
    per = {}
    for seed in range(args.trials):
        for k, v in trial_phases(r, args.drop_frac, args.noise_std, seed).items():
            per.setdefault(k, []).append(v)
        print(f"trial {seed}: " + ", ".join(f"{k} {v[-1]:.2f}" for k, v in per.items()) + " ms", flush=True)
    res["trial_ms"] = {k: spread(v) for k, v in per.items()}
    tot = res["trial_ms"]["total"]["median"]
    res["trial_share"] = {k: res["trial_ms"][k]["median"] / tot for k in per if k != "total"}

    # (b) the noise kernel against x + randn_like(x) * std
    x, std = r.data.x, args.noise_std
    buf = torch.empty_like(x)
    forms = {
        "torch_randn_like": lambda i: x + torch.randn_like(x) * std,
        "kernel_fresh_out": lambda i: R.add_noise(x, std, i),
        "kernel_reused_out": lambda i: R.add_noise(x, std, i, out=buf),
    }
    for f in forms.values():
        for i in range(3):
            f(i)
    ms = {k: [] for k in forms}
    for _ in range(args.reps):  # interleaved
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.calls):
                f(i)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.calls)
    nbytes = 2 * 4 * int(N) * int(F)
    res["noise"] = {"bytes_per_call": nbytes, "calls_per_window": args.calls, "copy_ceiling_bytes_per_s": COPY_CEILING,
                    "ms_per_call": {k: spread(v) for k, v in ms.items()}}
    for k in ("kernel_fresh_out", "kernel_reused_out"):
        bps = nbytes / (res["noise"]["ms_per_call"][k]["median"] * 1e-3)
        res["noise"][k + "_bytes_per_s"] = bps
        res["noise"][k + "_share_of_copy_ceiling"] = bps / COPY_CEILING
    res["noise"]["torch_over_kernel"] = (res["noise"]["ms_per_call"]["torch_randn_like"]["median"]
                                         / res["noise"]["ms_per_call"]["kernel_fresh_out"]["median"])
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(res, indent=2) + "\n")
    print(json.dumps(res, indent=2))


if __name__ == "__main__":
    main()
