"""A robustness trial with ``device_eval`` off (the LBFGS fit and the host sklearn metrics) and on (the
temperature fit, the record and its one host read on the device, libgnnmp K17), on the GPU, in the
setting of profiles/robustness_time.py: the full synthetic Elliptic-shape graph, SAGE preset, drop
0.1 / noise 0.01.  TRIALS warmed trials per arm, the two arms INTERLEAVED in one process with the same
seeds; every phase ends in a device synchronise or a host read.  Per arm: median and range of the
trial and of the perturbation (edge drop, plan, noise), the forward, the fit and the metrics; the
fit's update count; |T_device - T_lbfgs|; and the fit launch alone between device events.

    python profiles/device_eval_time.py            # writes profiles/device_eval.json

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


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=list(v))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def trial_phases(r, drop_frac, noise_std, seed, device_eval):
    """One trial of Run.trial / Run.evaluate, phase by phase (ms), on either path."""
    from elliptic_gnn_project_amd import _lib, calibrate, rank_metrics, robustness as R
    from elliptic_gnn_project_amd.graph import get_plan
    from elliptic_gnn_project_amd.train_gnn import _metrics

    ph, info = {}, {}

    def perturb():
        ei, _ = R.drop_edges(r.data.edge_index, drop_frac, seed)
        get_plan(ei, r.data.x.size(0), _lib.LOOPS_KEEP)
        return ei, R.add_noise(r.data.x, noise_std, seed)

    (ei, x), ph["perturb"] = timed(perturb)

    def fwd():
        with torch.no_grad():
            return r.model(x, ei, r.t_idx).float()

    logits, ph["forward"] = timed(fwd)
    vm = r.data.val_mask
    if device_eval:
        T, ph["temperature_fit"] = timed(lambda: calibrate.fit_temperature(logits, r.data.y, vm, info))

        def record():
            p = torch.softmax(logits / T, dim=1)[:, 1]
            return rank_metrics.evaluation_record(p, r.data.y, r.data.test_mask, r.threshold, r.cfg.get("topk", 100),
                                                  r.cfg.get("precision_target", 0.90))

        rec, ph["metrics"] = timed(record)
    else:
        T, ph["temperature_fit"] = timed(lambda: R.fit_temperature(logits[vm], r.data.y[vm]))

        def host():
            p = torch.softmax(logits / T, dim=1)[:, 1].cpu().numpy()
            return _metrics(r.y_test_bin, p[r.test_np], r.threshold, r.cfg)

        rec, ph["metrics"] = timed(host)
    ph["total"] = sum(ph.values())
    info.update(T=float(T), record=rec)
    return ph, info, logits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--drop_frac", type=float, default=0.1)
    ap.add_argument("--noise_std", type=float, default=0.01)
    ap.add_argument("--synthetic", type=json.loads, default={}, help="synthetic_elliptic kwargs (default: full shape)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "device_eval.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_eval_time.py measures on the GPU; none found")
    sys.path.insert(0, str(ROOT))
    from elliptic_gnn_project_amd import calibrate, robustness as R, train_gnn

    res = {"device": torch.cuda.get_device_name(0), "drop_frac": args.drop_frac, "noise_std": args.noise_std}
    with tempfile.TemporaryDirectory() as tmp:
        cfg = dict(run_name="rob", output_root=tmp, arch="sage", hidden_dim=128, layers=2, dropout=0.3, lr=0.005,
                   weight_decay=5e-4, max_epochs=args.epochs, patience=10 ** 6, grad_clip=1.0, amp=False,
                   symmetrize_edges=True, use_time_scalar=True, train_window_k=10, calibrate_temperature=True,
                   topk=100, synthetic=args.synthetic)
        train_gnn.main(cfg)
        r = R.Run(Path(tmp) / "gnn" / "rob")
    N = int(r.data.x.size(0))
    res.update(num_nodes=N, num_edges=int(r.data.edge_index.size(1)), val_rows=int(r.data.val_mask.sum()),
               test_rows=int(r.data.test_mask.sum()), trials=args.trials)
    for seed in (1000, 1001):  # warm-up of both arms: code objects, allocator, LBFGS state, buffers
        for arm in (False, True):
            trial_phases(r, args.drop_frac, args.noise_std, seed, arm)
    per = {False: {}, True: {}}
    its, dT = [], []
    for seed in range(args.trials):
        got = {}
        for arm in (False, True):  # interleaved
            ph, info, logits = trial_phases(r, args.drop_frac, args.noise_std, seed, arm)
            got[arm] = info
            for k, v in ph.items():
                per[arm].setdefault(k, []).append(v)
        its.append(got[True]["iterations"])
        dT.append(abs(got[True]["T"] - got[False]["T"]))
        print(f"trial {seed}: off {per[False]['total'][-1]:.2f} ms (fit {per[False]['temperature_fit'][-1]:.2f}, "
              f"metrics {per[False]['metrics'][-1]:.2f}), on {per[True]['total'][-1]:.2f} ms "
              f"(fit {per[True]['temperature_fit'][-1]:.3f}, metrics {per[True]['metrics'][-1]:.3f}), "
              f"updates {its[-1]}, |dT| {dT[-1]:.3g}", flush=True)
    res["off_ms"] = {k: spread(v) for k, v in per[False].items()}
    res["on_ms"] = {k: spread(v) for k, v in per[True].items()}
    res["fit_updates"] = its
    res["fit_status"] = got[True]["status"]
    res["abs_T_device_minus_T_lbfgs"] = dT
    res["T_device"], res["T_lbfgs"] = got[True]["T"], got[False]["T"]
    res["on_range_below_off_range"] = res["on_ms"]["total"]["max"] < res["off_ms"]["total"]["min"]
    res["ratio_off_over_on"] = {k: res["off_ms"][k]["median"] / res["on_ms"][k]["median"]
                                for k in ("total", "temperature_fit", "metrics")}

    # the fit's launch alone (with its wrapper's allocations and the status read): device events around CALLS calls
    vm = r.data.val_mask
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            calibrate.fit_temperature(logits, r.data.y, vm)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / args.calls)
    res["fit_call_ms"] = spread(ms)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(res, indent=2) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("off_ms", "on_ms")}, indent=2))
    for arm in ("off_ms", "on_ms"):
        print(arm, {k: (round(v["median"], 3), round(v["min"], 3), round(v["max"], 3)) for k, v in res[arm].items()})


if __name__ == "__main__":
    main()
