"""What the captured epoch loop (``epoch_block``, epoch_loop.EpochLoop, libgnnmp K21) is worth, on the GPU:
the wall time per epoch of train_gnn.main's epoch loop on the full synthetic Elliptic-shape graph (the graph
bench.py times its step on), for ``sage`` and ``sage_resbn`` (bench.py's presets), as

  (a) the loop without the key, ``device_metrics: true``     (one host read and one host decision per epoch)
  (b) ``epoch_block: 1``   (c) ``epoch_block: 10``   (d) ``epoch_block: 50``

A window is one whole loop of EPOCHS epochs with the patience set past it, timed from a synchronised start
to the loop's last host read: (a) from the first RunLogger.log_epoch to the last one, over the epochs between
them; (b)-(d) around EpochLoop.run, which starts after the capture and ends with the best state loaded.  The
four loops run interleaved, WINDOWS + 1 times each; the first window of each is warm-up (code objects, plans,
allocator) and dropped; best and median of the others are reported.

    python profiles/epoch_loop.py            # writes profiles/epoch_loop.json

Not a test and not the benchmark (bench.py measures the train step).  Needs the GPU: no fallback.
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
sys.path.insert(0, str(ROOT))

ARCHS = {  # bench.py's presets
    "sage": dict(arch="sage", hidden_dim=128, layers=2, dropout=0.5, symmetrize_edges=True, use_time_scalar=True,
                 train_window_k=10),
    "sage_resbn": dict(arch="sage_resbn", hidden_dim=64, layers=3, dropout=0.2, symmetrize_edges=True,
                       use_time_scalar=False, time_embed_dim=2, time_embed_type="sin", train_window_k=8, use_bn=True,
                       residual=True),
}
LOOPS = {"a_key_absent": 0, "b_block_1": 1, "c_block_10": 10, "d_block_50": 50}


def one_window(cfg, epochs):
    """ms per epoch of one loop of main(cfg)."""
    from elliptic_gnn_project_amd import epoch_loop, train_gnn

    stamps, span = [], []
    log_orig, run_orig = train_gnn.RunLogger.log_epoch, epoch_loop.EpochLoop.run

    def log_epoch(self, *a, **k):
        log_orig(self, *a, **k)
        stamps.append(time.perf_counter())

    def run(self, *a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run_orig(self, *a, **k)  # (ends with a host read of the state block)
        torch.cuda.synchronize()
        span.append((time.perf_counter() - t0, out["epochs"]))
        return out

    train_gnn.RunLogger.log_epoch, epoch_loop.EpochLoop.run = log_epoch, run
    try:
        train_gnn.main(cfg)
    finally:
        train_gnn.RunLogger.log_epoch, epoch_loop.EpochLoop.run = log_orig, run_orig
    if span:
        assert span[0][1] == epochs, span
        return span[0][0] / epochs * 1e3
    assert len(stamps) == epochs, len(stamps)
    return (stamps[-1] - stamps[0]) / (epochs - 1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--archs", nargs="+", default=list(ARCHS), choices=list(ARCHS))
    ap.add_argument("--synthetic", type=json.loads, default={}, help="synthetic_elliptic kwargs (default: full shape)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "epoch_loop.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("epoch_loop.py measures on the GPU; none found")
    from elliptic_gnn_project_amd.dataset_elliptic import save_graph, synthetic_elliptic

    res = {"device": torch.cuda.get_device_name(0), "epochs": args.epochs, "windows": args.windows,
           "unit": "ms per epoch", "archs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        graph = str(Path(tmp) / "graph.npz")
        save_graph(graph, synthetic_elliptic(**args.synthetic))  # generated once, loaded by every loop
        for arch in args.archs:
            base = dict(ARCHS[arch], output_root=tmp, graph_file=graph, lr=0.005, weight_decay=5e-4, max_epochs=args.epochs,
                        patience=10 ** 6, grad_clip=1.0, amp=False, calibrate_temperature=False, topk=100)
            per = {name: [] for name in LOOPS}
            for w in range(args.windows + 1):  # interleaved: a, b, c, d, a, b, ...
                for name, K in LOOPS.items():
                    cfg = dict(base, run_name=f"{arch}_{name}_{w}", **(dict(epoch_block=K) if K else dict(device_metrics=True)))
                    ms = one_window(cfg, args.epochs)
                    print(f"{arch} {name} window {w}{' (warm-up)' if w == 0 else ''}: {ms:.4f} ms/epoch", flush=True)
                    if w > 0:
                        per[name].append(ms)
            out = {name: dict(best=min(v), median=statistics.median(v), windows=v) for name, v in per.items()}
            for name in ("b_block_1", "c_block_10", "d_block_50"):
                out[name]["median_over_a"] = out[name]["median"] / out["a_key_absent"]["median"]
            res["archs"][arch] = out
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(res, indent=2) + "\n")
    print(json.dumps(res, indent=2))


if __name__ == "__main__":
    main()
