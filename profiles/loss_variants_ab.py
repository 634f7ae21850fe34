"""ms/step of the captured train_epoch step on the full-size synthetic graph (N = 203,769,
E_s = 468,710) for the loss settings of src/train_gnn.py:136-183 — default, time_loss_weighting
sqrt, focal gamma 2 — on SAGE (the headline preset) and SAGE-ResBN.  One JSON line per cell.

Run it on two checkouts in one session, alternating (profiles/r115_loss_variants.txt was made so):
    python profiles/loss_variants_ab.py --root <checkout> --tag parent|new
Each cell: CapturedStep(train_epoch, defer_loss=True), WARM replays, then REPS windows of STEPS
replays timed with device events; the cell's figure is the median window, min and max beside it."""
import argparse
import json
import os
import statistics
import sys

import torch

LOSSES = {
    "default": {},
    "sqrt": dict(time_loss_weighting="sqrt"),
    "focal2": dict(focal_loss=True, focal_gamma=2.0),
}
WARM, REPS, STEPS = 30, 7, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="new")
    ap.add_argument("--archs", default="sage,sage_resbn")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import bench
    from elliptic_gnn_project_amd import distributed as gdist
    from elliptic_gnn_project_amd.planes import register_input
    from elliptic_gnn_project_amd.train_gnn import CapturedStep, _make_loss_fn, build_model, train_epoch
    from elliptic_gnn_project_amd.train_ops import ClipAdam

    dev = torch.device("cuda", 0)
    scaler = torch.amp.GradScaler(device="cuda", enabled=False)
    for arch in args.archs.split(","):
        preset = bench.PRESETS[arch]
        full, _ = bench.make_global_graph(1, "strong", "powerlaw", preset["cfg"], preset.get("gen"))
        data = full.to(dev)
        register_input(data.x)
        cw, denom = gdist.global_class_weight_and_count(full.y, full.train_mask, None)
        t_train = full.timestep[full.train_mask]
        for name, lcfg in LOSSES.items():
            cfg = dict(preset["cfg"], **lcfg)
            torch.manual_seed(42)
            model = build_model(cfg["arch"], data.x.size(1), cfg).to(dev)
            opt = ClipAdam(model.parameters(), lr=0.003, weight_decay=1e-4, max_norm=1.0)
            loss_fn = _make_loss_fn(cfg, cw, model, int(t_train.min()), int(t_train.max()))

            def step():
                return train_epoch(model, data, data.edge_index, opt, loss_fn, scaler, False, cfg, dev, sync=False,
                                   denom=denom)

            cs = CapturedStep(step, defer_loss=True)
            for _ in range(WARM):
                cs()
            torch.cuda.synchronize()
            ms = []
            for _ in range(REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(STEPS):
                    out = cs()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / STEPS)
            print(json.dumps(dict(tag=args.tag, arch=arch, loss=name, ms_step=round(statistics.median(ms), 5),
                                  ms_min=round(min(ms), 5), ms_max=round(max(ms), 5), loss_value=float(out),
                                  nodes=int(data.x.size(0)), edges=int(data.edge_index.size(1)))), flush=True)
            del cs, model, opt


if __name__ == "__main__":
    main()
