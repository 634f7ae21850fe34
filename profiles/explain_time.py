"""Time per epoch of explain.explain_nodes on an Elliptic-size graph (bench.py's sage preset input):
fused_step on / off, B = 1 and B = 64 targets (the highest-scored nodes), with the concatenated row and
edge counts.  Run from the repository root on an MI355X:
    python profiles/explain_time.py [OUT.json]        (default profiles/explain.json)
Recorded, not gated: DESIGN.md §4 "Explainer" quotes the numbers."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elliptic_gnn_project_amd import explain as X  # noqa: E402
from elliptic_gnn_project_amd.dataset_elliptic import prepare_inputs, synthetic_elliptic  # noqa: E402
from elliptic_gnn_project_amd.train_gnn import build_model  # noqa: E402

EPOCHS = 50


def main(path):
    cfg = dict(arch="sage", hidden_dim=128, layers=2, dropout=0.5, symmetrize_edges=True, use_time_scalar=True,
               train_window_k=10)
    dev = torch.device("cuda:0")
    data = prepare_inputs(synthetic_elliptic(degree="powerlaw", seed=42), cfg).to(dev)
    torch.manual_seed(0)
    model = build_model("sage", data.x.size(1), cfg).to(dev).eval()
    with torch.no_grad():
        score = torch.softmax(model(data.x, data.edge_index), 1)[:, 1]
    top = torch.argsort(score, descending=True)[:64].tolist()
    F = int(data.x.size(1))
    out = dict(graph=dict(nodes=int(data.x.size(0)), edges=int(data.edge_index.size(1)), feats=F),
               model=f"SAGE 2L {F}->128->2 (bench.py sage preset, untrained weights)", epochs=EPOCHS, results=[])
    for B in (1, 64):
        for rep in range(2):  # the second pass is recorded (the first warms the allocator and the plans)
            for fused in (True, False):
                r = X.time_epochs(model, data, top[:B], epochs=EPOCHS, warmup=3, fused_step=fused)
                print(json.dumps(r), flush=True)
                if rep == 1:
                    out["results"].append(r)
    with open(path, "w") as f:
        json.dump(out, f, indent=2)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "explain.json"))
