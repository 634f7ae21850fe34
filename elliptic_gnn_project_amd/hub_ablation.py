"""Hub ablation (src/analysis/hub_ablation.py): evaluate a trained run on its graph without every edge
that touches one of the int(frac · N) nodes of highest in+out degree, and write the test metrics as JSON.

Hub sets are nested, so one degree ranking of the graph (libgnnmp K18, csrc/hub.hip) answers every
fraction.  For ``edge_index`` [2, E] with ids in [0, N):

    deg[v]         = #{e : src[e] = v} + #{e : dst[e] = v}     the reference's deg_src + deg_dst: a self loop
                                                               counts 2, duplicate edges count each time
    order          = the nodes by (deg descending, node id ascending);  rank = its inverse
    edge_rank[e]   = min(rank[src[e]], rank[dst[e]])
    removed_cum[r] = #{e : edge_rank[e] <= r}

``hubs(h) = order[:h]``; the ablated graph keeps the columns with ``edge_rank >= h`` in input order (as
the reference's ``edge_index_cpu[:, edge_mask]``), E - removed_cum[h - 1] of them.  A sweep over fractions
is one ranking plus one compaction per fraction, all on the device, with one host read for all the sizes.

Tie rule.  The reference picks its hubs with ``torch.topk``, which leaves the order of equal degrees
unspecified.  Here equal degrees go by ascending node id, so the hub set equals the reference's exactly
when the boundary is untied, ``deg[order[h-1]] > deg[order[h]]`` (``HubRanking.boundary_tied``); otherwise
it differs only in WHICH nodes of the boundary degree fill the last places (the hubs' degree multiset is
the same).  torch's tie order is not imitated.  ``train_gnn.main``'s ``ablate_hubs_frac`` keeps
``torch.topk`` (``train_gnn.hub_edge_mask``).

CUDA tensors go through the kernels; host tensors through the numpy mirror (identical integers).
"""
from __future__ import annotations

import argparse
import ctypes
import json
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

def num_hubs_of(num_nodes: int, frac: float) -> int:
    """int(frac · float(N)) as the reference (hub_ablation.py:60); a fraction outside [0, 1] or NaN raises."""
    frac = float(frac)
    if not (0.0 <= frac <= 1.0):  # (also refuses NaN)
        raise ValueError("frac must be within [0, 1]")
    return int(frac * float(int(num_nodes)))


def _check_edge_index(edge_index: torch.Tensor, num_nodes: int) -> Tuple[int, int]:
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    if edge_index.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"edge_index must be int64 or int32, got {edge_index.dtype}")
    N, E = int(num_nodes), int(edge_index.size(1))
    if N < 0 or N >= 2 ** 31 - 1 or E >= 2 ** 31 - 1:
        raise ValueError("num_nodes / num_edges outside the int32 range")
    return N, E


def host_ranking(edge_index, num_nodes: int) -> Tuple[np.ndarray, ...]:
    """(deg, order, rank, edge_rank, removed_cum) of the module docstring as int32 arrays: the numpy mirror."""
    ei = np.asarray(edge_index.detach().cpu() if isinstance(edge_index, torch.Tensor) else edge_index).astype(np.int64)
    N = int(num_nodes)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {ei.shape}")
    if ei.size and (int(ei.min()) < 0 or int(ei.max()) >= N):
        raise IndexError(f"edge_index holds a node id outside [0, {N})")
    src, dst = ei[0], ei[1]
    deg = np.bincount(src, minlength=N) + np.bincount(dst, minlength=N)
    order = np.argsort(-deg, kind="stable")
    rank = np.empty(N, dtype=np.int64)
    rank[order] = np.arange(N)
    edge_rank = np.minimum(rank[src], rank[dst])
    removed_cum = np.cumsum(np.bincount(edge_rank, minlength=N))
    return tuple(a.astype(np.int32) for a in (deg, order, rank, edge_rank, removed_cum))


class HubRanking:
    """The degree ranking of one graph: ``deg``, ``order``, ``rank``, ``removed_cum`` [N] and ``edge_rank`` [E],
    int32 tensors on ``edge_index``'s device.  The node ids are checked here, once (one host read)."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int):
        N, E = _check_edge_index(edge_index, num_nodes)
        self.edge_index, self.num_nodes, self.num_edges = edge_index, N, E
        dev = edge_index.device
        if E and N == 0:
            raise IndexError("edge_index holds a node id outside [0, 0)")
        if not edge_index.is_cuda:
            self._ei = edge_index.detach().to(torch.int64)
            arrays = host_ranking(self._ei, N)
            self.deg, self.order, self.rank, self.edge_rank, self.removed_cum = (torch.from_numpy(a) for a in arrays)
            return
        self._ei = ei = edge_index.detach().to(torch.int64).contiguous()
        if E:
            lo, hi = torch.aminmax(ei)
            lo, hi = torch.stack([lo, hi]).cpu().tolist()
            if lo < 0 or hi >= N:
                raise IndexError(f"edge_index holds a node id outside [0, {N})")
        self.deg, self.order, self.rank, self.removed_cum = (torch.empty(N, dtype=torch.int32, device=dev)
                                                             for _ in range(4))
        self.edge_rank = torch.empty(E, dtype=torch.int32, device=dev)
        if E == 0:  # no edge: every degree 0, the nodes in id order
            self.deg.zero_()
            self.removed_cum.zero_()
            torch.arange(N, dtype=torch.int32, device=dev, out=self.order)
            self.rank.copy_(self.order)
            return
        lib = _lib.load()
        b = _lib.c_size(0)
        _lib.check(lib.gnn_hub_rank_workspace_size(N, E, ctypes.byref(b)), "gnn_hub_rank_workspace_size")
        ws = torch.empty(max(int(b.value), 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("gnn_hub_rank", ei.data_ptr(), E, N, self.deg.data_ptr(), self.order.data_ptr(),
                      self.rank.data_ptr(), self.edge_rank.data_ptr(), self.removed_cum.data_ptr(), ws.data_ptr(),
                      ws.numel(), _lib.stream_handle(dev))

    def _num_hubs(self, h) -> int:
        h = int(h)
        if not 0 <= h <= self.num_nodes:
            raise ValueError(f"num_hubs {h} outside [0, {self.num_nodes}]")
        return h

    def describe(self, hs: Sequence[int]) -> List[Dict]:
        """Per hub count h: ``kept`` (the edges left), ``min_hub_degree`` (deg[order[h-1]]; None for h = 0) and
        ``boundary_tied`` (0 < h < N and deg[order[h-1]] == deg[order[h]]).  One gather and ONE host read
        for the whole list."""
        hs = [self._num_hubs(h) for h in hs]
        N, E = self.num_nodes, self.num_edges
        if not hs or N == 0:
            return [dict(kept=E, min_hub_degree=None, boundary_tied=False) for _ in hs]
        h_t = torch.tensor(hs, dtype=torch.int64, device=self.deg.device)
        last, nxt = (h_t - 1).clamp_(min=0), h_t.clamp(max=N - 1)
        got = torch.cat([self.removed_cum[last], self.deg[self.order[last].long()], self.deg[self.order[nxt].long()]])
        removed, d_last, d_next = got.cpu().view(3, -1).tolist()
        return [dict(kept=E - (removed[i] if h else 0), min_hub_degree=(d_last[i] if h else None),
                     boundary_tied=bool(0 < h < N and d_last[i] == d_next[i])) for i, h in enumerate(hs)]

    def kept_counts(self, hs: Sequence[int]) -> List[int]:
        """E - removed_cum[h - 1] (E for h = 0) of every h in ``hs``: one gather and one host read."""
        return [d["kept"] for d in self.describe(hs)]

    def boundary_tied(self, h: int) -> bool:
        """True when nodes of equal degree sit on both sides of the cut: hubs(h) is then one of several
        sets torch.topk may return (module docstring)."""
        return self.describe([h])[0]["boundary_tied"]

    def hubs(self, h: int) -> torch.Tensor:
        return self.order[:self._num_hubs(h)]

    def ablate(self, h: int, kept: Optional[int] = None) -> torch.Tensor:
        """edge_index without every edge that touches one of hubs(h): h = 0 returns ``edge_index`` itself,
        otherwise a new [2, kept] int64 tensor, columns in input order.  ``kept`` is ``kept_counts([h])[0]``;
        handing it in (from one kept_counts call for a whole sweep) saves this call's host read.  An
        ablation that leaves no edge raises RuntimeError."""
        h = self._num_hubs(h)
        if h == 0:
            return self.edge_index
        kept = self.kept_counts([h])[0] if kept is None else int(kept)
        if not 0 <= kept <= self.num_edges:
            raise ValueError(f"kept {kept} outside [0, {self.num_edges}]")
        if kept == 0:
            raise RuntimeError("Removing these hubs would leave an empty graph.")
        if not self._ei.is_cuda:
            out = self._ei[:, self.edge_rank >= h].contiguous()
            if out.size(1) != kept:
                raise ValueError(f"kept {kept} is not the count of hub-free edges ({out.size(1)})")
            return out
        E, dev = self.num_edges, self._ei.device
        out = torch.empty((2, kept), dtype=torch.int64, device=dev)
        lib = _lib.load()
        b = _lib.c_size(0)
        _lib.check(lib.gnn_hub_ablate_workspace_size(E, ctypes.byref(b)), "gnn_hub_ablate_workspace_size")
        ws = torch.empty(max(int(b.value), 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("gnn_hub_ablate", self._ei.data_ptr(), E, self.edge_rank.data_ptr(), h, kept, out.data_ptr(),
                      ws.data_ptr(), ws.numel(), _lib.stream_handle(dev))
        return out


def ablate_hubs(edge_index: torch.Tensor, num_nodes: int, frac: float) -> Tuple[torch.Tensor, int]:
    """(edge_index without the edges of the int(frac · N) top-degree nodes, that count): the reference's
    build_edge_index_ablated under the tie rule of the module docstring.  A count of 0 returns
    ``edge_index`` itself."""
    N, _ = _check_edge_index(edge_index, num_nodes)
    h = num_hubs_of(N, frac)
    if h == 0:
        return edge_index, 0
    return HubRanking(edge_index, N).ablate(h), h


# ----------------------------------------------------------------------------- the tool
class Tool:
    """A run loaded once (robustness.Run) with everything the ablated evaluations share: the base
    forward, the temperature fitted ONCE on the base validation logits (the reference does not refit it
    for the ablated logits, unlike robustness), the decision threshold recomputed from the base
    probabilities (the reference's compute_threshold; not read from metrics.json) and, on first need,
    the graph's HubRanking."""

    def __init__(self, run_dir, processed_dir=None, device_eval: Optional[bool] = None):
        from .robustness import Run, fit_temperature
        from .train_gnn import _max_f1_threshold, _threshold

        self.run = r = Run(run_dir, processed_dir, device_eval, check_width=True)
        d, cfg = r.data, r.cfg
        self.num_nodes, self.num_edges = int(d.x.size(0)), int(d.edge_index.size(1))
        self._ranking: Optional[HubRanking] = None
        self.base_logits = self.logits(d.edge_index)
        self.T = None
        if r.calibrate and bool(d.val_mask.any()):
            if r.device_eval:
                from .calibrate import fit_temperature as fit_device

                self.T = fit_device(self.base_logits, d.y, mask=d.val_mask)
            else:
                self.T = fit_temperature(self.base_logits[d.val_mask], d.y[d.val_mask])
        self.base_probs = self.probs(self.base_logits)
        use_val = bool(cfg.get("use_val_for_thresholds", True))
        if r.device_eval:
            from . import rank_metrics as RM

            self.threshold = RM.select_threshold(self.base_probs, d.y, d.val_mask, cfg.get("precision_target", 0.0))[0] \
                if use_val else RM.select_threshold(self.base_probs, d.y, d.test_mask)[0]
        else:
            p = self.base_probs.cpu().numpy()
            val_np = d.val_mask.cpu().numpy().astype(bool)
            self.threshold = _threshold((r.y_np[val_np] == 1).astype(int), p[val_np], cfg) if use_val \
                else _max_f1_threshold(r.y_test_bin, p[r.test_np])

    @property
    def ranking(self) -> HubRanking:
        if self._ranking is None:
            self._ranking = HubRanking(self.run.data.edge_index, self.num_nodes)
        return self._ranking

    def logits(self, edge_index: torch.Tensor) -> torch.Tensor:
        r = self.run
        with torch.no_grad():
            return r.model(r.data.x, edge_index, r.t_idx).float()

    def probs(self, logits: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            return torch.softmax(logits / self.T if self.T is not None else logits, dim=1)[:, 1]

    def record(self, frac: float, kept: Optional[int] = None, details: Optional[Dict] = None) -> Dict:
        """The reference's record for one fraction.  ``kept`` (from one ``ranking.kept_counts`` call for a
        sweep) saves the ablation's host read; ``details`` (a dict) receives edge_index / logits / probs."""
        from .train_gnn import _metrics

        r, frac = self.run, float(frac)
        h = num_hubs_of(self.num_nodes, frac)
        if h == 0:
            ei, logits, probs = r.data.edge_index, self.base_logits, self.base_probs
        else:
            ei = self.ranking.ablate(h, kept)
            logits = self.logits(ei)
            probs = self.probs(logits)
        if r.device_eval:
            from . import rank_metrics as RM

            rec = RM.evaluation_record(probs, r.data.y, r.data.test_mask, self.threshold, r.cfg.get("topk", 100),
                                       r.cfg.get("precision_target", 0.90))
            p_np = probs.cpu().numpy() if details is not None else None
        else:
            p_np = probs.cpu().numpy()
            rec = _metrics(r.y_test_bin, p_np[r.test_np], self.threshold, r.cfg) if r.y_test_bin.size else {}
        if details is not None:
            details.update(edge_index=ei, logits=logits, probs=p_np, probs_device=probs, temperature=self.T, n_hubs=h)
        rec.update(n_hubs=int(h), hub_fraction=frac, n_edges_remaining=int(ei.size(1)))
        return rec


def _file_name(frac: float) -> str:
    return "metrics_hub_removed_%s.json" % str(float(frac)).replace(".", "p")


def run(run_dir, frac: float, processed_dir=None, device_eval: Optional[bool] = None,
        details: Optional[Dict] = None) -> Dict:
    """The reference's tool for one fraction: returns the record (the reference's eleven keys: train_gnn._metrics' eight,
    ``n_hubs``, ``hub_fraction``, ``n_edges_remaining``) and writes it to
    ``metrics_hub_removed_{str(frac).replace(".", "p")}.json`` in the run directory.  ``device_eval``
    overrides the run's config key of that name."""
    frac = float(frac)
    num_hubs_of(1, frac)  # a bad fraction raises before the run is loaded
    tool = Tool(run_dir, processed_dir, device_eval)
    rec = tool.record(frac, details=details)
    with open(tool.run.run_dir / _file_name(frac), "w", encoding="utf-8") as f:
        json.dump(rec, f, indent=2)
    return rec


def sweep(run_dir, fracs: Iterable[float], processed_dir=None, device_eval: Optional[bool] = None) -> Dict:
    """Every fraction over one loaded run: one base forward, one temperature, one threshold, one
    HubRanking and one host read for all the edge counts; then one compaction and one forward per
    fraction.  Returns {"base": the record of no hub removed, "records": [one per fraction]}, each with
    ``min_hub_degree`` (the lowest degree among the hubs; None without one) and ``boundary_tied``
    (module docstring) beside the single run's keys, and writes it to ``hub_ablation_sweep.json``."""
    fracs = [float(v) for v in fracs]
    for v in fracs:
        num_hubs_of(1, v)
    tool = Tool(run_dir, processed_dir, device_eval)
    hs = [num_hubs_of(tool.num_nodes, v) for v in fracs]
    info = tool.ranking.describe(hs) if any(hs) else [dict(kept=tool.num_edges, min_hub_degree=None,
                                                           boundary_tied=False) for _ in hs]

    def one(frac, d):
        rec = tool.record(frac, kept=d["kept"])
        rec.update(min_hub_degree=d["min_hub_degree"], boundary_tied=d["boundary_tied"])
        return rec

    out = dict(base=one(0.0, dict(kept=tool.num_edges, min_hub_degree=None, boundary_tied=False)),
               records=[one(v, d) for v, d in zip(fracs, info)])
    with open(tool.run.run_dir / "hub_ablation_sweep.json", "w", encoding="utf-8") as f:
        json.dump(out, f, indent=2)
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Evaluate hub ablation for a trained GNN run")
    ap.add_argument("--run_dir", type=Path, required=True, help="Path to the GNN run directory")
    ap.add_argument("--frac", type=float, default=0.01, help="Fraction of nodes to ablate as hubs")
    ap.add_argument("--fracs", type=float, nargs="+", default=None, help="Sweep: the fractions")
    ap.add_argument("--processed_dir", type=Path, default=None,
                    help="Directory containing the processed graph (default: the run's config)")
    ap.add_argument("--device_eval", action="store_true", default=None,
                    help="Temperature fit and metrics on the device (default: the run's device_eval key)")
    args = ap.parse_args(argv)
    if args.fracs is not None:
        out = sweep(args.run_dir, args.fracs, args.processed_dir, args.device_eval)
    else:
        out = run(args.run_dir, args.frac, args.processed_dir, args.device_eval)
    print(json.dumps(out, indent=2))


if __name__ == "__main__":
    main()
