"""Robustness analysis (src/analysis/robustness.py): evaluate a trained run with a fraction of its
edges dropped uniformly at random and Gaussian noise added to its node features, refit the
temperature on the perturbed validation logits and write the test metrics as JSON.

The perturbations are seeded counter hashes (libgnnmp K15, csrc/perturb.hip) with a bit-exact numpy
mirror in this file, not torch's device RNG streams: a trial is a pure function of (drop_frac,
noise_std, seed) on the GPU and on the host.  All arithmetic below is mod 2^64 / 2^32.

    splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
                   z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31
    key(seed, stream) = splitmix64(seed ^ (stream * 0xD1B54A32D192ED03))     1 drop, 2 radius, 3 angle
    H(c, key) = fmix32(((uint32)c * 0x9E3779B1 + key_lo) ^ key_hi)           (the dropout mask's hash)

* ``drop_edges``: drop_count = min(int(round(drop_frac · E)), E) as the reference; the dropped edges are
  the drop_count columns e with the smallest (H(e, key(seed, 1)), e).  The kept columns stay in their
  ORIGINAL order (the reference returns them permuted): every row's summation order is kept, so a
  trial stays bit-comparable to the unperturbed forward on untouched rows.
* ``add_noise``: for element (row, col) of [rows, F], P = ceil(F / 2), c = row · P + (col >> 1):
  u1 = ((H(c, key(seed, 2)) >> 8) + 1) · 2^-24, u2 = (H(c, key(seed, 3)) >> 8) · 2^-24,
  r = sqrt(-2 ln u1), z = r cos(2π u2) (even col) / r sin(2π u2) (odd col), out = x + noise_std · z.

CUDA tensors go through the kernels; host tensors through the mirror (edge drop: identical bits; noise:
the float64 evaluation of the formulas, rounded once).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
import yaml

from . import _lib

_M64 = 0xFFFFFFFFFFFFFFFF
STREAM_DROP, STREAM_RADIUS, STREAM_ANGLE = 1, 2, 3

# the float metrics sweep() averages over seeds
SUMMARY_KEYS = ("pr_auc_illicit", "roc_auc", "f1_illicit_at_thr", "precision_at_k", "recall_at_precision", "ece",
                "temperature")


# ----------------------------------------------------------------------------- keys and hash (host mirror)
def splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def key(seed: int, stream: int) -> int:
    return splitmix64((int(seed) & _M64) ^ ((int(stream) * 0xD1B54A32D192ED03) & _M64))


def hash_u32(c, k: int) -> np.ndarray:
    """H(c, k) of every counter in ``c`` (integers below 2^32) as uint32."""
    c = np.asarray(c)
    if c.size and (int(c.max()) >= 2 ** 32 or int(c.min()) < 0):
        raise ValueError("hash_u32: counter outside [0, 2^32)")
    with np.errstate(over="ignore"):
        h = c.astype(np.uint32) * np.uint32(0x9E3779B1) + np.uint32(k & 0xFFFFFFFF)
        h = h ^ np.uint32(k >> 32)
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(0x85EBCA6B)
        h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xC2B2AE35)
        h = h ^ (h >> np.uint32(16))
    return h


# ----------------------------------------------------------------------------- edge drop
def drop_count_of(num_edges: int, drop_frac: float) -> int:
    """The reference's count (robustness.py:66-78): round half to even, clamped to E; raises as it does."""
    drop_frac = float(drop_frac)
    if not (0.0 <= drop_frac <= 1.0):  # (also refuses NaN)
        raise ValueError("drop_frac must be within [0, 1]")
    n = min(int(round(drop_frac * float(num_edges))), int(num_edges))
    if n > 0 and n >= num_edges:
        raise RuntimeError("Dropping all edges would leave an empty graph.")
    return n


def host_keep_mask(num_edges: int, drop_count: int, seed: int) -> np.ndarray:
    """keep[e] of the mirror: False for the drop_count edges of smallest (H(e, key(seed, 1)), e)."""
    h = hash_u32(np.arange(num_edges, dtype=np.uint64), key(seed, STREAM_DROP))
    keep = np.ones(num_edges, dtype=bool)
    keep[np.argsort(h, kind="stable")[:drop_count]] = False
    return keep


def drop_edges(edge_index: torch.Tensor, drop_frac: float, seed: int) -> Tuple[torch.Tensor, int]:
    """(edge_index without round(drop_frac · E) uniformly chosen columns, that count).  A count of 0
    returns ``edge_index`` itself; otherwise a new [2, E - count] int64 tensor, columns in input order."""
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    n = drop_count_of(int(edge_index.size(1)), drop_frac)
    return drop_edges_count(edge_index, n, seed), n


def drop_edges_count(edge_index: torch.Tensor, drop_count: int, seed: int) -> torch.Tensor:
    """drop_edges for a given count in [0, E): the kernel for CUDA tensors, the mirror for host tensors."""
    E, n = int(edge_index.size(1)), int(drop_count)
    if n == 0:
        return edge_index
    if not 0 < n < E:
        raise ValueError(f"drop_count {n} outside [0, {E})")
    if not edge_index.is_cuda:
        keep = torch.from_numpy(host_keep_mask(E, n, seed))
        return edge_index.to(torch.int64)[:, keep].contiguous()
    ei = edge_index.to(torch.int64).contiguous()
    out = torch.empty((2, E - n), dtype=torch.int64, device=ei.device)
    lib = _lib.load()
    b = _lib.c_size(0)
    _lib.check(lib.gnn_edge_drop_workspace_size(E, ctypes.byref(b)), "gnn_edge_drop_workspace_size")
    ws = torch.empty(max(int(b.value), 1), dtype=torch.uint8, device=ei.device)
    with torch.cuda.device(ei.device):
        _lib.call("gnn_edge_drop", ei.data_ptr(), E, n, key(seed, STREAM_DROP), out.data_ptr(), ws.data_ptr(),
                  ws.numel(), _lib.stream_handle(ei.device))
    return out


# ----------------------------------------------------------------------------- feature noise
def host_noise(rows: int, cols: int, seed: int) -> np.ndarray:
    """z [rows, cols] of the mirror, in float64."""
    P = (cols + 1) // 2
    if rows * P >= 2 ** 32:
        raise ValueError("add_noise: rows * ceil(F / 2) exceeds the 32-bit counter")
    c = np.arange(rows * P, dtype=np.uint64)
    a = (hash_u32(c, key(seed, STREAM_RADIUS)) >> np.uint32(8)).astype(np.float64)
    b = (hash_u32(c, key(seed, STREAM_ANGLE)) >> np.uint32(8)).astype(np.float64)
    r = np.sqrt(-2.0 * np.log((a + 1.0) * 2.0 ** -24))
    ang = (2.0 * math.pi) * (b * 2.0 ** -24)
    z = np.empty((rows, 2 * P), dtype=np.float64)
    z[:, 0::2] = (r * np.cos(ang)).reshape(rows, P)
    z[:, 1::2] = (r * np.sin(ang)).reshape(rows, P)
    return z[:, :cols]


def _touch(t: torch.Tensor) -> None:
    """Bump t's version counter without launching anything: an in-place op on an empty view of it.
    The kernels write through raw pointers, which autograd's counter does not see, while the package
    keys its per-input caches (planes.py images, their mean(x) half) on (data_ptr, _version)."""
    t.detach()[:0].zero_()


def add_noise(x: torch.Tensor, noise_std: float, seed: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x + noise_std · z for the seeded standard-normal z of the module docstring; ``noise_std`` <= 0
    returns x itself (src/analysis/robustness.py:85-90).  Without ``out`` every call returns a fresh
    tensor; a reused ``out`` (same shape, f32, unit column stride) has its version bumped, so every
    cache keyed on it sees an edited tensor.  A noisy x is not a constant of the run: never
    ``register_input`` it."""
    noise_std = float(noise_std)
    if noise_std <= 0:
        return x
    if x.dim() != 2:
        raise ValueError(f"add_noise: x must be [rows, F], got {tuple(x.shape)}")
    rows, cols = int(x.size(0)), int(x.size(1))
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device):
        raise ValueError("add_noise: out must match x in shape, dtype and device")
    if not x.is_cuda:
        z = torch.from_numpy(host_noise(rows, cols, seed))
        res = (x.detach().to(torch.float64) + noise_std * z).to(x.dtype)
        return res if out is None else out.copy_(res)
    if x.dtype != torch.float32:
        raise TypeError("add_noise: the device path takes float32 features")
    src = x.detach()
    if cols > 0 and src.stride(1) != 1:
        src = src.contiguous()
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    elif cols > 0 and out.stride(1) != 1:
        raise ValueError("add_noise: out needs unit column stride")
    if rows == 0 or cols == 0:
        return out
    with torch.cuda.device(x.device):
        _lib.call("gnn_feature_noise_f32", src.data_ptr(), int(src.stride(0)), rows, cols, noise_std,
                  int(seed) & _M64, out.data_ptr(), int(out.stride(0)), _lib.stream_handle(x.device))
    _touch(out)
    return out


# ----------------------------------------------------------------------------- temperature
def fit_temperature(logits_val: torch.Tensor, y_val: torch.Tensor) -> torch.Tensor:
    """TemperatureScaler.fit (src/utils/calibrate.py:8-30): the T [1] minimising the cross entropy of
    logits_val / T, by one LBFGS step of up to 1000 iterations from T = 1."""
    lv = logits_val.detach()
    yv = y_val.long()
    with torch.enable_grad():
        Tp = torch.ones(1, device=lv.device, requires_grad=True)
        lbfgs = torch.optim.LBFGS([Tp], lr=0.1, max_iter=1000)

        def closure():
            lbfgs.zero_grad()
            l = F.cross_entropy(lv / Tp, yv)
            l.backward()
            return l

        lbfgs.step(closure)
    return Tp.detach()


# ----------------------------------------------------------------------------- a trained run
def check_feature_width(model: torch.nn.Module, state: Dict, in_dim: int) -> None:
    """ValueError naming both widths when ``state`` (a checkpoint) was trained on another feature width
    than the ``in_dim`` columns ``model`` was built for: the first weight matrix of equal rows whose
    column counts differ gives the checkpoint's width.  (The reference's hub ablation pads or truncates
    the features instead, _align_features_to_model; inputs here come from the run's own config.)"""
    for k, w in model.state_dict().items():
        s = state.get(k)
        if s is not None and w.dim() == 2 and s.dim() == 2 and w.size(0) == s.size(0) and w.size(1) != s.size(1):
            raise ValueError(f"the checkpoint expects {int(in_dim) + int(s.size(1)) - int(w.size(1))} input features "
                             f"({k}: {tuple(s.shape)}), the prepared graph has {int(in_dim)}; features are not "
                             "padded or truncated")


class Run:
    """A run directory loaded once: config, decision threshold, prepared inputs and the best model."""

    def __init__(self, run_dir, processed_dir=None, device_eval: Optional[bool] = None, check_width: bool = False):
        from .train_gnn import _model_uses_time_embed, build_model, get_device, load_data
        from .dataset_elliptic import prepare_inputs
        from .planes import register_input

        self.run_dir = Path(run_dir)
        if not self.run_dir.exists():
            raise FileNotFoundError(f"Run directory not found: {self.run_dir}")
        for name in ("config_used.yaml", "metrics.json", "best.ckpt"):
            if not (self.run_dir / name).exists():
                raise FileNotFoundError(f"Expected {name} at {self.run_dir / name}")
        with open(self.run_dir / "config_used.yaml", encoding="utf-8") as f:
            self.cfg = yaml.safe_load(f)
        with open(self.run_dir / "metrics.json", encoding="utf-8") as f:
            base = json.load(f)
        if "threshold" not in base:
            raise KeyError("metrics.json does not contain 'threshold'")
        self.threshold = float(base["threshold"])
        cfg = dict(self.cfg)
        if processed_dir is not None:
            cfg["processed_dir"] = str(processed_dir)
            cfg.pop("graph_file", None)
        self.device = get_device(cfg)
        self.data = prepare_inputs(load_data(cfg), cfg).to(self.device)  # as train_gnn.main prepares them
        register_input(self.data.x)  # the unperturbed features are the run's constant input, as in main
        self.model = build_model(cfg["arch"], self.data.x.size(1), cfg).to(self.device)
        state = torch.load(self.run_dir / "best.ckpt", map_location=self.device, weights_only=True)
        if check_width:
            check_feature_width(self.model, state, int(self.data.x.size(1)))
        self.model.load_state_dict(state)
        self.model.eval()
        self.t_idx = self.data.timestep if _model_uses_time_embed(self.model) else None
        self.calibrate = bool(self.cfg.get("calibrate_temperature", True))
        # the run's ``device_eval`` key unless overridden: temperature fit and record on the device (K17)
        self.device_eval = bool(self.cfg.get("device_eval", False)) if device_eval is None else bool(device_eval)
        self.y_np = self.data.y.cpu().numpy()
        self.test_np = self.data.test_mask.cpu().numpy().astype(bool)
        self.y_test_bin = (self.y_np[self.test_np] == 1).astype(int)

    def evaluate(self, x: torch.Tensor, edge_index: torch.Tensor, edges_dropped: int, drop_frac: float,
                 noise_std: float, seed: int, details: Optional[Dict] = None) -> Dict:
        """One trial on already perturbed inputs: forward (fp32, no_grad), temperature refit on the
        validation logits, test metrics.  ``details`` (a dict) receives logits / probs / temperature.
        With ``device_eval`` the fit is calibrate.fit_temperature and the record
        rank_metrics.evaluation_record on the device probabilities (the same keys)."""
        from .train_gnn import _metrics

        with torch.no_grad():
            logits = self.model(x, edge_index, self.t_idx).float()
        T = None
        vm = self.data.val_mask
        if self.calibrate and bool(vm.any()):
            if self.device_eval:
                from .calibrate import fit_temperature as fit_device

                T = fit_device(logits, self.data.y, mask=vm)
            else:
                T = fit_temperature(logits[vm], self.data.y[vm])
        with torch.no_grad():
            probs = torch.softmax(logits / T if T is not None else logits, dim=1)[:, 1]
        if self.device_eval:
            from . import rank_metrics

            if details is not None:
                details.update(logits=logits, probs=probs.cpu().numpy(), temperature=T, edge_index=edge_index, x=x)
            rec = rank_metrics.evaluation_record(probs, self.data.y, self.data.test_mask, self.threshold,
                                                 self.cfg.get("topk", 100), self.cfg.get("precision_target", 0.90))
        else:
            p_np = probs.cpu().numpy()
            if details is not None:
                details.update(logits=logits, probs=p_np, temperature=T, edge_index=edge_index, x=x)
            rec = _metrics(self.y_test_bin, p_np[self.test_np], self.threshold, self.cfg)
        n0 = int(self.data.edge_index.size(1))
        rec.update(drop_frac_requested=float(drop_frac),
                   drop_frac_effective=float(edges_dropped / n0) if n0 else 0.0,
                   edges_dropped=int(edges_dropped), n_edges_original=n0,
                   n_edges_after_drop=int(edge_index.size(1)), noise_std=float(noise_std),
                   temperature=float(T) if T is not None else 1.0, seed=int(seed))
        return rec

    def trial(self, drop_frac: float, noise_std: float, seed: int, details: Optional[Dict] = None) -> Dict:
        ei, n = drop_edges(self.data.edge_index, drop_frac, seed)
        x = add_noise(self.data.x, noise_std, seed)
        return self.evaluate(x, ei, n, drop_frac, noise_std, seed, details)


def run(run_dir, drop_frac: float, noise_std: float, seed: int, processed_dir=None,
        device_eval: Optional[bool] = None) -> Dict:
    """The reference's tool for one (drop_frac, noise_std, seed): returns the record and writes it to
    ``robustness_drop{drop_frac}_noise{noise_std}.json`` in the run directory.  ``device_eval`` overrides
    the run's config key of that name."""
    drop_frac, noise_std = float(drop_frac), float(noise_std)
    r = Run(run_dir, processed_dir, device_eval)
    rec = r.trial(drop_frac, noise_std, int(seed))
    with open(r.run_dir / f"robustness_drop{drop_frac}_noise{noise_std}.json", "w", encoding="utf-8") as f:
        json.dump(rec, f, indent=2)
    return rec


def _mean_std(vals: List[float]) -> Tuple[float, Optional[float]]:
    a = np.asarray(vals, dtype=np.float64)
    return float(a.mean()), (float(a.std(ddof=1)) if a.size > 1 else None)


def sweep(run_dir, drop_fracs: Iterable[float], noise_stds: Iterable[float], seeds: Iterable[int],
          processed_dir=None, device_eval: Optional[bool] = None) -> Dict:
    """Every (drop_frac, noise_std, seed) trial over one loaded run: edges dropped once per (seed,
    drop_frac) — one graph plan each — and noise added once per (seed, noise_std).  Returns
    {"records": [one per trial], "summary": [per (drop_frac, noise_std): mean and sample standard
    deviation over the seeds of each float metric]} and writes it to ``robustness_sweep.json``."""
    drop_fracs = [float(v) for v in drop_fracs]
    noise_stds = [float(v) for v in noise_stds]
    seeds = [int(s) for s in seeds]
    r = Run(run_dir, processed_dir, device_eval)
    records = []
    for seed in seeds:
        noisy = {ns: add_noise(r.data.x, ns, seed) for ns in noise_stds}
        for df in drop_fracs:
            ei, n = drop_edges(r.data.edge_index, df, seed)
            for ns in noise_stds:
                records.append(r.evaluate(noisy[ns], ei, n, df, ns, seed))
        del noisy
    summary = []
    for df in drop_fracs:
        for ns in noise_stds:
            cell = [rec for rec in records if rec["drop_frac_requested"] == df and rec["noise_std"] == ns]
            stats = {k: _mean_std([rec[k] for rec in cell]) for k in SUMMARY_KEYS}
            summary.append(dict(drop_frac=df, noise_std=ns, n_seeds=len(cell),
                                mean={k: v[0] for k, v in stats.items()},
                                std={k: v[1] for k, v in stats.items()}))
    out = dict(records=records, summary=summary)
    with open(r.run_dir / "robustness_sweep.json", "w", encoding="utf-8") as f:
        json.dump(out, f, indent=2)
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Evaluate robustness of a trained GNN under noise and edge drop")
    ap.add_argument("--run_dir", type=Path, required=True, help="Path to the trained GNN run directory")
    ap.add_argument("--processed_dir", type=Path, default=None,
                    help="Directory containing the processed graph (default: the run's config)")
    ap.add_argument("--drop_frac", type=float, default=0.10, help="Fraction of edges to drop uniformly at random")
    ap.add_argument("--noise_std", type=float, default=0.01, help="Stddev of Gaussian noise added to node features")
    ap.add_argument("--seed", type=int, default=42, help="Random seed")
    ap.add_argument("--drop_fracs", type=float, nargs="+", default=None, help="Sweep: the drop fractions")
    ap.add_argument("--noise_stds", type=float, nargs="+", default=None, help="Sweep: the noise levels")
    ap.add_argument("--seeds", type=int, nargs="+", default=None, help="Sweep: the seeds")
    ap.add_argument("--device_eval", action="store_true", default=None,
                    help="Temperature fit and metrics on the device (default: the run's device_eval key)")
    args = ap.parse_args(argv)
    if args.drop_fracs is not None or args.noise_stds is not None or args.seeds is not None:
        out = sweep(args.run_dir, args.drop_fracs or [args.drop_frac], args.noise_stds or [args.noise_std],
                    args.seeds or [args.seed], args.processed_dir, args.device_eval)
        print(json.dumps(out["summary"], indent=2))
    else:
        print(json.dumps(run(args.run_dir, args.drop_frac, args.noise_std, args.seed, args.processed_dir, args.device_eval),
                         indent=2))


if __name__ == "__main__":
    main()
