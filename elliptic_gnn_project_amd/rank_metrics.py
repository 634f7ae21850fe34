"""Ranking metrics: average precision, per-group average precision, precision@k and the paired
bootstrap of src/analysis/bootstrap_compare.py — on the device (libgnnmp K14, csrc/rank_metrics.hip)
for CUDA tensors, in numpy for host tensors / arrays.

One arithmetic for both paths (the host path is the kernels' test oracle and is itself pinned
against the reference's sklearn-based metrics, tests/golden/make_bootstrap_golden.py):

* order by score descending, ties by ascending index; tie groups are bit-equal scores (-0.0 == +0.0);
* with integer weights w >= 0 (1 for the plain metrics, the draw counts of a bootstrap replicate),
  TP_g / FP_g the cumulative weighted counts at the end of tie group g and P = TP_last:
  AP = Σ_g (TP_g - TP_{g-1}) / P · TP_g / (TP_g + FP_g) over groups with TP_g + FP_g > 0, in f64;
  P = 0 gives 0.0 (what sklearn returns, with a warning);
* P@k walks the same order taking min(w_i, k - taken) copies of each element: Σ taken_i·y_i / k, with
  k clamped to the total weight.  This is the reference's precision_at_k wherever that is defined
  (its unstable argsort leaves a k-th place inside a mixed-label tie group undefined).

The device path keeps its plan and workspace buffers per (device, n, S, slot) and reuses them; a NaN
score among the included elements sets a bit of a device status word, which ``check_status`` (called
by default, one scalar read) turns into a ValueError.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

BOOT_CHUNK_ELEMS = 1 << 24  # sample indices uploaded per chunk of replicates (64 MiB of int32)


# ----------------------------------------------------------------------------- host path (numpy)
def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _host_order(scores: np.ndarray, include: np.ndarray, segment: Optional[np.ndarray] = None) -> np.ndarray:
    """Included indices by (segment ascending, score descending, index ascending)."""
    idx = np.nonzero(include)[0]
    s = scores[idx] + 0.0  # -0.0 -> +0.0
    if np.isnan(s).any():
        raise ValueError("rank_metrics: NaN score among the included elements")
    keys = (idx, -s) if segment is None else (idx, -s, segment[idx])
    return idx[np.lexsort(keys)]


def _host_ap_sorted(s: np.ndarray, y: np.ndarray, w: Optional[np.ndarray] = None) -> Tuple[float, int, int]:
    """(AP, P, total weight) of one segment already in rank order; y in {0,1}, w integer weights."""
    if s.size == 0:
        return 0.0, 0, 0
    y = y.astype(np.int64)
    w = np.ones_like(y) if w is None else w.astype(np.int64)
    tp = np.cumsum(w * y)
    fp = np.cumsum(w * (1 - y))
    s = s + 0.0
    ends = np.r_[s[1:] != s[:-1], True] & (tp + fp > 0)
    tp_g, fp_g = tp[ends], fp[ends]
    P = int(tp[-1])
    if P == 0:
        return 0.0, 0, int(tp[-1] + fp[-1])
    dtp = np.diff(tp_g, prepend=0).astype(np.float64)
    ap = float(np.sum(dtp / P * (tp_g / (tp_g + fp_g).astype(np.float64))))
    return ap, P, int(tp[-1] + fp[-1])


def _host_patk_sorted(y: np.ndarray, k: int, w: Optional[np.ndarray] = None) -> float:
    if y.size == 0:
        return 0.0
    y = y.astype(np.int64)
    w = np.ones_like(y) if w is None else w.astype(np.int64)
    W = np.cumsum(w)
    if W[-1] == 0:
        return 0.0
    k = min(int(k), int(W[-1]))
    taken = np.clip(k - (W - w), 0, w)
    return float(int(np.sum(taken * y)) / k)


def _host_inputs(scores, y, mask):
    s, yy = _np(scores), _np(y)
    inc = (yy >= 0) if mask is None else _np(mask).astype(bool)
    return s, (yy == 1).astype(np.int64), inc


def host_replicate_metrics(y, scores, sample_idx, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """Weighted AP and P@k of every row of ``sample_idx`` [B, n] (the kernels' oracle)."""
    s, pos = _np(scores), (_np(y) == 1).astype(np.int64)
    n = s.shape[0]
    order = _host_order(s, np.ones(n, dtype=bool))
    ss, ys = s[order], pos[order]
    ap, pk = [], []
    for row in np.asarray(sample_idx):
        w = np.bincount(row, minlength=n)[order]
        ap.append(_host_ap_sorted(ss, ys, w)[0])
        pk.append(_host_patk_sorted(ys, k, w))
    return np.asarray(ap, dtype=np.float64), np.asarray(pk, dtype=np.float64)


# ----------------------------------------------------------------------------- device path
class _Buffers:
    """Plan, outputs and workspaces of one (device, n, S, slot), allocated once and reused."""

    def __init__(self, device: torch.device, n: int, S: int):
        lib = _lib.load()
        self.n, self.S = n, S
        i32 = dict(dtype=torch.int32, device=device)
        self.order = torch.empty(max(n, 1), **i32)
        self.rank = torch.empty(max(n, 1), **i32)
        self.flags = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
        self.seg_ptr = torch.empty(S + 1, **i32)
        self.status = torch.zeros(1, **i32)
        self.ap = torch.empty(max(S, 1), dtype=torch.float64, device=device)
        self.patk = torch.empty(max(S, 1), dtype=torch.float64, device=device)
        self.num_pos = torch.empty(max(S, 1), dtype=torch.int64, device=device)
        self.count = torch.empty(max(S, 1), dtype=torch.int64, device=device)
        b = _lib.c_size(0)
        _lib.check(lib.gnn_rank_plan_workspace_size(n, S, ctypes.byref(b)), "gnn_rank_plan_workspace_size")
        self.ws_plan = torch.empty(b.value, dtype=torch.uint8, device=device)
        _lib.check(lib.gnn_rank_ap_workspace_size(n, S, ctypes.byref(b)), "gnn_rank_ap_workspace_size")
        self.ws_ap = torch.empty(b.value, dtype=torch.uint8, device=device)


_CACHE: Dict[tuple, _Buffers] = {}
_BOOT_WS: Dict[tuple, torch.Tensor] = {}


def _buffers(device: torch.device, n: int, S: int, slot: str = "a") -> _Buffers:
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), n, S, slot)
    buf = _CACHE.get(key)
    if buf is None:
        buf = _CACHE[key] = _Buffers(device, n, S)
    return buf


def _u8(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else (t != 0).view(torch.uint8)


def _build_plan(buf: _Buffers, scores: torch.Tensor, include: Optional[torch.Tensor],
                segment: Optional[torch.Tensor]) -> None:
    """Fill buf's plan from scores (zeroes its status word first)."""
    s = scores.detach().to(torch.float32).contiguous()
    inc = _u8(include)
    seg = None if segment is None else segment.to(torch.int32).contiguous()
    buf.status.zero_()
    _lib.call("gnn_rank_plan_build", _lib.ptr(s), _lib.ptr(inc), _lib.ptr(seg), buf.n, buf.S, _lib.ptr(buf.order),
              _lib.ptr(buf.flags), _lib.ptr(buf.seg_ptr), _lib.ptr(buf.rank), _lib.ptr(buf.status),
              _lib.ptr(buf.ws_plan), buf.ws_plan.numel(), _lib.stream_handle(s.device))


def _run_ap(buf: _Buffers, positive: torch.Tensor, k: int) -> None:
    _lib.call("gnn_rank_ap", _lib.ptr(buf.order), _lib.ptr(buf.flags), _lib.ptr(buf.seg_ptr), _lib.ptr(positive),
              buf.n, buf.S, int(k), _lib.ptr(buf.ap), _lib.ptr(buf.num_pos), _lib.ptr(buf.count),
              _lib.ptr(buf.patk) if k >= 1 else None, _lib.ptr(buf.ws_ap), buf.ws_ap.numel(),
              _lib.stream_handle(positive.device))


def check_status(status: torch.Tensor) -> None:
    """Raise for the bits a rank call left in its device status word (reads one int: a sync)."""
    st = int(status.reshape(-1)[0])
    if st & _lib.RANK_STATUS_NAN:
        raise ValueError("rank_metrics: NaN score among the included elements")
    if st & _lib.RANK_STATUS_SEGMENT:
        raise IndexError("rank_metrics: group id outside the plan's range")
    if st & _lib.RANK_STATUS_INDEX:
        raise IndexError("rank_metrics: bootstrap sample index outside [0, n)")


def _device_inputs(scores, y, mask, *more):
    """Every operand as a flat tensor of the same length on the CUDA device involved."""
    dev = next(t.device for t in (scores, y, mask) + more if isinstance(t, torch.Tensor) and t.is_cuda)
    scores = torch.as_tensor(scores).to(dev).reshape(-1)
    n = scores.numel()
    rest = [None if t is None else torch.as_tensor(t).to(dev).reshape(-1) for t in (y, mask) + more]
    for t in rest:
        if t is not None and t.numel() != n:
            raise ValueError(f"rank_metrics: operand of {t.numel()} elements for {n} scores")
    y, mask = rest[0], rest[1]
    inc = (y >= 0) if mask is None else mask.bool()
    return (scores, y, inc) + tuple(rest[2:])


def _device_metric(scores, y, mask, k: int, check: bool):
    scores, y, inc = _device_inputs(scores, y, mask)
    buf = _buffers(scores.device, scores.numel(), 1)
    _build_plan(buf, scores, inc, None)
    _run_ap(buf, _u8(y == 1), k)
    if check:
        check_status(buf.status)
    return buf


def _is_device(*ts) -> bool:
    return any(isinstance(t, torch.Tensor) and t.is_cuda for t in ts)


def average_precision(scores, y, mask=None, check: bool = True, return_status: bool = False):
    """Average precision of ``y == 1`` over the included elements (``mask``, default ``y >= 0``) as a
    0-dim f64 tensor — on the scores' device, with no host transfer when ``check`` is false.
    ``return_status`` also returns the call's device status word (for a caller that reads both at once)."""
    if _is_device(scores, y):
        buf = _device_metric(scores, y, mask, 0, check)
        out = buf.ap[0].clone()
        return (out, buf.status.clone()) if return_status else out
    s, pos, inc = _host_inputs(scores, y, mask)
    o = _host_order(s, inc)
    out = torch.tensor(_host_ap_sorted(s[o], pos[o])[0], dtype=torch.float64)
    return (out, torch.zeros(1, dtype=torch.int32)) if return_status else out


def precision_at_k(scores, y, k: int, mask=None, check: bool = True):
    """Mean of ``y == 1`` over the min(k, included) highest scores (ties by ascending index), 0-dim f64."""
    if int(k) < 1:
        raise ValueError("precision_at_k: k < 1")
    if _is_device(scores, y):
        return _device_metric(scores, y, mask, int(k), check).patk[0].clone()
    s, pos, inc = _host_inputs(scores, y, mask)
    o = _host_order(s, inc)
    return torch.tensor(_host_patk_sorted(pos[o], int(k)), dtype=torch.float64)


def average_precision_by_group(scores, y, group, mask=None, check: bool = True):
    """(group values ascending, ap[S], count[S]) over the included elements' groups; a group without a
    positive has AP 0.0.  Device inputs: one sort for all groups; the group values are read to size S."""
    if _is_device(scores, y):
        scores, y, inc, group = _device_inputs(scores, y, mask, group)
        dev = scores.device
        vals = torch.unique(group[inc])  # sorted; its length sizes the plan (one sync)
        S = int(vals.numel())
        if S == 0:
            return vals, torch.empty(0, dtype=torch.float64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
        seg = torch.searchsorted(vals, group).clamp_(max=S - 1)
        buf = _buffers(dev, scores.numel(), S)
        _build_plan(buf, scores, inc, seg)
        _run_ap(buf, _u8(y == 1), 0)
        if check:
            check_status(buf.status)
        return vals, buf.ap[:S].clone(), buf.count[:S].clone()
    s, pos, inc = _host_inputs(scores, y, mask)
    g = _np(group)
    vals = np.unique(g[inc])
    ap, cnt = [], []
    for v in vals:
        o = _host_order(s, inc & (g == v))
        ap.append(_host_ap_sorted(s[o], pos[o])[0])
        cnt.append(o.size)
    return (torch.as_tensor(vals), torch.tensor(ap, dtype=torch.float64), torch.tensor(cnt, dtype=torch.int64))


def replicate_metrics(y, scores_a, scores_b, sample_idx, k: int, check: bool = True):
    """Per-replicate (ap_a, ap_b, patk_a, patk_b), f64 [B], of sample_idx [B, n] — on the device for
    CUDA scores (sample_idx is uploaded), else the host path."""
    if not _is_device(scores_a, scores_b):
        ap_a, pk_a = host_replicate_metrics(y, scores_a, sample_idx, k)
        ap_b, pk_b = host_replicate_metrics(y, scores_b, sample_idx, k)
        return tuple(torch.from_numpy(v) for v in (ap_a, ap_b, pk_a, pk_b))
    scores_a, y, _, scores_b = _device_inputs(scores_a, y, None, scores_b)
    dev = scores_a.device
    n = scores_a.numel()
    idx = torch.as_tensor(np.ascontiguousarray(sample_idx, dtype=np.int32)) if not isinstance(sample_idx, torch.Tensor) \
        else sample_idx.to(torch.int32)
    if n == 0 or idx.numel() % n:
        raise ValueError("replicate_metrics: sample_idx is not [B, n]")
    idx = idx.to(dev).contiguous().view(-1, n)
    B = idx.size(0)
    if B >= 65536:
        raise ValueError("replicate_metrics: at most 65535 replicates per call")
    pa, pb = _buffers(dev, n, 1, "a"), _buffers(dev, n, 1, "b")
    _build_plan(pa, scores_a, None, None)
    _build_plan(pb, scores_b, None, None)
    pos = _u8(y == 1)
    lib = _lib.load()
    b = _lib.c_size(0)
    _lib.check(lib.gnn_rank_bootstrap_workspace_size(n, B, ctypes.byref(b)), "gnn_rank_bootstrap_workspace_size")
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), n)
    ws = _BOOT_WS.get(key)
    if ws is None or ws.numel() < b.value:
        ws = _BOOT_WS[key] = torch.empty(b.value, dtype=torch.uint8, device=dev)
    out = torch.empty(4, B, dtype=torch.float64, device=dev)
    status = pa.status  # the bootstrap call adds its bits to plan A's word; plan B's is checked too
    _lib.call("gnn_rank_bootstrap", _lib.ptr(pa.order), _lib.ptr(pa.rank), _lib.ptr(pa.flags), _lib.ptr(pb.order),
              _lib.ptr(pb.rank), _lib.ptr(pb.flags), _lib.ptr(pos), _lib.ptr(idx), n, B, int(k), _lib.ptr(out[0]),
              _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(out[3]), _lib.ptr(status), _lib.ptr(ws), ws.numel(),
              _lib.stream_handle(dev))
    if check:
        check_status(pa.status | pb.status)
    return out[0], out[1], out[2], out[3]


def paired_bootstrap(y, scores_a, scores_b, topk: int, n_boot: int, seed: Optional[int] = 42) -> Dict:
    """The reference's paired_bootstrap (src/analysis/bootstrap_compare.py:58-93) for two runs over the
    same samples: ``delta_pr_auc`` / ``delta_p_at_k`` of B - A, each {delta, ci_low, ci_high}.  The
    sample indices are drawn on the host exactly as the reference draws them (one
    ``default_rng(seed).choice(n, size=n, replace=True)`` per replicate, in order) and uploaded in
    bounded chunks of replicates; the per-replicate metrics run on the scores' device (CUDA) or in
    numpy (host inputs); mean and percentiles are taken on the host."""
    n = int(scores_a.shape[0])
    k = min(int(topk), n)
    if k < 1 or int(n_boot) < 1:
        raise ValueError("paired_bootstrap: topk < 1, n_boot < 1 or no samples")
    rng = np.random.default_rng(seed)
    chunk = int(max(1, min(int(n_boot), BOOT_CHUNK_ELEMS // max(n, 1), 65535)))
    d_ap, d_pk = [], []
    done = 0
    while done < int(n_boot):
        bc = min(chunk, int(n_boot) - done)
        idx = np.stack([rng.choice(n, size=n, replace=True) for _ in range(bc)]).astype(np.int32)
        ap_a, ap_b, pk_a, pk_b = replicate_metrics(y, scores_a, scores_b, idx, k)
        d_ap.append((ap_b - ap_a).cpu().numpy())
        d_pk.append((pk_b - pk_a).cpu().numpy())
        done += bc
    d_ap, d_pk = np.concatenate(d_ap), np.concatenate(d_pk)

    def summarize(d: np.ndarray) -> Dict[str, float]:
        lo, hi = np.percentile(d, [2.5, 97.5])
        return {"delta": float(np.mean(d)), "ci_low": float(lo), "ci_high": float(hi)}

    return {"delta_pr_auc": summarize(d_ap), "delta_p_at_k": summarize(d_pk)}
