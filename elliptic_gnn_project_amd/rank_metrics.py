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

The evaluation record (libgnnmp K17, csrc/calibrate.hip) walks the same order.  P / N the included
positives / negatives; at the end of tie group g with cumulative TP, FP and the group's gTP, gFP:
prec = TP / (TP + FP), rec = TP / P (1.0 when P = 0, as sklearn), f1 = 2.0*prec*rec/(prec+rec+1e-12)
in f64 in exactly that operation order (sklearn's precision_recall_curve points, metrics.py's f1):

* max-F1 threshold: the score of the group of largest f1, the lowest score among equals; 1.0 with
  f1 = 0 without a group (np.nanargmax over the ascending-threshold curve and its appended point);
* precision-target threshold: the lowest score among groups with prec >= target; without one, 1.0 when
  1 >= target (the appended point hits), else the max-F1 threshold;
* recall at precision: the largest rec among groups with prec >= target, else 0.0;
* ROC-AUC = Σ_g gFP·(2·TP − gTP) / (2·P·N): an integer sum and one f64 division; NaN when P or N is 0;
* F1 at a threshold: TP, FP, FN of (double)score >= thr, 2TP / (2TP + FP + FN), 0 for a zero denominator;
  thr must be a float32 value (a score or 1.0), where numpy's f32 comparison agrees with the f64 one;
* ECE: bin = clip(searchsorted(linspace(0, 1, bins + 1), (double)p, "right") - 1, 0, bins - 1), per bin
  count, Σy (integers) and Σp (f64), Σ_b cnt_b / n · |Σy_b / cnt_b − Σp_b / cnt_b| over non-empty bins.

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


# ----------------------------------------------------------------------------- evaluation record (K17)
ECE_BINS = 15  # metrics.expected_calibration_error's default, the only one the project uses
RECORD_KEYS = ("pr_auc_illicit", "roc_auc", "f1_illicit_at_thr", "threshold", "precision_at_k", "recall_at_precision",
               "ece", "n_test")


def _f32_threshold(thr) -> float:
    thr = float(thr)
    if thr != thr or float(np.float32(thr)) != thr:
        raise ValueError(f"rank_metrics: threshold {thr!r} is not a float32 value")
    return thr


def _host_curve(s: np.ndarray, y: np.ndarray, target: float) -> Dict[str, float]:
    """The curve metrics of one segment already in rank order (the module docstring's definitions)."""
    target = float(target)
    if target != target:
        raise ValueError("rank_metrics: precision target is NaN")
    m = int(s.size)
    if m == 0:
        return dict(thr_f1=1.0, f1=0.0, thr_prec=1.0, recall=0.0, roc_auc=float("nan"), P=0, N=0, m=0)
    y = y.astype(np.int64)
    s = s + 0.0
    ends = np.r_[s[1:] != s[:-1], True]
    TP, FP = np.cumsum(y)[ends], np.cumsum(1 - y)[ends]
    gTP, gFP = np.diff(TP, prepend=0), np.diff(FP, prepend=0)
    P, N = int(TP[-1]), int(FP[-1])
    sc = s[ends].astype(np.float64)
    prec = TP.astype(np.float64) / (TP + FP).astype(np.float64)
    rec = TP.astype(np.float64) / float(P) if P > 0 else np.ones(TP.size, dtype=np.float64)
    f1 = 2.0 * prec * rec / (prec + rec + 1e-12)
    i = f1.size - 1 - int(np.argmax(f1[::-1]))  # the largest f1, the lowest score among equals
    hit = np.nonzero(prec >= target)[0]
    if hit.size:
        thr_prec, recall = float(sc[hit[-1]]), float(rec[hit].max())
    else:
        thr_prec, recall = (1.0 if 1.0 >= target else float(sc[i])), 0.0
    auc = int(np.sum(gFP * (2 * TP - gTP)))
    roc = float(auc) / float(2 * P * N) if P > 0 and N > 0 else float("nan")
    return dict(thr_f1=float(sc[i]), f1=float(f1[i]), thr_prec=thr_prec, recall=recall, roc_auc=roc, P=P, N=N, m=m)


def _host_calibration(s: np.ndarray, pos: np.ndarray, inc: np.ndarray, thr: float, bins: int = ECE_BINS) -> Dict:
    """TP / FP / FN at ``thr``, the calibration bins, f1 and ece of the included elements."""
    thr = _f32_threshold(thr)
    p = s[inc].astype(np.float64)
    y = pos[inc].astype(np.int64)
    edges = np.linspace(0.0, 1.0, bins + 1)
    idx = np.clip(np.searchsorted(edges, p, side="right") - 1, 0, bins - 1)
    cnt = np.bincount(idx, minlength=bins).astype(np.int64)
    sy = np.bincount(idx, weights=y, minlength=bins).astype(np.int64)
    sp = np.bincount(idx, weights=p, minlength=bins).astype(np.float64)
    pred = p >= thr
    tp, fp, fn = int(np.sum(pred & (y == 1))), int(np.sum(pred & (y == 0))), int(np.sum(~pred & (y == 1)))
    den = 2 * tp + fp + fn
    n = int(cnt.sum())
    ece = 0.0
    for b in range(bins):
        c = int(cnt[b])
        if c:
            ece += (float(c) / float(n)) * abs(float(sy[b]) / float(c) - float(sp[b]) / float(c))
    return dict(tp=tp, fp=fp, fn=fn, bin_count=cnt, bin_pos=sy, bin_sum=sp,
                f1=float(2 * tp) / float(den) if den > 0 else 0.0, ece=float(ece))


class _EvalBuffers:
    """Outputs and workspaces of the K17 calls of one (device, n)."""

    def __init__(self, device: torch.device, n: int):
        lib = _lib.load()
        f64, i64 = dict(dtype=torch.float64, device=device), dict(dtype=torch.int64, device=device)
        self.curve = torch.empty(_lib.CURVE_OUTPUTS, **f64)
        self.cal = torch.empty(2, **f64)
        self.counts = torch.empty(3, **i64)
        self.bin_count = torch.empty(_lib.CALIB_MAX_BINS, **i64)
        self.bin_pos = torch.empty(_lib.CALIB_MAX_BINS, **i64)
        self.bin_sum = torch.empty(_lib.CALIB_MAX_BINS, **f64)
        b = _lib.c_size(0)
        _lib.check(lib.gnn_rank_curve_workspace_size(n, ctypes.byref(b)), "gnn_rank_curve_workspace_size")
        self.ws_curve = torch.empty(b.value, dtype=torch.uint8, device=device)
        _lib.check(lib.gnn_threshold_calibration_workspace_size(n, _lib.CALIB_MAX_BINS, ctypes.byref(b)),
                   "gnn_threshold_calibration_workspace_size")
        self.ws_cal = torch.empty(b.value, dtype=torch.uint8, device=device)


_EVAL_CACHE: Dict[tuple, _EvalBuffers] = {}


def _eval_buffers(device: torch.device, n: int) -> _EvalBuffers:
    key = (device.index if device.index is not None else torch.cuda.current_device(), n)
    ev = _EVAL_CACHE.get(key)
    if ev is None:
        ev = _EVAL_CACHE[key] = _EvalBuffers(device, n)
    return ev


def _run_curve(buf: _Buffers, ev: _EvalBuffers, positive: torch.Tensor, scores: torch.Tensor, target: float) -> None:
    _lib.call("gnn_rank_curve", _lib.ptr(buf.order), _lib.ptr(buf.flags), _lib.ptr(buf.seg_ptr), _lib.ptr(positive),
              _lib.ptr(scores), buf.n, buf.S, float(target), _lib.ptr(ev.curve), _lib.ptr(ev.ws_curve),
              ev.ws_curve.numel(), _lib.stream_handle(scores.device))


def _run_calibration(ev: _EvalBuffers, scores: torch.Tensor, positive: torch.Tensor, inc: Optional[torch.Tensor],
                     thr: float, bins: int) -> None:
    if not 1 <= int(bins) <= _lib.CALIB_MAX_BINS:
        raise ValueError(f"rank_metrics: bins outside [1, {_lib.CALIB_MAX_BINS}]")
    edges = np.linspace(0.0, 1.0, int(bins) + 1)
    _lib.call("gnn_threshold_calibration", _lib.ptr(scores), _lib.ptr(positive), _lib.ptr(inc), scores.numel(),
              _f32_threshold(thr), edges.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(bins),
              _lib.ptr(ev.counts), _lib.ptr(ev.bin_count), _lib.ptr(ev.bin_pos), _lib.ptr(ev.bin_sum),
              _lib.ptr(ev.cal), _lib.ptr(ev.ws_cal), ev.ws_cal.numel(), _lib.stream_handle(scores.device))


def _device_curve(scores, y, mask, target: float, check: bool):
    """Plan + curve metrics of the included elements; returns (plan buffers, K17 buffers, operands)."""
    scores, y, inc = _device_inputs(scores, y, mask)
    s = scores.detach().to(torch.float32).contiguous()
    buf = _buffers(s.device, s.numel(), 1)
    ev = _eval_buffers(s.device, s.numel())
    _build_plan(buf, s, inc, None)
    pos = _u8(y == 1)
    _run_curve(buf, ev, pos, s, target)
    if check:
        check_status(buf.status)
    return buf, ev, s, pos, _u8(inc)


def _host_sorted(scores, y, mask):
    s, pos, inc = _host_inputs(scores, y, mask)
    o = _host_order(s, inc)
    return s, pos, inc, o


def roc_auc(scores, y, mask=None, check: bool = True):
    """ROC-AUC of ``y == 1`` over the included elements, 0-dim f64; NaN when only one class is present."""
    if _is_device(scores, y):
        return _device_curve(scores, y, mask, 1.0, check)[1].curve[4].clone()
    s, pos, _, o = _host_sorted(scores, y, mask)
    return torch.tensor(_host_curve(s[o], pos[o], 1.0)["roc_auc"], dtype=torch.float64)


def recall_at_precision(scores, y, precision_target: float, mask=None, check: bool = True):
    """The best recall among PR-curve points with precision >= target (0.0 without one), 0-dim f64."""
    if _is_device(scores, y):
        return _device_curve(scores, y, mask, precision_target, check)[1].curve[3].clone()
    s, pos, _, o = _host_sorted(scores, y, mask)
    return torch.tensor(_host_curve(s[o], pos[o], precision_target)["recall"], dtype=torch.float64)


def select_threshold(scores, y, mask=None, precision_target: Optional[float] = None) -> Tuple[float, float]:
    """(decision threshold, the curve's largest F1) as Python floats (device inputs: one read): the
    precision-target threshold when ``precision_target`` > 0, else the max-F1 threshold
    (train_gnn._threshold over metrics.pick_threshold_for_precision / pick_threshold_max_f1)."""
    use_target = bool(precision_target) and float(precision_target) > 0
    target = float(precision_target) if use_target else 1.0
    if _is_device(scores, y):
        buf, ev, *_ = _device_curve(scores, y, mask, target, False)
        got = torch.cat([ev.curve, buf.status.to(torch.float64)]).cpu()
        check_status(got[-1:].to(torch.int32))
        c = dict(thr_f1=float(got[0]), f1=float(got[1]), thr_prec=float(got[2]))
    else:
        s, pos, _, o = _host_sorted(scores, y, mask)
        c = _host_curve(s[o], pos[o], target)
    return (c["thr_prec"] if use_target else c["thr_f1"]), c["f1"]


def _device_calibration(scores, y, mask, thr: float, bins: int) -> _EvalBuffers:
    scores, y, inc = _device_inputs(scores, y, mask)
    s = scores.detach().to(torch.float32).contiguous()
    ev = _eval_buffers(s.device, s.numel())
    _run_calibration(ev, s, _u8(y == 1), _u8(inc), thr, bins)
    return ev


def f1_at_threshold(scores, y, thr: float, mask=None):
    """F1 of ``score >= thr`` over the included elements (0 when nothing is predicted or positive), 0-dim f64."""
    if _is_device(scores, y):
        return _device_calibration(scores, y, mask, thr, ECE_BINS).cal[0].clone()
    s, pos, inc = _host_inputs(scores, y, mask)
    return torch.tensor(_host_calibration(s, pos, inc, thr)["f1"], dtype=torch.float64)


def expected_calibration_error(scores, y, mask=None, bins: int = ECE_BINS):
    """Equal-width-bin ECE of the included elements' positive-class probabilities, 0-dim f64."""
    if _is_device(scores, y):
        return _device_calibration(scores, y, mask, 1.0, bins).cal[1].clone()
    s, pos, inc = _host_inputs(scores, y, mask)
    return torch.tensor(_host_calibration(s, pos, inc, 1.0, bins)["ece"], dtype=torch.float64)


def evaluation_record(scores, y, mask, thr: float, topk: int, precision_target: float) -> Dict:
    """The eight keys of train_gnn._metrics for the included elements at decision threshold ``thr``; {}
    for an empty split.  Device inputs: one plan, the AP / P@k walk, the curve walk and the counting
    pass, every scalar packed into one f64 buffer that is read ONCE together with the status word."""
    k = int(topk)
    if k < 1:
        raise ValueError("evaluation_record: topk < 1")
    thr = _f32_threshold(thr)
    if _is_device(scores, y):
        buf, ev, s, pos, inc = _device_curve(scores, y, mask, precision_target, False)
        _run_ap(buf, pos, k)
        _run_calibration(ev, s, pos, inc, thr, ECE_BINS)
        got = torch.cat([buf.ap[:1], buf.patk[:1], ev.curve, ev.cal, buf.status.to(torch.float64)]).cpu()
        check_status(got[-1:].to(torch.int32))
        v = got.tolist()
        ap, patk, cur, f1, ece = v[0], v[1], v[2:10], v[10], v[11]
        roc, recall, m = cur[4], cur[3], int(cur[7])
    else:
        s, pos, inc, o = _host_sorted(scores, y, mask)
        m = int(o.size)
        c = _host_curve(s[o], pos[o], precision_target)
        cal = _host_calibration(s, pos, inc, thr)
        ap, patk = _host_ap_sorted(s[o], pos[o])[0], _host_patk_sorted(pos[o], k)
        roc, recall, f1, ece = c["roc_auc"], c["recall"], cal["f1"], cal["ece"]
    if m == 0:
        return {}
    return dict(pr_auc_illicit=ap, roc_auc=roc, f1_illicit_at_thr=f1, threshold=thr, precision_at_k=patk,
                recall_at_precision=recall, ece=ece, n_test=m)
