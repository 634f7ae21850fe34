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

The run reports (libgnnmp K19, csrc/report.hip; the tools eval_by_time, workload_curves, calibration_plots,
evaluate_ensemble) add: the hits of a whole list of k from one plan (``precision_curve``), TP / FP / FN and
the count per group at a threshold (``threshold_counts_by_group``, ``by_time_table``), the reliability
table from the ECE's bins (``reliability_table``), the join of two runs by node id (``join_by_id``) and the
two-run ensemble (``ensemble_pair``: 0.5·(a + b) in f32, or the closed form r / (r + q), r = √(a·b),
q = √((1−a)·(1−b)) of σ(½(logit a + logit b)) in f64 with every operation rounded once).

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


def average_precision_by_group(scores, y, group, mask=None, check: bool = True, device_order: bool = False):
    """(group values ascending, ap[S], count[S]) over the included elements' groups; a group without a
    positive has AP 0.0.  Device inputs: one sort for all groups; the group values are read to size S.
    ``device_order`` (host inputs): add the AP terms in the kernel's order — the device path's bits."""
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
    if device_order and vals.size:
        ss, ys, seg_ptr, _ = _host_plan(s, _np(y), inc, np.searchsorted(vals, g).clip(max=vals.size - 1), int(vals.size))
        return (torch.as_tensor(vals), torch.from_numpy(_host_plan_ap(ss, ys, seg_ptr)),
                torch.from_numpy(np.diff(seg_ptr).astype(np.int64)))
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


def evaluation_record(scores, y, mask, thr: float, topk: int, precision_target: float,
                      device_order: bool = False) -> Dict:
    """The eight keys of train_gnn._metrics for the included elements at decision threshold ``thr``; {}
    for an empty split.  Device inputs: one plan, the AP / P@k walk, the curve walk and the counting
    pass, every scalar packed into one f64 buffer that is read ONCE together with the status word.
    ``device_order`` (host inputs): add the AP terms and the calibration bins' sums in the kernels' order —
    the device path's bits for ``pr_auc_illicit`` and ``ece`` (the other keys have them anyway)."""
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
        if device_order:
            cal = _host_calibration_device_order(s, pos, inc, thr)
            ap = float(_host_plan_ap(s[o].astype(np.float32), pos[o], np.array([0, m], dtype=np.int64))[0])
        roc, recall, f1, ece = c["roc_auc"], c["recall"], cal["f1"], cal["ece"]
    if m == 0:
        return {}
    return dict(pr_auc_illicit=ap, roc_auc=roc, f1_illicit_at_thr=f1, threshold=thr, precision_at_k=patk,
                recall_at_precision=recall, ece=ece, n_test=m)


# ----------------------------------------------------------------------------- run reports (K19)
# The tools that read a finished run directory (eval_by_time, workload_curves, calibration_plots,
# evaluate_ensemble) write their numbers with repr(): for the device path and the host path to write the
# same bytes, the two f64 sums of this module that depend on the summation order — the AP terms and the
# calibration bins' Σp — have host forms that add in the kernels' order (``_host_plan_ap``,
# ``_host_calibration_device_order``).  Everything else is integer counts and single IEEE operations.
ENSEMBLE_MODES = {"prob": _lib.ENSEMBLE_PROB, "logit": _lib.ENSEMBLE_LOGIT}
_CLIP_LO, _CLIP_HI = np.float32(1e-6), np.float32(1.0 - 1e-6)  # np.clip(p, 1e-6, 1 - 1e-6) on f32 data
_WS: Dict[tuple, torch.Tensor] = {}


def _workspace(device: torch.device, name: str, nbytes: int) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), name)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    return ws


def _part_scan_tiles(term: np.ndarray, seg: np.ndarray):
    """gnn_rank_ap's segmented f64 scan over tiles of GNN_RANK_TILE positions, add by add: 4 positions per
    thread in sequence, a shuffle scan over the 64 lanes of each wave, the waves' totals in wave order.
    term / seg [nb, 256, 4]; returns the inclusive (sum, seg) of every position."""
    def pop(asum, aseg, bsum, bseg):
        return np.where(bseg, bsum, asum + bsum), aseg | bseg

    psum, pseg = term.copy(), seg.copy()
    for j in range(1, 4):
        psum[:, :, j], pseg[:, :, j] = pop(psum[:, :, j - 1], pseg[:, :, j - 1], psum[:, :, j], pseg[:, :, j])
    nb = term.shape[0]
    isum, iseg = psum[:, :, 3].reshape(nb, 4, 64).copy(), pseg[:, :, 3].reshape(nb, 4, 64).copy()
    d = 1
    while d < 64:
        nsum, nseg = pop(isum[:, :, :-d], iseg[:, :, :-d], isum[:, :, d:], iseg[:, :, d:])
        isum[:, :, d:], iseg[:, :, d:] = nsum, nseg
        d *= 2
    esum, eseg = np.zeros_like(isum), np.zeros_like(iseg)
    esum[:, :, 1:], eseg[:, :, 1:] = isum[:, :, :-1], iseg[:, :, :-1]
    xsum, xseg = np.empty_like(isum), np.empty_like(iseg)
    pre_s, pre_g = np.zeros(nb), np.zeros(nb, dtype=bool)
    for w in range(4):
        xsum[:, w, :], xseg[:, w, :] = pop(pre_s[:, None], pre_g[:, None], esum[:, w, :], eseg[:, w, :])
        pre_s, pre_g = pop(pre_s, pre_g, isum[:, w, 63], iseg[:, w, 63])
    xsum, xseg = xsum.reshape(nb, 256, 1), xseg.reshape(nb, 256, 1)
    return pop(xsum, xseg, psum, pseg)


def _host_plan_ap(s: np.ndarray, y: np.ndarray, seg_ptr: np.ndarray) -> np.ndarray:
    """ap[S] of a plan (s, y in plan order; seg_ptr[S + 1]) with gnn_rank_ap's operations in its order:
    the term gTP·(TP / (TP + FP)) at every tie group's end, the terms added as the kernel's scan adds them,
    the tiles' shares in tile order, one division by P.  The device path's bits."""
    T = _lib.RANK_TILE
    S, m = int(seg_ptr.size) - 1, int(seg_ptr[-1])
    ap = np.zeros(S, dtype=np.float64)
    if m == 0:
        return ap
    y = y[:m].astype(np.int64)
    s = s[:m] + np.float32(0.0)
    seg_id = np.repeat(np.arange(S), np.diff(seg_ptr))
    seg_start = np.zeros(m, dtype=bool)
    seg_start[seg_ptr[:-1][np.diff(seg_ptr) > 0]] = True
    grp_start = seg_start | np.r_[True, s[1:] != s[:-1]]
    grp_end = np.r_[grp_start[1:], True]
    cy = np.cumsum(y)
    before_seg = (cy - y)[seg_ptr[:-1].clip(max=m - 1)][seg_id]  # positives before the element's segment
    tp = cy - before_seg
    seen = np.arange(m) - seg_ptr[:-1][seg_id] + 1
    gfirst = np.maximum.accumulate(np.where(grp_start, np.arange(m), 0))
    gtp = cy - (cy - y)[gfirst]
    term = np.where(grp_end, gtp.astype(np.float64) * (tp.astype(np.float64) / seen.astype(np.float64)), 0.0)
    nb = -(-m // T)
    pad = nb * T - m
    qsum, qseg = _part_scan_tiles(np.r_[term, np.zeros(pad)].reshape(nb, 256, 4),
                                  np.r_[seg_start, np.zeros(pad, dtype=bool)].reshape(nb, 256, 4))
    qsum, qseg = qsum.reshape(-1), qseg.reshape(-1)
    for g in range(S):
        lo, hi = int(seg_ptr[g]), int(seg_ptr[g + 1])
        if hi <= lo:
            continue
        b0, b1 = lo // T, (hi - 1) // T
        total = qsum[min(hi, (b0 + 1) * T) - 1]  # from the segment's start to its end or its tile's end
        for b in range(b0 + 1, b1 + 1):
            total = total + qsum[min(hi, (b + 1) * T) - 1]
        P = int(tp[hi - 1])
        ap[g] = total / float(P) if P > 0 else 0.0
    return ap


def _host_plan(scores, y, mask, segment: Optional[np.ndarray] = None, S: int = 1):
    """(scores, positives) in plan order and seg_ptr, as gnn_rank_plan_build lays them out."""
    s, pos, inc = _host_inputs(scores, y, mask)
    o = _host_order(s, inc, segment)
    counts = np.bincount(segment[o], minlength=S) if segment is not None else np.array([o.size])
    return s[o].astype(np.float32), pos[o], np.r_[0, np.cumsum(counts)].astype(np.int64), o


def _host_calibration_device_order(s: np.ndarray, pos: np.ndarray, inc: np.ndarray, thr: float,
                                   bins: int = ECE_BINS) -> Dict:
    """_host_calibration with the bins' Σp added as gnn_threshold_calibration adds them: per block of 4096
    elements a column per (bin, thread) in element order, the 128 columns folded pairwise and by a
    butterfly, the blocks in block order.  The device path's bits."""
    out = _host_calibration(s, pos, inc, thr, bins)
    n = int(s.size)
    TB, ITEMS = 128, 32
    nb = -(-n // (TB * ITEMS)) if n else 0
    edges = np.linspace(0.0, 1.0, bins + 1)
    p = np.zeros(nb * TB * ITEMS, dtype=np.float64)
    p[:n] = s.astype(np.float64)
    live = np.zeros(p.size, dtype=bool)
    live[:n] = inc
    idx = np.clip(np.searchsorted(edges, p, side="right") - 1, 0, bins - 1)
    p, live, idx = (a.reshape(nb, ITEMS, TB) for a in (p, live, idx))
    sums = np.zeros((nb, bins, TB), dtype=np.float64)
    blk, tid = np.meshgrid(np.arange(nb), np.arange(TB), indexing="ij")
    for j in range(ITEMS):
        k = live[:, j, :]
        sums[blk[k], idx[:, j, :][k], tid[k]] += p[:, j, :][k]
    v = sums[:, :, :64] + sums[:, :, 64:]
    lane = np.arange(64)
    step = 32
    while step:
        v = v + v[:, :, lane ^ step]
        step //= 2
    total = np.zeros(bins, dtype=np.float64)
    for b in range(nb):
        total = total + v[b, :, 0]
    cnt, sy = out["bin_count"], out["bin_pos"]
    ece, m = 0.0, int(cnt.sum())
    for b in range(bins):
        c = int(cnt[b])
        if c:
            ece += (float(c) / float(m)) * abs(float(sy[b]) / float(c) - float(total[b]) / float(c))
    out.update(bin_sum=total, ece=float(ece))
    return out


def _report_status(st: int) -> None:
    check_status(torch.tensor([st & 7], dtype=torch.int32))
    if st & _lib.REPORT_STATUS_K:
        raise ValueError("rank_metrics: k < 1")


def precision_curve(scores, y, ks, mask=None, check: bool = True):
    """(k_eff int64 [K], hits int64 [K], precision f64 [K]) for a list of k >= 1 over the included elements:
    k_eff = min(k, m), hits the positives among the k_eff highest scores (ties by ascending index, as
    ``precision_at_k``), precision = hits / k_eff, NaN when nothing is included.  Device inputs: one plan,
    one scan (libgnnmp K19), tensors on the scores' device."""
    if _is_device(scores, y):
        scores, y, inc = _device_inputs(scores, y, mask)
        dev, n = scores.device, scores.numel()
        kt = torch.as_tensor(ks, dtype=torch.int64).to(dev).reshape(-1).contiguous()
        K = int(kt.numel())
        k_eff = torch.empty(K, dtype=torch.int64, device=dev)
        hits = torch.empty(K, dtype=torch.int64, device=dev)
        prec = torch.empty(K, dtype=torch.float64, device=dev)
        if K == 0:
            return k_eff, hits, prec
        buf = _buffers(dev, n, 1)
        _build_plan(buf, scores, inc, None)
        b = _lib.c_size(0)
        _lib.check(_lib.load().gnn_rank_hits_at_workspace_size(n, ctypes.byref(b)), "gnn_rank_hits_at_workspace_size")
        ws = _workspace(dev, "hits", b.value)
        _lib.call("gnn_rank_hits_at", _lib.ptr(buf.order), _lib.ptr(buf.seg_ptr), _lib.ptr(_u8(y == 1)), n, 1,
                  _lib.ptr(kt), K, _lib.ptr(k_eff), _lib.ptr(hits), _lib.ptr(prec), _lib.ptr(buf.status), _lib.ptr(ws),
                  ws.numel(), _lib.stream_handle(dev))
        if check:
            _report_status(int(buf.status[0]))
        return k_eff, hits, prec
    s, pos, inc = _host_inputs(scores, y, mask)
    kk = np.asarray(_np(ks), dtype=np.int64).reshape(-1)
    if (kk < 1).any():
        raise ValueError("rank_metrics: k < 1")
    o = _host_order(s, inc)
    m = int(o.size)
    k_eff = np.minimum(kk, m)
    cum = np.r_[0, np.cumsum(pos[o])].astype(np.int64)
    hits = cum[k_eff]
    with np.errstate(invalid="ignore", divide="ignore"):
        prec = np.where(k_eff > 0, hits.astype(np.float64) / k_eff.astype(np.float64), np.nan)
    return torch.from_numpy(k_eff), torch.from_numpy(hits), torch.from_numpy(prec)


def segment_threshold_counts(scores, y, segment, S: int, thr: float, mask=None, check: bool = True):
    """(counts int64 [S, 4], status word) — per segment id in [0, S) the TP, FP, FN of ``score >= thr`` and
    the number of included elements.  An included element with a segment outside [0, S) is skipped and
    sets RANK_STATUS_SEGMENT (an IndexError when ``check``).  ``thr`` must be a float32 value."""
    thr, S = _f32_threshold(thr), int(S)
    if not 0 <= S <= _lib.REPORT_MAX_SEGMENTS:
        raise ValueError(f"rank_metrics: {S} groups outside [0, {_lib.REPORT_MAX_SEGMENTS}]")
    if _is_device(scores, y):
        scores, y, inc, segment = _device_inputs(scores, y, mask, segment)
        dev, n = scores.device, scores.numel()
        s = scores.detach().to(torch.float32).contiguous()
        seg = segment.to(torch.int32).contiguous()
        counts = torch.zeros(S, 4, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        b = _lib.c_size(0)
        _lib.check(_lib.load().gnn_segment_threshold_counts_workspace_size(n, S, ctypes.byref(b)),
                   "gnn_segment_threshold_counts_workspace_size")
        ws = _workspace(dev, "segcounts", b.value)
        _lib.call("gnn_segment_threshold_counts", _lib.ptr(s), _lib.ptr(_u8(y == 1)), _lib.ptr(_u8(inc)), _lib.ptr(seg),
                  n, S, thr, _lib.ptr(counts), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
        if check:
            check_status(status)
        return counts, status
    s, pos, inc = _host_inputs(scores, y, mask)
    seg = _np(segment).astype(np.int64)
    ok = inc & (seg >= 0) & (seg < S)
    status = int(_lib.RANK_STATUS_SEGMENT) if bool((inc & ~ok).any()) else 0
    pred = s.astype(np.float64) >= thr
    cols = (pred & (pos == 1), pred & (pos == 0), ~pred & (pos == 1), np.ones_like(pred))
    counts = np.stack([np.bincount(seg[ok & c], minlength=S)[:S] for c in cols], axis=1).astype(np.int64)
    st = torch.tensor([status], dtype=torch.int32)
    if check:
        check_status(st)
    return torch.from_numpy(counts.reshape(S, 4)), st


def _group_mapping(group, inc):
    """(group values ascending, segment id of every element) over the included elements' groups — the
    mapping of ``average_precision_by_group``.  Device tensors or numpy arrays."""
    if isinstance(group, torch.Tensor):
        vals = torch.unique(group[inc])  # sorted; its length sizes the plan (one sync)
        S = int(vals.numel())
        return vals, (torch.searchsorted(vals, group).clamp_(max=max(S - 1, 0)) if S else torch.zeros_like(group))
    vals = np.unique(group[inc])
    S = int(vals.size)
    return vals, (np.searchsorted(vals, group).clip(max=max(S - 1, 0)) if S else np.zeros_like(group))


def threshold_counts_by_group(scores, y, group, thr: float, mask=None):
    """(group values ascending, counts int64 [S, 4]: TP, FP, FN at ``thr`` and the element count) over the
    included elements' groups; the mapping is ``average_precision_by_group``'s."""
    if _is_device(scores, y):
        scores, y, inc, group = _device_inputs(scores, y, mask, group)
        vals, seg = _group_mapping(group, inc)
        return vals, segment_threshold_counts(scores, y, seg, int(vals.numel()), thr, inc)[0]
    s, yy = _np(scores), _np(y)
    inc = (yy >= 0) if mask is None else _np(mask).astype(bool)
    vals, seg = _group_mapping(_np(group), inc)
    return torch.as_tensor(vals), segment_threshold_counts(s, yy, seg, int(vals.size), thr, inc)[0]


def _f1_of_counts(tp: int, fp: int, fn: int) -> float:
    den = 2 * tp + fp + fn
    return float(2 * tp) / float(den) if den > 0 else 0.0


def by_time_table(scores, y, timestep, thr: float, mask=None):
    """Rows {timestep, pr_auc_illicit, f1_illicit_at_thr, n} per timestep of the included elements, ascending
    (src/analysis/eval_by_time.py's table): the segmented average precision and the per-group threshold
    counts over ONE mapping; F1 = 2TP / (2TP + FP + FN), 0.0 for a zero denominator (sklearn's
    zero_division=0); a timestep without a positive has AP 0.0 (what sklearn returns, with a warning).
    Device inputs: after the mapping's size, one host read of every number.  The host path adds the AP
    terms in the kernel's order: both paths return the same bits."""
    thr = _f32_threshold(thr)
    if _is_device(scores, y):
        scores, y, inc, group = _device_inputs(scores, y, mask, timestep)
        if group.is_floating_point():
            raise TypeError("by_time_table: timesteps must be integers")
        vals, seg = _group_mapping(group, inc)
        S = int(vals.numel())
        if S == 0:
            return []
        buf = _buffers(scores.device, scores.numel(), S)
        _build_plan(buf, scores, inc, seg)
        _run_ap(buf, _u8(y == 1), 0)
        counts, st = segment_threshold_counts(scores, y, seg, S, thr, inc, check=False)
        f64 = torch.float64
        got = torch.cat([buf.ap[:S], counts.reshape(-1).to(f64), vals.to(f64), (buf.status | st).to(f64)]).cpu()
        check_status(got[-1:].to(torch.int32))
        ap, cnt, tv = got[:S].tolist(), got[S:5 * S].to(torch.int64).reshape(S, 4).tolist(), got[5 * S:6 * S].tolist()
    else:
        g = _np(timestep)
        if g.dtype.kind not in "iu":
            raise TypeError("by_time_table: timesteps must be integers")
        s, pos, inc = _host_inputs(scores, y, mask)
        vals, seg = _group_mapping(g, inc)
        S = int(vals.size)
        if S == 0:
            return []
        ss, ys, seg_ptr, _ = _host_plan(s, _np(y), inc, seg, S)
        ap = _host_plan_ap(ss, ys, seg_ptr).tolist()
        cnt = segment_threshold_counts(s, _np(y), seg, S, thr, inc)[0].tolist()
        tv = vals.tolist()
    return [dict(timestep=int(tv[g]), pr_auc_illicit=float(ap[g]), f1_illicit_at_thr=_f1_of_counts(*cnt[g][:3]),
                 n=int(cnt[g][3])) for g in range(S)]


def reliability_table(scores, y, mask=None, bins: int = ECE_BINS) -> Dict:
    """The reliability diagram's numbers over the included elements, per NON-EMPTY equal-width bin:
    ``bin_center`` ((edges[b] + edges[b+1]) / 2 of linspace(0, 1, bins + 1)), ``count``, ``accuracy``
    (positives / count) and ``confidence`` (Σp / count), and the ``ece`` — all from
    gnn_threshold_calibration's bins (K17), no further kernel.  src/analysis/calibration_plots.py drops a
    score outside [0, 1]; this clips it into the end bins, as the ECE of this module does.  Softmax
    probabilities never leave [0, 1], so the two agree on every run directory.  The host path adds Σp in
    the kernel's order: both paths return the same bits."""
    bins = int(bins)
    if not 1 <= bins <= _lib.CALIB_MAX_BINS:
        raise ValueError(f"rank_metrics: bins outside [1, {_lib.CALIB_MAX_BINS}]")
    if _is_device(scores, y):
        ev = _device_calibration(scores, y, mask, 1.0, bins)
        f64 = torch.float64
        got = torch.cat([ev.bin_count[:bins].to(f64), ev.bin_pos[:bins].to(f64), ev.bin_sum[:bins], ev.cal[1:2]]).cpu()
        got = got.numpy()
        cnt, sy, sp, ece = got[:bins].astype(np.int64), got[bins:2 * bins].astype(np.int64), got[2 * bins:3 * bins], got[-1]
    else:
        s, pos, inc = _host_inputs(scores, y, mask)
        c = _host_calibration_device_order(s, pos, inc, 1.0, bins)
        cnt, sy, sp, ece = c["bin_count"], c["bin_pos"], c["bin_sum"], c["ece"]
    edges = np.linspace(0.0, 1.0, bins + 1)
    keep = cnt > 0
    cf = cnt[keep].astype(np.float64)
    return dict(bin_center=((edges[:-1] + edges[1:]) / 2.0)[keep], count=cnt[keep],
                accuracy=sy[keep].astype(np.float64) / cf, confidence=sp[keep] / cf, ece=float(ece))


def join_by_id(base_ids, other_ids, what: str = "") -> torch.Tensor:
    """perm (int32) with ``other_ids[perm[i]] == base_ids[i]`` for two arrays of the same distinct,
    non-negative int64 ids; bit-equal arrays give the identity without a sort (the reference's _align).
    RuntimeError naming ``what`` (the split) for a duplicate or negative id and for two different id sets
    (the reference's "node indices differ between runs").  CUDA tensors: two radix sorts (libgnnmp K19)."""
    label = f"{what} " if what else ""
    if _is_device(base_ids, other_ids):
        dev = next(t.device for t in (base_ids, other_ids) if isinstance(t, torch.Tensor) and t.is_cuda)
        a = torch.as_tensor(base_ids).to(dev).reshape(-1).to(torch.int64).contiguous()
        b = torch.as_tensor(other_ids).to(dev).reshape(-1).to(torch.int64).contiguous()
        if a.numel() != b.numel():
            raise RuntimeError(f"{label}node indices differ between runs ({a.numel()} and {b.numel()} nodes)")
        n = int(a.numel())
        if n == 0 or torch.equal(a, b):
            return torch.arange(n, dtype=torch.int32, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        sz = _lib.c_size(0)
        _lib.check(_lib.load().gnn_id_join_workspace_size(n, ctypes.byref(sz)), "gnn_id_join_workspace_size")
        ws = _workspace(dev, "join", sz.value)
        _lib.call("gnn_id_join", _lib.ptr(a), _lib.ptr(b), n, _lib.ptr(perm), _lib.ptr(status), _lib.ptr(ws),
                  ws.numel(), _lib.stream_handle(dev))
        st = int(status[0])
    else:
        a = np.asarray(_np(base_ids)).reshape(-1).astype(np.int64)
        b = np.asarray(_np(other_ids)).reshape(-1).astype(np.int64)
        if a.size != b.size:
            raise RuntimeError(f"{label}node indices differ between runs ({a.size} and {b.size} nodes)")
        n = int(a.size)
        if n == 0 or np.array_equal(a, b):
            return torch.arange(n, dtype=torch.int32)
        pa, pb = np.argsort(a, kind="stable"), np.argsort(b, kind="stable")
        ka, kb = a[pa], b[pb]
        st = (_lib.JOIN_STATUS_NEGATIVE if (ka[0] < 0 or kb[0] < 0) else 0) \
            | (_lib.JOIN_STATUS_DUPLICATE if ((ka[1:] == ka[:-1]).any() or (kb[1:] == kb[:-1]).any()) else 0) \
            | (_lib.JOIN_STATUS_MISMATCH if (ka != kb).any() else 0)
        out = np.empty(n, dtype=np.int32)
        out[pa] = pb
        perm = torch.from_numpy(out)
    if st & _lib.JOIN_STATUS_NEGATIVE:
        raise RuntimeError(f"{label}node indices: a negative id")
    if st & _lib.JOIN_STATUS_DUPLICATE:
        raise RuntimeError(f"{label}node indices: a duplicate id inside one run")
    if st & _lib.JOIN_STATUS_MISMATCH:
        raise RuntimeError(f"{label}node indices differ between runs")
    return perm


def ensemble_pair(a, b, mode: str = "logit", perm_a=None, check: bool = True) -> torch.Tensor:
    """The two-run ensemble of src/analysis/evaluate_ensemble.py as f32 [n], ``a`` read as ``a[perm_a]``:

    * ``prob``: 0.5·(a + b) in f32 — numpy's expression on f32 scores, bit for bit;
    * ``logit``: σ(½(logit a + logit b)) with both inputs clipped in f32 to [f32(1e-6), f32(1 − 1e-6)]
      (numpy's clip on f32 data), in the closed form r / (r + q), r = √(a·b), q = √((1−a)·(1−b)),
      evaluated in f64 with every operation rounded once and the quotient rounded to f32.  Multiply,
      subtract, add, square root and divide are correctly rounded by IEEE 754, so this numpy expression
      and the kernel (libgnnmp K19) give the same bits; the result is within half an f32 ulp (plus the
      f64 roundings) of the exact value.  The reference's f32 log / exp chain is several ulps off it.

    A NaN score is a ValueError, a ``perm_a`` entry outside [0, n) an IndexError (when ``check``)."""
    if mode not in ENSEMBLE_MODES:
        raise ValueError(f"Unknown mode={mode!r}. Use 'prob' or 'logit'.")
    if _is_device(a, b):
        dev = next(t.device for t in (a, b) if isinstance(t, torch.Tensor) and t.is_cuda)
        ta = torch.as_tensor(a).to(dev).reshape(-1).to(torch.float32).contiguous()
        tb = torch.as_tensor(b).to(dev).reshape(-1).to(torch.float32).contiguous()
        pt = None if perm_a is None else torch.as_tensor(perm_a).to(dev).reshape(-1).to(torch.int32).contiguous()
        n = int(tb.numel())
        if ta.numel() != n or (pt is not None and pt.numel() != n):
            raise ValueError("ensemble_pair: operands of different lengths")
        out = torch.empty(n, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call("gnn_ensemble_pair", _lib.ptr(ta), _lib.ptr(tb), _lib.ptr(pt), n, ENSEMBLE_MODES[mode], _lib.ptr(out),
                  _lib.ptr(status), _lib.stream_handle(dev))
        if check:
            check_status(status)
        return out
    x, yv = _np(a).reshape(-1).astype(np.float32), _np(b).reshape(-1).astype(np.float32)
    n = int(yv.size)
    if perm_a is not None:
        p = _np(perm_a).reshape(-1).astype(np.int64)
        if p.size != n or x.size != n:
            raise ValueError("ensemble_pair: operands of different lengths")
        if ((p < 0) | (p >= n)).any():
            raise IndexError("ensemble_pair: perm_a entry outside [0, n)")
        x = x[p]
    elif x.size != n:
        raise ValueError("ensemble_pair: operands of different lengths")
    if check and (np.isnan(x).any() or np.isnan(yv).any()):
        raise ValueError("rank_metrics: NaN score among the included elements")
    if mode == "prob":
        return torch.from_numpy(np.float32(0.5) * (x + yv))
    with np.errstate(invalid="ignore"):
        da = np.clip(x, _CLIP_LO, _CLIP_HI).astype(np.float64)
        db = np.clip(yv, _CLIP_LO, _CLIP_HI).astype(np.float64)
        r = np.sqrt(da * db)
        q = np.sqrt((1.0 - da) * (1.0 - db))
        return torch.from_numpy((r / (r + q)).astype(np.float32))
