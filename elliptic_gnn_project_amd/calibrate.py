"""Temperature scaling (TemperatureScaler.fit, src/utils/calibrate.py:8-30) as the minimiser of the
validation NLL — on the device (libgnnmp K17, csrc/calibrate.hip: one launch) for CUDA logits, in
numpy f64 for host tensors.  The reference's LBFGS (lr = 0.1, no line search) stops when the loss
moves by less than 1e-9, a little short of the minimum; this fit computes the minimiser itself, which
is why the pipeline only uses it on request (``device_eval``).

One arithmetic for both paths, all in f64, for two-class logits z [N, 2] and labels y over the
included rows (``mask``; default: the rows with y in {0, 1}):

    m_i = z[i, y_i] - z[i, 1 - y_i]          beta = 1 / T
    f(beta) = mean softplus(-beta m_i)       (the NLL of z / T; convex in beta)
    g(beta) = -mean m_i sigma(-beta m_i)     h(beta) = mean m_i^2 sigma(beta m_i) sigma(-beta m_i)

with sigma and softplus through e = exp(-|t|): sigma(t) = 1 / (1 + e) for t >= 0, e / (1 + e) below;
softplus(-t) = max(-t, 0) + log1p(e).  The rules, in order:

1. no row: T = 1 (status EMPTY);
2. |g(1)| <= 1e-7: T = 1 exactly (FLAT) — LBFGS's tolerance_grad exit on its first closure, so a
   separable validation split keeps T = 1;
3. g(2^-10) >= 0: beta = 2^-10 (CLAMP_LOW); g(2^10) <= 0: beta = 2^10 (CLAMP_HIGH);
4. safeguarded Newton from beta = 1 inside the bracket g(lo) < 0 < g(hi): the candidate is
   beta - g / h, or the bracket's midpoint when h == 0 or the candidate is not strictly inside; it
   stops at g == 0, at |beta_new - beta| <= 2^-40 beta (beta_new is kept) or after 100 updates (MAXIT).
   A Newton step |g / h| <= 2^-40 beta is that stop too: its candidate is kept when strictly inside
   the bracket and beta itself otherwise (beta is an end of the bracket by then; falling back to the
   midpoint would restart a bisection from a converged point).

T = float32(1 / beta).  An included row with a label outside {0, 1} or a NaN / infinite logit is
skipped and reported: a ValueError here.  Other widths than two classes keep the LBFGS path.

The score calibrators of src/utils/calibrate.py:32-47 (``fit_isotonic``, ``fit_platt``,
``apply_calibrator``; libgnnmp K20, csrc/baseline.hip, for CUDA scores and numpy for the rest), defined on
f32 scores and positives ``y == 1`` over the included elements (``mask``, default ``y >= 0``):

* isotonic (IsotonicRegression(out_of_bounds="clip")): the points are the tie groups of bit-equal scores
  (-0.0 == +0.0) in ascending order — the groups of the rank plan — each with integers P (positives) and
  W (elements).  PAVA pools adjacent blocks a (left), b while P_a W_b >= P_b W_a (int64; equal means pool,
  as in sklearn); a block's value is the one f64 division P / W, so the solution is integer-exact and the
  same bits however the work is chunked.  Trim: the first and the last point stay, an interior point k
  stays iff y_k != y_{k-1} or y_k != y_{k+1}.  Apply (scipy's linear interp1d as sklearn calls it), in f64
  with each operation rounded once: x clipped to [x_0, x_{K-1}], i = clip(searchsorted_left(xs, x), 1,
  K - 1), slope = (y_i - y_{i-1}) / (x_i - x_{i-1}), out = slope (x - x_{i-1}) + y_{i-1}; K = 1 gives the
  constant.  sklearn first merges scores closer than the dtype's resolution (1e-10 apart for f64 input);
  this does not.
* Platt (LogisticRegression on the score): logreg.fit on the one raw column — the f32 score upcast, no
  standardising, C = 1, no class weight: the minimiser of sklearn's objective; apply = sigma(w s + b).

A NaN score among the included elements is a ValueError; an empty fit set gives the identity and status
EMPTY.  The calibrated score is the f64 value rounded once to f32 (the project's score dtype).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

BETA_LO, BETA_HI = 2.0 ** -10, 2.0 ** 10
FLAT_GRAD = 1e-7
STEP_TOL = 2.0 ** -40
MAX_IT = 100


def check_status(status: int) -> None:
    """Raise for the bits of a fit's status word that mean bad input."""
    if status & _lib.FIT_STATUS_LABEL:
        raise ValueError("fit_temperature: an included row's label is outside {0, 1}")
    if status & _lib.FIT_STATUS_NAN:
        raise ValueError("fit_temperature: NaN or infinite logit among the included rows")


# ----------------------------------------------------------------------------- host mirror (numpy f64)
def host_margins(logits: np.ndarray, y: np.ndarray, mask: Optional[np.ndarray]) -> Tuple[np.ndarray, int]:
    """(margins of the rows that count, status bits of the rows that were skipped)."""
    z = np.asarray(logits, dtype=np.float32)
    y = np.asarray(y).astype(np.int64)
    lab = (y == 0) | (y == 1)
    inc = lab if mask is None else np.asarray(mask).astype(bool)
    status = _lib.FIT_STATUS_LABEL if bool((inc & ~lab).any()) else 0
    rows = np.nonzero(inc & lab)[0]
    yy = y[rows]
    with np.errstate(invalid="ignore"):
        m = z[rows, yy].astype(np.float64) - z[rows, 1 - yy].astype(np.float64)
    ok = np.isfinite(m)
    if not bool(ok.all()):
        status |= _lib.FIT_STATUS_NAN
    return m[ok], status


def host_eval(m: np.ndarray, beta: float) -> Tuple[float, float, float]:
    """(f, g, h)(beta) of the module docstring over the margins m (at least one)."""
    t = beta * m
    e = np.exp(-np.abs(t))
    d = 1.0 + e
    sp = np.where(t >= 0.0, 1.0 / d, e / d)
    sn = np.where(t >= 0.0, e / d, 1.0 / d)
    n = float(m.size)
    f = float(np.sum(np.maximum(-t, 0.0) + np.log1p(e))) / n
    g = -(float(np.sum(m * sn)) / n)
    h = float(np.sum((m * m) * (sp * sn))) / n
    return f, g, h


def host_fit(m: np.ndarray) -> Dict:
    """The rules of the module docstring over the margins: {beta, f, g, iterations, status, T}."""
    def done(beta, e, it, st):
        flat = st & (_lib.FIT_STATUS_EMPTY | _lib.FIT_STATUS_FLAT)
        return dict(beta=beta, f=e[0], g=e[1], iterations=it, status=st,
                    T=np.float32(1.0) if flat else np.float32(1.0 / beta))

    if m.size == 0:
        return done(1.0, (0.0, 0.0, 0.0), 0, _lib.FIT_STATUS_EMPTY)
    e = host_eval(m, 1.0)
    if abs(e[1]) <= FLAT_GRAD:
        return done(1.0, e, 0, _lib.FIT_STATUS_FLAT)
    lo_e = host_eval(m, BETA_LO)
    if lo_e[1] >= 0.0:
        return done(BETA_LO, lo_e, 0, _lib.FIT_STATUS_CLAMP_LOW)
    hi_e = host_eval(m, BETA_HI)
    if hi_e[1] <= 0.0:
        return done(BETA_HI, hi_e, 0, _lib.FIT_STATUS_CLAMP_HIGH)
    beta, lo, hi, it = 1.0, BETA_LO, BETA_HI, 0  # g(lo) < 0 < g(hi)
    while e[1] != 0.0:
        it += 1
        if e[1] < 0.0:
            lo = beta
        else:
            hi = beta
        step = e[1] / e[2] if e[2] != 0.0 else float("nan")
        cand = beta - step
        conv = abs(step) <= STEP_TOL * beta  # (False for the NaN of h == 0)
        if not (lo < cand < hi):
            cand = beta if conv else 0.5 * (lo + hi)
        conv = conv or abs(cand - beta) <= STEP_TOL * beta
        beta = cand
        e = host_eval(m, beta)
        if conv:
            break
        if it == MAX_IT:
            return done(beta, e, it, _lib.FIT_STATUS_MAXIT)
    return done(beta, e, it, 0)


# ----------------------------------------------------------------------------- device path
_WS: Dict[tuple, torch.Tensor] = {}


def _workspace(device: torch.device, n: int) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), n)
    ws = _WS.get(key)
    if ws is None:
        b = _lib.c_size(0)
        _lib.check(_lib.load().gnn_temperature_fit_workspace_size(n, ctypes.byref(b)),
                   "gnn_temperature_fit_workspace_size")
        ws = _WS[key] = torch.empty(b.value, dtype=torch.uint8, device=device)
    return ws


def fit_temperature(logits: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor] = None,
                    details: Optional[Dict] = None) -> torch.Tensor:
    """The T [1] (f32, on the logits' device) minimising the cross entropy of ``logits / T`` against
    ``y`` over the rows of ``mask`` (default: the rows with y in {0, 1}).  CUDA logits [N, 2] (any row
    stride) run as one launch and one host read of the diagnostics and the status word; host logits run
    the numpy mirror.  ``details`` (a dict) receives beta, f, g, iterations and status.  Logits of
    another width take the reference's LBFGS path (robustness.fit_temperature)."""
    if logits.dim() != 2:
        raise ValueError(f"fit_temperature: logits must be [N, C], got {tuple(logits.shape)}")
    N = int(logits.size(0))
    if y.numel() != N or (mask is not None and mask.numel() != N):
        raise ValueError("fit_temperature: y / mask do not match the logits' rows")
    if logits.size(1) != 2:
        from .robustness import fit_temperature as lbfgs_fit

        rows = slice(None) if mask is None else mask.bool()
        return lbfgs_fit(logits[rows], y[rows])
    if not logits.is_cuda:
        z = logits.detach().to(torch.float32).numpy()
        m, skipped = host_margins(z, y.detach().cpu().numpy(), None if mask is None else mask.detach().cpu().numpy())
        got = host_fit(m)
        got["status"] |= skipped
        if details is not None:
            details.update({k: got[k] for k in ("beta", "f", "g", "iterations", "status")})
        check_status(got["status"])
        return torch.tensor([got["T"]], dtype=torch.float32)
    dev = logits.device
    z = logits.detach()
    if z.dtype != torch.float32:
        z = z.float()
    if z.stride(1) != 1 or (N > 1 and z.stride(0) < 2):
        z = z.contiguous()
    yy = y.detach().to(dev).to(torch.int64).contiguous()
    inc = None
    if mask is not None:
        inc = mask.detach().to(dev).contiguous()
        inc = inc.view(torch.uint8) if inc.dtype == torch.bool else (inc != 0).view(torch.uint8)
    T = torch.empty(1, dtype=torch.float32, device=dev)
    diag = torch.empty(5, dtype=torch.float64, device=dev)  # {beta, f, g, iterations} and the status word
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _workspace(dev, N)
    with torch.cuda.device(dev):
        _lib.call("gnn_temperature_fit", _lib.ptr(z), int(z.stride(0)) if N > 1 else 2, _lib.ptr(yy), _lib.ptr(inc), N,
                  _lib.ptr(T), _lib.ptr(diag), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
        diag[4:] = status
    got = diag.tolist()  # the one host read
    if details is not None:
        details.update(beta=got[0], f=got[1], g=got[2], iterations=int(got[3]), status=int(got[4]))
    check_status(int(got[4]))
    return T


# ----------------------------------------------------------------------------- score calibrators (K20)
class Calibrator:
    """kind "identity", "isotonic" (thresholds xs, ys: f64) or "platt" (w, b); ``status`` a FIT_STATUS_* word."""

    def __init__(self, kind: str, xs=None, ys=None, w: float = 1.0, b: float = 0.0, status: int = 0, model=None):
        self.kind, self.status, self.model = kind, int(status), model
        self.xs = np.zeros(0) if xs is None else np.asarray(xs, dtype=np.float64)
        self.ys = np.zeros(0) if ys is None else np.asarray(ys, dtype=np.float64)
        self.w, self.b = float(w), float(b)


def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _is_device(*ts) -> bool:
    return any(isinstance(t, torch.Tensor) and t.is_cuda for t in ts)


def _host_fit_inputs(scores, y, mask):
    s = np.asarray(_np(scores), dtype=np.float32).reshape(-1)
    yy = _np(y).reshape(-1)
    if yy.size != s.size or (mask is not None and _np(mask).size != s.size):
        raise ValueError("calibrate: y / mask do not match the scores")
    inc = (yy >= 0) if mask is None else _np(mask).reshape(-1).astype(bool)
    if np.isnan(s[inc]).any():
        raise ValueError("calibrate: NaN score among the included elements")
    return s, yy == 1, inc


def host_isotonic_fit(scores: np.ndarray, positive: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(xs, ys) of the module docstring for f32 scores (no NaN) and bool positives, at least one element."""
    s = np.asarray(scores, dtype=np.float32) + np.float32(0.0)  # -0.0 -> +0.0
    x, inv = np.unique(s, return_inverse=True)
    W = np.bincount(inv, minlength=x.size).astype(np.int64)
    P = np.bincount(inv, weights=np.asarray(positive, dtype=np.float64), minlength=x.size).astype(np.int64)
    bp, bw, bn = [], [], []  # the stack of blocks: positives, elements, points
    for p, w in zip(P.tolist(), W.tolist()):
        n = 1
        while bp and bp[-1] * w >= p * bw[-1]:
            p, w, n = p + bp.pop(), w + bw.pop(), n + bn.pop()
        bp.append(p)
        bw.append(w)
        bn.append(n)
    val = np.asarray(bp, dtype=np.float64) / np.asarray(bw, dtype=np.float64)
    yv = np.repeat(val, bn)
    keep = np.ones(x.size, dtype=bool)
    if x.size > 2:
        keep[1:-1] = (yv[1:-1] != yv[:-2]) | (yv[1:-1] != yv[2:])
    return x[keep].astype(np.float64), yv[keep]


def host_isotonic_apply(xs: np.ndarray, ys: np.ndarray, q: np.ndarray) -> np.ndarray:
    x = np.asarray(q, dtype=np.float32).astype(np.float64)
    K = int(xs.size)
    if K == 0:
        return x
    if K == 1:
        return np.where(np.isnan(x), np.nan, ys[0])
    xc = np.clip(x, xs[0], xs[-1])
    i = np.clip(np.searchsorted(xs, xc, side="left"), 1, K - 1)
    slope = (ys[i] - ys[i - 1]) / (xs[i] - xs[i - 1])
    return slope * (xc - xs[i - 1]) + ys[i - 1]


_ISO_WS: Dict[tuple, torch.Tensor] = {}


def _iso_workspace(device: torch.device, n: int) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), n)
    ws = _ISO_WS.get(key)
    if ws is None:
        b = _lib.c_size(0)
        _lib.check(_lib.load().gnn_isotonic_fit_workspace_size(n, ctypes.byref(b)), "gnn_isotonic_fit_workspace_size")
        ws = _ISO_WS[key] = torch.empty(b.value, dtype=torch.uint8, device=device)
    return ws


def _device_isotonic_fit(scores, y, mask) -> Calibrator:
    from . import rank_metrics

    s, yy, inc = rank_metrics._device_inputs(scores, y, mask)
    s = s.detach().to(torch.float32).contiguous()
    n, dev = int(s.numel()), s.device
    if n == 0:
        return Calibrator("identity", status=_lib.FIT_STATUS_EMPTY)
    buf = rank_metrics._buffers(dev, n, 1, "iso")
    xs = torch.empty(n, dtype=torch.float64, device=dev)
    ys = torch.empty(n, dtype=torch.float64, device=dev)
    K = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _iso_workspace(dev, n)
    with torch.cuda.device(dev):
        rank_metrics._build_plan(buf, s, inc, None)
        _lib.call("gnn_isotonic_fit", _lib.ptr(s), _lib.ptr(buf.order), _lib.ptr(buf.flags), _lib.ptr(buf.seg_ptr),
                  _lib.ptr(rank_metrics._u8(yy == 1)), n, 1, _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(K), _lib.ptr(ws),
                  ws.numel(), _lib.stream_handle(dev))
    got = torch.cat([K, buf.status.to(torch.int64)]).cpu()  # the one host read
    if int(got[1]) & _lib.RANK_STATUS_NAN:
        raise ValueError("calibrate: NaN score among the included elements")
    k = int(got[0])
    if k == 0:
        return Calibrator("identity", status=_lib.FIT_STATUS_EMPTY)
    return Calibrator("isotonic", xs[:k].cpu().numpy(), ys[:k].cpu().numpy())


def fit_isotonic(scores, y, mask=None) -> Calibrator:
    """The isotonic calibrator of the included elements (module docstring); CUDA tensors take the device
    path (one rank plan, gnn_isotonic_fit), arrays and host tensors the numpy mirror."""
    if _is_device(scores, y, mask):
        return _device_isotonic_fit(scores, y, mask)
    s, pos, inc = _host_fit_inputs(scores, y, mask)
    if not inc.any():
        return Calibrator("identity", status=_lib.FIT_STATUS_EMPTY)
    return Calibrator("isotonic", *host_isotonic_fit(s[inc], pos[inc]))


def fit_platt(scores, y, mask=None) -> Calibrator:
    """The Platt calibrator: logreg.fit on the one raw score column, C = 1, no class weight."""
    from . import logreg

    if _is_device(scores, y, mask):
        from . import rank_metrics

        s, yy, inc = rank_metrics._device_inputs(scores, y, mask)
        s = s.detach().to(torch.float32).contiguous()
        rows = torch.nonzero(inc).flatten()
        if bool(torch.isnan(s[rows]).any()):
            raise ValueError("calibrate: NaN score among the included elements")
    else:
        s, pos, incn = _host_fit_inputs(scores, y, mask)
        yy, rows = pos.astype(np.int64), np.nonzero(incn)[0]
    if int(rows.shape[0]) == 0:
        return Calibrator("identity", status=_lib.FIT_STATUS_EMPTY)
    m = logreg.fit(s.reshape(-1, 1), yy, rows=rows, C=1.0, class_weight=None, max_iter=MAX_IT, standardize=False)
    status = _lib.FIT_STATUS_MAXIT if m.status & logreg.STATUS_MAXIT else 0
    return Calibrator("platt", w=float(m.w[0]), b=m.b, status=status, model=m)


def apply_calibrator(cal: Calibrator, scores, dtype=np.float32):
    """The calibrated scores: a tensor on the scores' device for CUDA scores, else a numpy array, as f32
    (default; the f64 value rounded once) or f64.  A NaN score is a ValueError."""
    f64 = np.dtype(dtype) == np.float64
    if _is_device(scores):
        s = scores.detach().to(torch.float32).contiguous().reshape(-1)
        n, dev = int(s.numel()), s.device
        if cal.kind == "identity" or n == 0:
            return s.double() if f64 else s.clone()
        if cal.kind == "platt":
            from . import logreg

            if bool(torch.isnan(s).any()):
                raise ValueError("calibrate: NaN score")
            return logreg.predict_proba(cal.model, s.reshape(-1, 1), None, np.float64 if f64 else np.float32)
        xs = torch.from_numpy(cal.xs).to(dev)
        ys = torch.from_numpy(cal.ys).to(dev)
        K = torch.tensor([cal.xs.size], dtype=torch.int64, device=dev)
        o64 = torch.empty(n, dtype=torch.float64, device=dev)
        o32 = torch.empty(n, dtype=torch.float32, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("gnn_isotonic_apply", _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(K), _lib.ptr(s), n, _lib.ptr(o64),
                      _lib.ptr(o32), _lib.ptr(st), _lib.stream_handle(dev))
        if int(st) & _lib.BASELINE_STATUS_NAN:
            raise ValueError("calibrate: NaN score")
        return o64 if f64 else o32
    s = np.asarray(_np(scores), dtype=np.float32).reshape(-1)
    if np.isnan(s).any():
        raise ValueError("calibrate: NaN score")
    if cal.kind == "identity":
        out = s.astype(np.float64)
    elif cal.kind == "platt":
        from . import logreg

        out = logreg.host_predict(s.reshape(-1, 1), np.arange(s.size), cal.model)
    else:
        out = host_isotonic_apply(cal.xs, cal.ys, s)
    return out if f64 else out.astype(np.float32)
