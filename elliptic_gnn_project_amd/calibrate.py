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
