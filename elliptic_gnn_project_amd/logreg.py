"""L2-penalised logistic regression on standardised features (the feature-only baseline of
src/train_baselines.py: StandardScaler + LogisticRegression) — on the device (libgnnmp K20,
csrc/baseline.hip) for CUDA features, in numpy f64 for host tensors / arrays.

One arithmetic for both paths, all in f64, over the selected rows of x [N, D] (f32) and y in {0, 1}:

    mu_j = sum_i x_ij / n      var_j = sum_i (x_ij - mu_j)^2 / n (two passes)
    sd_j = sqrt(var_j), 1 where var_j == 0        z_ij = ((double)x_ij - mu_j) / sd_j   (never stored)
    t_i = z_i.w + b            s_i = class weight of y_i
    F(w, b) = C sum_i s_i [softplus(t_i) - y_i t_i] + 1/2 |w|^2        (the intercept is not penalised)
    g = C A^T r + (w, 0),  r_i = s_i (sigma(t_i) - y_i)                A = [Z | 1]
    H = C A^T S A + diag(1, .., 1, 0),  S_i = s_i sigma(t_i) sigma(-t_i)

with sigma and softplus through e = exp(-|t|) as in calibrate.py.  ``class_weight`` is None (1, 1),
"balanced" (n / (2 n_c)) or a {0: a, 1: b} dict.  sklearn's rule for near-constant columns (a variance
within rounding of zero counts as zero) is not reproduced: only var_j == 0 gives sd_j = 1.

The fit is the minimiser of F itself — sklearn's objective, not lbfgs's stopping point — by Newton's
method; one evaluation gives (F, g, H) on the device or in numpy, and the loop around it is the same
code for both (``newton``):

1. theta = 0;
2. delta = H^-1 g by a numpy f64 Cholesky solve of the (D + 1)^2 system (a failed factorisation:
   status SINGULAR and a RuntimeError);
3. a = 1, halved while F(theta - a delta) > F(theta) + 2^-40 |F(theta)| and a > 2^-20 (value-only
   evaluations; the slack keeps rounding noise at the minimum from cutting a converged step);
4. theta <- theta - a delta;
5. stop when max|delta| <= 2^-40 max(1, max|theta|) (the full step), else after min(max_iter, 100)
   updates with status MAXIT and a warning.

A train split with a single class is a ValueError (as in sklearn); D is at most 255.
"""
from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

STEP_TOL = 2.0 ** -40
ARMIJO_SLACK = 2.0 ** -40
MIN_STEP = 2.0 ** -20
MAX_IT = 100
STATUS_MAXIT, STATUS_SINGULAR = 1, 2


@dataclass
class LogRegModel:
    mu: Optional[np.ndarray]  # [D] f64 (None: raw columns)
    sd: Optional[np.ndarray]
    w: np.ndarray  # [D] f64, on the standardised columns
    b: float
    iterations: int
    status: int
    F: float = float("nan")

    @property
    def theta(self) -> np.ndarray:
        return np.concatenate([self.w, [self.b]])


def class_weights(y_sel: np.ndarray, class_weight) -> Tuple[float, float]:
    """(s of a negative row, s of a positive row); raises for a single-class selection."""
    n = int(y_sel.size)
    n1 = int(np.count_nonzero(y_sel))
    n0 = n - n1
    if n0 == 0 or n1 == 0:
        raise ValueError("logreg.fit: the train rows hold a single class; the fit needs both")
    if class_weight is None:
        return 1.0, 1.0
    if isinstance(class_weight, str):
        if class_weight != "balanced":
            raise ValueError(f"logreg.fit: class_weight {class_weight!r} (None, 'balanced' or a dict)")
        return float(n) / float(2 * n0), float(n) / float(2 * n1)
    cw = {int(k): float(v) for k, v in dict(class_weight).items()}
    return cw.get(0, 1.0), cw.get(1, 1.0)


# ----------------------------------------------------------------------------- the shared outer loop
def newton(evaluate: Callable[[np.ndarray, bool], Tuple], D: int, max_iter: int) -> Dict:
    """Rules 1-5 of the module docstring around ``evaluate(theta, value_only) -> (F, g, H)``."""
    theta = np.zeros(D + 1, dtype=np.float64)
    status, it = 0, 0
    limit = min(int(max_iter), MAX_IT)
    F, g, H = evaluate(theta, False)
    while True:
        if not np.isfinite(F) or not np.isfinite(g).all() or not np.isfinite(H).all():
            raise ValueError("logreg.fit: NaN or infinite value among the selected rows")
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            raise RuntimeError(f"logreg.fit: the Hessian is not positive definite (status {STATUS_SINGULAR})")
        delta = np.linalg.solve(L.T, np.linalg.solve(L, g))
        a = 1.0
        while True:
            Fn = evaluate(theta - a * delta, True)[0]
            if not (Fn > F + ARMIJO_SLACK * abs(F)) or not (a > MIN_STEP):
                break
            a *= 0.5
        theta = theta - a * delta
        it += 1
        done = float(np.max(np.abs(delta))) <= STEP_TOL * max(1.0, float(np.max(np.abs(theta))))
        if done:
            F = evaluate(theta, True)[0]
            break
        if it >= limit:
            status |= STATUS_MAXIT
            warnings.warn(f"logreg.fit: no convergence after {it} Newton updates (status MAXIT)", RuntimeWarning)
            F = evaluate(theta, True)[0]
            break
        F, g, H = evaluate(theta, False)
    return dict(theta=theta, iterations=it, status=status, F=float(F))


# ----------------------------------------------------------------------------- host mirror (numpy f64)
def host_moments(x: np.ndarray, rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    xs = np.asarray(x, dtype=np.float32)[rows].astype(np.float64)
    n = float(xs.shape[0])
    mu = xs.sum(axis=0) / n
    var = ((xs - mu) ** 2).sum(axis=0) / n
    return mu, np.where(var == 0.0, 1.0, np.sqrt(var))


def host_z(x: np.ndarray, rows: np.ndarray, mu, sd) -> np.ndarray:
    z = np.asarray(x, dtype=np.float32)[rows].astype(np.float64)
    return z if mu is None else (z - mu) / sd


def host_row_terms(t: np.ndarray, y: np.ndarray, s: np.ndarray):
    """(f_i, r_i, h_i, p_i) of the docstring from t through e = exp(-|t|)."""
    e = np.exp(-np.abs(t))
    d = 1.0 + e
    p = np.where(t >= 0.0, 1.0 / d, e / d)
    q = np.where(t >= 0.0, e / d, 1.0 / d)
    sp = np.maximum(t, 0.0) + np.log1p(e)
    f = s * np.where(y, sp - t, sp)
    r = np.where(y, -(s * q), s * p)
    return f, r, s * (p * q), p


def host_eval(z: np.ndarray, y: np.ndarray, w0: float, w1: float, C: float, theta: np.ndarray,
              value_only: bool = False):
    """(F, g, H) at theta over the standardised rows z [n, D] and y [n] (bool)."""
    D = z.shape[1]
    w, b = theta[:D], theta[D]
    s = np.where(y, w1, w0)
    f, r, h, _ = host_row_terms(z @ w + b, y, s)
    F = C * float(np.sum(f)) + 0.5 * float(w @ w)
    if value_only:
        return F, None, None
    A = np.concatenate([z, np.ones((z.shape[0], 1))], axis=1)
    g = C * (A.T @ r)
    g[:D] += w
    H = C * (A.T @ (A * h[:, None]))
    H = 0.5 * (H + H.T)  # (the device mirrors one triangle; BLAS may differ in the last bit)
    H[np.arange(D), np.arange(D)] += 1.0
    return F, g, H


def host_predict(x, rows, model: LogRegModel) -> np.ndarray:
    t = host_z(x, rows, model.mu, model.sd) @ model.w + model.b
    e = np.exp(-np.abs(t))
    return np.where(t >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


# ----------------------------------------------------------------------------- device path
_WS: Dict[tuple, torch.Tensor] = {}


def _workspace(device: torch.device, name: str, nbytes: int) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), name)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def check_status(status: int) -> None:
    if status & _lib.BASELINE_STATUS_ROW:
        raise IndexError("logreg: a listed row is outside the feature matrix")


class _DeviceProblem:
    """The operands of one fit on the device: x (f32, last stride 1), the row list, the label bytes."""

    def __init__(self, x: torch.Tensor, y: Optional[torch.Tensor], rows: torch.Tensor):
        self.dev = x.device
        x = x.detach()
        if x.dtype != torch.float32:
            x = x.float()
        if x.dim() != 2:
            raise ValueError(f"logreg: x must be [N, D], got {tuple(x.shape)}")
        if x.stride(1) != 1 or (x.size(0) > 1 and x.stride(0) < x.size(1)):
            x = x.contiguous()
        self.x, self.N, self.D = x, int(x.size(0)), int(x.size(1))
        self.ld = int(x.stride(0)) if self.N > 1 else self.D
        self.rows = rows.detach().to(self.dev).to(torch.int32).contiguous()
        self.n = int(self.rows.numel())
        self.y = None if y is None else (y.detach().to(self.dev).reshape(-1) == 1).view(torch.uint8).contiguous()
        self.status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.mu = self.sd = None
        self.out = torch.empty(1 + (self.D + 1) + (self.D + 1) ** 2, dtype=torch.float64, device=self.dev)

    def moments(self) -> None:
        b = _lib.c_size(0)
        _lib.check(_lib.load().gnn_column_moments_workspace_size(self.n, self.D, ctypes.byref(b)),
                   "gnn_column_moments_workspace_size")
        ws = _workspace(self.dev, "moments", b.value)
        self.mu = torch.empty(self.D, dtype=torch.float64, device=self.dev)
        self.sd = torch.empty(self.D, dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.call("gnn_column_moments", _lib.ptr(self.x), self.ld, self.N, _lib.ptr(self.rows), self.n, self.D,
                      _lib.ptr(self.mu), _lib.ptr(self.sd), _lib.ptr(self.status), _lib.ptr(ws), ws.numel(),
                      _lib.stream_handle(self.dev))

    def evaluate(self, theta: np.ndarray, value_only: bool, w0: float, w1: float, C: float):
        """(F, g, H) as numpy from one pair of launches and one host read."""
        b = _lib.c_size(0)
        _lib.check(_lib.load().gnn_logreg_eval_workspace_size(self.n, self.D, ctypes.byref(b)),
                   "gnn_logreg_eval_workspace_size")
        ws = _workspace(self.dev, "eval", b.value)
        D1 = self.D + 1
        th = torch.from_numpy(np.ascontiguousarray(theta, dtype=np.float64)).to(self.dev)
        F, g, H = self.out[:1], self.out[1:1 + D1], self.out[1 + D1:]
        with torch.cuda.device(self.dev):
            _lib.call("gnn_logreg_eval", _lib.ptr(self.x), self.ld, self.N, _lib.ptr(self.rows), self.n, self.D,
                      _lib.ptr(self.y), _lib.ptr(self.mu), _lib.ptr(self.sd), float(w0), float(w1), float(C),
                      _lib.ptr(th), 1 if value_only else 0, _lib.ptr(F), None if value_only else _lib.ptr(g),
                      None if value_only else _lib.ptr(H), _lib.ptr(self.status), _lib.ptr(ws), ws.numel(),
                      _lib.stream_handle(self.dev))
        if value_only:
            got = torch.cat([F, self.status.to(torch.float64)]).cpu().numpy()
            check_status(int(got[1]))
            return float(got[0]), None, None
        got = torch.cat([self.out, self.status.to(torch.float64)]).cpu().numpy()  # the one host read
        check_status(int(got[-1]))
        return float(got[0]), got[1:1 + D1].copy(), got[1 + D1:-1].reshape(D1, D1).copy()

    def predict(self, theta: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor]:
        th = torch.from_numpy(np.ascontiguousarray(theta, dtype=np.float64)).to(self.dev)
        p64 = torch.empty(self.n, dtype=torch.float64, device=self.dev)
        p32 = torch.empty(self.n, dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.call("gnn_logreg_predict", _lib.ptr(self.x), self.ld, self.N, _lib.ptr(self.rows), self.n, self.D,
                      _lib.ptr(self.mu), _lib.ptr(self.sd), _lib.ptr(th), _lib.ptr(p64), _lib.ptr(p32),
                      _lib.ptr(self.status), _lib.stream_handle(self.dev))
        return p64, p32


def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _is_device(x) -> bool:
    return isinstance(x, torch.Tensor) and x.is_cuda


# ----------------------------------------------------------------------------- public interface
def fit(x, y, rows=None, C: float = 1.0, class_weight=None, max_iter: int = 100,
        standardize: bool = True) -> LogRegModel:
    """Fit on the rows ``rows`` (indices; default all) of x [N, D] with labels y [N] (1 = positive, any
    other value negative).  CUDA x runs the device path, anything else the numpy mirror."""
    D = int(x.shape[1])
    if not 1 <= D <= _lib.LOGREG_MAX_D:
        raise ValueError(f"logreg.fit: D = {D} outside [1, {_lib.LOGREG_MAX_D}]")
    if not (float(C) > 0.0 and np.isfinite(float(C))):
        raise ValueError("logreg.fit: C must be positive and finite")
    rows_np = np.arange(int(x.shape[0]), dtype=np.int64) if rows is None else _np(rows).astype(np.int64).reshape(-1)
    if rows_np.size and (rows_np.min() < 0 or rows_np.max() >= int(x.shape[0])):
        raise IndexError("logreg.fit: a listed row is outside the feature matrix")
    y_sel = _np(y).reshape(-1)[rows_np] == 1
    w0, w1 = class_weights(y_sel, class_weight)
    if _is_device(x):
        prob = _DeviceProblem(x, torch.as_tensor(y), torch.from_numpy(rows_np))
        if standardize:
            prob.moments()
        got = newton(lambda th, vo: prob.evaluate(th, vo, w0, w1, float(C)), D, max_iter)
        mu = prob.mu.cpu().numpy() if standardize else None
        sd = prob.sd.cpu().numpy() if standardize else None
    else:
        xn = np.asarray(_np(x), dtype=np.float32)
        mu, sd = host_moments(xn, rows_np) if standardize else (None, None)
        z = host_z(xn, rows_np, mu, sd)
        got = newton(lambda th, vo: host_eval(z, y_sel, w0, w1, float(C), th, vo), D, max_iter)
    th = got["theta"]
    return LogRegModel(mu=mu, sd=sd, w=th[:D].copy(), b=float(th[D]), iterations=got["iterations"],
                       status=got["status"], F=got["F"])


def predict_proba(model: LogRegModel, x, rows=None, dtype=np.float64):
    """sigma(z.w + b) of the listed rows: a tensor on x's device for CUDA x, else a numpy array;
    ``dtype`` float64 or float32 (the f64 value rounded once)."""
    n_all = int(x.shape[0])
    if _is_device(x):
        r = torch.arange(n_all) if rows is None else torch.as_tensor(rows).reshape(-1)
        prob = _DeviceProblem(x, None, r)
        if prob.n == 0:
            return torch.empty(0, dtype=torch.float64 if dtype == np.float64 else torch.float32, device=x.device)
        if model.mu is not None:
            prob.mu = torch.from_numpy(model.mu).to(prob.dev)
            prob.sd = torch.from_numpy(model.sd).to(prob.dev)
        p64, p32 = prob.predict(model.theta)
        check_status(int(prob.status))
        return p64 if dtype == np.float64 else p32
    rows_np = np.arange(n_all, dtype=np.int64) if rows is None else _np(rows).astype(np.int64).reshape(-1)
    p = host_predict(np.asarray(_np(x), dtype=np.float32), rows_np, model)
    return p if dtype == np.float64 else p.astype(np.float32)
