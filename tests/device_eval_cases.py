"""Inputs shared by tests/test_device_eval_host.py and tests/test_gpu_device_eval.py: score / label
patterns (those of tests/test_gpu_rank_metrics.py's ``make`` and four more) and the seeded margin
sets of the temperature fit."""
import numpy as np

PATTERNS = ["distinct", "round1", "round2", "equal", "allpos", "onepos_last", "nopos", "informative", "ones"]
TARGETS = [0.9, 0.25, 1.0]
# (n, scale, shift) of margins scale * (N(0, 1) + shift * (2 y - 1))
FIT_SETS = [(3000, 3.0, 1.0), (3000, 8.0, 0.3), (3000, 0.3, 0.5), (5, 2.0, 0.5), (46000, 4.0, 0.8)]


def ap_tol(n: int) -> float:
    """A few f64 ulps per tie group, at most n groups (the project's bound for AP and ROC-AUC)."""
    return max(1e-12, 4 * n * 2.0 ** -53)


def make(pattern: str, n: int, seed: int = 0):
    """(labels int64 in {0, 1}, scores f32 in [0, 1]) of one pattern."""
    rng = np.random.default_rng(seed + n)
    y = (rng.random(n) < 0.2).astype(np.int64)
    s = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    if pattern == "round1":
        s = np.round(rng.random(n), 1).astype(np.float32)
    elif pattern == "round2":
        s = np.round(rng.random(n), 2).astype(np.float32)
    elif pattern == "equal":
        s[:] = 0.5
    elif pattern == "allpos":
        y[:] = 1
    elif pattern == "onepos_last":
        y[:] = 0
        y[int(np.argmin(s))] = 1
    elif pattern == "nopos":
        y[:] = 0
    elif pattern == "informative":  # scores that know something about the labels
        s = np.clip(0.45 * y + 0.55 * rng.random(n), 0.0, 1.0).astype(np.float32)
    elif pattern == "ones":  # 30 % of the scores exactly 1.0 (the last calibration bin's closed edge)
        s[rng.random(n) < 0.3] = 1.0
    return y, s


def fit_set(n: int, scale: float, shift: float, seed: int = 0):
    """(logits f32 [n, 2], labels int64 [n]) whose margins are scale * (N(0, 1) + shift * (2 y - 1))
    up to the float32 rounding of the logits."""
    rng = np.random.default_rng(1000 + seed + n)
    y = (rng.random(n) < 0.3).astype(np.int64)
    d = scale * (rng.standard_normal(n) + shift * (2 * y - 1))  # z1 - z0
    base = rng.standard_normal(n)
    z = np.stack([base - 0.5 * d, base + 0.5 * d], axis=1).astype(np.float32)
    return z, y
