"""Shared by tests/test_baselines_host.py, tests/test_gpu_baselines.py and the generator
tests/golden/make_baselines_golden.py: the seeded inputs of the logistic-regression cases (rebuilt from
the seed — the feature matrices are too large to commit; the fixture holds a checksum), the calibrator
patterns, and the fixture's loader."""
from pathlib import Path

import numpy as np

GOLDEN_PATH = Path(__file__).resolve().parent / "golden" / "baselines_golden.npz"

# name: (n, D, class_weight, kind)
LR_CASES = {
    "n257_d1": (257, 1, None, "noisy"),
    "n1000_d165_bal": (1000, 165, "balanced", "noisy"),
    "n4099_d167_bal": (4099, 167, "balanced", "noisy"),
    "n300_d64_separable": (300, 64, None, "separable"),
    "n2000_d255_bal": (2000, 255, "balanced", "noisy"),
    "n500_d10_constcol": (500, 10, "balanced", "constcol"),
}
PROB_TOL, COEF_TOL = 1e-9, 1e-8  # against sklearn's newton-cholesky at tol = 1e-12


def lr_inputs(name):
    """(x f32 [n, D], y int64 [n]) of a case: columns of different scale and offset, labels from a
    logistic model of a few columns (or its sign: separable)."""
    n, D, _, kind = LR_CASES[name]
    rng = np.random.default_rng(1000 + n + D)
    scale = np.exp(rng.uniform(-2.0, 2.0, size=D))
    shift = rng.uniform(-3.0, 3.0, size=D)
    x = (rng.standard_normal((n, D)) * scale + shift).astype(np.float32)
    w = rng.standard_normal(D) / np.sqrt(D)
    t = ((x - shift) / scale) @ w * 2.0 - 1.0
    if kind == "separable":
        y = (t > np.median(t)).astype(np.int64)
    else:
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-t))).astype(np.int64)
    if kind == "constcol":
        x[:, 3] = np.float32(2.5)
    assert 0 < y.sum() < n
    return x, y


def x_checksum(x):
    return np.array([x.astype(np.float64).sum(), float(x[0, 0]), float(x[-1, -1])])


# ----------------------------------------------------------------------------- calibrator patterns
def calibrator_inputs(pattern, n, seed=0):
    """(scores f32 [n], y int64 [n]) of a pattern."""
    rng = np.random.default_rng(77 + seed + n)
    y = (rng.random(n) < 0.3).astype(np.int64)
    if pattern == "distinct":
        s = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
        y = (rng.random(n) < s).astype(np.int64)
    elif pattern == "ties":
        s = np.round(np.clip(0.3 * y + 0.7 * rng.random(n), 0, 1), 2).astype(np.float32)
    elif pattern == "all_equal":
        s = np.full(n, 0.25, dtype=np.float32)
    elif pattern == "monotone":  # labels already monotone in the score: no pooling
        s = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
        y = (s > np.float32(0.6)).astype(np.int64)
    elif pattern == "reversed":  # labels fully reversed: one block
        s = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
        y = (s < np.float32(0.4)).astype(np.int64)
    elif pattern == "only_pos":
        s = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
        y = np.ones(n, dtype=np.int64)
    elif pattern == "only_neg":
        s = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
        y = np.zeros(n, dtype=np.int64)
    elif pattern == "sawtooth":  # alternating labels along the score: pooling across every seam
        s = ((np.arange(n) + 0.5) / n).astype(np.float32)[rng.permutation(n)]
        rank = np.argsort(np.argsort(s))
        y = ((rank % 2) == 0).astype(np.int64)
    else:
        raise ValueError(pattern)
    return s, y


CAL_CASES = [(p, n) for n in (1, 2, 3) for p in ("distinct", "all_equal", "only_pos", "only_neg")] + \
            [(p, 5000) for p in ("distinct", "ties", "all_equal", "monotone", "reversed", "only_pos", "only_neg")] + \
            [(p, 9000) for p in ("distinct", "ties")]


def cal_name(pattern, n):
    return f"{pattern}_n{n}"


def cal_queries(s, xs):
    """Queries below, at and above the range, at every threshold and at a spread of the scores."""
    lo, hi = float(s.min()), float(s.max())
    extra = np.array([lo - 1.0, lo, hi, hi + 1.0, 0.0, -0.0, 0.5], dtype=np.float32)
    return np.concatenate([extra, np.asarray(xs, dtype=np.float32), s[:: max(1, s.size // 400)]]).astype(np.float32)


def load_golden():
    with np.load(GOLDEN_PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def ulp_distance(a, b):
    """Largest distance in units of the last place between two f64 arrays of the same sign pattern."""
    a = np.asarray(a, dtype=np.float64).view(np.int64)
    b = np.asarray(b, dtype=np.float64).view(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0
