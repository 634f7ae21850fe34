"""Golden vectors for the feature-only baseline (logreg.py, calibrate.py's score calibrators), produced
with sklearn as the REFERENCE uses it: StandardScaler + LogisticRegression of src/train_baselines.py and
calibrate_isotonic / apply_sklearn_calibrator of src/utils/calibrate.py of the reference checkout.

    python tests/golden/make_baselines_golden.py <reference checkout>   # writes tests/golden/baselines_golden.npz

Needs a checkout of the reference and sklearn, so it is not run by the tests; the npz it writes is the
committed fixture tests/test_baselines_host.py and tests/test_gpu_baselines.py check against.  It records
inputs and outputs only; the feature matrices are rebuilt from their seeds (tests/baselines_cases.py) and
only their checksum is recorded.

Logistic regression.  The parity target is the minimiser of sklearn's objective: StandardScaler (f64 input)
+ LogisticRegression(solver="newton-cholesky", tol=1e-12).  A float64 Newton restatement of logreg.py's
rules is asserted here to agree with it within the tests' tolerances.  The reference's actual setting
(lbfgs, f32 features, default tol) is recorded with its objective value: it stops short of the minimum, so
the tests only check F(ours) <= F(lbfgs).

Calibrators.  Isotonic thresholds and outputs through the reference's functions on the f32 scores handed
over as f64; Platt from solver="newton-cholesky", tol=1e-12.  No two distinct scores are closer than
1e-15 (asserted), where sklearn's merge of near-equal scores is inert.  The integer PAVA restated here
gives sklearn's thresholds exactly and its values and outputs bit for bit on every case but the two large
all-distinct ones, where sklearn's float pooling (running weighted means) lands 3 and 1 ulp from the
correctly rounded P / W: the measured distance is recorded per case (``ulp``) and asserted <= 4.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import baselines_cases as bc  # noqa: E402

OUT = os.path.join(HERE, "baselines_golden.npz")


def objective(z, y, s, C, w, b):
    t = z @ w + b
    e = np.exp(-np.abs(t))
    sp = np.maximum(t, 0.0) + np.log1p(e)
    return C * float(np.sum(s * (sp - y * t))) + 0.5 * float(w @ w)


def newton_f64(z, y, s, C):
    """The rules of logreg.py restated: full Newton with the slack halving test."""
    n, D = z.shape
    A = np.concatenate([z, np.ones((n, 1))], axis=1)
    th = np.zeros(D + 1)
    F = lambda v: objective(z, y, s, C, v[:D], v[D])  # noqa: E731
    for _ in range(100):
        t = A @ th
        p = 1.0 / (1.0 + np.exp(-t))
        g = C * (A.T @ (s * (p - y)))
        g[:D] += th[:D]
        H = C * (A.T @ (A * (s * p * (1 - p))[:, None]))
        H[np.arange(D), np.arange(D)] += 1.0
        d = np.linalg.solve(H, g)
        a, f0 = 1.0, F(th)
        while F(th - a * d) > f0 + 2.0 ** -40 * abs(f0) and a > 2.0 ** -20:
            a *= 0.5
        th = th - a * d
        if np.abs(d).max() <= 2.0 ** -40 * max(1.0, np.abs(th).max()):
            break
    return th


def isotonic_int(s32, y):
    """The integer restatement: tie groups (P, W), PAVA on int cross products, P / W, trim; (xs, ys)."""
    x, inv = np.unique(s32 + np.float32(0.0), return_inverse=True)
    W = np.bincount(inv).tolist()
    P = np.bincount(inv, weights=y.astype(np.float64)).astype(np.int64).tolist()
    blocks = []
    for p, w in zip(P, W):
        c = 1
        while blocks and blocks[-1][0] * w >= p * blocks[-1][1]:
            q = blocks.pop()
            p, w, c = p + q[0], w + q[1], c + q[2]
        blocks.append((p, w, c))
    yv = np.repeat([b[0] / b[1] for b in blocks], [b[2] for b in blocks])
    keep = np.ones(x.size, dtype=bool)
    if x.size > 2:
        keep[1:-1] = (yv[1:-1] != yv[:-2]) | (yv[1:-1] != yv[2:])
    return x[keep].astype(np.float64), yv[keep]


def interp_clip(xs, ys, q):
    x = np.clip(q.astype(np.float64), xs[0], xs[-1])
    if xs.size == 1:
        return np.full(x.shape, ys[0])
    i = np.clip(np.searchsorted(xs, x, side="left"), 1, xs.size - 1)
    return (ys[i] - ys[i - 1]) / (xs[i] - xs[i - 1]) * (x - xs[i - 1]) + ys[i - 1]


def main():
    sys.path.insert(0, sys.argv[1])  # the reference checkout (imported as the package src)
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    from src.utils.calibrate import apply_sklearn_calibrator, calibrate_isotonic

    out = {}
    for name, (n, D, cw, _) in bc.LR_CASES.items():
        x, y = bc.lr_inputs(name)
        x64 = x.astype(np.float64)
        sc = StandardScaler().fit(x64)
        z = sc.transform(x64)
        lr = LogisticRegression(solver="newton-cholesky", tol=1e-12, C=1.0, class_weight=cw, max_iter=2000).fit(z, y)
        coef, icpt, prob = lr.coef_[0], float(lr.intercept_[0]), lr.predict_proba(z)[:, 1]
        s = np.ones(n) if cw is None else np.where(y == 1, n / (2.0 * y.sum()), n / (2.0 * (n - y.sum())))
        mu = x64.mean(axis=0)
        var = ((x64 - mu) ** 2).mean(axis=0)
        z_own = (x64 - mu) / np.where(var == 0.0, 1.0, np.sqrt(var))
        th = newton_f64(z_own, y, s, 1.0)
        p_own = 1.0 / (1.0 + np.exp(-(z_own @ th[:D] + th[D])))
        dp, dc = np.abs(p_own - prob).max(), max(np.abs(th[:D] - coef).max(), abs(th[D] - icpt))
        print(f"{name}: |p - sklearn| {dp:.3g}  |theta - sklearn| {dc:.3g}")
        assert dp <= bc.PROB_TOL / 25 and dc <= bc.COEF_TOL / 80, name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pipe = Pipeline([("scaler", StandardScaler(with_mean=True)),
                             ("clf", LogisticRegression(max_iter=2000, C=1.0, class_weight=cw, solver="lbfgs"))]).fit(x, y)
        lw, lb = pipe["clf"].coef_[0].astype(np.float64), float(pipe["clf"].intercept_[0])
        f_lbfgs, f_min = objective(z_own, y, s, 1.0, lw, lb), objective(z_own, y, s, 1.0, th[:D], th[D])
        assert f_min <= f_lbfgs
        print(f"    lbfgs: F - F_min {f_lbfgs - f_min:.3g}, |p_lbfgs - p| {np.abs(pipe.predict_proba(x)[:, 1] - prob).max():.3g}")
        out[f"lr/{name}/checksum"] = bc.x_checksum(x)
        out[f"lr/{name}/y"] = y.astype(np.int8)
        out[f"lr/{name}/coef"], out[f"lr/{name}/intercept"], out[f"lr/{name}/prob"] = coef, np.array([icpt]), prob
        out[f"lr/{name}/lbfgs_theta"] = np.concatenate([lw, [lb]])
        out[f"lr/{name}/lbfgs_F"] = np.array([f_lbfgs])

    for pattern, n in bc.CAL_CASES:
        name = bc.cal_name(pattern, n)
        s, y = bc.calibrator_inputs(pattern, n)
        u = np.unique(s.astype(np.float64))
        assert u.size < 2 or np.diff(u).min() > 1e-15, name
        ir = calibrate_isotonic(s.astype(np.float64), y)
        xs, ys = np.asarray(ir.X_thresholds_, dtype=np.float64), np.asarray(ir.y_thresholds_, dtype=np.float64)
        q = bc.cal_queries(s, xs)
        out[f"cal/{name}/scores"], out[f"cal/{name}/y"], out[f"cal/{name}/queries"] = s, y.astype(np.int8), q
        out[f"cal/{name}/xs"], out[f"cal/{name}/ys"] = xs, ys
        out[f"cal/{name}/iso"] = np.asarray(apply_sklearn_calibrator(ir, q.astype(np.float64)), dtype=np.float64)
        # the integer restatement against sklearn's float pooling: bit-equal, or the measured ulp distance
        xi, yi = isotonic_int(s, y)
        assert np.array_equal(xi, xs), name
        ulp = max(bc.ulp_distance(yi, ys), bc.ulp_distance(interp_clip(xi, yi, q), out[f"cal/{name}/iso"]))
        print(f"{name}: K = {xs.size}, integer PAVA against sklearn: {ulp} ulp")
        assert ulp <= 4, name
        out[f"cal/{name}/ulp"] = np.array([ulp])
        if 0 < y.sum() < n:
            lr = LogisticRegression(solver="newton-cholesky", tol=1e-12).fit(s.astype(np.float64).reshape(-1, 1), y)
            out[f"cal/{name}/platt_theta"] = np.array([lr.coef_[0, 0], lr.intercept_[0]])
            out[f"cal/{name}/platt"] = lr.predict_proba(q.astype(np.float64).reshape(-1, 1))[:, 1]
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
