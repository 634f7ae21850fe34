"""Golden vectors for the run reports (rank_metrics' K19 functions, eval_by_time, workload_curves,
calibration_plots, evaluate_ensemble), produced by the REFERENCE modules src/analysis/eval_by_time.py,
workload_curves.py, calibration_plots.py and evaluate_ensemble.py of the reference checkout (importable
here: they need numpy, sklearn and matplotlib).

    python tests/golden/make_reports_golden.py <reference checkout>   # writes tests/golden/reports_golden.json

Needs a checkout of the reference, so it is not run by the tests; the JSON it writes is the committed
fixture tests/test_reports_host.py and tests/test_gpu_reports.py check against.  It records inputs and the
reference's outputs only.  Scores are float32 values (stored exactly as JSON doubles), as softmax outputs
are.  Every property the tests rely on is asserted here.
"""
import json
import os
import sys
import warnings

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reports_golden.json")
BINS = 15


def f64_list(a):
    return np.asarray(a).astype(np.float64).tolist()


def pattern(name, seed, n):
    """The two score patterns of make_bootstrap_golden.py: (labels, scores A, scores B)."""
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.15).astype(np.int64)
    y[:20] = 1
    rng.shuffle(y)
    if name == "distinct":
        s_a = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
        rk = np.argsort(np.argsort(s_a + 0.25 * y + 0.1 * rng.random(n)))
        s_b = ((rk + 0.5) / n).astype(np.float32)
        assert len(np.unique(s_a)) == n and len(np.unique(s_b)) == n
    else:
        s_a = np.round(np.clip(0.3 * y + 0.7 * rng.random(n), 0, 1), 2).astype(np.float32)
        s_b = np.round(np.clip(0.4 * y + 0.6 * rng.random(n), 0, 1), 2).astype(np.float32)
        assert len(np.unique(s_a)) < n // 2
    return y, s_a, s_b


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def logit_f64(p32):
    """The reference's formula in f64 on its own clipped f32 inputs."""
    p = np.clip(p32, 1e-6, 1 - 1e-6)
    assert p.dtype == np.float32
    assert np.array_equal(p, np.clip(p32, np.float32(1e-6), np.float32(1 - 1e-6)))  # numpy's bounds on f32 data
    p = p.astype(np.float64)
    return np.log(p / (1.0 - p))


def main():
    sys.path.insert(0, sys.argv[1])  # the reference checkout (imported as the package src)
    from src.analysis.calibration_plots import compute_reliability
    from src.analysis.eval_by_time import compute_metrics_per_timestep
    from src.analysis.evaluate_ensemble import _ensemble, _metrics_for_test, _select_threshold
    from src.analysis.workload_curves import build_k_values, compute_precision_curve
    from src.utils.metrics import expected_calibration_error

    warnings.simplefilter("ignore")  # sklearn: no positive class in one timestep
    gold = {"source": "src/analysis/{eval_by_time,workload_curves,calibration_plots,evaluate_ensemble}.py"}

    # ---- by time: 8 timesteps of 50, one without a positive, one with positives only
    by_time = []
    for name, seed in (("distinct", 20), ("ties", 21)):
        n = 400
        y, s, _ = pattern(name, seed, n)
        rng = np.random.default_rng(seed + 100)
        ts = rng.permutation(np.repeat(np.arange(35, 43), 50)).astype(np.int64)
        y[ts == 37] = 0
        y[ts == 40] = 1
        thr = float(np.sort(s)[n // 2])
        assert thr in set(s.astype(np.float64).tolist()) and all(int((ts == t).sum()) == 50 for t in range(35, 43))
        assert int(y[ts == 37].sum()) == 0 and int(y[ts == 40].sum()) == 50
        rows = compute_metrics_per_timestep(y, s, ts, thr)
        assert len(rows) == 8
        by_time.append({"name": name, "y": y.tolist(), "scores": f64_list(s), "timestep": ts.tolist(),
                        "threshold": thr, "rows": rows})
    gold["by_time"] = by_time

    # ---- workload curve: distinct scores, the three shapes of the k grid and a tiny run
    y, s, _ = pattern("distinct", 22, 400)
    curves = []
    for k_max in (5000, 30, 7):
        ks = build_k_values(400, k_max)
        curves.append({"k_max": k_max, "ks": ks, "precision": compute_precision_curve(y, s, ks)})
    assert curves[0]["ks"][-1] == 400 and curves[1]["ks"] == [10, 20, 30] and curves[2]["ks"] == [7]
    y7 = np.array([0, 1, 0, 0, 1, 0, 1], dtype=np.int64)
    s7 = ((np.random.default_rng(23).permutation(7) + 0.5) / 7).astype(np.float32)
    ks7 = build_k_values(7, 5000)
    assert ks7 == [7]
    gold["workload"] = {"y": y.tolist(), "scores": f64_list(s), "curves": curves,
                        "tiny": {"y": y7.tolist(), "scores": f64_list(s7), "k_max": 5000, "ks": ks7,
                                 "precision": compute_precision_curve(y7, s7, ks7)}}

    # ---- reliability: two empty bins, scores exactly on the two bin edges a float32 holds
    rng = np.random.default_rng(24)
    n = 400
    edges = np.linspace(0.0, 1.0, BINS + 1)
    s = rng.random(n).astype(np.float32)
    for b in (4, 11):  # empty these two bins
        inside = (s.astype(np.float64) >= edges[b]) & (s.astype(np.float64) < edges[b + 1])
        s[inside] = (s[inside] * np.float32(0.05)).astype(np.float32)
    s[0], s[1] = 1.0, 0.0
    y = (rng.random(n) < s).astype(np.int64)
    counts = np.histogram(s.astype(np.float64), edges)[0]  # [lo, hi) and a closed last bin: the reference's masks
    assert int((counts == 0).sum()) == 2 and int(counts.sum()) == n
    centers, accs, confs = compute_reliability(y, s, BINS)
    assert len(centers) == BINS - 2
    gold["reliability"] = {"y": y.tolist(), "scores": f64_list(s), "bins": BINS, "bin_center": f64_list(centers),
                           "accuracy": f64_list(accs), "confidence": f64_list(confs),
                           "count": counts[counts > 0].tolist(), "ece": float(expected_calibration_error(y, s, BINS))}

    # ---- ensemble, logit mode: two runs over the same nodes in different orders, ids above 2^32
    rng = np.random.default_rng(25)
    splits, ref_dev, min_gap = {}, 0.0, np.inf
    for split, n in (("val", 300), ("test", 400)):
        e = (rng.permutation(n) + 0.5) / n
        z = np.log(e / (1.0 - e))
        d = rng.uniform(-1.5, 1.5, n)
        a_b = sigmoid(z + d).astype(np.float32)  # run A's scores in run B's order
        b = sigmoid(z - d).astype(np.float32)
        yb = (rng.random(n) < 0.1 + 0.6 * e * e).astype(np.int64)
        ids_b = (2 ** 32 + 7 * rng.choice(10 ** 6, n, replace=False)).astype(np.int64)
        pi = rng.permutation(n)
        assert not np.array_equal(pi, np.arange(n)) and int(ids_b.min()) > 2 ** 32
        ref = _ensemble(a_b, b, "logit")
        assert ref.dtype == np.float32
        exact = sigmoid(0.5 * (logit_f64(a_b) + logit_f64(b)))
        ref_dev = max(ref_dev, float(np.abs(ref.astype(np.float64) - exact).max()))
        min_gap = min(min_gap, float(np.diff(np.sort(exact)).min()))
        splits[split] = {"ids_a": ids_b[pi].tolist(), "ids_b": ids_b.tolist(), "a": f64_list(a_b[pi]), "b": f64_list(b),
                         "y_a": yb[pi].tolist(), "y_b": yb.tolist(), "ref": f64_list(ref), "_exact": exact}
    ts = np.repeat(np.arange(42, 50), 50).astype(np.int64)
    assert min_gap >= 64 * ref_dev, (min_gap, ref_dev)
    for sp in splits.values():  # no score within the reference's deviation of a bin edge
        assert np.abs(sp.pop("_exact")[:, None] - edges[None, :]).min() > ref_dev
    pv, pt = np.asarray(splits["val"]["ref"], dtype=np.float32), np.asarray(splits["test"]["ref"], dtype=np.float32)
    yv, yt = np.asarray(splits["val"]["y_b"]), np.asarray(splits["test"]["y_b"])
    thr = _select_threshold(yv, pv, 0.0)
    gold["ensemble_logit"] = {"val": splits["val"], "test": splits["test"], "timestep_test": ts.tolist(),
                              "precision_target": 0.0, "topk": 100, "threshold": thr, "ref_dev": ref_dev,
                              "min_gap": min_gap, "metrics": _metrics_for_test(yt, pt, thr, 100, timestep_test=ts)}

    # ---- ensemble, logit mode, scores only: the clip bounds, exact 0 and 1, both tails
    rng = np.random.default_rng(26)
    lo, hi = np.float32(1e-6), np.float32(1 - 1e-6)
    zero, one = np.float32(0), np.float32(1)
    edge = np.array([0.0, 1.0, lo, np.nextafter(lo, zero), np.nextafter(lo, one), hi, np.nextafter(hi, zero),
                     np.nextafter(hi, one)], dtype=np.float32)
    a = np.repeat(edge, edge.size)  # every combination, exact 0 and 1 among them
    b = np.tile(edge, edge.size)
    p = rng.random(484)
    a = np.r_[a, (p ** 8).astype(np.float32), (1 - p ** 8).astype(np.float32), (p ** 8).astype(np.float32)]
    b = np.r_[b, (rng.random(484) ** 8).astype(np.float32), (1 - rng.random(484) ** 8).astype(np.float32),
              (1 - rng.random(484) ** 8).astype(np.float32)]
    k = 2000 - a.size
    a = np.r_[a, rng.random(k).astype(np.float32)].astype(np.float32)
    b = np.r_[b, rng.random(k).astype(np.float32)].astype(np.float32)
    assert a.size == b.size == 2000
    for u in (0.0, 1.0):
        for v in (0.0, 1.0):
            assert bool(((a == u) & (b == v)).any())
    gold["ensemble_values"] = {"a": f64_list(a), "b": f64_list(b), "ref": f64_list(_ensemble(a, b, "logit"))}

    # ---- ensemble, prob mode
    _, s_a, s_b = pattern("distinct", 27, 400)
    ref = _ensemble(s_a, s_b, "prob")
    assert ref.dtype == np.float32
    gold["ensemble_prob"] = {"a": f64_list(s_a), "b": f64_list(s_b), "ref": f64_list(ref)}

    with open(OUT, "w") as fh:
        json.dump(gold, fh, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes; ref_dev", ref_dev, "min_gap", min_gap)


if __name__ == "__main__":
    main()
