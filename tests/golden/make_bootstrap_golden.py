"""Golden vectors for elliptic_gnn_project_amd/rank_metrics.py, produced by the REFERENCE modules
(src/utils/metrics.py and src/analysis/bootstrap_compare.py of the reference checkout, importable
here: they need only numpy and sklearn).

    python tests/golden/make_bootstrap_golden.py <reference checkout>   # writes tests/golden/bootstrap_golden.json

Needs a checkout of the reference, so it is not run by the tests; the JSON it writes is the
committed fixture tests/test_rank_metrics_host.py and tests/test_gpu_rank_metrics.py check against.  Scores are float32 values (stored exactly as JSON doubles), as softmax outputs are.
"""
import json
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bootstrap_golden.json")
N_BOOT, TOPK, SEED, N_REP = 50, 25, 42, 5


def main():
    sys.path.insert(0, sys.argv[1])  # the reference checkout (imported as the package src)
    from src.analysis.bootstrap_compare import paired_bootstrap
    from src.utils.metrics import pr_auc_illicit, precision_at_k

    cases = []
    for name, seed, n in [("distinct", 10, 400), ("ties", 11, 300)]:
        rng = np.random.default_rng(seed)
        y = (rng.random(n) < 0.15).astype(np.int64)
        y[:20] = 1  # at least 20 positives: every replicate draws one (P(no positive) < (1 - 20/n)^n ~ e^-20)
        rng.shuffle(y)
        assert int(y.sum()) >= 20
        if name == "distinct":  # (perm + 0.5)/n: distinct scores, P@k parity; B = A nudged towards the labels
            s_a = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
            rk = np.argsort(np.argsort(s_a + 0.25 * y + 0.1 * rng.random(n)))
            s_b = ((rk + 0.5) / n).astype(np.float32)
            assert len(np.unique(s_a)) == n and len(np.unique(s_b)) == n
        else:  # rounded to 2 decimals: tie-heavy (AP only)
            s_a = np.round(np.clip(0.3 * y + 0.7 * rng.random(n), 0, 1), 2).astype(np.float32)
            s_b = np.round(np.clip(0.4 * y + 0.6 * rng.random(n), 0, 1), 2).astype(np.float32)
            assert len(np.unique(s_a)) < n // 2
        case = {"name": name, "y": y.tolist(), "s_a": s_a.astype(np.float64).tolist(),
                "s_b": s_b.astype(np.float64).tolist(), "topk": TOPK, "n_boot": N_BOOT, "seed": SEED,
                "ap_a": pr_auc_illicit(y, s_a), "ap_b": pr_auc_illicit(y, s_b),
                "bootstrap": paired_bootstrap(y, s_a, y, s_b, TOPK, N_BOOT, SEED)}
        if name == "distinct":
            case["patk_a"] = precision_at_k(y, s_a, TOPK)
            case["patk_b"] = precision_at_k(y, s_b, TOPK)
        rng2 = np.random.default_rng(SEED)  # the first replicates of the same stream
        rep = {"ap_a": [], "ap_b": [], "patk_a": [], "patk_b": []}
        for _ in range(N_REP):
            idx = rng2.choice(n, size=n, replace=True)
            rep["ap_a"].append(pr_auc_illicit(y[idx], s_a[idx]))
            rep["ap_b"].append(pr_auc_illicit(y[idx], s_b[idx]))
            if name == "distinct":
                rep["patk_a"].append(precision_at_k(y[idx], s_a[idx], TOPK))
                rep["patk_b"].append(precision_at_k(y[idx], s_b[idx], TOPK))
        case["replicates"] = rep
        cases.append(case)
    with open(OUT, "w") as fh:
        json.dump({"source": "src/utils/metrics.py, src/analysis/bootstrap_compare.py", "cases": cases}, fh)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
