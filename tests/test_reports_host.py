"""CPU: the host paths of the run reports (rank_metrics' K19 functions and the four tools eval_by_time,
workload_curves, calibration_plots, evaluate_ensemble) against the reference's golden vectors
(tests/golden/make_reports_golden.py), the kernel-order host sums against the plain ones, and the
library's argument validation for the K19 entry points.  No device calls."""
import ctypes
import json
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from device_eval_cases import ap_tol
from reports_cases import (ECE_F32_TOL, GOLDEN, by_time_run, check_ensemble_metrics, check_logit_bounds, ensemble_runs,
                           f32, write_run)
from elliptic_gnn_project_amd import (_lib, bootstrap_compare, calibration_plots, eval_by_time, evaluate_ensemble,
                                      rank_metrics, workload_curves)

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gnnmp.h"
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
CPU = torch.device("cpu")
K19 = ("gnn_rank_hits_at_workspace_size", "gnn_rank_hits_at", "gnn_segment_threshold_counts_workspace_size",
       "gnn_segment_threshold_counts", "gnn_id_join_workspace_size", "gnn_id_join", "gnn_ensemble_pair")


# ----------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("case", GOLDEN["by_time"], ids=lambda c: c["name"])
def test_by_time_matches_the_reference(case):
    n = len(case["y"])
    rows = eval_by_time.by_time(f32(case["scores"]), np.asarray(case["y"]), np.asarray(case["timestep"]),
                                case["threshold"], CPU)
    assert [r["timestep"] for r in rows] == [r["timestep"] for r in case["rows"]]
    for got, want in zip(rows, case["rows"]):
        print(got, want)
        assert got["n"] == want["n"] and got["f1_illicit_at_thr"] == want["f1_illicit_at_thr"]
        assert abs(got["pr_auc_illicit"] - want["pr_auc_illicit"]) <= ap_tol(n)
    assert rows[2]["pr_auc_illicit"] == 0.0 and rows[5]["pr_auc_illicit"] == 1.0  # no positive / positives only


def test_workload_curve_matches_the_reference_bit_for_bit():
    g = GOLDEN["workload"]
    s, y = f32(g["scores"]), np.asarray(g["y"])
    for c in g["curves"]:
        ks, prec = workload_curves.workload_curve(s, y, c["k_max"], CPU)
        assert ks == c["ks"] == workload_curves.build_k_values(len(y), c["k_max"]) and prec == c["precision"], c["k_max"]
    t = g["tiny"]
    assert workload_curves.workload_curve(f32(t["scores"]), np.asarray(t["y"]), t["k_max"], CPU) == (t["ks"], t["precision"])
    assert workload_curves.build_k_values(25, 5000) == [10, 20, 25] and workload_curves.build_k_values(0, 10) == []
    assert workload_curves.build_k_values(7, 5000) == [7] and workload_curves.build_k_values(40, 30) == [10, 20, 30]
    assert workload_curves.workload_curve(np.zeros(0, np.float32), np.zeros(0, np.int64), 10, CPU) == ([], [])


def test_precision_curve_edges():
    y, s = np.array([1, 0, 1, -1, 0]), np.array([0.9, 0.8, 0.8, 0.99, 0.1], dtype=np.float32)
    k_eff, hits, prec = rank_metrics.precision_curve(s, y, [1, 2, 3, 4, 5, 10 ** 9])  # -1 is excluded: m = 4
    assert k_eff.tolist() == [1, 2, 3, 4, 4, 4] and hits.tolist() == [1, 1, 2, 2, 2, 2]
    assert prec.tolist() == [1.0, 0.5, 2 / 3, 0.5, 0.5, 0.5]
    for k in (1, 3):
        assert float(prec[k - 1]) == float(rank_metrics.precision_at_k(s, y, k))
    k_eff, hits, prec = rank_metrics.precision_curve(s, y, [1, 7], mask=np.zeros(5, dtype=bool))
    assert k_eff.tolist() == [0, 0] and hits.tolist() == [0, 0] and all(math.isnan(v) for v in prec.tolist())
    assert rank_metrics.precision_curve(s, y, [])[0].numel() == 0
    with pytest.raises(ValueError):
        rank_metrics.precision_curve(s, y, [3, 0])


def test_reliability_matches_the_reference():
    g = GOLDEN["reliability"]
    t = calibration_plots.reliability(f32(g["scores"]), np.asarray(g["y"]), g["bins"], CPU)
    assert t["bin_center"].tolist() == g["bin_center"] and t["count"].tolist() == g["count"]
    assert t["accuracy"].tolist() == g["accuracy"]
    d = np.abs(t["confidence"] - np.asarray(g["confidence"])).max()
    print(f"confidence |ours - reference| max {d:.3g}, ece |ours - reference| {abs(t['ece'] - g['ece']):.3g}")
    assert d <= ECE_F32_TOL and abs(t["ece"] - g["ece"]) <= ECE_F32_TOL
    assert len(g["count"]) == g["bins"] - 2 and int(np.sum(g["count"])) == len(g["y"])
    with pytest.raises(ValueError):
        rank_metrics.reliability_table(f32(g["scores"]), np.asarray(g["y"]), bins=0)


def test_ensemble_prob_is_the_reference_bit_for_bit():
    g = GOLDEN["ensemble_prob"]
    got = rank_metrics.ensemble_pair(f32(g["a"]), f32(g["b"]), "prob").numpy()
    assert got.dtype == np.float32 and got.tobytes() == f32(g["ref"]).tobytes()


def test_ensemble_logit_is_no_further_from_exact_than_the_reference():
    g = GOLDEN["ensemble_values"]
    a, b = f32(g["a"]), f32(g["b"])
    check_logit_bounds(rank_metrics.ensemble_pair(a, b, "logit").numpy(), a, b, f32(g["ref"]))
    for split in ("val", "test"):
        s = GOLDEN["ensemble_logit"][split]
        perm = rank_metrics.join_by_id(np.asarray(s["ids_b"]), np.asarray(s["ids_a"]), split)
        assert np.array_equal(np.asarray(s["ids_a"])[perm.numpy()], np.asarray(s["ids_b"]))
        a, b = f32(s["a"]), f32(s["b"])
        ours = rank_metrics.ensemble_pair(a, b, "logit", perm).numpy()
        check_logit_bounds(ours, a[perm.numpy()], b, f32(s["ref"]))
        assert ours.tobytes() == rank_metrics.ensemble_pair(a[perm.numpy()], b, "logit").numpy().tobytes()
    with pytest.raises(ValueError, match="Unknown mode"):
        rank_metrics.ensemble_pair(a, b, "mean")
    with pytest.raises(ValueError, match="NaN"):
        rank_metrics.ensemble_pair(np.array([np.nan], np.float32), np.array([0.5], np.float32))
    with pytest.raises(IndexError):
        rank_metrics.ensemble_pair(a[:2], b[:2], "prob", np.array([0, 2]))


def test_ensemble_record_matches_the_reference():
    g = GOLDEN["ensemble_logit"]
    run_a, run_b = ensemble_runs()
    arrays, m = evaluate_ensemble.ensemble(run_a, run_b, "logit", g["precision_target"], g["topk"], CPU)
    check_ensemble_metrics(m)
    assert arrays["scores_test"].dtype == np.float32 and np.array_equal(arrays["node_idx_test"], run_b["node_idx_test"])
    assert np.array_equal(arrays["y_val"], run_b["y_val"]) and arrays["scores_val"].shape == (300,)
    # the kernel-order sums are the plain host sums up to the project's bounds
    plain = rank_metrics.evaluation_record(arrays["scores_test"], run_b["y_test"], np.ones(400, dtype=bool),
                                           m["threshold"], g["topk"], 0.9)
    assert abs(plain["pr_auc_illicit"] - m["pr_auc_illicit"]) <= ap_tol(400) and abs(plain["ece"] - m["ece"]) <= 1e-12
    assert {k: v for k, v in plain.items() if k not in ("pr_auc_illicit", "ece")} == \
        {k: m[k] for k in plain if k not in ("pr_auc_illicit", "ece")}


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 3 * 1024 + 7, 9000])
def test_kernel_order_sums_equal_the_plain_sums_within_the_bounds(n):
    rng = np.random.default_rng(n)
    y = (rng.random(n) < 0.3).astype(np.int64)
    s = np.round(rng.random(n), 3).astype(np.float32)
    g = rng.integers(0, 5, n) * 3
    inc = rng.random(n) < 0.8
    v1, a1, c1 = rank_metrics.average_precision_by_group(s, y, g, inc)
    v2, a2, c2 = rank_metrics.average_precision_by_group(s, y, g, inc, device_order=True)
    assert v1.tolist() == v2.tolist() and c1.tolist() == c2.tolist()
    assert np.abs(a1.numpy() - a2.numpy()).max(initial=0.0) <= ap_tol(n)
    one = rank_metrics._host_plan_ap(*rank_metrics._host_plan(s, y, inc)[:3])[0]
    assert abs(one - float(rank_metrics.average_precision(s, y, inc))) <= ap_tol(n)
    pos = (y == 1).astype(np.int64)
    p, q = rank_metrics._host_calibration(s, pos, inc, 0.5), rank_metrics._host_calibration_device_order(s, pos, inc, 0.5)
    assert np.abs(p["bin_sum"] - q["bin_sum"]).max() <= 1e-12 * max(n, 1) and abs(p["ece"] - q["ece"]) <= 1e-12
    assert p["bin_count"].tolist() == q["bin_count"].tolist() and p["f1"] == q["f1"]


def test_threshold_counts_by_group():
    rng = np.random.default_rng(5)
    n = 500
    y, s = rng.integers(-1, 2, n), np.round(rng.random(n), 2).astype(np.float32)
    g = rng.choice([3, 8, 11, 40], n)
    thr = float(np.float32(0.37))
    vals, counts = rank_metrics.threshold_counts_by_group(s, y, g, thr)
    assert vals.tolist() == [3, 8, 11, 40] and counts.shape == (4, 4) and counts.dtype == torch.int64
    for i, v in enumerate(vals.tolist()):
        m = (g == v) & (y >= 0)
        pred = s[m].astype(np.float64) >= thr
        want = [int((pred & (y[m] == 1)).sum()), int((pred & (y[m] == 0)).sum()), int((~pred & (y[m] == 1)).sum()), int(m.sum())]
        assert counts[i].tolist() == want
    seg = np.where(g == 40, 9, 0)  # an out-of-range segment: skipped, and reported
    c, st = rank_metrics.segment_threshold_counts(s, y, seg, 3, thr, check=False)
    assert int(st) == _lib.RANK_STATUS_SEGMENT and c[1:].sum() == 0 and int(c[0, 3]) == int(((g != 40) & (y >= 0)).sum())
    with pytest.raises(IndexError):
        rank_metrics.segment_threshold_counts(s, y, seg, 3, thr)
    with pytest.raises(ValueError, match="float32"):
        rank_metrics.threshold_counts_by_group(s, y, g, 0.37)
    with pytest.raises(ValueError, match="float32"):
        rank_metrics.by_time_table(s, y, g, 0.37)


# ----------------------------------------------------------------------------- the tools' files
def test_the_four_tools_write_their_files(tmp_path, capsys):
    run = by_time_run(tmp_path / "run")
    eval_by_time.main(["--run_dir", str(run)], CPU)
    workload_curves.main(["--run_dir", str(run), "--k_max", "95"], CPU)
    calibration_plots.main(["--run_dir", str(run)], CPU)
    assert re.search(r"ECE=0\.\d{4}\n", capsys.readouterr().out)
    for name, header, rows in (("by_time.csv", "timestep,pr_auc_illicit,f1_illicit_at_thr,n", 8),
                               ("workload_curve.csv", "k,precision_at_k", 10),
                               ("calibration_curve.csv", "bin_center,accuracy,confidence,count", None)):
        lines = (run / name).read_text().splitlines()
        assert lines[0] == header and (rows is None or len(lines) == rows + 1), name
        assert all(len(ln.split(",")) == len(header.split(",")) for ln in lines), name
    assert (run / "workload_curve.csv").read_text().splitlines()[-1].startswith("95,")
    case = next(c for c in GOLDEN["by_time"] if c["name"] == "ties")
    first = (run / "by_time.csv").read_text().splitlines()[1].split(",")
    assert int(first[0]) == case["rows"][0]["timestep"] and float(first[2]) == case["rows"][0]["f1_illicit_at_thr"]
    assert int(first[3]) == 50


def test_the_ensemble_directory_is_a_run_directory(tmp_path, capsys):
    run_a, run_b = ensemble_runs()
    a = write_run(tmp_path / "a", run_a, {"best_val_pr_auc": 0.61, "threshold": 0.5})
    b = write_run(tmp_path / "b", run_b, {"best_val_pr_auc": 0.58, "threshold": 0.5})
    m = evaluate_ensemble.main(["--run_a", str(a), "--run_b", str(b)], CPU)
    out = b / "ensemble"  # the default output directory
    check_ensemble_metrics(m)
    on_disk = json.loads((out / "metrics.json").read_text())
    assert on_disk == json.loads(json.dumps(m)) and on_disk["best_val_pr_auc"] == 0.61
    assert on_disk["ensemble_sources"] == {"run_a": str(a.resolve()), "run_b": str(b.resolve()), "mode": "logit"}
    assert (out / "config_used.yaml").read_text() == \
        "run_name: ensemble_of_a_and_b\nprecision_target: 0.0\ntopk: 100\nensemble_mode: logit"
    for name in ("scores_val", "scores_test", "y_val", "y_test", "node_idx_val", "node_idx_test", "timestep_val",
                 "timestep_test"):
        assert (out / f"{name}.npy").exists(), name
    assert np.load(out / "scores_test.npy").dtype == np.float32
    assert np.array_equal(np.load(out / "node_idx_test.npy"), run_b["node_idx_test"])
    capsys.readouterr()
    # every tool that reads a run directory accepts it
    assert len(eval_by_time.main(["--run_dir", str(out)], CPU)) == 8
    assert workload_curves.main(["--run_dir", str(out)], CPU)[0][-1] == 400
    assert abs(calibration_plots.main(["--run_dir", str(out)], CPU)["ece"] - m["ece"]) == 0.0
    cmp = bootstrap_compare.main(["--run_a", str(b), "--run_b", str(out), "--n_boot", "20"])
    assert cmp["n_samples"] == 400 and (out / "bootstrap_compare.json").exists()
    # an explicit directory, the precision target and prob mode
    m2 = evaluate_ensemble.main(["--run_a", str(a), "--run_b", str(b), "--out_dir", str(tmp_path / "e2"), "--mode", "prob",
                                 "--precision_target", "0.5", "--topk", "50"], CPU)
    assert (tmp_path / "e2" / "config_used.yaml").read_text().endswith("topk: 50\nensemble_mode: prob")
    val = np.float32(0.5) * (run_a["scores_val"][rank_metrics.join_by_id(run_b["node_idx_val"], run_a["node_idx_val"]).numpy()]
                             + run_b["scores_val"])
    assert m2["threshold"] == rank_metrics.select_threshold(val, run_b["y_val"], np.ones(300, dtype=bool), 0.5)[0]


def test_join_errors_name_the_split(tmp_path):
    run_a, run_b = ensemble_runs()
    bad = dict(run_a)
    bad["node_idx_val"] = run_a["node_idx_val"].copy()
    bad["node_idx_val"][3] = bad["node_idx_val"][4]
    with pytest.raises(RuntimeError, match="VAL.*duplicate"):
        evaluate_ensemble.ensemble(bad, run_b, device=CPU)
    bad = dict(run_a)
    bad["node_idx_test"] = run_a["node_idx_test"].copy()
    bad["node_idx_test"][7] += 1
    with pytest.raises(RuntimeError, match="TEST node indices differ between runs"):
        evaluate_ensemble.ensemble(bad, run_b, device=CPU)
    bad = dict(run_a)
    bad["y_test"] = run_a["y_test"].copy()
    bad["y_test"][0] ^= 1
    with pytest.raises(RuntimeError, match="TEST labels differ"):
        evaluate_ensemble.ensemble(bad, run_b, device=CPU)
    with pytest.raises(RuntimeError, match="VAL.*negative"):
        rank_metrics.join_by_id(np.array([5, -1]), np.array([-1, 5]), "VAL")
    with pytest.raises(RuntimeError, match="differ"):
        rank_metrics.join_by_id(np.array([5, 6, 7]), np.array([5, 6]), "VAL")
    assert rank_metrics.join_by_id(np.array([9, 4]), np.array([9, 4])).tolist() == [0, 1]  # bit-equal: the identity
    assert rank_metrics.join_by_id(np.array([9, 4, 2 ** 40]), np.array([2 ** 40, 9, 4])).tolist() == [1, 2, 0]


# ----------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    return _lib.load()


def test_k19_is_additive_to_abi_32(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert int(re.search(r"#define GNNMP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gnn_abi_version() == 32
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for fn in K19:
        proto = re.search(r"gnn_status\s+%s\s*\((.*?)\)\s*;" % fn, text, re.S)
        assert proto, fn
        nargs = len([a for a in proto.group(1).split(",") if a.strip()])
        assert fn in _lib.SIGNATURES and len(_lib.SIGNATURES[fn][1]) == nargs, fn
        assert f" T {fn}\n" in exported, fn
    for name, value in (("GNN_REPORT_MAX_SEGMENTS", _lib.REPORT_MAX_SEGMENTS), ("GNN_REPORT_STATUS_K", _lib.REPORT_STATUS_K),
                        ("GNN_JOIN_STATUS_DUPLICATE", _lib.JOIN_STATUS_DUPLICATE),
                        ("GNN_JOIN_STATUS_NEGATIVE", _lib.JOIN_STATUS_NEGATIVE),
                        ("GNN_JOIN_STATUS_MISMATCH", _lib.JOIN_STATUS_MISMATCH),
                        ("GNN_ENSEMBLE_PROB", _lib.ENSEMBLE_PROB), ("GNN_ENSEMBLE_LOGIT", _lib.ENSEMBLE_LOGIT)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name


def test_k19_entry_points_validate_on_the_host(lib):
    """Bad arguments are refused before any device work; empty calls launch nothing (no GPU needed)."""
    b = _lib.c_size(0)
    one, big, imax = ctypes.c_void_p(1 << 20), 1 << 30, 2 ** 31 - 1  # never dereferenced
    g = lambda kw, k: kw.get(k, one)  # noqa: E731

    assert lib.gnn_rank_hits_at_workspace_size(-1, ctypes.byref(b)) == 1
    assert lib.gnn_rank_hits_at_workspace_size(4, None) == 1 and lib.gnn_rank_hits_at_workspace_size(imax, ctypes.byref(b)) == 1
    assert lib.gnn_rank_hits_at_workspace_size(5000, ctypes.byref(b)) == 0 and b.value >= 5000 * 4

    def hits(n=10, S=1, K=3, **kw):
        return lib.gnn_rank_hits_at(g(kw, "order"), g(kw, "seg_ptr"), g(kw, "pos"), n, S, g(kw, "ks"), K, g(kw, "k_eff"),
                                    g(kw, "hits"), g(kw, "prec"), g(kw, "status"), g(kw, "ws"), kw.get("ws_bytes", big), None)

    assert hits(n=-1) == 1 and hits(K=-1) == 1 and hits(n=imax) == 1 and hits(S=2) == 1 and hits(S=0) == 1
    for name in ("order", "seg_ptr", "pos", "ks", "k_eff", "hits", "prec", "status"):
        assert hits(**{name: None}) == 1, name
    assert b"gnn_rank_hits_at" in lib.gnn_last_error() and b"null buffer" in lib.gnn_last_error()
    assert hits(ws=None) == 4 and hits(ws_bytes=0) == 4 and hits(n=5000, ws_bytes=5000 * 4 - 1) == 4
    assert b"workspace too small" in lib.gnn_last_error()
    assert hits(K=0, order=None, ks=None, ws=None, ws_bytes=0) == 0  # no k: a no-op

    assert lib.gnn_segment_threshold_counts_workspace_size(-1, 3, ctypes.byref(b)) == 1
    assert lib.gnn_segment_threshold_counts_workspace_size(4, -1, ctypes.byref(b)) == 1
    assert lib.gnn_segment_threshold_counts_workspace_size(4, 3, None) == 1
    assert lib.gnn_segment_threshold_counts_workspace_size(4, _lib.REPORT_MAX_SEGMENTS + 1, ctypes.byref(b)) == 1
    assert lib.gnn_segment_threshold_counts_workspace_size(10000, 49, ctypes.byref(b)) == 0 and b.value >= 3 * 49 * 16

    def seg(n=10, S=3, thr=0.5, **kw):
        return lib.gnn_segment_threshold_counts(g(kw, "scores"), g(kw, "pos"), kw.get("include", None), g(kw, "segment"),
                                                n, S, thr, g(kw, "counts"), g(kw, "status"), g(kw, "ws"),
                                                kw.get("ws_bytes", big), None)

    assert seg(n=-1) == 1 and seg(S=-1) == 1 and seg(S=_lib.REPORT_MAX_SEGMENTS + 1) == 1
    assert seg(thr=0.37) == 1 and b"float32" in lib.gnn_last_error()
    assert seg(thr=float("nan")) == 1
    for name in ("scores", "pos", "segment", "counts", "status"):
        assert seg(**{name: None}) == 1, name
    assert seg(ws=None) == 4 and seg(ws_bytes=0) == 4 and seg(n=10000, S=49, ws_bytes=3 * 49 * 16 - 1) == 4
    assert seg(S=0, scores=None, counts=None, ws=None, ws_bytes=0) == 0  # no group: a no-op

    assert lib.gnn_id_join_workspace_size(-1, ctypes.byref(b)) == 1 and lib.gnn_id_join_workspace_size(4, None) == 1
    assert lib.gnn_id_join_workspace_size(imax, ctypes.byref(b)) == 1

    def join(n=10, **kw):
        return lib.gnn_id_join(g(kw, "base"), g(kw, "other"), n, g(kw, "perm"), g(kw, "status"), g(kw, "ws"),
                               kw.get("ws_bytes", big), None)

    assert join(n=-1) == 1 and join(n=imax) == 1
    for name in ("base", "other", "perm", "status"):
        assert join(**{name: None}) == 1, name
    assert join(ws=None) == 4 and join(ws_bytes=0) == 4
    assert join(n=1000, ws_bytes=1000 * (8 + 8 + 4 + 4 + 4) - 1) == 4  # below its five arrays of n
    assert b"gnn_id_join" in lib.gnn_last_error() and b"workspace too small" in lib.gnn_last_error()
    assert join(n=0, base=None, other=None, perm=None, ws=None, ws_bytes=0) == 0

    def ens(n=10, mode=1, **kw):
        return lib.gnn_ensemble_pair(g(kw, "a"), g(kw, "b"), kw.get("perm", None), n, mode, g(kw, "out"), g(kw, "status"), None)

    assert ens(n=-1) == 1 and ens(n=imax) == 1 and ens(mode=2) == 1 and ens(mode=-1) == 1
    assert b"mode" in lib.gnn_last_error()
    for name in ("a", "b", "out", "status"):
        assert ens(**{name: None}) == 1, name
    assert ens(n=0, a=None, b=None, out=None) == 0
