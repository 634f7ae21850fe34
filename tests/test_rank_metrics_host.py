"""CPU: the host path of rank_metrics (the kernels' oracle) against the reference's own metrics
(tests/golden/bootstrap_golden.json, written by make_bootstrap_golden.py from the reference modules;
metrics_golden.json), the library's argument validation for the K14 entry points, and the
bootstrap_compare entry point.  No device calls."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from elliptic_gnn_project_amd import _lib, bootstrap_compare, metrics, rank_metrics

GOLD = Path(__file__).parent / "golden"


def ap_tol(n: int) -> float:
    """A few f64 ulps per tie group, at most n groups."""
    return max(1e-12, 4 * n * 2.0 ** -53)


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLD / "bootstrap_golden.json").read_text())["cases"]


def _case(c):
    return (np.asarray(c["y"], dtype=np.int64), np.asarray(c["s_a"], dtype=np.float32),
            np.asarray(c["s_b"], dtype=np.float32))


def test_golden_inputs_meet_their_conditions(golden):
    names = {c["name"]: c for c in golden}
    assert set(names) == {"distinct", "ties"}
    for c in golden:
        y, sa, sb = _case(c)
        assert int(y.sum()) >= 20 and c["n_boot"] == 50 and len(c["replicates"]["ap_a"]) == 5
        assert np.array_equal(sa.astype(np.float64), np.asarray(c["s_a"]))  # float32 values, stored exactly
    y, sa, sb = _case(names["distinct"])
    n = len(y)
    assert np.array_equal(np.sort(sa), ((np.arange(n) + 0.5) / n).astype(np.float32))
    assert len(np.unique(sb)) == n
    y, sa, _ = _case(names["ties"])
    assert np.array_equal(sa, np.round(sa.astype(np.float64), 2).astype(np.float32)) and len(np.unique(sa)) < len(y) // 2


def test_host_ap_matches_reference(golden):
    for c in golden:
        y, sa, sb = _case(c)
        tol = ap_tol(len(y))
        assert abs(float(rank_metrics.average_precision(sa, y)) - c["ap_a"]) <= tol
        assert abs(float(rank_metrics.average_precision(torch.from_numpy(sb), torch.from_numpy(y))) - c["ap_b"]) <= tol


def test_host_replicates_match_reference(golden):
    for c in golden:
        y, sa, sb = _case(c)
        n = len(y)
        rng = np.random.default_rng(c["seed"])
        idx = np.stack([rng.choice(n, size=n, replace=True) for _ in range(5)])
        ap_a, ap_b, pk_a, pk_b = (v.numpy() for v in rank_metrics.replicate_metrics(y, sa, sb, idx, c["topk"]))
        assert np.abs(ap_a - np.asarray(c["replicates"]["ap_a"])).max() <= ap_tol(n)
        assert np.abs(ap_b - np.asarray(c["replicates"]["ap_b"])).max() <= ap_tol(n)
        if c["name"] == "distinct":  # P@k: exact where the reference's own result is defined
            assert pk_a.tolist() == c["replicates"]["patk_a"]
            assert pk_b.tolist() == c["replicates"]["patk_b"]


def test_host_patk_exact_on_distinct_scores(golden):
    c = next(c for c in golden if c["name"] == "distinct")
    y, sa, sb = _case(c)
    assert float(rank_metrics.precision_at_k(sa, y, c["topk"])) == c["patk_a"]
    assert float(rank_metrics.precision_at_k(sb, y, c["topk"])) == c["patk_b"]
    assert float(rank_metrics.precision_at_k(sa, y, len(y) + 5)) == float(y.mean())  # k clamps to n


def test_host_bootstrap_summary_matches_reference(golden):
    for c in golden:
        y, sa, sb = _case(c)
        got = rank_metrics.paired_bootstrap(y, sa, sb, c["topk"], c["n_boot"], c["seed"])
        assert set(got) == {"delta_pr_auc", "delta_p_at_k"}
        keys = ["delta_pr_auc"] + (["delta_p_at_k"] if c["name"] == "distinct" else [])  # ties: AP only
        for key in keys:
            assert set(got[key]) == {"delta", "ci_low", "ci_high"}
            for f in ("delta", "ci_low", "ci_high"):
                assert abs(got[key][f] - c["bootstrap"][key][f]) <= 1e-12, (c["name"], key, f)


def test_bootstrap_chunking_keeps_the_rng_stream(golden, monkeypatch):
    c = golden[0]
    y, sa, sb = _case(c)
    whole = rank_metrics.paired_bootstrap(y, sa, sb, c["topk"], 12, 7)
    monkeypatch.setattr(rank_metrics, "BOOT_CHUNK_ELEMS", 5 * len(y))  # 5 replicates per chunk: 5 + 5 + 2
    assert rank_metrics.paired_bootstrap(y, sa, sb, c["topk"], 12, 7) == whole


def test_host_ap_matches_pr_auc_illicit_on_metrics_golden():
    g = json.loads((GOLD / "metrics_golden.json").read_text())
    for c in g["cases"] + [g["reference_unit_case"]]:
        y, s = np.asarray(c["y"]), np.asarray(c["s"])
        assert abs(float(rank_metrics.average_precision(s, y)) - c["pr_auc"]) <= ap_tol(len(y))
        assert abs(float(rank_metrics.average_precision(s, y)) - metrics.pr_auc_illicit(y, s)) <= ap_tol(len(y))


def test_host_masks_groups_and_edge_cases():
    rng = np.random.default_rng(5)
    n = 500
    y = rng.integers(-1, 2, n)  # -1 unknown: excluded by default
    s = np.round(rng.random(n), 1).astype(np.float32)
    s[::7] = -0.0
    s[3::7] = 0.0
    m = y >= 0
    assert abs(float(rank_metrics.average_precision(s, y)) - metrics.pr_auc_illicit(y[m] == 1, s[m])) <= ap_tol(n)
    g = rng.integers(3, 9, n)
    g[g == 5] = 6  # no group 5
    y[g == 4] = np.minimum(y[g == 4], 0)  # group 4 without a positive -> 0.0
    vals, ap, cnt = rank_metrics.average_precision_by_group(s, y, g)
    assert vals.tolist() == [3, 4, 6, 7, 8]
    for v, a, k in zip(vals.tolist(), ap.tolist(), cnt.tolist()):
        mm = (y >= 0) & (g == v)
        assert k == int(mm.sum())
        want = 0.0 if v == 4 else metrics.pr_auc_illicit(y[mm] == 1, s[mm])
        assert abs(a - want) <= ap_tol(n)
    assert float(rank_metrics.average_precision(s, np.zeros(n, dtype=int))) == 0.0  # P = 0
    assert float(rank_metrics.average_precision(s[:0], y[:0])) == 0.0
    with pytest.raises(ValueError):
        rank_metrics.average_precision(np.array([0.1, np.nan], dtype=np.float32), np.array([1, 0]))
    assert float(rank_metrics.average_precision(np.array([0.1, np.nan], dtype=np.float32), np.array([1, -1]))) == 1.0


def test_abi_29_and_rank_entry_points_validate_before_device_work():
    lib = _lib.load()
    assert lib.gnn_abi_version() >= 29 and _lib.ABI_VERSION >= 29
    b = _lib.c_size(0)
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused on its arguments
    for fn in (lib.gnn_rank_plan_workspace_size, lib.gnn_rank_ap_workspace_size, lib.gnn_rank_bootstrap_workspace_size):
        assert fn(-1, 1, ctypes.byref(b)) == 1
        assert fn(4, -1, ctypes.byref(b)) == 1
        assert fn(4, 1, None) == 1
    plan = lambda n, S, **kw: lib.gnn_rank_plan_build(  # noqa: E731
        kw.get("scores", one), None, None, n, S, kw.get("order", one), one, kw.get("seg_ptr", one), None,
        kw.get("status", one), one, 1 << 20, None)
    assert plan(-1, 1) == 1 and plan(4, -1) == 1
    assert plan(4, 1, scores=None) == 1 and plan(4, 1, order=None) == 1
    assert plan(4, 1, seg_ptr=None) == 1 and plan(4, 1, status=None) == 1
    assert b"gnn_rank_plan_build" in lib.gnn_last_error()
    ap = lambda n, S, k, **kw: lib.gnn_rank_ap(  # noqa: E731
        kw.get("order", one), one, one, kw.get("pos", one), n, S, k, kw.get("ap", one), one, one, kw.get("patk", one),
        one, 1 << 20, None)
    assert ap(-1, 1, 1) == 1 and ap(4, -1, 1) == 1 and ap(4, 1, 0) == 1 and ap(4, 1, -3) == 1
    assert ap(4, 1, 1, order=None) == 1 and ap(4, 1, 1, pos=None) == 1 and ap(4, 1, 1, ap=None) == 1
    boot = lambda n, B, k, **kw: lib.gnn_rank_bootstrap(  # noqa: E731
        kw.get("order", one), one, one, one, one, one, one, kw.get("idx", one), n, B, k, kw.get("out", one), one, one,
        one, kw.get("status", one), one, kw.get("ws", 1 << 20), None)
    assert boot(-1, 2, 1) == 1 and boot(4, -1, 1) == 1 and boot(4, 2, 0) == 1
    assert boot(4, 2, 1, order=None) == 1 and boot(4, 2, 1, idx=None) == 1 and boot(4, 2, 1, out=None) == 1
    assert boot(4, 2, 1, status=None) == 1
    assert boot(_lib.RANK_BOOT_LDS_MAX_N + 1, 2, 1, ws=4096) == 4  # the global-count path needs its workspace
    assert _lib.check(lib.gnn_rank_bootstrap_workspace_size(_lib.RANK_BOOT_LDS_MAX_N + 1, 2, ctypes.byref(b))) is None
    assert b.value >= 2 * 2 * (_lib.RANK_BOOT_LDS_MAX_N + 1) * 4
    with pytest.raises(ValueError):
        rank_metrics.precision_at_k(np.zeros(3, dtype=np.float32), np.zeros(3, dtype=int), 0)


def test_header_constants_match_the_binding():
    text = (Path(__file__).resolve().parents[1] / "include" / "gnnmp.h").read_text()
    for name, val in (("GNN_RANK_TILE", _lib.RANK_TILE), ("GNN_RANK_BOOT_LDS_MAX_N", _lib.RANK_BOOT_LDS_MAX_N),
                      ("GNN_RANK_STATUS_NAN", _lib.RANK_STATUS_NAN), ("GNN_RANK_STATUS_SEGMENT", _lib.RANK_STATUS_SEGMENT),
                      ("GNN_RANK_STATUS_INDEX", _lib.RANK_STATUS_INDEX), ("GNNMP_ABI_VERSION", _lib.ABI_VERSION)):
        assert f"#define {name} {val}" in " ".join(text.split()), name


def _write_run(d: Path, y, s, nodes):
    d.mkdir(parents=True)
    np.save(d / "y_test.npy", y)
    np.save(d / "scores_test.npy", s)
    np.save(d / "node_idx_test.npy", nodes)


def test_bootstrap_compare_cli_writes_the_reference_files(tmp_path, golden, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # host path (this test is not a GPU test)
    c = next(c for c in golden if c["name"] == "distinct")
    y, sa, sb = _case(c)
    n = len(y)
    nodes = np.arange(100, 100 + n)
    perm = np.random.default_rng(0).permutation(n)[: n - 10]  # run B: other order, 10 nodes fewer
    _write_run(tmp_path / "run_a", y, sa, nodes)
    _write_run(tmp_path / "run_b", y[perm], sb[perm], nodes[perm])
    out = bootstrap_compare.main(["--run_a", str(tmp_path / "run_a"), "--run_b", str(tmp_path / "run_b"),
                                  "--topk", "25", "--n_boot", "20", "--seed", "3", "--out_dir", str(tmp_path / "x")])
    files = [tmp_path / "run_b" / "bootstrap_compare.json", tmp_path / "run_b" / "bootstrap_compare_run_a.json",
             tmp_path / "run_a" / "bootstrap_compare_run_b.json", tmp_path / "x" / "bootstrap_compare.json"]
    for f in files:
        assert json.loads(f.read_text()) == out
    assert list(out) == ["run_a", "run_b", "n_samples", "n_bootstrap", "top_k", "delta_pr_auc", "delta_p_at_k",
                         "pr_auc", "precision_at_k"]
    assert out["n_samples"] == n - 10 and out["n_bootstrap"] == 20 and out["top_k"] == 25
    keep = np.sort(perm)  # aligned order: ascending node index
    assert abs(out["pr_auc"]["run_a"] - metrics.pr_auc_illicit(y[keep], sa[keep])) <= ap_tol(n)
    assert out["precision_at_k"]["run_b"] == metrics.precision_at_k(y[keep], sb[keep], 25)
    want = rank_metrics.paired_bootstrap(y[keep], sa[keep], sb[keep], 25, 20, 3)
    assert out["delta_pr_auc"] == want["delta_pr_auc"] and out["delta_p_at_k"] == want["delta_p_at_k"]
    for key in ("delta_pr_auc", "delta_p_at_k"):
        assert list(out[key]) == ["delta", "ci_low", "ci_high"]
