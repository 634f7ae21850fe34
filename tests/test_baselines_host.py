"""CPU: the host mirrors of the feature-only baseline (logreg.py, calibrate.py's score calibrators,
train_baselines.main) against sklearn's golden vectors (tests/golden/make_baselines_golden.py), the tools
that read the run directory it writes, and the library's argument validation for the K20 entry points.
No device calls."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import baselines_cases as bc
from elliptic_gnn_project_amd import _lib, bootstrap_compare, calibrate, eval_by_time, logreg, rank_metrics, train_baselines

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gnnmp.h"
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
CPU = torch.device("cpu")
GOLDEN = bc.load_golden()
K20 = ("gnn_column_moments_workspace_size", "gnn_column_moments", "gnn_logreg_eval_workspace_size", "gnn_logreg_eval",
       "gnn_logreg_predict", "gnn_isotonic_fit_workspace_size", "gnn_isotonic_fit", "gnn_isotonic_apply")


# ----------------------------------------------------------------------------- logistic regression
@pytest.fixture(scope="module")
def lr_fits():
    """Every golden case fitted once by the host mirror: name -> (x, y, model, probabilities)."""
    out = {}
    for name, (n, D, cw, _) in bc.LR_CASES.items():
        x, y = bc.lr_inputs(name)
        assert np.array_equal(bc.x_checksum(x), GOLDEN[f"lr/{name}/checksum"]), "the seeded inputs changed"
        assert np.array_equal(y, GOLDEN[f"lr/{name}/y"])
        m = logreg.fit(x, y, None, 1.0, cw, 2000)
        out[name] = (x, y, m, logreg.predict_proba(m, x))
    return out


@pytest.mark.parametrize("name", list(bc.LR_CASES))
def test_host_fit_matches_sklearns_minimiser(lr_fits, name):
    x, y, m, p = lr_fits[name]
    dp = np.abs(p - GOLDEN[f"lr/{name}/prob"]).max()
    dc = max(np.abs(m.w - GOLDEN[f"lr/{name}/coef"]).max(), abs(m.b - float(GOLDEN[f"lr/{name}/intercept"][0])))
    print(f"{name}: {m.iterations} updates, |p - sklearn| {dp:.3g}, |theta - sklearn| {dc:.3g}")
    assert m.status == 0 and dp <= bc.PROB_TOL and dc <= bc.COEF_TOL
    assert logreg.predict_proba(m, x, None, np.float32).tobytes() == p.astype(np.float32).tobytes()


@pytest.mark.parametrize("name", list(bc.LR_CASES))
def test_host_fit_is_no_worse_than_the_references_lbfgs(lr_fits, name):
    """One formula, f64: F at our theta against F at the theta the reference's setting stops at."""
    x, y, m, _ = lr_fits[name]
    n, D, cw, _ = bc.LR_CASES[name]
    rows = np.arange(n)
    z = logreg.host_z(x, rows, m.mu, m.sd)
    w0, w1 = logreg.class_weights(y == 1, cw)
    ours = logreg.host_eval(z, y == 1, w0, w1, 1.0, m.theta, True)[0]
    theirs = logreg.host_eval(z, y == 1, w0, w1, 1.0, GOLDEN[f"lr/{name}/lbfgs_theta"], True)[0]
    print(f"{name}: F ours {ours!r}, F lbfgs {theirs!r} (recorded {float(GOLDEN[f'lr/{name}/lbfgs_F'][0])!r})")
    assert ours <= theirs and abs(theirs - float(GOLDEN[f"lr/{name}/lbfgs_F"][0])) <= 1e-9 * abs(theirs)


def test_constant_column_standardises_to_zero(lr_fits):
    _, _, m, _ = lr_fits["n500_d10_constcol"]
    assert m.sd[3] == 1.0 and m.mu[3] == 2.5 and m.w[3] == 0.0


@pytest.mark.parametrize("name", ["n257_d1", "n1000_d165_bal", "n300_d64_separable"])
def test_row_permutation_moves_the_probabilities_below_1e_12(lr_fits, name):
    x, y, m, p = lr_fits[name]
    n, _, cw, _ = bc.LR_CASES[name]
    perm = np.random.default_rng(3).permutation(n)
    m2 = logreg.fit(x, y, perm, 1.0, cw, 2000)
    d = np.abs(logreg.predict_proba(m2, x) - p).max()
    print(f"{name}: permutation moves p by {d:.3g}")
    assert d < 1e-12


def test_fit_refuses_bad_input():
    x = np.random.default_rng(0).standard_normal((40, 3)).astype(np.float32)
    y = np.zeros(40, dtype=np.int64)
    with pytest.raises(ValueError, match="single class"):
        logreg.fit(x, y)
    y[:7] = 1
    with pytest.raises(ValueError, match="single class"):
        logreg.fit(x, y, rows=np.arange(7))
    with pytest.raises(ValueError, match="D = 256"):
        logreg.fit(np.zeros((4, 256), np.float32), y[:4])
    with pytest.raises(IndexError):
        logreg.fit(x, y, rows=np.array([0, 40]))
    with pytest.raises(ValueError, match="class_weight"):
        logreg.fit(x, y, class_weight="auto")
    with pytest.raises(ValueError, match="NaN"):
        bad = x.copy()
        bad[3, 1] = np.nan
        logreg.fit(bad, y)
    m = logreg.fit(x, y, class_weight={0: 1.0, 1: 3.0})
    assert m.status == 0 and m.mu.shape == (3,)
    with pytest.warns(RuntimeWarning, match="MAXIT"):
        assert logreg.fit(x, y, max_iter=1).status == logreg.STATUS_MAXIT


# ----------------------------------------------------------------------------- calibrators
@pytest.mark.parametrize("pattern,n", bc.CAL_CASES, ids=lambda v: str(v))
def test_host_isotonic_is_sklearns_bit_for_bit(pattern, n):
    name = bc.cal_name(pattern, n)
    s, y = GOLDEN[f"cal/{name}/scores"], GOLDEN[f"cal/{name}/y"].astype(np.int64)
    assert np.array_equal(s, bc.calibrator_inputs(pattern, n)[0])
    cal = calibrate.fit_isotonic(s, y)
    assert cal.kind == "isotonic" and cal.xs.dtype == np.float64
    assert cal.xs.tobytes() == GOLDEN[f"cal/{name}/xs"].tobytes(), "thresholds"
    q = GOLDEN[f"cal/{name}/queries"]
    out = calibrate.apply_calibrator(cal, q, np.float64)
    # bit-equal, except where the generator measured sklearn's float pooling off the rounded P / W: 4 ulp there
    bound = 0 if int(GOLDEN[f"cal/{name}/ulp"][0]) == 0 else 4
    d = max(bc.ulp_distance(cal.ys, GOLDEN[f"cal/{name}/ys"]), bc.ulp_distance(out, GOLDEN[f"cal/{name}/iso"]))
    print(f"{name}: K = {cal.xs.size}, {d} ulp from sklearn (bound {bound})")
    assert d <= bound
    assert calibrate.apply_calibrator(cal, q).tobytes() == out.astype(np.float32).tobytes()
    # a mask and labels outside {0, 1} select the same fit
    s2, y2 = np.concatenate([s, [np.float32(0.5), np.float32(np.nan)]]), np.concatenate([y, [-1, -1]])
    c2 = calibrate.fit_isotonic(torch.from_numpy(s2), torch.from_numpy(y2))
    assert c2.xs.tobytes() == cal.xs.tobytes() and c2.ys.tobytes() == cal.ys.tobytes()


@pytest.mark.parametrize("pattern,n", [c for c in bc.CAL_CASES if f"cal/{bc.cal_name(*c)}/platt" in GOLDEN],
                         ids=lambda v: str(v))
def test_host_platt_matches_sklearns_minimiser(pattern, n):
    name = bc.cal_name(pattern, n)
    s, y = GOLDEN[f"cal/{name}/scores"], GOLDEN[f"cal/{name}/y"].astype(np.int64)
    cal = calibrate.fit_platt(s, y)
    out = calibrate.apply_calibrator(cal, GOLDEN[f"cal/{name}/queries"], np.float64)
    dp = np.abs(out - GOLDEN[f"cal/{name}/platt"]).max()
    dc = np.abs(np.array([cal.w, cal.b]) - GOLDEN[f"cal/{name}/platt_theta"]).max()
    print(f"{name}: |p - sklearn| {dp:.3g}, |theta - sklearn| {dc:.3g}")
    assert cal.kind == "platt" and dp <= bc.PROB_TOL and dc <= bc.COEF_TOL


def test_calibrator_edges():
    s, y = np.array([0.2, 0.7, 0.4], np.float32), np.array([0, 1, 1])
    for fit in (calibrate.fit_isotonic, calibrate.fit_platt):
        with pytest.raises(ValueError, match="NaN"):
            fit(np.array([0.2, np.nan], np.float32), np.array([0, 1]))
        cal = fit(s, y, mask=np.zeros(3, dtype=bool))
        assert cal.kind == "identity" and cal.status == _lib.FIT_STATUS_EMPTY
        assert calibrate.apply_calibrator(cal, s).tobytes() == s.tobytes()
        assert fit(np.zeros(0, np.float32), np.zeros(0, np.int64)).kind == "identity"
    with pytest.raises(ValueError, match="NaN"):
        calibrate.apply_calibrator(calibrate.fit_isotonic(s, y), np.array([np.nan], np.float32))
    with pytest.raises(ValueError, match="single class"):
        calibrate.fit_platt(s, np.ones(3, dtype=np.int64))
    # -0.0 and +0.0 are one point; equal means pool (2 of 4 then 1 of 2)
    cal = calibrate.fit_isotonic(np.array([-0.0, 0.0, 0.0, 0.0, 1.0, 1.0], np.float32), np.array([1, 1, 0, 0, 1, 0]))
    assert cal.xs.tolist() == [0.0, 1.0] and cal.ys.tolist() == [0.5, 0.5] and not np.signbit(cal.xs[0])
    assert calibrate.apply_calibrator(cal, np.array([0.3], np.float32), np.float64).tolist() == [0.5]


# ----------------------------------------------------------------------------- the tool
def small_cfg(tmp_path, **kw):
    cfg = dict(run_name="lr_small", seed=1, model="logistic_regression", calibration="isotonic", C=1.0, max_iter=2000,
               class_weight="balanced", device="cpu", n_jobs=4, topk=20, precision_target=0.0, output_root=str(tmp_path),
               graph_file=str(tmp_path / "absent.npz"),
               synthetic=dict(num_nodes=1500, num_edges=2000, num_feats=12, seed=5, num_illicit=150, num_licit=900))
    cfg.update(kw)
    return cfg


FILES = [f"{a}_{s}.npy" for a in ("scores", "scores_raw", "y", "node_idx", "timestep") for s in ("val", "test")] + \
        ["metrics.json", "model.npz"]


@pytest.mark.parametrize("calibration", ["none", "isotonic", "platt"])
def test_main_writes_a_run_directory_the_tools_accept(tmp_path, capsys, calibration):
    m = train_baselines.main(small_cfg(tmp_path, calibration=calibration))
    run = tmp_path / "baselines" / "lr_small"
    for f in FILES:
        assert (run / f).exists(), f
    assert tuple(m) == rank_metrics.RECORD_KEYS and json.loads((run / "metrics.json").read_text()) == json.loads(json.dumps(m))
    s, raw, y = np.load(run / "scores_test.npy"), np.load(run / "scores_raw_test.npy"), np.load(run / "y_test.npy")
    assert s.dtype == raw.dtype == np.float32 and m["n_test"] == len(y) == len(s) and set(np.unique(y)) <= {0, 1}
    z = np.load(run / "model.npz")
    assert str(z["calibration"]) == {"none": "identity"}.get(calibration, calibration) and z["w"].shape == (12,)
    if calibration == "none":
        assert s.tobytes() == raw.tobytes()
    if calibration == "isotonic":
        cal = calibrate.fit_isotonic(np.load(run / "scores_raw_val.npy"), np.load(run / "y_val.npy"))
        assert cal.xs.tobytes() == z["cal_xs"].tobytes() and calibrate.apply_calibrator(cal, raw).tobytes() == s.tobytes()
    thr = rank_metrics.select_threshold(np.load(run / "scores_val.npy"), np.load(run / "y_val.npy"))[0]
    assert m["threshold"] == thr == float(np.float32(thr))
    capsys.readouterr()
    rows = eval_by_time.main(["--run_dir", str(run)], CPU)
    assert sum(r["n"] for r in rows) == len(y)
    other = train_baselines.main(small_cfg(tmp_path, run_name="lr_c01", C=0.1, calibration=calibration))
    assert other["n_test"] == m["n_test"]
    cmp = bootstrap_compare.main(["--run_a", str(run), "--run_b", str(tmp_path / "baselines" / "lr_c01"), "--n_boot", "20"])
    assert cmp["n_samples"] == len(y)


def test_main_options(tmp_path):
    with pytest.raises(NotImplementedError, match="DESIGN.md §7"):
        train_baselines.main(small_cfg(tmp_path, model="xgboost"))
    with pytest.raises(ValueError, match="Unknown baseline model"):
        train_baselines.main(small_cfg(tmp_path, model="svm"))
    with pytest.raises(ValueError, match="calibration"):
        train_baselines.main(small_cfg(tmp_path, calibration="beta"))
    a = train_baselines.main(small_cfg(tmp_path, precision_target=0.5, train_window_k=5))
    run = tmp_path / "baselines" / "lr_small"
    sv, yv = np.load(run / "scores_val.npy"), np.load(run / "y_val.npy")
    assert a["threshold"] == rank_metrics.select_threshold(sv, yv, None, 0.5)[0]
    b = train_baselines.main(small_cfg(tmp_path, use_val_for_thresholds=False))
    assert b["threshold"] == rank_metrics.select_threshold(np.load(run / "scores_test.npy"), np.load(run / "y_test.npy"))[0]
    cfg = (ROOT / "configs" / "baseline_lr.yaml").read_text()
    import yaml

    c = yaml.safe_load(cfg)
    assert (c["model"], c["calibration"], c["C"], c["max_iter"], c["class_weight"]) == \
        ("logistic_regression", "isotonic", 1.0, 2000, "balanced")


# ----------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    return _lib.load()


def test_k20_is_additive_to_abi_32(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert int(re.search(r"#define GNNMP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gnn_abi_version() == 32
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for fn in K20:
        proto = re.search(r"gnn_status\s+%s\s*\((.*?)\)\s*;" % fn, text, re.S)
        assert proto, fn
        nargs = len([a for a in proto.group(1).split(",") if a.strip()])
        assert fn in _lib.SIGNATURES and len(_lib.SIGNATURES[fn][1]) == nargs, fn
        assert f" T {fn}\n" in exported, fn
    for name, value in (("GNN_LOGREG_MAX_D", _lib.LOGREG_MAX_D), ("GNN_LOGREG_ROWS", _lib.LOGREG_ROWS),
                        ("GNN_LOGREG_REDUCE_UNROLL", _lib.LOGREG_REDUCE_UNROLL), ("GNN_ISOTONIC_CHUNK", _lib.ISOTONIC_CHUNK),
                        ("GNN_BASELINE_STATUS_ROW", _lib.BASELINE_STATUS_ROW),
                        ("GNN_BASELINE_STATUS_NAN", _lib.BASELINE_STATUS_NAN)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name


def test_k20_entry_points_validate_on_the_host(lib):
    """Bad arguments are refused before any device work; empty calls launch nothing (no GPU needed)."""
    b = _lib.c_size(0)
    one, imax = ctypes.c_void_p(1 << 20), 2 ** 31 - 1  # never dereferenced
    INVALID, WORKSPACE = 1, 4
    assert lib.gnn_status_string(WORKSPACE).decode().lower().find("workspace") >= 0

    for size in (lib.gnn_column_moments_workspace_size, lib.gnn_logreg_eval_workspace_size):
        assert size(-1, 4, ctypes.byref(b)) == INVALID and size(4, 0, ctypes.byref(b)) == INVALID
        assert size(4, 256, ctypes.byref(b)) == INVALID and size(4, 4, None) == INVALID
        assert size(0, 255, ctypes.byref(b)) == 0 and b.value > 0
    assert lib.gnn_isotonic_fit_workspace_size(-1, ctypes.byref(b)) == INVALID
    assert lib.gnn_isotonic_fit_workspace_size(imax, ctypes.byref(b)) == INVALID
    assert lib.gnn_isotonic_fit_workspace_size(4, None) == INVALID
    assert lib.gnn_isotonic_fit_workspace_size(0, ctypes.byref(b)) == 0 and b.value > 0

    def moments(x=one, ld=4, N=8, rows=one, n=8, D=4, mu=one, sd=one, st=one, ws=one, wb=1 << 20):
        return lib.gnn_column_moments(x, ld, N, rows, n, D, mu, sd, st, ws, wb, None)

    assert moments(n=0) == 0 and moments(n=0, x=None, mu=None, sd=None, st=None, ws=None, wb=0) == 0
    for bad in (dict(n=-1), dict(D=0), dict(D=256), dict(ld=3), dict(N=-1), dict(n=imax), dict(x=None), dict(mu=None),
                dict(sd=None), dict(st=None)):
        assert moments(**bad) == INVALID, bad
    assert moments(ws=None) == WORKSPACE and moments(wb=8) == WORKSPACE

    def evaluate(x=one, ld=4, N=8, rows=one, n=8, D=4, y=one, mu=one, sd=one, w0=1.0, w1=1.0, C=1.0, th=one, vo=0,
                 F=one, g=one, H=one, st=one, ws=one, wb=1 << 24):
        return lib.gnn_logreg_eval(x, ld, N, rows, n, D, y, mu, sd, w0, w1, C, th, vo, F, g, H, st, ws, wb, None)

    assert evaluate(n=0) == 0 and evaluate(n=0, x=None, y=None, th=None, F=None, g=None, H=None, st=None, ws=None, wb=0) == 0
    for bad in (dict(n=-1), dict(D=0), dict(D=256), dict(ld=3), dict(n=imax), dict(x=None), dict(y=None), dict(th=None),
                dict(F=None), dict(g=None), dict(H=None), dict(st=None), dict(mu=None), dict(sd=None), dict(C=0.0),
                dict(C=float("nan")), dict(C=float("inf")), dict(w0=-1.0), dict(w1=float("nan"))):
        assert evaluate(**bad) == INVALID, bad
    assert evaluate(ws=None) == WORKSPACE and evaluate(wb=64) == WORKSPACE
    assert evaluate(vo=1, g=None, H=None, ws=None) == WORKSPACE  # value-only needs neither g nor H

    def predict(x=one, ld=4, N=8, rows=one, n=8, D=4, mu=one, sd=one, th=one, p64=one, p32=one, st=one):
        return lib.gnn_logreg_predict(x, ld, N, rows, n, D, mu, sd, th, p64, p32, st, None)

    assert predict(n=0) == 0
    for bad in (dict(n=-1), dict(D=256), dict(ld=1), dict(x=None), dict(th=None), dict(st=None), dict(p64=None, p32=None),
                dict(mu=None), dict(sd=None)):
        assert predict(**bad) == INVALID, bad

    def iso_fit(s=one, order=one, flags=one, seg=one, pos=one, n=8, S=1, xs=one, ys=one, K=one, ws=one, wb=1 << 20):
        return lib.gnn_isotonic_fit(s, order, flags, seg, pos, n, S, xs, ys, K, ws, wb, None)

    assert iso_fit(n=0) == 0 and iso_fit(n=0, s=None, order=None, ws=None, wb=0) == 0
    for bad in (dict(n=-1), dict(n=imax), dict(S=2), dict(S=0), dict(s=None), dict(order=None), dict(flags=None),
                dict(seg=None), dict(pos=None), dict(xs=None), dict(ys=None), dict(K=None)):
        assert iso_fit(**bad) == INVALID, bad
    assert iso_fit(ws=None) == WORKSPACE and iso_fit(wb=64) == WORKSPACE

    def iso_apply(xs=one, ys=one, K=one, q=one, n=8, o64=one, o32=one, st=one):
        return lib.gnn_isotonic_apply(xs, ys, K, q, n, o64, o32, st, None)

    assert iso_apply(n=0) == 0 and iso_apply(n=0, xs=None, q=None) == 0
    for bad in (dict(n=-1), dict(n=imax), dict(xs=None), dict(ys=None), dict(K=None), dict(q=None), dict(st=None),
                dict(o64=None, o32=None)):
        assert iso_apply(**bad) == INVALID, bad
    assert b"gnn_isotonic_apply" in lib.gnn_last_error()
