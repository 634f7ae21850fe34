"""GPU: the K20 kernels (csrc/baseline.hip) against the host mirrors of logreg.py / calibrate.py and
sklearn's golden vectors, at every geometry the kernels branch on, and train_baselines.main end to end.

Tolerances.  F, g and H are f64 sums of at most 2e4 terms added in another order than numpy's, of terms
whose exp / log1p may differ from libm's by an ulp or two: n eps is about 2e-12 of the sum of the terms'
magnitudes in the worst case and about sqrt(n) eps = 2e-14 typically, so each element is held to 1e-12 of
the sum of its terms' magnitudes (for F that is F itself: every term is positive).  The fitted
probabilities are held to 1e-10 of the mirror's (a row permutation moves them by 3.2e-15 on the CPU) and to
the golden tolerance of sklearn's.  The isotonic fit and its application are integer-exact / single
rounded operations: bit-equal."""
import json

import numpy as np
import pytest
import torch

import baselines_cases as bc
from elliptic_gnn_project_amd import _lib, calibrate, logreg, rank_metrics, train_baselines
from elliptic_gnn_project_amd.dataset_elliptic import save_graph, synthetic_elliptic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
R, L, U = _lib.LOGREG_ROWS, _lib.ISOTONIC_CHUNK, _lib.LOGREG_REDUCE_UNROLL
REL = 1e-12
GOLDEN = bc.load_golden()


# ----------------------------------------------------------------------------- moments and one evaluation
def eval_case(D, n, seed):
    """x wider than D (ld > D) and twice as long as the row list, which skips and shuffles rows."""
    rng = np.random.default_rng(seed)
    N = 2 * n + 3
    wide = (rng.standard_normal((N, D + 3)) * np.exp(rng.uniform(-1, 1, D + 3)) + rng.uniform(-2, 2, D + 3)).astype(np.float32)
    rows = rng.permutation(N)[:n].astype(np.int64)
    y = (rng.random(N) < 0.4).astype(np.int64)
    return wide, rows, y


# D: one tile (1, 7), several (64), the Elliptic widths (165, 167), the last width of one block of
# tiles and the first of two (175, 176), the cap (255: three).  n: one row, around one slab, several
# slabs, and one slab more than the reduce loads per step.
@pytest.mark.parametrize("D", [1, 7, 64, 165, 167, 175, 176, 255])
def test_moments_and_evaluation_match_the_mirror(D):
    for n in (1, R - 1, R, R + 1, 3 * R + 5, U * R, U * R + 1):
        wide, rows, y = eval_case(D, n, 100 * D + n)
        xd = torch.from_numpy(wide).to(DEV)[:, :D]
        assert xd.stride(0) == D + 3
        prob = logreg._DeviceProblem(xd, torch.from_numpy(y), torch.from_numpy(rows))
        assert prob.ld == D + 3 and prob.n == n
        prob.moments()
        mu, sd = prob.mu.cpu().numpy(), prob.sd.cpu().numpy()
        hmu, hsd = logreg.host_moments(wide[:, :D], rows)
        scale = np.abs(wide[rows, :D].astype(np.float64)).max(axis=0)
        dmu, dsd = np.abs(mu - hmu) / np.maximum(scale, 1e-300), np.abs(sd - hsd) / hsd
        assert dmu.max() <= REL and dsd.max() <= REL, (D, n, dmu.max(), dsd.max())
        if n == 1:
            assert (sd == 1.0).all() and np.array_equal(mu, wide[rows[0], :D].astype(np.float64))
        z = logreg.host_z(wide[:, :D], rows, mu, sd)  # the device's own moments: the evaluation alone
        A = np.abs(np.concatenate([z, np.ones((n, 1))], axis=1))
        yb = y[rows] == 1
        w0, w1, C = 0.75, 2.5, 0.5
        rng = np.random.default_rng(D + n)
        r = rng.standard_normal(D + 1)
        big = r * (40.0 / np.abs(z @ r[:D] + r[D]).max())  # |t| up to 40: the saturated sigmoid
        for theta in (np.zeros(D + 1), big):
            F, g, H = prob.evaluate(theta, False, w0, w1, C)
            F2, g2, H2 = prob.evaluate(theta, False, w0, w1, C)
            Fv = prob.evaluate(theta, True, w0, w1, C)[0]
            assert F == F2 == Fv and g.tobytes() == g2.tobytes() and H.tobytes() == H2.tobytes(), "not reproducible"
            assert H.tobytes() == np.ascontiguousarray(H.T).tobytes(), "H is not bitwise symmetric"
            hF, hg, hH = logreg.host_eval(z, yb, w0, w1, C, theta)
            s = np.where(yb, w1, w0)
            _, rr, hh, _ = logreg.host_row_terms(z @ theta[:D] + theta[D], yb, s)
            g_mag = C * (A.T @ np.abs(rr)) + np.abs(np.concatenate([theta[:D], [0.0]]))
            H_mag = C * (A.T @ (A * hh[:, None])) + np.diag(np.r_[np.ones(D), 0.0])
            eF, eg = abs(F - hF) / abs(hF), (np.abs(g - hg) / np.maximum(g_mag, 1e-300)).max()
            eH = (np.abs(H - hH) / np.maximum(H_mag, 1e-300)).max()
            assert eF <= REL and eg <= REL and eH <= REL, (D, n, eF, eg, eH)


def test_a_row_outside_x_is_reported():
    wide, rows, y = eval_case(4, 10, 1)
    bad = rows.copy()
    bad[3] = wide.shape[0]
    prob = logreg._DeviceProblem(torch.from_numpy(wide).to(DEV)[:, :4], torch.from_numpy(y), torch.from_numpy(bad))
    prob.moments()
    assert int(prob.status) == _lib.BASELINE_STATUS_ROW
    with pytest.raises(IndexError):
        prob.evaluate(np.zeros(5), True, 1.0, 1.0, 1.0)
    prob.status.zero_()
    p64, p32 = prob.predict(np.zeros(5))
    assert int(prob.status) == _lib.BASELINE_STATUS_ROW and bool(torch.isnan(p64[3])) and int(torch.isnan(p32).sum()) == 1


# ----------------------------------------------------------------------------- the full fit
@pytest.mark.parametrize("name", list(bc.LR_CASES))
def test_device_fit_matches_the_mirror_and_sklearn(name):
    n, D, cw, _ = bc.LR_CASES[name]
    x, y = bc.lr_inputs(name)
    host = logreg.fit(x, y, None, 1.0, cw, 2000)
    hp = logreg.predict_proba(host, x)
    xd = torch.from_numpy(x).to(DEV)
    m = logreg.fit(xd, torch.from_numpy(y), None, 1.0, cw, 2000)
    p = logreg.predict_proba(m, xd)
    assert p.is_cuda and p.dtype == torch.float64
    p = p.cpu().numpy()
    d_host, d_gold = np.abs(p - hp).max(), np.abs(p - GOLDEN[f"lr/{name}/prob"]).max()
    d_coef = max(np.abs(m.w - GOLDEN[f"lr/{name}/coef"]).max(), abs(m.b - float(GOLDEN[f"lr/{name}/intercept"][0])))
    print(f"{name}: {m.iterations} updates; |p - mirror| {d_host:.3g}, |p - sklearn| {d_gold:.3g}, |theta - sklearn| {d_coef:.3g}")
    assert m.status == 0 and d_host <= 1e-10 and d_gold <= bc.PROB_TOL and d_coef <= bc.COEF_TOL
    p32 = logreg.predict_proba(m, xd, torch.arange(0, n, 2), np.float32).cpu().numpy()
    assert p32.dtype == np.float32 and p32.tobytes() == p[::2].astype(np.float32).tobytes()
    with pytest.raises(ValueError, match="single class"):
        logreg.fit(xd, torch.zeros(n, dtype=torch.int64))


# ----------------------------------------------------------------------------- isotonic
PATTERNS = ("distinct", "ties", "all_equal", "monotone", "reversed", "only_pos", "only_neg", "sawtooth")


def check_isotonic(s, y, mask=None):
    sd, yd = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    md = None if mask is None else torch.from_numpy(mask).to(DEV)
    dev, host = calibrate.fit_isotonic(sd, yd, md), calibrate.fit_isotonic(s, y, mask)
    assert dev.kind == host.kind and dev.xs.size == host.xs.size, (dev.xs.size, host.xs.size)
    assert dev.xs.tobytes() == host.xs.tobytes() and dev.ys.tobytes() == host.ys.tobytes()
    q = bc.cal_queries(s, host.xs)
    for dt in (np.float64, np.float32):
        got = calibrate.apply_calibrator(dev, torch.from_numpy(q).to(DEV), dt)
        assert got.is_cuda and got.cpu().numpy().tobytes() == calibrate.apply_calibrator(host, q, dt).tobytes()
    return dev


# the number of points around the PAVA chunk (distinct scores: one point per element) and the number of
# elements around the rank plan's tile
@pytest.mark.parametrize("n", [L - 1, L, L + 1, 2 * L + 1, 5 * L + 3, 1023, 1024, 1025])
def test_device_isotonic_is_the_mirror_bit_for_bit(n):
    for pattern in PATTERNS:
        s, y = bc.calibrator_inputs(pattern, n)
        cal = check_isotonic(s, y)
        if pattern == "sawtooth":  # every seam pooled: one block of value 1/2 (and the last point alone when n is odd)
            assert cal.xs.size == 2 + n % 2 and cal.ys[0] == cal.ys[1] == 0.5
    s, y = bc.calibrator_inputs("distinct", n, seed=1)
    y[::5] = -1  # unlabelled elements and a mask
    check_isotonic(s, y)
    check_isotonic(s, y, np.arange(n) % 3 != 0)


@pytest.mark.parametrize("pattern,n", bc.CAL_CASES, ids=lambda v: str(v))
def test_device_isotonic_and_platt_on_the_golden_cases(pattern, n):
    name = bc.cal_name(pattern, n)
    s, y = GOLDEN[f"cal/{name}/scores"], GOLDEN[f"cal/{name}/y"].astype(np.int64)
    cal = check_isotonic(s, y)
    assert cal.xs.tobytes() == GOLDEN[f"cal/{name}/xs"].tobytes()
    q = GOLDEN[f"cal/{name}/queries"]
    out = calibrate.apply_calibrator(cal, torch.from_numpy(q).to(DEV), np.float64).cpu().numpy()
    bound = 0 if int(GOLDEN[f"cal/{name}/ulp"][0]) == 0 else 4  # (the generator's measured distance of sklearn)
    assert max(bc.ulp_distance(cal.ys, GOLDEN[f"cal/{name}/ys"]), bc.ulp_distance(out, GOLDEN[f"cal/{name}/iso"])) <= bound
    if f"cal/{name}/platt" in GOLDEN:  # Platt is the D = 1 fit on the raw column
        sd, yd = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
        dev, host = calibrate.fit_platt(sd, yd), calibrate.fit_platt(s, y)
        got = calibrate.apply_calibrator(dev, torch.from_numpy(q).to(DEV), np.float64).cpu().numpy()
        d_host = np.abs(got - calibrate.apply_calibrator(host, q, np.float64)).max()
        d_gold = np.abs(got - GOLDEN[f"cal/{name}/platt"]).max()
        d_theta = np.abs(np.array([dev.w, dev.b]) - GOLDEN[f"cal/{name}/platt_theta"]).max()
        print(f"{name}: platt |p - mirror| {d_host:.3g}, |p - sklearn| {d_gold:.3g}, |theta - sklearn| {d_theta:.3g}")
        assert d_host <= 1e-10 and d_gold <= bc.PROB_TOL and d_theta <= bc.COEF_TOL


def test_device_calibrator_edges():
    s = torch.tensor([0.2, 0.7, 0.4], device=DEV)
    y = torch.tensor([0, 1, 1], device=DEV)
    none = torch.zeros(3, dtype=torch.bool, device=DEV)
    for fit in (calibrate.fit_isotonic, calibrate.fit_platt):
        cal = fit(s, y, none)
        assert cal.kind == "identity" and cal.status == _lib.FIT_STATUS_EMPTY
        assert torch.equal(calibrate.apply_calibrator(cal, s), s)
        with pytest.raises(ValueError, match="NaN"):
            fit(torch.tensor([0.2, float("nan")], device=DEV), torch.tensor([0, 1], device=DEV))
    with pytest.raises(ValueError, match="NaN"):
        calibrate.apply_calibrator(calibrate.fit_isotonic(s, y), torch.tensor([float("nan")], device=DEV))


# ----------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def graph_file(tmp_path_factory):
    """A ~3k-node synthetic graph whose first 8 feature columns carry the label."""
    data = synthetic_elliptic(num_nodes=3000, num_edges=4000, num_feats=24, seed=9, num_illicit=300, num_licit=1800)
    lab = (data.y == 1).float()
    data.x[:, :8] += 0.8 * lab[:, None]
    path = tmp_path_factory.mktemp("graph") / "graph.npz"
    save_graph(str(path), data)
    return path


@pytest.mark.parametrize("calibration", ["none", "isotonic", "platt"])
def test_main_on_the_device_is_the_host_path_of_its_own_scores(tmp_path, graph_file, calibration):
    cfg = dict(run_name="lr", seed=3, model="logistic_regression", calibration=calibration, C=1.0, max_iter=2000,
               class_weight="balanced", device="auto", topk=50, precision_target=0.0, output_root=str(tmp_path),
               graph_file=str(graph_file))
    m = train_baselines.main(cfg)
    run = tmp_path / "baselines" / "lr"
    load = lambda f: np.load(run / f"{f}.npy")  # noqa: E731
    raw_val, raw_test, y_val, y_test = load("scores_raw_val"), load("scores_raw_test"), load("y_val"), load("y_test")
    s_val, s_test = load("scores_val"), load("scores_test")
    assert m["n_test"] == len(y_test) > 100 and m["pr_auc_illicit"] > 0.5, "the features carry the label"
    if calibration == "none":
        assert s_val.tobytes() == raw_val.tobytes() and s_test.tobytes() == raw_test.tobytes()
    elif calibration == "isotonic":
        cal = calibrate.fit_isotonic(raw_val, y_val)
        assert np.load(run / "model.npz")["cal_xs"].tobytes() == cal.xs.tobytes()
        assert calibrate.apply_calibrator(cal, raw_val).tobytes() == s_val.tobytes()
        assert calibrate.apply_calibrator(cal, raw_test).tobytes() == s_test.tobytes()
    else:  # the device's minimiser within 1e-10 of the mirror's, then one rounding to f32
        cal = calibrate.fit_platt(raw_val, y_val)
        d = np.abs(calibrate.apply_calibrator(cal, raw_test).astype(np.float64) - s_test.astype(np.float64)).max()
        assert d <= 1e-10 + 2.0 ** -24
    thr = rank_metrics.select_threshold(s_val, y_val)[0]
    want = rank_metrics.evaluation_record(s_test, y_test, np.ones(len(y_test), dtype=bool), thr, 50, 0.0, device_order=True)
    assert m == want and json.loads((run / "metrics.json").read_text()) == json.loads(json.dumps(want))
    # the host path of the whole run agrees with the device's scores to the fit's tolerance
    host = train_baselines.main(dict(cfg, run_name="lr_host", device="cpu"))
    d = np.abs(np.load(tmp_path / "baselines" / "lr_host" / "scores_raw_test.npy").astype(np.float64) - raw_test).max()
    assert d <= 1e-10 + 2.0 ** -24 and host["n_test"] == m["n_test"]
