"""GPU: the K17 kernels (csrc/calibrate.hip) against the host mirrors of rank_metrics / calibrate, which
tests/test_device_eval_host.py pins against sklearn and the LBFGS fit.  Thresholds, F1 values, recall
at precision, ROC-AUC (one division of equal integers) and every count are EQUAL; ECE within 4n·2^-53
(its per-bin sums run in another order); the fit's beta within 1e-10 relative and T within one f32
ulp; every output keeps its bits on a second call."""
import math

import numpy as np
import pytest
import torch

from device_eval_cases import FIT_SETS, PATTERNS, TARGETS, ap_tol, fit_set, make
from elliptic_gnn_project_amd import _lib, calibrate, rank_metrics

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 257, 1023, 1024, 1025, 4097, 70001]  # the wave, the tile, the multi-block carry
CURVE_KEYS = ("thr_f1", "f1", "thr_prec", "recall", "roc_auc", "P", "N", "m")


def _same(a: float, b: float) -> bool:
    return a == b or (math.isnan(a) and math.isnan(b))


def _bits(t: torch.Tensor):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64).cpu().tolist()


def check_curve_and_counts(device, y, s, mask=None):
    n = len(y)
    yt, st = torch.from_numpy(y).to(device), torch.from_numpy(s).to(device)
    mt = None if mask is None else torch.from_numpy(mask).to(device)
    hs, hpos, hinc = rank_metrics._host_inputs(s, y, mask)
    o = rank_metrics._host_order(hs, hinc)
    thr = 1.0
    for target in TARGETS:
        want = rank_metrics._host_curve(hs[o], hpos[o], target)
        got = rank_metrics._device_curve(st, yt, mt, target, True)[1].curve.clone()
        again = rank_metrics._device_curve(st, yt, mt, target, True)[1].curve
        assert _bits(got) == _bits(again)
        for key, v in zip(CURVE_KEYS, got.cpu().tolist()):
            assert _same(v, float(want[key])), (key, target, v, want[key])
        thr = want["thr_f1"]
    for t in (thr, 0.5):
        want = rank_metrics._host_calibration(hs, hpos, hinc, t)
        ev = rank_metrics._device_calibration(st, yt, mt, t, rank_metrics.ECE_BINS)
        got = [v.clone() for v in (ev.counts, ev.bin_count, ev.bin_pos, ev.bin_sum, ev.cal)]
        ev = rank_metrics._device_calibration(st, yt, mt, t, rank_metrics.ECE_BINS)
        assert [_bits(v) for v in got] == [_bits(v) for v in (ev.counts, ev.bin_count, ev.bin_pos, ev.bin_sum, ev.cal)]
        b = rank_metrics.ECE_BINS
        assert got[0].tolist() == [want["tp"], want["fp"], want["fn"]]
        assert got[1][:b].tolist() == want["bin_count"].tolist() and got[2][:b].tolist() == want["bin_pos"].tolist()
        tol = 4 * n * 2.0 ** -53
        # a bin's sum of at most n values <= 1: each order's error is at most n·2^-53 of it
        assert np.abs(got[3][:b].cpu().numpy() - want["bin_sum"]).max() <= 2 * n * 2.0 ** -53 * n
        f1, ece = got[4].tolist()
        print(f"ece |device - mirror| = {abs(ece - want['ece']):.3g} (bound {tol:.3g})")
        assert f1 == want["f1"] and abs(ece - want["ece"]) <= tol


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_curve_threshold_and_calibration_match_the_mirror(device, pattern, n):
    y, s = make(pattern, n)
    check_curve_and_counts(device, y, s)


def test_mask_keeping_three_of_4097(device):
    y, s = make("round2", 4097)
    mask = np.zeros(4097, dtype=bool)
    mask[[5, 2048, 4096]] = True
    y[5], y[2048], y[4096] = 1, 0, 1
    check_curve_and_counts(device, y, s, mask)
    y[::3] = -1  # unknown labels: out by default, negatives under a mask
    check_curve_and_counts(device, y, s)
    check_curve_and_counts(device, y, s, np.zeros(4097, dtype=bool))  # nothing included


@pytest.mark.parametrize("pattern", ["round2", "informative", "nopos"])
def test_evaluation_record_matches_the_mirror(device, pattern):
    n = 4097
    y, s = make(pattern, n)
    rng = np.random.default_rng(1)
    mask = rng.random(n) < 0.4
    thr = rank_metrics.select_threshold(s, y, ~mask, 0.25)[0]
    yt, st, mt = (torch.from_numpy(a).to(device) for a in (y, s, mask))
    assert rank_metrics.select_threshold(st, yt, ~mt, 0.25)[0] == thr
    assert rank_metrics.select_threshold(st, yt, ~mt) == rank_metrics.select_threshold(s, y, ~mask)
    want = rank_metrics.evaluation_record(s, y, mask, thr, 50, 0.9)
    got = rank_metrics.evaluation_record(st, yt, mt, thr, 50, 0.9)
    assert tuple(got) == tuple(want) == rank_metrics.RECORD_KEYS
    for k in rank_metrics.RECORD_KEYS:
        if k == "pr_auc_illicit":
            assert abs(got[k] - want[k]) <= ap_tol(n)
        elif k == "ece":
            assert abs(got[k] - want[k]) <= 4 * n * 2.0 ** -53
        else:
            assert _same(float(got[k]), float(want[k])), k
    again = rank_metrics.evaluation_record(st, yt, mt, thr, 50, 0.9)
    assert all(_same(float(got[k]), float(again[k])) for k in rank_metrics.RECORD_KEYS)
    assert rank_metrics.evaluation_record(st, yt, torch.zeros_like(mt), thr, 50, 0.9) == {}
    for name, args in (("roc_auc", ()), ("recall_at_precision", (0.25,)), ("f1_at_threshold", (thr,)),
                       ("expected_calibration_error", ())):
        fn = getattr(rank_metrics, name)
        a, b = fn(st, yt, *args, mask=mt), fn(s, y, *args, mask=mask)
        assert a.is_cuda and a.dtype == torch.float64 and a.dim() == 0
        assert _same(float(a), float(b)) or (name == "expected_calibration_error"
                                             and abs(float(a) - float(b)) <= 4 * n * 2.0 ** -53), name


def check_fit(device, z, y, mask=None, z_dev=None):
    zt = torch.from_numpy(z).to(device) if z_dev is None else z_dev
    yt = torch.from_numpy(y).to(device)
    mt = None if mask is None else torch.from_numpy(mask).to(device)
    want, got, again = {}, {}, {}
    Tw = calibrate.fit_temperature(torch.from_numpy(z), torch.from_numpy(y), None if mask is None else torch.from_numpy(mask),
                                   want)
    T = calibrate.fit_temperature(zt, yt, mt, got)
    T2 = calibrate.fit_temperature(zt, yt, mt, again)
    assert T.is_cuda and T.dtype == torch.float32 and T.shape == (1,)
    assert _bits(T) == _bits(T2) and got == again  # the same bits, diagnostics included
    assert got["status"] == want["status"], (got, want)
    print(f"beta device {got['beta']!r} mirror {want['beta']!r} iterations {got['iterations']} / {want['iterations']}")
    assert abs(got["beta"] - want["beta"]) <= 1e-10 * want["beta"]
    ulp = float(np.spacing(np.float32(Tw.item())))
    assert abs(float(T) - float(Tw)) <= ulp
    if want["status"]:  # EMPTY / FLAT / CLAMP: constants, identical
        assert float(T) == float(Tw) and got["beta"] == want["beta"]
    return got


@pytest.mark.parametrize("n,scale,shift", FIT_SETS)
def test_temperature_fit_matches_the_mirror(device, n, scale, shift):
    """The set's rows scattered over N = 2n + 7 rows under a mask (for the largest set the included rows
    span more than one pass of the workgroup's 1024 threads, and every wave's row range holds some)."""
    zs, ys = fit_set(n, scale, shift)
    N = 2 * n + 7
    rng = np.random.default_rng(n)
    rows = np.sort(rng.choice(N, size=n, replace=False))
    z = rng.standard_normal((N, 2)).astype(np.float32)
    y = rng.integers(-1, 2, N)
    z[rows], y[rows] = zs, ys
    mask = np.zeros(N, dtype=bool)
    mask[rows] = True
    got = check_fit(device, z, y, mask)
    assert got["status"] == 0 and abs(got["g"]) <= 1e-10


@pytest.mark.parametrize("n", [2, 64, 65, 1025])
def test_temperature_fit_small_sizes_and_strided_logits(device, n):
    z, y = fit_set(n, 3.0, 1.0)
    check_fit(device, z, y)
    wide = torch.zeros(n, 5, device=device)
    wide[:, 1:3] = torch.from_numpy(z).to(device)
    view = wide[:, 1:3]  # row stride 5, first element off the allocation's start
    assert not view.is_contiguous()
    a = check_fit(device, z, y, z_dev=view)
    assert a == check_fit(device, z, y)


def test_temperature_fit_rules_and_status(device):
    rng = np.random.default_rng(9)
    n = 3000
    y = (rng.random(n) < 0.4).astype(np.int64)
    sign = (2 * y - 1).astype(np.float32)
    sep = np.stack([-15.0 * sign, 15.0 * sign], axis=1).astype(np.float32)
    assert check_fit(device, sep, y)["status"] == _lib.FIT_STATUS_FLAT
    anti = (-(1.0 + rng.random(n)).astype(np.float32)[:, None] * np.stack([-sign, sign], axis=1)).astype(np.float32)
    got = check_fit(device, anti, y)
    assert got["status"] == _lib.FIT_STATUS_CLAMP_LOW and got["beta"] == 2.0 ** -10
    right = (0.01 * np.stack([-sign, sign], axis=1)).astype(np.float32)
    assert check_fit(device, right, y)["status"] == _lib.FIT_STATUS_CLAMP_HIGH
    assert check_fit(device, sep, y, np.zeros(n, dtype=bool))["status"] == _lib.FIT_STATUS_EMPTY
    T = calibrate.fit_temperature(torch.zeros(0, 2, device=device), torch.zeros(0, dtype=torch.long, device=device))
    assert float(T) == 1.0
    z, yy = fit_set(n, 3.0, 1.0)
    y2 = yy.copy()
    y2[::5] = -1
    check_fit(device, z, y2)  # unknown labels: excluded by default
    y2[3] = 2
    with pytest.raises(ValueError, match="label"):
        calibrate.fit_temperature(torch.from_numpy(z).to(device), torch.from_numpy(y2).to(device),
                                  torch.ones(n, dtype=torch.bool, device=device))
    zn = z.copy()
    zn[n - 1, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        calibrate.fit_temperature(torch.from_numpy(zn).to(device), torch.from_numpy(yy).to(device))
    m = np.ones(n, dtype=bool)
    m[n - 1] = False
    check_fit(device, zn, yy, m)  # the NaN row is outside the mask


def test_status_errors_raise(device):
    s = torch.tensor([0.1, float("nan"), 0.7], device=device)
    y = torch.tensor([1, 0, 1], device=device)
    for fn in (lambda: rank_metrics.roc_auc(s, y), lambda: rank_metrics.select_threshold(s, y),
               lambda: rank_metrics.evaluation_record(s, y, None, 0.5, 2, 0.9)):
        with pytest.raises(ValueError, match="NaN"):
            fn()
    assert float(rank_metrics.roc_auc(s, torch.tensor([1, -1, 0], device=device))) == 0.0  # the NaN is excluded
    with pytest.raises(ValueError):
        rank_metrics.f1_at_threshold(s, y, 0.1)  # not a float32 value
    with pytest.raises(ValueError):
        rank_metrics.expected_calibration_error(s, y, bins=_lib.CALIB_MAX_BINS + 1)
