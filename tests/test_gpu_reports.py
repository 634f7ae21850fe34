"""GPU: the run reports' kernels (libgnnmp K19, csrc/report.hip) against their host mirrors — hits at a
list of k, threshold counts per group, the join by id and the pair ensemble — and the four tools on the
device against their host-path runs, byte for byte.  No model is trained."""
import ctypes
import math

import numpy as np
import pytest
import torch

from reports_cases import (GOLDEN, by_time_run, check_ensemble_metrics, check_logit_bounds, ensemble_runs, f32,
                           write_run)
from elliptic_gnn_project_amd import _lib, calibration_plots, eval_by_time, evaluate_ensemble, rank_metrics, workload_curves

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")
TILE_SIZES = [1, 2, 1023, 1024, 1025, 3 * 1024 + 7]  # GNN_RANK_TILE boundaries


def make(pattern: str, n: int):
    rng = np.random.default_rng(n + (7 if pattern == "ties" else 0))
    y = (rng.random(n) < 0.2).astype(np.int64)
    if pattern == "distinct":
        s = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    else:
        s = np.round(np.clip(0.3 * y + 0.7 * rng.random(n), 0, 1), 2).astype(np.float32)
    return y, s, rng


def same_f64(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()  # NaN compared as NaN: the same bits


# ----------------------------------------------------------------------------- (a) hits at a list of k
@pytest.mark.parametrize("n", TILE_SIZES)
@pytest.mark.parametrize("pattern", ["distinct", "ties"])
def test_hits_at_equal_the_host(device, pattern, n):
    y, s, rng = make(pattern, n)
    third = rng.random(n) >= 1 / 3
    for mask in (third, np.zeros(n, dtype=bool), None):
        m = n if mask is None else int(mask.sum())
        ks = sorted({k for k in (1, m - 1, m, m + 1, 10 ** 9, 10, 1024, 1025) if k >= 1})
        dm = None if mask is None else torch.from_numpy(mask).to(device)
        got = rank_metrics.precision_curve(torch.from_numpy(s).to(device), torch.from_numpy(y).to(device), ks, dm)
        want = rank_metrics.precision_curve(s, y, ks, mask)
        assert all(t.is_cuda for t in got) and got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.float64
        assert got[0].tolist() == want[0].tolist() == [min(k, m) for k in ks] and got[1].tolist() == want[1].tolist()
        assert same_f64(got[2], want[2])
        if m == 0:
            assert all(math.isnan(v) for v in got[2].tolist())


def test_hits_at_flags_a_k_below_one(device):
    y, s, _ = make("distinct", 50)
    ds, dy = torch.from_numpy(s).to(device), torch.from_numpy(y).to(device)
    k_eff, hits, prec = rank_metrics.precision_curve(ds, dy, [3, 0, -5], check=False)
    assert k_eff.tolist() == [3, 0, 0] and hits.tolist()[1:] == [0, 0] and [math.isnan(v) for v in prec.tolist()] == [False, True, True]
    with pytest.raises(ValueError, match="k < 1"):
        rank_metrics.precision_curve(ds, dy, [3, 0])
    assert rank_metrics.precision_curve(ds, dy, [])[2].numel() == 0


# ----------------------------------------------------------------------------- (b) threshold counts per group
@pytest.mark.parametrize("n", TILE_SIZES + [4095, 4096, 4097, 3 * 4096 + 5])  # and the counting blocks' tile
@pytest.mark.parametrize("S", [1, 2, 49])
def test_segment_counts_equal_the_host(device, n, S):
    y, s, rng = make("ties", n)
    y[rng.random(n) < 0.1] = -1
    seg = rng.integers(0, max(S - 1, 1), n).astype(np.int32)  # S > 1: the last group stays empty
    j = n // 2
    seg[j] = S + 3 if n % 2 else -1  # one included element outside [0, S), on either side
    y[j] = 1
    thr = float(np.sort(s)[n // 2])
    for mask in (None, rng.random(n) >= 1 / 3):
        if mask is not None:
            mask[j] = True
        dm = None if mask is None else torch.from_numpy(mask).to(device)
        got, st = rank_metrics.segment_threshold_counts(torch.from_numpy(s).to(device), torch.from_numpy(y).to(device),
                                                        torch.from_numpy(seg).to(device), S, thr, dm, check=False)
        want, wst = rank_metrics.segment_threshold_counts(s, y, seg, S, thr, mask, check=False)
        assert got.is_cuda and got.dtype == torch.int64 and got.cpu().tolist() == want.tolist()
        assert int(st) == int(wst) == _lib.RANK_STATUS_SEGMENT
        inc = (y >= 0) if mask is None else mask
        assert int(got[:, 3].sum()) == int(inc.sum()) - 1 and (S == 1 or int(got[S - 1].sum()) == 0)
    with pytest.raises(IndexError):
        rank_metrics.segment_threshold_counts(torch.from_numpy(s).to(device), torch.from_numpy(y).to(device),
                                              torch.from_numpy(seg).to(device), S, thr)


def test_counts_by_group_share_the_ap_mapping(device):
    y, s, rng = make("ties", 3000)
    g = rng.choice([3, 8, 11, 40], 3000)
    thr = float(np.sort(s)[1000])
    ds, dy, dg = (torch.from_numpy(a).to(device) for a in (s, y, g))
    vals, counts = rank_metrics.threshold_counts_by_group(ds, dy, dg, thr)
    hv, hc = rank_metrics.threshold_counts_by_group(s, y, g, thr)
    assert vals.tolist() == hv.tolist() == rank_metrics.average_precision_by_group(ds, dy, dg)[0].tolist()
    assert counts.cpu().tolist() == hc.tolist()


# ----------------------------------------------------------------------------- (c) join by id
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_join_by_id(device, n):
    rng = np.random.default_rng(n)
    base = rng.choice(2 ** 40, n, replace=False).astype(np.int64)
    for name, other_of in (("identity", lambda b: b.copy()), ("reverse", lambda b: b[::-1].copy()),
                           ("random", lambda b: b[rng.permutation(n)])):
        other = other_of(base)
        perm = rank_metrics.join_by_id(torch.from_numpy(base).to(device), torch.from_numpy(other).to(device), "TEST")
        assert perm.is_cuda and perm.dtype == torch.int32 and np.array_equal(other[perm.cpu().numpy()], base), name
        assert perm.cpu().tolist() == rank_metrics.join_by_id(base, other).tolist(), name


@pytest.mark.parametrize("n", [3, 257, 4097])
def test_join_status_bits(device, n):
    rng = np.random.default_rng(n + 1)
    base = rng.choice(2 ** 40, n, replace=False).astype(np.int64)
    other = base[::-1].copy()

    def status(b, o):
        lib = _lib.load()
        db, do = torch.from_numpy(b).to(device), torch.from_numpy(o).to(device)
        perm = torch.empty(n, dtype=torch.int32, device=device)
        st = torch.zeros(1, dtype=torch.int32, device=device)
        sz = _lib.c_size(0)
        _lib.check(lib.gnn_id_join_workspace_size(n, ctypes.byref(sz)))
        ws = torch.empty(sz.value, dtype=torch.uint8, device=device)
        _lib.call("gnn_id_join", _lib.ptr(db), _lib.ptr(do), n, _lib.ptr(perm), _lib.ptr(st), _lib.ptr(ws), ws.numel(),
                  _lib.stream_handle(device))
        p = perm.cpu().numpy()
        assert ((p >= 0) & (p < n)).all()  # unspecified, but inside [0, n)
        return int(st)

    assert status(base, other) == 0
    dup_b, dup_o = base.copy(), other.copy()  # a two-element edit each: the same id twice in both arrays
    dup_b[0] = dup_b[1]
    dup_o[dup_o == base[0]] = base[1]
    assert status(dup_b, dup_o) == _lib.JOIN_STATUS_DUPLICATE
    neg_b, neg_o = base.copy(), other.copy()
    neg_b[0], neg_o[neg_o == base[0]] = -5, -5
    assert status(neg_b, neg_o) == _lib.JOIN_STATUS_NEGATIVE
    mis_b, mis_o = base.copy(), other.copy()
    mis_b[0], mis_o[0] = 2 ** 41 + 1, 2 ** 41 + 2
    assert status(mis_b, mis_o) & _lib.JOIN_STATUS_MISMATCH and not status(mis_b, mis_o) & _lib.JOIN_STATUS_NEGATIVE
    for b, o, word in ((dup_b, dup_o, "duplicate"), (neg_b, neg_o, "negative"), (mis_b, mis_o, "differ")):
        with pytest.raises(RuntimeError, match=f"VAL.*{word}"):
            rank_metrics.join_by_id(torch.from_numpy(b).to(device), torch.from_numpy(o).to(device), "VAL")


# ----------------------------------------------------------------------------- (d) pair ensemble
def test_ensemble_equals_the_host_mirror_bit_for_bit(device):
    rng = np.random.default_rng(0)
    for key, mode in (("ensemble_values", "logit"), ("ensemble_prob", "prob")):
        a, b = f32(GOLDEN[key]["a"]), f32(GOLDEN[key]["b"])
        perm = rng.permutation(a.size).astype(np.int32)
        da, db = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
        for p in (None, perm):
            got = rank_metrics.ensemble_pair(da, db, mode, None if p is None else torch.from_numpy(p).to(device))
            want = rank_metrics.ensemble_pair(a, b, mode, p)
            assert got.is_cuda and got.dtype == torch.float32 and got.cpu().numpy().tobytes() == want.numpy().tobytes(), (key, p is None)
        got = rank_metrics.ensemble_pair(da, db, mode).cpu().numpy()
        if mode == "logit":
            check_logit_bounds(got, a, b, f32(GOLDEN[key]["ref"]))
        else:
            assert got.tobytes() == f32(GOLDEN[key]["ref"]).tobytes()
    for split in ("val", "test"):
        s = GOLDEN["ensemble_logit"][split]
        a, b = f32(s["a"]), f32(s["b"])
        perm = rank_metrics.join_by_id(torch.tensor(s["ids_b"], device=device), torch.tensor(s["ids_a"], device=device), split)
        got = rank_metrics.ensemble_pair(torch.from_numpy(a).to(device), torch.from_numpy(b).to(device), "logit", perm).cpu().numpy()
        assert got.tobytes() == rank_metrics.ensemble_pair(a, b, "logit", perm.cpu()).numpy().tobytes()
        check_logit_bounds(got, a[perm.cpu().numpy()], b, f32(s["ref"]))


def test_ensemble_status_bits(device):
    a = torch.tensor([0.2, float("nan"), 0.4], device=device)
    b = torch.tensor([0.3, 0.5, 0.6], device=device)
    with pytest.raises(ValueError, match="NaN"):
        rank_metrics.ensemble_pair(a, b, "logit")
    out = rank_metrics.ensemble_pair(a, b, "prob", check=False).cpu()
    assert math.isnan(float(out[1])) and float(out[0]) == float(np.float32(0.5) * (np.float32(0.2) + np.float32(0.3)))
    with pytest.raises(IndexError):
        rank_metrics.ensemble_pair(b, b, "prob", torch.tensor([0, 3, 1], device=device))


# ----------------------------------------------------------------------------- the tables and the tools
def test_tables_equal_the_host_bit_for_bit(device):
    for n in (1, 1025, 3 * 4096 + 5):
        y, s, rng = make("ties", n)
        ts = rng.integers(30, 37, n)
        mask = rng.random(n) >= 0.25
        thr = float(np.sort(s)[n // 2])
        ds, dy, dt, dm = (torch.from_numpy(a).to(device) for a in (s, y, ts, mask))
        assert rank_metrics.by_time_table(ds, dy, dt, thr, dm) == rank_metrics.by_time_table(s, y, ts, thr, mask), n
        got, want = rank_metrics.reliability_table(ds, dy, dm), rank_metrics.reliability_table(s, y, mask)
        assert got.keys() == want.keys()
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (n, k)


def test_the_tools_write_the_same_bytes_on_both_paths(device, tmp_path, capsys):
    for name in ("ties", "distinct"):
        dev_run, host_run = by_time_run(tmp_path / name / "dev", name), by_time_run(tmp_path / name / "host", name)
        for run, where in ((dev_run, device), (host_run, CPU)):
            eval_by_time.main(["--run_dir", str(run)], where)
            workload_curves.main(["--run_dir", str(run)], where)
            calibration_plots.main(["--run_dir", str(run)], where)
        for f in ("by_time.csv", "workload_curve.csv", "calibration_curve.csv"):
            assert (dev_run / f).read_bytes() == (host_run / f).read_bytes(), (name, f)
    run_a, run_b = ensemble_runs()
    a = write_run(tmp_path / "a", run_a, {"best_val_pr_auc": 0.61})
    b = write_run(tmp_path / "b", run_b, {"best_val_pr_auc": 0.58})
    for mode in ("logit", "prob"):
        outs = []
        for where, out in ((device, tmp_path / f"dev_{mode}"), (CPU, tmp_path / f"host_{mode}")):
            m = evaluate_ensemble.main(["--run_a", str(a), "--run_b", str(b), "--out_dir", str(out), "--mode", mode], where)
            outs.append(out)
            if mode == "logit":
                check_ensemble_metrics(m)
        files = sorted(p.name for p in outs[0].iterdir())
        assert files == sorted(p.name for p in outs[1].iterdir()) and "metrics.json" in files and len(files) == 10
        for f in files:
            assert (outs[0] / f).read_bytes() == (outs[1] / f).read_bytes(), (mode, f)
    capsys.readouterr()
