"""GPU: libgnnmp K14 (csrc/rank_metrics.hip) through rank_metrics — average precision against
metrics.pr_auc_illicit (sklearn) over the sizes and score patterns that cross wave, block and
multi-block carry boundaries; segments; precision@k; the bootstrap replicates against the golden
vectors of the reference and against the host path on both sides of the LDS / global split; bitwise
repeatability; the NaN status; and train_gnn.main with ``device_metrics`` on and off."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from elliptic_gnn_project_amd import _lib, metrics, rank_metrics

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).parent / "golden"
SIZES = [1, 2, 63, 64, 65, 257, 4097, 70001]
PATTERNS = ["distinct", "round1", "equal", "allpos", "onepos_last", "nopos", "negzero"]


def ap_tol(n: int) -> float:
    """A few f64 ulps per tie group, at most n groups."""
    return max(1e-12, 4 * n * 2.0 ** -53)


def make(pattern: str, n: int, seed: int = 0):
    rng = np.random.default_rng(seed + n)
    y = (rng.random(n) < 0.2).astype(np.int64)
    s = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    if pattern == "round1":
        s = np.round(rng.random(n), 1).astype(np.float32)
    elif pattern == "equal":
        s[:] = 0.5
    elif pattern == "allpos":
        y[:] = 1
    elif pattern == "onepos_last":
        y[:] = 0
        y[int(np.argmin(s))] = 1
    elif pattern == "nopos":
        y[:] = 0
    elif pattern == "negzero":
        s = np.round(rng.random(n), 1).astype(np.float32)
        s[::3] = -0.0
        s[1::3] = 0.0
    return y, s


def ref_ap(y, s) -> float:
    return 0.0 if int((y == 1).sum()) == 0 else metrics.pr_auc_illicit((y == 1).astype(int), s)


def dev_ap(device, y, s, mask=None):
    yt, st = torch.from_numpy(y).to(device), torch.from_numpy(s).to(device)
    mt = None if mask is None else torch.from_numpy(mask).to(device)
    a = rank_metrics.average_precision(st, yt, mt)
    b = rank_metrics.average_precision(st, yt, mt)
    assert a.dtype == torch.float64 and a.dim() == 0 and a.is_cuda
    assert a.view(torch.int64).item() == b.view(torch.int64).item()  # two runs: the same bits
    return float(a)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_average_precision_matches_sklearn(device, pattern):
    for n in SIZES:
        y, s = make(pattern, n)
        got, want = dev_ap(device, y, s), ref_ap(y, s)
        print(f"{pattern} n={n}: device {got!r} sklearn {want!r} diff {abs(got - want):.3e} tol {ap_tol(n):.3e}")
        assert abs(got - want) <= ap_tol(n), (pattern, n)
        assert abs(got - float(rank_metrics.average_precision(s, y))) <= ap_tol(n)  # and the host path


def test_mask_keeps_three_of_4097(device):
    y, s = make("round1", 4097)
    mask = np.zeros(4097, dtype=bool)
    mask[[5, 2048, 4096]] = True
    y[[5, 4096]] = 1
    y[2048] = 0
    assert abs(dev_ap(device, y, s, mask) - ref_ap(y[mask], s[mask])) <= ap_tol(3)
    y[:] = -1  # default inclusion: y >= 0
    y[[7, 9, 4000]] = [1, 0, 1]
    assert abs(dev_ap(device, y, s) - ref_ap(y[y >= 0], s[y >= 0])) <= ap_tol(3)


def _segmented(device, y, s, seg, S, inc=None, k=0):
    """The raw plan + AP calls over S segments: (ap, num_pos, count, patk) as numpy, run twice."""
    n = len(y)
    outs = []
    for _ in range(2):
        buf = rank_metrics._buffers(device, n, S, "t")
        rank_metrics._build_plan(buf, torch.from_numpy(s).to(device), None if inc is None else torch.from_numpy(inc).to(device),
                                 torch.from_numpy(seg.astype(np.int32)).to(device))
        rank_metrics._run_ap(buf, rank_metrics._u8(torch.from_numpy(y == 1).to(device)), k)
        rank_metrics.check_status(buf.status)
        outs.append([t[:S].cpu().numpy().copy() for t in (buf.ap, buf.num_pos, buf.count, buf.patk)])
    for a, b in list(zip(*outs))[: 4 if k else 3]:  # (patk is not written without k)
        assert a.tobytes() == b.tobytes()  # two runs: the same bits
    return outs[0]


def test_49_segments_one_empty_one_without_positives(device):
    rng = np.random.default_rng(3)
    n, S = 6001, 49
    y = (rng.random(n) < 0.15).astype(np.int64)
    s = np.round(rng.random(n), 2).astype(np.float32)
    seg = rng.integers(0, S, n)
    seg[seg == 7] = 8          # segment 7 empty
    y[seg == 9] = 0            # segment 9 without a positive
    inc = rng.random(n) < 0.9
    ap, npos, cnt, patk = _segmented(device, y, s, seg, S, inc, k=20)
    for g in range(S):
        m = inc & (seg == g)
        assert cnt[g] == int(m.sum()) and npos[g] == int(y[m].sum())
        want = 0.0 if g in (7, 9) else ref_ap(y[m], s[m])
        assert abs(ap[g] - want) <= ap_tol(n), g
        o = rank_metrics._host_order(s, m)
        assert patk[g] == rank_metrics._host_patk_sorted(y[o], 20), g
    assert cnt[7] == 0 and ap[7] == 0.0 and ap[9] == 0.0 and cnt[9] > 0
    # the public per-group call: the groups present, ascending
    vals, gap, gcnt = rank_metrics.average_precision_by_group(
        torch.from_numpy(s).to(device), torch.from_numpy(y).to(device), torch.from_numpy(seg + 100).to(device),
        torch.from_numpy(inc).to(device))
    present = [g for g in range(S) if g != 7]
    assert vals.tolist() == [g + 100 for g in present]
    assert gap.cpu().numpy().tobytes() == ap[present].tobytes() and gcnt.tolist() == cnt[present].tolist()


def test_boundaries_on_a_block_boundary(device):
    T = _lib.RANK_TILE
    rng = np.random.default_rng(4)
    n = 3 * T + 17
    y = (rng.random(n) < 0.3).astype(np.int64)
    # a segment boundary exactly at position T and another at 3T of the order
    s = np.round(rng.random(n), 2).astype(np.float32)
    seg = np.r_[np.zeros(T), np.ones(2 * T), np.full(17, 2)].astype(np.int64)[rng.permutation(n)]
    ap, npos, cnt, _ = _segmented(device, y, s, seg, 3)
    assert cnt.tolist() == [T, 2 * T, 17]
    for g in range(3):
        assert abs(ap[g] - ref_ap(y[seg == g], s[seg == g])) <= ap_tol(n), g
    # one segment whose tie groups end exactly at positions T - 1 and 2T - 1
    s = np.r_[np.full(T, 0.9), np.full(T, 0.5), rng.random(T + 17) * 0.4].astype(np.float32)
    perm = rng.permutation(n)
    y, s = y[perm], s[perm]
    assert abs(dev_ap(device, y, s) - ref_ap(y, s)) <= ap_tol(n)


@pytest.mark.parametrize("k", [1, 100, 4097, 4097 + 5])
def test_precision_at_k_distinct_scores(device, k):
    y, s = make("distinct", 4097)
    yt, st = torch.from_numpy(y).to(device), torch.from_numpy(s).to(device)
    a, b = rank_metrics.precision_at_k(st, yt, k), rank_metrics.precision_at_k(st, yt, k)
    assert a.is_cuda and a.dtype == torch.float64 and a.view(torch.int64).item() == b.view(torch.int64).item()
    assert float(a) == metrics.precision_at_k(y, s, min(k, 4097))
    assert float(a) == float(rank_metrics.precision_at_k(s, y, k))


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLD / "bootstrap_golden.json").read_text())["cases"]


def _case(c, device):
    y, sa, sb = (np.asarray(c["y"], dtype=np.int64), np.asarray(c["s_a"], dtype=np.float32),
                 np.asarray(c["s_b"], dtype=np.float32))
    return y, torch.from_numpy(sa).to(device), torch.from_numpy(sb).to(device)


def test_bootstrap_golden_on_device(device, golden):
    for c in golden:
        y, sa, sb = _case(c, device)
        n = len(y)
        rng = np.random.default_rng(c["seed"])
        idx = np.stack([rng.choice(n, size=n, replace=True) for _ in range(5)])
        out = [v.cpu().numpy() for v in rank_metrics.replicate_metrics(y, sa, sb, idx, c["topk"])]
        for got, key in zip(out[:2], ("ap_a", "ap_b")):
            assert np.abs(got - np.asarray(c["replicates"][key])).max() <= ap_tol(n), (c["name"], key)
        if c["name"] == "distinct":
            assert out[2].tolist() == c["replicates"]["patk_a"] and out[3].tolist() == c["replicates"]["patk_b"]
        got = rank_metrics.paired_bootstrap(y, sa, sb, c["topk"], c["n_boot"], c["seed"])
        for key in ["delta_pr_auc"] + (["delta_p_at_k"] if c["name"] == "distinct" else []):
            for f in ("delta", "ci_low", "ci_high"):
                assert abs(got[key][f] - c["bootstrap"][key][f]) <= 1e-12, (c["name"], key, f)
        assert got == rank_metrics.paired_bootstrap(y, sa, sb, c["topk"], c["n_boot"], c["seed"])


@pytest.mark.parametrize("n", [300, _lib.RANK_BOOT_LDS_MAX_N - 7, _lib.RANK_BOOT_LDS_MAX_N + 9])
def test_bootstrap_device_matches_host_across_the_lds_split(device, n):
    rng = np.random.default_rng(n)
    y = (rng.random(n) < 0.1).astype(np.int64)
    y[:20] = 1
    sa = np.round(rng.random(n), 3).astype(np.float32)          # ties
    sb = ((rng.permutation(n) + 0.5) / n).astype(np.float32)    # distinct
    idx = rng.integers(0, n, (8, n))
    k = 100
    dev = [rank_metrics.replicate_metrics(y, torch.from_numpy(sa).to(device), torch.from_numpy(sb).to(device), idx, k)
           for _ in range(2)]
    for a, b in zip(*dev):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))  # bit-identical across two runs
    ap_a, ap_b, pk_a, pk_b = (v.cpu().numpy() for v in dev[0])
    h_ap_a, h_pk_a = rank_metrics.host_replicate_metrics(y, sa, idx, k)
    h_ap_b, h_pk_b = rank_metrics.host_replicate_metrics(y, sb, idx, k)
    print(f"n={n}: max |ap - host| {np.abs(ap_a - h_ap_a).max():.3e} {np.abs(ap_b - h_ap_b).max():.3e} tol {ap_tol(n):.3e}")
    assert np.abs(ap_a - h_ap_a).max() <= ap_tol(n) and np.abs(ap_b - h_ap_b).max() <= ap_tol(n)
    assert pk_a.tolist() == h_pk_a.tolist() and pk_b.tolist() == h_pk_b.tolist()
    r = idx[0]  # and one replicate against sklearn on the resampled arrays
    assert abs(ap_a[0] - metrics.pr_auc_illicit(y[r], sa[r])) <= ap_tol(n)


def test_status_word_raises(device):
    y = torch.tensor([1, 0, 1, 0, -1], device=device)
    s = torch.tensor([0.9, float("nan"), 0.3, 0.2, float("nan")], device=device)
    with pytest.raises(ValueError, match="NaN"):
        rank_metrics.average_precision(s, y)
    ap, st = rank_metrics.average_precision(s, y, check=False, return_status=True)  # no host read, status kept
    assert int(st) & _lib.RANK_STATUS_NAN
    keep = torch.tensor([True, False, True, True, False], device=device)
    assert float(rank_metrics.average_precision(s, y, keep)) == pytest.approx(1.0)  # excluded NaNs are ignored
    with pytest.raises(IndexError):
        rank_metrics.replicate_metrics(y[:4].clamp(min=0), s[[0, 2, 3, 0]], s[[3, 2, 0, 0]], np.array([[0, 1, 2, 4]]), 2)


def _cfg(tmp_path, name, **kw):
    base = dict(run_name=name, output_root=str(tmp_path), arch="sage", hidden_dim=32, layers=2, dropout=0.2, lr=0.005,
                weight_decay=1e-4, max_epochs=4, patience=10, grad_clip=1.0, amp=False, symmetrize_edges=True,
                use_time_scalar=True, train_window_k=10, calibrate_temperature=True, topk=50,
                synthetic=dict(num_nodes=6000, num_edges=9000, seed=3))
    base.update(kw)
    return base


def test_main_device_metrics_matches_host_metrics(device, tmp_path):
    from elliptic_gnn_project_amd.train_gnn import main

    m_off = main(_cfg(tmp_path, "off"))
    m_on = main(_cfg(tmp_path, "on", device_metrics=True))
    off, on = tmp_path / "gnn" / "off", tmp_path / "gnn" / "on"
    assert (off / "training_log.csv").read_text() == (on / "training_log.csv").read_text()
    n = 6000
    assert set(m_on) == set(m_off)
    for key in ("best_val_pr_auc", "pr_auc_last1", "pr_auc_last3", "pr_auc_last5"):
        print(key, m_off[key], m_on[key])
        assert abs(m_on[key] - m_off[key]) <= ap_tol(n), key
    np.testing.assert_allclose(m_on["test_pr_auc_by_time"], m_off["test_pr_auc_by_time"], rtol=0, atol=ap_tol(n))
    assert len(m_on["test_pr_auc_by_time"]) >= 5
    for key in set(m_off) - {"best_val_pr_auc", "pr_auc_last1", "pr_auc_last3", "pr_auc_last5", "test_pr_auc_by_time"}:
        assert m_on[key] == m_off[key] or (m_on[key] != m_on[key] and m_off[key] != m_off[key]), key
    a, b = torch.load(off / "best.ckpt", weights_only=True), torch.load(on / "best.ckpt", weights_only=True)
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert json.loads((on / "metrics.json").read_text())["best_val_pr_auc"] == m_on["best_val_pr_auc"]
