"""CPU: the host mirror of the seeded perturbations (elliptic_gnn_project_amd/robustness.py) — the
contract the K15 kernels (csrc/perturb.hip) are tested against on the GPU.

Keys and hash against known answers worked out in plain Python integers, the reference's argument
handling of drop_edges (src/analysis/robustness.py:65-82), uniformity of the edge drop over seeds,
and the first two moments, Kolmogorov-Smirnov distance, pair correlation and range of the noise at
fixed (shape, seed) cases.  Fixed seeds only: a scan over many seeds reaches small p by chance.
"""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from elliptic_gnn_project_amd import robustness as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gnnmp.h"
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
M64, M32 = (1 << 64) - 1, (1 << 32) - 1


# ----------------------------------------------------------------------------- plain-integer restatement
def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _key(seed, stream):
    return _splitmix64((seed & M64) ^ ((stream * 0xD1B54A32D192ED03) & M64))


def _H(c, key):
    h = ((c * 0x9E3779B1 + (key & M32)) & M32) ^ (key >> 32)
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


# (seed, stream, counter) -> (key, H): evaluated once with the integer code above and pinned
KNOWN = [
    ((0, 1, 0), (0x2D0F28C7E7E786B2, 0x0767977F)),
    ((42, 2, 12345), (0xFA797F03F3C87F80, 0x518D6F2F)),
    ((2 ** 63 + 7, 3, 2 ** 32 - 1), (0x30EF63FD8C68D5AA, 0x4E763394)),
]


def test_splitmix64_reference_vector():
    """splitmix64's published first outputs from state 0 (Vigna's splitmix64.c: the state advances by
    the golden gamma, so output i is the mix of i·gamma)."""
    gamma = 0x9E3779B97F4A7C15
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [R.splitmix64((i * gamma) & M64) for i in range(3)] == want
    assert [_splitmix64((i * gamma) & M64) for i in range(3)] == want


def test_key_and_hash_known_answers():
    for (seed, stream, c), (k_pin, h_pin) in KNOWN:
        assert _key(seed, stream) == k_pin and _H(c, k_pin) == h_pin
        assert R.key(seed, stream) == k_pin
        assert int(R.hash_u32(np.array([c], dtype=np.uint64), k_pin)[0]) == h_pin, (seed, stream, c)
    assert int(R.hash_u32(np.array([0]), 0)[0]) == 0  # fmix32 fixes 0
    with pytest.raises(ValueError):
        R.hash_u32(np.array([2 ** 32], dtype=np.uint64), 1)


def test_hash_is_a_bijection_sample():
    """For a fixed key H is a bijection on uint32: no two of 468,710 consecutive counters collide."""
    h = R.hash_u32(np.arange(468710, dtype=np.uint64), R.key(0, R.STREAM_DROP))
    assert np.unique(h).size == h.size


# ----------------------------------------------------------------------------- edge drop
def _ei(E):
    return torch.stack([torch.arange(E, dtype=torch.int64), torch.arange(E, dtype=torch.int64) * 7 % 1013])


def test_drop_edges_arguments():
    ei = _ei(3000)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            R.drop_edges(ei, bad, 0)
    out, n = R.drop_edges(ei, 0.0, 0)
    assert out is ei and n == 0
    out, n = R.drop_edges(ei, 1e-4, 0)  # rounds to 0 edges
    assert out is ei and n == 0
    with pytest.raises(RuntimeError, match="Dropping all edges would leave an empty graph."):
        R.drop_edges(ei, 1.0, 0)
    with pytest.raises(RuntimeError, match="empty graph"):
        R.drop_edges(ei, 0.9999, 0)  # rounds to all 3000


@pytest.mark.parametrize("frac,count", [(1e-4, 0), (0.1, 300), (0.5, 1500), (0.9995, 2998)])
def test_drop_counts_and_order(frac, count):
    ei = _ei(3000)
    out, n = R.drop_edges(ei, frac, 3)
    assert n == count and out.shape == (2, 3000 - count) and out.dtype == torch.int64
    # a subsequence of the input in its order: row 0 is the edge id here
    ids = out[0]
    assert bool((ids[1:] > ids[:-1]).all()) if ids.numel() > 1 else True
    assert torch.equal(out, ei[:, ids])
    # the dropped ones are the `count` smallest (H(e), e)
    k = _key(3, 1)
    order = sorted(range(3000), key=lambda e: (_H(e, k), e))
    assert sorted(set(range(3000)) - set(ids.tolist())) == sorted(order[:count])


def test_drop_seeds_differ_and_repeat():
    ei = _ei(3000)
    a, _ = R.drop_edges(ei, 0.1, 0)
    b, _ = R.drop_edges(ei, 0.1, 1)
    a2, _ = R.drop_edges(ei, 0.1, 0)
    assert torch.equal(a, a2) and not torch.equal(a, b)


def test_drop_uniformity_over_seeds():
    """E = 3000, frac 0.1, seeds 0..1999: each edge is dropped Binomial(2000, 0.1) times.  The z-scores'
    rms lies in [0.95, 1.05] (4 sigma of its sampling error, 1/sqrt(2·3000) = 0.013) and their max
    below 5; adjacent edges fall together with probability p² (independence)."""
    E, S, n = 3000, 2000, 300
    cnt = np.zeros(E)
    both = 0
    for seed in range(S):
        drop = ~R.host_keep_mask(E, n, seed)
        assert int(drop.sum()) == n
        cnt += drop
        both += int((drop[1:] & drop[:-1]).sum())
    z = (cnt - S * 0.1) / math.sqrt(S * 0.1 * 0.9)
    rms = float(np.sqrt(np.mean(z ** 2)))
    print(f"drop uniformity: z rms {rms:.4f}, max |z| {np.abs(z).max():.3f}, adjacent {both / (S * (E - 1)):.5f}")
    assert 0.95 <= rms <= 1.05
    assert float(np.abs(z).max()) < 5.0
    # pairs: mean p² = 0.01 (0.00997 without replacement), sampling error ~ sqrt(0.01 / (S·(E-1))) = 4e-5
    assert abs(both / (S * (E - 1)) - 0.1 * 299 / 2999) < 4 * math.sqrt(0.01 / (S * (E - 1)))


# ----------------------------------------------------------------------------- noise
def _ks_p(z):
    """Kolmogorov-Smirnov p of z against N(0, 1) (asymptotic series with Stephens' small-n correction)."""
    z = np.sort(z.ravel())
    n = z.size
    cdf = 0.5 * (1.0 + np.array([math.erf(v / math.sqrt(2.0)) for v in z])) if n < 50000 else _ncdf(z)
    i = np.arange(1, n + 1)
    d = max(float(np.max(i / n - cdf)), float(np.max(cdf - (i - 1) / n)))
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * d
    return min(1.0, max(0.0, 2.0 * sum((-1) ** (k - 1) * math.exp(-2.0 * k * k * lam * lam) for k in range(1, 101))))


def _ncdf(z):
    return 0.5 * torch.special.erfc(torch.from_numpy(-z / math.sqrt(2.0))).numpy()


NOISE_CASES = [(4096, 166, 0), (1000, 37, 1), (600, 167, 42), (2000, 5, 3)]


@pytest.mark.parametrize("rows,cols,seed", NOISE_CASES)
def test_noise_statistics(rows, cols, seed):
    z = R.host_noise(rows, cols, seed)
    assert z.shape == (rows, cols) and z.dtype == np.float64
    n = z.size
    mean_t = abs(z.mean()) * math.sqrt(n)
    std_t = abs(z.std() - 1.0) * math.sqrt(2 * n)
    p = _ks_p(z)
    ev, od = z[:, 0:cols - cols % 2:2].ravel(), z[:, 1::2].ravel()  # both halves of every whole pair
    corr = float(np.corrcoef(ev, od)[0, 1])
    print(f"noise {rows}x{cols} seed {seed}: mean·sqrt(n) {mean_t:.3f}, |std-1|·sqrt(2n) {std_t:.3f}, KS p {p:.4f}, "
          f"pair corr {corr:+.5f}, max|z| {np.abs(z).max():.3f}")
    assert mean_t < 4.0
    assert std_t < 4.0
    assert p > 1e-3
    assert abs(corr) < 4.0 / math.sqrt(n / 2)
    assert float(np.abs(z).max()) <= 5.78


def test_noise_formula_elementwise():
    """Three elements of a [5, 7] call (an even column, an odd one, the unpaired last column of a row)
    from the integer hash and math.*: the pair layout c = row·ceil(F/2) + col/2, no pair across rows."""
    rows, cols, seed = 5, 7, 9
    z = R.host_noise(rows, cols, seed)
    P = 4
    k2, k3 = _key(seed, 2), _key(seed, 3)
    for row, col in ((0, 0), (3, 5), (4, 6), (2, 1)):
        c = row * P + (col >> 1)
        u1 = ((_H(c, k2) >> 8) + 1) * 2.0 ** -24
        u2 = (_H(c, k3) >> 8) * 2.0 ** -24
        r = math.sqrt(-2.0 * math.log(u1))
        want = r * (math.cos(2 * math.pi * u2) if col % 2 == 0 else math.sin(2 * math.pi * u2))
        assert z[row, col] == pytest.approx(want, abs=1e-14)


def test_add_noise_host_path():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(50, 9, generator=g)
    assert R.add_noise(x, 0.0, 1) is x and R.add_noise(x, -1.0, 1) is x
    a, b, a2 = R.add_noise(x, 0.05, 1), R.add_noise(x, 0.05, 2), R.add_noise(x, 0.05, 1)
    assert a is not x and a.dtype == torch.float32 and torch.equal(a, a2) and not torch.equal(a, b)
    want = (x.double() + 0.05 * torch.from_numpy(R.host_noise(50, 9, 1))).float()
    assert torch.equal(a, want)
    out = torch.empty_like(x)
    v = out._version
    assert R.add_noise(x, 0.05, 1, out=out) is out and torch.equal(out, a) and out._version > v
    with pytest.raises(ValueError):
        R.add_noise(x, 0.05, 1, out=torch.empty(50, 8))


def test_fit_temperature_recovers_a_scale():
    """Logits whose calibrated form is known: labels drawn from softmax(l), then l·3 handed in gives T ≈ 3."""
    g = torch.Generator().manual_seed(0)
    l = torch.randn(20000, 2, generator=g) * 2
    y = torch.multinomial(torch.softmax(l, 1), 1, generator=g).view(-1)
    T = R.fit_temperature(l * 3.0, y)
    assert T.shape == (1,) and not T.requires_grad
    assert float(T) == pytest.approx(3.0, rel=0.05)


# ----------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    from elliptic_gnn_project_amd import _lib

    return _lib.load()


def test_abi_of_the_perturbation_calls(lib):
    from elliptic_gnn_project_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert int(re.search(r"#define GNNMP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gnn_abi_version()
    assert _lib.ABI_VERSION >= 30
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for fn in ("gnn_edge_drop_workspace_size", "gnn_edge_drop", "gnn_feature_noise_f32"):
        proto = re.search(r"gnn_status\s+%s\s*\((.*?)\)\s*;" % fn, text, re.S)
        assert proto, fn
        nargs = len([a for a in proto.group(1).split(",") if a.strip()])
        assert fn in _lib.SIGNATURES and len(_lib.SIGNATURES[fn][1]) == nargs, fn
        assert f" T {fn}\n" in exported, fn


def test_perturbation_calls_validate_on_the_host(lib):
    """Bad arguments are refused before any device work; empty calls launch nothing (no GPU needed)."""
    fake = 1 << 20
    assert lib.gnn_edge_drop(fake, 10, 10, 1, fake, fake, 1 << 30, None) == 1
    assert lib.gnn_edge_drop(fake, 10, -1, 1, fake, fake, 1 << 30, None) == 1
    assert b"drop_count" in lib.gnn_last_error()
    assert lib.gnn_edge_drop(fake, 10, 0, 1, fake, None, 0, None) == 0  # nothing to drop
    assert lib.gnn_edge_drop(None, 0, 0, 1, None, None, 0, None) == 0
    assert lib.gnn_edge_drop(fake, 2 ** 31, 1, 1, fake, fake, 1 << 30, None) == 1
    assert lib.gnn_feature_noise_f32(fake, 5, 0, 5, 1.0, 1, fake, 5, None) == 0
    assert lib.gnn_feature_noise_f32(fake, 5, 7, 0, 1.0, 1, fake, 5, None) == 0
    assert lib.gnn_feature_noise_f32(fake, 4, 7, 5, 1.0, 1, fake, 5, None) == 1
    assert b"leading dimension" in lib.gnn_last_error()
    assert lib.gnn_feature_noise_f32(fake, 5, 7, 5, 1.0, 1, fake, 4, None) == 1
    assert lib.gnn_feature_noise_f32(fake, 6, 2 ** 31, 5, 1.0, 1, fake, 6, None) == 1  # 2^31 · 3 counters
    assert b"counter" in lib.gnn_last_error()
