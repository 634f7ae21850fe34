"""GPU: the flag-driven layer-1 TN as column blocks with a deep load ring, and its empty row blocks.

Each row block of gnn_gemm_tn_active_f32 runs as gnn_gemm_tn_active_split() blocks over contiguous
k-tile ranges of the image, every one walking the row block's flagged chunks in the dense order with
the same scale, with the loads of gnn_gemm_tn_active_ring() chunks in flight; a row block without a
flagged chunk writes one word and the reduce skips its slab.  None of that may change a bit, so every
comparison here is torch.equal against the call without flags on the same operands (the operand
recipe of test_gpu_tn_active.py), and against float64 at test_tn_h2_vs_f64's relL2 < 1e-6.
GNNMP_TN_ACTIVE_SPLIT=0 / GNNMP_TN_EMPTY_SKIP=0 (read at every call) select the first form: one block
per row block, one chunk of loads, every slab written and read.
"""
import pytest
import torch

import test_gpu_tn_active as base
from test_gpu_tn_active import F, NPROJ, NR, _case, _nchunks, _run, rel_l2

pytestmark = pytest.mark.gpu

M_WRAP = 24601  # row blocks of 224 rows = 14 chunks (> 2 x the ring depth), a 9-row tail chunk
NAMES = ("dW", "db", "dW2", "dzsum")


def _form():
    from elliptic_gnn_project_amd import _lib

    lib = _lib.load()
    return lib.gnn_gemm_tn_active_split(), lib.gnn_gemm_tn_active_ring()


def _rows_per_block(M):
    """The dz form's row blocks (gemm_dispatch.hip tn_dz_rows): whole 32-row chunks over at most 128
    blocks up to 32,768 rows, 256 beyond."""
    cap = 128 if M <= 32768 else 256
    chunks = (M + 31) // 32
    return (chunks + cap - 1) // cap * 32


def _masked_dz(M, nz):
    c = _case(M)
    rows = nz.repeat_interleave(16)[:M]
    return torch.where(rows[:, None], c["dz"], torch.zeros_like(c["dz"]))


def _check(M, dz, flags, h=None, dense=None):
    """The flagged call equals the dense call bit for bit (returned), and float64 within 1e-6."""
    c = _case(M)
    out = _run(M, dz, flags, h=h)
    dense = _run(M, dz, None) if dense is None else dense
    for name, a, d in zip(NAMES, out, dense):
        assert torch.equal(a, d), (M, name, int((a != d).sum()))
    if bool((dz != 0).any()):
        Gd = torch.where(c["h"] > 0, (dz.double() @ c["proj"].double()) * 2.0, torch.zeros(M, NR, dtype=torch.float64))
        refs = (Gd.t() @ c["A"], Gd.sum(0), dz.double().t() @ c["h"].double(), dz.double().sum(0))
        for name, t, r in zip(NAMES, out, refs):
            e = rel_l2(t, r)
            print(f"M={M} {name}: relL2 {e:.3e}")
            assert e < 1e-6, (name, e)
    return out


# ------------------------------------------------------------------ ring start-up and drain
def _count_flags(M, counts):
    """Row block b holds counts[b % len(counts)] flagged chunks, spread from a rotating offset."""
    per = _rows_per_block(M) // 16
    n = _nchunks(M)
    flags = torch.zeros(n, dtype=torch.bool)
    for b in range((n + per - 1) // per):
        k = min(counts[b % len(counts)], per)
        for i in range(k):
            q = b * per + (b + i * max(per // max(k, 1), 1)) % per
            if q < n:
                flags[q] = True
    return flags


def test_ring_startup_and_drain():
    """M = 9600, 100 row blocks of 6 chunks holding 0, 1, .. 6 flagged chunks in turn: none, fewer than
    the ring, exactly the ring, one more, and an odd and an even count above it (ring depth <= 4)."""
    D = _form()[1]
    assert 1 <= D <= 4
    M = 9600
    assert _rows_per_block(M) == 96
    flags = _count_flags(M, list(range(7)))
    per_block = flags.view(100, 6).sum(1)
    assert set(per_block.tolist()) == set(range(7)) and D + 1 in per_block.tolist()
    _check(M, _masked_dz(M, flags), flags)


@pytest.mark.parametrize("counts", [(14,), (13, 0, 7, 14), (9, 14, 1)])
def test_ring_wraps(counts):
    """Row blocks of 14 chunks: the ring's sets are refilled several times over (the last row block is
    short and ends in a 9-row chunk whose base is shifted back)."""
    D = _form()[1]
    assert _rows_per_block(M_WRAP) // 16 == 14 > 2 * D
    flags = _count_flags(M_WRAP, list(counts))
    flags[-1] = True
    _check(M_WRAP, _masked_dz(M_WRAP, flags), flags)


# ------------------------------------------------------------------ tail
@pytest.mark.parametrize("M", [25, 4105])
def test_tail_after_an_unflagged_chunk(M):
    """The last chunk flagged, the one before it not: the tail's base is shifted back over rows of the
    unflagged chunk, which must reach neither dW nor dzᵀ·h — also with NaN in every unflagged h row."""
    n = _nchunks(M)
    flags = torch.zeros(n, dtype=torch.bool)
    flags[-1] = True
    if n > 3:
        flags[0] = True
    assert not bool(flags[-2])
    dz = _masked_dz(M, flags)
    out = _check(M, dz, flags)
    c = _case(M)
    h_nan = c["h_d"].clone()
    h_nan[(~flags).repeat_interleave(16)[:M].to(h_nan.device)] = float("nan")
    poisoned = _run(M, dz, flags, h=h_nan)
    for name, a, b in zip(NAMES, out, poisoned):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b), name


# ------------------------------------------------------------------ column split
def _tile_ranges(S, KT=11):
    """The k-tile range of each of a row block's S column blocks: KT dealt as evenly as it goes, the
    longer ranges first."""
    starts = [(k * KT + S - 1) // S for k in range(S + 1)]
    return list(zip(starts[:-1], starts[1:]))


@pytest.mark.parametrize("M", [121, 4105])
def test_column_ranges(M):
    """dW compared range by range of the image's columns — x1 in image columns [0, 166), pad columns
    166 and 167, x2 in [168, 334), so tile 5 holds both segments and the pad, and the last range is the
    short one — and the side sums, which only the first column block of a row block writes."""
    S = _form()[0]
    ranges = _tile_ranges(S)
    assert ranges[0][0] == 0 and ranges[-1][1] == 11 and all(a < b for a, b in ranges)
    assert len(set(b - a for a, b in ranges)) <= 2 and ranges[-1][1] - ranges[-1][0] == 11 // S
    g = torch.Generator().manual_seed(5 + M)
    flags = torch.rand(_nchunks(M), generator=g) < 0.5
    flags[0] = flags[-1] = True
    dz = _masked_dz(M, flags)
    out = _run(M, dz, flags)
    dense = _run(M, dz, None)
    img_col = torch.cat([torch.arange(F), 168 + torch.arange(F)])  # output column -> image column
    covered = torch.zeros(2 * F, dtype=torch.bool)
    for a, b in ranges:
        cols = ((img_col >= 32 * a) & (img_col < 32 * b)).nonzero().flatten()
        covered[cols] = True
        assert torch.equal(out[0][:, cols.to(out[0].device)], dense[0][:, cols.to(out[0].device)]), f"k-tiles [{a}, {b})"
    assert bool(covered.all())
    assert bool((out[0] != 0).any(0).all())  # (random operands: no output column is all zero)
    for name, a, d in zip(NAMES[1:], out[1:], dense[1:]):
        assert torch.equal(a, d), name


# ------------------------------------------------------------------ empty slabs
@pytest.fixture
def pinned_workspace(monkeypatch):
    """fused.gemm_tn allocates its workspace per call; here every call of one size gets the same
    tensor, so a slab a call does not write keeps what the call before left there."""
    from elliptic_gnn_project_amd import fused

    real, held = torch.empty, {}

    def empty(*size, **kw):
        n = size[0] if len(size) == 1 and isinstance(size[0], int) else None
        want = held.get("numel")
        if n is not None and n == want and kw.get("dtype") == torch.float32:
            return held["ws"]
        return real(*size, **kw)

    def pin(M):
        held["numel"] = max(fused._tn_ws_bytes(M, NR, 2 * F, NPROJ) // 4, 1)
        held["ws"] = real(held["numel"], dtype=torch.float32, device="cuda:0")
        return held["ws"]

    monkeypatch.setattr(torch, "empty", empty)
    return pin


@pytest.mark.parametrize("M", [4105, 9600])
def test_stale_slabs_are_not_read(pinned_workspace, M):
    """On one workspace: a call with every flag set fills every slab, then a call with sparse flags
    must equal its dense call — and again after the workspace is filled with NaN."""
    ws = pinned_workspace(M)
    n_out = NR * 2 * F + NR + NPROJ * NR + NPROJ
    assert n_out % 64 != 0  # the slab has pad words: this shape carries the empty word
    c = _case(M)
    g = torch.Generator().manual_seed(9 + M)
    flags = torch.rand(_nchunks(M), generator=g) < 0.1
    flags[_nchunks(M) // 2] = True
    per = _rows_per_block(M) // 16
    nblk = (_nchunks(M) + per - 1) // per
    empty_blocks = sum(1 for b in range(nblk) if not bool(flags[b * per:(b + 1) * per].any()))
    assert 0 < empty_blocks < nblk
    dz = _masked_dz(M, flags)
    ws.zero_()
    dense = _run(M, dz, None)
    ws.fill_(float("nan"))
    _run(M, c["dz"], torch.ones(_nchunks(M), dtype=torch.bool))
    sparse = _run(M, dz, flags)
    for name, a, d in zip(NAMES, sparse, dense):
        assert torch.equal(a, d), name
    ws.fill_(float("nan"))
    poisoned = _run(M, dz, flags)
    for name, a, d in zip(NAMES, poisoned, dense):
        assert torch.equal(a, d), name


@pytest.mark.parametrize("M", [121, 9600])
def test_no_flags_give_positive_zeros(pinned_workspace, M):
    """No flag at all: every slab skipped, every output bit zero — sign bit included — whatever the
    workspace held."""
    ws = pinned_workspace(M)
    ws.fill_(float("nan"))
    z = torch.zeros(_nchunks(M), dtype=torch.bool)
    out = _run(M, torch.zeros(M, NPROJ), z)
    for name, t in zip(NAMES, out):
        assert not bool(t.contiguous().view(torch.int32).any()), name


def test_first_row_block_alone_signed_and_zero_entries():
    """Only row block 0 flagged.  Its dz (random signs) gives dW negative and positive entries, and a
    column of h that is zero on the flagged rows masks G's column 5 there, so dW's row 5 is exactly
    zero: compared as bit patterns, the zeros' sign included."""
    M = 4105
    c = _case(M)
    per = _rows_per_block(M) // 16
    flags = torch.zeros(_nchunks(M), dtype=torch.bool)
    flags[:per] = True
    dz = _masked_dz(M, flags)
    h = c["h_d"].clone()
    h[: per * 16, 5] = 0.0  # G's column 5 is masked on every flagged row: dW row 5 is exactly zero
    out = _run(M, dz, flags, h=h)
    dense = _run(M, dz, None, h=h)
    for name, a, d in zip(NAMES, out, dense):
        assert torch.equal(a.contiguous().view(torch.int32), d.contiguous().view(torch.int32)), name
    dW = out[0]
    assert bool((dW < 0).any()) and bool((dW > 0).any())
    assert not bool(dW[5].contiguous().view(torch.int32).any())


# ------------------------------------------------------------------ the Σg² fold
def _tn_sq(M, dz, flags, device):
    from elliptic_gnn_project_amd import train_ops
    from elliptic_gnn_project_amd.fused import gemm_tn

    c = _case(M)
    buf = torch.full((train_ops._GRAD_SQ_CAP,), -1.0, device=device)
    step = torch.tensor([7.0], device=device)
    dW, db, dW2, dzs = gemm_tn(NR, None, None, dz=dz.to(device), proj=c["proj_d"], h=c["h_d"], hscale=2.0, planes=c["im"],
                               dz_active=flags.to(torch.uint8).to(device), sq=(buf, step), sq_skip=(5, 17))
    torch.cuda.synchronize()
    nb = train_ops._GRAD_SQ_DONE.pop(device)[3]
    return buf, nb, (torch.cat([dW[0], dW[1]], 1), db, dW2, dzs)


def test_sq_partials_equal_the_first_forms(device, monkeypatch):
    """With sq_partial registered: the reduce's norm partials, non-finite counts and step snapshot,
    bit for bit those of the first form (one block per row block, every slab written and read)."""
    M = 9600
    flags = _count_flags(M, [0, 0, 3, 6, 1])
    dz = _masked_dz(M, flags)
    new_buf, nb, new_out = _tn_sq(M, dz, flags, device)
    monkeypatch.setenv("GNNMP_TN_ACTIVE_SPLIT", "0")
    monkeypatch.setenv("GNNMP_TN_EMPTY_SKIP", "0")
    old_buf, nb2, old_out = _tn_sq(M, dz, flags, device)
    assert nb == nb2 and float(new_buf[2 * nb]) == 7.0 and float(new_buf[2 * nb + 1]) == -1.0
    assert float(new_buf[:nb].sum()) > 0.0
    assert torch.equal(new_buf.view(torch.int32), old_buf.view(torch.int32))
    for name, a, b in zip(NAMES, new_out, old_out):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------ determinism, the train step
def test_two_runs_are_equal():
    M = M_WRAP
    flags = _count_flags(M, [5, 0, 14, 2])
    dz = _masked_dz(M, flags)
    for a, b in zip(_run(M, dz, flags), _run(M, dz, flags)):
        assert torch.equal(a, b)


def test_train_step_equals_the_first_forms(device, monkeypatch):
    """One SAGE train step on a seeded synthetic Elliptic-shaped graph just above
    gnn_gemm_tn_active_pays (115,000 nodes, the routing test's graph): logits and every gradient bit
    for bit with the column split and the empty-slab skip on and off."""
    from elliptic_gnn_project_amd import _lib

    data = base._elliptic(115_000, 130_000, seed=1)
    assert _lib.load().gnn_gemm_tn_active_pays(data.x.size(0))
    lo, go, (flags, _) = base._step(device, data, monkeypatch, True)
    assert flags is not None
    monkeypatch.setenv("GNNMP_TN_ACTIVE_SPLIT", "0")
    monkeypatch.setenv("GNNMP_TN_EMPTY_SKIP", "0")
    lf, gf, (flags2, _) = base._step(device, data, monkeypatch, True)
    assert flags2 is not None
    assert torch.equal(lo, lf)
    for k in go:
        assert torch.equal(go[k], gf[k]), k
