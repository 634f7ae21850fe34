"""CPU: the hub ablation's host side (elliptic_gnn_project_amd/hub_ablation.py): the hub count, the numpy
mirror of the degree ranking against train_gnn.hub_edge_mask (torch.topk) where the boundary is untied
and against torch.topk's values where it is tied, small hand cases, and the library's argument
validation for the K18 entry points.  No device calls."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from elliptic_gnn_project_amd import hub_ablation as H

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gnnmp.h"
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"


# ----------------------------------------------------------------------------- the hub count
@pytest.mark.parametrize("N", [1, 7, 8000, 203769])
@pytest.mark.parametrize("frac", [0, 1e-4, 0.005, 0.01, 0.5, 1.0])
def test_num_hubs_of_is_the_reference_count(N, frac):
    assert H.num_hubs_of(N, frac) == int(frac * float(N))


@pytest.mark.parametrize("frac", [-1e-9, 1.0000001, 2, float("nan"), float("inf"), -float("inf")])
def test_bad_fractions_raise(frac):
    with pytest.raises(ValueError):
        H.num_hubs_of(100, frac)
    with pytest.raises(ValueError):
        H.ablate_hubs(torch.zeros((2, 3), dtype=torch.int64), 100, frac)


# ----------------------------------------------------------------------------- the mirror on the synthetic graph
@pytest.fixture(scope="module")
def synthetic():
    from elliptic_gnn_project_amd.dataset_elliptic import prepare_inputs, synthetic_elliptic

    d = prepare_inputs(synthetic_elliptic(num_nodes=8000, num_edges=12000, seed=5), dict(symmetrize_edges=True))
    return d.edge_index, int(d.num_nodes), H.HubRanking(d.edge_index, int(d.num_nodes))


def test_mirror_equals_hub_edge_mask_at_an_untied_boundary(synthetic):
    from elliptic_gnn_project_amd.train_gnn import hub_edge_mask

    ei, N, r = synthetic
    hubs, keep, h = hub_edge_mask(ei, N, 0.005)
    assert h == 40 == H.num_hubs_of(N, 0.005)
    assert not r.boundary_tied(40)  # the precondition of equality with torch.topk
    mine = torch.zeros(N, dtype=torch.bool)
    mine[r.hubs(40).long()] = True
    assert torch.equal(mine, hubs)
    assert torch.equal(r.edge_rank >= 40, keep)
    assert r.kept_counts([40]) == [int(keep.sum())]
    out, n = H.ablate_hubs(ei, N, 0.005)
    assert n == 40 and torch.equal(out, ei[:, keep]) and out.is_contiguous() and out.dtype == torch.int64


def test_tied_boundary_keeps_topk_degree_multiset(synthetic):
    ei, N, r = synthetic
    assert H.num_hubs_of(N, 0.01) == 80 and r.boundary_tied(80)
    deg = torch.bincount(ei[0], minlength=N) + torch.bincount(ei[1], minlength=N)
    assert torch.equal(r.deg.long(), deg)
    want = np.argsort(-deg.numpy(), kind="stable")[:80]
    assert np.array_equal(r.hubs(80).numpy(), want)
    assert sorted(deg[r.hubs(80).long()].tolist(), reverse=True) == torch.topk(deg, 80).values.tolist()
    d = r.describe([80])[0]
    assert d["min_hub_degree"] == int(deg[want[-1]]) == int(deg[r.order[80]]) and d["boundary_tied"] is True


# ----------------------------------------------------------------------------- hand cases
def _ei(pairs):
    return torch.tensor(pairs, dtype=torch.int64).t().contiguous().view(2, -1)


def test_degree_counts_self_loops_twice_and_duplicates_each_time():
    # node 3: a self loop (2) ; node 1: 0-1 twice and 1-2 (3) ; node 4 and 5 isolated
    ei = _ei([(3, 3), (0, 1), (0, 1), (1, 2)])
    deg, order, rank, edge_rank, removed_cum = H.host_ranking(ei, 6)
    assert deg.tolist() == [2, 3, 1, 2, 0, 0]
    assert order.tolist() == [1, 0, 3, 2, 4, 5]  # equal degrees by ascending id
    assert rank.tolist() == [1, 0, 3, 2, 4, 5]
    assert edge_rank.tolist() == [2, 0, 0, 0]
    assert removed_cum.tolist() == [3, 3, 4, 4, 4, 4]
    assert all(a.dtype == np.int32 for a in (deg, order, rank, edge_rank, removed_cum))
    r = H.HubRanking(ei, 6)
    assert r.kept_counts([0, 1, 2, 3, 6]) == [4, 1, 1, 0, 0]
    assert torch.equal(r.ablate(1), _ei([(3, 3)]))
    assert [r.boundary_tied(h) for h in range(7)] == [False, False, True, False, False, True, False]
    assert [d["min_hub_degree"] for d in r.describe([0, 1, 4, 5])] == [None, 3, 1, 0]


def test_no_hub_returns_the_same_tensor_and_all_hubs_raise():
    ei = _ei([(0, 1), (1, 2), (2, 0), (3, 3)])
    r = H.HubRanking(ei, 5)
    assert r.ablate(0) is ei
    out, n = H.ablate_hubs(ei, 5, 0.1)  # int(0.5) = 0
    assert out is ei and n == 0
    with pytest.raises(RuntimeError, match="empty graph"):
        r.ablate(5)
    with pytest.raises(RuntimeError, match="empty graph"):
        H.ablate_hubs(ei, 5, 1.0)
    with pytest.raises(ValueError):
        r.ablate(6)
    with pytest.raises(ValueError):
        r.kept_counts([-1])
    with pytest.raises(ValueError):
        r.ablate(1, kept=3)  # not this ablation's count
    with pytest.raises(IndexError):
        H.HubRanking(ei, 3)
    with pytest.raises(IndexError):
        H.HubRanking(_ei([(0, -1)]), 3)
    with pytest.raises(ValueError):
        H.HubRanking(torch.zeros((3, 4), dtype=torch.int64), 5)
    with pytest.raises(TypeError):
        H.HubRanking(torch.zeros((2, 4)), 5)


def test_ablations_are_nested_and_every_edge_is_removed_at_the_end():
    g = torch.Generator().manual_seed(7)
    N, E = 50, 400
    ei = torch.randint(0, 12, (2, E), generator=g)  # heavy ties, nodes 12..49 isolated
    r = H.HubRanking(ei, N)
    assert int(r.removed_cum[N - 1]) == E
    assert torch.equal(r.rank[r.order.long()], torch.arange(N, dtype=torch.int32))
    counts = r.kept_counts(range(N + 1))
    assert counts[0] == E and counts == sorted(counts, reverse=True)
    prev = torch.ones(E, dtype=torch.bool)
    for h in range(1, N + 1):
        keep = r.edge_rank >= h
        hubs = torch.zeros(N, dtype=torch.bool)
        hubs[r.hubs(h).long()] = True
        assert torch.equal(keep, ~(hubs[ei[0]] | hubs[ei[1]]))  # the reference's mask for this hub set
        assert bool((keep <= prev).all()) and int(keep.sum()) == counts[h]
        if counts[h]:
            assert torch.equal(r.ablate(h, counts[h]), ei[:, keep])
        prev = keep
    e32 = H.HubRanking(ei.to(torch.int32), N)  # an int32 edge_index ranks the same and comes back int64
    assert torch.equal(e32.edge_rank, r.edge_rank) and torch.equal(e32.ablate(3), r.ablate(3))
    empty = H.HubRanking(torch.zeros((2, 0), dtype=torch.int64), 4)
    assert empty.order.tolist() == [0, 1, 2, 3] and empty.kept_counts([0, 2]) == [0, 0]


def test_feature_width_mismatch_names_both_widths():
    from elliptic_gnn_project_amd.robustness import check_feature_width

    model = torch.nn.Sequential(torch.nn.Linear(7, 4), torch.nn.Linear(4, 2))
    check_feature_width(model, model.state_dict(), 7)
    other = torch.nn.Sequential(torch.nn.Linear(9, 4), torch.nn.Linear(4, 2))
    with pytest.raises(ValueError, match=r"expects 9 input features.*has 7"):
        check_feature_width(model, other.state_dict(), 7)


# ----------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    from elliptic_gnn_project_amd import _lib

    return _lib.load()


def test_k18_is_additive_to_abi_32(lib):
    from elliptic_gnn_project_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert int(re.search(r"#define GNNMP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gnn_abi_version() == 32
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for fn in ("gnn_hub_rank_workspace_size", "gnn_hub_rank", "gnn_hub_ablate_workspace_size", "gnn_hub_ablate"):
        proto = re.search(r"gnn_status\s+%s\s*\((.*?)\)\s*;" % fn, text, re.S)
        assert proto, fn
        nargs = len([a for a in proto.group(1).split(",") if a.strip()])
        assert fn in _lib.SIGNATURES and len(_lib.SIGNATURES[fn][1]) == nargs, fn
        assert f" T {fn}\n" in exported, fn


def test_k18_entry_points_validate_on_the_host(lib):
    """Bad arguments are refused before any device work; empty calls launch nothing (no GPU needed)."""
    from elliptic_gnn_project_amd import _lib

    b = _lib.c_size(0)
    one, big, imax = ctypes.c_void_p(1 << 20), 1 << 30, 2 ** 31 - 1  # never dereferenced
    assert lib.gnn_hub_rank_workspace_size(-1, 4, ctypes.byref(b)) == 1
    assert lib.gnn_hub_rank_workspace_size(4, -1, ctypes.byref(b)) == 1
    assert lib.gnn_hub_rank_workspace_size(4, 4, None) == 1
    assert lib.gnn_hub_rank_workspace_size(imax, 4, ctypes.byref(b)) == 1
    assert lib.gnn_hub_rank_workspace_size(4, imax, ctypes.byref(b)) == 1
    assert lib.gnn_hub_ablate_workspace_size(-1, ctypes.byref(b)) == 1
    assert lib.gnn_hub_ablate_workspace_size(4, None) == 1
    assert lib.gnn_hub_ablate_workspace_size(imax, ctypes.byref(b)) == 1

    def rank(E=10, N=5, **kw):
        g = lambda k: kw.get(k, one)  # noqa: E731
        return lib.gnn_hub_rank(g("ei"), E, N, g("deg"), g("order"), g("rank"), g("edge_rank"), g("removed_cum"),
                                g("ws"), kw.get("ws_bytes", big), None)

    assert rank(E=-1) == 1 and rank(N=-1) == 1 and rank(E=imax) == 1 and rank(N=imax) == 1 and rank(N=0) == 1
    for name in ("ei", "deg", "order", "rank", "edge_rank", "removed_cum"):
        assert rank(**{name: None}) == 1, name
    assert b"gnn_hub_rank" in lib.gnn_last_error() and b"null buffer" in lib.gnn_last_error()
    assert rank(ws=None) == 4 and rank(ws_bytes=0) == 4
    assert rank(N=1000, ws_bytes=3 * 4 * 1000 - 1) == 4  # below its three arrays of N
    assert b"workspace too small" in lib.gnn_last_error()
    assert rank(E=0) == 0 and rank(E=0, N=0, ei=None, deg=None, ws=None, ws_bytes=0) == 0  # no edge: a no-op

    def ablate(E=10, h=2, kept=5, **kw):
        g = lambda k: kw.get(k, one)  # noqa: E731
        return lib.gnn_hub_ablate(g("ei"), E, g("edge_rank"), h, kept, g("out"), g("ws"), kw.get("ws_bytes", big), None)

    assert ablate(E=-1) == 1 and ablate(E=imax) == 1
    assert ablate(h=-1) == 1 and ablate(h=imax) == 1
    assert b"num_hubs" in lib.gnn_last_error()
    assert ablate(kept=-1) == 1 and ablate(kept=11) == 1
    for name in ("ei", "edge_rank", "out"):
        assert ablate(**{name: None}) == 1, name
    assert ablate(ws=None) == 4 and ablate(ws_bytes=0) == 4 and ablate(E=1000, kept=10, ws_bytes=3999) == 4
    assert ablate(E=0, kept=0, ei=None, edge_rank=None, out=None, ws=None, ws_bytes=0) == 0
    assert ablate(h=0, kept=10, out=None, ws=None, ws_bytes=0) == 0  # no hub: the caller keeps edge_index
