"""CPU: the GAT entry points (csrc/gat.hip) refuse what they cannot take before any launch, each
call with the message of the first rule it breaks, and gnn_gat_bwd_workspace_size answers what the
recorded table says.  No device calls; the pointers below are never read.

Every row is (entry, arguments, status, the whole text after "entry: ").  1 = INVALID_ARG,
4 = WORKSPACE, 5 = UNSUPPORTED, 0 = the forward entries' empty-graph return."""
import ctypes
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
GOLDEN = ROOT / "tests" / "golden" / "gat_bwd_workspace_golden.json"
FAKE = 1 << 20
WS = 1 << 30

HEADS = b"heads must be a power of two <= 64"
SIZES = b"bad sizes"
ACT = b"unknown act"
DROP = b"dropout_p not in [0, 1)"
INDEX = b"dropout element index (rows x width) must be < 2^32"
PROJ = b"proj: concat, nproj <= 4, proj (16-byte aligned) and z"
Y_DPRE = b"bad y / dpre"
Y_DZ = b"bad y / dpre / dz / proj"
EDGE_W = b"edge_w and d_edge_w are required"
WORKSPACE = b"workspace too small"
NARROW = b"the narrow output form: heads 1, 1 <= C <= 2, no concat / act / dropout / edge_w"
NO_GP = b"null graph or params"
OUT_NULL = b"null operand / N < 1"


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():  # a fresh checkout: build it (hipcc cross-compiles gfx950 without a GPU)
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    from elliptic_gnn_project_amd import _lib

    return _lib.load()


_KEEP = []  # structs passed by pointer stay alive until the call


def _graph(L, num_nodes=1000, num_slots=4000, **kw):
    g = L.GnnGraph(num_nodes, num_slots, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
    for k, v in kw.items():
        setattr(g, k, v)
    _KEEP.append(g)
    return g


def _params(L, **kw):
    """A valid hidden-layer gnn_gat_fwd_params: H = 4, C = 8, concat, ELU, p = 0.5."""
    p = L.GnnGatFwdParams(heads=4, chans=8, concat=1, slope=0.2, xh=FAKE, ld_xh=32, att_src=FAKE, att_dst=FAKE,
                          act=L.ACT_ELU, dropout_p=0.5, seed=1, a_src=FAKE, a_dst=FAKE, alpha=FAKE, out=FAKE, ldo=32)
    for k, v in kw.items():
        setattr(p, k, v)
    _KEEP.append(p)
    return p


def _narrow(L, **kw):
    """A valid narrow output-layer gnn_gat_fwd_params: H = 1, C = 2, head mean, no act / dropout."""
    return _params(L, **dict(dict(heads=1, chans=2, concat=0, ld_xh=2, act=L.ACT_NONE, dropout_p=0.0, ldo=2), **kw))


def _spec(L, **kw):
    s = L.GnnCeSpec(y=FAKE, mask=FAKE, class_w=FAKE, inv_denom=1.0)
    for k, v in kw.items():
        setattr(s, k, v)
    _KEEP.append(s)
    return s


_BWD_HEAD = dict(g=None, H=4, C=8, concat=1, slope=0.2, xh=FAKE, ld_xh=32, a_src=FAKE, a_dst=FAKE, att_src=FAKE,
                 att_dst=FAKE, alpha=FAKE)
_ACT_HEAD = {k: v for k, v in _BWD_HEAD.items() if k != "concat"}
_POST = dict(act=1, dropout_p=0.5, seed=1, seed_ptr=None, y=FAKE, ld_y=32)
_WS = dict(workspace=FAKE, workspace_bytes=WS, stream=None)

# entry -> its arguments in C order, a valid call's values (g: filled per row, gp: a graph and params)
ARGS = {
    "gnn_gat_scores_f32": dict(N=1000, H=4, C=8, xh=FAKE, ld_xh=32, att_src=FAKE, att_dst=FAKE, a_src=FAKE,
                               a_dst=FAKE, stream=None),
    "gnn_gat_fwd_f32": dict(g=None, H=4, C=8, concat=1, slope=0.2, xh=FAKE, ld_xh=32, a_src=FAKE, a_dst=FAKE,
                            bias=None, alpha=FAKE, out=FAKE, ldo=32, stream=None),
    "gnn_gat_fwd_fused_f32": dict(g=None, p=None, stream=None),
    "gnn_gat_act_bwd_f32": dict(N=1000, F=32, act=1, dropout_p=0.5, seed=1, seed_ptr=None, y=FAKE, ldy=32, dy=FAKE,
                                lddy=32, dpre=FAKE, ld_dpre=32, stream=None),
    "gnn_gat_bwd_workspace_size": dict(N=1000, S=4000, H=4, C=8, bytes=None),
    "gnn_gat_bwd_f32": dict(_BWD_HEAD, dout=FAKE, ld_dout=32, dxh=FAKE, ld_dxh=32, d_att_src=FAKE, d_att_dst=FAKE,
                            **_WS),
    "gnn_gat_bwd_act_f32": dict(_ACT_HEAD, **_POST, dy=FAKE, ld_dy=32, dpre=FAKE, ld_dpre=32, dxh=FAKE, ld_dxh=32,
                                d_att_src=FAKE, d_att_dst=FAKE, **_WS),
    "gnn_gat_bwd_act_proj_f32": dict(_ACT_HEAD, **_POST, dz=FAKE, ld_dz=2, proj=FAKE, nproj=2, dpre=FAKE, ld_dpre=32,
                                     dxh=FAKE, ld_dxh=32, d_att_src=FAKE, d_att_dst=FAKE, dxh_rowmax=None, **_WS),
    "gnn_gat_bwd_ew_f32": dict(_BWD_HEAD, dout=FAKE, ld_dout=32, dxh=FAKE, ld_dxh=32, d_att_src=FAKE, d_att_dst=FAKE,
                               edge_w=FAKE, d_edge_w=FAKE, **_WS),
    "gnn_gat_out_ce_f32": dict(g=None, p=None, y=FAKE, mask=FAKE, class_w=FAKE, inv_denom=1.0, dlogits=FAKE, ld_d=2,
                               colsum=None, loss=FAKE, **_WS),
    "gnn_gat_out_ce_spec_f32": dict(g=None, p=None, spec=None, dlogits=FAKE, ld_d=2, colsum=None, loss=FAKE, **_WS),
}

NO = "no"  # a row's g / p / spec = NO: a null pointer


def _call(lib, L, entry, kw):
    """Call ``entry`` with a valid call's arguments but for ``kw``; g / p / spec take a dict of field
    overrides (or NO)."""
    a = dict(ARGS[entry])
    kw = dict(kw)
    make = dict(g=_graph, p=_narrow if "out_ce" in entry else _params, spec=_spec)
    for k, mk in make.items():
        if k in a:
            v = kw.pop(k, {})
            a[k] = None if v is NO else mk(L, **v)
    if entry == "gnn_gat_bwd_workspace_size":
        a["bytes"] = None if kw.pop("bytes", 1) is NO else L.c_size(0)
    assert set(kw) <= set(a), (entry, set(kw) - set(a))
    a.update(kw)
    return getattr(lib, entry)(*a.values())


EMPTY = dict(num_nodes=0, num_slots=0)
BIG = 1 << 27  # rows: x 32 columns = 2^32 elements

CASES = {
    # ---- gnn_gat_scores_f32
    "scores_n": ("gnn_gat_scores_f32", dict(N=-1), 1, SIZES),
    "scores_heads": ("gnn_gat_scores_f32", dict(H=0), 1, SIZES),
    "scores_chans": ("gnn_gat_scores_f32", dict(C=0), 1, SIZES),
    "scores_ld": ("gnn_gat_scores_f32", dict(ld_xh=31), 1, SIZES),
    "scores_empty": ("gnn_gat_scores_f32", dict(N=0, xh=None), 0, None),
    "scores_null": ("gnn_gat_scores_f32", dict(a_dst=None), 1, b"null"),
    "scores_ld_and_null": ("gnn_gat_scores_f32", dict(ld_xh=31, xh=None), 1, SIZES),
    # ---- gnn_gat_fwd_f32
    "fwd_graph": ("gnn_gat_fwd_f32", dict(g=NO), 1, b"null graph"),
    "fwd_heads_3": ("gnn_gat_fwd_f32", dict(H=3), 5, HEADS),
    "fwd_heads_128": ("gnn_gat_fwd_f32", dict(H=128, ld_xh=1024, ldo=1024), 5, HEADS),
    "fwd_heads_0": ("gnn_gat_fwd_f32", dict(H=0), 5, HEADS),
    "fwd_chans": ("gnn_gat_fwd_f32", dict(C=0), 1, SIZES),
    "fwd_ld_xh": ("gnn_gat_fwd_f32", dict(ld_xh=31), 1, SIZES),
    "fwd_ldo_concat": ("gnn_gat_fwd_f32", dict(ldo=31), 1, SIZES),
    "fwd_ldo_mean": ("gnn_gat_fwd_f32", dict(concat=0, ldo=7), 1, SIZES),
    "fwd_empty": ("gnn_gat_fwd_f32", dict(g=EMPTY, xh=None), 0, None),
    "fwd_null": ("gnn_gat_fwd_f32", dict(alpha=None), 1, b"null"),
    "fwd_null_rowptr": ("gnn_gat_fwd_f32", dict(g=dict(rowptr=None)), 1, b"null"),
    "fwd_graph_and_heads": ("gnn_gat_fwd_f32", dict(g=NO, H=3), 1, b"null graph"),
    "fwd_heads_and_sizes": ("gnn_gat_fwd_f32", dict(H=3, C=0), 5, HEADS),
    "fwd_sizes_and_null": ("gnn_gat_fwd_f32", dict(ldo=31, out=None), 1, SIZES),
    # ---- gnn_gat_fwd_fused_f32
    "fused_graph": ("gnn_gat_fwd_fused_f32", dict(g=NO), 1, NO_GP),
    "fused_params": ("gnn_gat_fwd_fused_f32", dict(p=NO), 1, NO_GP),
    "fused_heads": ("gnn_gat_fwd_fused_f32", dict(p=dict(heads=3)), 5, HEADS),
    "fused_chans": ("gnn_gat_fwd_fused_f32", dict(p=dict(chans=0)), 1, SIZES),
    "fused_ld_xh": ("gnn_gat_fwd_fused_f32", dict(p=dict(ld_xh=31)), 1, SIZES),
    "fused_ldo_mean": ("gnn_gat_fwd_fused_f32", dict(p=dict(concat=0, ldo=7)), 1, SIZES),
    "fused_act": ("gnn_gat_fwd_fused_f32", dict(p=dict(act=2)), 1, ACT),
    "fused_p_one": ("gnn_gat_fwd_fused_f32", dict(p=dict(dropout_p=1.0)), 1, DROP),
    "fused_p_negative": ("gnn_gat_fwd_fused_f32", dict(p=dict(dropout_p=-0.25)), 1, DROP),
    "fused_p_nan": ("gnn_gat_fwd_fused_f32", dict(p=dict(dropout_p=float("nan"))), 1, DROP),
    "fused_index": ("gnn_gat_fwd_fused_f32", dict(g=dict(num_nodes=BIG)), 5, INDEX),
    "fused_index_mean": ("gnn_gat_fwd_fused_f32", dict(g=dict(num_nodes=4 * BIG), p=dict(concat=0, ldo=8)), 5, INDEX),
    "fused_empty": ("gnn_gat_fwd_fused_f32", dict(g=EMPTY, p=dict(xh=None)), 0, None),
    "fused_null": ("gnn_gat_fwd_fused_f32", dict(p=dict(att_dst=None)), 1, b"null"),
    "fused_null_col": ("gnn_gat_fwd_fused_f32", dict(g=dict(col=None)), 1, b"null"),
    "fused_nproj_5": ("gnn_gat_fwd_fused_f32", dict(p=dict(nproj=5, proj=FAKE, z=FAKE, ldz=5)), 1, PROJ),
    "fused_nproj_negative": ("gnn_gat_fwd_fused_f32", dict(p=dict(nproj=-1)), 1, PROJ),
    "fused_proj_mean": ("gnn_gat_fwd_fused_f32", dict(p=dict(concat=0, ldo=8, nproj=2, proj=FAKE, z=FAKE, ldz=2)), 1,
                        PROJ),
    "fused_proj_null": ("gnn_gat_fwd_fused_f32", dict(p=dict(nproj=2, z=FAKE, ldz=2)), 1, PROJ),
    "fused_proj_no_z": ("gnn_gat_fwd_fused_f32", dict(p=dict(nproj=2, proj=FAKE, ldz=2)), 1, PROJ),
    "fused_proj_ldz": ("gnn_gat_fwd_fused_f32", dict(p=dict(nproj=2, proj=FAKE, z=FAKE, ldz=1)), 1, PROJ),
    "fused_proj_align": ("gnn_gat_fwd_fused_f32", dict(p=dict(nproj=2, proj=FAKE + 4, z=FAKE, ldz=2)), 1, PROJ),
    "fused_heads_and_act": ("gnn_gat_fwd_fused_f32", dict(p=dict(heads=3, act=2)), 5, HEADS),
    "fused_sizes_and_act": ("gnn_gat_fwd_fused_f32", dict(p=dict(ldo=31, act=2)), 1, SIZES),
    "fused_act_and_p": ("gnn_gat_fwd_fused_f32", dict(p=dict(act=2, dropout_p=1.0)), 1, ACT),
    "fused_index_and_null": ("gnn_gat_fwd_fused_f32", dict(g=dict(num_nodes=BIG), p=dict(xh=None)), 5, INDEX),
    "fused_null_and_proj": ("gnn_gat_fwd_fused_f32", dict(p=dict(xh=None, nproj=5)), 1, b"null"),
    # ---- gnn_gat_act_bwd_f32
    "act_bwd_n": ("gnn_gat_act_bwd_f32", dict(N=-1), 1, SIZES),
    "act_bwd_f_0": ("gnn_gat_act_bwd_f32", dict(F=0), 1, SIZES),
    "act_bwd_f_2_31": ("gnn_gat_act_bwd_f32", dict(F=1 << 31, ldy=1 << 31, lddy=1 << 31, ld_dpre=1 << 31, dropout_p=0.0),
                       1, SIZES),
    "act_bwd_ldy": ("gnn_gat_act_bwd_f32", dict(ldy=31), 1, SIZES),
    "act_bwd_lddy": ("gnn_gat_act_bwd_f32", dict(lddy=31), 1, SIZES),
    "act_bwd_ld_dpre": ("gnn_gat_act_bwd_f32", dict(ld_dpre=31), 1, SIZES),
    "act_bwd_act": ("gnn_gat_act_bwd_f32", dict(act=-1), 1, ACT),
    "act_bwd_p": ("gnn_gat_act_bwd_f32", dict(dropout_p=1.5), 1, DROP),
    "act_bwd_index": ("gnn_gat_act_bwd_f32", dict(N=BIG), 5, INDEX),
    "act_bwd_empty": ("gnn_gat_act_bwd_f32", dict(N=0, y=None), 0, None),
    "act_bwd_null": ("gnn_gat_act_bwd_f32", dict(dy=None), 1, b"null"),
    "act_bwd_sizes_and_act": ("gnn_gat_act_bwd_f32", dict(ldy=31, act=2), 1, SIZES),
    "act_bwd_p_and_index": ("gnn_gat_act_bwd_f32", dict(N=BIG, dropout_p=1.0), 1, DROP),
    # ---- gnn_gat_bwd_workspace_size
    "ws_bytes": ("gnn_gat_bwd_workspace_size", dict(bytes=NO), 1, b"bad args"),
    "ws_n": ("gnn_gat_bwd_workspace_size", dict(N=-1), 1, b"bad args"),
    "ws_s": ("gnn_gat_bwd_workspace_size", dict(S=-1), 1, b"bad args"),
    "ws_heads": ("gnn_gat_bwd_workspace_size", dict(H=0), 1, b"bad args"),
    "ws_chans": ("gnn_gat_bwd_workspace_size", dict(C=0), 1, b"bad args"),
    # ---- gnn_gat_bwd_f32
    "bwd_graph": ("gnn_gat_bwd_f32", dict(g=NO), 1, b"null graph"),
    "bwd_heads": ("gnn_gat_bwd_f32", dict(H=6), 5, HEADS),
    "bwd_chans": ("gnn_gat_bwd_f32", dict(C=0), 1, SIZES),
    "bwd_ld_xh": ("gnn_gat_bwd_f32", dict(ld_xh=31), 1, SIZES),
    "bwd_ld_dxh": ("gnn_gat_bwd_f32", dict(ld_dxh=31), 1, SIZES),
    "bwd_ld_dout_concat": ("gnn_gat_bwd_f32", dict(ld_dout=31), 1, SIZES),
    "bwd_ld_dout_mean": ("gnn_gat_bwd_f32", dict(concat=0, ld_dout=7), 1, SIZES),
    "bwd_null": ("gnn_gat_bwd_f32", dict(alpha=None), 1, b"null"),
    "bwd_null_csc2csr": ("gnn_gat_bwd_f32", dict(g=dict(csc2csr=None)), 1, b"null"),
    "bwd_workspace": ("gnn_gat_bwd_f32", dict(workspace_bytes=0), 4, WORKSPACE),
    "bwd_heads_and_sizes": ("gnn_gat_bwd_f32", dict(H=6, ld_dxh=1), 5, HEADS),
    "bwd_sizes_and_workspace": ("gnn_gat_bwd_f32", dict(ld_dxh=31, workspace_bytes=0), 1, SIZES),
    "bwd_null_and_workspace": ("gnn_gat_bwd_f32", dict(xh=None, workspace_bytes=0), 1, b"null"),
    # ---- gnn_gat_bwd_act_f32
    "bwd_act_act": ("gnn_gat_bwd_act_f32", dict(act=2), 1, ACT),
    "bwd_act_p": ("gnn_gat_bwd_act_f32", dict(dropout_p=1.0), 1, DROP),
    "bwd_act_graph": ("gnn_gat_bwd_act_f32", dict(g=NO), 1, Y_DPRE),
    "bwd_act_y": ("gnn_gat_bwd_act_f32", dict(y=None), 1, Y_DPRE),
    "bwd_act_dpre": ("gnn_gat_bwd_act_f32", dict(dpre=None), 1, Y_DPRE),
    "bwd_act_ld_y": ("gnn_gat_bwd_act_f32", dict(ld_y=31), 1, Y_DPRE),
    "bwd_act_ld_dpre": ("gnn_gat_bwd_act_f32", dict(ld_dpre=31), 1, Y_DPRE),
    "bwd_act_index": ("gnn_gat_bwd_act_f32", dict(g=dict(num_nodes=BIG)), 5, INDEX),
    "bwd_act_heads": ("gnn_gat_bwd_act_f32", dict(H=3), 5, HEADS),
    "bwd_act_ld_xh": ("gnn_gat_bwd_act_f32", dict(ld_xh=31), 1, SIZES),
    "bwd_act_ld_dy": ("gnn_gat_bwd_act_f32", dict(ld_dy=31), 1, SIZES),
    "bwd_act_null": ("gnn_gat_bwd_act_f32", dict(dy=None), 1, b"null"),
    "bwd_act_workspace": ("gnn_gat_bwd_act_f32", dict(workspace_bytes=0), 4, WORKSPACE),
    "bwd_act_act_and_y": ("gnn_gat_bwd_act_f32", dict(act=2, y=None), 1, ACT),
    "bwd_act_y_and_heads": ("gnn_gat_bwd_act_f32", dict(ld_y=23, H=3), 1, Y_DPRE),
    # ---- gnn_gat_bwd_act_proj_f32
    "bwd_proj_act": ("gnn_gat_bwd_act_proj_f32", dict(act=2), 1, ACT),
    "bwd_proj_p": ("gnn_gat_bwd_act_proj_f32", dict(dropout_p=-1.0), 1, DROP),
    "bwd_proj_graph": ("gnn_gat_bwd_act_proj_f32", dict(g=NO), 1, Y_DZ),
    "bwd_proj_y": ("gnn_gat_bwd_act_proj_f32", dict(y=None), 1, Y_DZ),
    "bwd_proj_dz": ("gnn_gat_bwd_act_proj_f32", dict(dz=None), 1, Y_DZ),
    "bwd_proj_proj": ("gnn_gat_bwd_act_proj_f32", dict(proj=None), 1, Y_DZ),
    "bwd_proj_ld_dpre": ("gnn_gat_bwd_act_proj_f32", dict(ld_dpre=31), 1, Y_DZ),
    "bwd_proj_nproj_0": ("gnn_gat_bwd_act_proj_f32", dict(nproj=0), 1, Y_DZ),
    "bwd_proj_nproj_5": ("gnn_gat_bwd_act_proj_f32", dict(nproj=5, ld_dz=5), 1, Y_DZ),
    "bwd_proj_ld_dz": ("gnn_gat_bwd_act_proj_f32", dict(ld_dz=1), 1, Y_DZ),
    "bwd_proj_align": ("gnn_gat_bwd_act_proj_f32", dict(proj=FAKE + 8), 1, Y_DZ),
    "bwd_proj_index": ("gnn_gat_bwd_act_proj_f32", dict(g=dict(num_nodes=BIG)), 5, INDEX),
    "bwd_proj_heads": ("gnn_gat_bwd_act_proj_f32", dict(H=3), 5, HEADS),
    "bwd_proj_ld_dxh": ("gnn_gat_bwd_act_proj_f32", dict(ld_dxh=31), 1, SIZES),
    "bwd_proj_null": ("gnn_gat_bwd_act_proj_f32", dict(att_src=None), 1, b"null"),
    "bwd_proj_null_colptr": ("gnn_gat_bwd_act_proj_f32", dict(g=dict(colptr=None)), 1, b"null"),
    "bwd_proj_workspace": ("gnn_gat_bwd_act_proj_f32", dict(workspace_bytes=0), 4, WORKSPACE),
    "bwd_proj_act_and_align": ("gnn_gat_bwd_act_proj_f32", dict(act=2, proj=FAKE + 4), 1, ACT),
    "bwd_proj_p_and_graph": ("gnn_gat_bwd_act_proj_f32", dict(dropout_p=1.0, g=NO), 1, DROP),
    "bwd_proj_align_and_index": ("gnn_gat_bwd_act_proj_f32", dict(proj=FAKE + 4, g=dict(num_nodes=BIG)), 1, Y_DZ),
    # ---- gnn_gat_bwd_ew_f32
    "bwd_ew_edge_w": ("gnn_gat_bwd_ew_f32", dict(edge_w=None), 1, EDGE_W),
    "bwd_ew_d_edge_w": ("gnn_gat_bwd_ew_f32", dict(d_edge_w=None), 1, EDGE_W),
    "bwd_ew_graph": ("gnn_gat_bwd_ew_f32", dict(g=NO), 1, b"null graph"),
    "bwd_ew_heads": ("gnn_gat_bwd_ew_f32", dict(H=5), 5, HEADS),
    "bwd_ew_ld_dout_mean": ("gnn_gat_bwd_ew_f32", dict(concat=0, ld_dout=7), 1, SIZES),
    "bwd_ew_null": ("gnn_gat_bwd_ew_f32", dict(d_att_dst=None), 1, b"null"),
    "bwd_ew_workspace": ("gnn_gat_bwd_ew_f32", dict(workspace_bytes=0), 4, WORKSPACE),
    "bwd_ew_edge_w_and_heads": ("gnn_gat_bwd_ew_f32", dict(edge_w=None, H=5), 1, EDGE_W),
    # ---- gnn_gat_out_ce_f32
    "out_ce_graph": ("gnn_gat_out_ce_f32", dict(g=NO), 1, NO_GP),
    "out_ce_params": ("gnn_gat_out_ce_f32", dict(p=NO), 1, NO_GP),
    "out_ce_heads": ("gnn_gat_out_ce_f32", dict(p=dict(heads=2, ld_xh=4)), 5, NARROW),
    "out_ce_chans": ("gnn_gat_out_ce_f32", dict(p=dict(chans=3, ld_xh=3, ldo=3)), 5, NARROW),
    "out_ce_concat": ("gnn_gat_out_ce_f32", dict(p=dict(concat=1)), 5, NARROW),
    "out_ce_act": ("gnn_gat_out_ce_f32", dict(p=dict(act=1)), 5, NARROW),
    "out_ce_dropout": ("gnn_gat_out_ce_f32", dict(p=dict(dropout_p=0.5)), 5, NARROW),
    "out_ce_edge_w": ("gnn_gat_out_ce_f32", dict(p=dict(edge_w=FAKE)), 5, NARROW),
    "out_ce_ld_xh": ("gnn_gat_out_ce_f32", dict(p=dict(ld_xh=1)), 1, b"bad leading dimensions"),
    "out_ce_ldo": ("gnn_gat_out_ce_f32", dict(p=dict(ldo=1)), 1, b"bad leading dimensions"),
    "out_ce_empty": ("gnn_gat_out_ce_f32", dict(g=EMPTY), 1, OUT_NULL),
    "out_ce_null": ("gnn_gat_out_ce_f32", dict(p=dict(a_src=None)), 1, OUT_NULL),
    "out_ce_null_col": ("gnn_gat_out_ce_f32", dict(g=dict(col=None)), 1, OUT_NULL),
    "out_ce_mask": ("gnn_gat_out_ce_f32", dict(mask=None), 1, b"CE operands"),
    "out_ce_class_w": ("gnn_gat_out_ce_f32", dict(class_w=None), 1, b"CE operands"),
    "out_ce_dlogits": ("gnn_gat_out_ce_f32", dict(dlogits=None), 1, b"CE operands"),
    "out_ce_ld_d": ("gnn_gat_out_ce_f32", dict(ld_d=1), 1, b"CE operands"),
    "out_ce_no_workspace": ("gnn_gat_out_ce_f32", dict(workspace=None), 4, WORKSPACE),
    "out_ce_workspace": ("gnn_gat_out_ce_f32", dict(workspace_bytes=15), 4, WORKSPACE),  # 4 blocks of 256 rows
    "out_ce_heads_and_ld": ("gnn_gat_out_ce_f32", dict(p=dict(heads=2, ldo=1)), 5, NARROW),
    "out_ce_mask_and_workspace": ("gnn_gat_out_ce_f32", dict(mask=None, workspace=None), 1, b"CE operands"),
    # ---- gnn_gat_out_ce_spec_f32
    "out_spec_params": ("gnn_gat_out_ce_spec_f32", dict(p=NO), 1, NO_GP),
    "out_spec_concat": ("gnn_gat_out_ce_spec_f32", dict(p=dict(concat=1)), 5, NARROW),
    "out_spec_ldo": ("gnn_gat_out_ce_spec_f32", dict(p=dict(ldo=1)), 1, b"bad leading dimensions"),
    "out_spec_null": ("gnn_gat_out_ce_spec_f32", dict(p=dict(alpha=None)), 1, OUT_NULL),
    "out_spec_mask": ("gnn_gat_out_ce_spec_f32", dict(spec=dict(mask=None)), 1, b"CE operands"),
    "out_spec_gamma": ("gnn_gat_out_ce_spec_f32", dict(spec=dict(focal=1, focal_gamma=0.5)), 1,
                       b"focal_gamma < 1 (unbounded gradient at p = 1)"),
    "out_spec_workspace": ("gnn_gat_out_ce_spec_f32", dict(workspace_bytes=15), 4, WORKSPACE),
    "out_spec_gamma_and_workspace": ("gnn_gat_out_ce_spec_f32",
                                     dict(spec=dict(focal=1, focal_gamma=0.5), workspace=None), 1,
                                     b"focal_gamma < 1 (unbounded gradient at p = 1)"),
}


@pytest.fixture()
def refusing(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a refusal that regressed would launch over fake pointers: CPU machines only")
    from elliptic_gnn_project_amd import _lib

    return lib, _lib


@pytest.mark.parametrize("case", sorted(CASES))
def test_gat_refusal(refusing, case):
    lib, _lib = refusing
    entry, kw, status, what = CASES[case]
    assert _call(lib, _lib, entry, kw) == status
    if what is not None:
        assert lib.gnn_last_error() == entry.encode() + b": " + what


def test_bwd_workspace_one_byte_short(refusing):
    """The carve takes all but the 256 bytes of slack the size query adds."""
    lib, _lib = refusing
    n = _lib.c_size(0)
    assert lib.gnn_gat_bwd_workspace_size(1000, 4000, 4, 8, n) == 0
    for entry in ("gnn_gat_bwd_f32", "gnn_gat_bwd_act_f32", "gnn_gat_bwd_act_proj_f32", "gnn_gat_bwd_ew_f32"):
        assert _call(lib, _lib, entry, dict(workspace_bytes=n.value - 257)) == 4
        assert lib.gnn_last_error() == entry.encode() + b": " + WORKSPACE


def test_bwd_workspace_size_matches_the_recorded_table(lib):
    """gnn_gat_bwd_workspace_size over N, S in {0, 1, 37, 5000} x (H, C) in {(1, 2), (4, 8), (4, 64), (64, 1)}:
    the bytes recorded from the build before carve_bwd's partial count got its name."""
    from elliptic_gnn_project_amd import _lib

    want = json.loads(GOLDEN.read_text())
    assert want["fields"] == ["N", "S", "H", "C", "bytes"] and len(want["rows"]) == 64
    seen = set()
    for N, S, H, C, nbytes in want["rows"]:
        n = _lib.c_size(0)
        assert lib.gnn_gat_bwd_workspace_size(N, S, H, C, n) == 0
        assert n.value == nbytes, (N, S, H, C)
        seen.add((N, S, H, C))
    assert seen == {(N, S, H, C) for N in (0, 1, 37, 5000) for S in (0, 1, 37, 5000)
                    for H, C in ((1, 2), (4, 8), (4, 64), (64, 1))}
