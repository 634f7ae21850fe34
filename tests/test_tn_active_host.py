"""CPU: the host side of the activity flags (include/gnnmp.h ABI 28) — gnn_agg_active's layout, the
shape rule gnn_gemm_tn_active_pays, the workspace's flag bytes, and every unsupported combination of
gnn_aggregate_active_f32 / gnn_gemm_tn_active_f32 refused before any launch (the pointers below are
never read).  No device calls."""
import ctypes
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gnnmp.h"
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
FAKE = 1 << 20


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():  # a fresh checkout: build it (hipcc cross-compiles gfx950 without a GPU)
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    from elliptic_gnn_project_amd import _lib

    return _lib.load()


def test_agg_active_layout_and_abi(lib, tmp_path):
    from elliptic_gnn_project_amd import _lib

    fields = ["row_active", "active_with", "ld_active_with", "active_with_cols"]
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
           'printf("size %zu\\n", sizeof(gnn_agg_active));', 'printf("rows %d\\n", GNN_ACTIVE_ROWS);',
           'printf("abi %d\\n", GNNMP_ABI_VERSION);']
    src += [f'printf("{f} %zu\\n", offsetof(gnn_agg_active, {f}));' for f in fields]
    src += ["return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    assert [f[0] for f in _lib.GnnAggActive._fields_] == fields
    assert int(got["size"]) == ctypes.sizeof(_lib.GnnAggActive)
    for f in fields:
        assert int(got[f]) == getattr(_lib.GnnAggActive, f).offset, f
    assert int(got["rows"]) == _lib.ACTIVE_ROWS == 16
    assert int(got["abi"]) == _lib.ABI_VERSION == lib.gnn_abi_version() and _lib.ABI_VERSION >= 28


def test_active_pays_is_a_rule_of_the_row_count(lib):
    """More than 448 rows per dz-form row block: M > 114,688 (256 blocks of 14 32-row chunks)."""
    for M, want in ((0, 0), (15, 0), (4000, 0), (32_768, 0), (100_000, 0), (114_688, 0), (114_689, 1), (115_000, 1),
                    (203_769, 1), (1_500_000, 1)):
        assert lib.gnn_gemm_tn_active_pays(M) == want, M


def test_tn_workspace_counts_the_flag_bytes(lib):
    from elliptic_gnn_project_amd import _lib

    def size(M, nproj):
        n = _lib.c_size(0)
        assert lib.gnn_gemm_tn_workspace_size(M, 128, 332, nproj, n) == 0
        return n.value

    def slabs(M, nproj):
        chunks = (M + 31) // 32
        per = (chunks + 255) // 256
        nblk = (chunks + per - 1) // per
        stride = (128 * 332 + 128 + nproj * 128 + nproj + 63) // 64 * 64
        return nblk * stride * 4

    assert size(203_769, 4) == slabs(203_769, 4) + (12_736 + 15) // 16 * 16
    assert size(203_769, 0) == slabs(203_769, 0)  # the g form has no dz
    assert size(100_000, 4) == slabs(100_000, 4)  # below the threshold: no flags


def _tn_params(_lib, M=1000):
    """The half-pair dz form with h over a 336-wide image: the one form that takes flags."""
    p = _lib.GnnGemmTNParams(M, 128, None, 0, FAKE, 4, FAKE, 4, FAKE, 128, 1.0, None, 0, None, 0, 166, None, 0, 166)
    p.math = _lib.MATH_SPLIT_BF16
    p.a_planes, p.planes_ld, p.planes_stride, p.planes_col2 = FAKE, 336, M * 336, 168
    p.planes_format = _lib.PLANES_HALF_PAIR
    return p


def test_tn_active_refusals(lib):
    from elliptic_gnn_project_amd import _lib

    ws = 1 << 30

    def call(p, flags=FAKE):
        return lib.gnn_gemm_tn_active_f32(p, flags, FAKE, FAKE, ws, None)

    p = _tn_params(_lib)
    p.gout, p.ldgout = FAKE, 128  # with gout
    assert call(p) == 5 and b"dz_active" in lib.gnn_last_error()
    p = _tn_params(_lib)
    g = _lib.GnnGraph(1000, 4000, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
    p.dz_graph, p.dz_u, p.ldu, p.dz_cols = ctypes.addressof(g), FAKE, 2, 2  # with the CSC fold
    assert call(p) == 5
    p = _tn_params(_lib)
    p.dz, p.lddz, p.proj, p.nproj, p.h, p.ldh = None, 0, None, 0, None, 0  # the plain g form
    p.g, p.ldg = FAKE, 128
    assert call(p) == 5
    p = _tn_params(_lib)
    p.h, p.ldh = None, 0  # the dz form without h
    assert call(p) == 5
    p = _tn_params(_lib)
    p.planes_format = _lib.PLANES_SPLIT_BF16  # the split-image family
    assert call(p) == 5
    p = _tn_params(_lib)
    p.a_planes = None  # f32 operands: the split / in-kernel families
    p.a1, p.lda1, p.a2, p.lda2 = FAKE, 166, FAKE, 166
    assert call(p) == 5
    p.math = _lib.MATH_HALF_PAIR
    assert call(p) == 5
    p = _tn_params(_lib)
    p.math = _lib.MATH_F32
    assert call(p) == 5
    p = _tn_params(_lib)
    p.planes_ld, p.planes_stride = 176, 1000 * 176  # a half-pair image the dz form does not take
    assert call(p) == 5
    p = _tn_params(_lib, M=15)  # below one chunk
    assert call(p) == 5
    p = _tn_params(_lib)
    assert call(p, FAKE + 4) == 1 and b"aligned" in lib.gnn_last_error()


def test_aggregate_active_refusals(lib):
    from elliptic_gnn_project_amd import _lib

    g = _lib.GnnGraph(1000, 4000, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)

    def call(mode, F, act):
        p = _lib.GnnAggParams(mode, 1, FAKE, FAKE, 1)
        return lib.gnn_aggregate_active_f32(g, p, FAKE, F, F, FAKE, F, act, None)

    act = _lib.GnnAggActive(FAKE, FAKE, 2, 2)
    assert call(_lib.AGG_SUM, 8, act) == 5 and b"narrow" in lib.gnn_last_error()  # the lane-group gather
    assert call(_lib.AGG_SUM, 64, act) == 5  # the flat / wave gathers (and the long-segment split)
    assert call(_lib.AGG_MEAN_BWD, 5, act) == 5
    assert call(_lib.AGG_GCN, 4, act) == 5  # GCN's narrow form stops at F = 2
    assert call(_lib.AGG_EDGE_W, 2, act) == 5
    assert call(_lib.AGG_SUM, 2, _lib.GnnAggActive(FAKE + 1, FAKE, 2, 2)) == 1  # unaligned flags
    assert call(_lib.AGG_SUM, 2, _lib.GnnAggActive(FAKE, FAKE, 2, 5)) == 1  # more than 4 other columns
    assert call(_lib.AGG_SUM, 2, _lib.GnnAggActive(FAKE, FAKE, 1, 2)) == 1  # ld below the columns
    assert call(_lib.AGG_SUM, 2, _lib.GnnAggActive(FAKE, None, 0, 2)) == 1  # columns without a pointer
