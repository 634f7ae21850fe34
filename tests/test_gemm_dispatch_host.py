"""CPU: the GEMM dispatch (csrc/gemm_dispatch.hip) decides as the recorded table says, and refuses
what it cannot take before any launch.  No device calls; the pointers below are never read.

The table (tests/golden/gemm_dispatch_golden.json, written by tests/golden/make_gemm_dispatch_golden.py
from the build before the dispatch had a file of its own) holds what the side-effect-free entries
answer over a lattice of calls; the replay runs in a child process without the GNNMP_TN_* A/B
switches, which the library reads once per process."""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
GOLDEN = ROOT / "tests" / "golden" / "gemm_dispatch_golden.json"
FAKE = 1 << 20
WS = 1 << 30


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():  # a fresh checkout: build it (hipcc cross-compiles gfx950 without a GPU)
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    from elliptic_gnn_project_amd import _lib

    return _lib.load()


def test_decisions_match_the_recorded_table(lib):
    env = {k: v for k, v in os.environ.items() if k not in ("GNNMP_TN_KSPLIT_MAXM", "GNNMP_TN_CSC_INKERNEL")}
    out = subprocess.run([sys.executable, str(GOLDEN.with_name("make_gemm_dispatch_golden.py")), "--print"], env=env,
                         capture_output=True, text=True, check=True).stdout
    got, want = json.loads(out), json.loads(GOLDEN.read_text())
    assert sorted(got) == sorted(want)
    assert len(want["nt"]) > 1000 and len(want["tn"]) > 1000
    for table, rows in want.items():
        assert len(got[table]) == len(rows), table
        for g, w in zip(got[table], rows):
            assert g == w, (table, want.get(table[:2] + "_fields"), w, g)


# ------------------------------------------------------------------------------- refusals
# One case per refusal of the two dispatchers that fake pointers reach: (entry, params, status,
# substring of gnn_last_error).  1 = INVALID_ARG, 4 = WORKSPACE, 5 = UNSUPPORTED.

def _nt(_lib, M=1000, N=128, k1=128, k2=0, **kw):
    """A valid f32-operand NT call in the w1 form."""
    p = _lib.GnnGemmNTParams(M, N, FAKE, k1, k1, FAKE if k2 else None, k2, k2, None, 0, FAKE, FAKE if k2 else None,
                             k1, k2, FAKE, N)
    p.math = _lib.MATH_SPLIT_BF16
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _nt_img(_lib, fmt, M=1000, N=128, **kw):
    """A valid NT call over a 336-wide image alone (no f32 A), with a workspace."""
    p = _nt(_lib, M, N, 166, 166, a1=None, a2=None, lda1=0, lda2=0, a_planes=FAKE, planes_ld=336,
            planes_stride=M * 336, planes_col2=168, planes_format=fmt, workspace=FAKE, workspace_bytes=WS)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


NT_REFUSALS = {
    "shapes": (lambda L: _nt(L, k1=0), 1, b"bad shapes"),
    "no_a": (lambda L: _nt(L, a1=None), 1, b"bad shapes"),
    "no_b": (lambda L: _nt(L, w1=None), 1, b"need bt or w1"),
    "w_form_n": (lambda L: _nt(L, N=129, ldc=129), 1, b"w1/w2 form"),
    "ldw": (lambda L: _nt(L, ldw1=127), 1, b"w1/w2 form"),
    "lda": (lambda L: _nt(L, lda1=127), 1, b"leading dimensions"),
    "ldc": (lambda L: _nt(L, ldc=127), 1, b"leading dimensions"),
    "proj": (lambda L: _nt(L, nproj=2, proj=FAKE), 1, b"projection"),
    "nproj": (lambda L: _nt(L, nproj=5, proj=FAKE, z=FAKE, ldz=5), 1, b"projection"),
    "dropout_p": (lambda L: _nt(L, dropout_p=1.0), 1, b"dropout p"),
    "math": (lambda L: _nt(L, math=3), 1, b"bad math mode"),
    "dtype": (lambda L: _nt(L, c_dtype=2), 1, b"bad dtype"),
    "ldmask": (lambda L: _nt(L, N=8, ldc=8, mask=FAKE, ldmask=7), 1, b"bad ldmask"),
    "planes_format": (lambda L: _nt_img(L, 2), 1, b"bad planes_format"),
    "planes_exp": (lambda L: _nt_img(L, L.PLANES_HALF_PAIR, planes_exp=101), 1, b"planes_exp"),
    "keep_mask": (lambda L: _nt_img(L, L.PLANES_HALF_PAIR, keep_mask=FAKE), 1, b"keep_mask"),
    "row_exp_image": (lambda L: _nt_img(L, L.PLANES_HALF_PAIR, row_exp=FAKE), 5, b"row_exp"),
    "row_exp_shape": (lambda L: _nt(L, k1=166, lda1=166, ldw1=166, math=L.MATH_HALF_PAIR, row_exp=FAKE, workspace=FAKE,
                                    workspace_bytes=WS), 5, b"row_exp"),
    "colsum_shape": (lambda L: _nt(L, colsum_part=FAKE, colsum_cap=1 << 40), 5, b"colsum_part"),
    "colsum_cap": (lambda L: _nt(L, N=64, k1=8, lda1=8, ldw1=8, ldc=64, colsum_part=FAKE, colsum_cap=63), 1,
                   b"colsum_cap"),
    "h2_image_shape": (lambda L: _nt_img(L, L.PLANES_HALF_PAIR, N=126, ldc=126), 5, b"half-pair image A"),
    "h2_image_no_workspace": (lambda L: _nt_img(L, L.PLANES_HALF_PAIR, workspace_bytes=0), 5, b"half-pair image A"),
    "bf16_image_shape": (lambda L: _nt_img(L, L.PLANES_SPLIT_BF16, a_dtype=L.DTYPE_BF16), 5, b"bf16 image A"),
    "split_image_shape": (lambda L: _nt_img(L, L.PLANES_SPLIT_BF16, N=64, ldc=64), 5, b"split-image A"),
    "split_image_f32_math": (lambda L: _nt_img(L, L.PLANES_SPLIT_BF16, math=L.MATH_F32), 5, b"split-image A"),
    "b_ready": (lambda L: _nt(L, b_ready=1), 1, b"image-A"),
    "mask_shape": (lambda L: _nt(L, mask=FAKE, ldmask=128), 5, b"mask epilogue"),
    "bf16_c": (lambda L: _nt(L, c_dtype=L.DTYPE_BF16), 5, b"bf16 NT"),
    "bf16_f32_math": (lambda L: _nt(L, a_dtype=L.DTYPE_BF16, c_dtype=L.DTYPE_BF16, math=L.MATH_F32), 5, b"bf16 NT"),
}


def _tn(_lib, M=1000, Nr=128, dz=False, **kw):
    """A valid f32-operand TN call: the plain g form, or the dz form with h."""
    p = _lib.GnnGemmTNParams(M, Nr, None, 0, None, 0, None, 0, None, 0, 1.0, None, 0, FAKE, 166, 166, FAKE, 166, 166)
    if dz:
        p.dz, p.lddz, p.proj, p.nproj, p.h, p.ldh = FAKE, 4, FAKE, 4, FAKE, Nr
    else:
        p.g, p.ldg = FAKE, Nr
    p.math = _lib.MATH_SPLIT_BF16
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _tn_img(_lib, fmt, M=1000, ld=336, **kw):
    """A valid TN call over an image alone (no f32 A)."""
    return _tn(_lib, M, **dict(dict(a1=None, a2=None, lda1=0, lda2=0, a_planes=FAKE, planes_ld=ld, planes_stride=M * ld,
                                    planes_col2=168, planes_format=fmt), **kw))


_GRAPHS = []


def _csc(_lib, M, **kw):
    """dz_graph fields of a CSC fold over M nodes."""
    _GRAPHS.append(_lib.GnnGraph(M, 4 * M, FAKE, FAKE, FAKE, FAKE, FAKE, None, None))
    return dict(dict(dz_graph=ctypes.addressof(_GRAPHS[-1]), dz_u=FAKE, ldu=2, dz_cols=2), **kw)


def _slabs(M, Nr, Kc, nproj):
    """Bytes of the slabs of the 256-block TN launch: the least workspace any call takes."""
    chunks = (M + 31) // 32
    per = (chunks + 255) // 256
    return (chunks + per - 1) // per * ((Nr * Kc + Nr + nproj * Nr + nproj + 63) // 64 * 64) * 4


TN_REFUSALS = {  # name: (params, status, substring[, workspace bytes[, dz_active]])
    "nr": (lambda L: _tn(L, Nr=129, ldg=129), 5, b"1 <= Nr <= 128"),
    "kc": (lambda L: _tn(L, k1=200, k2=200, lda1=200, lda2=200), 5, b"k1 + k2 <= 384"),
    "no_a": (lambda L: _tn(L, a1=None), 1, b"bad A operands"),
    "lda": (lambda L: _tn(L, lda2=165), 1, b"bad A operands"),
    "dz_nproj": (lambda L: _tn(L, dz=True, nproj=5, lddz=5), 1, b"dz form"),
    "no_g": (lambda L: _tn(L, g=None), 1, b"need g"),
    "ldh": (lambda L: _tn(L, h=FAKE, ldh=127), 1, b"bad ldh"),
    "math": (lambda L: _tn(L, math=3), 1, b"bad math mode"),
    "ldgout": (lambda L: _tn(L, gout=FAKE, ldgout=127), 1, b"bad ldgout"),
    "workspace": (lambda L: _tn(L), 4, b"workspace too small", _slabs(1000, 128, 332, 0) - 1),
    "sq_step": (lambda L: _tn(L, sq_partial=FAKE, sq_cap=1 << 20), 1, b"sq_partial"),
    "sq_cap": (lambda L: _tn(L, sq_partial=FAKE, sq_step=FAKE, sq_cap=10), 1, b"sq_partial"),
    "dz_graph_cols": (lambda L: _tn_img(L, L.PLANES_HALF_PAIR, dz=True, **_csc(L, 1000, dz_cols=3)), 1, b"dz_graph"),
    "dz_graph_g_form": (lambda L: _tn_img(L, L.PLANES_HALF_PAIR, **_csc(L, 1000)), 1, b"dz_graph"),
    "dtype": (lambda L: _tn(L, h_dtype=2), 1, b"bad dtype"),
    "bf16_g": (lambda L: _tn(L, g_dtype=L.DTYPE_BF16), 5, b"bf16 g"),
    "bf16_h": (lambda L: _tn(L, dz=True, h_dtype=L.DTYPE_BF16), 5, b"bf16 h"),
    "planes_format": (lambda L: _tn_img(L, 2), 1, b"bad planes_format"),
    "planes_exp": (lambda L: _tn_img(L, L.PLANES_HALF_PAIR, planes_exp=-101), 1, b"planes_exp"),
    "active_shape": (lambda L: _tn_img(L, L.PLANES_HALF_PAIR, dz=True, planes_col2=164), 5, b"dz_active outside",
                     WS, FAKE),
    "flags_workspace": (lambda L: _tn_img(L, L.PLANES_HALF_PAIR, M=203_769, dz=True, **_csc(L, 203_769)), 4,
                        b"activity flags", _slabs(203_769, 128, 332, 4)),
    "h2_image_shape": (lambda L: _tn_img(L, L.PLANES_HALF_PAIR, ld=256), 5, b"half-pair image A"),
    "dz_graph_f32_a": (lambda L: _tn(L, dz=True, **_csc(L, 1000)), 5, b"dz_graph outside"),
    "dz_graph_split_image": (lambda L: _tn_img(L, L.PLANES_SPLIT_BF16, dz=True, **_csc(L, 1000)), 5, b"dz_graph outside"),
    "bf16_image_shape": (lambda L: _tn_img(L, L.PLANES_SPLIT_BF16, ld=176, a_dtype=L.DTYPE_BF16), 5, b"bf16 image A"),
    "split_image_shape": (lambda L: _tn_img(L, L.PLANES_SPLIT_BF16, M=15), 5, b"split-image A"),
    "split_image_f32_math": (lambda L: _tn_img(L, L.PLANES_SPLIT_BF16, math=L.MATH_F32), 5, b"split-image A"),
    "skinny_workspace": (lambda L: _tn(L, M=100_000, Nr=8, ldg=8), 4, b"workspace too small", _slabs(100_000, 8, 332, 0)),
    "bf16_f32_math": (lambda L: _tn(L, a_dtype=L.DTYPE_BF16, math=L.MATH_F32), 5, b"bf16 TN"),
    "bf16_rows": (lambda L: _tn(L, M=15, a_dtype=L.DTYPE_BF16), 5, b"bf16 TN"),
}


@pytest.fixture()
def refusing(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a refusal that regressed would launch over fake pointers: CPU machines only")
    from elliptic_gnn_project_amd import _lib

    return lib, _lib


def test_null_params_are_refused(refusing):
    lib, _lib = refusing
    assert lib.gnn_gemm_nt_f32(None, None) == 1 and b"null params" in lib.gnn_last_error()
    assert lib.gnn_gemm_tn_f32(None, FAKE, FAKE, WS, None) == 1 and b"null params" in lib.gnn_last_error()
    assert lib.gnn_gemm_tn_f32(_tn(_lib), None, FAKE, WS, None) == 1 and b"null params" in lib.gnn_last_error()
    assert lib.gnn_gemm_tn_f32(_tn(_lib), FAKE, None, WS, None) == 4 and b"workspace" in lib.gnn_last_error()


@pytest.mark.parametrize("case", sorted(NT_REFUSALS))
def test_nt_refusal(refusing, case):
    lib, _lib = refusing
    make, status, what = NT_REFUSALS[case]
    assert lib.gnn_gemm_nt_f32(make(_lib), None) == status
    assert what in lib.gnn_last_error()


def test_nt_prep_b_refusal(refusing):
    lib, _lib = refusing  # (test_host.py: the f32-operand form); an image outside its kernel's shapes
    assert lib.gnn_gemm_nt_prep_b(_nt_img(_lib, _lib.PLANES_SPLIT_BF16, N=64, ldc=64), None) == 5
    assert b"split-image A" in lib.gnn_last_error()


@pytest.mark.parametrize("case", sorted(TN_REFUSALS))
def test_tn_refusal(refusing, case):
    lib, _lib = refusing
    make, status, what, *rest = TN_REFUSALS[case]
    ws, flags = (rest + [WS, None][len(rest):])
    p = make(_lib)
    if flags is None:
        assert lib.gnn_gemm_tn_f32(p, FAKE, FAKE, ws, None) == status
    else:
        assert lib.gnn_gemm_tn_active_f32(p, flags, FAKE, FAKE, ws, None) == status
    assert what in lib.gnn_last_error()
