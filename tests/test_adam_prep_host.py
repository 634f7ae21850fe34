"""CPU: gnn_clip_adam_prep_f32 refuses, before any launch, whatever its row-owner blocks could not
take (include/gnnmp.h).  No device calls: the pointers below are never dereferenced."""
import ctypes
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
FAKE = 1 << 20
N, F, LD, M = 128, 166, 336, 1000
IMG_BYTES = 21 * 3 * 256 * 16 + 128 * 4  # the B image (21 k-steps) and the column scales


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    from elliptic_gnn_project_amd import _lib

    return _lib.load()


def _nt(w1=FAKE, w2=FAKE + (1 << 18)):
    """Params that select the half-pair NT: [agg | x] image of 336 columns, W1 / W2 [128, 166]."""
    from elliptic_gnn_project_amd import _lib

    p = _lib.GnnGemmNTParams()
    p.M, p.N, p.k1, p.k2 = M, N, F, F
    p.w1, p.w2, p.ldw1, p.ldw2 = w1, w2, F, F
    p.math = _lib.MATH_SPLIT_BF16
    p.a_planes, p.planes_ld, p.planes_stride, p.planes_col2 = FAKE << 4, LD, M * LD, 168
    p.planes_format, p.planes_exp = _lib.PLANES_HALF_PAIR, 3
    p.workspace, p.workspace_bytes = FAKE << 5, IMG_BYTES
    return p


def _group(extra=40_000, w1=FAKE, w2=FAKE + (1 << 18), n1=N * F):
    """[W1, bias, W2, extra]: more than 2^15 elements unless extra says otherwise."""
    from elliptic_gnn_project_amd import _lib

    g = _lib.GnnAdamGroup()
    g.lr, g.beta1, g.beta2, g.eps, g.max_norm = 1e-3, 0.9, 0.999, 1e-8, 1.0
    sizes = [(w1, n1), (FAKE << 2, N), (w2, N * F), (FAKE << 3, extra)]
    g.num_tensors = len(sizes)
    for t, (ptr, n) in zip(g.tensors, sizes):
        t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.numel = ptr, ptr + (1 << 30), ptr + (2 << 30), ptr + (3 << 30), n
    return g


def _call(lib, g, p, num=1, ws_bytes=(2 * 64 + 2) * 4):
    return lib.gnn_clip_adam_prep_f32(ctypes.byref(g), FAKE, None, FAKE, ws_bytes, ctypes.byref(p) if p is not None else None,
                                      num, None)


def test_refusals_come_before_any_launch(lib):
    from elliptic_gnn_project_amd import _lib

    assert _call(lib, _group(), None) == 1 and b"null nts" in lib.gnn_last_error()
    assert _call(lib, _group(), _nt(), num=0) == 1
    assert _call(lib, _group(), _nt(), num=5) == 1
    assert _call(lib, _group(), _nt(), ws_bytes=16) == 4  # the Adam workspace: GNN_ERR_WORKSPACE, as gnn_clip_adam_f32
    # the weight pointers are not in the group; or the tensor behind one is not [N, k]
    assert _call(lib, _group(), _nt(w1=FAKE + 64)) == 1 and b"tensors of the group" in lib.gnn_last_error()
    assert _call(lib, _group(), _nt(w2=FAKE + 64)) == 1 and b"tensors of the group" in lib.gnn_last_error()
    assert _call(lib, _group(n1=N * F - 1), _nt()) == 1 and b"tensors of the group" in lib.gnn_last_error()
    # one tensor under both halves: an element would have two owners
    assert _call(lib, _group(), _nt(w2=FAKE)) == 1 and b"tensors of the group" in lib.gnn_last_error()
    # ldw != k: the owner blocks walk contiguous rows
    p = _nt()
    p.ldw1 = F + 2
    assert _call(lib, _group(), p) == 1 and b"contiguous" in lib.gnn_last_error()
    # outside nt_h2_ok: N % 4 != 0; a split-bf16 image; f32 math
    p = _nt()
    p.N = 126
    assert _call(lib, _group(), p) == 1 and b"half-pair NT" in lib.gnn_last_error()
    p = _nt()
    p.planes_format = _lib.PLANES_SPLIT_BF16
    assert _call(lib, _group(), p) == 1 and b"half-pair NT" in lib.gnn_last_error()
    p = _nt()
    p.math = _lib.MATH_F32
    assert _call(lib, _group(), p) == 1 and b"half-pair NT" in lib.gnn_last_error()
    # the B workspace is too small, or missing
    p = _nt()
    p.workspace_bytes = IMG_BYTES - 4
    assert _call(lib, _group(), p) == 1 and b"half-pair NT" in lib.gnn_last_error()
    p.workspace, p.workspace_bytes = None, IMG_BYTES
    assert _call(lib, _group(), p) == 1
    # the one-launch form (no grad_sq_partial, <= 2^15 elements) has no row-owner blocks;
    # [W1, bias, W2] alone are 42,624 elements, so shrink the NT to N = 4
    small = _nt()
    small.N = 4
    g = _lib.GnnAdamGroup()
    g.lr, g.beta1, g.beta2, g.eps, g.max_norm = 1e-3, 0.9, 0.999, 1e-8, 1.0
    g.num_tensors = 2
    for t, (ptr, n) in zip(g.tensors, [(FAKE, 4 * F), (FAKE + (1 << 18), 4 * F)]):
        t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.numel = ptr, ptr + (1 << 30), ptr + (2 << 30), ptr + (3 << 30), n
    assert _call(lib, g, small) == 1 and b"one-launch form" in lib.gnn_last_error()
    # the NT's own validation still speaks first: a negative M
    p = _nt()
    p.M = -1
    assert _call(lib, _group(), p) == 1


def test_entry_point_is_declared_and_bound(lib):
    from elliptic_gnn_project_amd import _lib

    assert "gnn_clip_adam_prep_f32" in (ROOT / "include" / "gnnmp.h").read_text()
    assert "gnn_clip_adam_prep_f32" in _lib.SIGNATURES and lib.gnn_clip_adam_prep_f32 is not None
