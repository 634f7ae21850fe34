"""CPU: the host side of the fused loss variants (include/gnnmp.h gnn_ce_spec, ABI 27) — which
configurations of ``_make_loss_fn`` are fusable, the cached per-node time weights against the
reference's own expressions (src/train_gnn.py:166-173) bit for bit, the ctypes mirror of the spec
struct, the ``_spec`` symbols and the argument checks the library makes before any device work."""
import ctypes
import subprocess
from pathlib import Path

import pytest
import torch

from elliptic_gnn_project_amd.train_gnn import _make_loss_fn

from test_loss_golden import CASES

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gnnmp.h"
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
SPEC_SYMBOLS = ("gnn_masked_ce_spec_f32", "gnn_sage_out_mean_ce_spec_f32", "gnn_gcn_out_ce_spec_f32",
                "gnn_gat_out_ce_spec_f32")


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():  # a fresh checkout: build it (hipcc cross-compiles gfx950 without a GPU)
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    from elliptic_gnn_project_amd import _lib

    return _lib.load()


def _fn(cfg):
    return _make_loss_fn(cfg, torch.tensor([0.6, 2.5]), torch.nn.Module(), 1, 34)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plain_unchanged_and_every_golden_case_fusable(name):
    cfg = CASES[name][0]
    fn = _fn(cfg)
    plain = (not cfg.get("focal_loss", False) and cfg.get("time_loss_weighting", "none") == "none"
             and cfg.get("time_embed_l2", 0.0) == 0.0)
    assert fn.plain == plain
    assert fn.plain == (name == "ce_weighted")
    assert fn.fusable


def test_focal_gamma_below_one_keeps_the_torch_loss():
    fn = _fn(dict(focal_loss=True, focal_gamma=0.5))
    assert not fn.plain and not fn.fusable
    assert _fn(dict(focal_loss=True, focal_gamma=1.0)).fusable
    assert _fn(dict(focal_loss=True, focal_gamma=1.5, time_loss_weighting="sqrt", time_embed_l2=1e-4)).fusable
    assert not _fn(dict(time_loss_weighting="cubic")).fusable  # loss_fn raises on it, as the reference does


@pytest.mark.parametrize("scheme", ["linear", "sqrt"])
def test_cached_row_weights_are_the_reference_expression(scheme):
    """The weights of all nodes, built once, hold on the selected rows exactly the bits the
    reference computes from those rows' timesteps — t < t_min and t > t_max included (the
    clamps), t = t_min too (the 1e-3 floor)."""
    t_min, t_max = 5, 34
    fn = _make_loss_fn(dict(time_loss_weighting=scheme), torch.tensor([1.0, 1.0]), torch.nn.Module(), t_min, t_max)
    g = torch.Generator().manual_seed(3)
    t_all = torch.cat([torch.tensor([1, 4, 5, 6, 34, 35, 49]), torch.randint(1, 50, (500,), generator=g)])
    idx = torch.cat([torch.arange(7), torch.randperm(500, generator=g)[:200] + 7])
    rw = fn.row_weights(t_all)
    assert rw.dtype == torch.float32 and rw.shape == t_all.shape
    t_sel = t_all.index_select(0, idx)
    ref = (t_sel.float() - float(t_min)) / max(float(t_max - t_min), 1.0)  # src/train_gnn.py:116-121
    if scheme == "sqrt":
        ref = torch.sqrt(torch.clamp(ref, min=0.0))
    ref = torch.clamp(ref, min=1e-3)
    assert torch.equal(rw.index_select(0, idx), ref)
    assert float(rw[0]) == float(rw[2]) == float(torch.tensor(1e-3))  # below and at t_min: the floor
    assert float(rw[5]) > 1.0  # past t_max: not clamped from above, as in the reference
    assert fn.row_weights(t_all) is rw  # cached per (tensor, version)
    t_all[3] = 20
    rw2 = fn.row_weights(t_all)  # an in-place edit bumps the version: rebuilt
    assert rw2 is not rw and float(rw2[3]) != float(rw[3])


def test_ce_operands_carry_the_variant():
    """The plain loss keeps its five operands (and its key); a variant appends its field and
    extends the key, so a forward's precomputed CE is never taken for another variant's."""
    from elliptic_gnn_project_amd.train_ops import _ce_operands

    y = torch.zeros(8, dtype=torch.long)
    m = torch.ones(8, dtype=torch.bool)
    w = torch.ones(2)
    rw = torch.rand(8)
    plain = _ce_operands(y, m, w, 4.0, "cpu")
    assert len(plain) == 5
    v1 = _ce_operands(y, m, w, 4.0, "cpu", row_w=rw)
    v2 = _ce_operands(y, m, w, 4.0, "cpu", focal_gamma=2.0)
    v3 = _ce_operands(y, m, w, 4.0, "cpu", defer=False)
    assert len(v1) == len(v2) == len(v3) == 6
    assert len({plain[0], v1[0], v2[0], v3[0]}) == 4
    assert v1[0][:4] == plain[0] and v1[5][0] is rw and v2[5][1] == 2.0 and v3[5] == (None, None, False)
    with pytest.raises(ValueError, match="focal_gamma >= 1"):
        _ce_operands(y, m, w, 4.0, "cpu", focal_gamma=0.5)
    with pytest.raises(ValueError, match="one weight per row"):
        _ce_operands(y, m, w, 4.0, "cpu", row_w=torch.rand(7))


def test_ce_spec_struct_layout_matches_c(tmp_path):
    from elliptic_gnn_project_amd import _lib

    fields = ["y", "mask", "class_w", "row_w", "inv_denom", "focal", "focal_gamma", "reserved"]
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
           'printf("size %zu\\n", sizeof(gnn_ce_spec));']
    src += [f'printf("{f} %zu\\n", offsetof(gnn_ce_spec, {f}));' for f in fields]
    src += ["return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    cls = _lib.GnnCeSpec
    assert [f[0] for f in cls._fields_] == fields
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f in fields:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_spec_symbols_resolve_and_abi(lib):
    from elliptic_gnn_project_amd import _lib

    assert _lib.ABI_VERSION >= 27 and lib.gnn_abi_version() == _lib.ABI_VERSION
    for name in SPEC_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None


def test_library_rejects_focal_gamma_below_one(lib):
    """Refused on the host with a message, before any device work (no GPU here): every pointer is a
    dummy the call never reads."""
    from elliptic_gnn_project_amd import _lib

    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    sp = _lib.GnnCeSpec()
    sp.y = sp.mask = sp.class_w = p
    sp.inv_denom, sp.focal, sp.focal_gamma = 1.0, 1, 0.5
    assert lib.gnn_masked_ce_spec_f32(4, 2, p, 2, sp, p, 2, p, p, 64 * 4, None, None) == 1
    assert b"focal_gamma" in lib.gnn_last_error()
    g = _lib.GnnGraph()
    assert lib.gnn_sage_out_mean_ce_spec_f32(g, p, p, 4, 2, None, p, 2, sp, p, 2, None, 0, None, p, p, 256, None) == 1
    assert b"focal_gamma" in lib.gnn_last_error()
    assert lib.gnn_gcn_out_ce_spec_f32(g, p, p, 2, 2, None, p, 2, sp, p, 2, None, p, p, 256, None) == 1
    assert b"focal_gamma" in lib.gnn_last_error()
    sp.focal_gamma = float("nan")
    assert lib.gnn_masked_ce_spec_f32(4, 2, p, 2, sp, p, 2, p, p, 64 * 4, None, None) == 1
    assert lib.gnn_masked_ce_spec_f32(4, 2, p, 2, None, p, 2, p, p, 64 * 4, None, None) == 1
    sp.focal, sp.focal_gamma = 0, 0.0  # (gamma is not read without focal) the wrapped entry's C limit holds
    assert lib.gnn_masked_ce_spec_f32(4, 17, p, 17, sp, p, 17, p, p, 64 * 4, None, None) == 1
