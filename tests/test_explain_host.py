"""CPU: the host side of the GNNExplainer search (elliptic_gnn_project_amd/explain.py).

* ``host_mask_step`` — the float64 mirror the K16 kernel is tested against on the GPU — against torch
  float64 autograd of the loss expressions (PyG 2.5.3 GNNExplainer._loss: per-block size and entropy
  regularisers over the hard entries) plus one torch.optim.Adam step, to 1e-12.
* gnn_explain_mask_step_f32 refuses bad arguments before any launch (the library loads without a GPU),
  and header, ctypes mirror and library agree on the ABI and the params struct's layout.
* The node picker and the JSON export on hand-made artefacts.
"""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from elliptic_gnn_project_amd import explain as X

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gnnmp.h"
LIB = ROOT / "elliptic_gnn_project_amd" / "libgnnmp.so"
EPS = 1e-15


# ----------------------------------------------------------------------------- host_mask_step vs autograd
def _ent(s):
    return -s * torch.log(s + EPS) - (1 - s) * torch.log(1 - s + EPS)


def _blocks_case(gate, seed):
    """Three blocks: 0 and 1 with different hard counts, 2 without a hard entry."""
    g = torch.Generator().manual_seed(seed)
    n, Fd = 23, 5
    blk = torch.tensor([0] * 9 + [1] * 8 + [2] * 6)
    shape = (n, Fd) if gate else (n,)
    logit = 2.0 * torch.randn(shape, generator=g, dtype=torch.float64)
    logit.view(-1)[::7] = 12.0
    logit.view(-1)[3::11] = -12.0
    hard = torch.rand(shape, generator=g) < 0.6
    hard[blk == 2] = False
    hard[0] = True
    grad_src = torch.randn(shape, generator=g, dtype=torch.float64) * (torch.rand(shape, generator=g) < 0.7)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    m1 = 0.01 * torch.randn(shape, generator=g, dtype=torch.float64)
    m2 = 1e-4 * torch.rand(shape, generator=g, dtype=torch.float64)
    return blk, logit, hard, grad_src, x, m1, m2


def _scales(hard, blk, B, feature):
    cnt = torch.zeros(B, dtype=torch.float64).index_add_(0, blk, hard.reshape(hard.size(0), -1).sum(1).double())
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1), torch.zeros_like(cnt))
    if feature:
        return 1.0 * inv, 0.1 * inv
    return torch.where(cnt > 0, torch.full_like(cnt, 0.005), torch.zeros_like(cnt)), 1.0 * inv


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("epoch0", [True, False])
def test_host_mask_step_matches_autograd_and_adam(gate, epoch0):
    blk, logit, hard, gs, x, m1, m2 = _blocks_case(gate, 3)
    B, t = 3, (1 if epoch0 else 7)
    if epoch0:
        m1, m2 = torch.zeros_like(m1), torch.zeros_like(m2)
    p = logit.clone().requires_grad_(True)
    # the prediction loss stands in as <gs, h> (gate form: h = x * sigmoid(p)) or <gs, p> (plain form)
    loss = (gs * (x * p.sigmoid())).sum() if gate else (gs * p).sum()
    if not epoch0:
        for b in range(B):  # PyG's regularisers, block by block, by boolean indexing
            sel = hard & ((blk == b).view(-1, *([1] * (logit.dim() - 1))))
            if not bool(sel.any()):
                continue
            s = p[sel].sigmoid()
            if gate:
                loss = loss + 1.0 * s.mean() + 0.1 * _ent(s).mean()
            else:
                loss = loss + 0.005 * s.sum() + 1.0 * _ent(s).mean()
    loss.backward()
    opt = torch.optim.Adam([p], lr=0.01)
    if not epoch0:
        opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=m1.clone(), exp_avg_sq=m2.clone())
    want_hard = p.grad != 0
    opt.step()
    ss, es = _scales(hard, blk, B, gate)
    kw = dict(dh=gs.numpy(), x=x.numpy()) if gate else dict(grad=gs.numpy())
    if not epoch0:
        kw.update(hard=hard.numpy(), size_scale=ss.numpy(), ent_scale=es.numpy())
    got = X.host_mask_step(logit.numpy(), m1.numpy(), m2.numpy(), blk.numpy(), t, num_blocks=B, **kw)
    st = opt.state[p]
    for name, want in (("mask", p.detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])):
        err = float(np.abs(got[name] - want.numpy()).max())
        print(f"host_mask_step gate={gate} epoch0={epoch0} {name}: max abs {err:.2e}")
        assert err <= 1e-12, name
    if epoch0:
        assert np.array_equal(got["hard_out"], want_hard.numpy())
    if gate:
        assert float(np.abs(got["h"] - (x * p.detach().sigmoid()).numpy()).max()) <= 1e-12
    assert not got["skipped"].any()


def test_host_mask_step_skips_bad_blocks_and_forms_h():
    blk, logit, hard, gs, x, m1, m2 = _blocks_case(True, 4)
    blk = blk.clone()
    blk[5], blk[11] = -1, 3
    got = X.host_mask_step(logit.numpy(), m1.numpy(), m2.numpy(), blk.numpy(), 2, dh=gs.numpy(), x=x.numpy(),
                           hard=hard.numpy(), size_scale=np.ones(3), ent_scale=np.ones(3), num_blocks=3)
    for r in (5, 11):
        assert got["skipped"][r].all()
        assert np.array_equal(got["mask"][r], logit.numpy()[r]) and np.array_equal(got["exp_avg"][r], m1.numpy()[r])
    assert got["skipped"].sum() == 2 * logit.size(1) and not np.array_equal(got["mask"][0], logit.numpy()[0])
    only_h = X.host_mask_step(logit.numpy(), m1.numpy(), m2.numpy(), blk.numpy().clip(0, 2), 0, x=x.numpy(), num_blocks=3)
    assert np.array_equal(only_h["mask"], logit.numpy())
    assert np.allclose(only_h["h"], (x * logit.sigmoid()).numpy(), rtol=0, atol=1e-15)


def test_init_masks_host_mirror():
    """The documented streams: M from noise seed 2·seed over [N, F], m from 2·seed + 1 over [E, 1], keyed
    by global row / edge id (a row subset of a larger call is that call's rows)."""
    from elliptic_gnn_project_amd.robustness import host_noise

    M, m = X.host_init_masks(50, 7, 31, seed=5)
    assert M.shape == (50, 7) and m.shape == (31,)
    assert np.array_equal(M, 0.1 * host_noise(50, 7, 10))
    std = np.sqrt(2.0) * np.sqrt(2.0 / (2.0 * 50))
    assert np.array_equal(m, std * host_noise(31, 1, 11)[:, 0])
    M2, _ = X.host_init_masks(50, 7, 31, seed=6)
    assert not np.array_equal(M, M2)
    assert X.edge_init_std(50) == pytest.approx(std)


# ----------------------------------------------------------------------------- ABI and argument checks
@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        subprocess.run(["make", "-C", str(ROOT / "elliptic_gnn_project_amd" / "csrc"), "-j8"], check=True)
    from elliptic_gnn_project_amd import _lib

    return _lib.load()


def test_abi_of_the_mask_step(lib, tmp_path):
    from elliptic_gnn_project_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert int(re.search(r"#define GNNMP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gnn_abi_version()
    assert _lib.ABI_VERSION >= 31
    assert int(re.search(r"#define GNN_EXPLAIN_STATUS_BLOCK (\d+)", text).group(1)) == _lib.EXPLAIN_STATUS_BLOCK
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    fn = "gnn_explain_mask_step_f32"
    proto = re.search(r"gnn_status\s+%s\s*\((.*?)\)\s*;" % fn, text, re.S)
    assert proto and len([a for a in proto.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[fn][1]) == 2
    assert f" T {fn}\n" in exported
    # the struct: field names in the header's order, size and offsets as the C compiler lays them out
    body = text[text.index("typedef struct {\n  int64_t n;"):]
    body = body[: body.index("} gnn_explain_step_params;")]
    fields = [f for decl in re.findall(r"([^;{]+);", body) for f in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.split(None, 1)[1])]
    cls = _lib.GnnExplainStepParams
    assert [f[0] for f in cls._fields_] == fields
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
           'printf("size %zu\\n", sizeof(gnn_explain_step_params));']
    src += [f'printf("{f} %zu\\n", offsetof(gnn_explain_step_params, {f}));' for f in fields]
    src += ["return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c99", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f in fields:
        assert int(got[f]) == getattr(cls, f).offset, f


FAKE = 1 << 20


def _params(**kw):
    from elliptic_gnn_project_amd import _lib

    base = dict(n=8, F=4, mask=FAKE, ld_mask=4, dh=FAKE, ld_dh=4, x=FAKE, ld_x=4, h=FAKE, ld_h=4, exp_avg=FAKE,
                exp_avg_sq=FAKE, ld_state=4, hard=FAKE, ld_hard=4, block_of=FAKE, num_blocks=2, t=3, size_scale=FAKE,
                ent_scale=FAKE, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, status=FAKE)
    base.update(kw)
    return _lib.GnnExplainStepParams(**base)


def test_mask_step_validates_on_the_host(lib):
    """Every bad argument is refused with INVALID_ARG before any launch, and empty calls launch nothing:
    the pointers are fake, so a launch could not go unnoticed (no GPU is needed)."""
    call = lambda **kw: lib.gnn_explain_mask_step_f32(ctypes.byref(_params(**kw)), None)  # noqa: E731
    for ld in ("ld_mask", "ld_dh", "ld_x", "ld_h", "ld_state", "ld_hard"):
        assert call(**{ld: 3}) == 1, ld
        assert b"leading dimension" in lib.gnn_last_error()
    assert call(t=-1) == 1 and b"step count" in lib.gnn_last_error()
    assert call(num_blocks=0) == 1 and b"num_blocks" in lib.gnn_last_error()
    for missing in ("mask", "dh", "exp_avg", "exp_avg_sq", "block_of", "status", "size_scale", "ent_scale"):
        assert call(**{missing: None}) == 1, missing
    assert call(hard=None, hard_out=None) == 1 and b"hard_out" in lib.gnn_last_error()  # epoch 0 without hard_out
    assert call(n=-1) == 1 and call(F=-1) == 1
    assert call(t=0, h=None) == 1  # t = 0 only forms h
    plain = dict(x=None, dh=None, h=None, grad=FAKE, F=0)
    assert call(**plain, t=0) == 1
    assert call(**dict(plain, grad=None)) == 1
    assert call(**dict(plain, num_blocks=0)) == 1
    assert lib.gnn_explain_mask_step_f32(None, None) == 1
    # nothing to do: returns OK without touching the fake pointers
    assert call(n=0) == 0 and call(F=0) == 0 and call(**dict(plain, n=0)) == 0


# ----------------------------------------------------------------------------- picker and export
def _run_dir(tmp_path, scores, labels, node_ids, threshold=None):
    np.save(tmp_path / "scores_test.npy", np.asarray(scores, dtype=np.float64))
    np.save(tmp_path / "y_test.npy", np.asarray(labels))
    np.save(tmp_path / "node_idx_test.npy", np.asarray(node_ids))
    if threshold is not None:
        (tmp_path / "metrics.json").write_text(json.dumps({"threshold": threshold}))
    return tmp_path


def test_pick_nodes(tmp_path):
    ids = [40, 41, 42, 43, 44, 45]
    d = _run_dir(tmp_path, [0.95, 0.9, 0.8, 0.3, 0.85, 0.1], [0, 1, 1, 1, 0, 0], ids, threshold=0.7)
    assert X.pick_nodes(d, [43]) == [(43, {"selection": "user", "score": 0.3, "label": 1})]
    assert [v for v, _ in X.pick_nodes(d, [45, 40])] == [45, 40]
    with pytest.raises(ValueError, match="not one of the run's test nodes"):
        X.pick_nodes(d, [7])
    assert X.pick_nodes(d) == [(41, {"selection": "auto_true_positive", "score": 0.9, "label": 1})]
    top = X.pick_nodes(d, top=3)
    assert [v for v, _ in top] == [40, 41, 44] and all(s["selection"] == "top_k" for _, s in top)
    assert [v for v, _ in X.pick_nodes(d, top=10)] == [40, 41, 44, 42]  # only the predicted positives
    # no true positive above the threshold: the first false positive
    d2 = tmp_path / "fp"
    d2.mkdir()
    _run_dir(d2, [0.95, 0.2, 0.8], [0, 1, 0], [5, 6, 7], threshold=0.7)
    assert X.pick_nodes(d2) == [(5, {"selection": "auto_false_positive", "score": 0.95, "label": 0})]
    # nothing predicted positive: the highest score; without metrics.json the threshold is 0.5
    d3 = tmp_path / "hi"
    d3.mkdir()
    _run_dir(d3, [0.1, 0.4, 0.3], [1, 0, 1], [5, 6, 7])
    assert X.pick_nodes(d3) == [(6, {"selection": "auto_high_score", "score": 0.4, "label": 0})]
    assert X.pick_nodes(d3, top=2) == X.pick_nodes(d3)
    with pytest.raises(FileNotFoundError):
        X.pick_nodes(tmp_path / "fp" / "none")


def test_importance_record_names_order_and_ties():
    ei = torch.tensor([[0, 1, 2, 3, 4, 5, 6], [9, 9, 8, 8, 7, 7, 6]])
    nm = torch.zeros(3, 4)
    nm[0] = torch.tensor([0.2, 0.9, 0.2, 0.0])
    nm[2] = torch.tensor([0.2, 0.1, 0.2, 0.5])
    em = torch.tensor([0.7, 0.0, 0.7, 0.3])
    ex = X.NodeExplanation(node_id=9, n_id=torch.tensor([9, 0, 1]), e_id=torch.tensor([5, 1, 0, 3]), node_mask=nm,
                           edge_mask=em, node_hard=nm != 0, edge_hard=torch.tensor([True, False, True, True]), target=1,
                           probability_illicit=0.75)
    rec = X.importance_record(ex, ei, num_nodes=10, cfg=dict(use_time_scalar=True, time_embed_dim=0),
                              selection={"selection": "user", "score": 0.5, "label": 1})
    assert list(rec) == ["node_id", "selection", "probability_illicit", "feature_importance", "edge_importance"]
    assert rec["node_id"] == 9 and rec["probability_illicit"] == 0.75
    feats = rec["feature_importance"]
    # column sums over the subgraph divided by the FULL graph's 10 rows; the tie f0 / f2 goes to f0
    assert [f["feature"] for f in feats] == ["f1", "time_scalar", "f0", "f2"]
    assert feats[0]["importance"] == pytest.approx(1.0 / 10) and feats[2]["importance"] == pytest.approx(0.4 / 10)
    # three hard edges; the tie between edge ids 5 and 0 goes to the lower id
    assert [(e["source"], e["target"]) for e in rec["edge_importance"]] == [(0, 9), (5, 7), (3, 8)]
    assert rec["edge_importance"][0]["importance"] == pytest.approx(0.7)
    named = X.importance_record(ex, ei, 10, dict(use_time_scalar=True, time_embed_dim=4), {}, probability=0.5)
    assert [f["feature"] for f in named["feature_importance"]][1] == "f3" and named["probability_illicit"] == 0.5
    full_n, full_e = ex.to_full(10, 7)
    assert full_n.shape == (10, 4) and torch.equal(full_n[9], nm[0]) and torch.equal(full_n[1], nm[2])
    assert float(full_n.sum()) == pytest.approx(float(nm.sum()))
    assert full_e.tolist() == pytest.approx([0.7, 0.0, 0, 0.3, 0, 0.7, 0])


def test_more_than_twenty_entries_are_cut():
    nm = torch.rand(2, 30, generator=torch.Generator().manual_seed(0))
    E = 40
    ei = torch.stack([torch.arange(E), torch.arange(E) + 1])
    em = torch.rand(E, generator=torch.Generator().manual_seed(1))
    hard = torch.ones(E, dtype=torch.bool)
    ex = X.NodeExplanation(0, torch.tensor([0, 1]), torch.arange(E), nm, em, nm != 0, hard, 1, 0.5)
    rec = X.importance_record(ex, ei, 2, {}, {})
    assert len(rec["feature_importance"]) == 20 and len(rec["edge_importance"]) == 20
    imp = [e["importance"] for e in rec["edge_importance"]]
    assert imp == sorted(em.tolist(), reverse=True)[:20]
    assert [f["feature"] for f in rec["feature_importance"]][0] == f"f{int(nm.sum(0).argmax())}"
