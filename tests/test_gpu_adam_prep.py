"""The half-pair NT's B image built inside the clip + Adam launch (gnn_clip_adam_prep_f32): extra
blocks own the rows of the NT's weights, update them exactly as gnn_clip_adam_f32 does and write
the image gnn_gemm_nt_prep_b would write for the updated weights.

Kernel level: every comparison is bit for bit against the two existing entry points.  The group is
[W1 [Nc, k1], bias [Nc], W2 [Nc, k2], extra]: bias and extra stay in the flat 64-block partition
(extra makes the group larger than the one-launch form's 2^15 elements at every shape).
Step level (2-layer fused SAGE on the 600-node fixture): GNNMP_ADAM_PREP 0 against 1."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 33          # NT rows: two 32-row tiles, the second partial
EXTRA = 40_000  # > 2^15: never the one-launch form
NB = 7          # blocks of the synthetic folded partials

# (Nc, k1, k2): the headline's weights; dead columns 120 .. 127; the smallest w2-absent shape
# nt_h2_ok takes (N % 4 == 0, k1 >= 1, an x-only image of 176 columns)
SHAPES = [(128, 166, 166), (120, 166, 166), (4, 1, 0)]
# (clip active, weight decay, one inf gradient under skip_nonfinite)
CASES = {"clip_wd0": (True, 0.0, False), "noclip_wd": (False, 1e-2, False), "inf_skip": (True, 1e-2, True)}


def _image(Nc, k1, k2, device, g):
    """A half-pair image of M rows for an NT with these weights: [agg | x], or x alone."""
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.planes import HalfPairImage, X_ONLY_LD, h2_exp

    if k2:
        x = torch.randn(M, k2, generator=g).to(device)
        agg = (torch.randn(M, k1, generator=g) * 0.7).to(device)
        im = HalfPairImage(M, k1, k2, device)
        im.fill_x(x)
        _lib.call("gnn_split_h2_f32", agg.data_ptr(), k1, M, k1, im.ptr, im.ld, im.ps, 0, im.col2, im.exp,
                  _lib.stream_handle(device))
        return im, (agg, x)
    x = torch.randn(M, k1, generator=g).to(device)
    im = HalfPairImage(M, k1, 0, device, X_ONLY_LD)
    im.exp = h2_exp(x)
    _lib.call("gnn_split_h2_f32", x.data_ptr(), k1, M, k1, im.ptr, im.ld, im.ps, 0, im.ld, im.exp,
              _lib.stream_handle(device))
    return im, (x,)


def _state(Nc, k1, k2, inf, g, device):
    """p, g, m, v of the group, with the rows the image is sensitive to: row 1 all zero and never
    moving (zero gradient and momentum: column scale 1), row 2 spanning 1e-6 .. 1e3 (held still
    the same way, so the span survives the update)."""
    shapes = [(Nc, k1), (Nc,)] + ([(Nc, k2)] if k2 else []) + [(EXTRA,)]
    P = [torch.randn(*s, generator=g) * 0.08 for s in shapes]
    P[1] = P[1].abs() + 0.05  # a positive bias: the NT's ReLU output is not all zero at any shape
    G = [torch.randn(*s, generator=g) * 0.05 for s in shapes]
    Mo = [torch.randn(*s, generator=g) * 0.01 for s in shapes]
    V = [torch.rand(*s, generator=g) * 1e-3 for s in shapes]
    for j in [0, 2] if k2 else [0]:
        k = shapes[j][1]
        P[j][1].zero_()
        sign = torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0)
        P[j][2] = torch.logspace(-6, 3, k) * sign if k > 1 else torch.tensor([1e-6])
        for r in (1, 2):
            G[j][r].zero_()
            Mo[j][r].zero_()
    if inf:
        G[0][Nc - 1, k1 - 1] = float("inf")  # in a row-owner block's rows
    return [[t.to(device).contiguous() for t in L] for L in (P, G, Mo, V)]


def _group(state, clip, wd, skip, partials):
    from elliptic_gnn_project_amd import _lib

    P, G, Mo, V = state
    grp = _lib.GnnAdamGroup()
    grp.num_tensors = len(P)
    grp.lr, grp.beta1, grp.beta2, grp.eps, grp.weight_decay = 0.003, 0.9, 0.999, 1e-8, wd
    grp.max_norm = 1.0
    grp.skip_nonfinite = int(skip)
    for j in range(len(P)):
        t = grp.tensors[j]
        t.param, t.grad, t.exp_avg, t.exp_avg_sq = (x[j].data_ptr() for x in (P, G, Mo, V))
        t.numel = P[j].numel()
    if partials is not None:
        grp.grad_sq_partial, grp.grad_sq_nblk = partials.data_ptr(), NB
    return grp


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("form", ["folded", "two_launch"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_riding_prep_equals_adam_then_prep(device, shape, form, case):
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.fused import _nt_workspace, gemm_nt

    Nc, k1, k2 = shape
    clip, wd, inf = CASES[case]
    g = torch.Generator().manual_seed(1000 * Nc + k1)
    im, a_ops = _image(Nc, k1, k2, device, g)
    ref = _state(Nc, k1, k2, inf, g, device)
    if not clip:  # a norm below max_norm = 1: the two-launch form sums these gradients itself
        for t in ref[1]:
            t.mul_(1e-3)
    got = [[t.clone() for t in L] for L in ref]
    partials = None
    if form == "folded":  # the TN reduce's layout: NB partials of Σg², NB non-finite counts, the step count
        partials = torch.zeros(2 * NB + 1)
        partials[:NB] = torch.rand(NB, generator=g) * (4.0 if clip else 1e-3)
        partials[NB + 2] = 1.0 if inf else 0.0
        partials[2 * NB] = 3.0
        partials = partials.to(device)
    step = [torch.full((1,), 3.0, device=device) for _ in range(2)]
    norm = [torch.zeros(1, device=device) for _ in range(2)]
    aws = [torch.zeros(2 * 64 + 2, device=device) for _ in range(2)]
    bias = ref[0][1]
    proj = torch.randn(4, Nc, generator=g).to(device)

    def nt_kw(st, z):
        return dict(w1=st[0][0], w2=st[0][2] if k2 else None, bias=bias, relu=True, proj=proj, z=z)

    # reference: gnn_clip_adam_f32, then the standalone prep and an NT over the updated weights
    _lib.call("gnn_clip_adam_f32", _group(ref, clip, wd, inf, partials), step[0].data_ptr(), norm[0].data_ptr(),
              aws[0].data_ptr(), aws[0].numel() * 4, _lib.stream_handle(device))
    ws_ref = _nt_workspace(device, Nc, im.k1, im.k2).zero_()
    z_ref = torch.zeros(M, 4, device=device)
    assert gemm_nt(None, None, Nc, planes=im, check_planes=True, **nt_kw(ref, z_ref))
    gemm_nt(None, None, Nc, planes=im, workspace=ws_ref, b_stage="prep", **nt_kw(ref, z_ref))
    c_ref = gemm_nt(None, None, Nc, planes=im, **nt_kw(ref, z_ref))  # the NT with its own prep

    ws = torch.zeros_like(ws_ref)
    z = torch.zeros(M, 4, device=device)
    prm = gemm_nt(None, None, Nc, planes=im, workspace=ws, b_stage="params", **nt_kw(got, z))
    _lib.call("gnn_clip_adam_prep_f32", _group(got, clip, wd, inf, partials), step[1].data_ptr(), norm[1].data_ptr(),
              aws[1].data_ptr(), aws[1].numel() * 4, ctypes.byref(prm), 1, _lib.stream_handle(device))
    # (a) the update
    names = ("param", "grad", "exp_avg", "exp_avg_sq")
    for name, A, B in zip(names, ref, got):
        for j, (a, b) in enumerate(zip(A, B)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, j)
    assert torch.equal(step[0], step[1]) and float(step[0]) == (3.0 if inf else 4.0)
    assert norm[0].view(torch.int32).equal(norm[1].view(torch.int32))
    # (b) the image and the column scales: the workspace words, all of them
    assert torch.equal(ws.view(torch.int32), ws_ref.view(torch.int32))
    # (c) the NT over the riding image
    c = gemm_nt(None, None, Nc, planes=im, workspace=ws, b_stage="ready", **nt_kw(got, z))
    assert torch.equal(c, c_ref) and torch.equal(z, z_ref)
    # ... and both are the product: the half-pair NT's bound against float64 (test_gpu_h2.py)
    A = torch.cat([t.double().cpu() for t in a_ops], 1)
    W = torch.cat([ref[0][0].double().cpu()] + ([ref[0][2].double().cpu()] if k2 else []), 1)
    want = torch.relu(A @ W.t() + bias.double().cpu())
    assert float(want.norm()) > 0
    assert float((c.double().cpu() - want).norm() / want.norm()) < 1e-6


def test_skipped_step_leaves_weights_and_builds_their_image(device):
    """One inf gradient under skip_nonfinite: no parameter, moment, gradient or step count moves,
    and the workspace holds the image of the unchanged weights."""
    from elliptic_gnn_project_amd import _lib
    from elliptic_gnn_project_amd.fused import _nt_workspace, gemm_nt

    Nc, k1, k2 = 120, 166, 166
    g = torch.Generator().manual_seed(77)
    im, _ = _image(Nc, k1, k2, device, g)
    st = _state(Nc, k1, k2, True, g, device)
    before = [[t.clone() for t in L] for L in st]
    step, norm, aws = torch.full((1,), 5.0, device=device), torch.zeros(1, device=device), torch.zeros(130, device=device)
    kw = dict(w1=st[0][0], w2=st[0][2], bias=st[0][1], relu=True)
    ws = _nt_workspace(device, Nc, im.k1, im.k2).zero_()
    prm = gemm_nt(None, None, Nc, planes=im, workspace=ws, b_stage="params", **kw)
    _lib.call("gnn_clip_adam_prep_f32", _group(st, True, 1e-2, True, None), step.data_ptr(), norm.data_ptr(),
              aws.data_ptr(), aws.numel() * 4, ctypes.byref(prm), 1, _lib.stream_handle(device))
    for A, B in zip(before, st):
        for a, b in zip(A, B):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(step) == 5.0
    ws_ref = torch.zeros_like(ws)
    gemm_nt(None, None, Nc, planes=im, workspace=ws_ref, b_stage="prep", **kw)
    assert torch.equal(ws.view(torch.int32), ws_ref.view(torch.int32))


# ------------------------------------------------------------------------------- step level
GOLD = Path(__file__).resolve().parent / "golden" / "elliptic600.npz"


@pytest.fixture
def lib_calls(monkeypatch):
    """The names of the libgnnmp calls made from Python, in order."""
    from elliptic_gnn_project_amd import _lib

    calls, real = [], _lib.call

    def call(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", call)
    return calls


class _Run:
    """2-layer fused SAGE (166 -> 128 -> 2) on the 600-node fixture, registered x, ClipAdam."""

    def __init__(self, device, seed=11):
        from elliptic_gnn_project_amd.gnn import SAGENet
        from elliptic_gnn_project_amd.planes import register_input
        from elliptic_gnn_project_amd.train_gnn import _make_loss_fn
        from elliptic_gnn_project_amd.train_ops import ClipAdam
        from oracle import pyg_ref

        with np.load(GOLD) as z:
            self.x = register_input(torch.from_numpy(z["x"]).to(device))
            self.ei = torch.from_numpy(z["edge_index"]).to(device)
        g = torch.Generator().manual_seed(5)
        n = self.x.size(0)
        self.y = torch.randint(0, 2, (n,), generator=g).to(device)
        self.mask = (torch.rand(n, generator=g) < 0.6).to(device)
        torch.manual_seed(seed)
        self.model = SAGENet(self.x.size(1), 128, layers=2, dropout=0.0).to(device)
        self.opt = ClipAdam(self.model.parameters(), lr=0.01, weight_decay=1e-4, max_norm=1.0)
        self.loss_fn = _make_loss_fn({}, pyg_ref.class_weight(self.y[self.mask].cpu()), self.model, 1, 34)
        self.denom = float(self.mask.sum())
        self.logits = None

    def step(self):
        self.model.train()
        self.opt.zero_grad(set_to_none=False)
        self.logits = self.model(self.x, self.ei)
        loss = self.loss_fn.full(self.logits, self.y, self.mask, denom=self.denom)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def snap(self, loss):
        return [loss.clone(), self.logits.detach().clone()] + [p.detach().clone() for p in self.model.parameters()]

    def other_state(self):
        g = torch.Generator().manual_seed(99)
        return {k: torch.randn(v.shape, generator=g) * 0.05 for k, v in self.model.state_dict().items()}


def _same(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i


def _trace(device, monkeypatch, switch, captured):
    """5 steps (eager, or replays of a CapturedStep), then other weights loaded and 2 more, then an
    eager step with the switch off (ClipAdam writes the weights and builds no image) and one more."""
    from elliptic_gnn_project_amd.train_gnn import CapturedStep

    monkeypatch.setenv("GNNMP_ADAM_PREP", switch)
    r = _Run(device)
    step = CapturedStep(r.step, warmup=2) if captured else r.step
    out = []
    for _ in range(5):
        out.append(r.snap(step()))
    r.model.load_state_dict(r.other_state())  # copies in place: the weights' _version moves
    for _ in range(2):
        out.append(r.snap(step()))
    monkeypatch.setenv("GNNMP_ADAM_PREP", "0")
    out.append(r.snap(r.step()))
    monkeypatch.setenv("GNNMP_ADAM_PREP", switch)
    out.append(r.snap(step()))
    return r, out


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_steps_keep_the_bits_of_the_switch_off_path(device, monkeypatch, lib_calls, captured):
    _, ref = _trace(device, monkeypatch, "0", captured)
    assert "gnn_clip_adam_prep_f32" not in lib_calls
    del lib_calls[:]
    r, got = _trace(device, monkeypatch, "1", captured)
    for a, b in zip(got, ref):
        _same(a, b)
    assert r.opt.last_prep == (not captured)  # (captured: the last call from Python was the eager switch-off step)
    preps = [i for i, c in enumerate(lib_calls) if c == "gnn_gemm_nt_prep_b"]
    adams = [i for i, c in enumerate(lib_calls) if c.startswith("gnn_clip_adam") and c.endswith("_f32")]
    assert [lib_calls[i] for i in adams].count("gnn_clip_adam_f32") == 1  # the step with the switch off
    if captured:  # the only standalone preps: the replay guard's, after load_state_dict and after the eager step
        assert len(preps) == 2 and preps[0] > adams[-2] and preps[1] > adams[-1]
    else:  # an eager NT call launches its own prep inside gnn_gemm_nt_f32 (b_ready = 0): none standalone
        assert not preps


def test_ready_only_with_a_valid_tag(device, monkeypatch):
    """The forward passes b_ready only for the weights, image and workspace the last optimizer
    launch built the image from: not on a first step, not after load_state_dict, not after x is
    registered anew, not after a step with the switch off."""
    from elliptic_gnn_project_amd import _lib, fused
    from elliptic_gnn_project_amd.planes import register_input

    monkeypatch.setattr(fused, "_K1_PREP", False)  # K1 (a first forward over an image) carries no prep here
    ready, real = [], _lib.call

    def call(name, *args):
        if name == "gnn_gemm_nt_f32" and args[0].a_planes and args[0].N == 128:
            ready.append(int(args[0].b_ready))
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setenv("GNNMP_ADAM_PREP", "1")
    r = _Run(device)
    r.step(), r.step(), r.step()
    assert ready == [0, 1, 1]
    r.model.load_state_dict(r.other_state())
    r.step(), r.step()
    assert ready[3:] == [0, 1]
    r.x = register_input(r.x.clone())  # another x: another image, another workspace
    r.step(), r.step()
    assert ready[5:] == [0, 1]
    monkeypatch.setenv("GNNMP_ADAM_PREP", "0")
    r.step()
    monkeypatch.setenv("GNNMP_ADAM_PREP", "1")
    r.step(), r.step()
    assert ready[7:] == [0, 0, 1]
