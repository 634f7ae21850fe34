"""The agg half of the SAGE layer-0 image is written once per registered x and graph plan
(planes.SplitImage.mean_cached): K1 — the layer-1 mean gather — leaves the steady-state step, and
every result keeps the bits of a run with GNNMP_AGG_CACHE=0 (K1 on every forward).

SAGE 166 -> 128 -> 2 (F = 166: the half-pair image path) on 600 nodes with one hub row (degree
40: the plan has a hub form) and 20 isolated nodes."""
import pytest
import torch

from oracle import pyg_ref

pytestmark = pytest.mark.gpu

N, F = 600, 166


def _edges():
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 580, (1500,), generator=g)  # nodes 580 .. 599 stay isolated
    dst = torch.randint(0, 580, (1500,), generator=g)
    hub_src = torch.arange(100, 140)                    # node 7: 40 more in-neighbours
    ei = torch.stack([torch.cat([src, hub_src]), torch.cat([dst, torch.full((40,), 7)])])
    return ei, ei[:, 9:].contiguous()                   # the second graph: a few edges dropped


@pytest.fixture
def k1_calls(monkeypatch):
    """Launches of the layer-1 mean gather made from Python: K1 into the image, or (no image) the
    F = 166 mean aggregation."""
    from elliptic_gnn_project_amd import _lib

    calls, real = [], _lib.call

    def call(name, *args):
        if (name.startswith("gnn_sage_mean_fwd") or (name == "gnn_aggregate_f32" and args[4] == F)
                or (name == "gnn_aggregate_bf16" and args[4] in (F, F + 2))):  # bf16: x or its padded half
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", call)
    return calls


class _Run:
    def __init__(self, device, registered=True, bf16=False, layers=2):
        from elliptic_gnn_project_amd.gnn import SAGENet
        from elliptic_gnn_project_amd.planes import register_input
        from elliptic_gnn_project_amd.train_gnn import _make_loss_fn
        from elliptic_gnn_project_amd.train_ops import ClipAdam

        g = torch.Generator().manual_seed(5)
        self.x_cpu = torch.randn(N, F, generator=g)
        self.x = self.x_cpu.to(device)
        if bf16:
            self.x = self.x.to(torch.bfloat16)
        if registered:
            register_input(self.x)
        ei, ei2 = _edges()
        self.ei_cpu, self.ei2_cpu = ei, ei2
        self.ei, self.ei2 = ei.to(device), ei2.to(device)
        self.y = torch.randint(0, 2, (N,), generator=g).to(device)
        self.mask = (torch.rand(N, generator=g) < 0.6).to(device)
        torch.manual_seed(11)
        self.model = SAGENet(F, 128, layers=layers, dropout=0.0).to(device)
        self.opt = ClipAdam(self.model.parameters(), lr=0.01, weight_decay=1e-4, max_norm=1.0)
        cw = pyg_ref.class_weight(self.y[self.mask].cpu())
        self.loss_fn = _make_loss_fn({}, cw, self.model, 1, 34)
        self.denom = float(self.mask.sum())
        self.logits = None

    def forward(self):
        self.model.train()
        self.opt.zero_grad(set_to_none=False)
        self.logits = self.model(self.x, self.ei)
        return self.loss_fn.full(self.logits, self.y, self.mask, denom=self.denom)

    def step(self):
        loss = self.forward()
        loss.backward()
        out = [self.logits.detach().clone()] + [p.grad.clone() for p in self.model.parameters()]
        self.opt.step()
        return out

    def captured_step(self):
        loss = self.forward()
        loss.backward()
        self.opt.step()
        return loss

    def eval2(self):
        self.model.eval()
        with torch.no_grad():
            return self.model(self.x, self.ei2)

    def params(self):
        return [p.detach().clone() for p in self.model.parameters()]


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def _uncached(monkeypatch):
    from elliptic_gnn_project_amd import fused

    monkeypatch.setattr(fused, "_AGG_CACHE", False)  # what GNNMP_AGG_CACHE=0 sets


def test_three_steps_run_k1_once_and_keep_the_bits(device, k1_calls, monkeypatch):
    r = _Run(device)
    got = [r.step() for _ in range(3)]
    assert k1_calls == ["gnn_sage_mean_fwd_h2"]
    _uncached(monkeypatch)
    r0 = _Run(device)
    ref = [r0.step() for _ in range(3)]
    assert len(k1_calls) == 1 + 3
    for a, b in zip(got, ref):
        _same(a, b)


def test_edit_of_x_runs_k1_again(device, k1_calls, monkeypatch):
    def run(r):
        a = r.step()
        r.x.add_(0.25)  # bumps _version: the image and its agg half are rebuilt
        return a + r.step() + r.step()

    got = run(_Run(device))
    assert len(k1_calls) == 2
    _uncached(monkeypatch)
    _same(got, run(_Run(device)))
    assert len(k1_calls) == 2 + 3


def test_other_graph_between_forward_and_backward(device, k1_calls):
    r0 = _Run(device)
    r0.step()
    ref = r0.step()  # the uninterleaved second step
    k1_calls.clear()
    r = _Run(device)
    r.step()
    assert len(k1_calls) == 1
    loss = r.forward()  # plan A: a hit
    assert len(k1_calls) == 1
    r.eval2()  # plan B overwrites the agg half
    assert len(k1_calls) == 2
    loss.backward()  # the generation check refreshes plan A's means
    assert len(k1_calls) == 3
    _same([r.logits.detach()] + [p.grad for p in r.model.parameters()], ref)
    r.opt.step()
    r.forward()  # what the image holds is no longer recorded: K1 again
    assert len(k1_calls) == 4
    r.forward()
    assert len(k1_calls) == 4


def test_bf16_image_three_steps_gather_once(device, k1_calls, monkeypatch):
    """The bf16-storage layer-0 image (3 layers: every hidden NT on images) under the same rule."""
    r = _Run(device, bf16=True, layers=3)
    got = [r.step() for _ in range(3)]
    assert k1_calls == ["gnn_aggregate_bf16"]
    r.x.add_(0.25)
    got.append(r.step())
    assert len(k1_calls) == 2
    _uncached(monkeypatch)
    k1_calls.clear()
    r0 = _Run(device, bf16=True, layers=3)
    ref = [r0.step() for _ in range(3)]
    r0.x.add_(0.25)
    ref.append(r0.step())
    assert len(k1_calls) == 4
    for a, b in zip(got, ref):
        _same(a, b)


def test_unregistered_x_gathers_on_every_forward(device, k1_calls):
    r = _Run(device, registered=False)
    for i in range(3):
        r.step()
        assert len(k1_calls) == i + 1


def _eager_params(device, steps):
    r = _Run(device)
    out = []
    for _ in range(steps):
        r.step()
        out.append(r.params())
    return out


def test_captured_step_skips_k1_and_the_pin_holds(device, k1_calls):
    from elliptic_gnn_project_amd.planes import HalfPairImage, x_image
    from elliptic_gnn_project_amd.train_gnn import CapturedStep

    ref = _eager_params(device, 7)
    k1_calls.clear()
    r = _Run(device)
    cs = CapturedStep(r.captured_step, warmup=3)
    assert k1_calls == ["gnn_sage_mean_fwd_h2"]  # the first warm-up step; none recorded into the graph
    for i in range(3):
        cs()
        torch.cuda.synchronize()
        _same(r.params(), ref[3 + i])
    assert len(k1_calls) == 1
    # an evaluation over another edge_index between replays must not touch the pinned agg half:
    # it takes the f32-operand path (its own gather, no K1 into the image)
    im = x_image(r.x, HalfPairImage)
    assert im.agg_pin is not None
    params = {k: v.detach().cpu().clone() for k, v in r.model.state_dict().items()}
    logits2 = r.eval2()
    assert k1_calls[1:] == ["gnn_aggregate_f32"]
    oracle = pyg_ref.model_forward("sage", params, r.x_cpu, r.ei2_cpu, layers=2)
    assert float((logits2.cpu().double() - oracle.double()).abs().max()) <= 1e-5
    cs()
    torch.cuda.synchronize()
    _same(r.params(), ref[6])


def test_capture_on_a_cold_cache(device, k1_calls, monkeypatch):
    from elliptic_gnn_project_amd import fused
    from elliptic_gnn_project_amd.planes import HalfPairImage, x_image
    from elliptic_gnn_project_amd.train_gnn import CapturedStep

    ref = _eager_params(device, 4)
    k1_calls.clear()
    r = _Run(device)
    # one warm-up step builds what a capture cannot (the plan, x's planes, the optimizer state) —
    # on a side stream, as every capture of a backward needs (CapturedStep's own warm-up does the
    # same) — and, with the cache switched off for it, records nothing of the agg half
    monkeypatch.setattr(fused, "_AGG_CACHE", False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r.step()
    r.logits = None  # no autograd graph of the warm-up outlives it
    torch.cuda.current_stream().wait_stream(side)
    monkeypatch.setattr(fused, "_AGG_CACHE", True)
    im = x_image(r.x, HalfPairImage)
    assert len(k1_calls) == 1 and im.agg_key is None
    cs = CapturedStep(r.captured_step, warmup=0)  # K1 is recorded into the graph: it has not run
    assert len(k1_calls) == 2
    assert im.agg_key is None and im.agg_pin is None
    r.model.eval()
    with torch.no_grad():
        e0 = r.model(r.x, r.ei)  # before the first replay: nothing to reuse
        assert len(k1_calls) == 3
        e1 = r.model(r.x, r.ei)  # replays rewrite the agg half unseen: the image stays uncached
        assert len(k1_calls) == 4
    assert torch.equal(e0, e1)
    for i in range(3):
        cs()
        torch.cuda.synchronize()
        _same(r.params(), ref[1 + i])
