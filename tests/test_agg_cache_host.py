"""Host logic of the layer-0 image's cached agg half (planes.SplitImage.mean_cached,
fused._layer0_image), with the library call stubbed out: when K1 is skipped, when it runs, what is
recorded under stream capture, and what a captured step that relied on the cache pins."""
import pytest
import torch


class _Plan:
    """What fill_mean reads of a GraphPlan."""

    def __init__(self, n):
        self.c_graph = None
        self.deg = torch.ones(n)
        self.hub = None
        self.num_nodes, self.num_slots = n, 0


@pytest.fixture
def stub(monkeypatch):
    from elliptic_gnn_project_amd import _lib, planes

    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(_lib, "stream_handle", lambda dev=None: 0)
    state = {"capturing": False}
    monkeypatch.setattr(planes, "_capturing", lambda: state["capturing"])
    return calls, state


def _image(n=40, f=166):
    from elliptic_gnn_project_amd.planes import HalfPairImage, register_input

    x = register_input(torch.randn(n, f))
    im = HalfPairImage(n, f, f, x.device)
    im.x_key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()))
    return im, x


K1 = "gnn_sage_mean_fwd_h2"


def test_same_key_skips_and_each_key_part_fills(stub):
    calls, _ = stub
    im, x = _image()
    pa, pb = _Plan(40), _Plan(40)
    assert im.mean_cached(pa, x) == (1, False) and calls == [K1]
    assert im.mean_cached(pa, x) == (1, True) and calls == [K1]  # same key: no launch, same generation
    # plan identity
    assert im.mean_cached(pb, x) == (2, False)
    assert im.mean_cached(pb, x) == (2, True)
    # hub flag
    assert im.mean_cached(pb, x, hub=False) == (3, False)
    assert im.mean_cached(pb, x, hub=False) == (3, True)
    # exp
    im.exp = 3
    assert im.mean_cached(pb, x, hub=False) == (4, False)
    # x version (the image key x_image refreshes)
    im.x_key = im.x_key[:1] + (im.x_key[1] + 1,) + im.x_key[2:]
    assert im.mean_cached(pb, x, hub=False) == (5, False)
    assert im.mean_cached(pb, x, hub=False) == (5, True)
    assert calls == [K1] * 5


def test_no_skip_for_keep_bits_unregistered_or_switched_off(stub):
    calls, _ = stub
    im, x = _image()
    p = _Plan(40)
    im.mean_cached(p, x)
    kb = torch.zeros(40, 4, dtype=torch.int32)
    assert im.mean_cached(p, x, keep=(kb, 128, 0.5, 1, None))[1] is False  # K1 writes the keep bits
    assert im.mean_cached(p, x)[1] is True  # ... and the same means: still recorded
    assert im.mean_cached(p, x, cache=False)[1] is False
    assert im.agg_key is None and im.mean_cached(p, x, cache=False)[1] is False  # nothing recorded
    y = torch.randn(40, 166)  # not registered
    im.x_key = (y.data_ptr(), y._version, tuple(y.shape), tuple(y.stride()))
    assert im.mean_cached(p, y)[1] is False and im.mean_cached(p, y)[1] is False


def test_a_direct_fill_forgets_the_key(stub):
    im, x = _image()
    pa, pb = _Plan(40), _Plan(40)
    im.mean_cached(pa, x)
    im.fill_mean(pb, x)  # e.g. a backward refreshing the image: the cache no longer knows the content
    assert im.agg_key is None
    assert im.mean_cached(pa, x)[1] is False


def test_a_dead_plan_never_matches(stub):
    im, x = _image()
    p = _Plan(40)
    im.mean_cached(p, x)
    del p
    assert im.mean_cached(_Plan(40), x)[1] is False


def test_capturing_records_no_key_and_disables_the_cache(stub):
    calls, state = stub
    im, x = _image()
    p = _Plan(40)
    state["capturing"] = True
    assert im.mean_cached(p, x)[1] is False  # cold cache under capture: K1 is captured ...
    assert im.agg_key is None and im.agg_pin is None  # ... it has not run: nothing recorded
    state["capturing"] = False
    assert im.mean_cached(p, x)[1] is False  # an eager forward before the first replay runs K1
    assert im.mean_cached(p, x)[1] is False  # replays rewrite the agg half unseen: stays uncached
    assert calls == [K1] * 3


def test_captured_hit_pins_the_key(stub, monkeypatch):
    from elliptic_gnn_project_amd import fused, planes

    calls, state = stub
    im, x = _image()
    pa, pb = _Plan(40), _Plan(40)
    im.mean_cached(pa, x)
    state["capturing"] = True
    assert im.mean_cached(pa, x)[1] is True and calls == [K1]
    state["capturing"] = False
    assert im.agg_pin is not None and not im.agg_foreign(pa) and im.agg_foreign(pb) and im.agg_foreign(pa, hub=False)
    # _layer0_image: no image for a foreign plan (the f32-operand path), the image for the pinned one
    monkeypatch.setattr(fused, "mean_planes_ok", lambda t: True)
    monkeypatch.setattr(fused, "h2_ok", lambda t: True)
    monkeypatch.setattr(fused, "x_image", lambda t, cls=None: im)
    monkeypatch.setattr(fused, "gemm_nt", lambda *a, **k: True)
    assert fused._layer0_image(x, 128, {}, h2=True, plan=pb) is None
    assert fused._layer0_image(x, 128, {}, h2=True, plan=pa) is im
    assert fused._layer0_image(x, 128, {}, h2=True) is im  # no plan given: as before
    # x edited: planes.x_image rebuilds the image and unpins it
    im.agg_reset()
    assert im.agg_pin is None and im.agg_key is None
    assert fused._layer0_image(x, 128, {}, h2=True, plan=pb) is im
    assert planes.SplitImage._same_key(None, im.agg_key_of(pa)) is False


def test_bf16_image_follows_the_same_rules(stub):
    from elliptic_gnn_project_amd.planes import BfImage, register_input

    _, state = stub
    x = register_input(torch.randn(40, 166).to(torch.bfloat16))
    im = BfImage(40, 166, 166, x.device, zero=True)
    im.x_key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()))
    fills = []
    pa, pb = _Plan(40), _Plan(40)
    assert im.mean_cached(pa, x, lambda: fills.append("a")) is False
    assert im.mean_cached(pa, x, lambda: fills.append("a")) is True
    assert im.mean_cached(pb, x, lambda: fills.append("b")) is False
    assert im.mean_cached(pb, x, lambda: fills.append("b"), cache=False) is False
    assert im.mean_cached(pb, x, lambda: fills.append("b")) is False  # the uncached fill forgot the key
    assert fills == ["a", "b", "b", "b"]
    state["capturing"] = True
    assert im.mean_cached(pb, x, lambda: fills.append("b")) is True  # a captured hit pins plan b
    state["capturing"] = False
    assert im.agg_foreign(pa) and not im.agg_foreign(pb)
    im.agg_reset()
    state["capturing"] = True
    assert im.mean_cached(pa, x, lambda: fills.append("a")) is False  # a captured fill: volatile from here on
    state["capturing"] = False
    assert im.agg_volatile and im.mean_cached(pa, x, lambda: fills.append("a")) is False
