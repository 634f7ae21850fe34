"""CPU side of test_gpu_gat_numerics: the inputs that module uses do what its tests claim, and the
float32 oracle is accurate enough on them for K * e_32 to be a meaningful bound.  Everything here
comes from the two oracle runs (float64, float32) alone; no device, no library.
"""
import time

import pytest

import gat_numerics_cases as gc

GRAD_Q = ("out", "dxh", "datt_src", "datt_dst", "dbias", "dew")
E32_GRAD_MAX = 1e-3   # the probe behind these tests measured 4e-4 at worst (scale 32, C = 1)
E32_ALPHA_MAX = 1e-5  # and 7e-6 absolute on alpha


def all_cases():
    """(kind, graph, shape, scale, slope, form) of every oracle pair the GPU module asks for."""
    for gname in gc.GRAPH_NAMES:
        for shape in gc.SHAPES:
            for slope in gc.SLOPES:
                yield "randn", gname, shape, 1, slope, "conv"
            for scale in gc.RANGE_SCALES:
                for slope in gc.RANGE_SLOPES:
                    yield "randn", gname, shape, scale, slope, "conv"
        for shape in gc.KINK_SHAPES:
            for slope in gc.KINK_SLOPES:
                yield "kink", gname, shape, 0, slope, "conv"
    for gname, shape, form in gc.EPILOGUE_CASES:
        yield "randn", gname, shape, 1, 0.5, form


def test_reference_work_is_quick():
    """Both oracle runs of every case of the GPU module, together: seconds, not minutes.  (The
    pairs are cached: the tests below, like the GPU tests, reuse them.)"""
    t0 = time.perf_counter()
    n = sum(1 for c in all_cases() if gc.oracle_pair(*c))
    dt = time.perf_counter() - t0
    print(f"{n} oracle pairs in {dt:.1f} s")
    assert dt < 60.0


def test_case_table_matches_dispatch_predicate():
    for (C, H, concat), fam in gc.SHAPES.items():
        got, v, FL = gc.gat_family(C, H, concat)
        assert got == fam, (C, H, concat)
        if fam == "narrow":  # the same shape with the narrow form off: a lane-group kernel
            got, v, FL = gc.gat_family(C, H, concat, narrow=False)
            assert got == "group"
        if got == "group":
            assert (v, FL) == gc.GEOM[(C, H, concat)]
    assert gc.gat_family(3, 2, False)[1:] == (1, 6) and gc.gat_family(130, 1, True)[1:] == (2, 65)
    # the epilogue forms: ELU + dropout and the projection keep (8, 4, T) on the lane groups and
    # (130, 1, T) on the generic kernels; explain mode always runs the generic kernels
    assert gc.gat_family(8, 4, True, post=True)[0] == "group"
    assert gc.gat_family(130, 1, True, post=True)[0] == "generic"
    assert gc.gat_family(8, 4, True, edge_w=True)[0] == gc.gat_family(4, 2, False, edge_w=True)[0] == "generic"


@pytest.mark.parametrize("gname", gc.GRAPH_NAMES)
@pytest.mark.parametrize("shape", gc.KINK_SHAPES)
def test_kink_inputs_sit_on_the_kink(gname, shape):
    inp = gc.kink_inputs(gname, *shape)
    assert inp.xh.abs().max() <= 2 and bool((inp.xh == inp.xh.round()).all())
    for a in (inp.att_src, inp.att_dst):
        assert set(a.flatten().tolist()) <= {-1.0, 0.0, 1.0}
    st = gc.score_stats(inp, 0.5)
    print(gname, shape, f"z == 0: {st.zero:.3f}  z > 0: {st.pos:.3f}  z < 0: {st.neg:.3f}")
    assert st.zero >= gc.KINK_SHARE and st.pos >= 0.1 and st.neg >= 0.1
    # integer scores: the float32 oracle takes the float64 oracle's branches, so its alpha error
    # is rounding only
    for slope in gc.KINK_SLOPES:
        _, _, e32 = gc.oracle_pair("kink", gname, shape, 0, slope)
        assert e32["alpha"] < 2.0 ** -20


@pytest.mark.parametrize("scale", gc.RANGE_SCALES)
@pytest.mark.parametrize("shape", list(gc.SHAPES))
def test_range_inputs_are_wide(shape, scale):
    """On both graphs with a hub, under every slope: some row's scores a_src[j] + a_dst[i] span more
    than 40, and the hub row's maximum softmax argument arrives after the first window (the online
    softmax has to rescale what it summed)."""
    for gname in gc.HUB_ROW:
        inp = gc.randn_inputs(gname, *shape, scale)
        for slope in gc.RANGE_SLOPES:
            st = gc.score_stats(inp, slope)
            print(gname, shape, scale, slope, f"spread z {st.spread:.1f} e {st.espread:.1f} late {st.hub_late_max}")
            assert st.spread > gc.MIN_SPREAD, (gname, slope)
            assert st.hub_late_max, (gname, slope)


def test_f32_oracle_error_keeps_the_bound_meaningful():
    worst = {}
    for case in all_cases():
        _, _, e32 = gc.oracle_pair(*case)
        for q, v in e32.items():
            if v > worst.get(q, (0.0, None))[0]:
                worst[q] = (v, case)
            assert v < (E32_ALPHA_MAX if q == "alpha" else E32_GRAD_MAX), (q, v, case)
    for q, (v, case) in worst.items():
        print(f"worst e_32 {q:9s} {v:.2e} at {case}")
