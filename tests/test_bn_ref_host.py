"""CPU: tests/bn_ref.py, the float64 reference the K12 geometry tests (test_gpu_bn_geometry.py) stand on.

The reference equals float64 nn.BatchNorm1d + autograd with the same keep mask (one and two shards,
both momentum modes) to 1e-12; its Python geometry equals hand-computed values of csrc/bn.hip's; the
conditions on the inputs hold at every case of the table (tie window, integer probes); and the
checkers have teeth: a float32 emulation of the kernel formulas passes them, and the same emulation
with one row dropped from a sum, the other shard's n, or the mask index shifted by one does not.
"""
import numpy as np
import pytest
import torch

import bn_ref
from oracle.dropout_hash import keep_mask

SHAPES = [(2, 3), (33, 64), (17, 100), (9, 257), (2049, 1)]
CLOSE = dict(rtol=1e-12, atol=1e-12)


def _torch_ref(a, p, seed, momentum, nbt0, split=None):
    """float64 nn.BatchNorm1d + autograd over the whole batch; masks numbered per shard."""
    N, C = a.z.shape
    bn = torch.nn.BatchNorm1d(C, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.copy_(a.w)
        bn.bias.copy_(a.b)
        bn.running_mean.copy_(a.rm)
        bn.running_var.copy_(a.rv)
        bn.num_batches_tracked.fill_(nbt0)
    z = a.z.double().requires_grad_(True)
    parts = [N] if split is None else [split, N - split]
    keep = torch.cat([torch.from_numpy(keep_mask(seed, n, C, p)) for n in parts]).double() if p > 0 else 1.0
    out = torch.relu(bn(z)) * keep * bn_ref.drop_scale(p) + a.r.double()
    out.backward(a.dh.double())
    return bn, out.detach(), z.grad


@pytest.mark.parametrize("N,C", SHAPES)
@pytest.mark.parametrize("momentum,nbt0", [(0.1, 0), (None, 2)])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_reference_is_float64_batchnorm(N, C, momentum, nbt0, p):
    a = bn_ref.make_inputs(N, C)
    bn, out, dz = _torch_ref(a, p, 99, momentum, nbt0)
    ref = bn_ref.tail(a.z, a.r, a.w, a.b, p, 99, a.dh)
    torch.testing.assert_close(ref.out, out, **CLOSE)
    torch.testing.assert_close(ref.dz, dz, **CLOSE)
    torch.testing.assert_close(ref.dweight, bn.weight.grad, **CLOSE)
    torch.testing.assert_close(ref.dbias, bn.bias.grad, **CLOSE)
    rm, rv, nbt, _, _ = bn_ref.running_update(a.rm, a.rv, nbt0, ref.mean, ref.var, float(ref.n), momentum)
    torch.testing.assert_close(rm, bn.running_mean, **CLOSE)
    torch.testing.assert_close(rv, bn.running_var, **CLOSE)
    assert nbt == int(bn.num_batches_tracked)


@pytest.mark.parametrize("N,split,C", [(777, 700, 64), (40, 39, 257), (33, 5, 100)])
@pytest.mark.parametrize("momentum,nbt0", [(0.1, 0), (None, 1)])
def test_reference_two_shards(N, split, C, momentum, nbt0):
    """Each shard's rows of the full-batch answer; local parameter sums adding up to the batch's."""
    a = bn_ref.make_inputs(N, C)
    p, seed = 0.5, 7
    bn, out, dz = _torch_ref(a, p, seed, momentum, nbt0, split=split)
    lo, hi = slice(0, split), slice(split, N)
    tot_w = tot_b = 0
    for me, ot in ((lo, hi), (hi, lo)):
        ref = bn_ref.tail(a.z[me], a.r[me], a.w, a.b, p, seed, a.dh[me], other=(a.z[ot], a.dh[ot]))
        torch.testing.assert_close(ref.out, out[me], **CLOSE)
        torch.testing.assert_close(ref.dz, dz[me], **CLOSE)
        torch.testing.assert_close(ref.dweight + ref.sums2[C:], bn.weight.grad, **CLOSE)
        torch.testing.assert_close(ref.dbias + ref.sums2[:C], bn.bias.grad, **CLOSE)
        assert float(ref.stats2[2 * C]) == a.z[ot].size(0) and ref.n == N
        tot_w, tot_b = tot_w + ref.dweight, tot_b + ref.dbias
        rm, rv, nbt, _, _ = bn_ref.running_update(a.rm, a.rv, nbt0, ref.mean, ref.var, float(ref.n), momentum)
        torch.testing.assert_close(rm, bn.running_mean, **CLOSE)
        torch.testing.assert_close(rv, bn.running_var, **CLOSE)
    torch.testing.assert_close(tot_w, bn.weight.grad, **CLOSE)
    torch.testing.assert_close(tot_b, bn.bias.grad, **CLOSE)


def test_geometry_matches_hand_computed_values():
    assert [bn_ref.lanes(c) for c in (1, 3, 8, 64, 100, 128, 129, 255, 256, 257, 600)] == [256, 85, 32, 4, 2, 2, 1, 1, 1, 1, 1]
    assert (bn_ref.unit(64), bn_ref.unit(100), bn_ref.unit(257), bn_ref.unit(1)) == (32, 16, 8, 2048)
    assert bn_ref.rows_per_block(65537, 64) == 64 and bn_ref.rows_per_block(65536, 64) == 32
    assert bn_ref.rows_per_block(2, 1) == 2048 and bn_ref.rows_per_block(16385, 257) == 16
    assert bn_ref.grid(8193, 64) == 2048 and bn_ref.grid(8192, 64) == 2048 and bn_ref.grid(8188, 64) == 2047
    assert bn_ref.grid(2, 600) == 2 and bn_ref.grid(2, 1) == 1
    assert (bn_ref.passes(256), bn_ref.passes(257), bn_ref.passes(600)) == (1, 2, 3)
    assert bn_ref.chain(33, 64) == 4 + 4 + 17 and bn_ref.chain(65537, 64) == 8 + 4 + 17
    assert bn_ref.chain(4194305, 1) == 8 + 256 + 17
    table = bn_ref.case_table()
    assert len(table) == 3 * 11 + 2 * 4 and len(set(table)) == len(table)
    assert max(n * c for n, c in table) == 16385 * 257 and (4194305, 1) in table and (8193, 64) in table
    assert bn_ref.effective_seed(5) == 5 and bn_ref.effective_seed(-1) == 2 ** 64 - 1
    assert bn_ref.effective_seed(3, 5) == (5 * 0x9E3779B97F4A7C15 + 3) % 2 ** 64
    assert bn_ref.drop_scale(0.5) == 2.0 and bn_ref.drop_scale(0.0) == 1.0
    assert bn_ref.drop_scale(0.2) == float(np.float32(1.0 / (1.0 - float(np.float32(0.2)))))


@pytest.mark.parametrize("N,C", bn_ref.case_table())
def test_inputs_meet_the_conditions(N, C):
    """At most 1e-5 of a case's elements in the ReLU tie window; the integer probes' precondition."""
    a = bn_ref.make_inputs(N, C)
    ref = bn_ref.tail(a.z, a.r, a.w, a.b, 0.5, 1234567)
    assert ref.ties <= bn_ref.TIE_CAP * N * C, (ref.ties, N * C)
    z, dh = bn_ref.integer_inputs(N, C)
    assert bn_ref.integer_precondition(z, dh)
    assert float(z.abs().max()) <= 3 and float(dh.abs().max()) <= 3
    assert torch.equal(z, z.round()) and torch.equal(dh, dh.round())


@pytest.mark.parametrize("N,C", [(33, 64), (9, 257), (681, 3)])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_float32_emulation_meets_the_bounds(N, C, p):
    a = bn_ref.make_inputs(N, C)
    ref = bn_ref.tail(a.z, a.r, a.w, a.b, p, 42, a.dh)
    bn_ref.check_all(bn_ref.emulate_f32(a.z, a.r, a.w, a.b, p, 42, a.dh), ref)
    ref2 = bn_ref.tail(a.z[:-4], a.r[:-4], a.w, a.b, p, 42, a.dh[:-4], other=(a.z[-4:], a.dh[-4:]))
    bn_ref.check_all(bn_ref.emulate_f32(a.z[:-4], a.r[:-4], a.w, a.b, p, 42, a.dh[:-4], other=(a.z[-4:], a.dh[-4:])), ref2)


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("N,C", [(33, 64), (9, 257)])
@pytest.mark.parametrize("mutate", ["drop_row", "other_n", "mask_shift"])
def test_bounds_reject_a_mutated_kernel(N, C, mutate):
    """One row missing from the sums: the sums' and dz's bounds.  The other shard's n: every bound.
    The mask index shifted by one: every bound (half the elements change)."""
    a = bn_ref.make_inputs(N, C)
    p, seed, k = 0.5, 42, 4
    me, ot = slice(0, N - k), slice(N - k, N)
    other = (a.z[ot], a.dh[ot])
    ref = bn_ref.tail(a.z[me], a.r[me], a.w, a.b, p, seed, a.dh[me], other=other)
    good = bn_ref.emulate_f32(a.z[me], a.r[me], a.w, a.b, p, seed, a.dh[me], other=other)
    bn_ref.check_all(good, ref)
    bad = bn_ref.emulate_f32(a.z[me], a.r[me], a.w, a.b, p, seed, a.dh[me], other=other, mutate=mutate)
    assert _rejected(lambda: bn_ref.check_sums(bad.dweight, bad.dbias, ref))
    assert _rejected(lambda: bn_ref.check_dz(bad.dz, ref))
    if mutate != "drop_row":  # (the forward has no sum of its own to lose a row from)
        assert _rejected(lambda: bn_ref.check_forward(bad.out, ref))
    if mutate == "other_n":
        bn = torch.nn.BatchNorm1d(C, momentum=0.1)
        rm, rv, _, _, _ = bn_ref.running_update(a.rm, a.rv, 0, bad.mean, bad.var, float(bad.n), 0.1)
        with torch.no_grad():
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
            bn.num_batches_tracked.fill_(1)
        assert _rejected(lambda: bn_ref.check_running(bn, a.rm, a.rv, 0, ref, 0.1))


@pytest.mark.parametrize("N,C", [(33, 64), (9, 257)])
@pytest.mark.parametrize("mutate", ["drop_row", "other_n", "mask_shift"])
def test_exact_probes_reject_a_mutated_kernel(N, C, mutate):
    """The integer probes: bias.grad bit for bit, float32(mean) exactly."""
    z, dh = bn_ref.integer_inputs(N, C)
    one, zero = torch.ones(C), torch.zeros(C)
    p, seed, k = 0.5, 42, 4
    other = (z[N - k:], dh[N - k:])
    ref = bn_ref.tail(z[:N - k], None, one, zero, p, seed, dh[:N - k], other=other)
    good = bn_ref.emulate_f32(z[:N - k], None, one, zero, p, seed, dh[:N - k], other=other)
    assert torch.equal(good.dbias.double(), ref.dbias) and torch.equal(good.mean.float(), ref.mean.float())
    bad = bn_ref.emulate_f32(z[:N - k], None, one, zero, p, seed, dh[:N - k], other=other, mutate=mutate)
    assert not (torch.equal(bad.dbias.double(), ref.dbias) and torch.equal(bad.mean.float(), ref.mean.float()))
