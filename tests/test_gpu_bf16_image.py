"""The bf16 image GEMMs past one tile per block, element by element (cases, references and bounds:
bf16_image_cases; what they claim is checked on the CPU by test_bf16_image_host).

NT (gemm_nt_img16_kernel): M chosen from the device's CU count so that blocks run 2, 3, 4 and 7
tiles — every wait form of the LDS-DMA ring, every buffer reused, both C tiles, the clamped
look-ahead DMAs and a tail tile deep in a block's sweep.  Every case asserts the per-element bound,
the exact zeros of the keep mask (oracle.dropout_hash) and of ReLU, the misrounded count against
the CPU float32 evaluation's, z against the stored h, sentinels around an output written into the
a2 half of a second image and into a padded buffer, and that the two runs agree bit for bit.  At
the deepest shape the output rows of three row ranges are also bit-identical to a one-tile-per-block
run over a copy of those image rows.

TN (gemm_tn_img16_kernel): row blocks of 4, 6 and 8 chunks with last blocks of 3, 5, 7 and 1 (clamped)
chunks, Nr of 128, 72 and 8, the four forms with and without gout, f32 and bf16 g / gout: dW per
output row against the float64 RNE(G)^T A, db, dz^T h, sum dz, gout element by element, and
sentinels around the flat output, the slab workspace and gout.
"""
import functools

import pytest
import torch

import bf16_image_cases as bc

pytestmark = pytest.mark.gpu

SENT16 = 0x7F5A        # bf16 3.0e38: no output of these cases
SENT32 = 0x7FC12345    # a float32 NaN payload
GUARD = 64             # floats on either side of a guarded allocation (keeps 16-byte alignment)


@pytest.fixture(scope="module")
def cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def _fill(buf):
    if buf.element_size() == 2:
        buf.view(torch.int16).fill_(SENT16)
    else:
        buf.view(torch.int32).fill_(SENT32)
    return buf


def _outside_untouched(buf, r0, r1, c0, c1):
    """Whether every element of the 2-D ``buf`` outside [r0, r1) x [c0, c1) still holds the sentinel bits."""
    v, s = (buf.view(torch.int16), SENT16) if buf.element_size() == 2 else (buf.view(torch.int32), SENT32)
    v = v.clone()
    v[r0:r1, c0:c1] = s
    return bool((v == s).all())


def _image(a1, a2, device):
    from elliptic_gnn_project_amd.planes import BfImage

    im = BfImage(a1.size(0), a1.size(1), a2.size(1), device, zero=True)
    im.a1.copy_(a1.to(device))
    im.a2.copy_(a2.to(device))
    return im


@functools.lru_cache(maxsize=1)
def _nt_device(M, k1, k2, nc, device):
    op = bc.nt_operands(M, k1, k2, nc)
    assert (op.M, bc.image_ld(k1, k2)[1]) == (M, op.K)
    im = _image(op.a1, op.a2, device)
    assert (im.col2, im.ld) == bc.image_ld(k1, k2)
    return im, {k: getattr(op, k).to(device) for k in ("w1", "w2", "bias", "proj")}


def _run_nt(im, t, nc, epi, out, z=None, seed=bc.DROP_SEED, seed_ptr=None):
    from elliptic_gnn_project_amd.fused import gemm_nt

    bias, relu, drop, proj = bc.EPIS[epi]
    kw = dict(planes=im, out=out, w1=t["w1"], w2=t["w2"])
    if bias:
        kw["bias"] = t["bias"]
    if relu:
        kw["relu"] = True
    if drop:
        kw.update(dropout_p=bc.DROP_P, seed=seed, seed_ptr=seed_ptr)
    if proj:
        kw.update(proj=t["proj"], z=z)
    assert gemm_nt(None, None, nc, check_planes=True, **kw)
    c = gemm_nt(None, None, nc, **kw)
    assert c.data_ptr() == out.data_ptr() and c.dtype == torch.bfloat16
    return c


def _dest_image(M, nc, device):
    """The a2 half of a second image (as the model's NT writes the next layer's operand)."""
    from elliptic_gnn_project_amd.planes import BfImage

    im2 = BfImage(M, 128, nc, device, zero=True)
    _fill(im2.img)
    return im2.img, im2.a2, (0, M, im2.col2, im2.col2 + nc)


def _dest_padded(M, nc, device):
    """A plain buffer with the pitch of the wide image, two guard rows on either side."""
    buf = _fill(torch.empty((M + 4, 336), dtype=torch.bfloat16, device=device))
    return buf, buf[2:M + 2, 168:168 + nc], (2, M + 2, 168, 168 + nc)


def _dest_z(M, device):
    zb = _fill(torch.empty((M + 2, 8), dtype=torch.float32, device=device))
    return zb, zb[1:M + 1, :4], (1, M + 1, 0, 4)


def _nt_case_run(device, cus, case, seed=bc.DROP_SEED, seed_ptr=None):
    s, k1, k2, nc, epi = case
    M = bc.nt_rows(cus)[s]
    assert bc.nt_sweep(M, cus)[2] >= 2  # more tiles than blocks
    im, t = _nt_device(M, k1, k2, nc, device)
    proj = bool(bc.EPIS[epi][3])
    outs = []
    for dest in (_dest_image, _dest_padded):
        buf, out, box = dest(M, nc, device)
        zb, z, zbox = _dest_z(M, device) if proj else (None, None, None)
        _run_nt(im, t, nc, epi, out, z, seed, seed_ptr)
        torch.cuda.synchronize()
        assert _outside_untouched(buf, *box), dest.__name__
        if proj:
            assert _outside_untouched(zb, *zbox), dest.__name__
        outs.append((out, z))
    assert torch.equal(outs[0][0], outs[1][0])  # two calls, two destinations: the same bits
    if proj:
        assert torch.equal(outs[0][1], outs[1][1])
    return outs[0][0].cpu(), outs[0][1].cpu() if proj else None


def _assert_nt(r, c, z, allow, name):
    res = bc.nt_check(r, c)
    print(name, f"worst bound ratio {res.worst:.3f} at {res.worst_at}, misrounded {res.misrounded} / {res.n}, "
                f"allowed {allow}, nonzero where zero is exact {res.zero_bad}")
    assert res.bound_bad == 0, (res.bound_bad, res.worst, res.worst_at)
    assert res.zero_bad == 0  # keep mask off (the counter hash, bit for bit), or ReLU of a clearly negative sum
    assert res.misrounded <= allow, (res.misrounded, allow)
    if r.proj is not None:
        assert bc.nt_check_z(r, c, z) == 0


@pytest.mark.parametrize("case", bc.NT_CASES, ids=bc.nt_id)
def test_nt_image_past_one_tile_per_block(device, cus, case):
    r = bc.nt_reference(case, cus)
    c, z = _nt_case_run(device, cus, case)
    _assert_nt(r, c, z, bc.misround_allowance(bc.cpu_misrounded(case, cus, r)), bc.nt_id(case))


def test_nt_image_seed_counter(device, cus):
    """With seed_ptr set the mask is the oracle's under seed = *seed_ptr * phi + seed (mod 2^64), at
    every tile of a block's sweep."""
    case = (1, 128, 128, 128, "drop_proj")
    assert case in bc.NT_CASES
    counter = 0x1_0000_0005  # past 32 bits: the product wraps in 64
    seed = bc.effective_seed(bc.DROP_SEED, counter)
    assert seed != bc.DROP_SEED
    r = bc.nt_reference(case, cus, seed=seed)
    assert not torch.equal(r.keep, bc.nt_reference(case, cus).keep)
    ctr = torch.tensor([counter], dtype=torch.int64, device=device)
    c, z = _nt_case_run(device, cus, case, seed_ptr=ctr)
    cpu = bc.nt_check(r, r.cpu).misrounded
    _assert_nt(r, c, z, bc.misround_allowance(cpu), "seed counter")


@pytest.mark.parametrize("case", bc.RANGE_CASES, ids=bc.nt_id)
def test_nt_ring_position_changes_no_bit(device, cus, case):
    """A tile's arithmetic does not depend on where in a block's sweep it runs: rows [r0, r1) of the
    deepest shape's output equal, bit for bit, a run over a copy of those image rows (one tile per
    block: the path test_gpu_bf16 pins).  A stale ring buffer or a C-tile mix-up shows here even
    where it stays inside the float64 bound."""
    from elliptic_gnn_project_amd.planes import BfImage

    s, k1, k2, nc, epi = case
    M = bc.nt_rows(cus)[s]
    assert bc.nt_sweep(M, cus)[1:3] == (6, 7) or cus < 77
    im, t = _nt_device(M, k1, k2, nc, device)
    proj = bool(bc.EPIS[epi][3])
    big = torch.empty((M, nc), dtype=torch.bfloat16, device=device)
    zbig = torch.empty((M, 4), device=device) if proj else None
    _run_nt(im, t, nc, epi, big, zbig)
    for r0, r1 in bc.nt_ranges(cus):
        assert bc.nt_sweep(r1 - r0, cus)[2] == 1
        sub = BfImage(r1 - r0, k1, k2, device, zero=True)
        sub.img.copy_(im.img[r0:r1])
        out = torch.empty((r1 - r0, nc), dtype=torch.bfloat16, device=device)
        zs = torch.empty((r1 - r0, 4), device=device) if proj else None
        _run_nt(sub, t, nc, epi, out, zs)
        assert torch.equal(big[r0:r1], out), (r0, r1)
        if proj:
            assert torch.equal(zbig[r0:r1], zs), (r0, r1)


# ------------------------------------------------------------------------------------------ TN
class _GuardedEmpty:
    """torch.empty for the duration of one gemm_tn call: its flat float32 allocations (the output,
    the slab workspace) come from the middle of sentinel-filled buffers."""

    def __init__(self):
        self.empty, self.bufs = torch.empty, []

    def __call__(self, *size, **kw):
        if len(size) != 1 or not isinstance(size[0], int) or kw.get("dtype") != torch.float32:
            return self.empty(*size, **kw)
        buf = _fill(self.empty(size[0] + 2 * GUARD, **kw))
        self.bufs.append((buf, size[0]))
        return buf[GUARD:GUARD + size[0]]

    def untouched(self):
        return [bool((torch.cat([b[:GUARD], b[GUARD + n:]]).view(torch.int32) == SENT32).all()) for b, n in self.bufs]


@functools.lru_cache(maxsize=1)
def _tn_device(M, k1, k2, device):
    op = bc.tn_operands(M, k1, k2)
    return _image(op.a1, op.a2, device)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("case", bc.TN_CASES, ids=bc.tn_id)
def test_tn_image_chunk_ring(device, monkeypatch, case):
    from elliptic_gnn_project_amd.fused import gemm_tn

    M, k1, k2, nr, form, want_gout, gdt = case
    r = bc.tn_reference(case)
    im = _tn_device(M, k1, k2, device)
    assert im.ld == bc.image_ld(k1, k2)[1]
    kw = dict(planes=im, hscale=r.hs)
    if r.h is not None:
        kw["h"] = r.h.to(device)
    if r.g_in is None:
        kw.update(dz=r.op.dz.to(device), proj=r.proj.to(device))
    else:
        kw["g"] = r.g_in.to(device)
    gbuf = gout = None
    if want_gout:  # a wider destination: a guard row above and below, guard columns on both sides
        gbuf = _fill(torch.empty((M + 2, nr + 8), dtype=torch.bfloat16 if gdt == "bf16" else torch.float32, device=device))
        gout = kw["gout"] = gbuf[1:M + 1, 4:4 + nr]
    assert gemm_tn(nr, None, None, check_planes=True, **kw)
    guard = _GuardedEmpty()
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", guard)
        (dW1, dW2_), db, dW2, dzs = gemm_tn(nr, None, None, **kw)
    torch.cuda.synchronize()
    assert len(guard.bufs) == 2 and guard.bufs[0][1] == nr * (k1 + k2) + nr + (4 * nr + 4 if r.g_in is None else 0)
    assert guard.untouched() == [True, True]  # nothing past the Nr-row layout, nothing past the slabs
    assert dW1.shape == (nr, k1) and dW2_.shape == (nr, k2) and db.shape == (nr,)

    gc = None
    if want_gout:
        assert _outside_untouched(gbuf, 1, M + 1, 4, 4 + nr)
        gc = gout.cpu()
        if r.g_in is not None:
            assert torch.equal(gc.double(), r.G)  # g * mask * 2: exact in either dtype
        elif gdt == "f32":
            assert bool(((gc.double() - r.G).abs() <= r.eps).all())
        else:  # the rounded G: between the roundings of the float64 G -+ its f32 formation error
            assert bool(((gc.double() >= bc.rne_bf16(r.G - r.eps)) & (gc.double() <= bc.rne_bf16(r.G + r.eps))).all())
    operand, slack = bc.tn_operand(r, gc)
    ref = operand.t() @ r.op.A64
    dW = torch.cat([dW1, dW2_], 1).cpu()
    misses = bc.row_misses(dW, ref, slack)
    d = (dW.double() - ref).norm(dim=1)
    print(bc.tn_id(case), f"dW worst row {float((d / ref.norm(dim=1)).max()):.2e} whole {_rel(dW, ref):.2e} "
                          f"flip slack {float((slack / ref.norm(dim=1)).max()):.2e} db {_rel(db, r.db):.2e}")
    assert misses == []
    assert float((dW.double() - ref).norm()) <= 1e-5 * float(ref.norm()) + float(slack.norm())
    assert _rel(db, r.db) < 1e-5
    if r.g_in is None:
        assert _rel(dzs, r.dzs) < 1e-5
        if r.h is not None:
            assert bc.row_misses(dW2.cpu(), r.dw2) == [] and _rel(dW2, r.dw2) < 1e-5
        else:
            assert not bool(dW2.any())  # no h: dz^T h is zero
    else:
        assert dW2 is None and dzs is None
