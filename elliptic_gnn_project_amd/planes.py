"""Split images ("planes") of the SAGE layer-1 GEMM operand [agg | x].

The split-bf16 GEMMs run every f32 operand as three bf16 terms, v = hi + mid + lo exactly
(hi = RNE(v), mid = RNE(v - hi), lo = RNE(v - hi - mid)).  Splitting inside the GEMMs costs
~5.5 VALU per element, twice per step for the [N, 332] layer-1 operand.  A ``SplitImage`` holds
the three planes in HBM instead ([3, N, ld] bf16, include/gnnmp.h gnn_split_planes_f32):

    columns [0, k1)               agg = mean_{j->i} x[j]   K1 (gnn_sage_mean_fwd_planes), once per
                                                           registered x and graph plan
    columns [col2, col2 + k2)     x                        written once per input tensor
    everything else               zero

``x`` is a constant of the training run (the reference prepares it once, src/train_gnn.py:
315-350), so its planes are cached on the tensor like the graph plan (graph.py), keyed on
(data_ptr, _version): an in-place edit of x rebuilds them.

The agg half depends on x and the graph plan alone — not on the weights, the dropout seed or the
step — and K1 is deterministic, so for a registered x it is cached too (``mean_cached``): K1 runs
when the image's agg half does not already hold the means of this (x, plan, hub form, exp), which
in a training run is the first forward; every later epoch and evaluation over the same edge_index
reads the same bits K1 would write again.  Nothing computed from the weights or the step's inputs
is reused across steps.  GNNMP_AGG_CACHE=0 (fused.py) runs K1 on every forward.  The rules that
keep the cache right under graph capture are ``mean_cached``'s (``_AggCache``); the bf16-storage
layer-0 image (``BfImage``, ``bf_x_image``) caches its aggregate the same way.

A forward stamps the image with a generation number (bumped by every K1 run); the backward
checks it, and recomputes the agg half (deterministically: the same bits) if a forward over
another plan rewrote it in between.
"""
from __future__ import annotations

import ctypes
import weakref

import torch

from . import _lib

_ATTR = "_gnnmp_split_image"


def _pad8(k: int) -> int:
    return (k + 7) // 8 * 8


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class _AggCache:
    """The agg half of a layer-0 image as a cache (module docstring): what it holds, and the
    rules that keep that right under graph capture."""

    def _agg_init(self) -> None:
        self.agg_key = None        # what the agg half holds (mean_cached), None: unknown
        self.agg_pin = None        # the key a captured step that skipped the gather reads on every replay
        self.agg_volatile = False  # a gather was captured: replays rewrite the agg half unseen
        self._agg_event = None     # (stream, event) of the gather agg_key records

    def agg_key_of(self, plan, hub=True):
        """The identity of an agg half: x's image key, the plan object (plans are rebuilt when
        edge_index is edited, so identity suffices; held weakly), the hub choice and exp."""
        return (self.x_key, weakref.ref(plan), bool(hub), int(getattr(self, "exp", 0)))

    @staticmethod
    def _same_key(a, b) -> bool:
        if a is None or b is None:
            return False
        pa, pb = a[1](), b[1]()
        return pa is not None and pa is pb and a[0] == b[0] and a[2:] == b[2:]

    def agg_foreign(self, plan, hub=True) -> bool:
        """Whether a captured step pinned the agg half to another key than (plan, hub)'s: a gather
        for this plan would overwrite what that step's replays read."""
        return self.agg_pin is not None and not self._same_key(self.agg_pin, self.agg_key_of(plan, hub))

    def agg_reset(self) -> None:
        """x was edited (its planes are rebuilt): the agg half is stale and no longer pinned."""
        self.agg_key = None
        self.agg_pin = None

    def _agg_written(self) -> None:
        """Before any launch that writes the agg half."""
        self.agg_key = None  # rewritten: recorded again after the launch (_agg_record)
        if _capturing():
            self.agg_volatile = True

    def _agg_hit(self, key, x: torch.Tensor, cache=True) -> bool:
        if not (cache and not self.agg_volatile and is_registered(x) and self._same_key(self.agg_key, key)):
            return False
        if _capturing():
            self.agg_pin = key
        elif self._agg_event is not None:
            st, ev = self._agg_event
            cur = torch.cuda.current_stream(x.device)
            if st != cur:  # the gather ran on another stream
                cur.wait_event(ev)
        return True

    def _agg_record(self, key, x: torch.Tensor, cache=True) -> None:
        if cache and not _capturing() and not self.agg_volatile and is_registered(x):
            self.agg_key = key
            self._agg_event = None
            if x.is_cuda:
                cur = torch.cuda.current_stream(x.device)
                ev = torch.cuda.Event()
                ev.record(cur)
                self._agg_event = (cur, ev)


class SplitImage(_AggCache):
    """[3, N, ld] bf16 planes of [A1 | A2] with A1 at column 0 and A2 at column ``col2``."""

    nplanes = 3
    fmt = _lib.PLANES_SPLIT_BF16
    _split_fn = "gnn_split_planes_f32"
    _mean_fn = "gnn_sage_mean_fwd_planes"

    @staticmethod
    def layout(k1: int, k2: int):
        """(col2, ld) of an image of [A1 (k1 columns) | A2 (k2 columns)]."""
        col2 = _pad8(k1)
        return col2, (col2 + _pad8(k2) + 15) // 16 * 16

    @classmethod
    def addressable(cls, n: int, k1: int, k2: int, ld: int | None = None) -> bool:
        """The kernels address the planes with 31-bit byte offsets."""
        return cls.nplanes * int(n) * max(SplitImage.layout(k1, k2)[1], ld or 0) * 2 < 2 ** 31

    def __init__(self, n: int, k1: int, k2: int, device: torch.device, ld: int | None = None):
        self.n, self.k1, self.k2 = int(n), int(k1), int(k2)
        self.col2, self.ld = self.layout(k1, k2)
        if ld is not None:  # a wider row (zeros past the operand): the kernels' fixed image widths
            self.ld = max(self.ld, int(ld))
        self.ps = self.n * self.ld
        dt = torch.bfloat16 if self.nplanes == 3 else torch.float16
        self.img = torch.empty((self.nplanes, self.n, self.ld), dtype=dt, device=device)
        self.gen = 0
        self.x_key = None
        self.exp = 0  # half-pair images: the pre-scale exponent of the image's values (h2_exp)
        self._agg_init()

    @property
    def ptr(self) -> int:
        return self.img.data_ptr()

    def fill_x(self, x: torch.Tensor) -> None:
        """Planes of x into columns [col2, ld) (zeros past k2)."""
        with torch.cuda.device(x.device):
            _lib.call(self._split_fn, x.data_ptr(), int(x.stride(0)), self.n, self.k2, self.ptr, self.ld,
                      self.ps, self.col2, self.ld - self.col2, *self._exp_arg(), _lib.stream_handle(x.device))

    def _exp_arg(self):
        return ()

    def fill_mean(self, plan, x: torch.Tensor, keep=None, prep_b=None, x_pad=None, hub=True) -> int:
        """K1: planes of mean_{j->i} x[j] into columns [0, col2); returns the new generation.
        keep (half-pair images only): (mask [N, 4] int32, cols, p, seed, seed_ptr) — K1 also writes
        the dropout keep bits of the NT that reads this image (include/gnnmp.h gnn_sage_mean_fwd_h2).
        prep_b (half-pair images only): the GnnGemmNTParams of that NT (fused.gemm_nt b_stage
        "params"); its B-image prep runs inside K1's launch, the NT then runs with b_ready.
        x_pad: x padded with zero columns to the image's col2 (planes.x_padded): K1 gathers it
        (16-byte pieces) and writes the agg half at full width, padding columns zero.
        hub (half-pair images only): the plan's hub form when it has one (graph.K1_HUB_MAX_N: the
        hub rows on blocks of their own); False: one wave per 16 rows throughout."""
        from .aggregation import KernelTimer, agg_bytes

        self._agg_written()
        e0 = KernelTimer.begin()
        src, F = (x_pad, int(x_pad.size(1))) if x_pad is not None else (x, self.k1)
        args = (plan.c_graph, plan.deg.data_ptr(), src.data_ptr(), int(src.stride(0)), F, self.ptr, self.ld,
                self.ps, self.col2)
        if self.nplanes == 2:
            km, cols, p, seed, sptr = keep if keep is not None else (None, 0, 0.0, 0, None)
            hs = getattr(plan, "hub", None) if hub else None
            args += (int(self.exp), _lib.ptr(km), int(cols), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(sptr), prep_b,
                     ctypes.byref(hs["c"]) if hs is not None else None)
        elif prep_b is not None:
            raise ValueError("prep_b needs a half-pair image")
        _lib.call(self._mean_fn, *args, _lib.stream_handle(x.device))
        # algorithmic bytes of K1 as SURVEY §8(d) counts them (f32 output); the planes store 6 B
        KernelTimer.end(e0, ("agg", _lib.AGG_MEAN, False, self.k1), agg_bytes(plan, self.k1, _lib.AGG_MEAN, False, False))
        self.gen += 1
        return self.gen

    def mean_cached(self, plan, x: torch.Tensor, keep=None, prep_b=None, x_pad=None, hub=True, cache=True):
        """The agg half for (x, plan): (generation, hit).  A hit launches nothing — the image
        already holds these means — and needs: the same key as the last K1 recorded
        (agg_key_of), a registered x, no keep bits asked of K1, ``cache`` (GNNMP_AGG_CACHE).
        Otherwise K1 runs (fill_mean; ``prep_b`` may be a callable, evaluated only then) and
        its key is recorded.

        Under stream capture: a key is never recorded (a captured K1 has not run), and an image
        whose K1 was captured stays uncached, since every replay rewrites its agg half.  A
        captured step that hit the cache pins the image to its key: its replays read the agg
        half, so no K1 for another key may write it (agg_foreign; fused._layer0_image then takes
        the f32-operand path) until x is edited."""
        key = self.agg_key_of(plan, hub)
        if keep is None and self._agg_hit(key, x, cache):
            return self.gen, True
        if callable(prep_b):
            prep_b = prep_b()
        gen = self.fill_mean(plan, x, keep, prep_b=prep_b, x_pad=x_pad, hub=hub)
        self._agg_record(key, x, cache)
        return gen, False

class HalfPairImage(SplitImage):
    """[2, N, ld] f16 half-pair planes of [A1 | A2] · 2^exp (include/gnnmp.h gnn_split_h2_f32):
    u = v·2^exp, hi = RNE_f16(u), lo = RNE_f16((u - hi)·2^11).  The half-pair GEMMs read them with
    3 f16 products per product (the split-bf16 image needs 6) and 4 B per element (6), and undo
    the power-of-two pre-scale exactly in their epilogues.  ``exp`` (h2_exp of x) brings x's
    largest magnitude into [2^13, 2^14), so every value within 2^-26 of it keeps hi and lo f16
    normals — full 2^-22 relative precision whatever x's magnitude; the mean half is a mean of
    x's rows and stays inside the same range."""

    nplanes = 2
    fmt = _lib.PLANES_HALF_PAIR
    _split_fn = "gnn_split_h2_f32"
    _mean_fn = "gnn_sage_mean_fwd_h2"

    def _exp_arg(self):
        return (int(self.exp),)

    def fill_x(self, x: torch.Tensor) -> None:
        self.exp = h2_exp(x)
        if self.exp is None:
            raise ValueError("a half-pair image needs finite x (h2_ok)")
        super().fill_x(x)

    def keep_buffer(self) -> torch.Tensor:
        """[N, 4] int32 keep bits of the dropout that follows this image's NT (written by K1)."""
        kb = getattr(self, "_keep", None)
        if kb is None:
            kb = self._keep = torch.empty((self.n, 4), dtype=torch.int32, device=self.img.device)
        return kb

    _B_WS_MAX = 8  # sets of weights whose workspace one image keeps (the oldest leaves first)

    def b_workspace(self, w1: torch.Tensor, w2, nfloats: int) -> torch.Tensor:
        """The persistent B workspace (B image + column scales) of this image's half-pair NT over
        the Linear weights w1 / w2, one per (image, weights): what the optimizer's launch builds
        for the next forward (fused.adam_prep_*, gnn_clip_adam_prep_f32).  Allocated on first use
        — the eager warm-up, before any capture; a CapturedStep whose graph reads one holds it."""
        held = getattr(self, "_b_ws", None)
        if held is None:
            held = self._b_ws = {}
        key = (w1.data_ptr(), w2.data_ptr() if w2 is not None else 0)
        ws = held.get(key)
        if ws is None or ws.numel() < nfloats:
            ws = torch.empty(max(int(nfloats), 1), dtype=torch.float32, device=self.img.device)
            held.pop(key, None)
            while len(held) >= self._B_WS_MAX:
                held.pop(next(iter(held)))
            held[key] = ws
        return ws


H2_TOP = 14  # a half-pair image's largest magnitude is pre-scaled into [2^(H2_TOP-1), 2^H2_TOP)


def _k1_takes(ptr: int, ldx: int, F: int, width: int) -> bool:
    """The predicate of gnn_sage_mean_fwd_planes / _h2 (aggregate.hip sage_mean_fwd_image) for a
    gather source at ``ptr`` with pitch ``ldx`` and an image whose agg half is ``width`` wide: the
    images themselves are allocator-aligned with ld and plane stride multiples of 16."""
    v4 = F % 4 == 0 and ldx % 4 == 0 and width % 4 == 0 and ptr % 16 == 0
    v2 = F % 2 == 0 and ldx % 2 == 0 and width % 2 == 0 and ptr % 8 == 0
    vec = 4 if v4 else 2
    return v2 and F // vec > 32 and -(-width // vec) <= 128


def mean_planes_ok(x: torch.Tensor) -> bool:
    """Whether gnn_sage_mean_fwd_planes / _h2 takes x itself as its gather source (f32 rows, even F
    with 32 < F/vec, the image's agg half at most 128 lane pieces wide, x 8-byte aligned — 16 for
    the 4-wide gather).  A forward that gathers x_padded(x) instead asks padded_mean_planes_ok
    too; x itself is still asked there, since a backward that refills the agg half
    (SplitImage.fill_mean without x_pad) gathers x."""
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda:
        return False
    return _k1_takes(x.data_ptr(), x.stride(0), x.size(1), _pad8(x.size(1)))


def padded_mean_planes_ok(x: torch.Tensor) -> bool:
    """Whether K1 takes x_padded(x, pad8(F)) (its own 16-byte rows, as wide as the image's agg
    half): e.g. F = 70 pads to 72 columns, 18 lane pieces of 4 — fewer than K1's 32."""
    col2 = _pad8(x.size(1))
    return _k1_takes(0, col2, col2, col2)


def x_image(x: torch.Tensor, cls=SplitImage) -> SplitImage:
    """The cached split image of [agg | x] for x (its x half filled), rebuilt after in-place edits.
    cls: SplitImage (split-bf16) or HalfPairImage."""
    key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()))
    attr = _ATTR if cls is SplitImage else _ATTR + "_h2"
    im = getattr(x, attr, None)
    if im is None or im.n != x.size(0) or im.k2 != x.size(1):
        im = cls(x.size(0), x.size(1), x.size(1), x.device)
        try:
            setattr(x, attr, im)
        except (AttributeError, RuntimeError):  # e.g. inference tensors: no caching
            pass
    if im.x_key != key:
        im.fill_x(x)
        im.x_key = key
        im.agg_reset()
    return im


def x_padded(x: torch.Tensor, width: int) -> torch.Tensor:
    """x with its rows padded by zero columns to ``width`` (a multiple of 4: 16-byte rows), cached
    on x with the image key: K1's gather then reads one 16-byte piece per lane (VEC 4, one pass
    over the row) instead of two 8-byte ones.  The padding columns aggregate to the zeros the
    image holds there anyway."""
    key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()), int(width))
    got = getattr(x, _ATTR + "_pad", None)
    if got is not None and got[0] == key:
        return got[1]
    xp = torch.zeros((x.size(0), width), dtype=x.dtype, device=x.device)
    xp[:, : x.size(1)].copy_(x)
    try:
        setattr(x, _ATTR + "_pad", (key, xp))
    except (AttributeError, RuntimeError):
        pass
    return xp


def h2_exp(x: torch.Tensor):
    """The half-pair pre-scale exponent of x — e = 14 - E for max|x| in [2^(E-1), 2^E), so the
    image holds x·2^e with its largest magnitude in [2^13, 2^14) (0 for an all-zero x; clamped to
    the ABI's [-100, 100]) — or None when x has a non-finite value (such inputs keep the split-bf16
    image).  One reduction per x, cached with the image key (data_ptr, _version)."""
    import math

    key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()))
    got = getattr(x, _ATTR + "_h2exp", None)
    if got is not None and got[0] == key:
        return got[1]
    if x.numel() == 0:
        e = 0
    else:
        amax = float(x.detach().abs().amax())  # inf / nan propagate
        if not math.isfinite(amax):
            e = None
        elif amax == 0.0:
            e = 0
        else:
            e = max(-100, min(100, H2_TOP - math.frexp(amax)[1]))
    try:
        setattr(x, _ATTR + "_h2exp", (key, e))
    except (AttributeError, RuntimeError):
        pass
    return e


def h2_ok(x: torch.Tensor) -> bool:
    """Whether x fits a half-pair image: every value finite (the power-of-two pre-scale, h2_exp,
    takes any finite magnitude)."""
    return h2_exp(x) is not None


_ATTR_X = _ATTR + "_x"


_CONST = "_gnnmp_const_input"


def is_registered(x: torch.Tensor) -> bool:
    """Whether x was declared a constant input (register_input)."""
    return bool(getattr(x, _CONST, False))


def register_input(x: torch.Tensor) -> torch.Tensor:
    """Declare x a constant input of the run (the training loop's node features, prepared once,
    src/train_gnn.py:315-350): layers whose A operand is x then read it from a split image built
    once per (unmodified) x — a per-graph input layout, like the CSR plan: the SAGE layer-1
    [agg | x] image (the x half once per x, the agg half once per x and graph plan:
    SplitImage.mean_cached) and the GCN / GAT layer-1 x-only image.  Unregistered inputs (a
    mini-batch's gathered rows, a per-step time-injected input) keep the f32-operand kernels, so
    no call allocates an image or pays a split pass it cannot reuse.  Returns x."""
    try:
        setattr(x, _CONST, True)
    except (AttributeError, RuntimeError):
        pass
    return x


X_ONLY_LD = 176


def x_only_image(x: torch.Tensor, cls=SplitImage):
    """The cached split image of a registered input x alone (x in columns [0, F), k2 = 0) for the
    GEMMs of a layer whose A operand is x (GCN / GAT layer 1: y = x·Wᵀ and dW = Gᵀ·x), or None.
    cls: SplitImage (split-bf16, both GEMMs) or HalfPairImage (x must be finite: h2_ok).

    Built on first use (one split pass) and reused while x is unmodified (data_ptr, _version);
    every call over a registered x takes the same kernels, so repeated forwards are bit-identical."""
    if (not getattr(x, _CONST, False) or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1
            or not x.is_cuda or x.requires_grad or x.size(0) < 32 or x.size(1) > 328):
        return None
    if cls is HalfPairImage and not h2_ok(x):
        return None
    key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()))
    attr = _ATTR_X if cls is SplitImage else _ATTR_X + "_h2"
    im = getattr(x, attr, None)
    # rows of 176 (the input GEMMs' image width) for any x of <= 176 columns, zeros past x
    ld = X_ONLY_LD if x.size(1) <= X_ONLY_LD else None
    if im is None or im.n != x.size(0) or im.k1 != x.size(1):
        if not cls.addressable(x.size(0), x.size(1), 0, ld):  # checked before allocating
            return None
        im = cls(x.size(0), x.size(1), 0, x.device, ld)
        try:
            setattr(x, attr, im)
        except (AttributeError, RuntimeError):  # e.g. inference tensors: not cached, still used
            pass
    if im.x_key != key:
        if cls is HalfPairImage:
            im.exp = h2_exp(x)
        with torch.cuda.device(x.device):
            _lib.call(cls._split_fn, x.data_ptr(), int(x.stride(0)), im.n, im.k1, im.ptr, im.ld, im.ps,
                      0, im.ld, *im._exp_arg(), _lib.stream_handle(x.device))
        im.x_key = key
    return im


# ----------------------------------------------------------------------------- bf16 images
class BfImage(_AggCache):
    """One-plane bf16 image [N, ld] of a bf16-storage layer operand [A1 | A2] (BASELINE configs[4]):
    A1 (the layer's aggregate) in columns [0, k1), A2 (its input h) in [col2, col2 + k2), zeros
    elsewhere, ld a multiple of 16 (whole MFMA k-steps).  The producers write straight into it —
    the bf16 aggregation into ``a1`` (row pitch ld) and the previous layer's NT into ``a2`` — so
    the weight-stationary bf16 NT (gemm_ws.hip gemm_nt_img16_kernel) stages whole 16-byte k-step
    pieces with no gather or padding pass."""

    bf16 = True

    def __init__(self, n: int, k1: int, k2: int, device: torch.device, zero: bool = False):
        self.n, self.k1, self.k2 = int(n), int(k1), int(k2)
        self.col2 = _pad8(k1)
        self.ld = (self.col2 + _pad8(k2) + 15) // 16 * 16
        self.ps = self.n * self.ld
        alloc = torch.zeros if (zero or self.col2 != self.k1 or self.col2 + self.k2 != self.ld) else torch.empty
        self.img = alloc((self.n, self.ld), dtype=torch.bfloat16, device=device)
        self.x_key = None
        self._agg_init()

    def mean_cached(self, plan, x: torch.Tensor, fill, cache=True) -> bool:
        """The layer-0 agg half for (x, plan), as SplitImage.mean_cached: ``fill()`` (the bf16
        aggregation into ``a1``) runs unless the image already holds it; returns whether it did."""
        key = self.agg_key_of(plan)
        if self._agg_hit(key, x, cache):
            return True
        self._agg_written()
        fill()
        self._agg_record(key, x, cache)
        return False

    @property
    def ptr(self) -> int:
        return self.img.data_ptr()

    @property
    def a1(self) -> torch.Tensor:
        return self.img[:, : self.k1]

    @property
    def a2(self) -> torch.Tensor:
        return self.img[:, self.col2: self.col2 + self.k2]


def bf_x_image(x: torch.Tensor) -> BfImage:
    """The cached bf16 image of [agg | x] for a bf16 input x (its x half copied in once, like the
    graph plan: rebuilt after an in-place edit of x); the agg half is written once per registered
    x and plan (BfImage.mean_cached)."""
    key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()))
    attr = _ATTR + "_bf16"
    im = getattr(x, attr, None)
    if im is None or im.n != x.size(0) or im.k2 != x.size(1):
        im = BfImage(x.size(0), x.size(1), x.size(1), x.device, zero=True)
        try:
            setattr(x, attr, im)
        except (AttributeError, RuntimeError):
            pass
    if im.x_key != key:
        im.a2.copy_(x)  # one layout copy per input tensor (the padding columns stay zero)
        im.x_key = key
        im.agg_reset()
    return im
