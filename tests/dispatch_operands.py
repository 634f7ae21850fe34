"""Operands at a chosen alignment and row pitch, for the dispatch-lattice tests
(test_gpu_dispatch_agg.py, test_gpu_dispatch_gemm.py).

Every host entry point of libgnnmp picks its kernel from the row width, the row pitch and the
pointer alignment of each operand.  ``Carved`` builds an operand whose pointer and pitch are
chosen by the test and that reaches the kernel without a copy:

  ("flat", o)          buf[o : o + N*F].view(N, F) of a flat buffer: contiguous, pitch F, pointer
                       4*o bytes (f32) past a 16-byte boundary.  Survives every .contiguous().
  ("pad", o, extra)    buf[G : G+N, o : o+F] of an [N + 2G, F + extra] buffer: pitch F + extra,
                       column offset o, G guard rows before and after.  (G = 8, so the first row's
                       offset G * pitch is a multiple of 8 elements whatever the pitch: the pointer
                       alignment is o's alone.)

The whole buffer is first filled with one fixed quiet-NaN bit pattern.  For an input that means
a value read from outside the view shows up in the result as NaN; for an output it means an
element the kernel never wrote stays NaN, and ``check_outside`` proves bit for bit that no store
landed outside the view (past F, before the first row, after the last).
"""
import torch

GUARD = 8
NAN_BITS = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FC5, torch.float16: 0x7E55}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def ld_of(layout, F):
    return F if layout[0] == "flat" else F + layout[2]


def offset_of(layout):
    """Element offset of the view's first element from a 16-byte boundary (mod what matters)."""
    return layout[1]


class Carved:
    def __init__(self, rows, cols, layout, device, dtype=torch.float32, data=None):
        self.rows, self.cols, self.layout = rows, cols, layout
        if layout[0] == "flat":
            o = layout[1]
            self.buf = torch.empty(o + rows * cols + 9, dtype=dtype, device=device)
            self.view = self.buf[o:o + rows * cols].view(rows, cols)
            self.mask = torch.ones(self.buf.shape, dtype=torch.bool, device=device)
            self.mask[o:o + rows * cols] = False
        else:
            _, o, extra = layout
            assert extra >= o
            self.buf = torch.empty((rows + 2 * GUARD, cols + extra), dtype=dtype, device=device)
            self.view = self.buf[GUARD:GUARD + rows, o:o + cols]
            self.mask = torch.ones(self.buf.shape, dtype=torch.bool, device=device)
            self.mask[GUARD:GUARD + rows, o:o + cols] = False
        esz = self.buf.element_size()
        assert self.buf.data_ptr() % 16 == 0
        self.bits = self.buf.view(_INT[dtype])
        self.bits.fill_(NAN_BITS[dtype])
        if data is not None:
            self.view.copy_(data.to(device=device, dtype=dtype))
        # the geometry the dispatcher will see is the geometry the case's table entry states
        assert self.view.data_ptr() % 16 == (esz * offset_of(layout)) % 16, layout
        if rows > 1:
            assert self.view.stride(0) == ld_of(layout, cols) and self.view.stride(1) == 1
        self.before = self.bits.clone()

    @property
    def ld(self):
        return ld_of(self.layout, self.cols)

    def check_outside(self):
        """No byte outside the view changed since construction."""
        assert torch.equal(self.bits[self.mask], self.before[self.mask]), f"store outside the view ({self.layout})"

    def check_unchanged(self):
        """No byte of the buffer changed at all (inputs; refused calls' outputs)."""
        assert torch.equal(self.bits, self.before), f"buffer written ({self.layout})"


def align_bytes(layout, esz=4):
    """Largest power of two <= 16 dividing the view's pointer."""
    a = (esz * offset_of(layout)) % 16
    for b in (16, 8, 4, 2):
        if a % b == 0:
            return b
    return 1
