"""Embedded operands for the leading-dimension tests (tests/test_gpu_strides.py, the contract of
include/gp2d.h "Leading dimensions"): a matrix placed inside a larger sentinel-filled buffer at
the weakest base alignment and the smallest row slack its entry's rule allows, with guard rows
above and below so that a kernel indexing with the row length for the leading dimension still
lands inside the allocation — and shows up as a changed sentinel or a NaN in the result."""
import ctypes

import torch

# one fixed quiet-NaN bit pattern: any arithmetic on it poisons a result, any store over it shows
SENTINEL_BITS = 0x7FF8DEADBEEF0001


def sentinel_buffer(shape, device):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int64, device=device).view(torch.float64)


def is_sentinel(t):
    """Elementwise: does this (row-strided) float64 tensor still hold the sentinel's bits?"""
    return t.view(torch.int64) == SENTINEL_BITS


class Embedded:
    """rows × cols at rows [top, top + rows), columns [c0, c0 + cols) of a sentinel buffer with row
    stride ld.  even = True (an entry that moves 16-byte pairs): c0 = 2 and ld = cols + 4, so the
    base is 16-byte but not 32-byte aligned and rows are neither 64- nor 128-byte aligned.
    even = False (8-byte accesses only): c0 = 1 and the smallest slack >= 1 that makes ld odd, so
    the base and every second row are only 8-byte aligned.  top = rows + 1: `rows` guard rows and
    the row offset r0 = 1 (2 where that is what puts the odd-ld base off a 16-byte boundary);
    `rows` guard rows below."""

    def __init__(self, rows, cols, even, device, fill=None, extra=0):
        assert extra % 4 == 0   # further slack (to tell two operands' leading dimensions apart)
        self.rows, self.cols = rows, cols
        self.c0 = 2 if even else 1
        self.ld = cols + self.c0 + (2 if even else (1 if (cols + self.c0 + 1) % 2 else 2)) + extra
        self.top = rows + 1
        if not even and self.top % 2:   # an even row count above keeps the odd-ld base off 16 bytes
            self.top += 1
        self.buf = sentinel_buffer((self.top + 2 * rows, self.ld), device)
        assert self.buf.data_ptr() % 32 == 0   # the alignment asserted below is the view's own
        self.view = self.buf[self.top:self.top + rows, self.c0:self.c0 + cols]
        if fill is not None:
            self.view.copy_(fill)
        align = self.view.data_ptr() % (32 if even else 16)
        assert align == (16 if even else 8) and self.ld % 2 == (0 if even else 1), (align, self.ld)
        self.mask = torch.ones(self.buf.shape, dtype=torch.bool, device=device)
        self.mask[self.top:self.top + rows, self.c0:self.c0 + cols] = False

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def assert_slack_intact(self):
        """No word outside the block changed (the buffer started as sentinel everywhere there)."""
        assert bool(is_sentinel(self.buf)[self.mask].all()), "a sentinel outside the embedded block was overwritten"


def embed(mat, even, fill=True, extra=0):
    """`mat` (2-D device tensor) embedded; fill = False leaves the block sentinel too (an output)."""
    return Embedded(mat.shape[0], mat.shape[1], even, mat.device, mat if fill else None, extra)


def same_bits(a, b):
    """Bitwise equality of two tensors of one shape (NaN-safe: float64 compared as int64)."""
    if a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return a.shape == b.shape and torch.equal(a, b)


def assert_unchanged(buf, before):
    """No word of `buf` differs from `before`, a clone taken before the call."""
    assert same_bits(buf, before), "a word outside the operand changed"
