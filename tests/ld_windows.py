"""Leading dimensions and write windows: the buffers every "honours its ld" test is built from (tests/test_fp8_kernels_gpu.py,
tests/test_ld_windows_gpu.py; checked on the CPU by tests/test_ld_windows_cpu.py).

A kernel's 2-D operand or output is handed over as a [rows, cols] VIEW of a wider byte buffer with one spare row above, one below
and pad_cols spare columns behind every row - so its leading dimension is cols + pad_cols, and whatever the kernel stores outside
[rows, cols] (a ragged last tile, a wrong ld in a bound) lands in bytes the test looks at instead of in allocator slack.

  padded         an output window: every byte of the buffer is SENTINEL
  into_padded    an input: a copy of a tensor inside such a buffer (finite pads)
  into_poisoned  an input whose spare rows and pad columns are byte 0xFF: NaN in bf16, fp16 and fp32, so a pad cell that reaches
                 arithmetic and then a stored output shows up deterministically
  guards_intact  no byte outside the window changed
  guarded        a 1-D output (row statistics, column sums) with guard cells on both sides
  same_window_bits  two tensors word for word (NaN cells compare as words)"""
import torch

SENTINEL = 0xA5
POISON = 0xFF


def padded(rows, cols, dtype, pad_cols=8, device="cuda", fill=SENTINEL):
    """([rows, cols] view of a sentinel-filled buffer with spare rows above and below and pad_cols spare columns, the buffer).  One spare
    row on either side wherever a row is a whole number of 16-byte pieces (every fp8 and fp32 case, 16-bit rows with ld % 8 == 0);
    where it is not (a 16-bit ld that is only a multiple of 4) as many as put the window's first cell on a 16-byte boundary, where a
    fresh allocation would put it - the kernels check the alignment of the base pointers they are given."""
    esz = torch.empty((), dtype=dtype).element_size()
    ld = (cols + pad_cols) * esz
    spare = next(s for s in (1, 2, 4, 8, 16) if s * ld % 16 == 0)
    buf = torch.full((rows + 2 * spare, ld), fill, dtype=torch.uint8, device=device)
    return buf.view(dtype)[spare:spare + rows, :cols], buf


def guards_intact(view, buf):
    """no byte of buf outside the window `view` (from padded, or 1-D from guarded) differs from the sentinel"""
    rows, cols = view.shape if view.dim() == 2 else (1, view.numel())
    top = (view.data_ptr() - buf.data_ptr()) // buf.stride(0)
    assert (view.data_ptr() - buf.data_ptr()) % buf.stride(0) == 0 and top + rows <= buf.shape[0]
    b = buf.clone()
    b[top:top + rows, :cols * view.element_size()] = SENTINEL
    return bool((b == SENTINEL).all())


def into_padded(t, pad_cols, device="cuda"):
    """a copy of the 2-D tensor t as a view into a wider sentinel-filled buffer"""
    view, _ = padded(t.shape[0], t.shape[1], t.dtype, pad_cols, device)
    view.copy_(t)
    return view


def into_poisoned(t, pad_cols, device="cuda"):
    """into_padded with the spare row above, the spare row below and the pad columns filled with byte 0xFF (NaN in bf16, fp16 and fp32)"""
    view, _ = padded(t.shape[0], t.shape[1], t.dtype, pad_cols, device, fill=POISON)
    view.copy_(t)
    return view


def guarded(n, dtype=torch.float32, device="cuda"):
    """(1-D view of n cells with at least four sentinel cells on either side, 16-byte aligned like a fresh allocation; the buffer)"""
    assert torch.empty((), dtype=dtype).element_size() == 4
    view, buf = padded(1, n, dtype, 4 + (-n) % 4, device)
    return view[0], buf


def same_window_bits(a, b):
    """number of cells whose words differ between two tensors of one shape and dtype (NaN cells included: the words compare)"""
    assert a.shape == b.shape and a.dtype == b.dtype, f"shape / dtype: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    wa, wb = (t.contiguous().view(torch.uint8).reshape(t.numel(), -1) for t in (a, b))
    return int((wa != wb).any(1).sum())
