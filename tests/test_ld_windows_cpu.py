"""The detectors of tests/ld_windows.py on CPU tensors: a guard check that cannot see a stray byte, or a poison that is not a NaN,
would make every leading-dimension test on the GPU pass for nothing."""
import pytest
import torch

from ld_windows import POISON, SENTINEL, guarded, guards_intact, into_padded, into_poisoned, padded, same_window_bits

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
ROWS, COLS, PAD = 5, 24, 8


def stray_places(view, buf):
    """(name, buffer row, byte column) of one byte in each of the four places a kernel can write outside its window"""
    esz, ld = view.element_size(), buf.shape[1]
    top = (view.data_ptr() - buf.data_ptr()) // ld           # the window's first buffer row
    assert top >= 1 and buf.shape[0] == ROWS + 2 * top
    return [("row above", top - 1, ld - 1), ("row below", top + ROWS, 0), ("pad columns of a middle row", top + 1, COLS * esz),
            ("pad columns of the last row", top + ROWS - 1, ld - 1)]


@pytest.mark.parametrize("dtype", DTYPES + [torch.uint8])
def test_guards_report_one_changed_byte_in_each_place(dtype):
    for pad in (PAD, 4):                                     # 4: a 16-bit window then starts two rows down
        for name, r, c in stray_places(*padded(ROWS, COLS, dtype, pad, device="cpu")):
            view, buf = padded(ROWS, COLS, dtype, pad, device="cpu")
            assert guards_intact(view, buf)
            buf[r, c] ^= 1
            assert not guards_intact(view, buf), f"{dtype}: a changed byte in the {name} went unseen"
            buf[r, c] ^= 1
            assert guards_intact(view, buf)


@pytest.mark.parametrize("dtype", DTYPES)
def test_guards_ignore_the_window(dtype):
    view, buf = padded(ROWS, COLS, dtype, PAD, device="cpu")
    view.copy_(torch.randn(ROWS, COLS).to(dtype))
    view[0, 0], view[ROWS - 1, COLS - 1] = 1.0, -2.0               # the four corners of the window belong to it
    view[0, COLS - 1], view[ROWS - 1, 0] = 3.0, -4.0
    assert guards_intact(view, buf)
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_views_carry_the_padded_leading_dimension(dtype):
    for pad in (4, 8, 16):
        view, buf = padded(ROWS, COLS, dtype, pad, device="cpu")
        assert view.stride(0) == COLS + pad and view.stride(1) == 1 and view.shape == (ROWS, COLS)
        ld, off = (COLS + pad) * view.element_size(), view.data_ptr() - buf.data_ptr()
        spare = 1 if ld % 16 == 0 else 2                     # one spare row above and below; two where one row is not a whole number of 16 bytes
        assert off == spare * ld and off % 16 == 0 and buf.shape == (ROWS + 2 * spare, ld)
    t = torch.randn(ROWS, COLS).to(dtype)
    assert into_padded(t, 16, device="cpu").stride(0) == COLS + 16 and into_poisoned(t, 4, device="cpu").stride(0) == COLS + 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_poison_is_nan_in_every_format_and_the_window_is_the_tensor(dtype):
    t = torch.randn(ROWS, COLS).to(dtype)
    view = into_poisoned(t, PAD, device="cpu")
    assert same_window_bits(view, t) == 0 and torch.equal(view, t)
    ld = COLS + PAD
    top = view.storage_offset() // ld
    whole = torch.as_strided(view, (ROWS + 2 * top, ld), (ld, 1), 0)
    outside = torch.ones(ROWS + 2 * top, ld, dtype=torch.bool)
    outside[top:top + ROWS, :COLS] = False
    assert top >= 1 and bool(torch.isnan(whole[outside]).all()) and int(outside.sum()) == 2 * top * ld + ROWS * PAD
    assert not torch.isnan(whole[~outside]).any()
    assert bool(torch.isnan(torch.full((4,), POISON, dtype=torch.uint8).view(dtype)).all())
    # ... while into_padded's pads are finite: the two runs differ in nothing but what the pads decode to
    calm = into_padded(t, PAD, device="cpu")
    whole = torch.as_strided(calm, (ROWS + 2 * top, ld), (ld, 1), 0)
    assert bool(torch.isfinite(whole.float()).all()) and same_window_bits(calm, t) == 0


def test_guarded_vectors_have_cells_on_both_sides():
    for n in (65, 130, 192, 2 * 2 * 65):
        view, buf = guarded(n, device="cpu")
        assert view.shape == (n,) and view.is_contiguous() and (view.data_ptr() - buf.data_ptr()) % 16 == 0
        view.fill_(1.0)
        assert guards_intact(view, buf)
        flat = buf.view(-1)
        first = view.data_ptr() - buf.data_ptr()
        for at in (first - 1, first + 4 * n):                      # the byte in front of the first cell, the byte behind the last
            flat[at] ^= 1
            assert not guards_intact(view, buf)
            flat[at] ^= 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_window_bits_compares_words(dtype):
    a = torch.randn(ROWS, COLS).to(dtype)
    a[1, 2] = float("nan")
    b = a.clone()
    assert same_window_bits(a, b) == 0                               # a NaN equals itself as a word
    b[3, 4] = -b[3, 4]
    b[0, 0] = 0.0
    a[0, 0] = -0.0                                                   # equal as numbers, different words
    assert same_window_bits(a, b) == 2
    assert same_window_bits(into_padded(a, PAD, device="cpu"), a) == 0         # a strided view against a dense tensor
    with pytest.raises(AssertionError):
        same_window_bits(a, b.float() if dtype != torch.float32 else b.half())
