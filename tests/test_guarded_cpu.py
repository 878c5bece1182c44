"""tests/guarded.py on CPU tensors: every region's violation is detected and located, an untouched buffer passes, and the interior
view has the shape, stride and alignment the C ABI asks for."""
import math

import pytest
import torch

from guarded import BACK_ROWS, FRONT_BYTES, Guarded

DTYPES = [torch.float32, torch.bfloat16]


def _flip(g: Guarded, flat_index: int) -> None:
    g.bits[flat_index] = g.bits[flat_index] ^ 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,ld", [(5, 12, 20), (1, 8, 8), (130, 132, 140)])
def test_interior_view(dtype, rows, cols, ld):
    g = Guarded.output(rows, cols, ld, dtype, "cpu")
    assert g.t.shape == (rows, cols) and g.t.stride() == (ld, 1) and g.t.dtype == dtype
    assert g.ptr() % 16 == 0
    assert g.ptr() - g.raw.data_ptr() == FRONT_BYTES
    es = g.esize
    assert g.raw.numel() * es - FRONT_BYTES - rows * ld * es == max(64 * 1024, BACK_ROWS * ld * es)
    assert g.untouched_interior() == rows * cols
    g.check("fresh")


@pytest.mark.parametrize("dtype", DTYPES)
def test_untouched_buffer_passes_and_interior_writes_are_free(dtype):
    g = Guarded.output(7, 12, 20, dtype, "cpu")
    g.t.copy_(torch.randn(7, 12).to(dtype))
    assert g.violation() is None
    assert g.untouched_interior() == 0
    old = torch.randn(7, 12).to(dtype)
    g2 = Guarded.output(7, 12, 20, dtype, "cpu", old=old)
    assert torch.equal(g2.t, old) and g2.violation() is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_region_is_detected_and_located(dtype):
    rows, cols, ld = 9, 12, 20
    # front guard: the element just in front of the matrix, and the very first one
    for off in (1, None):
        g = Guarded.output(rows, cols, ld, dtype, "cpu")
        idx = g.front - off if off else 0
        _flip(g, idx)
        assert g.violation() == ("front", None, idx)
        with pytest.raises(AssertionError, match="front guard"):
            g.check("front")
    # a pad column of the first, a middle and the last row
    for r, c in ((0, cols), (4, ld - 1), (rows - 1, cols + 3)):
        g = Guarded.output(rows, cols, ld, dtype, "cpu")
        _flip(g, g.front + r * ld + c)
        assert g.violation() == ("pad", r, c)
        with pytest.raises(AssertionError, match=f"row {r}, col {c} "):
            g.check("pad")
    # back guard: one row too far (first element behind the matrix), eight columns into it, and the last element
    for off in (0, 8, None):
        g = Guarded.output(rows, cols, ld, dtype, "cpu")
        idx = g.front + g.body + off if off is not None else g.raw.numel() - 1
        _flip(g, idx)
        assert g.violation() == ("back", None, idx - g.front - g.body)
        with pytest.raises(AssertionError, match="back guard"):
            g.check("back")
    # the first offender in memory order is the one reported
    g = Guarded.output(rows, cols, ld, dtype, "cpu")
    _flip(g, g.front + 6 * ld + cols + 1)
    _flip(g, g.front + 2 * ld + cols + 5)
    assert g.violation() == ("pad", 2, cols + 5)
    # a value written over the sentinel (not only a flipped bit) is seen as well, zero included
    g = Guarded.output(rows, cols, ld, dtype, "cpu")
    g.raw[g.front + g.body] = 0.0
    assert g.violation() == ("back", None, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_input_form_and_vectors(dtype):
    data = torch.randn(6, 10).to(dtype)
    g = Guarded.input(data, 18)
    assert torch.equal(g.t, data) and g.t.stride() == (18, 1) and g.ptr() % 16 == 0
    assert bool(torch.isnan(g.raw[:g.front]).all()) and bool(torch.isnan(g.raw[g.front + g.body:]).all())
    body = g.raw[g.front:g.front + g.body].view(6, 18)
    assert bool(torch.isnan(body[:, 10:]).all()) and not bool(torch.isnan(body[:, :10]).any())
    v = Guarded.input(torch.randn(37).to(dtype))
    assert v.vec().shape == (37,) and bool(torch.isnan(v.raw[v.front - 1])) and bool(torch.isnan(v.raw[v.front + 37]))
    o = Guarded.output_vec(37, dtype, "cpu")
    o.vec()[:] = 1.0
    o.check("vector")
    o.raw[o.front + 37] = 1.0
    assert o.violation() == ("back", None, 0)
    with pytest.raises(AssertionError):
        Guarded.input(data, 18).check("inputs carry no sentinel")


def test_workspace_of_exact_bytes():
    w = Guarded.output_bytes(1000, "cpu")
    assert w.t.numel() == 1000 and w.ptr() % 16 == 0
    w.t.fill_(0)
    w.check("workspace")
    w.raw[w.front + 1000] = 0
    assert w.violation() == ("back", None, 0)
    assert Guarded.output_bytes(0, "cpu").t.numel() == 1


def test_sentinels_are_nans_with_a_payload():
    for dtype in DTYPES:
        g = Guarded.output(1, 8, 8, dtype, "cpu")
        assert bool(torch.isnan(g.raw).all())
        assert math.isnan(float(g.raw[0]))
