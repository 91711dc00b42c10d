"""Positive controls of the guard-band harness (tests/footprint.py), on the CPU.

Plain torch "kernels" that take what the C ABI takes -- a flat buffer, the element offset of the
logical origin, sizes and row strides -- run against Boxes; each planted fault must be reported, at
the right (row, col), and the correct kernel must pass clean.  This is what shows that the checks
of test_gpu_footprint.py can fail: turn any planted fault back into the correct kernel and its
control fails.
"""
import pytest
import torch

from footprint import Box, WsBox

# (dtype, ld - cols, offset_bytes): tight and aligned, padded, odd stride on a shifted base
LAYOUTS = [(torch.float32, 0, 0), (torch.float32, 8, 16), (torch.float32, 3, 4), (torch.bfloat16, 8, 0),
           (torch.bfloat16, 1, 2), (torch.int64, 5, 8)]
ROWS, COLS = 40, 21


def _arg(box):
    """The "pointer" a kernel gets: flat storage and the origin's element offset."""
    return box._flat, box.origin


def k_double(x, ldx, y, ldy, rows, cols, fault=None):
    """y[r, c] = 2 x[r, c], element (r, c) at base + r*ld + c; `fault` plants one footprint error."""
    (xf, xo), (yf, yo) = x, y
    for r in range(rows):
        yf[yo + r * ldy: yo + r * ldy + cols] = xf[xo + r * ldx: xo + r * ldx + cols] * 2
    if fault == "past_row_end":          # a vector store that crosses the end of row 37
        yf[yo + 37 * ldy + cols] = 1
    elif fault == "past_last_row":       # a tail tile that stores one row too many
        yf[yo + rows * ldy: yo + rows * ldy + cols] = 1
    elif fault == "front_guard":         # an index that went negative
        yf[yo - 1] = 1
    elif fault == "touch_input":         # scribbling on a const operand
        xf[xo + 5 * ldx + 3] += 1


def k_rowsum(x, ldx, out, rows, cols, ws=None, fault=None):
    """out[r] = sum_c x[r, c] in fp32 through a one-float-per-row workspace."""
    (xf, xo), (of, oo) = x, out
    width = cols + 1 if fault == "read_wide" else cols
    wsf = ws.view[0, :rows * 4].view(torch.float32) if ws is not None else torch.zeros(rows)
    for r in range(rows):
        s = xf[xo + r * ldx: xo + r * ldx + width].float().sum()
        if fault == "ws_accumulate":     # += into a partial nobody zeroed
            wsf[r] += s
        else:
            wsf[r] = s
        of[oo + r] = wsf[r]


def _boxes(dtype, pad, off):
    g = torch.Generator().manual_seed(0)
    data = torch.randint(1, 50, (ROWS, COLS), generator=g).to(dtype)
    kw = {"pad": 0} if not dtype.is_floating_point else {}
    x = Box(ROWS, COLS, dtype, ld=COLS + pad, offset_bytes=off, **kw).fill(data).snapshot()
    y = Box(ROWS, COLS, dtype, ld=COLS + pad + 2, offset_bytes=off)
    return data, x, y


@pytest.mark.parametrize("dtype,pad,off", LAYOUTS)
def test_correct_kernel_passes_every_check(dtype, pad, off):
    data, x, y = _boxes(dtype, pad, off)
    res = []
    for how in ("nan", "zero"):
        y.prefill(how)
        k_double(_arg(x), x.ld, _arg(y), y.ld, ROWS, COLS)
        assert torch.equal(y.view, data * 2)
        y.assert_clean("y")
        x.assert_unchanged("x")
        assert x.unchanged() and y.stray().shape == (0, 2)
        res.append(y.bits())
    assert torch.equal(*res)


@pytest.mark.parametrize("dtype,pad,off", LAYOUTS)
def test_write_past_row_end_is_reported(dtype, pad, off):
    _, x, y = _boxes(dtype, pad, off)
    k_double(_arg(x), x.ld, _arg(y), y.ld, ROWS, COLS, fault="past_row_end")
    assert y.stray().tolist() == [[37, COLS]]
    with pytest.raises(AssertionError, match=rf"y \[40 x 21, ld {y.ld}\].*\(row 37, col {COLS}\)"):
        y.assert_clean("y")


@pytest.mark.parametrize("dtype,pad,off", LAYOUTS)
def test_write_past_last_row_is_reported(dtype, pad, off):
    _, x, y = _boxes(dtype, pad, off)
    k_double(_arg(x), x.ld, _arg(y), y.ld, ROWS, COLS, fault="past_last_row")
    assert y.stray().tolist() == [[ROWS, c] for c in range(COLS)]
    with pytest.raises(AssertionError, match=rf"\(row {ROWS}, col 0\).* and {COLS - 6} more"):
        y.assert_clean("y")


@pytest.mark.parametrize("dtype,pad,off", LAYOUTS)
def test_write_into_front_guard_is_reported(dtype, pad, off):
    _, x, y = _boxes(dtype, pad, off)
    k_double(_arg(x), x.ld, _arg(y), y.ld, ROWS, COLS, fault="front_guard")
    assert y.stray().tolist() == [[-1, y.ld - 1]]


@pytest.mark.parametrize("dtype,pad,off", LAYOUTS)
def test_modified_const_input_is_reported(dtype, pad, off):
    _, x, y = _boxes(dtype, pad, off)
    k_double(_arg(x), x.ld, _arg(y), y.ld, ROWS, COLS, fault="touch_input")
    assert not x.unchanged() and x.changed().tolist() == [[5, 3]]
    with pytest.raises(AssertionError, match=r"const operand modified at \(row 5, col 3\)"):
        x.assert_unchanged("x")
    y.assert_clean("y")


@pytest.mark.parametrize("dtype,pad,off", [l for l in LAYOUTS if l[0].is_floating_point])
def test_wide_read_reaches_the_result(dtype, pad, off):
    """Reading cols + 1 elements of a row takes in the padding (or, at ld == cols, the next row and
    after the last row the guard): the poison is a NaN in fp32 and in bf16, so the sum is one."""
    data, x, _ = _boxes(dtype, pad, off)
    out = Box(1, ROWS, torch.float32)
    k_rowsum(_arg(x), x.ld, _arg(out), ROWS, COLS)
    assert torch.equal(out.view[0], data.float().sum(1))
    out.prefill("nan")
    k_rowsum(_arg(x), x.ld, _arg(out), ROWS, COLS, fault="read_wide")
    bad = torch.isnan(out.view[0])
    assert bad[ROWS - 1] and (bad.all() if pad else bad.sum() == 1)
    out.assert_clean("out")
    x.assert_unchanged("x")


def test_integer_input_padding_is_a_valid_index():
    """An over-read of an integer input sees the pad value -- a valid index, never the out-of-range
    poison of integer outputs -- and still changes the answer."""
    idx = Box(1, 9, torch.int64, ld=12, pad=3).fill(torch.arange(9) % 3)
    assert int(idx._flat.max()) == 3 and int(idx._flat.min()) >= 0
    table = torch.arange(4.0) * 10
    assert float(table[idx._flat[idx.origin: idx.origin + 9]].sum()) == 90.0
    assert float(table[idx._flat[idx.origin: idx.origin + 10]].sum()) == 120.0     # one past: pad = 3
    out = Box(1, 9, torch.int64)
    assert int(out._flat.min()) > 2 ** 60        # an output's poison is out of range on purpose


@pytest.mark.parametrize("nbytes", [ROWS * 4, ROWS * 4 + 3])
def test_workspace_read_before_write_differs_between_prefills(nbytes):
    data, x, _ = _boxes(torch.float32, 4, 0)
    res = {}
    for fault in (None, "ws_accumulate"):
        for how in ("nan", "zero", "ones"):
            ws = WsBox(nbytes, how)
            out = Box(1, ROWS, torch.float32)
            k_rowsum(_arg(x), x.ld, _arg(out), ROWS, COLS, ws=ws, fault=fault)
            ws.assert_clean("ws")
            out.assert_clean("out")
            res[fault, how] = out.bits()
    assert torch.equal(res[None, "nan"], res[None, "zero"]) and torch.equal(res[None, "nan"], res[None, "ones"])
    assert torch.equal(res[None, "zero"][0].view(torch.float32), data.float().sum(1))
    assert torch.equal(res["ws_accumulate", "zero"], res[None, "zero"])       # zeros hide the fault ...
    assert not torch.equal(res["ws_accumulate", "nan"], res[None, "nan"])     # ... NaN and 0xFF show it
    assert not torch.equal(res["ws_accumulate", "ones"], res["ws_accumulate", "zero"])


def test_workspace_overrun_is_reported():
    ws = WsBox(1001, "zero")
    assert ws.view.shape == (1, 1001) and ws.nbytes == 1001
    ws._flat[ws.origin + 1001] = 7           # one byte past what *_workspace() returned
    assert ws.stray().tolist() == [[0, 1001]]
    with pytest.raises(AssertionError, match=r"\(row 0, col 1001\)"):
        ws.assert_clean("ws")


def test_poison_survives_fp32_bf16_conversion_and_guards_hold_a_tile():
    for dt, other in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)):
        b = Box(3, 5, dt, ld=9, offset_bytes=4)
        assert torch.isnan(b._flat).all() and torch.isnan(b._flat.to(other)).all()
        isz = b._flat.element_size()
        assert b.origin >= 256 * b.ld + 4096 // isz
        assert b._flat.numel() - (b.origin + 3 * b.ld) >= 256 * b.ld + 4096 // isz
        assert (b.view.data_ptr() - b._raw.data_ptr()) % 256 == 4
    with pytest.raises(ValueError):
        Box(3, 5, torch.float32, offset_bytes=2)
