"""The row-per-lane dense kernel (``linear_rowlane_kernel<34>``, csrc/dense.hip) at the row counts and layouts the model
never gives it, and the neighbouring calls that must leave it, against float64.

``mpx_linear`` takes the kernel for N = 128, K = 68 without bias or activation, an even ldx, ldy % 4 == 0 and aligned
operands, from 9 rows on; ``launch_routes.linear_form`` asks the library itself (``mpx_linear_form``: the launcher's own
predicates).  The launch is 4 waves per CU, each walking 32-row tiles with a static stride of the grid ``W = 4 cus`` and
requesting its next tile before the current one's matrix instructions; rows past M in the last tile read row M - 1 and are
not stored.  The row counts: one ragged tile (9, 31), one full tile, one row more (33), three tiles (95), every wave one tile
(32 W), one wave a second 1-row tile (32 W + 1), three uneven passes with a ragged end (32 (2 W + 5) + 7).

Every case: the library reports the row-lane form; every element lies within ``float64_linear.bar`` of the float64 product
(the worst case of a 68-term fp32 sum, no margin); the padding columns of x hold NaN, so a read past K poisons a row; the 40
rows below y and the columns beside it keep their sentinel; a second run gives the same bits; and rows 0..8 equal, bit for
bit, the 9-row call on the same rows -- the "same rounding order for every M" of the kernel's comment."""
import functools

import numpy as np
import pytest
import torch

import float64_linear as fl
from float64_policy import cu_count
from launch_routes import linear_form

pytestmark = pytest.mark.gpu

N, K = fl.N_OUT, fl.K_IN
SENTINEL = -12345.0
EXTRA_ROWS = 40
DROP_K = 8  # the column of w with the largest smallest entry: the dropped product is far over the bar in every column

# row counts, as functions of the launch's grid W = 4 cus
ROWS = {"9": lambda W: 9, "31": lambda W: 31, "32": lambda W: 32, "33": lambda W: 33, "95": lambda W: 95,
        "32W": lambda W: 32 * W, "32W+1": lambda W: 32 * W + 1, "32(2W+5)+7": lambda W: 32 * (2 * W + 5) + 7}
LARGEST = "32(2W+5)+7"
# name -> (ldx, first float of x in its buffer, row length of y's buffer, first column of y in it)
LAYOUTS = {"68/128": (68, 0, 128, 0), "72/132": (72, 0, 132, 0), "76/128": (76, 0, 128, 0),
           "x+16B": (68, 4, 128, 0), "y-slice": (68, 0, 136, 4)}
CASES = [(m, "68/128") for m in ROWS] + [(m, lay) for m in ("95", "32W+1") for lay in LAYOUTS if lay != "68/128"]
# the calls that must leave the form: name -> (rows, K, bias, act, ldy, first column of y, the route, DMA staging)
NEIGHBOURS = {"bias": (95, 68, True, fl.ACT_NONE, 128, 0, "tile", False),
              "relu": (95, 68, False, fl.ACT_RELU, 128, 0, "tile", False),
              "leaky": (95, 68, False, fl.ACT_LEAKY, 128, 0, "tile", False),
              "ldy130": (95, 68, False, fl.ACT_NONE, 130, 0, "tile", False),
              "y+4B": (95, 68, False, fl.ACT_NONE, 132, 1, "tile", False),
              "M8": (8, 68, False, fl.ACT_NONE, 128, 0, "gemv", False),
              "K64": (95, 64, False, fl.ACT_NONE, 128, 0, "tile", True)}
SEEN = {}  # case -> (rowlane, dma) as the library reported them (test_cases_take_and_leave_both_forms)


def grid():
    return 4 * cu_count()


@functools.lru_cache(maxsize=None)
def problem(M, k=K, bias=False, act=fl.ACT_NONE):
    """-> x, w, bias, float64 reference and bar: made once per shape, shared and read-only."""
    x, w = fl.make_x(M, k), fl.make_w(N, k)
    b = fl.make_bias() if bias else None
    out = (x, w, b, fl.reference(x, w, b, act), fl.bar(x, w, b, act))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def run(x, w, bias, act, ldx, xoff, ldy, ycol):
    """One ``mpx_linear`` call on x laid out with row length ldx (NaN in the padding) ``xoff`` floats into its buffer, into
    columns [ycol, ycol + N) of a sentinel-filled [M + 40, ldy] buffer -> (the whole buffer as numpy, the library's form)."""
    from mpinets_amd import _lib

    dev = torch.device("cuda:0")
    M, k = x.shape
    xbuf = torch.full((xoff + M * ldx,), float("nan"), dtype=torch.float32, device=dev)
    xd = xbuf[xoff:].view(M, ldx)
    xd[:, :k] = torch.tensor(x).to(dev)
    wd = torch.tensor(w).to(dev)
    bd = None if bias is None else torch.tensor(bias).to(dev)
    ybuf = torch.full((M + EXTRA_ROWS, ldy), SENTINEL, dtype=torch.float32, device=dev)
    yp = ybuf.data_ptr() + 4 * ycol
    assert xd.data_ptr() % 16 == 0 and ybuf.data_ptr() % 16 == 0 and ycol + N <= ldy
    args = (xd.data_ptr(), ldx, wd.data_ptr(), _lib.ptr(bd), M, N, k, act, yp, ldy)
    form = linear_form(*args)
    _lib.call("mpx_linear", *args)
    torch.cuda.synchronize()
    return ybuf.cpu().numpy(), form


def split(buf, M, ycol):
    """-> y [M,N] and whether everything else of the buffer still holds the sentinel."""
    rest = buf.copy()
    rest[:M, ycol:ycol + N] = SENTINEL
    return buf[:M, ycol:ycol + N], bool((rest == np.float32(SENTINEL)).all())


@functools.lru_cache(maxsize=None)
def nine_rows(layout):
    """The 9-row call of a layout (the reference of the leading rows of every larger call)."""
    ldx, xoff, ldy, ycol = LAYOUTS[layout]
    x, w = problem(9)[:2]
    buf, form = run(x, w, None, fl.ACT_NONE, ldx, xoff, ldy, ycol)
    assert form == ("tile", True, False)
    y, clean = split(buf, 9, ycol)
    assert clean
    return y.copy()


@pytest.mark.parametrize("rows,layout", CASES, ids=[f"M{m}-{lay}" for m, lay in CASES])
def test_rowlane_against_float64(rows, layout):
    M = ROWS[rows](grid())
    ldx, xoff, ldy, ycol = LAYOUTS[layout]
    x, w, _, ref, bar = problem(M)
    buf, form = run(x, w, None, fl.ACT_NONE, ldx, xoff, ldy, ycol)
    SEEN[rows, layout] = form[1:]
    assert form == ("tile", True, False), form  # the row-per-lane kernel, no tile kernel behind it
    y, clean = split(buf, M, ycol)
    bad, worst = fl.offending_rows(y, ref, bar)
    print(f"ROWLANE M={M} ({rows}, W={grid()}) {layout}: largest err / bar = {worst:.4f}, rows over the bar: {len(bad)}")
    assert bad == set(), sorted(bad)[:20]
    assert (y[1] == 0).all()
    assert clean, "a row past M or a column beside y was written"
    again, _ = run(x, w, None, fl.ACT_NONE, ldx, xoff, ldy, ycol)
    assert np.array_equal(buf.view(np.uint32), again.view(np.uint32)), "a second run gave other bits"
    assert np.array_equal(y[:9].view(np.uint32), nine_rows(layout).view(np.uint32)), "rows 0..8 differ from the 9-row call"
    print(f"ROWLANE M={M} {layout}: second run and rows 0..8 vs the 9-row call bit-equal")
    if rows == LARGEST and layout == "68/128":
        # the comparator sees a defect planted into THIS output: a product dropped from a row of the ragged last tile,
        # and two rows swapped that sit 32 apart (the same lane of two tiles)
        last = M - 1 - int(np.argmax(np.abs(x[M - 7:, DROP_K])[::-1]))
        assert M - 7 <= last < M and fl.dropped_over_bar(x, w, bar, last, DROP_K) > 2.0
        assert fl.offending_rows(fl.drop_term(y, x, w, last, DROP_K), ref, bar)[0] == {last}
        r = 32 * (grid() + 3) + 11
        assert fl.offending_rows(fl.swap_rows(y, r, r + 32), ref, bar)[0] == {r, r + 32}
        print(f"ROWLANE M={M}: planted controls flag rows {{{last}}} and {{{r}, {r + 32}}} exactly")


@pytest.mark.parametrize("name", list(NEIGHBOURS))
def test_neighbours_leave_the_rowlane_form(name):
    M, k, with_bias, act, ldy, ycol, route, dma = NEIGHBOURS[name]
    x, w, bias, ref, bar = problem(M, k, with_bias, act)
    buf, form = run(x, w, bias, act, k, 0, ldy, ycol)
    SEEN[name] = form[1:]
    assert form == (route, False, dma), form
    y, clean = split(buf, M, ycol)
    bad, worst = fl.offending_rows(y, ref, bar)
    print(f"ROWLANE neighbour {name}: form {form}, largest err / bar = {worst:.4f}")
    assert bad == set(), sorted(bad)[:20]
    assert clean, "a row past M or a column beside y was written"


def test_cases_take_and_leave_both_forms():
    """The cases above, asked of the library without a launch: the row-per-lane form and the DMA staging are each seen on
    and off, and each row count is what its name says on this device."""
    W = grid()
    seen = {}
    for rows, layout in CASES:
        ldx, xoff, ldy, ycol = LAYOUTS[layout]
        seen[rows, layout] = linear_form(4096 + 4 * xoff, ldx, 8192, None, ROWS[rows](W), N, K, fl.ACT_NONE, 16384 + 4 * ycol, ldy)[1:]
    for name, (M, k, with_bias, act, ldy, ycol, _, _) in NEIGHBOURS.items():
        seen[name] = linear_form(4096, k, 8192, 12288 if with_bias else None, M, N, k, act, 16384 + 4 * ycol, ldy)[1:]
    for key, forms in SEEN.items():  # what the launching tests saw with real addresses, where they ran
        assert seen[key] == forms, key
    print("\n".join(f"  {key}: rowlane {'on' if r else 'off'}, dma {'on' if d else 'off'}" for key, (r, d) in seen.items()))
    assert {r for r, _ in seen.values()} == {False, True} and {d for _, d in seen.values()} == {False, True}
    assert all(seen[c] == (True, False) for c in CASES) and not any(seen[n][0] for n in NEIGHBOURS)
    tiles = lambda m: -(-ROWS[m](W) // 32)  # noqa: E731
    assert tiles("32W") == W and tiles("32W+1") == W + 1 and ROWS["32W+1"](W) % 32 == 1
    assert 2 * W < tiles(LARGEST) < 3 * W and tiles(LARGEST) % W not in (0, 1) and ROWS[LARGEST](W) % 32 == 7
