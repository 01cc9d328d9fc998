"""CPU: the float64 reference of ``mpx_linear``, its bar and its comparator (tests/float64_linear.py) hold on their own.

Two float32 emulations of the sum -- ascending k with rounded products, and the row-per-lane kernel's documented order of
(k, k + 34) pairs -- lie inside the bar at every element of the GPU test's own data, so the bar is not tighter than fp32
arithmetic; the two planted defects lie outside it and are attributed to exactly the planted rows, so it is not looser than
the defects the GPU test must see."""
import ctypes

import numpy as np
import pytest

import float64_linear as fl

M = 95               # three 32-row tiles, the last one ragged: a shape of tests/test_gpu_linear_rowlane.py
ROW = 40             # the planted row, picked with the data seeds: see test_planted_defects_are_outside_the_bar
DROP_K = (0, 33, 34, 67)  # the first and the last k of both halves of a lane's row


@pytest.fixture(scope="module")
def data():
    x, w = fl.make_x(M), fl.make_w()
    ref, bar = fl.reference(x, w), fl.bar(x, w)
    for a in (x, w, ref, bar):
        a.setflags(write=False)
    return x, w, ref, bar


def test_generator_makes_what_the_gpu_test_states(data):
    x, w, ref, bar = data
    assert x.dtype == w.dtype == np.float32 and x.shape == (M, fl.K_IN) and w.shape == (fl.N_OUT, fl.K_IN)
    assert (x[1] == 0).all() and (ref[1] == 0).all() and (bar[1] == 0).all()
    assert np.abs(x[2, 0::2]).max() > 1e3 and 0 < np.abs(x[2, 1::2]).max() < 1e-3
    np.testing.assert_array_equal(fl.make_x(9), x[:9])  # the leading rows do not depend on M
    assert 0.5 < x[3:].std() < 1.5 and 0.5 < w.std() * np.sqrt(fl.K_IN) < 1.5
    assert fl.gamma(68) == pytest.approx(68 * 2.0 ** -24, rel=1e-5) and fl.gamma(68) > 68 * 2.0 ** -24


def test_both_summation_orders_lie_within_the_bar(data):
    x, w, ref, bar = data
    a, b = fl.ascending_f32(x, w), fl.rowlane_order_f32(x, w)
    assert a.dtype == b.dtype == np.float32 and not np.array_equal(a, b)  # (two orders: two roundings)
    for name, got in (("ascending", a), ("rowlane order", b)):
        rows, worst = fl.offending_rows(got, ref, bar)
        print(f"LINEARREF {name}: largest err / bar = {worst:.4f}")
        assert rows == set() and worst <= 1.0
        assert (got[1] == 0).all()
    # with a bias and each activation: one and two more terms
    bias = fl.make_bias()
    for act in (fl.ACT_NONE, fl.ACT_RELU, fl.ACT_LEAKY):
        z = a + bias[None, :]
        got = {fl.ACT_NONE: z, fl.ACT_RELU: np.maximum(z, np.float32(0)),
               fl.ACT_LEAKY: np.where(z >= 0, z, z * np.float32(0.01))}[act]
        assert got.dtype == np.float32
        rows, worst = fl.offending_rows(got, fl.reference(x, w, bias, act), fl.bar(x, w, bias, act))
        print(f"LINEARREF ascending + bias, act {act}: largest err / bar = {worst:.4f}")
        assert rows == set() and worst <= 1.0


def test_planted_defects_are_outside_the_bar(data):
    x, w, ref, bar = data
    good = fl.rowlane_order_f32(x, w)
    for k in DROP_K:
        # not vacuous: the dropped product is over twice the bar in EVERY column (float32's rounding of the edited row is
        # below bar / 68), so every column of the planted row is wrong
        assert fl.dropped_over_bar(x, w, bar, ROW, k) > 2.0, k
        bad = fl.drop_term(good, x, w, ROW, k)
        assert bad.dtype == np.float32 and (np.abs(bad[ROW].astype(np.float64) - ref[ROW]) > bar[ROW]).all()
        assert fl.offending_rows(bad, ref, bar)[0] == {ROW}, k
    assert fl.offending_rows(fl.swap_rows(good, ROW, ROW + 32), ref, bar)[0] == {ROW, ROW + 32}
    assert fl.offending_rows(good, ref, bar)[0] == set()  # (the copies were edited, not the output)


def test_form_query_answers_on_the_host():
    """``mpx_linear_form`` needs no GPU and touches no operand (the addresses here are made up): it names the row-per-lane
    form for exactly the operands ``mpx_linear`` documents, and refuses what ``mpx_linear`` refuses."""
    from mpinets_amd import _lib

    from launch_routes import linear_form

    X, W, Bi, Y = 4096, 8192, 12288, 16384
    on = ("tile", True, False)
    assert linear_form(X, 68, W, None, 9, 128, 68, 0, Y, 128) == on
    assert linear_form(X + 16, 72, W, None, 1 << 20, 128, 68, 0, Y + 16, 132) == on
    assert linear_form(X, 68, W, None, 8, 128, 68, 0, Y, 128) == ("gemv", False, False)
    for args in ((X, 68, W, Bi, 95, 128, 68, 0, Y, 128), (X, 68, W, None, 95, 128, 68, 1, Y, 128), (X, 68, W, None, 95, 128, 68, 2, Y, 128),
                 (X, 68, W, None, 95, 128, 68, 0, Y, 130), (X, 68, W, None, 95, 128, 68, 0, Y + 4, 132),
                 (X, 68, W, None, 95, 128, 68, 0, Y + 8, 132), (X, 68, W, None, 95, 64, 68, 0, Y, 128)):
        assert linear_form(*args) == ("tile", False, False), args
    assert linear_form(X, 64, W, None, 95, 128, 64, 0, Y, 128) == ("tile", False, True)      # K % 16 == 0: DMA staging
    assert linear_form(X, 64, W, None, 8, 128, 64, 0, Y, 128) == ("gemv", False, False)     # ... of a tile kernel only
    lib = _lib.load()
    out = (ctypes.c_int32 * 3)(7, 7, 7)
    for args, word in (((X, 70, W, None, 95, 128, 68, 0, Y, 128), b"multiples of 4"), ((X + 8, 68, W, None, 95, 128, 68, 0, Y, 128), b"aligned"),
                       ((X, 68, W, None, 95, 128, 68, 3, Y, 128), b"activation"), ((X, 68, W, None, 0, 128, 68, 0, Y, 128), b"no rows"),
                       ((X, 68, W, None, 95, 128, 68, 0, Y, 127), b"leading dimension")):
        assert lib.mpx_linear_form(*args, out) != 0 and word in lib.mpx_last_error(), args
    assert list(out) == [7, 7, 7]  # a refused query writes nothing


def test_comparator_checks_every_element_and_refuses_non_finite_values(data):
    x, w, ref, bar = data
    good = fl.rowlane_order_f32(x, w)
    for r, c in ((0, 0), (M - 1, fl.N_OUT - 1), (1, 5), (63, 127)):  # corners, the zero row, a tile's last row
        bad = good.copy()
        bad[r, c] = np.float32(ref[r, c] + 3 * bar[r, c] + 1e-30)
        assert fl.offending_rows(bad, ref, bar)[0] == {r}
    for v in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[7, 9] = v
        assert fl.offending_rows(bad, ref, bar)[0] == {7}
