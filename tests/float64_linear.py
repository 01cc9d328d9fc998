"""``y = act(x . w^T + bias)`` (csrc/dense.hip, ``mpx_linear``) on the CPU in float64, the bar an fp32 kernel is held to,
the comparator, two planted defects and the seeded inputs of tests/test_gpu_linear_rowlane.py.

``reference`` is a float64 product of the FLOAT32 operands (LeakyReLU's slope is the float32 0.01 the kernel multiplies by).

``bar`` is the textbook worst case of an n-term fp32 inner product in ANY summation order, fused or not (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1): ``gamma_n (sum_k |x_ik| |w_jk| + |b_j|)`` per element with ``gamma_n = n u /
(1 - n u)``, ``u = 2^-24``, ``n = K`` plus one where a bias is added plus one for LeakyReLU's multiplication (ReLU and the
identity round nothing).  It is derived, not measured, and carries no margin: it holds for the row-per-lane kernel, the tile
kernel and the gemv kernel alike.  An all-zero row has bar 0: the kernel owes exact zeros there.

``ascending_f32`` and ``rowlane_order_f32`` are numpy float32 emulations of two summation orders, for
tests/test_linear_reference_host.py: products rounded and added one at a time in ascending k, and the order the row-per-lane
kernel documents -- a chain of fused steps over the pairs (k, k + K / 2) in ascending k.  Nothing here shares code with a
kernel."""
import numpy as np

U = 2.0 ** -24
N_OUT, K_IN = 128, 68
LEAKY_SLOPE = np.float64(np.float32(0.01))
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
X_SEED, W_SEED = 6803, 12868


def gamma(n):
    return n * U / (1.0 - n * U)


def make_x(M, K=K_IN, seed=X_SEED):
    """float32 [M,K] ~ N(0,1); row 1 all zeros, row 2 alternating 1e4 and 1e-4 magnitudes.  The leading rows do not depend on
    M (the generator fills row by row)."""
    x = np.random.default_rng(seed).standard_normal((M, K), dtype=np.float32)
    if M > 1:
        x[1] = 0.0
    if M > 2:
        x[2] *= np.where(np.arange(K) % 2 == 0, np.float32(1e4), np.float32(1e-4))
    return x


def make_w(N=N_OUT, K=K_IN, seed=W_SEED):
    """float32 [N,K] ~ N(0,1) / sqrt(K)."""
    return (np.random.default_rng(seed).standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)


def make_bias(N=N_OUT, seed=W_SEED + 1):
    return np.random.default_rng(seed).standard_normal(N).astype(np.float32)


def _act(z, act):
    if act == ACT_RELU:
        return np.maximum(z, 0.0)
    if act == ACT_LEAKY:
        return np.where(z >= 0, z, z * LEAKY_SLOPE)
    assert act == ACT_NONE
    return z


def reference(x, w, bias=None, act=ACT_NONE):
    """float32 x [M,K], w [N,K], bias [N] or None -> float64 [M,N]."""
    x, w = np.asarray(x, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    z = x @ w.T
    if bias is not None:
        z = z + np.asarray(bias, np.float32).astype(np.float64)
    return _act(z, act)


def bar(x, w, bias=None, act=ACT_NONE):
    """-> float64 [M,N]: the largest |fp32 result - reference| any summation order can give (see the module docstring)."""
    x, w = np.abs(np.asarray(x, np.float32).astype(np.float64)), np.abs(np.asarray(w, np.float32).astype(np.float64))
    mag = x @ w.T
    n = x.shape[1]
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, np.float32).astype(np.float64))
        n += 1
    if act == ACT_LEAKY:
        n += 1
    return gamma(n) * mag


def offending_rows(got, ref, bar_):
    """The comparator: EVERY element is checked -> (the set of rows with an entry further than its bar from the reference,
    or not finite; the largest err / bar over the entries with bar > 0)."""
    got, ref, bar_ = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bar_, np.float64)
    assert got.shape == ref.shape == bar_.shape and got.ndim == 2
    err = np.abs(got - ref)
    bad = ~(err <= bar_)  # (a NaN is not <= anything)
    pos = bar_ > 0
    worst = float(np.max(np.where(pos & np.isfinite(err), err, 0.0) / np.where(pos, bar_, 1.0))) if got.size else 0.0
    return set(np.flatnonzero(bad.any(axis=1)).tolist()), worst


def drop_term(y, x, w, row, k):
    """Planted defect: a copy of ``y`` whose row ``row`` lacks the product x[row, k] . w[:, k]."""
    out = np.array(y, copy=True)
    out[row] = (out[row].astype(np.float64) - np.float64(x[row, k]) * np.asarray(w, np.float32)[:, k].astype(np.float64)).astype(out.dtype)
    return out


def swap_rows(y, r0, r1):
    """Planted defect: a copy of ``y`` with two rows swapped."""
    out = np.array(y, copy=True)
    out[[r0, r1]] = out[[r1, r0]]
    return out


def dropped_over_bar(x, w, bar_, row, k):
    """The smallest |x[row, k] w[j, k]| / bar[row, j] over the columns: above 1 (by more than float32's rounding of the
    result) the defect of ``drop_term`` is outside the bar in EVERY column, so a control that plants it cannot pass vacuously."""
    prod = np.abs(np.float64(x[row, k]) * np.asarray(w, np.float32)[:, k].astype(np.float64))
    return float(np.min(prod / bar_[row]))


def ascending_f32(x, w):
    """float32 [M,N]: each product rounded to float32, added in ascending k, every sum rounded."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k in range(x.shape[1]):
        acc = acc + x[:, k, None] * w[None, :, k]
        assert acc.dtype == np.float32
    return acc


def _fused(acc, a, b):
    """fl32(acc + a b): the product of two float32 is exact in float64."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def rowlane_order_f32(x, w):
    """float32 [M,N]: a chain of fused steps over (k, k + K / 2), k ascending -- the order csrc/dense.hip documents for the
    row-per-lane kernel."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    kh = x.shape[1] // 2
    assert 2 * kh == x.shape[1]
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k in range(kh):
        acc = _fused(acc, x[:, k, None], w[None, :, k])
        acc = _fused(acc, x[:, k + kh, None], w[None, :, k + kh])
    return acc
