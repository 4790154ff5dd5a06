"""Exactly rounded row sums of y = A x, and a bound that every summation order of every correct kernel meets.

`exact_rows` splits every product a_ij * x_j into an exact pair (p, e) with p + e == a_ij * x_j (TwoProduct: Dekker's
product with a Veltkamp split, vectorised in numpy -- numpy rounds every operation on its own, no FMA), then sums each row's
pairs with math.fsum, which returns the correctly rounded value of an exact sum of doubles.  The result is the one double
nearest to the true row sum: no order, no rounding of the products.

This is exact while no product overflows and no error term underflows.  Both hold when every nonzero |a| and |x| lies in
[2^-200, 2^200]: |a x| <= 2^400, and the smallest piece the split makes, al * xl, is at least 2^-200-53 squared = 2^-506,
far above the subnormal range (2^-1022).  The functions assert that range (zeros are allowed anywhere).

`check_any_order` asserts, for every row i with n_i stored entries, the classical bound of a floating-point dot product

    |y_i - sum_j a_ij x_j|  <=  gamma(n_i + 1) * sum_j |a_ij x_j|,      gamma(n) = n u / (1 - n u),  u = 2^-53

measured exactly (the difference is an fsum of y_i and the negated pairs).  Recursive summation of n rounded products in
any order and any tree, with or without FMA, stays within gamma(n) of the true sum (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., section 3.1); the extra 1 covers the one rounding of sum |a x| itself.  ELL padding adds
exact zeros and changes nothing.  So the check never fails for a correct kernel, on any data in range.  A row with
sum |a x| == 0 must give 0 exactly, and NaN or Inf is always wrong.  Rows up to about 900 entries get a tighter bound
than the suite's tight_error <= 1e-13; the two are used side by side, never one instead of the other."""
import math

import numpy as np

U = 2.0 ** -53
LO, HI = 2.0 ** -200, 2.0 ** 200
_SPLIT = 134217729.0                  # 2^27 + 1: Veltkamp's constant for doubles


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def _in_range(v, what):
    v = np.abs(np.asarray(v, dtype=np.float64))
    nz = v[v != 0]
    assert np.isfinite(v).all(), f"{what}: NaN or Inf (exact_ref covers finite data only)"
    assert nz.size == 0 or (nz.min() >= LO and nz.max() <= HI), \
        f"{what}: a nonzero magnitude lies outside [2^-200, 2^200] ({nz.min():.3e} .. {nz.max():.3e}): the sums would not be exact"


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def two_products(a, b):
    """(p, e) with p = fl(a * b) and p + e == a * b exactly, elementwise"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = al * bl - (((p - ah * bh) - al * bh) - ah * bl)
    return p, e


def _pairs(IRP, JA, AS, x):
    IRP = np.asarray(IRP).astype(np.int64)
    JA = np.asarray(JA).astype(np.int64)
    AS = np.asarray(AS, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    assert IRP[0] == 0 and IRP[-1] == JA.size == AS.size, "not a CSR matrix"
    assert JA.size == 0 or (JA.min() >= 0 and JA.max() < x.size), "column out of range"
    _in_range(AS, "A")
    _in_range(x, "x")
    p, e = two_products(AS, x[JA])
    return IRP, p, e


def _row_fsums(IRP, parts):
    """math.fsum of each row's entries of every array in `parts` (all in CSR order)"""
    k = len(parts)
    flat = np.stack(parts, axis=1).ravel().tolist() if parts[0].size else []
    b = (IRP * k).tolist()
    fs = math.fsum
    return np.array([fs(flat[s:t]) for s, t in zip(b[:-1], b[1:])], dtype=np.float64) + 0.0


def exact_rows(IRP, JA, AS, x):
    """the correctly rounded sum_j a_ij x_j of every row (+0.0 for an empty or exactly cancelling row).  Rows may be
    unsorted and repeat columns: every stored entry is a term of its own."""
    IRP, p, e = _pairs(IRP, JA, AS, x)
    return _row_fsums(IRP, [p, e])


def abs_rows(IRP, JA, AS, x):
    """sum_j |a_ij x_j| of every row, rounded once (|p + e| = |p| + sign(p) e, both summed exactly)"""
    IRP, p, e = _pairs(IRP, JA, AS, x)
    return _row_fsums(IRP, [np.abs(p), np.copysign(1.0, p) * e])


def check_any_order(IRP, JA, AS, x, y, what=""):
    """assert that y = A x could have come from a correct kernel that adds every row's rounded products in SOME order
    (see the module docstring for the bound); the message names the first bad row, its n_i, its error in ulps of
    sum |a x|, and `what`"""
    IRP, p, e = _pairs(IRP, JA, AS, x)
    y = np.asarray(y, dtype=np.float64)
    M = IRP.size - 1
    assert y.shape == (M,), f"{what}: y has shape {y.shape}, expected ({M},)"
    n = np.diff(IRP)

    def fail(i, reason):
        raise AssertionError(f"{what}: row {i} (n_i = {int(n[i])}): {reason}")

    bad = np.flatnonzero(~np.isfinite(y))
    if bad.size:
        fail(int(bad[0]), f"y = {y[bad[0]]!r} ({bad.size} non-finite rows)")
    exact = _row_fsums(IRP, [p, e])
    scale = _row_fsums(IRP, [np.abs(p), np.copysign(1.0, p) * e])
    bound = gamma(n + 1) * scale
    # exact error |y_i - sum a x| only where y differs from the rounded exact sum (elsewhere it is at most half an ulp of
    # the sum, which gamma(n_i + 1) * scale covers: gamma(2) > u)
    rows = np.flatnonzero(y != exact)
    if rows.size == 0:
        return
    neg = np.stack([-p, -e], axis=1).ravel().tolist()
    b = (IRP * 2).tolist()
    fs = math.fsum
    for i in rows.tolist():
        err = abs(fs([float(y[i])] + neg[b[i]:b[i + 1]]))
        if not err <= bound[i]:
            ulps = err / np.spacing(scale[i]) if scale[i] > 0 else np.inf
            fail(i, f"y = {y[i]!r}, exact {exact[i]!r}, |error| = {err:.3e} = {ulps:.1f} ulp of sum|a x| = {scale[i]!r}, "
                    f"bound gamma(n_i + 1) * sum|a x| = {bound[i]:.3e} ({rows.size} rows differ from the exact sum)")
