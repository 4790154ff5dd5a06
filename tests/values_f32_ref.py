"""Test-side references for the single-precision value form (spmvHipValuesF32).

The form is AS32[p] = (float)AS[p], round to nearest even, subnormals kept; a product from it is sgemvSerial on
A~ = (double)AS32.  The reference rounding is numpy's astype(float32).astype(float64); `round32_plain` restates it in plain
Python with exact rational arithmetic, and tests/test_values_f32_abi.py holds the two against each other on the boundary
set.  The inputs of the GPU tests live here so that the host tests can show what they distinguish."""
import functools
import math
from fractions import Fraction

import numpy as np

import serial_order_inputs as si

FLT_MAX = float(np.finfo(np.float32).max)                     # (2 - 2^-23) * 2^127
OVERFLOW = (2.0 - 2.0 ** -24) * 2.0 ** 127                    # the smallest magnitude that rounds to Inf (a tie, to even = 2^128)


def round32(a):
    """(double)(float)a, elementwise"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def round32_plain(d):
    """the same for one Python float, from the definition: the nearest multiple of the quantum 2^max(e - 24, -149) (d = m 2^e,
    1/2 <= m < 1), ties to the even multiple, 2^128 and above Inf, the sign kept"""
    if d != d or d in (math.inf, -math.inf) or d == 0.0:
        return d
    a = abs(d)
    _, e = math.frexp(a)
    q = max(e - 24, -149)
    n = Fraction(a) / Fraction(2) ** q
    k = n.numerator // n.denominator
    rest = n - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k % 2 == 1):
        k += 1
    r = math.ldexp(float(k), q)                                   # exact: k <= 2^24
    if r >= 2.0 ** 128:
        r = math.inf
    return math.copysign(r, d)


def boundary_values():
    """the values at which the rounding changes its behaviour, and their negatives"""
    pos = [0.0, 1.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 2.0 ** -149, 2.0 ** -150, float(np.nextafter(2.0 ** -150, 1.0)),
           FLT_MAX, float(np.nextafter(OVERFLOW, 0.0)), OVERFLOW, math.inf, math.nan]
    return np.array(pos + [-v for v in pos], dtype=np.float64)


# what each boundary value must become (NaN: any NaN)
BOUNDARY_EXPECT = [0.0, 1.0, 1.0, 1.0 + 2.0 ** -22, 2.0 ** -149, 0.0, 2.0 ** -149, FLT_MAX, FLT_MAX, math.inf, math.inf, math.nan]


def counts(a):
    """what spmvHipValuesF32Info reports for the values a: (inexact, overflowed, flushed, firstOverflow)"""
    a = np.asarray(a, dtype=np.float64)
    r = round32(a)
    inexact = ~np.isnan(a) & (r != a)
    over = np.isfinite(a) & np.isinf(r)
    flushed = (a != 0) & (r == 0)
    return int(inexact.sum()), int(over.sum()), int(flushed.sum()), int(np.flatnonzero(over)[0]) if over.any() else -1


def rounded(A):
    """A~ of a matrix (M, N, IRP, JA, AS)"""
    return A[:4] + (round32(A[4]),)


def same(a, ref, what):
    """finite values by bits, infinities by sign, NaN as NaN"""
    from bits import assert_same_bits
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert_same_bits(a[fin], ref[fin], what)
    inf = np.isinf(ref)
    assert np.array_equal(a[inf], ref[inf]), what
    assert np.isnan(a[np.isnan(ref)]).all(), what


# ------------------------------------------------------------------------------------------------ the product cases
def _csr(rng, M, N, lens, sort):
    lens = np.asarray(lens, dtype=np.int64)
    rows = np.repeat(np.arange(M), lens)
    cols = rng.integers(0, N, rows.size)
    if sort:
        o = np.lexsort((cols, rows))
        rows, cols = rows[o], cols[o]
    IRP, JA, AS = si.assemble(M, rows, cols, si.order_values(rng, rows.size))
    return M, N, IRP, JA, AS, si.order_values(rng, N)


def _empty_rows(rng):
    lens = rng.integers(0, 6, 40)
    lens[[0, 1, 17, 38, 39]] = 0
    return _csr(rng, 40, 50, lens, True)


def _random_300(rng):
    """unsorted rows, and repeated (row, column) pairs: every row's first entry again as its last"""
    M, N, IRP, JA, AS, x = _csr(rng, 300, 300, rng.integers(0, 40, 300), False)
    rows = si.row_of_entry(IRP)
    first = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]]) if rows.size else np.zeros(0, np.int64)
    r2, c2 = np.concatenate([rows, rows[first]]), np.concatenate([JA.astype(np.int64), JA[first].astype(np.int64)])
    v2 = np.concatenate([AS, si.order_values(rng, first.size)])
    return (M, N) + si.assemble(M, r2, c2, v2) + (x,)


def _boundary(rng):
    """every boundary value against an ordinary x, +-Inf and +-0 in rows of one entry (a value flushed to zero times Inf is a
    NaN where the double product is an Inf), then rows that mix them with ordinary entries"""
    vals = boundary_values()
    xs = np.array([1.5, math.inf, -math.inf, 0.0, -0.0, -3.25e-3, 7.0e5, 2.0 ** -30])
    rows, cols, a = [], [], []
    r = 0
    for v in vals:
        for c in range(5):
            rows.append(r); cols.append(c); a.append(v)
            r += 1
    for v in vals:                                                  # three ordinary entries around the boundary value
        oc = rng.integers(5, 8, 3)
        for c, w in ((oc[0], si.order_values(rng, 1)[0]), (int(rng.integers(0, 8)), v), (oc[1], si.order_values(rng, 1)[0]),
                     (oc[2], si.order_values(rng, 1)[0])):
            rows.append(r); cols.append(int(c)); a.append(w)
        r += 1
    M = r
    IRP, JA, AS = si.assemble(M, np.array(rows), np.array(cols), np.array(a))
    return M, xs.size, IRP, JA, AS, xs


CASES = {
    "empty": lambda: (0, 5, np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0), si.order_values(np.random.default_rng(4100), 5)),
    "empty-rows": lambda: _empty_rows(np.random.default_rng(4101)),
    "one-row-5000": lambda: _csr(np.random.default_rng(4102), 1, 6000, [5000], True),                # long-row path: 3 chunks of 2048
    "three-rows-4100": lambda: _csr(np.random.default_rng(4103), 3, 5000, [4100, 4100, 4100], True),  # ... 3 chunks, 3 long blocks
    "short-1300": lambda: _csr(np.random.default_rng(4104), 1300, 900, np.random.default_rng(4105).integers(0, 4, 1300), True),
    "random-300": lambda: _random_300(np.random.default_rng(4106)),
    "boundary": lambda: _boundary(np.random.default_rng(4107)),
}
ORDINARY = ("empty-rows", "one-row-5000", "three-rows-4100", "short-1300", "random-300")     # finite, order-sensitive values


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def unit_case(value):
    """the pattern of random-300 with every value `value`"""
    M, N, IRP, JA, AS, x = case("random-300")
    return M, N, IRP, JA, np.full(JA.size, value), x


# ------------------------------------------------------------------------------------------------------- the hierarchy
def rounded_levels(levels):
    """a reference hierarchy (amg_ref / amg_sa_ref / filter_ref setup_ref) as spmvHipAmgSetStorage(F32) applies it: every
    A_l, R_l and P_l that a product of the cycle streams rounded through float32; dinv, and the matrices rho_l and the
    Chebyshev tables are taken from, stay the doubles'"""
    from krylov_ref import Csr
    out = []
    for lv in levels:
        n = dict(lv)
        for key in ("csr", "Rcsr", "Pcsr"):
            if key in lv:
                c = lv[key]
                n[key] = Csr(c.M, c.IRP, c.JA, round32(c.AS))
        out.append(n)
    return out


# (hierarchy, smoother of amg_block_ref.SMOOTHERS, the fused-correction threshold of the setup)
AMG_CONFIGS = {"plain-jacobi": ("plain", "jacobi118", 0), "smoothed-jacobi": ("smoothed", "jacobi223", 0),
               "smoothed-chebyshev": ("smoothed", "cheb222", 0), "smoothed-chebyshev-fused": ("smoothed", "cheb314", 64),
               "strength-jacobi": ("strength", "jacobi118", 0)}


@functools.lru_cache(maxsize=None)
def amg_matrix(values=0):
    """the 12 x 10 x 8 seven-point pattern with order-sensitive symmetric off-diagonals and a dominant diagonal (every value
    inexact in single precision); values: another seed on the same pattern"""
    from test_fsai_abi import stencil
    return stencil(np.random.default_rng(4500 + values), 12, 10, 8)


@functools.lru_cache(maxsize=None)
def amg_reference(config, values=0):
    """(levels, rounded levels, options, smoother) of a configuration, computed once"""
    import amg_block_ref as br
    import amg_cheb_ref as cr
    hierarchy, smoother, _ = AMG_CONFIGS[config]
    kw = dict(theta=0.0) if hierarchy == "strength" else {}
    levels, o = cr.setup_ref(amg_matrix(values), hierarchy, coarseRows=8, **kw)
    return levels, rounded_levels(levels), o, br.smoother_of(o, smoother)
