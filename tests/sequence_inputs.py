"""Matrix families and value kinds of the operation-sequence test (tests/test_gpu_sequences.py), shared with the host
checks of the exact reference (tests/test_exact_ref.py), so the mutation checks there run on the very data the GPU
test uses.

Every family has at least 2^18 entries (AUTO_MIN_NNZ: the selections and the private formats are in play) and two x
vectors.  Every value kind stays inside the range where exact_ref.exact_rows is exact (nonzero magnitudes in
[2^-200, 2^200])."""
import functools

import numpy as np

from serial_order_inputs import AUTO_MIN_NNZ, shuffled

FAMILIES = ("uploaded", "adopted64", "square", "shuffled")
KINDS = ("uniform", "wide", "cancel", "constant", "constant_but_one")
CONSTANTS = (1.0, -2.5, -0.0, 0.0)


def _csr(M, rows, cols):
    """sorted distinct columns per row (duplicates of the draw dropped)"""
    key = np.unique(rows.astype(np.int64) * (1 << 32) + cols.astype(np.int64))
    rows, cols = key >> 32, key & 0xFFFFFFFF
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return IRP, cols.astype(np.uint64)


def _xs(rng, N):
    x0 = rng.choice([-1.0, 1.0], N) * rng.uniform(0.5, 1.0, N) * 2.0 ** rng.integers(-8, 9, N)
    x1 = np.sin(rng.uniform(0.1, 3.0, N)) * 3e-5 * rng.choice([-1.0, 1.0], N)
    return x0, x1


@functools.lru_cache(maxsize=None)
def family(name):
    """(M, N, IRP u64, JA u64, x0, x1): the pattern and the two x of one family (values come from `values`)"""
    rng = np.random.default_rng(FAMILIES.index(name) + 4100)
    if name == "uploaded":                     # 32-bit row pointers, short rows
        M = N = 36_000
        lens = rng.integers(5, 15, M)
        lens[[0, 17, M - 1]] = 0
        rows = np.repeat(np.arange(M), lens)
        IRP, JA = _csr(M, rows, rng.integers(0, N, rows.size))
    elif name == "adopted64":                  # rectangular, a few rows past 256 entries (SELL's workgroup rows)
        M, N = 30_000, 50_000
        lens = rng.integers(4, 16, M)
        lens[[7, 1000, 2000, M - 1]] = [300, 5000, 1200, 0]
        rows = np.repeat(np.arange(M), lens)
        IRP, JA = _csr(M, rows, rng.integers(0, N, rows.size))
    elif name == "square":                     # every row holds its diagonal once: triangular solves
        M = N = 40_000
        lens = rng.integers(3, 12, M)
        rows = np.concatenate([np.repeat(np.arange(M), lens), np.arange(M)])
        cols = np.concatenate([rng.integers(0, N, lens.sum()), np.arange(M)])
        IRP, JA = _csr(M, rows, cols)
    elif name == "shuffled":                   # unsorted rows, repeated columns, empty rows
        M, N, IRP, JA, _, _ = shuffled()
        IRP, JA = IRP.astype(np.uint64), JA.astype(np.uint64)
    else:
        raise KeyError(name)
    assert JA.size >= AUTO_MIN_NNZ, (name, JA.size)
    x0, x1 = _xs(rng, N)
    return M, N, IRP, JA, x0, x1


def values(rng, kind, IRP, JA, x):
    """NZ new values of one kind.  `cancel` pairs every second entry of a row with the one before it so that their
    products against `x` cancel up to one rounding: the row sums are tiny next to sum |a x|."""
    nnz = JA.size
    if kind == "uniform":
        return rng.uniform(-1.0, 1.0, nnz)
    if kind == "wide":
        return rng.choice([-1.0, 1.0], nnz) * 2.0 ** rng.uniform(-60.0, 60.0, nnz)
    if kind == "cancel":
        a = rng.uniform(-1.0, 1.0, nnz) * 2.0 ** rng.integers(-10, 11, nnz)
        lens = np.diff(IRP.astype(np.int64))
        local = np.arange(nnz) - np.repeat(IRP[:-1].astype(np.int64), lens)
        q = np.flatnonzero(local % 2 == 1)
        j = JA.astype(np.int64)
        a[q] = -a[q - 1] * x[j[q - 1]] / x[j[q]]
        return a
    if kind == "constant":
        return np.full(nnz, CONSTANTS[rng.integers(len(CONSTANTS))])
    if kind == "constant_but_one":
        a = np.full(nnz, (1.0, -2.5, 0.5)[rng.integers(3)])
        a[rng.integers(nnz)] = rng.uniform(-1.0, 1.0)
        return a
    raise KeyError(kind)


def unit_of(AS):
    """(True, value) when every stored value has the same bit pattern (the library's unit detection), else (False, None)"""
    b = np.ascontiguousarray(AS, dtype=np.float64).view(np.uint64)
    if b.size and (b == b[0]).all():
        return True, float(AS[0])
    return False, None
