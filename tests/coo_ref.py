"""The serial loop of spmvHipCooAssemble (include/spmvHip.h) in numpy: the test side's reference of the COO assembly.

    kept = the entries with row != SKIP and col != SKIP, ascending e
    a STABLE sort of the kept entries by (row, col) -- np.lexsort is stable --, so the duplicates of an (i, j) stand in input
    order; every run is then added with np.float64 scalars, one plain add per duplicate ("sum"), or its last member taken
    ("last").  A single entry, and the last one, are copied, never computed with: their bits stay.

A matrix is the tuple the other references use: (M, N, IRP, JA, AS) with uint64 indices."""
import numpy as np

from bits import assert_same_bits

SKIP = 0xFFFFFFFF
SUM, LAST = 0, 1
MODES = {"sum": SUM, "last": LAST}


def as_index(a):
    """an index array of any integer dtype as int64 with SKIP at the skipped places (-1 is the skip marker too)"""
    a = np.asarray(a)
    assert np.issubdtype(a.dtype, np.integer), a.dtype
    out = a.astype(np.int64) if a.dtype != np.uint64 else np.where(a > SKIP, -2, a).astype(np.int64)
    assert np.all((out == -1) | ((out >= 0) & (out <= SKIP))), "an index that is neither -1 nor in [0, 2^32 - 1]"
    return np.where(out == -1, SKIP, out)


def runs_of(M, N, rows, cols):
    """(order, starts): the kept entries in (row, col, e) order, and the start of every run in that order with the kept count
    appended.  An index out of range raises, naming the smallest such e, as the library's line does."""
    rows, cols = as_index(rows), as_index(cols)
    assert rows.shape == cols.shape and rows.ndim == 1
    kept = np.flatnonzero((rows != SKIP) & (cols != SKIP))
    bad = kept[(rows[kept] >= M) | (cols[kept] >= N)]
    if bad.size:
        raise IndexError(int(bad[0]))
    order = kept[np.lexsort((cols[kept], rows[kept]))]            # stable: equal (row, col) keep ascending e
    r, c = rows[order], cols[order]
    head = np.ones(order.size, dtype=bool)
    head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    return order, np.append(np.flatnonzero(head), order.size)


def values_of(order, starts, vals, mode=SUM):
    """the value of every run from `vals` (the whole triplet list's values): the loop, one np.float64 add per duplicate"""
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    out = np.empty(starts.size - 1, dtype=np.float64)
    last = vals[order[starts[1:] - 1]] if out.size else out
    if mode == LAST:
        return last.copy()
    out[:] = vals[order[starts[:-1]]] if out.size else out
    with np.errstate(invalid="ignore", over="ignore"):             # Inf + -Inf and an overflowing sum are results, not errors
        for q in np.flatnonzero(np.diff(starts) > 1).tolist():
            v = np.float64(vals[order[starts[q]]])
            for e in order[starts[q] + 1:starts[q + 1]].tolist():
                v = v + np.float64(vals[e])
            out[q] = v
    return out


def assemble_ref(M, N, rows, cols, vals, duplicates="sum"):
    """(C, info, (order, starts)): C = (M, N, IRP, JA, AS), info = the counts of spmvCooInfo as a dict"""
    mode = MODES[duplicates] if isinstance(duplicates, str) else int(duplicates)
    order, starts = runs_of(M, N, rows, cols)
    rows, cols = as_index(rows), as_index(cols)
    heads = order[starts[:-1]]
    IRP = np.zeros(M + 1, dtype=np.uint64)
    if M:
        IRP[1:] = np.cumsum(np.bincount(rows[heads], minlength=M))
    C = (M, N, IRP, cols[heads].astype(np.uint64), values_of(order, starts, vals, mode))
    lens = np.diff(starts)
    info = dict(nEntries=rows.size, skipped=rows.size - order.size, nnzC=heads.size, duplicates=order.size - heads.size,
                maxRun=int(lens.max()) if lens.size else 0, maxRowNnz=int(np.diff(IRP.astype(np.int64)).max()) if M else 0)
    return C, info, (order, starts)


def refresh_ref(C, runs, vals, duplicates="sum"):
    """C with its values again from a new value list over the build's runs"""
    mode = MODES[duplicates] if isinstance(duplicates, str) else int(duplicates)
    return C[:4] + (values_of(runs[0], runs[1], vals, mode),)


def to_coo_ref(A):
    """(rows, cols, vals) of a CSR tuple in stored order"""
    M, _, IRP, JA, AS = A
    return (np.repeat(np.arange(M, dtype=np.uint32), np.diff(np.asarray(IRP).astype(np.int64))), np.asarray(JA).astype(np.uint32),
            np.asarray(AS, dtype=np.float64))


def same_bits(C, R, what="", nan_sums=None):
    """shape and indices exact, values as bits; nan_sums: the entries of R that are a SUM and a NaN -- there the payload is
    not pinned, and C must hold a NaN"""
    assert (int(C[0]), int(C[1])) == (int(R[0]), int(R[1])), f"{what}: shape"
    assert np.array_equal(np.asarray(C[2]).astype(np.uint64), np.asarray(R[2]).astype(np.uint64)), f"{what}: IRP"
    assert np.array_equal(np.asarray(C[3]).astype(np.uint64), np.asarray(R[3]).astype(np.uint64)), f"{what}: JA"
    got, want = np.asarray(C[4], dtype=np.float64).copy(), np.asarray(R[4], dtype=np.float64).copy()
    assert got.shape == want.shape, f"{what}: AS shape"
    if nan_sums is not None and nan_sums.size:
        assert np.all(np.isnan(got[nan_sums])), f"{what}: a NaN sum"
        got[nan_sums] = want[nan_sums] = 0.0
    assert_same_bits(got, want, f"{what}: AS")


def nan_sums_of(R, runs):
    """the entries of R whose value is a NaN computed by adds (a run of two or more)"""
    return np.flatnonzero(np.isnan(R[4]) & (np.diff(runs[1]) > 1))
