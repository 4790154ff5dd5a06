"""The test side's reference of spmvHipCsrAdd: the serial loop of include/spmvHip.h in plain Python (add_loop), a vectorised
numpy form of the same loop (add_ref), and small (alpha, A, beta, B) cases.

A matrix is the tuple of tests/spgemm_ref.py: (M, N, IRP, JA, AS), IRP / JA uint64, AS float64, rows as stored (unsorted,
repeats allowed).  The sum is (M, N, IRP, JA, AS) with strictly ascending rows.  Every accumulator starts at +0.0 and takes
A's terms alpha * A.AS[p] of its row in stored order, then B's terms beta * B.AS[q]: each term a rounded product, then the
add."""
import numpy as np

import serial_order_inputs as si
from spgemm_ref import (aggregation, csr, dense, distinct_csr, laplacian7, random_csr, reverse_rows, same_bits,  # noqa: F401
                        transpose)
from spgemm_ref import integer_values, spgemm_ref


def add_loop(alpha, A, beta, B):
    """the loop, with numpy float64 scalars: multiply and add are two operations"""
    M, N, irpA, jaA, asA = A
    _, _, irpB, jaB, asB = B
    IRP = np.zeros(M + 1, dtype=np.uint64)
    JA, AS = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(M):
            acc = {}
            for s, irp, ja, a in ((np.float64(alpha), irpA, jaA, asA), (np.float64(beta), irpB, jaB, asB)):
                for p in range(int(irp[i]), int(irp[i + 1])):
                    j = int(ja[p])
                    if j not in acc:
                        acc[j] = np.float64(0.0)
                    term = s * np.float64(a[p])
                    acc[j] = acc[j] + term
            for j in sorted(acc):
                JA.append(j)
                AS.append(acc[j])
            IRP[i + 1] = len(JA)
    return M, N, IRP, np.array(JA, dtype=np.uint64), np.array(AS, dtype=np.float64)


def terms(alpha, A, beta, B):
    """every term in the loop's order -- row by row, A's entries then B's --: rows i, columns j, rounded values"""
    ra, rb = si.row_of_entry(A[2]), si.row_of_entry(B[2])
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.concatenate([np.float64(alpha) * A[4], np.float64(beta) * B[4]])
    i = np.concatenate([ra, rb]).astype(np.int64)
    j = np.concatenate([A[3], B[3]]).astype(np.int64)
    side = np.concatenate([np.zeros(ra.size, dtype=np.int64), np.ones(rb.size, dtype=np.int64)])
    order = np.lexsort((side, i))                                  # stable: stored order inside (row, side)
    return i[order], j[order], v[order]


def add_ref(alpha, A, beta, B):
    """the same loop, vectorised: a stable sort of the terms by (i, j) keeps the loop's order inside a key; the runs are then
    added one term per pass, all runs at once"""
    M, N = A[0], A[1]
    i, j, v = terms(alpha, A, beta, B)
    IRP = np.zeros(M + 1, dtype=np.uint64)
    if not v.size:
        return M, N, IRP, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float64)
    order = np.lexsort((j, i))
    i, j, v = i[order], j[order], v[order]
    head = np.ones(v.size, dtype=bool)
    head[1:] = (i[1:] != i[:-1]) | (j[1:] != j[:-1])
    starts = np.flatnonzero(head)
    run_len = np.diff(np.append(starts, v.size))
    acc = np.zeros(starts.size, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(int(run_len.max())):
            live = run_len > t
            acc[live] = acc[live] + v[starts[live] + t]
    IRP[1:] = np.cumsum(np.bincount(i[starts], minlength=M))
    return M, N, IRP, j[starts].astype(np.uint64), acc


def row_terms(A, B):
    """t[i]: the terms of row i"""
    return (np.diff(A[2].astype(np.int64)) + np.diff(B[2].astype(np.int64))).astype(np.int64)


def row_plain(A):
    """per row: the stored columns ascend strictly"""
    M, _, IRP, JA, _ = A
    ok = np.ones(M, dtype=bool)
    if JA.size > 1:
        r = si.row_of_entry(IRP)
        inner = r[1:] == r[:-1]
        bad = inner & (JA[1:].astype(np.int64) <= JA[:-1].astype(np.int64))
        ok[r[1:][bad]] = False
    return ok


def classes(A, B, laneMax=32, waveMax=2048, allSorted=False):
    """(rowsLane, rowsWave, rowsSorted) of the header's rule"""
    t = row_terms(A, B)
    plain = row_plain(A) & row_plain(B) & (not allSorted)
    lane = (t > 0) & plain & (t <= laneMax)
    wave = (t > 0) & plain & ~lane & (t <= waveMax)
    return int(lane.sum()), int(wave.sum()), int(((t > 0) & ~lane & ~wave).sum())


def identity(M, value=1.0):
    return csr(M, M, np.arange(M), np.arange(M), np.full(M, value))


def diagonal(A):
    """the sums of A's diagonal entries, as dense() adds them"""
    r = si.row_of_entry(A[2])
    d = np.zeros(A[0])
    on = r == A[3].astype(np.int64)
    np.add.at(d, r[on], A[4][on])
    return d


def smoothed_prolongator(A, T, omega):
    """T - omega D^-1 A T composed as the public calls compose it: Dinv (A T) by two products, then the sum"""
    Dinv = identity(A[0])[:4] + (1.0 / diagonal(A),)
    return add_ref(1.0, T, -omega, spgemm_ref(Dinv, spgemm_ref(A, T)))


# ------------------------------------------------------------------------------------------------------------- inputs
def sorted_csr(rng, M, N, lens, values=None):
    """rows of the given lengths with distinct columns in ASCENDING stored order: plain rows"""
    lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), (M,))
    rows = np.repeat(np.arange(M), lens)
    cols = np.concatenate([np.sort(rng.choice(N, size=int(n), replace=False)) for n in lens]) if rows.size else np.zeros(0, dtype=np.int64)
    vals = si.order_values(rng, rows.size) if values is None else values(rng, rows.size)
    return csr(M, N, rows, cols, vals)


def from_rows(N, rows, rng):
    """a matrix from a list of column lists, stored as given, with order-sensitive values"""
    lens = [len(r) for r in rows]
    cols = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if sum(lens) else np.zeros(0, dtype=np.int64)
    return csr(len(rows), N, np.repeat(np.arange(len(rows)), lens), cols, si.order_values(rng, cols.size))


def plain_rows(rng):
    """rows of at most 12 entries: disjoint column sets, identical patterns, interleaved columns, all of B below all of A and
    the other way round, a match at the first and at the last position only, A's row empty, B's row empty, both empty"""
    a = [[1, 4, 9, 20], [2, 3, 5, 7, 11], [0, 2, 4, 6, 8, 10], [30, 31, 32, 33], [0, 1, 2], [5, 10, 15, 20], [3, 10, 15, 28], [],
         [7, 8, 9], [], [0, 39], list(range(0, 24, 2))]
    b = [[0, 5, 10, 21], [2, 3, 5, 7, 11], [1, 3, 5, 7, 9, 11], [0, 1, 2], [30, 31, 32, 33], [5, 11, 16, 21], [4, 11, 16, 28], [7, 8, 9],
         [], [], [39], list(range(1, 24, 2))]
    return from_rows(40, a, rng), from_rows(40, b, rng)


def mixed_37x53(rng):
    """37 x 53, unsorted rows and repeats in both; row 3 of A repeats column 7 three times, row 3 of B twice"""
    A = random_csr(rng, 37, 53, rng.integers(0, 12, 37))
    B = random_csr(rng, 37, 53, rng.integers(0, 12, 37))
    la = np.diff(A[2].astype(np.int64))
    lb = np.diff(B[2].astype(np.int64))
    if la[3] < 3 or lb[3] < 2:
        la[3], lb[3] = max(la[3], 3), max(lb[3], 2)
        A, B = random_csr(rng, 37, 53, la), random_csr(rng, 37, 53, lb)
    A[3][int(A[2][3]):int(A[2][3]) + 3] = 7
    B[3][int(B[2][3]):int(B[2][3]) + 2] = 7
    return A, B


def special_values(rng):
    """+-Inf, -0.0 alone in its column, +0.0 and cancelling Infs of plain rows and rows with repeats"""
    A, B = plain_rows(rng)
    a, b = A[4].copy(), B[4].copy()
    a[[0, 5, 9]] = (np.inf, -np.inf, -0.0)                        # (0, 1), (1, 3) and (2, 0): the -0.0 alone in its column
    b[[0, 1, 5]] = (-0.0, np.inf, np.inf)                         # (0, 0) alone, (0, 5) alone, (1, 3): -Inf + Inf
    a[14] = 0.0
    return A[:4] + (a,), B[:4] + (b,)


def small_cases():
    """name -> (alpha, A, beta, B)"""
    rng = np.random.default_rng(2500)
    cases = {}
    cases["1x1"] = (2.0, csr(1, 1, [0], [0], [-2.5]), -3.0, csr(1, 1, [0], [0], [3.0]))
    cases["mixed37x53"] = (1.0, *_ab(mixed_37x53(rng), 1.0))
    cases["mixed37x53 scaled"] = (2.0 / 3.0, *_ab(mixed_37x53(rng), -1e300))
    cases["plain"] = (1.0, *_ab(plain_rows(rng), -1.0))
    cases["special"] = (1.0, *_ab(special_values(rng), 1.0))
    cases["special alpha=0"] = (0.0, *_ab(special_values(rng), 2.0))      # 0 * Inf: a NaN at its place, A's pattern kept
    A = mixed_37x53(rng)[0]
    cases["cancel"] = (1.0, A, -1.0, A)
    cases["negzero"] = (1.0, csr(2, 3, [0, 0, 1], [2, 0, 1], [-0.0, -0.0, 5.0]), 1.0, csr(2, 3, [0, 1], [2, 0], [-0.0, -0.0]))
    cases["empty_rows"] = (1.5, random_csr(rng, 9, 6, [0, 3, 0, 0, 2, 1, 0, 4, 0]), -0.5, random_csr(rng, 9, 6, [2, 0, 0, 3, 0, 1, 0, 0, 0]))
    cases["integer"] = (3.0, random_csr(rng, 20, 15, 6, integer_values), -2.0, random_csr(rng, 20, 15, 5, integer_values))
    return cases


def _ab(pair, beta):
    return pair[0], beta, pair[1]


def nan_case():
    rng = np.random.default_rng(2501)
    A, B = mixed_37x53(rng)
    a, b = A[4].copy(), B[4].copy()
    a.view(np.uint64)[::17] = 0x7FF8000000000001
    b.view(np.uint64)[5::29] = 0xFFF800000000BEEF
    a[3] = np.inf
    return 0.0, A[:4] + (a,), 1.0, B[:4] + (b,)
