"""The test side's reference of spmvHipSpGEMM: the serial loop of include/spmvHip.h in plain Python (spgemm_loop), a
vectorised numpy form of the same loop (spgemm_ref), and small (A, B) pairs.

A matrix here is a tuple (M, N, IRP, JA, AS): IRP / JA uint64, AS float64, rows as stored (unsorted, repeats allowed).
The product is (M, N, IRP, JA, AS) with strictly ascending rows.  Every accumulator starts at +0.0 and takes its terms in
(p, q) order -- p over A's row as stored, q over B's row JA[p] as stored --, each term a rounded product, then the add."""
import numpy as np

import serial_order_inputs as si


def spgemm_loop(A, B):
    """the loop, with numpy float64 scalars: multiply and add are two operations"""
    M, _, irpA, jaA, asA = A
    _, N, irpB, jaB, asB = B
    IRP = np.zeros(M + 1, dtype=np.uint64)
    JA, AS = [], []
    for i in range(M):
        acc = {}
        for p in range(int(irpA[i]), int(irpA[i + 1])):
            k = int(jaA[p])
            a = np.float64(asA[p])
            for q in range(int(irpB[k]), int(irpB[k + 1])):
                j = int(jaB[q])
                if j not in acc:
                    acc[j] = np.float64(0.0)
                prod = a * np.float64(asB[q])
                acc[j] = acc[j] + prod
        for j in sorted(acc):
            JA.append(j)
            AS.append(acc[j])
        IRP[i + 1] = len(JA)
    return M, N, IRP, np.array(JA, dtype=np.uint64), np.array(AS, dtype=np.float64)


def products(A, B):
    """every product in (i, p, q) order: rows i, columns j, rounded values"""
    M, _, irpA, jaA, asA = A
    _, N, irpB, jaB, asB = B
    irpB = irpB.astype(np.int64)
    k = jaA.astype(np.int64)
    lens = irpB[k + 1] - irpB[k] if k.size else np.zeros(0, dtype=np.int64)
    total = int(lens.sum())
    src = np.repeat(np.arange(k.size), lens)                       # the entry p of A behind every product
    first = np.cumsum(lens) - lens
    q = irpB[k][src] + (np.arange(total) - first[src])
    i = si.row_of_entry(irpA)[src] if total else np.zeros(0, dtype=np.int64)
    return i, jaB[q].astype(np.int64), asA[src] * asB[q], lens


def spgemm_ref(A, B):
    """the same loop, vectorised: a stable sort of the products by (i, j) keeps (p, q) order inside a key; the runs are
    then added one term per pass, all runs at once"""
    M, N = A[0], B[1]
    i, j, v, _ = products(A, B)
    IRP = np.zeros(M + 1, dtype=np.uint64)
    if not v.size:
        return M, N, IRP, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float64)
    order = np.lexsort((j, i))                                     # lexsort is stable
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


def row_products(A, B):
    """ub[i]: the products of row i"""
    lens = products(A, B)[3]
    r = si.row_of_entry(A[2])
    return np.bincount(r, weights=lens, minlength=A[0]).astype(np.int64) if lens.size else np.zeros(A[0], dtype=np.int64)


def same_bits(C, R, what=""):
    """indices exact, values as bits, NaN as NaN (its payload is not pinned)"""
    assert (C[0], C[1]) == (R[0], R[1]), f"{what}: shape"
    assert np.array_equal(np.asarray(C[2], dtype=np.uint64), R[2]), f"{what}: IRP"
    assert np.array_equal(np.asarray(C[3], dtype=np.uint64), R[3]), f"{what}: JA"
    a, b = np.asarray(C[4], dtype=np.float64), R[4]
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), f"{what}: NaN places"
    assert np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]), f"{what}: AS bits"


def dense(A):
    M, N, IRP, JA, AS = A
    D = np.zeros((M, N))
    np.add.at(D, (si.row_of_entry(IRP), JA.astype(np.int64)), AS)
    return D


def structural(A, B):
    """the pattern every product reaches, as a boolean dense matrix (independent of any order)"""
    pa = np.zeros((A[0], A[1]), dtype=np.int64)
    pb = np.zeros((B[0], B[1]), dtype=np.int64)
    pa[si.row_of_entry(A[2]), A[3].astype(np.int64)] = 1
    pb[si.row_of_entry(B[2]), B[3].astype(np.int64)] = 1
    return (pa @ pb) > 0


def pattern_of(C):
    P = np.zeros((C[0], C[1]), dtype=bool)
    P[si.row_of_entry(C[2]), C[3].astype(np.int64)] = True
    return P


def reverse_rows(A):
    perm = si.reversed_rows(A[2])
    return A[0], A[1], A[2], A[3][perm], A[4][perm]


def transpose(A):
    """A^T as spmvHipCsrTranspose builds it: row j holds column j's entries in CSR position order"""
    M, N, IRP, JA, AS = A
    order = np.argsort(JA.astype(np.int64), kind="stable")
    irp = np.zeros(N + 1, dtype=np.uint64)
    irp[1:] = np.cumsum(np.bincount(JA.astype(np.int64), minlength=N))
    return N, M, irp, si.row_of_entry(IRP)[order].astype(np.uint64), AS[order]


# ------------------------------------------------------------------------------------------------------------- inputs
def csr(M, N, rows, cols, vals):
    IRP, JA, AS = si.assemble(M, np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64))
    return M, N, IRP, JA, AS


def random_csr(rng, M, N, lens, values=None):
    """rows of the given lengths with random columns in random stored order: unsorted, repeats likely in short ranges"""
    lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), (M,)) if N else np.zeros(M, dtype=np.int64)
    rows = np.repeat(np.arange(M), lens)
    cols = rng.integers(0, max(N, 1), rows.size)
    vals = si.order_values(rng, rows.size) if values is None else values(rng, rows.size)
    return csr(M, N, rows, cols, vals)


def integer_values(rng, n):
    return rng.integers(-4, 5, n).astype(np.float64)


def distinct_csr(rng, M, N, lens, values=None):
    """rows of the given lengths with DISTINCT random columns in random stored order"""
    lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), (M,))
    rows = np.repeat(np.arange(M), lens)
    cols = np.concatenate([rng.choice(N, size=int(n), replace=False) for n in lens]) if rows.size else np.zeros(0, dtype=np.int64)
    vals = si.order_values(rng, rows.size) if values is None else values(rng, rows.size)
    return csr(M, N, rows, cols, vals)


def laplacian7(nx, ny, nz, values=None):
    """the 7-point Laplacian, rows ascending"""
    idx = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(idx.size, 6.0)]
    for ax in range(3):
        lo = np.take(idx, np.arange(idx.shape[ax] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, idx.shape[ax]), axis=ax).ravel()
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [np.full(lo.size, -1.0)] * 2
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.lexsort((cols, rows))
    M = idx.size
    A = csr(M, M, rows[o], cols[o], vals[o])
    if values is not None:
        A = A[:4] + (values(np.random.default_rng(M), A[3].size),)
    return A


def aggregation(nx, ny, nz):
    """P of the 2 x 2 x 2 aggregation: fine vertex (x, y, z) -> coarse (x // 2, y // 2, z // 2), every value 1.0"""
    cx, cy, cz = (nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    coarse = ((x // 2) * cy + (y // 2)) * cz + z // 2
    M = nx * ny * nz
    return csr(M, cx * cy * cz, np.arange(M), coarse.ravel(), np.ones(M))


def mixed_37x53x29(rng):
    """37 x 53 times 53 x 29, unsorted rows and repeats in both; B's row 5 repeats column 3 at entries 10 and 40 (inside one
    64-entry span), its row 9 repeats column 7 at entries 2 and 67 (one more than 64 entries apart)"""
    la = rng.integers(0, 12, 37)
    la[3] = max(la[3], 2)
    A = random_csr(rng, 37, 53, la)
    lens = rng.integers(0, 9, 53)
    lens[5], lens[9] = 50, 90
    B = random_csr(rng, 53, 29, lens)
    irp, ja = B[2].astype(np.int64), B[3].copy()
    ja[irp[5]:irp[6]] = np.resize(np.delete(np.arange(29), 3), 50)
    ja[irp[5] + 10] = ja[irp[5] + 40] = 3
    ja[irp[9]:irp[10]] = np.resize(np.delete(np.arange(29), 7), 90)
    ja[irp[9] + 2] = ja[irp[9] + 67] = 7
    A[3][int(A[2][3]):int(A[2][3]) + 2] = (5, 9)                    # row 3 of A (at least two entries) reaches both
    return A, (B[0], B[1], B[2], ja, B[4])


def special_values(rng, A, B):
    """+Inf, -0.0 and +0.0 among A's values, B positive: Inf and signed-zero sums, and no NaN (no Inf meets a zero or an
    opposite Inf)"""
    a, b = A[4].copy(), np.abs(B[4]) + 0.5
    at = rng.choice(a.size, size=min(a.size, 12), replace=False)
    a[at[:3]] = np.inf
    a[at[3:6]] = -0.0
    a[at[6:9]] = 0.0
    return A[:4] + (a,), B[:4] + (b,)


def small_cases():
    rng = np.random.default_rng(2200)
    cases = {}
    cases["1x1"] = (csr(1, 1, [0], [0], [-2.5]), csr(1, 1, [0], [0], [3.0]))
    cases["mixed37x53x29"] = mixed_37x53x29(rng)
    A, B = mixed_37x53x29(rng)
    cases["special"] = special_values(rng, A, B)
    # cancelling pairs: A's row holds (k, a) and (k, -a): every accumulator of the row ends at +0.0, and is stored
    k = rng.integers(0, 8, 12)
    a = si.order_values(rng, 12)
    cases["cancel"] = (csr(12, 8, np.repeat(np.arange(12), 2), np.repeat(k, 2), np.column_stack([a, -a]).ravel()),
                       random_csr(rng, 8, 11, 4))
    # all products -0.0: the sum is +0.0
    cases["negzero"] = (csr(2, 2, [0, 0, 1], [0, 1, 1], [-0.0, 0.0, -0.0]), csr(2, 3, [0, 0, 1, 1], [2, 0, 0, 2], [1.0, 2.0, -3.0, 4.0]))
    cases["empty_rows"] = (random_csr(rng, 9, 6, [0, 3, 0, 0, 2, 1, 0, 4, 0]), random_csr(rng, 6, 7, [2, 0, 3, 0, 0, 1]))
    cases["integer"] = (random_csr(rng, 20, 15, 6, integer_values), random_csr(rng, 15, 18, 5, integer_values))
    return cases


def nan_case():
    rng = np.random.default_rng(2201)
    A, B = mixed_37x53x29(rng)
    a, b = A[4].copy(), B[4].copy()
    a.view(np.uint64)[::17] = 0x7FF8000000000001
    b.view(np.uint64)[5::29] = 0xFFF800000000BEEF
    a[3] = np.inf
    b[::31] = 0.0                                                   # Inf * 0 among them
    return A[:4] + (a,), B[:4] + (b,)
