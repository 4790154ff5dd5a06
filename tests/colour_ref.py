"""Test-side reference of spmvHipColourCSR, spmvHipCsrPermute and spmvHipVecPermute (include/spmvHip.h): the colouring
loop in plain Python (colour_loop) and in numpy rounds (colour_ref), the (colour, id) order, the symmetric permutation
with its stable in-row order, and the small pattern cases both test files share."""
import numpy as np

NATURAL, HASH = 0, 1
M32 = 0xFFFFFFFF


def fmix32(h):
    """the murmur3 32-bit finaliser on a Python int"""
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def fmix32_np(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def rank(M, order, seed=0):
    """rank[i]: j wins against i exactly when rank[j] < rank[i]"""
    ids = np.arange(M, dtype=np.int64)
    if order == NATURAL:
        return ids
    key = fmix32_np(ids.astype(np.uint64) ^ np.uint64(seed & M32)).astype(np.int64)
    o = np.lexsort((-ids, -key))                               # descending (key, id)
    r = np.empty(M, dtype=np.int64)
    r[o] = ids
    return r


def colour_loop(M, IRP, JA, order, seed=0, incoming=True):
    """the loop of include/spmvHip.h in plain Python.  incoming=False plants the fault of ignoring the transposed edges."""
    adj = [set() for _ in range(M)]
    for i in range(M):
        for p in range(int(IRP[i]), int(IRP[i + 1])):
            j = int(JA[p])
            if j == i or j >= M:
                continue
            adj[i].add(j)
            if incoming:
                adj[j].add(i)

    def wins(j, i):
        if order == NATURAL:
            return j < i
        return (fmix32(j ^ seed), j) > (fmix32(i ^ seed), i)

    if order == NATURAL:
        seq = list(range(M))
    else:
        seq = sorted(range(M), key=lambda i: (fmix32(i ^ seed), i), reverse=True)
    colour = [None] * M
    for i in seq:
        used = {colour[j] for j in adj[i] if wins(j, i)}
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    return np.array(colour, dtype=np.uint32).reshape(M)


def colour_ref(M, IRP, JA, order, seed=0):
    """the same colours by Jones-Plassmann rounds on numpy arrays.  Returns (colour, rounds): rounds as a device that
    never sees a colour written in the same round would count them."""
    IRP = np.asarray(IRP, dtype=np.int64)
    JA = np.asarray(JA, dtype=np.int64)
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(IRP))
    keep = (JA != rows) & (JA < M)
    a, b = np.concatenate([rows[keep], JA[keep]]), np.concatenate([JA[keep], rows[keep]])
    rk = rank(M, order, seed)
    w = rk[b] < rk[a]                                          # edges (a <- b) along which b wins against a
    a, b = a[w], b[w]
    colour = np.full(M, -1, dtype=np.int64)
    rounds = 0
    todo = np.ones(M, dtype=bool)
    while todo.any():
        blocked = np.zeros(M, dtype=bool)
        blocked[a[colour[b] < 0]] = True
        ready = np.flatnonzero(todo & ~blocked)
        assert ready.size
        e = np.isin(a, ready)
        ea, ec = a[e], colour[b[e]]
        new = np.zeros(ready.size, dtype=np.int64)
        pos = np.full(M, -1, dtype=np.int64)
        pos[ready] = np.arange(ready.size)
        if ea.size:                                            # first-fit: the smallest c with no (row, c) among the edges
            o = np.lexsort((ec, ea))
            ea, ec = ea[o], ec[o]
            first = np.r_[True, (ea[1:] != ea[:-1]) | (ec[1:] != ec[:-1])]
            ea, ec = ea[first], ec[first]
            start = np.r_[True, ea[1:] != ea[:-1]]
            idx = np.arange(ea.size) - np.maximum.accumulate(np.where(start, np.arange(ea.size), 0))
            gap = ec != idx                                    # the k-th distinct colour of a row is k until the first gap
            mex = np.bincount(ea, minlength=M)                 # no gap: the number of distinct colours
            g = np.flatnonzero(gap)
            if g.size:
                fg = np.full(M, np.iinfo(np.int64).max, dtype=np.int64)
                np.minimum.at(fg, ea[g], idx[g])
                mex = np.minimum(mex, fg)
            new = mex[ready]
        colour[ready] = new
        todo[ready] = False
        rounds += 1
    return colour.astype(np.uint32), rounds


def perm_of(colour):
    """rows by (colour, id): perm[new] = old"""
    return np.argsort(np.asarray(colour, dtype=np.int64), kind="stable").astype(np.uint32)


def is_proper(M, IRP, JA, colour):
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(np.asarray(IRP, dtype=np.int64)))
    JA = np.asarray(JA, dtype=np.int64)
    keep = (JA != rows) & (JA < M)
    return bool(np.all(colour[rows[keep]] != colour[JA[keep]]))


def permute_ref(M, IRP, JA, AS, perm):
    """B = P A P^T: row r of B = row perm[r] of A, column j -> inv[j], sorted by new column, stable.  Returns
    (IRP, JA, AS, map) with AS_B[p] = AS[map[p]]."""
    IRP = np.asarray(IRP, dtype=np.int64)
    JA = np.asarray(JA, dtype=np.int64)
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(M, dtype=np.int64)
    inv[perm] = np.arange(M)
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(IRP))
    o = np.lexsort((np.arange(JA.size), inv[JA], inv[rows]))   # new row, then new column, then the stored position
    irp = np.zeros(M + 1, dtype=np.int64)
    irp[1:] = np.cumsum(np.bincount(inv[rows], minlength=M))
    return irp.astype(np.uint32), inv[JA][o].astype(np.uint32), np.asarray(AS, dtype=np.float64)[o], o.astype(np.uint32)


# ------------------------------------------------------------------------------------------------- patterns
def csr_of(M, rows, cols):
    """CSR pattern of the (row, col) list in the given order within each row"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    o = np.argsort(rows, kind="stable")
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return IRP, cols[o].astype(np.uint64)


def laplacian7(nx, ny, nz):
    """7-point stencil pattern, x fastest, sorted rows with the diagonal; values 6 / -1"""
    ids = np.arange(nx * ny * nz, dtype=np.int64)
    x, y, z = ids % nx, ids // nx % ny, ids // (nx * ny)
    rows, cols = [ids], [ids]
    for ok, d in ((z > 0, -nx * ny), (y > 0, -nx), (x > 0, -1), (x < nx - 1, 1), (y < ny - 1, nx), (z < nz - 1, nx * ny)):
        rows.append(ids[ok])
        cols.append(ids[ok] + d)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    IRP = np.zeros(ids.size + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=ids.size))
    return ids.size, IRP, cols.astype(np.uint64), np.where(rows == cols, 6.0, -1.0)


def bidiagonal(M):
    """strictly one-directional: row i stores (i, i) and (i, i-1) only"""
    rows = np.r_[np.arange(M), np.arange(1, M)]
    cols = np.r_[np.arange(M), np.arange(0, M - 1)]
    o = np.lexsort((cols, rows))
    return (M,) + csr_of(M, rows[o], cols[o])


def no_diagonal(M, seed=7):
    """a random pattern without a diagonal entry, not symmetric, some empty rows"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(M), rng.integers(0, 5, M))
    cols = (rows + rng.integers(1, M, rows.size)) % M
    return (M,) + csr_of(M, rows, cols)


def unsorted_repeats(M=90, seed=11):
    """unsorted rows, every pair stored twice, the diagonal in the middle"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(M), 3)
    cols = rng.integers(0, M, rows.size)
    rows, cols = np.r_[rows, np.arange(M), rows], np.r_[cols, np.arange(M), cols]
    o = rng.permutation(rows.size)
    return (M,) + csr_of(M, rows[o], cols[o])


def clique_star(clique=70, leaves=300):
    """a `clique`-clique (upper triangle stored only: the other direction comes in transposed) whose vertex 0 is also
    the hub of a star: more than 64 colours, and rows of more than 64 adjacency entries"""
    r, c = np.triu_indices(clique, 1)
    hub = np.zeros(leaves, dtype=np.int64)
    leaf = clique + np.arange(leaves)
    M = clique + leaves
    rows, cols = np.r_[r, leaf, np.arange(M)], np.r_[c, hub, np.arange(M)]
    o = np.lexsort((cols, rows))
    return (M,) + csr_of(M, rows[o], cols[o])


def chain(M):
    """symmetric tridiagonal pattern: under NATURAL the longest ascending path has M vertices"""
    rows = np.r_[np.arange(M), np.arange(1, M), np.arange(0, M - 1)]
    cols = np.r_[np.arange(M), np.arange(0, M - 1), np.arange(1, M)]
    o = np.lexsort((cols, rows))
    return (M,) + csr_of(M, rows[o], cols[o])


def random_sym(M, seed):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(M), 3)
    cols = rng.integers(0, max(M, 1), rows.size)
    rows, cols = np.r_[rows, cols, np.arange(M)], np.r_[cols, rows, np.arange(M)]
    key = np.unique(rows * max(M, 1) + cols)
    return (M,) + csr_of(M, key // max(M, 1), key % max(M, 1))


def small_cases():
    """name -> (M, IRP, JA): every small pattern of the GPU test"""
    out = {f"random{M}": random_sym(M, 100 + M) for M in (0, 1, 255, 256, 257)}
    out["laplacian12x10x8"] = laplacian7(12, 10, 8)[:3]
    out["bidiagonal"] = bidiagonal(200)
    out["no_diagonal"] = no_diagonal(150)
    out["unsorted_repeats"] = unsorted_repeats()
    out["clique_star"] = clique_star()
    return out


CONFIGS = ((NATURAL, 0), (HASH, 0), (HASH, 0x9E3779B9))
