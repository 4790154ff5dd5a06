"""Inputs that make the serial-order contract of hipSpMVRowsCSR observable (tests/test_gpu_serial_order.py, and the host
checks in tests/test_serial_order_inputs.py that show the inputs would catch another order).

The contract is "the bits of sgemvSerial": a row starts at +0.0 and adds its products in stored (ascending-j) order.  The
inputs are built so that any other order shows:
  * order-sensitive values: a and x are U(-1, 1) * 10^k with k in -4..4 and mixed signs, so the rounding of a partial sum
    depends on what was added before it.  (A wider spread lets one product dominate its row, and then most orders give
    the same bits: at 10^+-12 only about 35 % of the rows change when reversed, at 10^+-4 about 65 %.)
  * repeated columns: sorted rows with runs of ONE column (2, 63, 64, 65, 130 entries and one row of 70 000), each entry
    with its own product of one magnitude (no entry dominates the row), so the stored order of equal columns -- which a
    stable sort keeps and an unstable one does not -- decides the bits;
  * signed zeros: x and the values hold +0.0 and -0.0, rows whose products are all -0.0 (the oracle gives +0.0), single
    -0.0 products, runs that cancel exactly (a, -a), and empty rows at the first, the last and at bin edges.
Everything is built with vectorised numpy; only the few dozen special rows are listed one by one."""
import functools

import numpy as np

AUTO_MIN_NNZ = 1 << 18            # the serial-order selection offers the format kernels from this size on
SLICE = 1 << 14                   # columns per slice of the two-phase format (tiles.hip PB_CBITS)
RUN_LENGTHS = (2, 63, 64, 65, 130)
LONG_RUN = 70_000                 # longer than a 16-bit local count


def order_values(rng, n, e=4):
    return rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-e, e + 1, n)


def assemble(M, rows, cols, vals):
    """CSR from entries listed in stored order within each row (rows need not be grouped yet: stable by row)"""
    order = np.argsort(rows, kind="stable")
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return IRP, cols[order].astype(np.uint64), vals[order].astype(np.float64)


def row_of_entry(IRP):
    return np.repeat(np.arange(IRP.size - 1), np.diff(IRP.astype(np.int64)))


def permuted(IRP, JA, AS, perm):
    return IRP, JA[perm], AS[perm]


def reversed_rows(IRP):
    """permutation that reverses every row's entries"""
    r = row_of_entry(IRP)
    b, e = IRP[:-1].astype(np.int64), IRP[1:].astype(np.int64)
    return b[r] + e[r] - 1 - np.arange(r.size)


def stable_rows_by(IRP, key):
    """permutation that sorts every row's entries by key, stably (equal keys keep their stored order)"""
    return np.lexsort((key, row_of_entry(IRP)))


def runs_reversed(IRP, JA):
    """permutation that reverses every run of equal columns inside a row and keeps everything else in place"""
    r = row_of_entry(IRP)
    n = r.size
    new = np.ones(n, dtype=bool)
    new[1:] = (r[1:] != r[:-1]) | (JA[1:] != JA[:-1])
    run = np.cumsum(new) - 1
    starts = np.flatnonzero(new)
    ends = np.append(starts[1:], n)
    return starts[run] + ends[run] - 1 - np.arange(n)


class Input:
    def __init__(self, name, M, N, IRP, JA, AS, x, special):
        self.name, self.M, self.N, self.IRP, self.JA, self.AS, self.x = name, M, N, IRP, JA, AS, x
        self.special = special        # kind of special row -> row indices

    def lens(self):
        return np.diff(self.IRP.astype(np.int64))

    def with_values(self, AS):
        return Input(self.name, self.M, self.N, self.IRP, self.JA, AS, self.x, self.special)


def _empty_rows(M):
    """row 0, the last row, and both sides of the bin edges of the formats (64-row multiples; sub-bins of 1250, bins of
    5000 and 20 000 rows)"""
    e = {0, M - 1}
    for b in (64 * 97, 1250, 5000, 20000):
        for k in range(1, M // b + 1):
            e.update({k * b - 1, k * b})
    return np.array(sorted(r for r in e if 0 <= r < M), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def make(name):
    """name: "mixed" (every special row, M = 45 001, N = 2^17 + 1), "narrow17" (N = 2^17 - 1, rows that span all columns),
    "widespan" (N = 2^20, columns of most rows below 40 000 and a few at the far end: a stripes step spans >= 2^17
    columns, so the format picks the 32-bit-column encoding by itself)"""
    seed = {"mixed": 11, "narrow17": 12, "widespan": 13}[name]
    rng = np.random.default_rng(seed)
    M, N = {"mixed": (45_001, (1 << 17) + 1), "narrow17": (40_003, (1 << 17) - 1), "widespan": (30_002, 1 << 20)}[name]
    x = order_values(rng, N)
    zc = rng.choice(N, size=N // 25, replace=False)               # 4 % of x is a signed zero, half of them -0.0
    x[zc[: zc.size // 2]] = 0.0
    x[zc[zc.size // 2:]] = -0.0
    pos0, neg0 = zc[: zc.size // 2], zc[zc.size // 2:]
    empty = _empty_rows(M)
    free = np.setdiff1d(np.arange(M), empty)
    n_special = 120
    special_rows = np.sort(rng.choice(free[1:-1], size=n_special, replace=False))
    base_rows = np.setdiff1d(free, special_rows)
    # base: 0..32 entries a row, sorted columns, repeats allowed (a non-decreasing row counts as sorted)
    lens = np.zeros(M, dtype=np.int64)
    lens[base_rows] = rng.integers(0, 33, base_rows.size)
    rows = np.repeat(np.arange(M), lens)
    hi = 40_000 if name == "widespan" else N
    cols = rng.integers(0, hi, rows.size)
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    vals = order_values(rng, rows.size)
    z = rng.random(rows.size)
    vals[z < 0.01] = 0.0
    vals[(z >= 0.01) & (z < 0.02)] = -0.0
    parts_r, parts_c, parts_v = [rows], [cols], [vals]
    special = {}
    it = iter(special_rows)

    def add(kind, c, v):
        r = next(it)
        special.setdefault(kind, []).append(r)
        c = np.asarray(c, dtype=np.int64)
        parts_r.append(np.full(c.size, r))
        parts_c.append(c)
        parts_v.append(np.asarray(v, dtype=np.float64))

    def sorted_cols(n, lo, hi_):
        return np.sort(rng.integers(lo, hi_, n))

    run_cols = np.unique(np.minimum([SLICE - 1, SLICE, SLICE + 5, N // 2, N - 1, 5], N - 1))
    x[run_cols] = rng.uniform(0.5, 2.0, run_cols.size) * rng.choice([-1.0, 1.0], run_cols.size)

    def unit_products(c):
        """values whose products with x are U(-1, 1) (x != 0), so that no entry of the row dominates it"""
        xc = np.abs(x[c])
        return rng.uniform(-1.0, 1.0, c.size) / np.where(xc > 0, xc, 1.0)

    # runs of one column, starting at several offsets of the row (lane 30, 63, 64 of the row's first wavefront ...), at
    # the slice edge, in the middle, at the last column
    for L in RUN_LENGTHS:
        for pre, c in ((0, SLICE - 1), (30, SLICE), (63, N // 2), (64, N - 1), (1, 5)):
            c = min(c, N - 1)
            left = sorted_cols(pre, 0, c)
            right = sorted_cols(int(rng.integers(0, 20)), c + 1, N) if c + 1 < N else np.zeros(0, np.int64)
            cc = np.concatenate([left, np.full(L, c), right])
            add("run" if L > 2 else "run-pair", cc, unit_products(cc))     # (a pair is added the same in both orders)
    # two runs meeting at the slice edge: 65 x column 16383, 65 x column 16384
    cc = np.concatenate([np.full(65, SLICE - 1), np.full(65, SLICE)])
    add("run", cc, unit_products(cc))
    if name == "mixed":
        add("long-run", np.full(LONG_RUN, SLICE + 5), unit_products(np.full(LONG_RUN, SLICE + 5)))
    # all products -0.0: (+v) x (-0.0), (-v) x (+0.0), (-0.0) x (+x); 1..6 entries
    for n in (1, 1, 1, 2, 3, 6, 6):
        kind = rng.integers(0, 3, n)
        c = np.where(kind == 0, rng.choice(neg0, n), np.where(kind == 1, rng.choice(pos0, n), 0))
        xp = np.flatnonzero(x > 0)
        c = np.where(kind == 2, rng.choice(xp, n), c)
        v = np.where(kind == 0, rng.uniform(0.5, 2, n), np.where(kind == 1, -rng.uniform(0.5, 2, n), -0.0))
        o = np.argsort(c, kind="stable")
        add("negzero" if n > 1 else "negzero-single", c[o], v[o])
    # exact cancellation inside a run: a, -a  /  a, -a, b, -b  (sum +0.0 in stored order; -0.0 seeds would show)
    for _ in range(6):
        c = int(rng.integers(0, N))
        a, b = order_values(rng, 2)
        add("cancel", [c, c], [a, -a])
        add("cancel", [c, c, c, c], [a, -a, b, -b])
    if name == "narrow17":                    # rows whose entries span the whole column range (0 and N - 1)
        for _ in range(8):
            cc = np.concatenate([[0], sorted_cols(int(rng.integers(1, 40)), 0, N), [N - 1]])
            add("span", cc, order_values(rng, cc.size))
    if name == "widespan":                    # a few entries far beyond the others: a stripes step spans >= 2^17 columns
        for _ in range(8):
            cc = np.concatenate([sorted_cols(int(rng.integers(1, 20)), 0, 40_000), [N - 1 - int(rng.integers(0, 4))]])
            add("span", cc, order_values(rng, cc.size))
    IRP, JA, AS = assemble(M, np.concatenate(parts_r), np.concatenate(parts_c), np.concatenate(parts_v))
    special = {k: np.array(v) for k, v in special.items()}
    special["empty"] = empty
    inp = Input(name, M, N, IRP, JA, AS, x, special)
    assert JA.size >= AUTO_MIN_NNZ and np.all(np.diff(JA.astype(np.int64))[np.diff(row_of_entry(IRP)) == 0] >= 0)
    return inp


def unit(inp):
    """the same pattern with every value -2.5 (a pattern handle: the kernels keep the value in a register)"""
    return inp.with_values(np.full(inp.JA.size, -2.5))


@functools.lru_cache(maxsize=None)
def sorted_with_long_rows(seed):
    """sorted matrix, distinct columns, nnz >= 2^18, whose row 7 and row 1000 hold 300 entries and whose last row 40"""
    rng = np.random.default_rng(seed)
    M, N = 30_001, 100_000
    lens = rng.integers(0, 25, M)
    lens[7] = lens[1000] = 300
    lens[-1] = 40
    rows = np.repeat(np.arange(M), lens)
    # distinct sorted columns per row: random gaps of >= 1
    gaps = rng.integers(1, 8, rows.size)
    first = np.r_[True, rows[1:] != rows[:-1]]
    cols = np.cumsum(gaps)
    cols -= np.repeat(cols[first] - gaps[first], lens[lens > 0])
    IRP, JA, AS = assemble(M, rows, cols, order_values(rng, rows.size))
    assert JA.size >= AUTO_MIN_NNZ and int(JA.max()) < N
    return M, N, IRP, JA, AS, order_values(rng, N)


def descending_pair(where, seed=5):
    """sorted everywhere except ONE descending pair: at the last two entries of the last row, or across entries 63/64 or
    127/128 of a row of 300.  Returns (M, N, IRP, JA, AS, x, row)."""
    M, N, IRP, JA, AS, x = sorted_with_long_rows(seed)
    JA, AS = JA.copy(), AS.copy()
    row, k = {"last-row": (M - 1, 38), "63/64": (7, 63), "127/128": (1000, 127)}[where]
    b, j = int(IRP[row]), int(IRP[row]) + k
    JA[j], JA[j + 1] = JA[j + 1], JA[j]
    # values of the pair for which the two orders of the pair give other bits (a kernel that sorted the row would show)
    rng = np.random.default_rng(seed)
    c = JA[b:int(IRP[row + 1])].astype(np.int64)
    a = AS[b:int(IRP[row + 1])]
    scale = max(abs(serial_sum(a[:k], x[c[:k]])), 1.0) / np.abs(x[c[k:k + 2]])       # products as large as the sum before them
    for _ in range(1000):
        AS[j:j + 2] = rng.uniform(-1.0, 1.0, 2) * scale
        swap = np.arange(a.size)
        swap[k], swap[k + 1] = k + 1, k
        if serial_sum(a, x[c]) != serial_sum(a[swap], x[c[swap]]):
            break
    return M, N, IRP, JA, AS, x, row


def serial_sum(a, x):
    """one row of sgemvSerial: +0.0, then every product in order"""
    s = 0.0
    for p in (a * x).tolist():
        s += p
    return s


@functools.lru_cache(maxsize=None)
def shuffled(seed=9):
    """every row's entries in random order; several 16 Ki-column slices, repeated columns"""
    rng = np.random.default_rng(seed)
    M, N = 25_003, 5 * SLICE + 77
    lens = rng.integers(0, 40, M)
    lens[[0, M - 1, 5000, 12500]] = 0
    rows = np.repeat(np.arange(M), lens)
    cols = rng.integers(0, N, rows.size)
    dup = rng.random(rows.size) < 0.1                      # some entries repeat their neighbour's column
    cols[1:][dup[1:] & (rows[1:] == rows[:-1])] = cols[:-1][dup[1:] & (rows[1:] == rows[:-1])]
    IRP, JA, AS = assemble(M, rows, cols, order_values(rng, rows.size))
    assert JA.size >= AUTO_MIN_NNZ
    return M, N, IRP, JA, AS, order_values(rng, N)


def stripes_order(IRP, JA):
    """the order the deterministic stripes forms add a row in: stable by column"""
    return stable_rows_by(IRP, JA.astype(np.int64))


def tiles_order(IRP, JA):
    """the order the deterministic two-phase form adds a row in: stable by 16 Ki-column slice"""
    return stable_rows_by(IRP, JA.astype(np.int64) >> 14)
