"""The test side's references for spmvHipFsaiSetup / spmvHipFsaiApply (include/spmvHip.h): the factorised sparse approximate
inverse G of a square CSR matrix, G^T G ~ A^-1.

Row i of G stores P = (the columns j < i of row i of the pattern, then i); its values are the loop of the header on the dense
block B = A(P, P), of which only the lower triangle is read:

  fsai_loop    the header's loop, scalar by scalar, on Python floats (IEEE double; every product, difference, quotient and
               square root rounded on its own)
  fsai_vec     all rows of equal n together with numpy, in the same operation order: every entry of B gets its updates one
               at a time in ascending k, every acc[t] its terms in descending s
  fsai_crout   deliberately different: the left-looking form sums an entry's updates first and subtracts once, and adds
               acc[t] in ascending s -- the same numbers to rounding, other bits

A matrix is (M, N, IRP, JA, AS) with strictly ascending rows, as everywhere in the suite; a result is (G, info) with G such
a tuple and info = dict(nnz, maxRow, badRows, firstBadRow)."""
import math

import numpy as np

import serial_order_inputs as si
from krylov_ref import Csr
from transpose_ref import stable_transpose

MAX_ROW = 64


def pattern(M, IRPs, JAs):
    """(IRPg, JAg) of G: row i holds the columns j < i of row i of the pattern, ascending, then i"""
    IRPs, JAs = np.asarray(IRPs).astype(np.int64), np.asarray(JAs).astype(np.int64)
    rows = si.row_of_entry(IRPs)
    low = JAs < rows
    r = np.concatenate([rows[low], np.arange(M, dtype=np.int64)])
    c = np.concatenate([JAs[low], np.arange(M, dtype=np.int64)])
    o = np.lexsort((c, r))
    IRPg = np.zeros(M + 1, dtype=np.int64)
    IRPg[1:] = np.cumsum(np.bincount(r, minlength=M))
    return IRPg, c[o]


class _Lookup:
    """the value of the stored entry (r, c) of A, +0.0 where row r stores no column c"""

    def __init__(self, A):
        M, _, IRP, JA, AS = A
        self.M = max(int(M), 1)
        self.keys = si.row_of_entry(np.asarray(IRP)).astype(np.int64) * self.M + np.asarray(JA).astype(np.int64)
        assert np.all(np.diff(self.keys) > 0), "rows must ascend strictly"
        self.AS = np.asarray(AS, dtype=np.float64)

    def __call__(self, r, c):
        key = np.asarray(r, dtype=np.int64) * self.M + np.asarray(c, dtype=np.int64)
        at = np.minimum(np.searchsorted(self.keys, key), max(self.keys.size - 1, 0))
        if self.keys.size == 0:
            return np.zeros(key.shape)
        return np.where(self.keys[at] == key, self.AS[at], 0.0)


def blocks(look, IRPg, JAg, n):
    """(rows, B): the rows of G with n entries and their dense blocks B[r][s][t] = A(p_s, p_t) for t <= s (+0.0 above);
    look: _Lookup(A)"""
    rows = np.flatnonzero(np.diff(IRPg) == n)
    P = JAg[IRPg[rows][:, None] + np.arange(n)[None, :]]
    return rows, np.tril(look(P[:, :, None], P[:, None, :]))


# ----------------------------------------------------------------------------------------------- one row, scalar by scalar
def _bad(v):
    return not (v > 0.0) or v == math.inf


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan


def row_loop(B):
    """g of the header's loop for one dense block (a list of n lists of floats; the lower triangle is used); None: BAD"""
    n = len(B)
    B = [list(map(float, row)) for row in B]
    for k in range(n):
        if _bad(B[k][k]):
            return None
        B[k][k] = math.sqrt(B[k][k])
        for s in range(k + 1, n):
            B[s][k] = B[s][k] / B[k][k]
        for t in range(k + 1, n):
            for s in range(t, n):
                B[s][t] = B[s][t] - B[s][k] * B[t][k]
    y = [0.0] * n
    y[n - 1] = (1.0 / B[n - 1][n - 1]) / B[n - 1][n - 1]
    for t in range(n - 2, -1, -1):
        acc = 0.0
        for s in range(n - 1, t, -1):
            acc = acc + B[s][t] * y[s]
        y[t] = (0.0 - acc) / B[t][t]
    d = _sqrt(y[n - 1])
    if _bad(d):
        return None
    return [v / d for v in y]


def row_crout(B):
    """the same row by the left-looking form: sum first, subtract once; acc[t] in ascending s.  None: BAD"""
    n = len(B)
    A = [list(map(float, row)) for row in B]
    L = [[0.0] * n for _ in range(n)]
    for s in range(n):
        for t in range(s + 1):
            acc = 0.0
            for k in range(t):
                acc = acc + L[s][k] * L[t][k]
            v = A[s][t] - acc
            if t == s:
                if _bad(v):
                    return None
                L[s][s] = math.sqrt(v)
            else:
                L[s][t] = v / L[t][t]
    y = [0.0] * n
    y[n - 1] = (1.0 / L[n - 1][n - 1]) / L[n - 1][n - 1]
    for t in range(n - 2, -1, -1):
        acc = 0.0
        for s in range(t + 1, n):
            acc = acc + L[s][t] * y[s]
        y[t] = (0.0 - acc) / L[t][t]
    d = _sqrt(y[n - 1])
    if _bad(d):
        return None
    return [v / d for v in y]


# ------------------------------------------------------------------------------------ all rows of one n, the loop's order
def rows_vec(B):
    """(g, bad) for the blocks B (R, n, n), every row by the operations of row_loop in its order"""
    B = np.array(B, dtype=np.float64)
    R, n, _ = B.shape
    bad = np.zeros(R, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(n):
            p = B[:, k, k]
            bad |= ~(p > 0.0) | (p == np.inf)                        # (a BAD row's later numbers are never looked at)
            d = np.sqrt(p)
            B[:, k, k] = d
            B[:, k + 1:, k] = B[:, k + 1:, k] / d[:, None]
            col = B[:, k + 1:, k]
            B[:, k + 1:, k + 1:] = B[:, k + 1:, k + 1:] - col[:, :, None] * col[:, None, :]     # (only t <= s is ever read)
        y = np.zeros((R, n))
        dn = B[:, n - 1, n - 1]
        y[:, n - 1] = (1.0 / dn) / dn
        acc = np.zeros((R, n))
        for s in range(n - 1, 0, -1):
            acc[:, :s] = acc[:, :s] + B[:, s, :s] * y[:, s:s + 1]
            y[:, s - 1] = (0.0 - acc[:, s - 1]) / B[:, s - 1, s - 1]
        d = np.sqrt(y[:, n - 1])
        bad |= ~(d > 0.0) | (d == np.inf)
        g = y / d[:, None]
    g[bad] = 0.0
    g[bad, n - 1] = 1.0
    return g, bad


# --------------------------------------------------------------------------------------------------------- whole matrices
def _run(A, S, per_block):
    M = A[0]
    S = A if S is None else S
    assert S[0] == M
    IRPg, JAg = pattern(M, S[2], S[3])
    lens = np.diff(IRPg)
    if M and int(lens.max()) > MAX_ROW:
        raise ValueError(f"row {int(np.flatnonzero(lens > MAX_ROW)[0])} of the pattern gives more than {MAX_ROW} entries")
    ASg = np.zeros(JAg.size)
    bad_rows = []
    look = _Lookup(A)
    for n in np.unique(lens):
        rows, B = blocks(look, IRPg, JAg, int(n))
        g, bad = per_block(B)
        ASg[IRPg[rows][:, None] + np.arange(int(n))[None, :]] = g
        bad_rows += list(rows[bad])
    info = dict(nnz=int(JAg.size), maxRow=int(lens.max()) if M else 0, badRows=len(bad_rows), firstBadRow=min(bad_rows) if bad_rows else -1)
    return (M, M, IRPg.astype(np.uint64), JAg.astype(np.uint64), ASg), info


def _scalar(row_fn):
    def per_block(B):
        n = B.shape[1]
        g, bad = np.zeros((B.shape[0], n)), np.zeros(B.shape[0], dtype=bool)
        for r in range(B.shape[0]):
            v = row_fn(B[r].tolist())
            bad[r] = v is None
            g[r] = [0.0] * (n - 1) + [1.0] if v is None else v
        return g, bad
    return per_block


def fsai_loop(A, S=None):
    """(G, info) by the header's loop, scalar by scalar; S: the pattern matrix (None: A itself)"""
    return _run(A, S, _scalar(row_loop))


def fsai_crout(A, S=None):
    return _run(A, S, _scalar(row_crout))


def fsai_vec(A, S=None):
    """(G, info), the rows of equal n together"""
    return _run(A, S, rows_vec)


# ------------------------------------------------------------------------------------------------------------ the apply
def transposed(G):
    """G^T as spmvHipCsrTranspose makes it"""
    M, N, IRP, JA, AS = G
    IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, AS)
    return N, M, IRPt, JAt, ASt


class Applied:
    """z = G^T (G v), both products serial-order SpMV"""

    def __init__(self, G):
        T = transposed(G)
        self.G, self.T = Csr(G[0], G[2], G[3], G[4]), Csr(T[0], T[2], T[3], T[4])

    def __call__(self, v):
        return self.T.spmv(self.G.spmv(np.asarray(v, dtype=np.float64)))


class PrecondCsr(Csr):
    """krylov_ref's matrix whose M^-1 v is G^T (G v): what cg_ref / bicgstab_ref / gmres_ref take as A"""

    def __init__(self, A, G):
        super().__init__(A[0], A[2], A[3], A[4])
        self.F = G[4]                                                # (not None: the loops ask precond())
        self.apply = Applied(G)

    def precond(self, v):
        return self.apply(v)


def dense(A):
    M, N, IRP, JA, AS = A
    D = np.zeros((M, N))
    D[si.row_of_entry(np.asarray(IRP)), np.asarray(JA).astype(np.int64)] = AS
    return D
