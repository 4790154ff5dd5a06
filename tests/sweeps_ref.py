"""The test side's references for the triangular solves by Jacobi sweeps (hipSpTRSVSweepsCSR, include/spmvHip.h):

    x0[i] = STORED ? b[i] / d_i : b[i]
    for s = 1 .. S:   for every i:
        acc = +0.0
        for p in IRP[i] .. IRP[i+1]-1   (stored order)
            j = JA[p];  if (lower ? j < i : j > i):  acc += AS[p] * x(s-1)[j]
        x(s)[i] = STORED ? (b[i] - acc) / d_i : (b[i] - acc)

written twice, independently: `sweeps_loop` is the literal loop in plain Python floats, one row and one entry at a time;
`sweeps_numpy` goes sweep by sweep over all rows at once, walking position k of every row that has one and skipping the
positions outside the triangle (never adding +0.0 in their place).  Both round every product and every add separately.
`sweeps_loop` also takes a planted `fault` (FAULTS) for the tests that show the inputs tell each one apart.
`SweepCsr` is krylov_ref.Csr with M^-1 = the sweep pair, for the preconditioned solver references."""
from fractions import Fraction

import numpy as np

from krylov_ref import Csr
from trsv_ref import diag_pos

FAULTS = ("sorted", "zero_added", "fma", "gauss_seidel", "reciprocal")


def _div(r, d):
    """IEEE double division (Python raises on / 0.0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(r) / np.float64(d))


def _fma(a, x, acc):
    """a * x + acc with one rounding (non-finite operands: as the plain expression gives)"""
    if not (np.isfinite(a) and np.isfinite(x) and np.isfinite(acc)):
        return acc + a * x
    return float(Fraction(a) * Fraction(x) + Fraction(acc))


def sweeps_loop(M, IRP, JA, AS, b, S, lower=True, unit=False, fault=None):
    """the loop above, one row and one entry at a time"""
    assert fault is None or fault in FAULTS
    irp, ja, a = [int(v) for v in IRP], [int(v) for v in JA], [float(v) for v in AS]
    bb = [float(v) for v in b]
    d = [None] * M
    if not unit:
        for i in range(M):
            on = [p for p in range(irp[i], irp[i + 1]) if ja[p] == i]
            assert len(on) == 1, f"row {i}: {len(on)} diagonal entries"
            d[i] = a[on[0]]

    def scale(r, i):
        if unit:
            return r
        return r * _div(1.0, d[i]) if fault == "reciprocal" else _div(r, d[i])

    x = [scale(bb[i], i) for i in range(M)]
    for _ in range(S):
        prev = x if fault == "gauss_seidel" else list(x)
        new = prev if fault == "gauss_seidel" else [0.0] * M
        order = range(M) if lower else range(M - 1, -1, -1)      # (any order without the fault: rows read only prev)
        for i in order:
            ps = list(range(irp[i], irp[i + 1]))
            if fault == "sorted":
                ps.sort(key=lambda p: ja[p])
            acc = 0.0
            for p in ps:
                j = ja[p]
                if ((j < i) if lower else (i < j < M)):
                    acc = _fma(a[p], prev[j], acc) if fault == "fma" else acc + a[p] * prev[j]
                elif fault == "zero_added":
                    acc = acc + a[p] * 0.0
            new[i] = scale(bb[i] - acc, i)
        x = new
    return np.array(x, dtype=np.float64)


def sweeps_numpy(M, IRP, JA, AS, b, S, lower=True, unit=False):
    """sweep by sweep, every row's ordered sum advanced together position by position (same bits as sweeps_loop)"""
    IRP = np.asarray(IRP, dtype=np.int64)
    JA = np.asarray(JA, dtype=np.int64)
    AS = np.asarray(AS, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if M == 0:
        return b.copy()
    lens = np.diff(IRP)
    rows_at = [np.flatnonzero(lens > k) for k in range(int(lens.max()))]
    steps = []                                            # per position k: (rows, CSR positions, columns) inside the triangle
    for k, rows in enumerate(rows_at):
        p = IRP[rows] + k
        j = JA[p]
        tri = (j < rows) if lower else ((j > rows) & (j < M))
        steps.append((rows[tri], p[tri], j[tri]))
    with np.errstate(all="ignore"):
        if unit:
            dv = None
            x = b.copy()
        else:
            dpos, bad = diag_pos(M, IRP, JA)
            assert bad < 0, f"row {bad} does not hold exactly one diagonal entry"
            dv = AS[dpos]
            x = b / dv
        for _ in range(S):
            acc = np.zeros(M)
            for rows, p, j in steps:
                acc[rows] = acc[rows] + AS[p] * x[j]
            r = b - acc
            x = r if unit else r / dv
    return x


def sweeps_block(M, IRP, JA, AS, B, S, lower=True, unit=False):
    """column by column the single solve"""
    B = np.asarray(B, dtype=np.float64)
    return np.stack([sweeps_numpy(M, IRP, JA, AS, B[:, c], S, lower, unit) for c in range(B.shape[1])], axis=1) if B.shape[1] else B.copy()


class SweepCsr(Csr):
    """krylov_ref.Csr whose M^-1 v is U~^-1 (L~^-1 v) by s_lower unit lower and s_upper stored upper sweeps on the factors F"""

    def __init__(self, M, IRP, JA, AS, F, s_lower, s_upper):
        super().__init__(M, IRP, JA, AS, F)
        self.s_lower, self.s_upper = s_lower, s_upper
        self.applications = 0

    def precond(self, v):
        self.applications += 1
        w = sweeps_numpy(self.M, self.IRP, self.JA, self.F, v, self.s_lower, True, True)
        return sweeps_numpy(self.M, self.IRP, self.JA, self.F, w, self.s_upper, False, False)
