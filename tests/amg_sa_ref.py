"""The test side's reference of the smoothed-aggregation hierarchy of include/spmvHip.h (spmvHipAmgSetupSmoothed): the chain
P = T - w D^-1 A T, R = P^T, A' = R (A P) composed from the references of the public calls that the library chains
(amg_ref's aggregation and dinv, spgemm_ref's product and stable transpose, add_ref's sum), the one piece of arithmetic
that is the setup's own (rho_of: the row sums of |a_ij| in stored order, times |dinv|, and their max), and the cycle whose
correction is z = z + P e (cycle_ref; gather=True plants the plain hierarchy's e[agg] in its place).  SaCsr is the cycle as
the preconditioner of the Krylov reference loops.  numpy rounds every product and add on its own, as IEEE double does."""
import numpy as np

import add_ref as ad
import amg_ref as ar
import spgemm_ref as sr
from krylov_ref import Csr


def rho_of(A, dinv):
    """(rho, g): g_i = |dinv_i| * s_i, s_i the sum of |AS[p]| over row i in stored order from +0.0; rho = max g_i"""
    M, _, IRP, _, AS = A
    irp = IRP.astype(np.int64)
    lens = np.diff(irp)
    s = np.zeros(M)
    with np.errstate(all="ignore"):
        for t in range(int(lens.max()) if M else 0):
            live = np.flatnonzero(lens > t)
            s[live] = s[live] + np.abs(AS[irp[live] + t])
        g = np.abs(dinv) * s
    return (np.float64(g.max()) if M else np.float64(0.0)), g


def damping(rho, omegaP=0.0):
    """w of a level: the caller's omegaP, or (4/3) / rho -- two rounded divisions"""
    return np.float64(omegaP) if omegaP != 0.0 else (np.float64(4.0) / np.float64(3.0)) / rho


def diag_handle(dinv):
    return sr.csr(dinv.size, dinv.size, np.arange(dinv.size), np.arange(dinv.size), dinv)


def setup_ref(A, omegaP=0.0, **kw):
    """A = (M, M, IRP, JA, AS).  The levels of amg_ref.setup_ref with, but for the last, T (the unit prolongator), w, P, R,
    AP and their Csr forms"""
    o = ar._opts(kw)
    levels = []
    while True:
        M = A[0]
        lv = dict(A=A, dinv=ar.dinv_of(A), csr=Csr(M, A[2], A[3], A[4]))
        levels.append(lv)
        if M <= o["coarseRows"] or len(levels) == o["maxLevels"]:
            break
        agg = ar.aggregate_ref(M, A[2], A[3], o["seed"])
        nAgg = int(agg.max()) + 1
        if nAgg == M:
            break
        T = ar.prolongator(M, agg, nAgg)
        rho, g = rho_of(A, lv["dinv"])
        assert np.all(np.isfinite(g)) and 0.0 < rho < np.inf, "the setup refuses this level"
        w = damping(rho, omegaP)
        P = ad.add_ref(1.0, T, -w, sr.spgemm_ref(diag_handle(lv["dinv"]), sr.spgemm_ref(A, T)))
        R = sr.transpose(P)
        AP = sr.spgemm_ref(A, P)
        lv.update(agg=agg, T=T, rho=rho, w=w, P=P, R=R, AP=AP, Pcsr=Csr(P[0], P[2], P[3], P[4]), Rcsr=Csr(R[0], R[2], R[3], R[4]))
        A = sr.spgemm_ref(R, AP)
    return levels, o


def cycle_ref(levels, o, r, l=0, gather=False):
    """V(l, r) of the header with the correction z = z + P e (gather: the planted fault z = z + e[agg])"""
    lv = levels[l]
    last = l + 1 == len(levels)
    A, dinv, omega = lv["csr"], lv["dinv"], np.float64(o["omega"])
    with np.errstate(all="ignore"):
        sweeps = o["nuCoarse"] if last else o["nu1"]
        if sweeps == 0:
            z = np.zeros(A.M)
        else:
            z = omega * (dinv * r)
            for _ in range(sweeps - 1):
                t = A.spmv(z)
                z = z + omega * (dinv * (r - t))
        if last:
            return z
        d = r - A.spmv(z)
        e = cycle_ref(levels, o, lv["Rcsr"].spmv(d), l + 1, gather)
        z = z + (e[lv["agg"].astype(np.int64)] if gather else lv["Pcsr"].spmv(e))
        for _ in range(o["nu2"]):
            t = A.spmv(z)
            z = z + omega * (dinv * (r - t))
        return z


class SaCsr(Csr):
    """krylov_ref.Csr whose M^-1 v is the smoothed cycle"""

    def __init__(self, A, omegaP=0.0, **kw):
        super().__init__(A[0], A[2], A[3], A[4])
        self.levels, self.o = setup_ref(A, omegaP, **kw)
        self.F = self.levels                                   # (not None: the loops then call precond)

    def precond(self, v):
        return cycle_ref(self.levels, self.o, np.asarray(v, dtype=np.float64))


def complexity(levels):
    """sum of nnz over the levels / nnz of level 0 (1.0 for a matrix without entries, as the library reports)"""
    nnz = [lv["A"][3].size for lv in levels]
    return sum(nnz) / nnz[0] if nnz[0] else 1.0


# ------------------------------------------------------------------------------------------------------------- inputs
def with_one_diagonal(M, IRP, JA, seed=0):
    """(M, M, IRP, JA, AS) on a small graph's pattern made fit for the setup's STORED rule: the stored diagonal entries are
    dropped and ONE is put back per row at a random place of the row, everything else -- unsorted rows, repeated entries,
    one-directional edges, rows with nothing else -- stays.  Off-diagonal values are negative and not all alike, the
    diagonal dominates its row."""
    rng = np.random.default_rng(seed)
    irp = IRP.astype(np.int64)
    rows, cols, vals = [], [], []
    for i in range(M):
        off = [int(j) for j in JA[irp[i]:irp[i + 1]] if int(j) != i]
        v = [-(1.0 + 0.5 * rng.random()) for _ in off]
        at = int(rng.integers(0, len(off) + 1))
        off.insert(at, i)
        v.insert(at, 1.5 - sum(v) + rng.random())
        rows += [i] * len(off)
        cols += off
        vals += v
    m, irp2, ja2 = ar.pattern(M, rows, cols)
    return m, m, irp2, ja2, np.array(vals, dtype=np.float64)
