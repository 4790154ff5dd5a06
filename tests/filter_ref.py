"""The test side's reference of spmvHipCsrFilter / spmvHipCsrFilterRefresh: the serial loop of include/spmvHip.h in plain Python
(filter_loop), a vectorised form of the same loop (filter_ref, filter_refresh_ref) and the strength-filtered smoothed
aggregation composed from it and the references of the calls the library chains (strength_setup_ref).  numpy rounds every
product and add on its own, as IEEE double does with no FMA; values are moved as bits."""
import numpy as np

import add_ref as ad
import amg_ref as ar
import amg_sa_ref as sa
import serial_order_inputs as si
import spgemm_ref as sr
from krylov_ref import Csr

BAND, ABS, STRENGTH = 0, 1, 2
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def opts(mode, lo=None, hi=None, theta=0.0, lump=False):
    return dict(mode=mode, lo=INT64_MIN if lo is None else int(lo), hi=INT64_MAX if hi is None else int(hi), theta=float(theta),
                lump=bool(lump))


def needs_diagonal(o):
    return o["lump"] or o["mode"] == STRENGTH


def diagonal_places(A):
    """the position of the one stored entry (i, i) of every row; raises with the first row that has not exactly one"""
    M, _, IRP, JA, _ = A
    rows = si.row_of_entry(IRP)
    at = np.flatnonzero(JA.astype(np.int64) == rows)
    count = np.bincount(rows[at], minlength=M)
    bad = np.flatnonzero(count != 1)
    if bad.size:
        raise ValueError(f"row {int(bad[0])} does not hold exactly one stored diagonal entry")
    return at


def _keep(A, o, dpos):
    M, _, IRP, JA, AS = A
    i, j = si.row_of_entry(IRP), JA.astype(np.int64)
    with np.errstate(all="ignore"):
        if o["mode"] == BAND:
            keep = np.array([o["lo"] <= int(b) - int(a) <= o["hi"] for a, b in zip(i, j)], dtype=bool)
        elif o["mode"] == ABS:
            keep = np.abs(AS) > np.float64(o["theta"])
        else:
            d = AS[dpos]
            tt = np.float64(o["theta"]) * np.float64(o["theta"])
            keep = AS * AS > tt * np.abs(d[i] * d[j])
    if needs_diagonal(o):
        keep = keep | (i == j)
    return keep


def _lump(A, keep, dpos, AS_new=None):
    """v_i = d_i, then + the dropped values of row i in stored order; also the rows with a dropped entry"""
    M, _, IRP, _, AS = A
    AS = AS if AS_new is None else AS_new
    v = AS[dpos].copy()
    drop = np.flatnonzero(~keep)
    rows = si.row_of_entry(IRP)[drop]
    n = np.bincount(rows, minlength=M)
    first = np.concatenate(([0], np.cumsum(n)[:-1])) if M else np.zeros(0, dtype=np.int64)
    with np.errstate(all="ignore"):
        for t in range(int(n.max()) if n.size else 0):
            live = np.flatnonzero(n > t)
            v[live] = v[live] + AS[drop[first[live] + t]]
    return v, int(np.count_nonzero(n))


def _gathered(A, keep, o, dpos, AS_new=None):
    M, N, IRP, JA, AS = A
    AS = AS if AS_new is None else AS_new
    kept = np.flatnonzero(keep)
    irp = np.zeros(M + 1, dtype=np.uint64)
    irp[1:] = np.cumsum(np.bincount(si.row_of_entry(IRP)[kept], minlength=M))
    val = AS[kept].copy()                                     # (fancy indexing moves the 8 bytes: payloads and -0.0 stay)
    lumped = 0
    if o["lump"]:
        v, lumped = _lump(A, keep, dpos, AS_new)
        val[np.searchsorted(kept, dpos)] = v
    return (M, N, irp, JA[kept].astype(np.uint64), val), kept, lumped


def filter_ref(A, o, info=False):
    """A = (M, N, IRP, JA, AS), o = opts(...).  Returns (C, kept): C's arrays and the positions in A of C's entries; with
    info also the rows that were lumped"""
    dpos = diagonal_places(A) if needs_diagonal(o) else None
    C, kept, lumped = _gathered(A, _keep(A, o, dpos), o, dpos)
    return (C, kept, lumped) if info else (C, kept)


def filter_refresh_ref(kept, A_new, o):
    """the build's kept set on A's new values: nothing is judged again"""
    keep = np.zeros(A_new[3].size, dtype=bool)
    keep[kept] = True
    dpos = diagonal_places(A_new) if o["lump"] else None
    return _gathered(A_new, keep, o, dpos)[0]


def filter_loop(A, o):
    """the loop of the header, entry by entry"""
    M, N, IRP, JA, AS = A
    diag = needs_diagonal(o)
    d = AS[diagonal_places(A)] if diag else None
    theta = np.float64(o["theta"])
    irp, ja, val, kept = [0], [], [], []
    with np.errstate(all="ignore"):
        for i in range(M):
            v = d[i] if o["lump"] else None
            at = None
            for p in range(int(IRP[i]), int(IRP[i + 1])):
                j, a = int(JA[p]), AS[p]
                if diag and j == i:
                    keep = True
                    at = len(ja)
                elif o["mode"] == BAND:
                    keep = o["lo"] <= j - i <= o["hi"]
                elif o["mode"] == ABS:
                    keep = bool(np.abs(a) > theta)
                else:
                    keep = bool(a * a > (theta * theta) * np.abs(d[i] * d[j]))
                if keep:
                    ja.append(j)
                    val.append(AS[p:p + 1])
                    kept.append(p)
                elif o["lump"]:
                    v = v + a
            if o["lump"]:
                val[at] = np.array([v])
            irp.append(len(ja))
    vals = np.concatenate(val) if val else np.zeros(0)
    return (M, N, np.array(irp, dtype=np.uint64), np.array(ja, dtype=np.uint64), vals), np.array(kept, dtype=np.int64)


def same_bits(C, R, what="", lumped=False):
    """indices exact, values as bits, a copied NaN with its payload.  lumped: a diagonal entry that is a NaN in the
    reference (an add made it: its payload is not pinned) only has to be a NaN"""
    assert (C[0], C[1]) == (R[0], R[1]), f"{what}: shape"
    assert np.array_equal(np.asarray(C[2], dtype=np.uint64), R[2]), f"{what}: IRP"
    assert np.array_equal(np.asarray(C[3], dtype=np.uint64), R[3]), f"{what}: JA"
    a, b = np.ascontiguousarray(C[4], dtype=np.float64), np.ascontiguousarray(R[4], dtype=np.float64)
    assert a.shape == b.shape, f"{what}: AS length"
    loose = np.zeros(b.size, dtype=bool)
    if lumped:
        loose = np.isnan(b) & (R[3].astype(np.int64) == si.row_of_entry(R[2]))
        assert np.isnan(a[loose]).all(), f"{what}: a lumped NaN"
    bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)) & ~loose)
    assert bad.size == 0, (f"{what}: {bad.size} of {b.size} values differ in their bits; first at {int(bad[0])}: "
                           f"0x{int(a.view(np.uint64)[bad[0]]):016x} != expected 0x{int(b.view(np.uint64)[bad[0]]):016x}")


def dense_keep(A, o):
    """the kept places of a matrix WITHOUT repeats as a dense boolean array, from the definitions alone"""
    D = sr.dense(A)
    M, N = D.shape
    i, j = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    stored = sr.pattern_of(A)
    with np.errstate(all="ignore"):
        if o["mode"] == BAND:
            k = (j - i >= max(o["lo"], -(1 << 40))) & (j - i <= min(o["hi"], 1 << 40))
        elif o["mode"] == ABS:
            k = np.abs(D) > o["theta"]
        else:
            d = np.diag(D)
            k = D * D > (np.float64(o["theta"]) * np.float64(o["theta"])) * np.abs(np.outer(d, d))
    if needs_diagonal(o):
        k = k | (i == j)
    return k & stored


# ------------------------------------------------------------------------------------- strength-filtered smoothed AMG
THETA, THETA_SCALE = 0.08, 0.5


def strength_setup_ref(A, theta=None, thetaScale=None, omegaP=0.0, **kw):
    """amg_sa_ref.setup_ref with the aggregation and the prolongator smoother on F_l = filter(A_l, STRENGTH, theta_l, lump)
    and the Galerkin product on the full A_l.  Levels but the last also hold F, kept (for the refresh), theta and dF"""
    o = ar._opts(kw)
    th = np.float64(THETA if not theta else theta)
    scale = np.float64(THETA_SCALE if not thetaScale else thetaScale)
    levels = []
    while True:
        M = A[0]
        lv = dict(A=A, dinv=ar.dinv_of(A), csr=Csr(M, A[2], A[3], A[4]))
        levels.append(lv)
        if M <= o["coarseRows"] or len(levels) == o["maxLevels"]:
            break
        fo = opts(STRENGTH, theta=th, lump=True)
        F, kept = filter_ref(A, fo)
        agg = ar.aggregate_ref(M, F[2], F[3], o["seed"])
        nAgg = int(agg.max()) + 1
        if nAgg == M:
            break
        level_from(lv, A, F, kept, fo, agg, nAgg, omegaP)
        A = sr.spgemm_ref(lv["R"], lv["AP"])
        th = th * scale
    return levels, o


def level_from(lv, A, F, kept, fo, agg, nAgg, omegaP):
    """everything of a level that follows from A_l, F_l and the aggregates"""
    T = ar.prolongator(A[0], agg, nAgg)
    dF = ar.dinv_of(F)
    rho, g = sa.rho_of(F, dF)
    assert np.all(np.isfinite(g)) and 0.0 < rho < np.inf, "the setup refuses this level"
    w = sa.damping(rho, omegaP)
    P = ad.add_ref(1.0, T, -w, sr.spgemm_ref(sa.diag_handle(dF), sr.spgemm_ref(F, T)))
    R = sr.transpose(P)
    AP = sr.spgemm_ref(A, P)
    lv.update(F=F, kept=kept, fo=fo, theta=np.float64(fo["theta"]), dF=dF, agg=agg, T=T, rho=rho, w=w, P=P, R=R, AP=AP,
              Pcsr=Csr(P[0], P[2], P[3], P[4]), Rcsr=Csr(R[0], R[2], R[3], R[4]))


def strength_refresh_ref(levels, o, A_new, omegaP=0.0):
    """spmvHipAmgRefresh on a strength hierarchy: the kept sets and the aggregates of `levels`, A's new values"""
    out = []
    A = A_new
    for old in levels:
        lv = dict(A=A, dinv=ar.dinv_of(A), csr=Csr(A[0], A[2], A[3], A[4]))
        out.append(lv)
        if "agg" not in old:
            break
        F = filter_refresh_ref(old["kept"], A, old["fo"])
        level_from(lv, A, F, old["kept"], old["fo"], old["agg"], int(old["agg"].max()) + 1, omegaP)
        A = sr.spgemm_ref(lv["R"], lv["AP"])
    return out


class StrengthCsr(Csr):
    """krylov_ref.Csr whose M^-1 v is the cycle of the strength-filtered hierarchy (the cycle is amg_sa_ref's)"""

    def __init__(self, A, theta=None, thetaScale=None, omegaP=0.0, **kw):
        super().__init__(A[0], A[2], A[3], A[4])
        self.levels, self.o = strength_setup_ref(A, theta, thetaScale, omegaP, **kw)
        self.F = self.levels

    def precond(self, v):
        return sa.cycle_ref(self.levels, self.o, np.asarray(v, dtype=np.float64))


# ------------------------------------------------------------------------------------------------------------- inputs
def stencil7(nx, ny, nz, weights=(1.0, 1.0, 1.0)):
    """the 7-point stencil with one weight per axis: -w off the diagonal, 2 (wx + wy + wz) on it; rows ascending"""
    idx = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(idx.size, 2.0 * (weights[0] + weights[1] + weights[2]))]
    for ax in range(3):
        lo = np.take(idx, np.arange(idx.shape[ax] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, idx.shape[ax]), axis=ax).ravel()
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [np.full(lo.size, -float(weights[ax]))] * 2
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    return sr.csr(idx.size, idx.size, rows[order], cols[order], vals[order])


def special_values(rng, n):
    """order-sensitive values seeded with -0.0, +-Inf, a NaN with a payload, denormals and a stored 0.0"""
    v = si.order_values(rng, n)
    special = np.array([0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000ABCDEF, 0x0000000000000001,
                        0x800000000000FFFF, 0x0000000000000000], dtype=np.uint64).view(np.float64)
    if n:
        at = rng.choice(n, size=min(n, 2 * special.size), replace=False)
        v[at] = np.resize(special, at.size)
    return v


def lump_inputs(seed=0):
    """name -> (M, M, IRP, JA, AS): amg_sa_ref.with_one_diagonal on every small graph (the STORED rule holds on each)"""
    return {name: sa.with_one_diagonal(*g, seed=seed) for name, g in ar.small_graphs().items()}
