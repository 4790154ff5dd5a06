"""The test side's reference for the block triangular solve (hipSpTRSMCSR, include/spmvHip.h): `trsv_ref.trsv_levels` with
an (rows, k) accumulator.  Every column goes through the same elementwise operations as the single-vector form -- the
positions of a level's rows walked together in stored order, positions outside the triangle skipped, each product and
each add rounded separately -- so column c of the result has the bits of `trsv_ref.trsv_loop` on column c of B."""
import numpy as np

from trsv_ref import diag_pos, levels


def trsm_levels(M, IRP, JA, AS, B, lower=True, unit=False, lvl=None):
    """X = T^-1 B, B of shape (M, k); the loop of trsv_ref per column, vectorised over the rows of each level"""
    IRP = np.asarray(IRP, dtype=np.int64)
    JA = np.asarray(JA, dtype=np.int64)
    AS = np.asarray(AS, dtype=np.float64)
    X = np.array(B, dtype=np.float64, copy=True, order="C")
    assert X.ndim == 2 and X.shape[0] == M
    if M == 0:
        return X
    if lvl is None:
        lvl = levels(M, IRP, JA, lower)
    if not unit:
        dpos, bad = diag_pos(M, IRP, JA)
        assert bad < 0, f"row {bad} does not hold exactly one diagonal entry"
    order = np.argsort(lvl, kind="stable")
    bounds = np.searchsorted(lvl[order], np.arange(lvl.max() + 2))
    with np.errstate(all="ignore"):
        for l in range(lvl.max() + 1):
            R = order[bounds[l]:bounds[l + 1]]
            s, lens = IRP[R], IRP[R + 1] - IRP[R]
            acc = np.zeros((R.size, X.shape[1]))
            for e in range(int(lens.max()) if R.size else 0):
                live = np.flatnonzero(e < lens)
                p = s[live] + e
                j = JA[p]
                tri = (j < R[live]) if lower else ((j > R[live]) & (j < M))
                live, p, j = live[tri], p[tri], j[tri]
                acc[live] = acc[live] + AS[p][:, None] * X[j]
            r = X[R] - acc
            X[R] = r if unit else r / AS[dpos[R]][:, None]
    return X
