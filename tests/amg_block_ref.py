"""The test side's reference of the multigrid cycle for a block of vectors (spmvHipAmgApplyBlock) and of a hierarchy as dM of
the block solvers (include/spmvHip.h): column by column the cycle of tests/amg_cheb_ref.py (which takes the levels of all
three setups and both smoothers) and, for the solves, block_krylov_ref.block_ref on amg_cheb_ref.ChebCsr.  No new
arithmetic: a block cycle is k single cycles, and that is all this file says.  It also holds the test blocks."""
import numpy as np

import amg_cheb_ref as cr
from block_krylov_ref import block_ref

HIERARCHIES = ("plain", "smoothed", "strength")
# (kind, nu1, nu2, nuCoarse) of the cycle tests
SMOOTHERS = {"jacobi118": (cr.JACOBI, 1, 1, 8), "jacobi223": (cr.JACOBI, 2, 2, 3), "cheb222": (cr.CHEBYSHEV, 2, 2, 2), "cheb314": (cr.CHEBYSHEV, 3, 1, 4)}


def smoother_of(o, name):
    kind, nu1, nu2, nuCoarse = SMOOTHERS[name]
    return cr.smoother(o, kind=kind, nu1=nu1, nu2=nu2, nuCoarse=nuCoarse)


def block_cycle_ref(levels, o, R, sm):
    """Z[:, c] = V(0, R[:, c])"""
    R = np.asarray(R, dtype=np.float64)
    tabs = cr.tables(levels, sm) if sm["kind"] == cr.CHEBYSHEV else None
    if R.shape[1] == 0:
        return np.zeros_like(R)
    return np.stack([cr.cycle_ref(levels, o, np.ascontiguousarray(R[:, c]), sm, tabs=tabs) for c in range(R.shape[1])], axis=1)


def block_solve_ref(solver, A, B, X0, tol, maxiter):
    """block_krylov_ref.block_ref with A a ChebCsr: (columns, (status, iterations, rr, bb))"""
    return block_ref(solver, A, B, X0, tol, maxiter)


def restrictions(levels, o, r, sm):
    """[r_0, r_1, ...]: the right-hand side of every level on the way down, from the reference's own functions: the
    pre-smoothed z of level l is the cycle of the one-level hierarchy [level l] with nuCoarse = nu1"""
    out = [np.asarray(r, dtype=np.float64)]
    for l in range(len(levels) - 1):
        lv = levels[l]
        one = dict(sm, nuCoarse=sm["nu1"])
        z = cr.cycle_ref([lv], o, out[-1], one)
        with np.errstate(all="ignore"):
            out.append(lv["Rcsr"].spmv(out[-1] - lv["csr"].spmv(z)))
    return out


def assert_columns_differ_on_every_level(levels, o, R, sm):
    """no two columns of R have the same bits in any row of any level's right-hand side: a column written to the place of
    another changes bits wherever it lands"""
    per = [restrictions(levels, o, R[:, c], sm) for c in range(R.shape[1])]
    for l in range(len(levels)):
        cols = np.stack([p[l] for p in per], axis=1).view(np.uint64)
        for c in range(cols.shape[1]):
            for e in range(c + 1, cols.shape[1]):
                assert not np.any(cols[:, c] == cols[:, e]), (l, c, e)


def ordinary_block(M, k, seed=31):
    """k columns of standard normals (the first min(k, k') columns of two blocks of one seed are the same)"""
    return np.ascontiguousarray(np.random.default_rng(seed).standard_normal((M, 40))[:, :k])


SPECIAL = {1: "zero", 3: "negzero", 4: "nan", 6: "inf"}          # column -> what it holds, between ordinary columns


def special_block(M, seed=32):
    """8 columns: ordinary ones at 0, 2, 5, 7; an all-zero column, one with -0.0 entries, one with a NaN, one with +Inf,
    -Inf and 1e308"""
    R = ordinary_block(M, 8, seed)
    R[:, 1] = 0.0
    R[::3, 3] = -0.0
    R[M // 2, 4] = np.nan
    R[M // 3, 6], R[M // 3 + 1, 6], R[M - 2, 6] = np.inf, -np.inf, 1e308
    return R


def tamed(R, seed=33):
    """the special block with its special columns replaced by ordinary ones"""
    out = R.copy()
    fill = ordinary_block(R.shape[0], 8, seed)
    for c in SPECIAL:
        out[:, c] = fill[:, c]
    return out
