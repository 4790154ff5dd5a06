"""The test side's reference for spmvHipBlockDot, hipSpCGBlockCSR and hipSpBiCGStabBlockCSR (include/spmvHip.h): column by
column the references of tests/krylov_ref.py (`dot_ref`, `cg_ref`, `bicgstab_ref`).  No new arithmetic: a block solve is k
single solves, and that is all this file says."""
from collections import namedtuple

import numpy as np

from krylov_ref import CONVERGED, bicgstab_ref, cg_ref, dot_ref

Column = namedtuple("Column", "x status iterations history rr bb label half")


def block_dot_ref(U, V):
    """h[c] = dot_ref(U[:, c], V[:, c])"""
    return np.array([dot_ref(U[:, c], V[:, c]) for c in range(U.shape[1])], dtype=np.float64)


def column_ref(solver, A, b, x0, tol, maxiter):
    """one column: the single loop on (A, b, x0), with the label of its exit and, at a half-step exit, its half record"""
    trace, half = [], {}
    kw = {"half": half} if solver == "bicgstab" else {}
    x, status, it, hist, rr = (cg_ref if solver == "cg" else bicgstab_ref)(A, b, x0, tol, maxiter, trace=trace, **kw)
    assert len(trace) == 1
    return Column(x, status, it, hist, rr, dot_ref(b, b), trace[0], half)


def block_ref(solver, A, B, X0, tol, maxiter):
    """the k columns of a block solve (a list of Column) and the block's info (status, iterations, rr, bb): the largest
    status, the largest count, rr and bb of the lowest-numbered column with that status"""
    cols = [column_ref(solver, A, B[:, c], X0[:, c], tol, maxiter) for c in range(B.shape[1])]
    status = max(c.status for c in cols)
    lead = next(c for c in cols if c.status == status)
    return cols, (status, max(c.iterations for c in cols), lead.rr, lead.bb)


def block_x(cols):
    return np.stack([c.x for c in cols], axis=1)


def one_more_iteration(solver, A, b, x0, tol, maxiter, col):
    """the planted fault: a column that stopped CONVERGED at iteration j < maxiter and goes on being updated for one more
    iteration.  With tol = 0 the loop's arithmetic up to j is the column's (tol enters only the stop test), so a run capped
    at j + 1 iterations gives the x that the faulty block would hold.  Returns that x, or None where the column gives the
    fault no room (another status, j == maxiter, or the loop ends at j by another exit too)."""
    if col.status != CONVERGED or col.iterations >= maxiter:
        return None
    again = column_ref(solver, A, b, x0, 0.0, col.iterations + 1)
    return again.x if again.iterations == col.iterations + 1 else None
