"""Inputs that send hipSpDavidsonCSR through every exit of its loop (the labels of davidson_ref.DAVIDSON_EXITS) and through
every way the loop reaches an exit that the contract tells apart (`how`), shared by tests/test_davidson_abi.py (the labelled
reference takes the claimed exit on every case: no GPU needed) and tests/test_gpu_precond_eigsh.py (the device gives the
reference's bits and counts on every case).

`how`: "step1" at the first step; "pass1" in the first pass, before any restart; "restarts" after at least two restarts;
"cols=nev" with exactly nev columns in the basis; "short" with fewer than nev columns; "mid" maxIter between two restarts,
after one; "restart" maxIter on a step whose basis is full; "exact" beta == 0 from a start vector in an invariant subspace;
"l>0" beta == 0 on a target other than the first pair; "inf" an Inf entry of A; "huge" finite entries of H whose residual
overflows; "dM" an M^-1 whose result overflows; "-" nothing to tell apart.

The small cases are the 5 x 4 five-point Laplacian (n = 20) and diagonal matrices; `dm`, where it is not None, is the diagonal
of a diagonal M handed over as a CSR handle whose triangles are applied (M^-1 v = v / dm, element by element); `2I` is a
unit-value handle of 2^14 rows with v0 = +-4, so that v[0] = +-1/128, H = 2 and R = w - 2 v[0] = 0 are all exact."""
from collections import namedtuple

import numpy as np

from lanczos_exit_inputs import _diag, _e0, _lap, _lap_inf, _two_identity, _v0
from lanczos_ref import LARGEST, SMALLEST

Case = namedtuple("Case", "name label how M IRP JA AS v0 nev ncv which tol maxiter keep dm status found restarts")
CONVERGED, MAXITER, BREAKDOWN, NONFINITE = 0, 1, 2, 3

# the exits for which the table has no input, with the reason; tests/test_davidson_abi.py checks that it has no other hole
HOLES = {
    "jacobi_nonfinite": "unreachable: every entry of H is a dot product of a unit vector with a product A v that the step before "
                        "found finite, and Jacobi's rotations do not grow a finite matrix past the largest double (as for "
                        "hipSpLanczosCSR); the return guards the host loop against an H that is not what the loop makes",
}
# (label, how) that the table must hold
REQUIRED = (("v0_zero", "-"), ("v0_nonfinite", "-"), ("init_maxiter", "-"), ("h_nonfinite", "inf"), ("res_nonfinite", "huge"),
            ("beta_nonfinite", "dM"), ("converged", "step1"), ("converged", "pass1"), ("converged", "restarts"),
            ("converged", "cols=nev"), ("maxiter", "short"), ("maxiter", "mid"), ("maxiter", "restart"), ("breakdown", "exact"),
            ("breakdown", "l>0"))

_D8 = [3, 1, 4, 1, 5, 9, 2, 6]
_D8U = [3, 1, 4, 7, 5, 9, 2, 6]                         # (no repeated eigenvalue)


def _huge():
    return _diag([1e200, 1, 2, 3, 4, 5, 6, 7])


# name: (label, how, matrix, v0, nev, ncv, which, tol, maxiter, keep, dm, status, found, restarts)
_ROWS = {
    "v0_zero": ("v0_zero", "-", _lap, lambda n: np.zeros(n), 2, 6, LARGEST, 1e-8, 100, 0, None, BREAKDOWN, 0, 0),
    "v0_nan": ("v0_nonfinite", "-", _lap, lambda n: np.where(np.arange(n) == 3, np.nan, 1.0), 2, 6, LARGEST, 1e-8, 100, 0, None, NONFINITE, 0, 0),
    "v0_inf": ("v0_nonfinite", "-", _lap, lambda n: np.where(np.arange(n) == 19, np.inf, 1.0), 2, 6, SMALLEST, 1e-8, 100, 0, None, NONFINITE, 0, 0),
    "maxiter0": ("init_maxiter", "-", _lap, _v0, 2, 6, LARGEST, 1e-8, 0, 0, None, MAXITER, 0, 0),
    "inf_entry": ("h_nonfinite", "inf", _lap_inf, _v0, 2, 6, LARGEST, 1e-8, 100, 0, None, NONFINITE, 0, 0),
    # H = v^T A v is about 1e200 / 8, finite; the residual's squares overflow
    "huge_entry": ("res_nonfinite", "huge", _huge, lambda n: np.ones(n), 1, 4, LARGEST, 1e-8, 100, 0, None, NONFINITE, 0, 0),
    # M = 1e-200 I: t = 1e200 r, and dot(t, t) overflows
    "tiny_dm": ("beta_nonfinite", "dM", lambda: _diag(_D8), _v0, 2, 4, SMALLEST, 1e-8, 100, 0, [1e-200] * 8, NONFINITE, 0, 0),
    "diag_e0_nev1": ("converged", "step1", lambda: _diag(_D8), _e0, 1, 4, LARGEST, 1e-8, 100, 0, None, CONVERGED, 1, 0),
    "diag_e0_nev2": ("breakdown", "exact", lambda: _diag(_D8), _e0, 2, 4, SMALLEST, 1e-8, 100, 0, None, BREAKDOWN, 1, 0),
    # two eigenvalues, 0 and 2, eight rows each, v0 = 1: the second step holds both pairs exactly
    "diag02_nev2": ("converged", "cols=nev", lambda: _diag([0, 2] * 8), lambda n: np.ones(n), 2, 6, LARGEST, 1e-8, 100, 0, None, CONVERGED, 2, 0),
    "diag02_nev3": ("breakdown", "l>0", lambda: _diag([0, 2] * 8), lambda n: np.ones(n), 3, 6, LARGEST, 1e-8, 100, 0, None, BREAKDOWN, 2, 0),
    "maxiter_short": ("maxiter", "short", _lap, _v0, 3, 7, SMALLEST, 1e-8, 2, 0, None, MAXITER, 2, 0),
    "maxiter_mid": ("maxiter", "mid", _lap, _v0, 2, 6, LARGEST, 1e-8, 9, 0, None, MAXITER, 2, 2),
    "maxiter_restart_first": ("maxiter", "restart", _lap, _v0, 2, 6, LARGEST, 1e-8, 6, 0, None, MAXITER, 2, 0),
    "maxiter_restart_third": ("maxiter", "restart", _lap, _v0, 2, 6, SMALLEST, 1e-8, 10, 0, None, MAXITER, 2, 2),
    "converged_first": ("converged", "pass1", _lap, _v0, 2, 19, LARGEST, 1e-8, 100, 0, None, CONVERGED, 2, 0),
    "converged_la": ("converged", "restarts", _lap, _v0, 2, 6, LARGEST, 1e-8, 400, 0, None, CONVERGED, 2, 12),
    "converged_sa": ("converged", "restarts", _lap, _v0, 3, 7, SMALLEST, 1e-8, 400, 0, None, CONVERGED, 3, 11),
    "converged_keep_nev": ("converged", "restarts", _lap, _v0, 2, 6, SMALLEST, 1e-8, 400, 2, None, CONVERGED, 2, None),
    "converged_keep_m1": ("converged", "restarts", _lap, _v0, 2, 6, LARGEST, 1e-8, 400, 5, None, CONVERGED, 2, None),
    "smallest_basis": ("converged", "restarts", _lap, _v0, 1, 2, LARGEST, 1e-8, 2000, 0, None, CONVERGED, 1, None),
    # M = A: the exact inverse of a diagonal matrix, applied through the two triangular solves
    "diag_exact_dm": ("converged", "restarts", lambda: _diag(_D8U), _v0, 2, 4, SMALLEST, 1e-8, 100, 0, _D8U, CONVERGED, 2, None),
    # M = 6 I on the Laplacian: the Jacobi preconditioner, which scales every residual alike
    "lap_jacobi_dm": ("converged", "restarts", _lap, _v0, 2, 6, SMALLEST, 1e-8, 400, 0, [6.0] * 20, CONVERGED, 2, None),
}
NAMES = tuple(_ROWS) + ("2I",)
SMALL = tuple(_ROWS)                                    # the cases small enough for the loop in plain Python


def case(name):
    """one case of the table, built on demand"""
    if name == "2I":
        (M, IRP, JA, AS), v0 = _two_identity()
        return Case(name, "converged", "step1", M, IRP, JA, AS, v0, 1, 8, LARGEST, 1e-8, 100, 0, None, CONVERGED, 1, 0)
    label, how, mat, v0, nev, ncv, which, tol, maxiter, keep, dm, status, found, restarts = _ROWS[name]
    M, IRP, JA, AS = mat()
    return Case(name, label, how, M, IRP, JA, AS, np.asarray(v0(M), dtype=np.float64), nev, ncv, which, tol, maxiter, keep,
                None if dm is None else np.asarray(dm, dtype=np.float64), status, found, restarts)


def precond_of(c):
    """the case's M^-1 as davidson_ref takes it"""
    if c.dm is None:
        return None
    return lambda v: v / c.dm
