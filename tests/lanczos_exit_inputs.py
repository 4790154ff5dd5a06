"""Inputs that send hipSpLanczosCSR through every exit of its loop (the labels of lanczos_ref.LANCZOS_EXITS) and through
every way the loop reaches an exit that the contract tells apart (`how`), shared by tests/test_lanczos_abi.py (the labelled
reference takes the claimed exit on every case: no GPU needed) and tests/test_gpu_lanczos.py (the device gives the
reference's bits on every case).

`how`: "j0" beta == 0 at the first step; "exact" beta == 0 with fewer than nev columns; "mid" maxIter inside a cycle;
"end" maxIter at a cycle's last step; "first" in the first cycle; "restarts" after at least two restarts; "inf" an Inf entry
of A; "-" nothing to tell apart.

The small cases are the 5 x 4 five-point Laplacian (n = 20) and diagonal matrices; `2I` is a unit-value handle of 2^14 rows
with v0 = +-4, so that v[0] = +-1/128, dot(v[0], v[0]) = 1 and w - 2 v[0] = 0 are all exact."""
from collections import namedtuple

import numpy as np

from lanczos_ref import LARGEST, SMALLEST
from test_trsv_abi import laplacian7

Case = namedtuple("Case", "name label how M IRP JA AS v0 nev ncv which tol maxiter keep status found cycles")
CONVERGED, MAXITER, BREAKDOWN, NONFINITE = 0, 1, 2, 3

# the exits for which the table has no input, with the reason; tests/test_lanczos_abi.py checks that it has no other hole
HOLES = {
    "jacobi_nonfinite": "unreachable: a finite beta = sqrt(dot(w,w)) bounds every entry of w, hence alpha and every entry of T, by "
                        "about 1.4e154, and Jacobi's rotations do not grow a matrix of that size past the largest double; the "
                        "return guards the host loop against a T that is not what the loop makes",
}
# (label, how) that the table must hold
REQUIRED = (("v0_zero", "-"), ("v0_nonfinite", "-"), ("init_maxiter", "-"), ("step_nonfinite", "inf"), ("converged", "j0"),
            ("breakdown", "exact"), ("maxiter", "mid"), ("maxiter", "end"), ("converged", "first"), ("converged", "restarts"))


def _lap():
    IRP, JA, AS = laplacian7(5, 4, 1)
    return 20, IRP, JA, AS


def _diag(d):
    n = len(d)
    return n, np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint64), np.array(d, dtype=np.float64)


def _v0(n, seed=1):
    return np.random.default_rng(seed).standard_normal(n)


def _e0(n):
    v = np.zeros(n)
    v[0] = 3.0
    return v


def _lap_inf():
    M, IRP, JA, AS = _lap()
    AS = AS.copy()
    AS[np.flatnonzero(AS > 0)[7]] = np.inf
    return M, IRP, JA, AS


def _two_identity(n=16_384):
    i = np.arange(n, dtype=np.uint64)
    v0 = 4.0 * np.where(np.random.default_rng(5101).integers(0, 2, n) > 0, 1.0, -1.0)
    return (n, np.arange(n + 1, dtype=np.uint64), i, np.full(n, 2.0)), v0


# name: (label, how, matrix, v0, nev, ncv, which, tol, maxiter, keep, status, found, cycles)
_ROWS = {
    "v0_zero": ("v0_zero", "-", _lap, lambda n: np.zeros(n), 2, 6, LARGEST, 1e-8, 100, 0, BREAKDOWN, 0, 0),
    "v0_nan": ("v0_nonfinite", "-", _lap, lambda n: np.where(np.arange(n) == 3, np.nan, 1.0), 2, 6, LARGEST, 1e-8, 100, 0, NONFINITE, 0, 0),
    "v0_inf": ("v0_nonfinite", "-", _lap, lambda n: np.where(np.arange(n) == 19, np.inf, 1.0), 2, 6, SMALLEST, 1e-8, 100, 0, NONFINITE, 0, 0),
    "maxiter0": ("init_maxiter", "-", _lap, _v0, 2, 6, LARGEST, 1e-8, 0, 0, MAXITER, 0, 0),
    "inf_entry": ("step_nonfinite", "inf", _lap_inf, _v0, 2, 6, LARGEST, 1e-8, 100, 0, NONFINITE, 0, 1),
    "diag_e0_nev1": ("converged", "j0", lambda: _diag([3, 1, 4, 1, 5, 9, 2, 6]), _e0, 1, 4, LARGEST, 1e-8, 100, 0, CONVERGED, 1, 1),
    "diag_e0_nev2": ("breakdown", "exact", lambda: _diag([3, 1, 4, 1, 5, 9, 2, 6]), _e0, 2, 4, SMALLEST, 1e-8, 100, 0, BREAKDOWN, 1, 1),
    # two eigenvalues, 0 and 2, eight rows each, v0 = 1: every step is exact, and beta == 0 at j = 1 with cols = nev
    "diag02_exact": ("converged", "first", lambda: _diag([0, 2] * 8), lambda n: np.ones(n), 2, 6, LARGEST, 1e-8, 100, 0, CONVERGED, 2, 1),
    "maxiter_mid": ("maxiter", "mid", _lap, _v0, 2, 6, LARGEST, 1e-8, 9, 0, MAXITER, 2, 3),
    "maxiter_first_mid": ("maxiter", "mid", _lap, _v0, 3, 7, SMALLEST, 1e-8, 2, 0, MAXITER, 2, 1),
    "maxiter_end_first": ("maxiter", "end", _lap, _v0, 2, 6, LARGEST, 1e-8, 6, 0, MAXITER, 2, 1),
    "maxiter_end_second": ("maxiter", "end", _lap, _v0, 2, 6, SMALLEST, 1e-8, 8, 0, MAXITER, 2, 2),
    "converged_first": ("converged", "first", _lap, _v0, 2, 19, LARGEST, 1e-8, 100, 0, CONVERGED, 2, 1),
    "converged_la": ("converged", "restarts", _lap, _v0, 2, 6, LARGEST, 1e-8, 200, 0, CONVERGED, 2, 13),
    "converged_sa": ("converged", "restarts", _lap, _v0, 3, 7, SMALLEST, 1e-8, 200, 0, CONVERGED, 3, 12),
    "converged_keep_nev": ("converged", "restarts", _lap, _v0, 2, 6, SMALLEST, 1e-8, 400, 2, CONVERGED, 2, None),
    "converged_keep_m1": ("converged", "restarts", _lap, _v0, 2, 6, LARGEST, 1e-8, 400, 5, CONVERGED, 2, None),
    "smallest_basis": ("converged", "restarts", _lap, _v0, 1, 2, LARGEST, 1e-8, 400, 0, CONVERGED, 1, 73),
}
NAMES = tuple(_ROWS) + ("2I",)
SMALL = tuple(_ROWS)                                    # the cases small enough for the loop in plain Python


def case(name):
    """one case of the table, built on demand"""
    if name == "2I":
        (M, IRP, JA, AS), v0 = _two_identity()
        return Case(name, "converged", "j0", M, IRP, JA, AS, v0, 1, 8, LARGEST, 1e-8, 100, 0, CONVERGED, 1, 1)
    label, how, mat, v0, nev, ncv, which, tol, maxiter, keep, status, found, cycles = _ROWS[name]
    M, IRP, JA, AS = mat()
    return Case(name, label, how, M, IRP, JA, AS, np.asarray(v0(M), dtype=np.float64), nev, ncv, which, tol, maxiter, keep, status,
                found, cycles)
