"""Inputs that send hipSpGMRESCSR through every exit of its loop (the labels of gmres_ref.GMRES_EXITS) and through every
way a cycle can end (gmres_ref.CYCLE_ENDS and the dropped step "d0"), with and without ILU(0), shared by
tests/test_gmres_abi.py (the labelled reference takes the claimed exit on every case: no GPU needed) and
tests/test_gpu_gmres.py (the device gives the reference's bits on every case).

The small cases are integer matrices of order 2 to 4 with entries in -2 .. 2, found by a random search with the labelled
reference, as those of krylov_exit_inputs.py were.  `ends` is what ended the LAST cycle: every condition that held at
that step, joined by "+" ("est" the estimate at or under thresh, "estnf" the estimate not finite, "hn0", "restart"
j == restart-1, "maxiter" k == maxIter), or "d0" for the dropped step.  hn == 0 makes sn = 0 and so est = 0: it never
comes without "est"; with tol = 0 the true residual may still be a rounding error above thresh = 0, and that is the
BREAKDOWN of a lucky breakdown that did not converge.  `early` cases stop at iteration <= 1, `late` ones at >= 2;
`cycles` > 1 says that an earlier cycle ended and the loop went on.

A `large` twin is kron(I_c, A) with b tiled, c = 4^p with c * nnz(A) >= 2^18 (so sqrt(c) = 2^p: beta, every h and every
quotient is the small case's times a power of two, exactly), x0 a nonzero integer vector and b shifted by A x0."""
from collections import namedtuple

import numpy as np

from krylov_exit_inputs import dense_csr, kron_identity
from serial_order_inputs import AUTO_MIN_NNZ
from test_trsv_abi import laplacian7

Case = namedtuple("Case", "name label ends when cycles precond M IRP JA AS b x0 tol maxiter restart")
NAN = float("nan")

# (label, ends of the last cycle, when, cycles, preconditioned, A, b, tol, maxiter, restart, with a large twin)
_SMALL = [
    # ---- no preconditioner
    ("init_converged", "", "early", 0, False, [[-1, 0], [0, 1]], [0, 0], 1e-8, 6, 3, False),
    ("init_nonfinite", "", "early", 0, False, [[NAN, 0], [0, 1]], [1, 1], 1e-8, 6, 3, False),
    ("init_maxiter", "", "early", 0, False, [[2, -1], [0, 2]], [1, 2], 1e-8, 0, 3, True),
    ("d0_cols0", "d0", "early", 1, False, [[2, 0], [-1, 0]], [0, -1], 0.0, 6, 3, True),
    ("d0_cols0", "d0", "early", 2, False, [[-2, -2, -2], [0, 0, 0], [0, -1, -1]], [-1, -1, 1], 1e-8, 2, 1, False),
    ("d0_cols0", "d0", "late", 3, False, [[-2, -2], [-2, -2]], [-2, 0], 0.0, 6, 1, False),
    ("breakdown", "d0", "early", 1, False, [[2, -2], [2, -2]], [1, -1], 1e-8, 3, 3, True),
    ("breakdown", "d0", "late", 1, False, [[0, 2], [0, 0]], [-2, 1], 1e-8, 3, 3, False),
    ("breakdown", "d0", "late", 2, False, [[-2, -2, -2], [-1, -1, -1], [0, 1, -1]], [0, 1, -2], 1e-8, 6, 64, False),
    ("breakdown", "est+hn0", "late", 1, False, [[-1, 2], [0, -2]], [0, -2], 0.0, 3, 64, False),
    ("breakdown", "est+hn0", "late", 2, False, [[-1, -2], [-1, 1]], [-2, 2], 0.0, 6, 3, False),
    ("converged", "d0", "late", 1, False, [[-1, -2, 1], [0, 1, -1], [-2, -2, 2]], [2, 0, 2], 0.0, 3, 3, False),
    ("converged", "est", "early", 1, False, [[2, -1], [1, 0]], [2, 2], 1e-8, 6, 3, True),
    ("converged", "est", "late", 1, False, [[2, 2, 0, 2], [2, -1, -2, 2], [0, 0, 2, 2], [2, -2, -2, 0]], [0, -1, -1, 0], 1e-8, 6, 64, False),
    ("converged", "est", "late", 2, False, [[-2, 2, 0], [0, -1, 0], [-2, 0, -2]], [-2, -2, 2], 1e-8, 6, 2, True),
    ("converged", "est+hn0", "early", 1, False, [[1, -1], [0, -1]], [-1, -2], 1e-8, 6, 2, True),
    ("converged", "est+hn0", "late", 1, False, [[0, 1], [1, -1]], [-2, 0], 0.0, 6, 3, False),       # hn == 0 at j = n-1
    ("converged", "est+restart", "late", 2, False, [[-2, -2], [0, -2]], [-1, 1], 1e-8, 6, 1, False),  # restart = 1
    ("converged", "restart", "late", 2, False, [[0, -2], [-1, -1]], [1, 1], 0.0, 6, 2, False),       # on the true rr alone
    ("converged", "maxiter", "late", 1, False, [[1, 0], [0, -1]], [-1, 1], 0.0, 6, 64, False),
    ("maxiter", "maxiter", "early", 1, False, [[0, -1, -2, 0], [-2, 1, 2, -1], [0, -2, -2, -1], [2, 2, 1, 0]], [0, -2, -1, 2], 1e-8, 1, 2, True),
    ("maxiter", "maxiter", "late", 1, False, [[0, -2, 1], [2, 1, -2], [0, -1, 2]], [2, -2, 0], 0.0, 6, 64, False),   # restart > n
    ("maxiter", "maxiter", "late", 2, False, [[-2, 1, -2], [-2, 0, -1], [0, 2, 2]], [0, 1, 2], 1e-8, 3, 2, True),    # mid-cycle
    ("maxiter", "restart+maxiter", "late", 2, False, [[0, -2, 0, 0], [2, 1, -1, -2], [0, -1, 1, 2], [-1, 2, 0, 0]], [1, 1, 2, 2], 0.0, 2, 1, False),
    ("maxiter", "restart+maxiter", "late", 1, False, [[1, 1, 2, 0], [1, 2, -1, -2], [-1, -1, 2, 2], [-2, 0, 2, -2]], [1, -2, 0, 2], 1e-8, 2, 2, True),
    ("maxiter", "est+maxiter", "late", 2, False, [[1, 2, -2], [-1, -2, 2], [1, -1, -1]], [-2, 0, 1], 1e-8, 6, 64, False),  # est cycles, true rr above
    ("nonfinite", "estnf", "early", 1, False, [[1.5e308, 1.5e308], [-1.5e308, -1.5e308]], [1, 1], 1e-8, 6, 3, False),  # w = (Inf, -Inf): h is NaN
    # ---- with ILU(0)
    ("init_converged", "", "early", 0, True, [[-1, 0], [0, -1]], [0, 0], 1e-8, 6, 3, False),
    ("init_nonfinite", "", "early", 0, True, [[-1, 0], [0, -1]], [NAN, 1], 1e-8, 6, 3, False),
    ("init_maxiter", "", "early", 0, True, [[-1, 0], [0, -1]], [-2, -2], 1e-8, 0, 3, False),
    ("d0_cols0", "d0", "early", 1, True, [[1, 1, 2], [-2, -1, -2], [-2, 0, 0]], [0, 0, -1], 1e-8, 6, 1, True),
    ("d0_cols0", "d0", "late", 2, True, [[2, -1, 1], [1, 0, 0], [0, -1, 1]], [-1, 1, 0], 1e-8, 6, 3, False),
    ("breakdown", "d0", "early", 1, True, [[1, 2, 1], [2, 0, 1], [-2, 0, -1]], [1, 1, 0], 1e-8, 6, 2, True),
    ("breakdown", "est+hn0", "early", 1, True, [[-1, -2, 2], [1, 1, -2], [1, -2, 2]], [0, -2, 1], 0.0, 3, 64, False),
    ("breakdown", "est+hn0", "late", 2, True, [[1, 2, -2], [0, -1, -2], [2, 1, -1]], [-1, -1, 1], 0.0, 6, 3, False),
    ("converged", "est", "early", 1, True, [[1, -1, -2, 2], [-1, 2, -1, -1], [1, -2, -2, 1], [2, 2, -2, -2]], [-1, 1, 2, 2], 1e-8, 6, 2, False),
    ("converged", "est", "late", 1, True, [[-2, 1, 0], [-2, -1, 0], [1, 0, 1]], [2, 1, -1], 1e-8, 3, 3, True),
    ("converged", "est+hn0", "early", 1, True, [[1, 0], [-2, 2]], [2, 0], 0.0, 3, 64, True),
    ("converged", "est+hn0", "late", 2, True, [[-1, -2], [-2, 2]], [-1, 2], 0.0, 6, 2, False),
    ("converged", "est+restart", "late", 2, True, [[2, 0, -2, -1], [2, -2, 0, -1], [0, -2, -1, -2], [1, -1, -2, 1]], [-2, -2, -1, -2], 1e-8, 6, 1, False),
    ("converged", "restart", "late", 2, True, [[-1, -1], [0, 2]], [-2, 2], 0.0, 6, 2, False),
    ("maxiter", "maxiter", "late", 1, True, [[1, 2, 2], [2, 1, -1], [0, 1, -2]], [1, -2, -1], 0.0, 2, 64, False),
    ("maxiter", "maxiter", "late", 2, True, [[2, 2, -2, 1], [0, -2, 2, 2], [2, 1, -2, 1], [0, 1, 0, 2]], [0, -1, 1, 1], 0.0, 3, 2, False),
    ("maxiter", "restart+maxiter", "late", 2, True, [[1, 0, 0], [1, -2, 2], [-1, 0, 2]], [1, 1, 2], 0.0, 2, 1, False),
    ("maxiter", "est+maxiter", "late", 2, True, [[1, -2, 2], [2, 2, 1], [1, 0, 1]], [-2, 0, 2], 1e-8, 6, 64, False),
    ("nonfinite", "estnf", "early", 1, True, [[0, 1, -2, 1], [0, 2, 1, 2], [1, 2, -2, 1], [1, -1, -1, 1]], [-2, -2, 2, 1], 1e-8, 3, 2, False),  # a zero pivot
    ("nonfinite", "estnf+restart", "early", 1, True, [[2, 2], [-1, -1]], [1, 0], 0.0, 3, 1, False),
]

# (label, a condition in the last cycle's ends) that the table must hold without and with ILU(0)
REQUIRED = (("converged", "est"), ("converged", "restart"), ("converged", "hn0"), ("breakdown", "hn0"), ("breakdown", "d0"),
            ("maxiter", "maxiter"), ("maxiter", "restart"), ("nonfinite", "estnf"))
# labels that must come `early` and `late`
BOTH_WHENS = ("converged", "breakdown")
# (preconditioned, label, condition or when) for which the table has no input, with the reason; tests/test_gmres_abi.py
# checks that it has no other hole
HOLES = {}


def _small_name(i, row, large):
    label, ends, when, cycles, pre = row[:5]
    return f"gmres{'+ilu0' if pre else ''}:{label}:{ends or '-'}:{when}:c{cycles}:n{len(row[5])}:m{row[9]}:#{i}" + (":large" if large else "")


def _small(i, row, large):
    label, ends, when, cycles, pre, A, b, tol, maxiter, restart, _ = row
    M, IRP, JA, AS = dense_csr(A, pre)
    b, x0 = np.array(b, np.float64), np.zeros(M)
    if large:
        c = 1
        while c * JA.size < AUTO_MIN_NNZ:
            c *= 4
        x0 = np.arange(1, M + 1, dtype=np.float64) * (-1.0) ** np.arange(M)
        b = b + np.array(A, np.float64) @ x0                            # small integers: exact
        M, IRP, JA, AS = kron_identity(c, M, IRP, JA, AS)
        b, x0 = np.tile(b, c), np.tile(x0, c)
    return Case(_small_name(i, row, large), label, ends, when, cycles, pre, M, IRP, JA, AS, b, x0, tol, maxiter, restart)


def _overflow():
    """krylov_exit_inputs' 8^3 Laplacian with one diagonal value 1e308 (CG and BiCGStab end NONFINITE on it): the init
    residual is finite, the first A v overflows to one Inf, so h[0] and d are Inf and the estimate is not finite: the
    cycle ends after its first step, and what it adds to x leaves the true residual where it was.  Under this loop the
    solve stagnates: 50 cycles of one step, then MAXITER."""
    IRP, JA, AS = laplacian7(8, 8, 8)
    AS = AS.copy()
    AS[np.flatnonzero(AS > 0)[100]] = 1e308
    b = 100.0 * (1.0 + np.random.default_rng(5100).random(512))
    return Case("gmres:maxiter:estnf+maxiter:late:c50:laplacian", "maxiter", "estnf+maxiter", "late", 50, False, 512, IRP, JA, AS, b, np.zeros(512),
                1e-8, 50, 30)


def _two_identity(n=16_384):
    """A = 2 I (a unit handle): w = 2 v[0], h = 2, hn == 0 at j = 0 for any b with an exact v[0]: b = +-4 in 2^14 entries,
    beta = 2^9"""
    i = np.arange(n, dtype=np.uint64)
    b = 4.0 * np.where(np.random.default_rng(5101).integers(0, 2, n) > 0, 1.0, -1.0)
    return Case("gmres:converged:est+hn0:early:2I", "converged", "est+hn0", "early", 1, False, n,
                np.arange(n + 1, dtype=np.uint64), i, np.full(n, 2.0), b, np.zeros(n), 1e-8, 6, 30)


def _build():
    out = {}
    for i, row in enumerate(_SMALL):
        for large in (False, True)[:1 + row[-1]]:
            out[_small_name(i, row, large)] = lambda i=i, row=row, large=large: _small(i, row, large)
    out["gmres:maxiter:estnf+maxiter:late:c50:laplacian"] = _overflow
    out["gmres:converged:est+hn0:early:2I"] = _two_identity
    return out


_BUILDERS = _build()
NAMES = tuple(_BUILDERS)


def case(name):
    """one case of the table, built on demand"""
    c = _BUILDERS[name]()
    assert c.name == name
    return c
