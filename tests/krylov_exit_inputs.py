"""Inputs that send hipSpCGCSR / hipSpBiCGStabCSR through every exit of their loops (the labels of krylov_ref.CG_EXITS and
BICGSTAB_EXITS), with and without ILU(0), shared by tests/test_krylov_abi.py (the labelled reference takes the claimed
exit on every case: no GPU needed) and tests/test_gpu_krylov.py (the device gives the reference's bits on every case).

The small cases are integer matrices of order 2 to 4 with entries in -2 .. 2, found by an exhaustive search over the 2 x 2
ones and a random one over the others with the labelled reference: the first iteration's dot products are exact on them,
so `== 0` is met exactly.  `early` cases stop at iteration <= 1, `late` ones at iteration >= 2: a whole iteration has run,
beta and omega are live, and a batch of K = 16 iterations is enqueued far past the stop.  Only the nonzero entries are
stored, except on the diagonal of a preconditioned case; rows may be empty without a preconditioner.

A `large` twin of a case is kron(I_c, A) with b tiled, c a power of two with c * nnz(A) >= 2^18 (the kernel selection and
the private formats are in play, n spans many blocks of 4 096): every dot is c times the small one's, exactly, so the
quotients and the exit are the small case's.  Its x0 is a nonzero integer vector and b is shifted by A x0 (exact), which
leaves r0, and so the exit, alone.  tests/test_krylov_abi.py asserts the label of every twin too."""
from collections import namedtuple

import numpy as np

from serial_order_inputs import AUTO_MIN_NNZ
from test_trsv_abi import laplacian7

Case = namedtuple("Case", "name solver label when precond M IRP JA AS b x0 tol maxiter")
NAN = float("nan")

# (solver, label, when, preconditioned, A, b, maxiter, with a large twin); tol = 1e-8, x0 = 0
_SMALL = [
    # ---- CG, no preconditioner (symmetric, definite or not: the loop is the contract)
    ("cg", "init_converged", "early", False, [[-1, 0], [0, 1]], [0, 0], 6, False),
    ("cg", "init_nonfinite", "early", False, [[NAN, 0], [0, 1]], [1, 1], 6, False),
    ("cg", "init_maxiter", "early", False, [[2, -1], [-1, 2]], [1, 2], 0, True),
    ("cg", "pq0", "early", False, [[1, 0], [0, -1]], [1, 1], 6, True),
    ("cg", "pq0", "late", False, [[-1, 0, 0], [0, -1, 0], [0, 0, 0]], [-2, 1, 2], 6, True),
    ("cg", "converged", "early", False, [[-2, -2], [-2, -2]], [-1, -1], 6, True),
    ("cg", "converged", "late", False, [[-1, 0], [0, 1]], [-2, -1], 6, True),
    ("cg", "nonfinite", "late", False, [[-2.0 ** 400, 0], [0, 2]], [-2.0 ** 101, 2.0 ** 300], 6, False),
    ("cg", "maxiter", "early", False, [[-1, -1], [-1, -1]], [-2, -1], 1, True),
    ("cg", "maxiter", "late", False, [[-1, -1], [-1, -1]], [-2, -1], 6, False),
    # ---- CG with ILU(0)
    ("cg", "init_converged", "early", True, [[-1, 0], [0, -1]], [0, 0], 6, False),
    ("cg", "init_nonfinite", "early", True, [[-1, 0], [0, -1]], [NAN, 1], 6, False),
    ("cg", "init_maxiter", "early", True, [[-1, 0], [0, -1]], [-2, -2], 0, False),
    ("cg", "pq0", "early", True, [[-1, 0], [0, 1]], [-2, -2], 6, False),
    ("cg", "pq0", "late", True, [[2, 1, 1], [1, 1, 0], [1, 0, 1]], [-2, -1, 0], 6, True),
    ("cg", "converged", "early", True, [[-1, 0], [0, -1]], [-2, -2], 6, True),
    ("cg", "converged", "late", True, [[1, 1, 1], [1, -2, 0], [1, 0, -1]], [0, 1, 0], 6, False),
    ("cg", "nonfinite", "early", True, [[1, -1], [-1, 1]], [0, 1], 6, False),           # a zero pivot: M^-1 r is not finite
    ("cg", "nonfinite", "late", True, [[2, 1, 0], [1, -1, 1], [0, 1, -1]], [-1, 0, 0], 6, False),
    ("cg", "maxiter", "late", True, [[-1, -1, -2], [-1, 1, 0], [-2, 0, -2]], [2, -2, 2], 6, False),
    # ---- BiCGStab, no preconditioner
    ("bicgstab", "init_converged", "early", False, [[-1, 0], [0, 1]], [0, 0], 6, False),
    ("bicgstab", "init_nonfinite", "early", False, [[NAN, 0], [0, 1]], [1, 1], 6, False),
    ("bicgstab", "init_maxiter", "early", False, [[2, -1], [0, 2]], [1, 2], 0, True),
    ("bicgstab", "rv0", "early", False, [[1, 0], [0, -1]], [1, 1], 6, True),
    ("bicgstab", "rv0", "late", False, [[-1, -1], [0, 0]], [-2, -1], 6, True),
    ("bicgstab", "half_converged", "early", False, [[-2, -2], [-2, -2]], [-1, -1], 6, True),
    ("bicgstab", "half_converged", "late", False, [[-1, 0], [0, 1]], [-2, -1], 6, True),
    ("bicgstab", "tt0", "early", False, [[-2, -2], [1, 1]], [-1, -1], 6, True),
    ("bicgstab", "tt0", "late", False, [[-2, -2], [-1, -1]], [-2, -2], 6, False),
    ("bicgstab", "converged", "early", False, [[-1, -1], [0, -1]], [0, -2], 6, True),
    ("bicgstab", "converged", "late", False, [[1, 0, 0], [0, -2, 0], [0, 1, -1]], [2, -2, -2], 6, True),
    ("bicgstab", "nonfinite", "late", False, [[2.0 ** 100, 1], [2.0 ** 301, 2]], [2.0 ** 100, 0], 6, False),
    ("bicgstab", "omega0", "early", False, [[-1, -1], [-1, 0]], [-2, 0], 6, True),
    ("bicgstab", "omega0", "early", False, [[-1, -1], [-1, 0]], [-2, 0], 1, True),   # omega == 0 is tested before k == maxIter
    ("bicgstab", "omega0", "late", False, [[0, -1, 0], [-1, -1, 0], [0, 0, 0]], [-2, 1, 1], 6, True),
    ("bicgstab", "maxiter", "early", False, [[-1, 0, 0], [0, 0, 1], [0, 0, 0]], [1, 2, 2], 1, True),  # rhon == 0: tested after
    ("bicgstab", "maxiter", "late", False, [[-2, 0], [-1, 0]], [-2, 1], 6, True),
    ("bicgstab", "rho0", "early", False, [[-1, 0, 0], [0, 0, 1], [0, 0, 0]], [1, 2, 2], 6, True),
    ("bicgstab", "rho0", "late", False, [[-2, 0, 0], [0, 2, 0], [1, 0, 0]], [-2, 1, 0], 6, False),
    # ---- BiCGStab with ILU(0); a diagonal or triangular A is its own factors: M^-1 A = I, s = 0 at k = 1
    ("bicgstab", "init_converged", "early", True, [[-1, 0], [0, -1]], [0, 0], 6, False),
    ("bicgstab", "init_nonfinite", "early", True, [[-1, 0], [0, -1]], [NAN, 1], 6, False),
    ("bicgstab", "init_maxiter", "early", True, [[-1, 0], [0, -1]], [-2, -2], 0, False),
    ("bicgstab", "rv0", "early", True, [[1, -1, 0], [2, -1, 0], [-1, 0, 1]], [2, -2, -2], 6, True),
    ("bicgstab", "rv0", "late", True, [[-2, 0, 2], [-2, -1, 0], [0, -1, -2]], [2, 1, 0], 6, False),
    ("bicgstab", "half_converged", "early", True, [[-1, 0], [0, -1]], [-2, -2], 6, False),
    ("bicgstab", "half_converged", "early", True, [[2, 0, 0], [-1, 1, 0], [1, -2, -2]], [1, -2, 2], 6, True),
    ("bicgstab", "half_converged", "late", True, [[1, 1, 0], [0, -1, 0], [1, 0, -1]], [1, 1, 1], 6, False),
    ("bicgstab", "tt0", "early", True, [[-2, 1, 0], [0, 1, -1], [-2, 0, 1]], [-2, 2, 0], 6, True),
    ("bicgstab", "converged", "early", True, [[1, 0, 1], [1, 1, 0], [0, 0, 2]], [2, 0, 1], 6, True),
    ("bicgstab", "converged", "late", True, [[-1, 1, -1], [1, 1, 0], [-1, 0, -2]], [-2, -1, 1], 6, False),
    ("bicgstab", "nonfinite", "early", True, [[1, -1], [-1, 1]], [0, 1], 6, False),     # a zero pivot
    ("bicgstab", "nonfinite", "late", True,
     [[2, 0, -1], [-2.0 ** 100, -2, -2.0 ** 601], [-1, -2.0 ** 401, 1]], [1, -2, -2.0 ** 300], 6, False),
    ("bicgstab", "omega0", "early", True, [[-1, 2, 0], [0, -1, 0], [-1, 0, 2]], [0, -1, -1], 6, True),
    ("bicgstab", "omega0", "late", True, [[-1, -2, -2], [0, -1, 0], [-1, 0, 1]], [0, -2, 2], 6, False),
    ("bicgstab", "maxiter", "late", True, [[1, -2, 0], [0, 1, 1], [-1, 0, -2]], [-2, -2, 2], 6, False),
    ("bicgstab", "rho0", "early", True, [[2, -1, -1], [-1, -2, 0], [-1, 0, 2]], [-1, 0, 0], 6, True),
    ("bicgstab", "rho0", "late", True, [[-1, 2, -1, 0], [2, 2, 0, 0], [-1, 0, 2, 1], [0, 0, 1, -1]], [2, 0, 0, 1], 6, False),
]

# labels that must come `early` and `late`; the others need one case
BOTH_WHENS = ("pq0", "rv0", "converged", "nonfinite")
# labels (of BiCGStab, un-preconditioned) that must have a large twin; CG's `converged` too
LARGE_REQUIRED = ("half_converged", "tt0", "rv0", "omega0", "rho0", "converged")
# (solver, preconditioned, label, when) for which no input is known, with the reason; tests/test_krylov_abi.py checks that
# the table has no other hole
HOLES = {}


def dense_csr(A, keep_diagonal):
    """the nonzero entries of a dense matrix (and its diagonal when asked) as CSR, columns ascending"""
    n = len(A)
    IRP, JA, AS = [0], [], []
    for i in range(n):
        for j in range(n):
            if A[i][j] != 0 or (keep_diagonal and i == j):
                JA.append(j)
                AS.append(float(A[i][j]))
        IRP.append(len(JA))
    return n, np.array(IRP, np.uint64), np.array(JA, np.uint64), np.array(AS, np.float64)


def kron_identity(c, M, IRP, JA, AS):
    """kron(I_c, A): c copies of A down the diagonal"""
    nnz = JA.size
    irp = (np.arange(c, dtype=np.uint64)[:, None] * np.uint64(nnz) + IRP[None, :-1]).ravel()
    ja = (np.arange(c, dtype=np.uint64)[:, None] * np.uint64(M) + JA[None, :]).ravel()
    return c * M, np.append(irp, np.uint64(c * nnz)), ja, np.tile(AS, c)


def _small_name(row, large):
    solver, label, when, pre, A, _, maxiter, _ = row
    return f"{solver}{'+ilu0' if pre else ''}:{label}:{when}:n{len(A)}:maxiter{maxiter}" + (":large" if large else "")


def _small(row, large):
    solver, label, when, pre, A, b, maxiter, _ = row
    M, IRP, JA, AS = dense_csr(A, pre)
    b, x0 = np.array(b, np.float64), np.zeros(M)
    name = _small_name(row, large)
    if large:
        c = 1
        while c * JA.size < AUTO_MIN_NNZ:
            c *= 2
        x0 = np.arange(1, M + 1, dtype=np.float64) * (-1.0) ** np.arange(M)
        b = b + np.array(A, np.float64) @ x0                            # small integers: exact
        M, IRP, JA, AS = kron_identity(c, M, IRP, JA, AS)
        b, x0 = np.tile(b, c), np.tile(x0, c)
    return Case(name, solver, label, when, pre, M, IRP, JA, AS, b, x0, 1e-8, maxiter)


def _overflow(solver):
    """NONFINITE inside the loop: an 8^3 Laplacian with one diagonal value 1e308 and b of magnitude 10^2: the init
    residual is finite, the first A p overflows"""
    IRP, JA, AS = laplacian7(8, 8, 8)
    AS = AS.copy()
    AS[np.flatnonzero(AS > 0)[100]] = 1e308
    b = 100.0 * (1.0 + np.random.default_rng(5100).random(512))
    return Case(f"{solver}:nonfinite:early:laplacian", solver, "nonfinite", "early", False, 512, IRP, JA, AS, b, np.zeros(512),
                1e-8, 50)


def _two_identity(n=10_000):
    """A = 2 I: every stored value the same double (a unit handle); alpha = 1/2 and s = 0 at k = 1 for any b"""
    i = np.arange(n, dtype=np.uint64)
    b = np.random.default_rng(5101).integers(-8, 9, n).astype(np.float64) / 4
    b[0] = 1.0
    return Case("bicgstab:half_converged:early:2I", "bicgstab", "half_converged", "early", False, n,
                np.arange(n + 1, dtype=np.uint64), i, np.full(n, 2.0), b, np.zeros(n), 1e-8, 6)


def _build():
    out = {}
    for row in _SMALL:
        for large in (False, True)[:1 + row[-1]]:
            name = _small_name(row, large)
            assert name not in out, name
            out[name] = lambda row=row, large=large: _small(row, large)
    for solver in ("cg", "bicgstab"):
        out[f"{solver}:nonfinite:early:laplacian"] = lambda solver=solver: _overflow(solver)
    out["bicgstab:half_converged:early:2I"] = _two_identity
    return out


_BUILDERS = _build()
NAMES = tuple(_BUILDERS)


def case(name):
    """one case of the table, built on demand (a large one is a few MB)"""
    c = _BUILDERS[name]()
    assert c.name == name
    return c
