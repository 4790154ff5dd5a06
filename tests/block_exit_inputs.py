"""Blocks of right-hand sides whose columns leave hipSpCGBlockCSR / hipSpBiCGStabBlockCSR by different exits at different
iterations: the direct sum of the small cases of krylov_exit_inputs._SMALL.  Shared by tests/test_block_krylov_abi.py (every
column takes the label and the early / late class its case has in the table: no GPU needed) and
tests/test_gpu_block_krylov.py.

One 4-row slot per case: a case of order < 4 is padded, with ILU(0) the padding rows carry a diagonal 1.0, so every case
starts at a row offset that is a multiple of 4.  Column c is case c's b in its own slot and zero elsewhere; maxIter = 6,
tol = 1e-8.  A column's dots are then the bits of the small case: the products of rows 4 s .. 4 s + 3 sit in the adjacent
lanes 2 s and 2 s + 1 of the fixed-order dot, which meet last in its tree, and everything else adds +0.0.  Only the
maxiter == 6 cases with a finite matrix are taken, with ILU(0) those without a zero pivot: a NaN in A and a zero pivot reach
every column through NaN * 0 -- the loop's behaviour, not a fault, but it makes all columns alike.  The unpreconditioned
sums get one more slot, [[-1, 0], [0, 1]] with b = [NaN, 1], for `init_nonfinite`.  `init_maxiter` needs maxIter = 0 and
so a call of its own.

A `large` twin is kron(I_c, A) of the whole sum's matrix with B tiled, c the smallest power of two with
c * nnz >= AUTO_MIN_NNZ, X0 a nonzero integer block and B shifted by A X0 as the table's twins do.  The sums have 8 and 16
slots, so a copy is 32 or 64 rows and every copy meets the dot's slices of 512 alike.  A column whose case has a large
twin in the table is tiled into every copy, with its X0 and its shift.  The other columns would not all keep their label
that way (a lane of the dot adds eight equal products, and 3 v is not exact), so their b goes, with X0 = 0, only into the
copies that lie in the first 512 rows of every block of 4 096: each lane then adds one nonzero product per block, every dot
is a power of two times the small case's, exactly, and the column takes the small case's exit at its iteration.
tests/test_block_krylov_abi.py asserts the label and the class of every column of every twin."""
import functools
from collections import namedtuple

import numpy as np

import krylov_exit_inputs as exits
from serial_order_inputs import AUTO_MIN_NNZ

SLOT = 4
TOL, MAXITER = 1e-8, 6
Sum = namedtuple("Sum", "name solver precond M IRP JA AS B X0 labels whens")
KINDS = (("cg", False), ("cg", True), ("bicgstab", False), ("bicgstab", True))
# the extra slot of the unpreconditioned sums
_EXTRA = ("init_nonfinite", "early", [[-1, 0], [0, 1]], [exits.NAN, 1])


def _finite(A):
    return bool(np.isfinite(np.array(A, np.float64)).all())


def _zero_pivot(A):
    from ilu0_ref import ilu0_levels
    M, IRP, JA, AS = exits.dense_csr(A, True)
    with np.errstate(all="ignore"):
        F = ilu0_levels(M, IRP, JA, AS)
    rows = np.repeat(np.arange(M), np.diff(IRP.astype(np.int64)))
    return bool((F[JA.astype(np.int64) == rows] == 0).any()) or not np.isfinite(F).all()


def _small_integers(A, b):
    a = np.array(A, np.float64)
    b = np.array(b, np.float64)
    return bool((np.abs(a) <= 2).all() and (np.isnan(b) | (np.abs(b) <= 2)).all())


def rows_of(solver, precond):
    """(label, when, A, b, in the twin) of the slots of a sum, in the table's order"""
    out = []
    for s, label, when, pre, A, b, maxiter, twin in exits._SMALL:
        if (s, pre) != (solver, precond) or maxiter != MAXITER or not _finite(A) or (pre and _zero_pivot(A)):
            continue
        out.append((label, when, A, b, twin))
    if not precond:
        out.append(_EXTRA + (False,))
    return out


@functools.lru_cache(maxsize=None)
def block_sum(solver, precond, large=False):
    rows = rows_of(solver, precond)
    k = len(rows)
    M = SLOT * k
    IRP, JA, AS = [0], [], []
    B, X0 = np.zeros((M, k)), np.zeros((M, k))
    for c, (_, _, A, b, twin) in enumerate(rows):
        n = len(A)
        for i in range(SLOT):
            for j in range(n if i < n else 0):
                if A[i][j] != 0 or (precond and i == j):
                    JA.append(SLOT * c + j)
                    AS.append(float(A[i][j]))
            if i >= n and precond:
                JA.append(SLOT * c + i)
                AS.append(1.0)
            IRP.append(len(JA))
        b = np.array(b, np.float64)
        if large and twin:                                               # as the table's twins: x0 != 0, b shifted by A x0 (exact)
            x0 = np.arange(1, n + 1, dtype=np.float64) * (-1.0) ** np.arange(n)
            X0[SLOT * c:SLOT * c + n, c] = x0
            b = b + np.array(A, np.float64) @ x0
        B[SLOT * c:SLOT * c + n, c] = b
    IRP, JA, AS = np.array(IRP, np.uint64), np.array(JA, np.uint64), np.array(AS, np.float64)
    name = f"{solver}{'+ilu0' if precond else ''}:sum" + (":large" if large else "")
    if large:                                                            # the whole matrix, the twin's columns
        keep = list(range(k))
        rows = [rows[c] for c in keep]
        c = 1
        while c * JA.size < AUTO_MIN_NNZ:
            c *= 2
        M, IRP, JA, AS = exits.kron_identity(c, M, IRP, JA, AS)
        B, X0 = np.tile(B[:, keep], (c, 1)), np.tile(X0[:, keep], (c, 1))
        others = [i for i, r in enumerate(rows) if not r[4]]
        B[np.ix_(np.arange(M) % 4096 >= 512, others)] = 0.0
    for a in (IRP, JA, AS, B, X0):
        a.setflags(write=False)
    return Sum(name, solver, precond, M, IRP, JA, AS, B, X0, tuple(r[0] for r in rows), tuple(r[1] for r in rows))


@functools.lru_cache(maxsize=None)
def reference(solver, precond, large=False):
    """(Csr with its factors, columns, block info) of a sum, computed once and shared; nothing in it may be changed"""
    from block_krylov_ref import block_ref
    from ilu0_ref import ilu0_levels
    from krylov_ref import Csr
    s = block_sum(solver, precond, large)
    with np.errstate(all="ignore"):
        F = ilu0_levels(s.M, s.IRP, s.JA, s.AS) if precond else None
    A = Csr(s.M, s.IRP, s.JA, s.AS, F)
    cols, info = block_ref(solver, A, s.B, s.X0, TOL, MAXITER)
    for c in cols:
        c.x.setflags(write=False)
        c.history.setflags(write=False)
    return A, cols, info
