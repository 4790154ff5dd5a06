"""The block entry points (spmvHipBlockDot, hipSpCGBlockCSR, hipSpBiCGStabBlockCSR) are declared, exported and bound in
Python; the block reference (tests/block_krylov_ref.py) is the single reference per column; every column of every sum of
tests/block_exit_inputs.py and of its large twin takes the label and the early / late class its case has in the exit
table, and together the columns take every exit of each loop but `init_maxiter` (which a maxIter = 0 call takes); and a
planted fault -- a stopped column that goes on being updated for one more iteration -- changes that column's bits.  No GPU
needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import block_exit_inputs as sums
import serial_order_inputs as si
from bits import assert_same_bits
from block_krylov_ref import block_dot_ref, block_ref, block_x, column_ref, one_more_iteration
from c_header import HEADER, code as _code
from conftest import ROOT
from krylov_ref import BICGSTAB_EXITS, CG_EXITS, MAXITER, Csr, bicgstab_ref, cg_ref, dot_ref
from test_trsv_abi import laplacian7

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
_DENSE = r"const\s+double\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*int\s+\w+\s*,\s*"
_SOLVER = (r"spmat\s*\*\s*\w+\s*,\s*spmat\s*\*\s*\w+\s*,\s*unsigned\s+k\s*,\s*" + _DENSE +
           r"double\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+spmvKrylovOpts\s*\*\s*\w+\s*,\s*"
           r"spmvKrylovColumn\s*\*\s*\w+\s*,\s*spmvKrylovInfo\s*\*\s*\w+")
DECLS = {
    "spmvHipBlockDot": r"size_t\s+n\s*,\s*unsigned\s+k\s*,\s*" + _DENSE + _DENSE + r"double\s*\*\s*\w+",
    "hipSpCGBlockCSR": _SOLVER,
    "hipSpBiCGStabBlockCSR": _SOLVER,
}
COLUMN = ("status", "iterations", "rr", "bb")


def test_header_declares_the_three_and_the_struct():
    code = _code(HEADER)
    for name, params in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spmvKrylovColumn\s*;", code, re.S)
    assert body and re.findall(r"(\w+)\s*;", body.group(1)) == list(COLUMN)


def test_library_exports_the_three():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_three():
    from spmv_openmp_cuda_amd import api
    for name, n in (("spmvHipBlockDot", 9), ("hipSpCGBlockCSR", 12), ("hipSpBiCGStabBlockCSR", 12)):
        assert name in api._sigs
        assert len(getattr(api.lib, name).argtypes) == n, name
    for m in ("cg_block", "bicgstab_block"):
        assert callable(getattr(api.DeviceMatrix, m))
    assert callable(api.block_dot)
    assert [f for f, _ in api.spmvKrylovColumn._fields_] == list(COLUMN)


# ------------------------------------------------------------------------------------------------- the sums and their twins
@pytest.mark.parametrize("solver,precond", sums.KINDS)
def test_shape_of_the_sums(solver, precond):
    s = sums.block_sum(solver, precond)
    want = {("cg", False): (8, 32), ("cg", True): (8, 32), ("bicgstab", False): (16, 64), ("bicgstab", True): (16, 64)}
    assert (s.B.shape[1], s.M) == want[solver, precond]
    assert s.B.shape == (s.M, len(s.labels)) and not s.X0.any()
    for c in range(s.B.shape[1]):                                        # column c lives in its own slot
        outside = np.ones(s.M, bool)
        outside[sums.SLOT * c:sums.SLOT * (c + 1)] = False
        assert not s.B[outside, c].any()


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("solver,precond", sums.KINDS)
def test_every_column_takes_its_label(solver, precond, large):
    s = sums.block_sum(solver, precond, large)
    _, cols, info = sums.reference(solver, precond, large)
    if large:
        assert s.JA.size >= si.AUTO_MIN_NNZ and s.X0.any()
        small = sums.block_sum(solver, precond)
        assert s.M % small.M == 0 and s.labels == small.labels
    for c, (label, when, col) in enumerate(zip(s.labels, s.whens, cols)):
        assert col.label == label, (s.name, c, col.label, label)
        assert (col.iterations <= 1) == (when == "early"), (s.name, c, col.iterations, when)
    stops = {c.iterations for c in cols}
    assert {0, 1, 2, sums.MAXITER} <= stops, stops                      # and one column runs to maxIter
    assert info[0] == max(c.status for c in cols) and info[1] == sums.MAXITER


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_the_label_set_is_complete(solver):
    """with and without ILU(0) together, the columns take every exit of the loop except init_maxiter; a maxIter = 0 call
    takes that one on every column that does not stop before it"""
    seen = set()
    for precond in (False, True):
        seen |= {c.label for c in sums.reference(solver, precond)[1]}
    assert seen == set(CG_EXITS if solver == "cg" else BICGSTAB_EXITS) - {"init_maxiter"}
    s = sums.block_sum(solver, False)
    A = sums.reference(solver, False)[0]
    cols, info = block_ref(solver, A, s.B, s.X0, sums.TOL, 0)
    labels = {c.label for c in cols}
    assert "init_maxiter" in labels and labels <= {"init_maxiter", "init_converged", "init_nonfinite"}
    assert all(c.iterations == 0 for c in cols)


# ------------------------------------------------------------------------------------------------- the reference
def test_block_dot_reference_is_the_dot_per_column():
    rng = np.random.default_rng(2700)
    n, k = 2 * 4096 + 3, 5
    U = np.stack([si.order_values(rng, n, 8) for _ in range(k)], axis=1)
    V = np.stack([si.order_values(rng, n, 8) for _ in range(k)], axis=1)
    h = block_dot_ref(U, V)
    for c in range(k):
        assert_same_bits(h[c:c + 1], np.array([dot_ref(U[:, c].copy(), V[:, c].copy())]), f"column {c}")
    assert len({x.tobytes() for x in h}) == k


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_block_reference_is_the_single_reference_per_column(solver):
    n = 6
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    rng = np.random.default_rng(2701)
    B = np.stack([rng.random(M) * 10.0 ** e for e in (0, 3, -3)] + [np.zeros(M)], axis=1)
    X0 = rng.uniform(-1, 1, B.shape)
    A = Csr(M, IRP, JA, AS)
    cols, info = block_ref(solver, A, B, X0, 1e-6, 50)
    single = cg_ref if solver == "cg" else bicgstab_ref
    for c, col in enumerate(cols):
        x, st, it, hist, rr = single(A, B[:, c].copy(), X0[:, c].copy(), 1e-6, 50)
        assert (col.status, col.iterations) == (st, it)
        assert_same_bits(col.x, x, f"column {c}: x")
        assert_same_bits(col.history, hist, f"column {c}: history")
        assert_same_bits(np.array([col.rr, col.bb]), np.array([rr, dot_ref(B[:, c], B[:, c])]), f"column {c}: rr, bb")
    assert block_x(cols).shape == B.shape
    assert len({c.iterations for c in cols}) > 1                        # the columns do stop at different iterations
    lead = next(c for c in cols if c.status == info[0])
    assert info == (max(c.status for c in cols), max(c.iterations for c in cols), lead.rr, lead.bb)


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_a_planted_fault_changes_a_column(solver):
    """a stopped column that is updated for one more iteration: its x differs from the reference's in at least one bit,
    so a comparison by bits with the reference catches a block loop that does not freeze its stopped columns.  (With
    ILU(0) the converged columns of the sums have rr = 0, and one more iteration is a breakdown that writes nothing; the
    unpreconditioned sums have columns with room for the fault.)"""
    caught = 0
    for precond in (False, True):
        s = sums.block_sum(solver, precond)
        A, cols, _ = sums.reference(solver, precond)
        for c, col in enumerate(cols):
            x = one_more_iteration(solver, A, s.B[:, c], s.X0[:, c], sums.TOL, sums.MAXITER, col)
            if x is not None and x.tobytes() != col.x.tobytes():
                caught += 1
                with pytest.raises(AssertionError):
                    assert_same_bits(x, col.x, f"{s.name}, column {c}")
    assert caught >= 1, solver
