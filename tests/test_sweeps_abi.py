"""The sweep-solve entry points (spmvHipTriSweepsPrepare, hipSpTRSVSweepsCSR, hipSpTRSMSweepsCSR, spmvHipTriSetApply,
spmvHipTriSweepsInfo) are declared, exported and bound in Python with the C layout of spmvTriSweepsInfo; the two references
of tests/sweeps_ref.py agree bit for bit on every input of tests/sweeps_inputs.py, equal the exact triangular loop from
levels - 1 sweeps on, and tell each planted fault apart; and the sweep preconditioner's iteration counts behave as the
contract says.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import c_header
import serial_order_inputs as si
import sweeps_inputs
from bits import differing_rows
from c_header import HEADER, code as _code
from conftest import ROOT
from gmres_ref import gmres_ref
from ilu0_ref import ilu0_levels
from krylov_ref import CONVERGED, Csr, bicgstab_ref, cg_ref
from sweeps_ref import FAULTS, SweepCsr, sweeps_loop, sweeps_numpy
from test_trsv_abi import _same, laplacian7, random_square
from trsv_ref import levels, trsv_levels, trsv_loop

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
SP, I, U, CD, D, SZ = r"spmat\s*\*\s*\w+", r"int\s+\w+", r"unsigned\s+\w+", r"const\s+double\s*\*\s*\w+", r"double\s*\*\s*\w+", r"size_t\s+\w+"
DECLS = {
    "spmvHipTriSweepsPrepare": (SP, U),
    "hipSpTRSVSweepsCSR": (SP, I, I, U, CD, D),
    "hipSpTRSMSweepsCSR": (SP, I, I, U, U, CD, SZ, I, D, SZ, I),
    "spmvHipTriSetApply": (SP, I, U, U, U),
    "spmvHipTriSweepsInfo": (SP, r"spmvTriSweepsInfo\s*\*\s*\w+"),
}
FIELDS = ("mode", "lowerSweeps", "upperSweeps", "width", "solveLaunches", "applyLaunches", "firstBadDiag", "sorted", "prepares", "bytes", "diagPos",
          "workspace")


# ------------------------------------------------------------------------------------------------- the boundary
def test_header_declares_the_five():
    code = _code(HEADER)
    for name, params in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + r"\s*,\s*".join(params) + r"\s*\)\s*;", code, re.M), name
    for const, value in (("SPMV_TRI_APPLY_EXACT", 0), ("SPMV_TRI_APPLY_SWEEPS", 1), ("SPMV_TRI_SWEEPS_MAX", 4096)):
        assert re.search(r"#define\s+" + const + r"\s+" + str(value) + r"\b", code), const


def test_header_states_the_loop_and_its_consequence():
    text = open(HEADER).read()
    for piece in ("x0[i] = STORED ? b[i] / d_i : b[i]", "acc += AS[p] * x(s-1)[j]", "S >= levels - 1", "bits of\n *      hipSpTRSVCSR",
                  "S = 0 is the diagonal scaling", "never added as 0.0"):
        assert piece in text, piece


def test_library_exports_the_five():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_five():
    from spmv_openmp_cuda_amd import api
    for name, params in DECLS.items():
        assert name in api._sigs
        assert len(getattr(api.lib, name).argtypes) == len(params), name
    for m in ("solve_triangular", "solve_triangular_block", "set_triangular_apply", "triangular_sweeps_info", "prepare_triangular_sweeps"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert [f[0] for f in api.spmvTriSweepsInfo._fields_] == list(FIELDS)
    assert (api.SPMV_TRI_APPLY_EXACT, api.SPMV_TRI_APPLY_SWEEPS, api.SPMV_TRI_SWEEPS_MAX) == (0, 1, 4096)


def test_struct_layout_matches_c(tmp_path):
    from spmv_openmp_cuda_amd import api
    assert c_header.structs()["spmvTriSweepsInfo"] == list(FIELDS)
    body = '    printf("%zu", sizeof(spmvTriSweepsInfo));\n' + "".join(f'    printf(" %zu", offsetof(spmvTriSweepsInfo, {f}));\n' for f in FIELDS)
    got = [int(v) for v in c_header.run_c(tmp_path, body, "sweeps_layout").split()]
    assert got == [C.sizeof(api.spmvTriSweepsInfo)] + [getattr(api.spmvTriSweepsInfo, f).offset for f in FIELDS]


# ------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("name", sweeps_inputs.NAMES)
def test_the_two_references_agree_and_reach_the_exact_loop(name):
    """both triangles, both diagonals, S in {0, 1, 2, 3, levels - 1, levels + 1}: loop == numpy by bits; from levels - 1
    sweeps on both have the bits of the exact triangular loop (levels computed here)"""
    M, IRP, JA, AS, b = sweeps_inputs.make(name)
    for lower in (True, False):
        counts, L = sweeps_inputs.sweep_counts(M, IRP, JA, lower)
        assert L == int(levels(M, IRP, JA, lower).max()) + 1
        for unit in (False, True):
            exact = trsv_levels(M, IRP, JA, AS, b, lower, unit)
            if M <= 300:
                _same(exact, trsv_loop(M, IRP, JA, AS, b, lower, unit), f"{name}: the exact references")
            for S in counts:
                what = f"{name}, lower {lower}, unit {unit}, S = {S}"
                x = sweeps_numpy(M, IRP, JA, AS, b, S, lower, unit)
                if M <= 300 or S <= 1 or S == L - 1:                # (the plain-Python loop on every small case and some of the large)
                    _same(sweeps_loop(M, IRP, JA, AS, b, S, lower, unit), x, what + ": loop against numpy")
                if S >= L - 1:
                    _same(x, exact, what + ": against the exact loop")


def test_fewer_sweeps_than_levels_differ_from_the_exact_solve():
    """the level argument is sharp: with levels - 2 sweeps some row of the last level is not final yet"""
    M = 10                                                 # the chain x[i] - x[i-1] = 1: x[i] = i + 1, x(S)[i] = min(i, S) + 1
    i = np.arange(M)
    IRP, JA, AS = si.assemble(M, np.concatenate([i, i[1:]]), np.concatenate([i, i[1:] - 1]), np.concatenate([np.ones(M), -np.ones(M - 1)]))
    for S in range(M + 2):
        assert np.array_equal(sweeps_numpy(M, IRP, JA, AS, np.ones(M), S, True, False), np.minimum(i, S) + 1.0), S
    M, IRP, JA, AS, b = sweeps_inputs.make("r65")
    x1 = sweeps_numpy(M, IRP, JA, AS, b, 1, True, False)
    lvl = levels(M, IRP, JA, True)
    exact = trsv_levels(M, IRP, JA, AS, b, True, False)
    assert differing_rows(x1[lvl <= 1], exact[lvl <= 1]).size == 0, "rows of level <= S are exact"


def test_zero_sweeps_is_the_diagonal_scaling():
    M, IRP, JA, AS, b = sweeps_inputs.make("r64")
    from trsv_ref import diag_pos
    dpos, _ = diag_pos(M, IRP, JA)
    _same(sweeps_loop(M, IRP, JA, AS, b, 0, True, False), b / AS[dpos], "S = 0, STORED")
    _same(sweeps_loop(M, IRP, JA, AS, b, 0, False, True), b, "S = 0, UNIT")


def _fault_inputs():
    """(M, IRP, JA, AS, b, unit): order-sensitive unsorted rows with repeated pairs; and a matrix whose diagonal holds 0.0,
    NaN and Inf solved with a UNIT diagonal -- those entries lie outside the strict triangle, and a sum that takes them in
    as value * 0.0 turns NaN where the loop, which skips them, stays finite (with finite values the same slip can only
    show as the sign of a zero, which a sum that starts at +0.0 never keeps)"""
    rng = np.random.default_rng(77)
    M = 120
    IRP, JA, AS = random_square(rng, M, 8)
    yield M, IRP, JA, AS, si.order_values(rng, M), False
    M, IRP, JA, AS, b = sweeps_inputs.make("bad_diagonals")
    yield M, IRP, JA, AS, b, True


@pytest.mark.parametrize("fault", FAULTS)
def test_every_planted_fault_is_told_apart(fault):
    hit = 0
    for M, IRP, JA, AS, b, unit in _fault_inputs():
        for lower in (True, False):
            for S in (1, 2, 3):
                good = sweeps_loop(M, IRP, JA, AS, b, S, lower, unit)
                hit += differing_rows(sweeps_loop(M, IRP, JA, AS, b, S, lower, unit, fault=fault), good).size > 0
    assert hit > 0, f"no input tells the fault '{fault}' from the loop"


# ------------------------------------------------------------------------------------------------- the preconditioner
GRID = (12, 12, 12)
COUNTS = (0, 1, 2, 3, 4, 6, 8, 12, 20)


@pytest.fixture(scope="module")
def laplacian():
    IRP, JA, AS = laplacian7(*GRID)
    M = GRID[0] * GRID[1] * GRID[2]
    F = ilu0_levels(M, IRP, JA, AS)
    b = np.random.default_rng(12).standard_normal(M)
    L = int(levels(M, IRP, JA, True).max()) + 1
    assert L == sum(GRID) - 2 == int(levels(M, IRP, JA, False).max()) + 1
    return M, IRP, JA, AS, F, b, L


def _iterations(solver, A, b):
    if solver == "gmres":
        x, status, it, hist, rr = gmres_ref(A, b, np.zeros_like(b), 1e-8, 300, 30)
    else:
        x, status, it, hist, rr = (cg_ref if solver == "cg" else bicgstab_ref)(A, b, np.zeros_like(b), 1e-8, 300)
    assert status == CONVERGED
    return it, x


@pytest.mark.parametrize("solver", ["cg", "bicgstab", "gmres"])
def test_iteration_counts_on_the_12_cubed_laplacian(laplacian, solver):
    """ILU(0) of the 12 x 12 x 12 7-point Laplacian (34 levels per triangle), b standard normal (seed 12), tol 1e-8, the
    reference loops of krylov_ref / gmres_ref with M^-1 by S sweeps per triangle.  Iterations to convergence:

        S          none   0    1    2    3    4    6    8   12   20   33 (= levels - 1)   exact
        cg           48  48   27   20   18   18   18   18   18   18   18                   18
        bicgstab     37  37   18   14   12   12   12   11   11   11   11                   11
        gmres(30)    59  59   26   19   18   18   18   18   18   18   18                   18

    The counts never grow from S = 0 to the exact solve, and at S = levels - 1 the whole solve has the bits of the exact
    preconditioner's, x included."""
    M, IRP, JA, AS, F, b, L = laplacian
    exact_it, exact_x = _iterations(solver, Csr(M, IRP, JA, AS, F), b)
    counts = []
    for S in COUNTS + (L - 1,):
        it, x = _iterations(solver, SweepCsr(M, IRP, JA, AS, F, S, S), b)
        counts.append(it)
    print(solver, "none", _iterations(solver, Csr(M, IRP, JA, AS), b)[0], dict(zip(COUNTS + (L - 1,), counts)), "exact", exact_it)
    assert all(a >= c for a, c in zip(counts, counts[1:])), counts
    assert counts[-1] == exact_it
    assert differing_rows(x, exact_x).size == 0
