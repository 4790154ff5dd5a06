"""The sweep preconditioner inside every Krylov solver (spmvHipTriSetApply; DeviceMatrix.set_triangular_apply): on the ILU(0)
factors of a 6 x 5 x 4 Laplacian and of a nonsymmetric upwind stencil of the same size, x, every history entry, status and
counts of hipSpCGCSR, hipSpBiCGStabCSR, hipSpGMRESCSR, hipSpCGBlockCSR and hipSpBiCGStabBlockCSR have the bits of the
reference loops already used for the ILU(0)-preconditioned tests (krylov_ref, gmres_ref, block_krylov_ref) with the two exact
solves replaced by the sweep loops (sweeps_ref.SweepCsr); the launch counters count the sweep launches; a column of a block
that stops early freezes; and after set_triangular_apply(None) the exact bits are back."""
import numpy as np
import pytest

from block_krylov_ref import block_ref
from gmres_ref import gmres_ref
from ilu0_ref import ilu0_levels
from krylov_ref import CONVERGED, Csr, bicgstab_ref, cg_ref
from sweeps_ref import SweepCsr
from test_gpu_solver_counters import block_rule, single_rule
from test_gpu_trsv import same
from test_krylov_abi import convdiff7
from test_trsv_abi import laplacian7

pytestmark = pytest.mark.gpu
GRID = (6, 5, 4)
TOL, CAP, RESTART, K = 1e-9, 60, 7, 16
COUNTS = {"cg": ((2, 2), (0, 0), (12, 12)), "bicgstab": ((2, 2), (3, 1), (0, 2), (2, 0)), "gmres": ((2, 2), (1, 3), (2, 0))}
REFS = {"cg": cg_ref, "bicgstab": bicgstab_ref}


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(scope="module", params=["laplacian", "convdiff"])
def problem(api, request):
    """(name, M, IRP, JA, AS, F, b, (B, X0), dA, dM): dM holds the ILU(0) factors F.  Of the block's five columns the
    second is zero (it stops at the init) and the fourth starts 1e-5 from its solution (it stops some iterations before the
    others): both must freeze while the rest go on"""
    IRP, JA, AS = laplacian7(*GRID) if request.param == "laplacian" else convdiff7(*GRID)
    M = GRID[0] * GRID[1] * GRID[2]
    rng = np.random.default_rng(4400)
    b = rng.standard_normal(M)
    B = np.stack([b, np.zeros(M), b * 0.5 + rng.standard_normal(M), 1e-3 * rng.standard_normal(M), rng.standard_normal(M)], axis=1)
    dense = np.zeros((M, M))
    dense[np.repeat(np.arange(M), np.diff(IRP.astype(np.int64))), JA.astype(np.int64)] = AS
    X0 = np.zeros_like(B)
    X0[:, 3] = np.linalg.solve(dense, B[:, 3]) * (1.0 + 1e-5 * rng.standard_normal(M))
    B = (B, X0)
    dA = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    dM = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    dM.ilu0()
    yield request.param, M, IRP, JA, AS, ilu0_levels(M, IRP, JA, AS), b, B, dA, dM
    dM.free()
    dA.free()


def _solvers(name):
    return ("cg", "bicgstab", "gmres") if name == "laplacian" else ("bicgstab", "gmres")


def _single(dA, dM, solver, b):
    kw = {"restart": RESTART} if solver == "gmres" else {}
    return getattr(dA, solver)(b, precond=dM, tol=TOL, maxiter=CAP, history=True, **kw)


def _reference(solver, A, b):
    if solver == "gmres":
        return gmres_ref(A, b, np.zeros_like(b), TOL, CAP, RESTART)
    return REFS[solver](A, b, np.zeros_like(b), TOL, CAP)


def _check(got, ref, what):
    x, info = got
    rx, st, it, hist, rr = ref
    assert (info.status, info.iterations) == (st, it), (what, info.status, info.iterations, st, it)
    same(x, rx, what + ": x")
    same(info.history, hist, what + ": history")
    same(np.array([info.rr]), np.array([rr]), what + ": rr")


def test_single_solvers_have_the_reference_bits_and_count_the_sweep_launches(api, problem):
    name, M, IRP, JA, AS, F, b, B, dA, dM = problem
    for solver in _solvers(name):
        for sl, su in COUNTS[solver]:
            what = f"{name}, {solver}, sweeps ({sl}, {su})"
            dM.set_triangular_apply((sl, su))
            plan = dM.triangular_sweeps_info()
            c = sl + su + (0 if sl and su else 1)
            assert (plan.mode, plan.lowerSweeps, plan.upperSweeps, plan.applyLaunches) == (1, sl, su, c), what
            A = SweepCsr(M, IRP, JA, AS, F, sl, su)
            got, ref = _single(dA, dM, solver, b), _reference(solver, A, b)
            _check(got, ref, what)
            if solver != "gmres":
                want = single_rule(solver, CAP, K, ref[2], True, c)
                assert (got[1].launches, got[1].hostChecks) == want, (what, got[1].launches, got[1].hostChecks, want)
    # (the factorisation analysed the lower triangle for itself; the solves analysed nothing more)
    assert dM.triangular_info(True).analyses == 1 and dM.triangular_info(False).levels == 0, "a dM in SWEEPS mode is not analysed"


def test_gmres_launches_grow_by_the_sweep_launches_alone(api, problem):
    """levels - 1, levels + 1 and levels + 3 sweeps give the same bits, so the same cycles: a cycle enqueues `restart` steps
    and its update whether or not it ends early (a stopped step's kernels return at once but are launched), each with one
    application, so the launch counts differ by 4 (restart + 1) per cycle each time"""
    name, M, IRP, JA, AS, F, b, B, dA, dM = problem
    L = sum(GRID) - 2
    runs = []
    for S in (L - 1, L + 1, L + 3):
        dM.set_triangular_apply(S)
        runs.append(_single(dA, dM, "gmres", b))
    A = SweepCsr(M, IRP, JA, AS, F, L - 1, L - 1)
    stats = {}
    _check(runs[0], gmres_ref(A, b, np.zeros_like(b), TOL, CAP, RESTART, stats=stats), f"{name}, gmres at levels - 1")
    for r in runs[1:]:
        same(r[0], runs[0][0], "the same bits from levels - 1 sweeps on")
    l0, l1, l2 = (int(r[1].launches) for r in runs)
    assert l1 - l0 == l2 - l1 == 4 * stats["cycles"] * (RESTART + 1), (l0, l1, l2, stats["cycles"])


def test_exact_mode_gives_the_exact_bits_again(api, problem):
    name, M, IRP, JA, AS, F, b, B, dA, dM = problem
    L = sum(GRID) - 2
    for solver in _solvers(name):
        dM.set_triangular_apply(L - 1)
        at_levels = _single(dA, dM, solver, b)
        dM.set_triangular_apply((1, 1))
        dM.set_triangular_apply(None)
        info = dM.triangular_sweeps_info()
        assert (info.mode, info.applyLaunches, info.prepares) == (0, 0, 1)
        exact = _single(dA, dM, solver, b)
        _check(exact, _reference(solver, Csr(M, IRP, JA, AS, F), b), f"{name}, {solver}, EXACT again")
        _check(at_levels, _reference(solver, Csr(M, IRP, JA, AS, F), b), f"{name}, {solver}, levels - 1 sweeps")
    assert dM.triangular_info(True).levels == L == dM.triangular_info(False).levels


def test_block_solvers_column_by_column(api, problem):
    name, M, IRP, JA, AS, F, b, (B, X0), dA, dM = problem
    for solver in _solvers(name)[:-1]:                     # (cg on the symmetric matrix only; gmres has no block form)
        for sl, su in ((2, 2),) if solver == "cg" else ((2, 2), (3, 1)):
            what = f"{name}, {solver}_block, sweeps ({sl}, {su})"
            dM.set_triangular_apply((sl, su), block_width=5)
            assert dM.triangular_sweeps_info().width >= 5
            A = SweepCsr(M, IRP, JA, AS, F, sl, su)
            cols, (status, its, rr, bb) = block_ref(solver, A, B, X0, TOL, CAP)
            X, info = getattr(dA, solver + "_block")(B, X0=X0, precond=dM, tol=TOL, maxiter=CAP, history=True)
            assert (info.status, info.iterations) == (status, its), what
            stops = sorted({c.iterations for c in cols})
            assert stops[0] == 0 and len(stops) >= 3, "columns stop at different iterations: the early ones must freeze"
            for c, r in enumerate(cols):
                assert (info.columns[c].status, info.columns[c].iterations) == (r.status, r.iterations), (what, c)
                same(X[:, c], r.x, f"{what}, column {c}: x")
                same(info.history[c], r.history, f"{what}, column {c}: history")
            c1 = sl + su + (0 if sl and su else 1)
            want = block_rule(solver, CAP, K, its, True, c1)
            assert (info.launches, info.hostChecks) == want, (what, info.launches, info.hostChecks, want)
        dM.set_triangular_apply(None)
        X, info = getattr(dA, solver + "_block")(B, X0=X0, precond=dM, tol=TOL, maxiter=CAP)
        cols, _ = block_ref(solver, Csr(M, IRP, JA, AS, F), B, X0, TOL, CAP)
        for c, r in enumerate(cols):
            same(X[:, c], r.x, f"{name}, {solver}_block, EXACT again, column {c}")
