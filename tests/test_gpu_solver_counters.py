"""What a CG / BiCGStab solve enqueues and how often the host looks, for the single solves and the block solves, as one
table: (status, iterations, launches, hostChecks) of every case against the rules below, and column 0 of a block's X
against the single solve's x in all bits.  The matrix is the 7-point Laplacian 17 x 17 x 17: its 4 913 rows make two
blocks of dot partials, the second partly filled.

The rules (c: the launches of one M^-1; n: the iterations enqueued; K: iterations per host check; j*: the iteration in
whose kernels the stop was set, 0 for a stop at the init):
  CG enqueues 4 + 6 n (+ (n + 1)(c + 2) with a dM), BiCGStab 3 + n (11 + 2 c).
  single, maxIter >= 1: hostChecks = max(1, ceil(j* / K)), n = min(maxIter, K hostChecks); maxIter = 0: no check, n = 0.
  block: one check after the init; every column stopped there: 3 launches and nothing more; otherwise one more check
  per batch, ceil(j* / K) of them with j* the largest over the columns, n = min(maxIter, K ceil(j* / K)).
A block of one column runs the block path when its leading dimension is padded (a plain vector takes the single solve)."""
import ctypes as C

import numpy as np
import pytest

from amg_gpu import _up, cycle_launches
from bits import assert_same_bits
from krylov_ref import CONVERGED, MAXITER
from spgemm_ref import laplacian7

pytestmark = pytest.mark.gpu

GRID = (17, 17, 17)
TOL = 1e-8
CAP = 200
SINGLE = {"cg": "hipSpCGCSR", "bicgstab": "hipSpBiCGStabCSR"}
BLOCK = {"cg": "hipSpCGBlockCSR", "bicgstab": "hipSpBiCGStabBlockCSR"}
WIDTHS = ((1, 2), (2, 2), (3, 3), (17, 17))             # (k, leading dimension of the row-major B and X)
ROW = 0


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    for name in list(SINGLE.values()) + list(BLOCK.values()):
        a.set_variant(name, 16)
    a.spmvHipFinalize()


@pytest.fixture(scope="module")
def problem(api):
    """the matrix, the three dM with the launches of one M^-1, and b"""
    A = laplacian7(*GRID)
    da, ilu = _up(api, A), _up(api, A)
    ilu.ilu0()
    for lower in (True, False):                         # (a solve would analyse the upper triangle at its first use)
        ilu.triangular_analyse(lower)
    h = da.amg()
    h.set_block_width(17)
    c_ilu = ilu.triangular_info(True).launches + ilu.triangular_info(False).launches
    assert c_ilu > 0 and h.info.levels >= 2
    b = np.random.default_rng(17).standard_normal(A[0])
    yield da, {"none": (None, 0), "ilu": (ilu, c_ilu), "amg": (h, cycle_launches(1, 1, 8, h.info.levels))}, b
    h.free()
    ilu.free()
    da.free()


def launches(method, n, pre, c):
    if method == "cg":
        return 4 + 6 * n + ((n + 1) * (c + 2) if pre else 0)
    return 3 + n * (11 + 2 * c)


def single_rule(method, maxiter, K, jstar, pre, c):
    """(launches, hostChecks) of a single solve"""
    if maxiter == 0:
        return launches(method, 0, pre, c), 0
    checks = max(1, -(-jstar // K))
    return launches(method, min(maxiter, K * checks), pre, c), checks


def block_rule(method, maxiter, K, jstar, pre, c):
    """(launches, hostChecks) of a block solve whose last column stopped in iteration jstar"""
    if jstar == 0:
        return 3, 1
    batches = -(-jstar // K)
    return launches(method, min(maxiter, K * batches), pre, c), 1 + batches


def block_solve(api, method, da, dm, Bh, ld, maxiter):
    """the C call on row-major device blocks with leading dimension ld, X from zeros: (info, columns, X)"""
    n, k = Bh.shape
    host = np.zeros((n, ld))
    host[:, :k] = Bh
    B = api.DeviceBuffer(host.nbytes).up(host)
    X = api.DeviceBuffer(host.nbytes).up(np.zeros((n, ld)))
    try:
        opts = api.spmvKrylovOpts(TOL, maxiter, None)
        info = api.spmvKrylovInfo()
        cols = (api.spmvKrylovColumn * k)()
        rc = getattr(api.lib, BLOCK[method])(C.byref(da.handle), C.byref(dm.handle) if dm is not None else None, k, B.ptr, ld, ROW,
                                             X.ptr, ld, ROW, C.byref(opts), cols, C.byref(info))
        assert rc == 0
        return info, cols, X.down(np.float64).reshape(n, ld)[:, :k]
    finally:
        B.free()
        X.free()


@pytest.mark.parametrize("precond", ["none", "ilu", "amg"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_counters(api, problem, method, precond):
    da, dms, b = problem
    dm, c = dms[precond]
    pre = dm is not None
    _, full = getattr(da, method)(b, precond=dm, tol=TOL, maxiter=CAP)
    conv = int(full.iterations)
    assert full.status == CONVERGED and 2 < conv < CAP and conv % 16, "the stop falls inside a batch of 16"
    # the exits: (b, maxIter, status, iterations) -- the stop is set in the kernels of iteration `iterations`
    exits = {"maxIter = 0": (b, 0, MAXITER, 0), "b = 0": (np.zeros_like(b), CAP, CONVERGED, 0),
             "converges inside a batch": (b, CAP, CONVERGED, conv), "maxiter below the count": (b, conv - 2, MAXITER, conv - 2)}
    for K in (1, 16):
        api.set_variant(SINGLE[method], K)
        api.set_variant(BLOCK[method], K)
        for name, (rhs, maxiter, status, its) in exits.items():
            what = f"{method}, dM {precond}, K = {K}, {name}"
            x, info = getattr(da, method)(rhs, precond=dm, tol=TOL, maxiter=maxiter)
            got = (info.status, info.iterations, info.launches, info.hostChecks)
            want = (status, its) + single_rule(method, maxiter, K, its, pre, c)
            print(what, "single", got, want)
            assert got == want, (what, got, want)
            for k, ld in WIDTHS:
                # column 0 is the single solve's; column 1 stops at the init; the others are column 0 times a power of two
                Bh = np.stack([rhs * 2.0 ** (-(col // 2)) if col != 1 else np.zeros_like(rhs) for col in range(k)], axis=1)
                binfo, cols, X = block_solve(api, method, da, dm, Bh, ld, maxiter)
                got = (binfo.status, binfo.iterations, binfo.launches, binfo.hostChecks)
                want = (status, its) + block_rule(method, maxiter, K, its, pre, c)
                print(what, f"k = {k}", got, want)
                assert got == want, (what, k, got, want)
                for col in range(k):
                    assert (cols[col].status, cols[col].iterations) == ((CONVERGED, 0) if col == 1 else (status, its)), (what, k, col)
                assert_same_bits(X[:, 0], x, f"{what}, k = {k}: column 0 against the single solve")
