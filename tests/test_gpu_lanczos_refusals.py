"""Every device allocation of hipSpLanczosCSR refused in turn (spmvHipAllocRefuse), with and without a restart in the
solve -- by the method of tests/test_gpu_rcm_refusals.py.

The call runs unarmed twice (the first chooses the handle's SpMV kernel, which may allocate on its own; the second counts
N, the allocations of the solve itself: the basis, w, the partials, S and the state).  Then, for every n in [0, N), once
with that allocation alone refused and once with every allocation from it on:

  1 refusal     refused >= 1, EXIT_FAILURE, a "libspmvhip" line on stderr
  2 ledger      no bad release; the library holds what it held before the call
  3 outputs     theta, res, X and a patterned info still hold their patterns
  4 no sticky   spmvHipVecFill on a scratch vector and a download succeed and show the fill
  5 retry       the same call, unarmed, succeeds with the reference's bits"""
import ctypes as C

import numpy as np
import pytest

import lanczos_ref as lr
from krylov_ref import Csr
from test_gpu_trsv import same
from test_trsv_abi import laplacian7

pytestmark = pytest.mark.gpu

NAME = "hipSpLanczosCSR"
PATTERN = 0xA5
FILL = 0x7FF8DEADBEEF0001
POISON = 0x7FF4DEADBEEF0001


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.alloc_refuse(-1)
    a.spmvHipInit(0)
    yield a
    a.alloc_refuse(-1)
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _disarm(api):
    yield
    api.alloc_refuse(-1)
    if api.lib.spmvHipDeviceSynchronize() != 0:                      # a device error is a finding: nothing more runs on it
        pytest.exit("the device reports an error after this case: the remaining cases are not run", returncode=3)


def _level(api):
    st = api.alloc_stats()
    return int(st.live), int(st.liveBytes)


def _poisoned(n):
    return np.full(n, POISON, dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("maxiter", [9, 300], ids=["one_cycle", "restarts"])
def test_every_allocation_refused_in_turn(api, capfd, maxiter):
    IRP, JA, AS = laplacian7(9, 8, 7)
    M, nev, ncv = 504, 2, 10
    v0 = np.random.default_rng(8600).standard_normal(M)
    rtheta, rres, rX, st, found, it, cyc = lr.lanczos_ref(Csr(M, IRP, JA, AS), v0, nev, ncv, lr.SMALLEST, 1e-8, maxiter)
    assert found == nev and (cyc == 1) == (maxiter == 9)
    dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    dv, dx, scratch = api.DeviceVector(M), api.DeviceVector(nev * M), api.DeviceVector(64)
    dv.up(v0)
    opts = api.spmvLanczosOpts(nev, ncv, lr.SMALLEST, 1e-8, maxiter, 0)

    def call(info):
        theta, res = _poisoned(nev), _poisoned(nev)
        dx.up(_poisoned(nev * M))
        rc = api.lib.hipSpLanczosCSR(C.byref(dm.handle), dv.ptr, C.byref(opts), dx.ptr, M, theta.ctypes.data, res.ctypes.data, C.byref(info))
        return rc, theta, res

    def is_reference(info, theta, res, what):
        assert (info.status, info.found, info.iterations, info.cycles) == (st, found, it, cyc), what
        same(theta, rtheta, what + ": theta")
        same(res, rres, what + ": res")
        same(dx.down().reshape(nev, M).T, rX, what + ": X")

    try:
        info = api.spmvLanczosInfo()
        assert call(info)[0] == 0                                    # (the handle's first SpMV chooses its kernel)
        level = _level(api)
        api.alloc_refuse(-1)
        rc, theta, res = call(info)
        total = int(api.alloc_stats().calls)
        assert rc == 0 and total == 5 and _level(api) == level, "the basis, w, the partials, S, the state"
        is_reference(info, theta, res, "unarmed")
        print(f"{NAME} maxiter={maxiter}: {total} allocations, {info.launches} launches, {info.hostChecks} read-backs")
        for n in range(total):
            for from_then_on in (False, True):
                what = f"allocation {n}" + (" and every later one" if from_then_on else "") + " refused"
                info = api.spmvLanczosInfo()
                C.memset(C.addressof(info), PATTERN, C.sizeof(info))
                capfd.readouterr()
                with api.alloc_refused(n, from_then_on):
                    rc, theta, res = call(info)
                    stats = api.alloc_stats()
                err = capfd.readouterr().err
                assert stats.refused >= 1 and rc == 1 and "libspmvhip" in err and NAME in err, (what, rc, err)
                assert stats.badFrees == 0 and _level(api) == level, f"{what}: nothing the call allocated is still held"
                assert C.string_at(C.addressof(info), C.sizeof(info)) == bytes([PATTERN]) * C.sizeof(info), f"{what}: info is not written"
                assert (theta.view(np.uint64) == POISON).all() and (res.view(np.uint64) == POISON).all(), f"{what}: theta, res"
                assert (dx.down().view(np.uint64) == POISON).all(), f"{what}: X is not written"
                assert api.lib.spmvHipVecFill(scratch.ptr, scratch.n, FILL) == 0, f"{what}: the next, unrelated call is judged on its own"
                assert np.all(scratch.down().view(np.uint64) == FILL)
                rc, theta, res = call(info)
                assert rc == 0, f"{what}: the same call made again succeeds"
                is_reference(info, theta, res, what + ": retry")
                assert _level(api) == level
    finally:
        for b in (scratch, dx, dv):
            b.free()
        dm.free()
