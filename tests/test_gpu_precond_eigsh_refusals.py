"""Every device allocation of hipSpDavidsonCSR refused in turn (spmvHipAllocRefuse), without a dM and with one, with restarts
in the solve -- by the method of tests/test_gpu_lanczos_refusals.py.

The call runs unarmed twice (the first chooses the handle's SpMV kernel and analyses the dM's triangles, which may allocate
on their own; the second counts N, the allocations of the solve itself: v, w, R, with a dM t, the partials, theta and S, the
state).  Then, for every n in [0, N), once with that allocation alone refused and once with every allocation from it on:

  1 refusal     refused >= 1, EXIT_FAILURE, a "libspmvhip" line on stderr
  2 ledger      no bad release; the library holds what it held before the call
  3 outputs     theta, res, X and a patterned info still hold their patterns
  4 no sticky   spmvHipVecFill on a scratch vector and a download succeed and show the fill
  5 retry       the same call, unarmed, succeeds with the reference's bits"""
import ctypes as C

import numpy as np
import pytest

import davidson_ref as dr
import lanczos_ref as lr
from ilu0_ref import ilu0_levels
from krylov_ref import CONVERGED, Csr
from test_gpu_trsv import same
from test_trsv_abi import laplacian7

pytestmark = pytest.mark.gpu

NAME = "hipSpDavidsonCSR"
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


@pytest.mark.parametrize("precond", [False, True], ids=["no_dM", "ilu0_dM"])
def test_every_allocation_refused_in_turn(api, capfd, precond):
    IRP, JA, AS = laplacian7(9, 8, 7)
    M, nev, ncv = 504, 2, 10
    v0 = np.random.default_rng(8600).standard_normal(M)
    host = Csr(M, IRP, JA, AS, ilu0_levels(M, IRP, JA, AS) if precond else None)
    rtheta, rres, rX, st, found, it, restarts = dr.davidson_ref(host, v0, nev, ncv, lr.SMALLEST, 1e-8, 300, precond=host.precond if precond else None)
    assert st == CONVERGED and found == nev and restarts >= 1
    dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    pm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    pm.ilu0()
    dv, dx, scratch = api.DeviceVector(M), api.DeviceVector(nev * M), api.DeviceVector(64)
    dv.up(v0)
    opts = api.spmvDavidsonOpts(nev, ncv, lr.SMALLEST, 1e-8, 300, 0)

    def call(info):
        theta, res = _poisoned(nev), _poisoned(nev)
        dx.up(_poisoned(nev * M))
        rc = api.lib.hipSpDavidsonCSR(C.byref(dm.handle), C.byref(pm.handle) if precond else None, dv.ptr, C.byref(opts), dx.ptr, M,
                                      theta.ctypes.data, res.ctypes.data, C.byref(info))
        return rc, theta, res

    def is_reference(info, theta, res, what):
        assert (info.status, info.found, info.iterations, info.restarts) == (st, found, it, restarts), what
        same(theta, rtheta, what + ": theta")
        same(res, rres, what + ": res")
        same(dx.down().reshape(nev, M).T, rX, what + ": X")

    try:
        info = api.spmvDavidsonInfo()
        assert call(info)[0] == 0                                    # (the handle's first SpMV chooses its kernel; dM is analysed)
        level = _level(api)
        api.alloc_refuse(-1)
        rc, theta, res = call(info)
        total = int(api.alloc_stats().calls)
        assert rc == 0 and total == (7 if precond else 6) and _level(api) == level, "v, w, R, (t,) the partials, theta and S, the state"
        is_reference(info, theta, res, "unarmed")
        print(f"{NAME} precond={precond}: {total} allocations, {info.launches} launches, {info.hostChecks} read-backs")
        for n in range(total):
            for from_then_on in (False, True):
                what = f"allocation {n}" + (" and every later one" if from_then_on else "") + " refused"
                info = api.spmvDavidsonInfo()
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
        pm.free()
        dm.free()
