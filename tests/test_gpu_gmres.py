"""hipSpGMRESCSR on the device against the numpy loop of tests/gmres_ref.py, bit for bit: every case of the exit table
(tests/gmres_exit_inputs.py) with a poisoned history, the number of cycles, the plain and the fused update, an odd-sized
convection-diffusion system with b and x at odd element offsets without and with ILU(0) and with dM == dA, a unit-value
handle, the refusals, a value update, and DeviceMatrix.gmres with numpy and torch inputs."""
import ctypes as C

import numpy as np
import pytest

import gmres_exit_inputs as exits
import serial_order_inputs as si
from gmres_ref import gmres_ref
from ilu0_ref import ilu0_levels
from krylov_ref import CONVERGED, Csr, dot_ref
from test_gpu_trsv import POISON, _carved, _outside_intact, same
from test_krylov_abi import convdiff7
from test_trsv_abi import laplacian7

pytestmark = pytest.mark.gpu

ODD_GRID = (21, 19, 17)                 # n = 6 783: odd, one block of 4 096 plus a short one


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.lib.spmvHipSetVariant(b"hipSpGMRESCSR", 0)


def _torch():
    return pytest.importorskip("torch")


def _poisoned(n):
    return np.full(n, POISON, dtype=np.uint64).view(np.float64)


def _raw(api, A, P, b_ptr, x_ptr, tol, maxiter, restart):
    hist = _poisoned(maxiter + 1)
    opts = api.spmvGmresOpts(float(tol), int(maxiter), int(restart), hist.ctypes.data_as(C.POINTER(C.c_double)))
    info = api.spmvKrylovInfo()
    rc = api.lib.hipSpGMRESCSR(C.byref(A.handle) if A is not None else None, C.byref(P.handle) if P is not None else None,
                               b_ptr, x_ptr, C.byref(opts), C.byref(info))
    return rc, info, hist


def _check_raw(info, hist, x, ref, cycles, what):
    rx, st, it, rhist, rr = ref
    assert (info.status, info.iterations) == (st, it), (what, info.status, info.iterations, st, it)
    same(x, rx, what + ": x")
    same(hist[:it + 1], rhist, what + ": history")
    assert (hist[it + 1:].view(np.uint64) == POISON).all(), what + ": history written past `iterations`"
    same(np.array([info.rr]), np.array([rr]), what + ": rr")
    assert info.hostChecks == cycles, (what, info.hostChecks, cycles)


def _ref(M, IRP, JA, AS, F, b, x0, tol, maxiter, restart):
    stats = {}
    with np.errstate(all="ignore"):
        out = gmres_ref(Csr(M, IRP, JA, AS, F), b, x0, tol, maxiter, restart, None, stats)
    return out, stats["cycles"]


@pytest.mark.parametrize("name", exits.NAMES)
def test_every_exit(api, name):
    torch = _torch()
    c = exits.case(name)
    with np.errstate(all="ignore"):
        F = ilu0_levels(c.M, c.IRP, c.JA, c.AS) if c.precond else None
    ref, cycles = _ref(c.M, c.IRP, c.JA, c.AS, F, c.b, c.x0, c.tol, c.maxiter, c.restart)
    assert cycles == c.cycles
    A = api.spMatCpyCSR(api.HostCSR(c.M, c.M, c.IRP, c.JA, c.AS))
    P = None
    db = torch.from_numpy(c.b).cuda()
    try:
        if c.precond:
            P = api.spMatCpyCSR(api.HostCSR(c.M, c.M, c.IRP, c.JA, c.AS))
            P.ilu0()
        if name.endswith(":2I"):
            v = C.c_double(0)
            assert api.lib.spmvHipUnitValue(C.byref(A.handle), C.byref(v)) == 1 and v.value == 2.0
        for fused in (0, 1):
            assert api.lib.spmvHipSetVariant(b"hipSpGMRESCSR", fused) == 0
            dx = torch.from_numpy(c.x0).cuda()
            rc, info, hist = _raw(api, A, P, db.data_ptr(), dx.data_ptr(), c.tol, c.maxiter, c.restart)
            assert rc == 0
            _check_raw(info, hist, dx.cpu().numpy(), ref, cycles, f"{name} fused={fused}")
            same(np.array([info.bb]), np.array([dot_ref(c.b, c.b)]), name + ": bb")
    finally:
        A.free()
        if P is not None:
            P.free()


@pytest.mark.parametrize("precond", ["none", "ilu0", "self"])
def test_convection_diffusion_odd_offsets(api, precond):
    """n = 21 * 19 * 17 upwind convection-diffusion, restart 1, 3 and 30; b and x views at element offset 1 (the scalar
    forms of the passes on them and of the first SpMV); nothing outside the views is touched"""
    torch = _torch()
    IRP, JA, AS0 = convdiff7(*ODD_GRID)
    M = int(np.prod(ODD_GRID))
    rng = np.random.default_rng(8100)
    b, x0 = rng.random(M), rng.uniform(-1, 1, M)
    AS = AS0
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P = F = None
    try:
        if precond == "ilu0":
            P = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
            P.ilu0()
            F = ilu0_levels(M, IRP, JA, AS)
        elif precond == "self":                                          # A holds its own ILU(0) factors: matrix and dM at once
            A.ilu0()
            AS = F = ilu0_levels(M, IRP, JA, AS0)
            P = A
        for restart, maxiter in ((1, 12), (3, 20), (30, 45)):
            ref, cycles = _ref(M, IRP, JA, AS, F, b, x0, 1e-10, maxiter, restart)
            for fused in (0, 1):
                assert api.lib.spmvHipSetVariant(b"hipSpGMRESCSR", fused) == 0
                what = f"precond={precond} restart={restart} fused={fused}"
                bigb, vb = _carved(torch, b, 1)
                bigx, vx = _carved(torch, x0, 1)
                assert vb.data_ptr() % 16 == 8 and vx.data_ptr() % 16 == 8
                rc, info, hist = _raw(api, A, P, vb.data_ptr(), vx.data_ptr(), 1e-10, maxiter, restart)
                assert rc == 0
                _check_raw(info, hist, vx.cpu().numpy(), ref, cycles, what)
                _outside_intact(bigb, 1, M, what + " (b)")
                _outside_intact(bigx, 1, M, what + " (x)")
                same(vb.cpu().numpy(), b, what + ": b is read only")
    finally:
        A.free()
        if P is not None and P is not A:
            P.free()


def test_python_numpy_and_torch_and_update_values(api):
    torch = _torch()
    n = 12
    IRP, JA, AS = convdiff7(n, n, n)
    M = n ** 3
    rng = np.random.default_rng(8200)
    b = rng.random(M)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    try:
        ref, cycles = _ref(M, IRP, JA, AS, None, b, np.zeros(M), 1e-9, 300, 10)
        x, info = A.gmres(b, tol=1e-9, maxiter=300, restart=10, history=True)
        assert info.status == CONVERGED == ref[1] and info.iterations == ref[2] and info.hostChecks == cycles and info.launches > 0
        same(x, ref[0], "numpy: x")
        same(info.history, ref[3], "numpy: history")
        xt, info_t = A.gmres(torch.from_numpy(b).cuda(), tol=1e-9, maxiter=300, restart=10)
        assert xt.is_cuda
        same(xt.cpu().numpy(), ref[0], "torch: x")
        res = b - Csr(M, IRP, JA, AS).spmv(x)
        assert np.linalg.norm(res) <= 1.01e-9 * np.linalg.norm(b)
        AS2 = np.where(AS > 0, AS + rng.random(AS.size), AS)             # new values: the next solve uses them
        A.update_values(AS2)
        ref2, _ = _ref(M, IRP, JA, AS2, None, b, x, 1e-9, 300, 30)
        x2, info2 = A.gmres(b, x0=x, tol=1e-9, maxiter=300, history=True)
        assert (info2.status, info2.iterations) == (ref2[1], ref2[2])
        same(x2, ref2[0], "after spmvHipUpdateValues: x")
        assert not np.array_equal(x2, x)
    finally:
        A.free()


def test_unit_value_handle(api):
    """every stored value 1.0 (a pattern handle): the unit kernels inside the solve"""
    n = 10
    IRP, JA, AS = convdiff7(n, n, n)
    M = n ** 3
    ones = np.ones_like(AS)
    b = np.random.default_rng(8300).random(M)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, ones))
    try:
        v = C.c_double(0)
        assert api.lib.spmvHipUnitValue(C.byref(A.handle), C.byref(v)) == 1 and v.value == 1.0
        ref, cycles = _ref(M, IRP, JA, ones, None, b, np.zeros(M), 1e-8, 25, 7)
        x, info = A.gmres(b, maxiter=25, restart=7, history=True)
        assert (info.status, info.iterations, info.hostChecks) == (ref[1], ref[2], cycles)
        same(x, ref[0], "x")
        same(info.history, ref[3], "history")
    finally:
        A.free()


def test_refusals_leave_x_untouched(api, capfd):
    torch = _torch()
    n = 6
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    rect = api.spMatCpyCSR(api.HostCSR(M, M + 1, IRP, JA, AS))
    ell = api.spMatCpyELL(api.HostCSR(M, M, IRP, JA, AS).to_ell())
    b = torch.from_numpy(np.random.default_rng(8400).random(M)).cuda()
    x = torch.full((M,), 3.25, dtype=torch.float64).cuda()
    big = torch.zeros(2 * M, dtype=torch.float64).cuda()
    try:
        cases = [
            (A, b.data_ptr(), x.data_ptr(), 1e-8, 0), (A, b.data_ptr(), x.data_ptr(), 1e-8, 65),
            (None, b.data_ptr(), x.data_ptr(), 1e-8, 30), (A, None, x.data_ptr(), 1e-8, 30), (A, b.data_ptr(), None, 1e-8, 30),
            (ell, b.data_ptr(), x.data_ptr(), 1e-8, 30), (rect, b.data_ptr(), x.data_ptr(), 1e-8, 30),
            (A, x.data_ptr(), x.data_ptr(), 1e-8, 30), (A, big.data_ptr(), big.data_ptr() + 8 * (M // 2), 1e-8, 30),
            (A, b.data_ptr(), x.data_ptr(), -1.0, 30), (A, b.data_ptr(), x.data_ptr(), float("nan"), 30),
        ]
        for i, (dA, bp, xp, tol, restart) in enumerate(cases):
            rc, _, hist = _raw(api, dA, None, bp, xp, tol, 10, restart)
            assert rc == 1, i
            assert torch.all(x == 3.25).item() and not big.any().item(), i
            assert (hist.view(np.uint64) == POISON).all(), i
        assert api.lib.hipSpGMRESCSR(C.byref(A.handle), None, b.data_ptr(), x.data_ptr(), None, None) == 1
        assert torch.all(x == 3.25).item()
        assert "hipSpGMRESCSR" in capfd.readouterr().err
    finally:
        for m in (A, rect, ell):
            m.free()


def test_M_zero(api):
    """M = 0 succeeds: CONVERGED, 0, hist[0] = +0.0, no read-back, x and its neighbours untouched"""
    torch = _torch()
    empty = (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    A = api.spMatCpyCSR(api.HostCSR(0, 0, *empty))
    big = torch.from_numpy(_poisoned(4)).cuda()
    try:
        rc, info, hist = _raw(api, A, None, big.data_ptr(), big.data_ptr() + 16, 1e-8, 5, 30)
        assert rc == 0 and (info.status, info.iterations, info.hostChecks) == (CONVERGED, 0, 0)
        assert hist[:1].view(np.uint64)[0] == 0 and (hist[1:].view(np.uint64) == POISON).all()
        assert (big.cpu().numpy().view(np.uint64) == POISON).all()
    finally:
        A.free()
