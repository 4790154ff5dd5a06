"""hipSpLanczosCSR on the device against the numpy loop of tests/lanczos_ref.py, bit for bit: theta, res, X, status, found,
iterations, cycles and hostChecks on every case of the exit table (tests/lanczos_exit_inputs.py) with poisoned outputs
intact beyond `found`; the odd-sized Laplacian with v0 and X at element offset 1 and ldx = n + 3 at the smallest basis,
at both ends of the spectrum and at the widest rotation; keep at both bounds; a unit-value handle; a value update; the
refusals; and DeviceMatrix.eigsh with numpy and torch inputs."""
import ctypes as C

import numpy as np
import pytest

import lanczos_exit_inputs as exits
import lanczos_ref as lr
from krylov_ref import CONVERGED, MAXITER, NONFINITE, Csr
from test_gpu_trsv import POISON, _carved, _outside_intact, same
from test_trsv_abi import laplacian7

pytestmark = pytest.mark.gpu

ODD_GRID = (21, 19, 17)                 # n = 6 783: odd, one dot block of 4 096 plus a short one


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


def _torch():
    return pytest.importorskip("torch")


def _poisoned(n):
    return np.full(n, POISON, dtype=np.uint64).view(np.float64)


def _raw(api, A, v0_ptr, x_ptr, ldx, nev, ncv, which, tol, maxiter, keep=0):
    theta, res = _poisoned(max(nev, 1) + 1), _poisoned(max(nev, 1) + 1)
    opts = api.spmvLanczosOpts(int(nev), int(ncv), int(which), float(tol), int(maxiter), int(keep))
    info = api.spmvLanczosInfo()
    C.memset(C.addressof(info), 0xA5, C.sizeof(info))
    rc = api.lib.hipSpLanczosCSR(C.byref(A.handle) if A is not None else None, v0_ptr, C.byref(opts), x_ptr, ldx,
                                 theta.ctypes.data, res.ctypes.data, C.byref(info))
    return rc, info, theta, res


def _ref(M, IRP, JA, AS, v0, nev, ncv, which, tol, maxiter, keep=0):
    stats = {}
    out = lr.lanczos_ref(Csr(M, IRP, JA, AS), v0, nev, ncv, which, tol, maxiter, keep, None, stats)
    return out, stats


def _launches(ncv, kk, maxiter, steps, rotations):
    """3 before the first cycle; 9 per ENQUEUED step (a cycle enqueues min(ncv - k, maxIter - it) of them, and a step after
    beta == 0 or a value that is not finite still counts: it returns at once); one rotation per cycle that reaches one"""
    total, it = 3 + rotations, 0
    for i, done in enumerate(steps):
        total += 9 * min(ncv - (kk if i else 0), maxiter - it)
        it += done
    return total


def _check(info, theta, res, xbuf, ldx, off, n, opts, ref, stats, what):
    """xbuf: the whole poisoned host copy of the buffer that holds X at element offset `off`; opts: (nev, ncv, maxiter, keep)"""
    nev, ncv, maxiter, keep = opts
    rtheta, rres, rX, st, found, it, cyc = ref
    assert (info.status, info.found, info.iterations, info.cycles, info.hostChecks) == (st, found, it, cyc, cyc), \
        (what, info.status, info.found, info.iterations, info.cycles, info.hostChecks, ref[3:])
    same(theta[:found], rtheta, what + ": theta")
    same(res[:found], rres, what + ": res")
    assert (theta[found:].view(np.uint64) == POISON).all() and (res[found:].view(np.uint64) == POISON).all(), what + ": written past found"
    mask = np.ones(xbuf.size, bool)
    for i in range(found):
        same(xbuf[off + i * ldx:off + i * ldx + n], rX[:, i], what + f": X[:, {i}]")
        mask[off + i * ldx:off + i * ldx + n] = False
    assert (xbuf.view(np.uint64)[mask] == POISON).all(), what + ": X written outside its first `found` columns"
    if cyc:
        same(np.array([info.scale]), np.array([stats["scale"]]), what + ": scale")
        assert info.sweepsMax == stats["sweeps"], (what, info.sweepsMax, stats["sweeps"])
        rotations = cyc - (1 if st == NONFINITE else 0)
        assert info.launches == _launches(ncv, keep or lr.default_keep(nev, ncv), maxiter, stats["steps"], rotations), (what, info.launches)
    else:
        assert info.launches == 3 and info.sweepsMax == 0


def _solve(api, torch, A, M, v0, nev, ncv, which, tol, maxiter, keep, ref, stats, what, off=0, pad=0):
    ldx = M + pad
    bigv, dv = _carved(torch, v0, off)
    xhost = _poisoned(off + nev * ldx + 3)
    dx = torch.from_numpy(xhost).cuda()
    rc, info, theta, res = _raw(api, A, dv.data_ptr(), dx.data_ptr() + 8 * off, ldx, nev, ncv, which, tol, maxiter, keep)
    assert rc == 0, what
    _check(info, theta, res, dx.cpu().numpy(), ldx, off, M, (nev, ncv, maxiter, keep), ref, stats, what)
    _outside_intact(bigv, off, M, what + " (v0)")
    same(dv.cpu().numpy(), v0, what + ": v0 is read only")
    return info


@pytest.mark.parametrize("name", exits.NAMES)
def test_every_exit(api, name):
    torch = _torch()
    c = exits.case(name)
    ref, stats = _ref(c.M, c.IRP, c.JA, c.AS, c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep)
    assert (ref[3], ref[4]) == (c.status, c.found)
    A = api.spMatCpyCSR(api.HostCSR(c.M, c.M, c.IRP, c.JA, c.AS))
    try:
        if name == "2I":
            v = C.c_double(0)
            assert api.lib.spmvHipUnitValue(C.byref(A.handle), C.byref(v)) == 1 and v.value == 2.0
        for off, pad in ((0, 0), (1, 1)):
            _solve(api, torch, A, c.M, c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep, ref, stats, f"{name} offset {off}", off, pad)
    finally:
        A.free()


@pytest.fixture(scope="module")
def odd():
    IRP, JA, AS = laplacian7(*ODD_GRID)
    M = int(np.prod(ODD_GRID))
    return M, IRP, JA, AS, np.random.default_rng(0).standard_normal(M)


# (nev, ncv, which, maxiter, keep): the smallest legal basis (capped: it needs thousands of steps), (4, 20) at both ends
# to convergence, the widest rotation, and keep at both of its bounds
ODD_CASES = [(1, 2, lr.LARGEST, 40, 0), (4, 20, lr.LARGEST, 2000, 0), (4, 20, lr.SMALLEST, 2000, 0), (8, 64, lr.LARGEST, 2000, 0),
             (4, 20, lr.LARGEST, 60, 4), (4, 20, lr.SMALLEST, 60, 19)]


@pytest.mark.parametrize("nev,ncv,which,maxiter,keep", ODD_CASES)
def test_odd_laplacian_at_odd_offsets(api, odd, nev, ncv, which, maxiter, keep):
    """v0 and X views at element offset 1 (8-byte aligned only), ldx = n + 3: the scalar forms of the passes on them and
    of the final rotation; nothing outside the views is touched"""
    torch = _torch()
    M, IRP, JA, AS, v0 = odd
    ref, stats = _ref(M, IRP, JA, AS, v0, nev, ncv, which, 1e-8, maxiter, keep)
    assert ref[3] == (CONVERGED if maxiter == 2000 else MAXITER)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    try:
        what = f"nev={nev} ncv={ncv} which={which} keep={keep}"
        info = _solve(api, torch, A, M, v0, nev, ncv, which, 1e-8, maxiter, keep, ref, stats, what, off=1, pad=3)
        print(f"{what}: status {info.status}, {info.iterations} matvecs, {info.cycles} cycles, {info.sweepsMax} sweeps, {info.ms:.1f} ms")
    finally:
        A.free()


def test_unit_value_handle_and_update_values(api):
    """a pattern handle (every stored value 1.0: the unit kernels inside the loop), then new values and a second call"""
    torch = _torch()
    IRP, JA, AS = laplacian7(10, 9, 8)
    M = 720
    ones = np.ones_like(AS)
    v0 = np.random.default_rng(8500).standard_normal(M)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, ones))
    try:
        v = C.c_double(0)
        assert api.lib.spmvHipUnitValue(C.byref(A.handle), C.byref(v)) == 1 and v.value == 1.0
        ref, stats = _ref(M, IRP, JA, ones, v0, 3, 12, lr.LARGEST, 1e-8, 300)
        _solve(api, torch, A, M, v0, 3, 12, lr.LARGEST, 1e-8, 300, 0, ref, stats, "unit values")
        A.update_values(AS)
        ref2, stats2 = _ref(M, IRP, JA, AS, v0, 3, 12, lr.LARGEST, 1e-8, 300)
        _solve(api, torch, A, M, v0, 3, 12, lr.LARGEST, 1e-8, 300, 0, ref2, stats2, "after spmvHipUpdateValues")
        assert not np.array_equal(ref[0], ref2[0])
    finally:
        A.free()


def test_python_numpy_and_torch(api):
    torch = _torch()
    IRP, JA, AS = laplacian7(12, 10, 8)
    M = 960
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    try:
        v0 = np.random.default_rng(0).standard_normal(M)
        for which, code in (("LA", lr.LARGEST), ("SA", lr.SMALLEST)):
            ref, stats = _ref(M, IRP, JA, AS, v0, 4, 20, code, 1e-8, 10 * M)
            theta, X, info = A.eigsh(k=4, which=which)                   # ncv = max(2k + 1, 20) = 20, v0 = default_rng(0)
            assert (info.status, info.found, info.iterations, info.cycles) == (CONVERGED,) + ref[4:]
            same(theta, ref[0], which + ": theta")
            same(info.res, ref[1], which + ": res")
            same(X, ref[2], which + ": X")
            th, Xt, info_t = A.eigsh(k=4, which=which, v0=torch.from_numpy(v0).cuda(), ncv=20)
            assert Xt.is_cuda and Xt.shape == (M, 4)
            same(th, ref[0], which + ": theta (torch)")
            same(Xt.cpu().numpy(), ref[2], which + ": X (torch)")
            true = np.linalg.norm(Csr(M, IRP, JA, AS).spmv(X[:, 0]) - theta[0] * X[:, 0])
            assert true <= 1e-8 * info.scale + 1e-13
        ref6, _ = _ref(M, IRP, JA, AS, v0, 6, 20, lr.LARGEST, 1e-8, 10 * M)
        theta6, X6, info6 = A.eigsh()                                    # k = 6
        same(theta6, ref6[0], "defaults: theta")
        with pytest.raises(api.SpmvHipError):
            A.eigsh(which="LM")
    finally:
        A.free()


def test_refusals_leave_the_outputs_untouched(api, capfd):
    torch = _torch()
    n = 6
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    rect = api.spMatCpyCSR(api.HostCSR(M, M + 1, IRP, JA, AS))
    ell = api.spMatCpyELL(api.HostCSR(M, M, IRP, JA, AS).to_ell())
    dead = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    dead.free()
    v0 = torch.ones(M, dtype=torch.float64).cuda()
    x = torch.full((4 * M,), 3.25, dtype=torch.float64).cuda()
    V, X = v0.data_ptr(), x.data_ptr()
    try:
        # (handle, v0, X, ldx, nev, ncv, which, tol, keep)
        cases = [
            (None, V, X, M, 2, 8, 0, 1e-8, 0), (dead, V, X, M, 2, 8, 0, 1e-8, 0), (ell, V, X, M, 2, 8, 0, 1e-8, 0), (rect, V, X, M, 2, 8, 0, 1e-8, 0),
            (A, None, X, M, 2, 8, 0, 1e-8, 0), (A, V, None, M, 2, 8, 0, 1e-8, 0),
            (A, V, X, M, 0, 8, 0, 1e-8, 0), (A, V, X, M, 8, 8, 0, 1e-8, 0), (A, V, X, M, 2, 65, 0, 1e-8, 0),
            (A, V, X, M, 2, 8, 2, 1e-8, 0), (A, V, X, M, 2, 8, -1, 1e-8, 0),
            (A, V, X, M, 2, 8, 0, -1.0, 0), (A, V, X, M, 2, 8, 0, float("nan"), 0),
            (A, V, X, M, 2, 8, 0, 1e-8, 1), (A, V, X, M, 2, 8, 0, 1e-8, 8),
            (A, V, X, M - 1, 2, 8, 0, 1e-8, 0),
            (A, X + 8 * (M + 3), X, M, 2, 8, 0, 1e-8, 0), (A, X, X, M, 2, 8, 0, 1e-8, 0),
        ]
        for i, (dA, vp, xp, ldx, nev, ncv, which, tol, keep) in enumerate(cases):
            rc, info, theta, res = _raw(api, dA, vp, xp, ldx, nev, ncv, which, tol, 50, keep)
            assert rc == 1, i
            assert torch.all(x == 3.25).item(), i
            assert (theta.view(np.uint64) == POISON).all() and (res.view(np.uint64) == POISON).all(), i
            assert C.string_at(C.addressof(info), C.sizeof(info)) == b"\xa5" * C.sizeof(info), i
        tiny = api.spMatCpyCSR(api.HostCSR(3, 3, np.arange(4, dtype=np.uint64), np.arange(3, dtype=np.uint64), np.ones(3)))
        try:
            rc, _, _, _ = _raw(api, tiny, V, X, 3, 1, 4, 0, 1e-8, 50)    # ncv > M
            assert rc == 1
        finally:
            tiny.free()
        opts = api.spmvLanczosOpts(2, 8, 0, 1e-8, 50, 0)
        th = np.zeros(2)
        assert api.lib.hipSpLanczosCSR(C.byref(A.handle), V, None, X, M, th.ctypes.data, th.ctypes.data, None) == 1
        assert api.lib.hipSpLanczosCSR(C.byref(A.handle), V, C.byref(opts), X, M, None, th.ctypes.data, None) == 1
        assert api.lib.hipSpLanczosCSR(C.byref(A.handle), V, C.byref(opts), X, M, th.ctypes.data, None, None) == 1
        assert torch.all(x == 3.25).item()
        assert "hipSpLanczosCSR" in capfd.readouterr().err
        assert api.lib.hipSpLanczosCSR(C.byref(A.handle), V, C.byref(opts), X, M, th.ctypes.data, th.ctypes.data + 0, None) == 0   # info may be NULL
    finally:
        for m in (A, rect, ell):
            m.free()
