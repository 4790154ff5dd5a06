"""hipSpDavidsonCSR on the device against the numpy loop of tests/davidson_ref.py, bit for bit: theta, res, X, status, found,
iterations, restarts, precondApplies, hostChecks, launches, scale and sweepsMax on every case of the exit table
(tests/davidson_exit_inputs.py) with poisoned outputs intact beyond `found`; the odd-sized Laplacian with v0 and X at
element offset 1 and ldx = n + 3 at both ends of the spectrum, at the widest basis and at nev = 16; SMALLEST with each kind
of preconditioner once (ILU(0) by level sets and by sweeps, FSAI in both storages, a plain hierarchy, a smoothed one with
Chebyshev, one with Gauss-Seidel); a unit-value handle; a value update; DeviceMatrix.eigsh with numpy and torch inputs and
its unchanged default; the refusals."""
import ctypes as C

import numpy as np
import pytest

import davidson_exit_inputs as exits
import davidson_ref as dr
import lanczos_ref as lr
from krylov_ref import CONVERGED, MAXITER, Csr
from test_gpu_trsv import POISON, _carved, _outside_intact, same
from test_trsv_abi import laplacian7

pytestmark = pytest.mark.gpu

ODD_GRID = (21, 19, 17)                 # n = 6 783: odd, one dot block of 4 096 plus a short one
AMG_GRID = (12, 10, 8)                  # 960 rows: the grid of the multigrid tests' Krylov solves, three levels at coarseRows = 8


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


def _raw(api, A, dM, v0_ptr, x_ptr, ldx, nev, ncv, which, tol, maxiter, keep=0):
    theta, res = _poisoned(max(nev, 1) + 1), _poisoned(max(nev, 1) + 1)
    opts = api.spmvDavidsonOpts(int(nev), int(ncv), int(which), float(tol), int(maxiter), int(keep))
    info = api.spmvDavidsonInfo()
    C.memset(C.addressof(info), 0xA5, C.sizeof(info))
    rc = api.lib.hipSpDavidsonCSR(C.byref(A.handle) if A is not None else None, C.byref(dM.handle) if dM is not None else None, v0_ptr,
                                  C.byref(opts), x_ptr, ldx, theta.ctypes.data, res.ctypes.data, C.byref(info))
    return rc, info, theta, res


def _ref(A, v0, nev, ncv, which, tol, maxiter, keep=0, precond=None):
    stats = {}
    return dr.davidson_ref(A, v0, nev, ncv, which, tol, maxiter, keep, precond, None, stats), stats


def _apply_launches(api, A, dM):
    """the kernels one application of dM enqueues, from hipSpCGCSR's own count: one iteration enqueued is 4 + 6 launches of
    CG's and two applications, each followed by a dot pass and its finish (tests/test_gpu_fsai.py)"""
    if dM is None:
        return 0
    _, info = A.cg(np.ones(int(A.handle.N)), precond=dM, maxiter=1, tol=0.0)
    assert (info.launches - 10) % 2 == 0
    return (int(info.launches) - 10) // 2 - 2


def _check(info, theta, res, xbuf, ldx, off, n, ref, stats, apply_launches, what):
    """xbuf: the whole poisoned host copy of the buffer that holds X at element offset `off`"""
    rtheta, rres, rX, st, found, it, restarts = ref
    got = (info.status, info.found, info.iterations, info.restarts, info.precondApplies, info.hostChecks)
    assert got == (st, found, it, restarts, stats["applies"], stats["checks"]), (what, got, ref[3:], stats["applies"], stats["checks"])
    same(theta[:found], rtheta, what + ": theta")
    same(res[:found], rres, what + ": res")
    assert (theta[found:].view(np.uint64) == POISON).all() and (res[found:].view(np.uint64) == POISON).all(), what + ": written past found"
    mask = np.ones(xbuf.size, bool)
    for i in range(found):
        same(xbuf[off + i * ldx:off + i * ldx + n], rX[:, i], what + f": X[:, {i}]")
        mask[off + i * ldx:off + i * ldx + n] = False
    assert (xbuf.view(np.uint64)[mask] == POISON).all(), what + ": X written outside its first `found` columns"
    same(np.array([info.scale]), np.array([stats["scale"]]), what + ": scale")
    assert info.sweepsMax == stats["sweeps"], (what, info.sweepsMax, stats["sweeps"])
    assert info.launches == dr.launches(stats, apply_launches), (what, info.launches, dr.launches(stats, apply_launches), stats)


def _solve(api, torch, A, dM, M, v0, nev, ncv, which, tol, maxiter, keep, ref, stats, apply_launches, what, off=0, pad=0):
    ldx = M + pad
    bigv, dv = _carved(torch, v0, off)
    xhost = _poisoned(off + nev * ldx + 3)
    dx = torch.from_numpy(xhost).cuda()
    rc, info, theta, res = _raw(api, A, dM, dv.data_ptr(), dx.data_ptr() + 8 * off, ldx, nev, ncv, which, tol, maxiter, keep)
    assert rc == 0, what
    _check(info, theta, res, dx.cpu().numpy(), ldx, off, M, ref, stats, apply_launches, what)
    _outside_intact(bigv, off, M, what + " (v0)")
    same(dv.cpu().numpy(), v0, what + ": v0 is read only")
    return info


@pytest.mark.parametrize("name", exits.NAMES)
def test_every_exit(api, name):
    torch = _torch()
    c = exits.case(name)
    ref, stats = _ref(Csr(c.M, c.IRP, c.JA, c.AS), c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep, exits.precond_of(c))
    assert (ref[3], ref[4]) == (c.status, c.found)
    A = api.spMatCpyCSR(api.HostCSR(c.M, c.M, c.IRP, c.JA, c.AS))
    dM = None
    if c.dm is not None:                                                 # the diagonal M as a CSR handle: its triangles are applied
        i = np.arange(c.M, dtype=np.uint64)
        dM = api.spMatCpyCSR(api.HostCSR(c.M, c.M, np.arange(c.M + 1, dtype=np.uint64), i, c.dm))
    try:
        if name == "2I":
            v = C.c_double(0)
            assert api.lib.spmvHipUnitValue(C.byref(A.handle), C.byref(v)) == 1 and v.value == 2.0
        P = _apply_launches(api, A, dM)
        for off, pad in ((0, 0), (1, 1)):
            _solve(api, torch, A, dM, c.M, c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep, ref, stats, P, f"{name} offset {off}", off, pad)
    finally:
        if dM is not None:
            dM.free()
        A.free()


@pytest.fixture(scope="module")
def odd():
    IRP, JA, AS = laplacian7(*ODD_GRID)
    M = int(np.prod(ODD_GRID))
    return M, IRP, JA, AS, np.random.default_rng(0).standard_normal(M)


# (nev, ncv, which, maxiter): (4, 20) at both ends to convergence, the widest basis, and nev = 16 with the smallest basis
# that holds it (every step restarts; capped)
ODD_CASES = [(4, 20, lr.LARGEST, 2000), (4, 20, lr.SMALLEST, 2000), (8, 64, lr.LARGEST, 2000), (16, 17, lr.SMALLEST, 40)]


@pytest.mark.parametrize("nev,ncv,which,maxiter", ODD_CASES)
def test_odd_laplacian_at_odd_offsets(api, odd, nev, ncv, which, maxiter):
    """v0 and X views at element offset 1 (8-byte aligned only), ldx = n + 3: the scalar forms of the passes on them and
    of the final rotation; nothing outside the views is touched"""
    torch = _torch()
    M, IRP, JA, AS, v0 = odd
    ref, stats = _ref(Csr(M, IRP, JA, AS), v0, nev, ncv, which, 1e-8, maxiter)
    assert ref[3] == (CONVERGED if maxiter == 2000 else MAXITER)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    try:
        what = f"nev={nev} ncv={ncv} which={which}"
        info = _solve(api, torch, A, None, M, v0, nev, ncv, which, 1e-8, maxiter, 0, ref, stats, 0, what, off=1, pad=3)
        print(f"{what}: status {info.status}, {info.iterations} products, {info.restarts} restarts, {info.sweepsMax} sweeps, "
              f"{info.launches} launches, {info.ms:.1f} ms")
    finally:
        A.free()


# ------------------------------------------------------------------------------------------------- the preconditioners
def _ilu(api, A, da, sweeps):
    from ilu0_ref import ilu0_levels
    from sweeps_ref import SweepCsr
    M, _, IRP, JA, AS = A
    dM = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    dM.ilu0()
    F = ilu0_levels(M, IRP, JA, AS)
    if sweeps:
        dM.set_triangular_apply((sweeps, sweeps))
        return dM, SweepCsr(M, IRP, JA, AS, F, sweeps, sweeps)
    return dM, Csr(M, IRP, JA, AS, F)


def _fsai(api, A, da, storage):
    import fsai_ref as fr
    import values_f32_ref as vr
    G = fr.fsai_vec(A)[0]
    return da.fsai(storage=storage), fr.PrecondCsr(A, vr.rounded(G) if storage == "f32" else G)


def _plain(api, A, da):
    import amg_ref as ar
    return da.amg(coarseRows=8), ar.AmgCsr(A, coarseRows=8)


def _chebyshev(api, A, da):
    import amg_cheb_ref as cr
    h = da.amg(coarseRows=8, smoothed=True)
    h.set_smoother(nu1=2, nu2=2)
    return h, cr.ChebCsr(A, "smoothed", sm=dict(nu1=2, nu2=2), coarseRows=8)


def _gauss_seidel(api, A, da):
    import amg_gs_ref as gr
    h = da.amg(coarseRows=8)
    h.set_gauss_seidel(nu1=2, nu2=2)
    return h, gr.GsCsr(A, "plain", sm=dict(nu1=2, nu2=2), coarseRows=8)


PRECONDS = {"ilu0-levels": lambda *a: _ilu(*a, 0), "ilu0-sweeps": lambda *a: _ilu(*a, 3), "fsai-f64": lambda *a: _fsai(*a, "f64"),
            "fsai-f32": lambda *a: _fsai(*a, "f32"), "amg-plain": _plain, "amg-smoothed-chebyshev": _chebyshev,
            "amg-gauss-seidel": _gauss_seidel}


@pytest.fixture(scope="module")
def amg_problem(api):
    import spgemm_ref as sr
    A = sr.laplacian7(*AMG_GRID)
    M = A[0]
    v0 = np.random.default_rng(0).standard_normal(M)
    da = api.spMatCpyCSR(api.HostCSR(M, M, A[2], A[3], A[4]))
    plain, stats = _ref(Csr(M, A[2], A[3], A[4]), v0, 4, 20, lr.SMALLEST, 1e-8, 2000)
    yield A, v0, da, plain
    da.free()


@pytest.mark.parametrize("kind", list(PRECONDS))
def test_smallest_pairs_with_each_preconditioner(api, amg_problem, kind):
    torch = _torch()
    A, v0, da, plain = amg_problem
    M = A[0]
    dM, refA = PRECONDS[kind](api, A, da)
    try:
        ref, stats = _ref(refA, v0, 4, 20, lr.SMALLEST, 1e-8, 2000, precond=refA.precond)
        assert ref[3] == CONVERGED and stats["applies"] == stats["expansions"] > 0
        P = _apply_launches(api, da, dM)
        assert P > 0
        info = _solve(api, torch, da, dM, M, v0, 4, 20, lr.SMALLEST, 1e-8, 2000, 0, ref, stats, P, kind, off=1, pad=1)
        print(f"{kind}: {info.iterations} products ({plain[5]} without a dM), {info.precondApplies} applications of {P} launches, "
              f"{info.restarts} restarts, {info.ms:.1f} ms")
        assert np.abs(ref[0] - plain[0]).max() <= 1e-7 * stats["scale"], "the same eigenvalues as without a dM"
    finally:
        dM.free()


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
        ref, stats = _ref(Csr(M, IRP, JA, ones), v0, 3, 12, lr.LARGEST, 1e-8, 300)
        _solve(api, torch, A, None, M, v0, 3, 12, lr.LARGEST, 1e-8, 300, 0, ref, stats, 0, "unit values")
        A.update_values(AS)
        ref2, stats2 = _ref(Csr(M, IRP, JA, AS), v0, 3, 12, lr.LARGEST, 1e-8, 300)
        _solve(api, torch, A, None, M, v0, 3, 12, lr.LARGEST, 1e-8, 300, 0, ref2, stats2, 0, "after spmvHipUpdateValues")
        assert not np.array_equal(ref[0], ref2[0])
    finally:
        A.free()


def test_python_numpy_and_torch_and_the_default_is_lanczos(api):
    torch = _torch()
    IRP, JA, AS = laplacian7(12, 10, 8)
    M = 960
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    dM = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    try:
        v0 = np.random.default_rng(0).standard_normal(M)
        host = Csr(M, IRP, JA, AS)
        for which, code in (("LA", lr.LARGEST), ("SA", lr.SMALLEST)):
            ref, stats = _ref(host, v0, 4, 20, code, 1e-8, 10 * M)
            theta, X, info = A.eigsh(k=4, which=which, method="davidson")    # ncv = max(2k + 1, 20) = 20, v0 = default_rng(0)
            assert isinstance(info, api.spmvDavidsonInfo)
            assert (info.status, info.found, info.iterations, info.restarts) == (CONVERGED,) + ref[4:]
            same(theta, ref[0], which + ": theta")
            same(info.res, ref[1], which + ": res")
            same(X, ref[2], which + ": X")
            th, Xt, info_t = A.eigsh(k=4, which=which, v0=torch.from_numpy(v0).cuda(), ncv=20, method="davidson")
            assert Xt.is_cuda and Xt.shape == (M, 4)
            same(th, ref[0], which + ": theta (torch)")
            same(Xt.cpu().numpy(), ref[2], which + ": X (torch)")
            true = np.linalg.norm(host.spmv(X[:, 0]) - theta[0] * X[:, 0])
            assert abs(true - info.res[0]) <= 1e-13 and true <= 1e-8 * info.scale + 1e-13
        # with a preconditioner
        from ilu0_ref import ilu0_levels
        dM.ilu0()
        pre = Csr(M, IRP, JA, AS, ilu0_levels(M, IRP, JA, AS))
        ref, stats = _ref(pre, v0, 4, 20, lr.SMALLEST, 1e-8, 10 * M, precond=pre.precond)
        theta, X, info = A.eigsh(k=4, which="SA", method="davidson", precond=dM)
        assert (info.status, info.iterations, info.precondApplies) == (CONVERGED, ref[5], stats["applies"])
        same(theta, ref[0], "ILU(0): theta")
        same(X, ref[2], "ILU(0): X")
        # the default is today's Lanczos, bit for bit
        lref = lr.lanczos_ref(host, v0, 6, 20, lr.LARGEST, 1e-8, 10 * M)
        theta6, X6, info6 = A.eigsh()
        assert isinstance(info6, api.spmvLanczosInfo) and (info6.iterations, info6.cycles) == lref[5:]
        same(theta6, lref[0], "defaults: theta")
        same(X6, lref[2], "defaults: X")
        same(info6.res, lref[1], "defaults: res")
        theta6b, X6b, _ = A.eigsh(method="lanczos")
        same(theta6b, lref[0], "method='lanczos': theta")
        same(X6b, lref[2], "method='lanczos': X")
        for kw in (dict(method="lobpcg"), dict(precond=dM), dict(precond=dM, method="lanczos"), dict(precond=dM, method="davidson"),
                   dict(precond=dM, method="davidson", which="LA"), dict(method="davidson", which="LM"), dict(method="davidson", k=17, ncv=40)):
            with pytest.raises(api.SpmvHipError):
                A.eigsh(**kw)
    finally:
        dM.free()
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
    ilu = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    ilu.ilu0()
    IRP5, JA5, AS5 = laplacian7(5, 5, 5)
    small = api.spMatCpyCSR(api.HostCSR(125, 125, IRP5, JA5, AS5))                # a dM of another size
    other = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    hier = other.amg(coarseRows=8)                                               # a hierarchy of another matrix
    nodiag = api.spMatCpyCSR(api.HostCSR(M, M, np.arange(M + 1, dtype=np.uint64), ((np.arange(M) + 1) % M).astype(np.uint64), np.ones(M)))
    v0 = torch.ones(M, dtype=torch.float64).cuda()
    x = torch.full((18 * M,), 3.25, dtype=torch.float64).cuda()
    V, X = v0.data_ptr(), x.data_ptr()
    SA, LA = lr.SMALLEST, lr.LARGEST
    try:
        # (handle, dM, v0, X, ldx, nev, ncv, which, tol, keep)
        cases = [
            (None, None, V, X, M, 2, 8, SA, 1e-8, 0), (dead, None, V, X, M, 2, 8, SA, 1e-8, 0), (ell, None, V, X, M, 2, 8, SA, 1e-8, 0),
            (rect, None, V, X, M, 2, 8, SA, 1e-8, 0),
            (A, None, None, X, M, 2, 8, SA, 1e-8, 0), (A, None, V, None, M, 2, 8, SA, 1e-8, 0),
            (A, None, V, X, M, 0, 8, SA, 1e-8, 0), (A, None, V, X, M, 8, 8, SA, 1e-8, 0), (A, None, V, X, M, 2, 65, SA, 1e-8, 0),
            (A, None, V, X, M, 17, 40, SA, 1e-8, 0),                                 # nev > 16
            (A, None, V, X, M, 2, 8, 2, 1e-8, 0), (A, None, V, X, M, 2, 8, -1, 1e-8, 0),
            (A, None, V, X, M, 2, 8, SA, -1.0, 0), (A, None, V, X, M, 2, 8, SA, float("nan"), 0),
            (A, None, V, X, M, 2, 8, SA, 1e-8, 1), (A, None, V, X, M, 2, 8, SA, 1e-8, 8),
            (A, None, V, X, M - 1, 2, 8, SA, 1e-8, 0),
            (A, None, X + 8 * (M + 3), X, M, 2, 8, SA, 1e-8, 0), (A, None, X, X, M, 2, 8, SA, 1e-8, 0),
            (A, ilu, V, X, M, 2, 8, LA, 1e-8, 0),                                    # a dM with LARGEST
            (A, small, V, X, M, 2, 8, SA, 1e-8, 0), (A, hier, V, X, M, 2, 8, SA, 1e-8, 0), (A, dead, V, X, M, 2, 8, SA, 1e-8, 0),
            (A, ell, V, X, M, 2, 8, SA, 1e-8, 0), (A, nodiag, V, X, M, 2, 8, SA, 1e-8, 0),
        ]
        for i, (dA, dM, vp, xp, ldx, nev, ncv, which, tol, keep) in enumerate(cases):
            capfd.readouterr()
            rc, info, theta, res = _raw(api, dA, dM, vp, xp, ldx, nev, ncv, which, tol, 50, keep)
            err = capfd.readouterr().err
            assert rc == 1, i
            assert "libspmvhip" in err, i
            if dM is ilu:
                assert "SPMV_EIG_LARGEST" in err and "DESIGN.md section 42" in err
            assert torch.all(x == 3.25).item(), i
            assert (theta.view(np.uint64) == POISON).all() and (res.view(np.uint64) == POISON).all(), i
            assert C.string_at(C.addressof(info), C.sizeof(info)) == b"\xa5" * C.sizeof(info), i
        tiny = api.spMatCpyCSR(api.HostCSR(3, 3, np.arange(4, dtype=np.uint64), np.arange(3, dtype=np.uint64), np.ones(3)))
        try:
            rc, _, _, _ = _raw(api, tiny, None, V, X, 3, 1, 4, SA, 1e-8, 50)    # ncv > M
            assert rc == 1
        finally:
            tiny.free()
        opts = api.spmvDavidsonOpts(2, 8, SA, 1e-8, 50, 0)
        th = np.zeros(2)
        f = api.lib.hipSpDavidsonCSR
        assert f(C.byref(A.handle), None, V, None, X, M, th.ctypes.data, th.ctypes.data, None) == 1
        assert f(C.byref(A.handle), None, V, C.byref(opts), X, M, None, th.ctypes.data, None) == 1
        assert f(C.byref(A.handle), None, V, C.byref(opts), X, M, th.ctypes.data, None, None) == 1
        assert torch.all(x == 3.25).item()
        assert "hipSpDavidsonCSR" in capfd.readouterr().err
        th2 = np.zeros(2)
        assert f(C.byref(A.handle), None, V, C.byref(opts), X, M, th.ctypes.data, th2.ctypes.data, None) == 0   # info may be NULL
        assert f(C.byref(A.handle), C.byref(ilu.handle), V, C.byref(opts), X, M, th.ctypes.data, th2.ctypes.data, None) == 0
    finally:
        hier.free()
        for m in (A, rect, ell, ilu, small, other, nodiag):
            m.free()
