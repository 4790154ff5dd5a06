"""spmvHipDot, hipSpCGCSR and hipSpBiCGStabCSR on the device against the numpy loops of tests/krylov_ref.py, bit for bit:
the dot at block boundaries and with special values, CG and BiCGStab with and without ILU(0), every check interval,
every exit status, the handle kinds, the refusals, a non-default stream and the device memory; then every exit of both
loops (tests/krylov_exit_inputs.py) at K = 1, 16 and 64, b and x at odd element offsets (the scalar forms of the fused
passes), and the clauses of the header on dM."""
import ctypes as C

import numpy as np
import pytest

import krylov_exit_inputs as exits
import serial_order_inputs as si
from bits import assert_same_bits
from ilu0_ref import ilu0_levels
from krylov_ref import BREAKDOWN, CONVERGED, MAXITER, NONFINITE, Csr, bicgstab_ref, cg_ref, dot_ref
from test_gpu_trsv import POISON, Source, _carved, _outside_intact, same
from test_krylov_abi import convdiff7
from test_trsv_abi import laplacian7

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.lib.spmvHipSetStream(None)
    api.lib.spmvHipSetSync(1)
    api.lib.spmvHipSetVariant(b"hipSpCGCSR", 16)
    api.lib.spmvHipSetVariant(b"hipSpBiCGStabCSR", 16)


def _torch():
    return pytest.importorskip("torch")


def same_scalar(got, ref, what):
    same(np.array([float(got)]), np.array([float(ref)]), what)


# ------------------------------------------------------------------------------------------------- the dot product
@pytest.mark.parametrize("n", [0, 1, 255, 256, 4095, 4096, 4097, 3 * 4096 + 5, (1 << 22) + 17])
def test_dot_bits(api, n):
    torch = _torch()
    rng = np.random.default_rng(3000 + n % 1000)
    u, v = si.order_values(rng, n, 8), si.order_values(rng, n, 8)
    got = api.dot(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda())
    assert got.dim() == 0 and got.is_cuda
    same_scalar(got.item(), dot_ref(u, v), f"n={n}")


def test_dot_special_values_and_odd_offsets(api):
    torch = _torch()
    rng = np.random.default_rng(3010)
    n = 3 * 4096 + 5
    u, v = si.order_values(rng, n + 1, 8), si.order_values(rng, n + 1, 8)
    u[7], v[100], u[5000] = -0.0, 5e-324, 2.2e-308                      # -0.0 and subnormals
    du, dv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    for a, b, what in ((du[1:], dv[1:], "both at an odd offset"), (du[1:], dv[:-1], "one at an odd offset"),
                       (du[:-1], dv[:-1], "aligned")):
        same_scalar(api.dot(a, b).item(), dot_ref(a.cpu().numpy(), b.cpu().numpy()), what)
    neg = np.full(9000, -0.0)
    assert_same_bits(np.array([api.dot(torch.from_numpy(neg).cuda(), torch.ones(9000, dtype=torch.float64).cuda()).item()]),
                     np.array([0.0]), "-0.0 products sum to +0.0")
    for special, want in ((np.inf, np.inf), (-np.inf, -np.inf), (np.nan, np.nan)):
        w = u.copy()
        w[4097] = special
        got = api.dot(torch.from_numpy(w).cuda(), torch.from_numpy(np.abs(v)).cuda()).item()
        same_scalar(got, dot_ref(w, np.abs(v)), f"{special}")
        assert (np.isnan(got) if np.isnan(want) else got == want), special


def test_dot_refusals(api, capfd):
    torch = _torch()
    x = torch.ones(10, dtype=torch.float64).cuda()
    out = torch.zeros((), dtype=torch.float64).cuda()
    assert api.lib.spmvHipDot(10, None, x.data_ptr(), out.data_ptr()) == 1
    assert api.lib.spmvHipDot(10, x.data_ptr(), x.data_ptr(), None) == 1
    assert out.item() == 0.0
    assert "spmvHipDot" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------- solves
def _ref(kind, M, IRP, JA, AS, F, b, x0, tol, maxiter):
    return (cg_ref if kind == "cg" else bicgstab_ref)(Csr(M, IRP, JA, AS, F), b, x0, tol, maxiter)


def _solve(kind, dm, b, **kw):
    return getattr(dm, kind)(b, history=True, **kw)


def _check(kind, got, ref, what):
    x, info = got
    rx, st, it, hist, rr = ref
    assert (info.status, info.iterations) == (st, it), (what, info.status, info.iterations, st, it)
    same(x, rx, what + ": x")
    same(info.history, hist, what + ": history")
    same_scalar(info.rr, rr, what + ": rr")
    assert info.launches > 0


def _factors(api, M, IRP, JA, AS):
    P = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P.ilu0()
    return P, ilu0_levels(M, IRP, JA, AS)


@pytest.mark.parametrize("n,precond", [(40, False), (40, True), (64, False)])
def test_cg_laplacian(api, n, precond):
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    rng = np.random.default_rng(3100 + n)
    b = rng.random(M)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P, F = _factors(api, M, IRP, JA, AS) if precond else (None, None)
    try:
        got = _solve("cg", A, b, precond=P, tol=1e-8, maxiter=1000)
        ref = _ref("cg", M, IRP, JA, AS, F, b, np.zeros(M), 1e-8, 1000)
        _check("cg", got, ref, f"cg {n}^3 precond={precond}")
        assert got[1].status == CONVERGED
        res = b - Csr(M, IRP, JA, AS).spmv(got[0])
        assert np.linalg.norm(res) <= 1.01e-8 * np.linalg.norm(b)
    finally:
        A.free()
        if P is not None:
            P.free()


@pytest.mark.parametrize("precond", [False, True])
def test_bicgstab_convection_diffusion(api, precond):
    n = 40
    IRP, JA, AS = convdiff7(n, n, n)
    M = n ** 3
    b = np.random.default_rng(3200).random(M)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P, F = _factors(api, M, IRP, JA, AS) if precond else (None, None)
    try:
        got = _solve("bicgstab", A, b, precond=P, tol=1e-9, maxiter=500)
        ref = _ref("bicgstab", M, IRP, JA, AS, F, b, np.zeros(M), 1e-9, 500)
        _check("bicgstab", got, ref, f"bicgstab precond={precond}")
        assert got[1].status == CONVERGED
        res = b - Csr(M, IRP, JA, AS).spmv(got[0])
        assert np.linalg.norm(res) <= 1.01e-9 * np.linalg.norm(b)
    finally:
        A.free()
        if P is not None:
            P.free()


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_check_interval_gives_the_same_bits(api, kind):
    """K = 1, 5, 64: iterations enqueued past the stop write nothing"""
    n = 24
    IRP, JA, AS = laplacian7(n, n, n) if kind == "cg" else convdiff7(n, n, n)
    M = n ** 3
    b = np.random.default_rng(3300).random(M)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P, F = _factors(api, M, IRP, JA, AS)
    name = b"hipSpCGCSR" if kind == "cg" else b"hipSpBiCGStabCSR"
    try:
        for pre, Fm in ((None, None), (P, F)):
            ref = _ref(kind, M, IRP, JA, AS, Fm, b, np.zeros(M), 1e-10, 400)
            checks = []
            for K in (1, 5, 64):
                assert api.lib.spmvHipSetVariant(name, K) == 0
                got = _solve(kind, A, b, precond=pre, tol=1e-10, maxiter=400)
                _check(kind, got, ref, f"{kind} K={K} precond={pre is not None}")
                checks.append(got[1].hostChecks)
            it = ref[2]
            assert checks[0] == it and checks[2] == -(-it // 64), checks
    finally:
        A.free()
        P.free()


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_edge_cases(api, kind):
    n = 12
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    rng = np.random.default_rng(3400)
    b = rng.random(M)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    try:
        for maxiter in (0, 1, 4):                                        # the cap
            got = _solve(kind, A, b, tol=1e-12, maxiter=maxiter)
            _check(kind, got, _ref(kind, M, IRP, JA, AS, None, b, np.zeros(M), 1e-12, maxiter), f"maxiter={maxiter}")
            assert got[1].status == MAXITER
        got = _solve(kind, A, np.zeros(M))                              # b = 0
        assert (got[1].status, got[1].iterations) == (CONVERGED, 0)
        _check(kind, got, _ref(kind, M, IRP, JA, AS, None, np.zeros(M), np.zeros(M), 1e-8, 1000), "b = 0")
        xs = rng.integers(-8, 9, M).astype(np.float64)                  # x0 = the exact solution (integers: exact)
        bx = Csr(M, IRP, JA, AS).spmv(xs)
        got = _solve(kind, A, bx, x0=xs, tol=0.0)
        assert (got[1].status, got[1].iterations) == (CONVERGED, 0) and np.array_equal(got[0], xs)
        bad = AS.copy()                                                  # a NaN value
        bad[5] = np.nan
        A.update_values(bad)
        got = _solve(kind, A, b)
        assert got[1].status == NONFINITE
        _check(kind, got, _ref(kind, M, IRP, JA, bad, None, b, np.zeros(M), 1e-8, 1000), "NaN")
    finally:
        A.free()
    # a crafted breakdown: A = diag(1, -1), b = (1, 1): p^T A p = 0 (CG), rhat^T A p = 0 (BiCGStab)
    IRP2, JA2, AS2 = np.array([0, 1, 2], np.uint64), np.array([0, 1], np.uint64), np.array([1.0, -1.0])
    A2 = api.spMatCpyCSR(api.HostCSR(2, 2, IRP2, JA2, AS2))
    try:
        got = _solve(kind, A2, np.ones(2))
        assert (got[1].status, got[1].iterations) == (BREAKDOWN, 0)
        _check(kind, got, _ref(kind, 2, IRP2, JA2, AS2, None, np.ones(2), np.zeros(2), 1e-8, 1000), "breakdown")
    finally:
        A2.free()


def test_handle_kinds(api):
    """a pattern handle (every value 1.0), adopted handles with 4- and 8-byte row pointers, and a Newton-style value update
    followed by a refactorisation, each bit for bit"""
    n = 20
    IRP, JA, AS = convdiff7(n, n, n)
    M = n ** 3
    rng = np.random.default_rng(3500)
    b = rng.random(M)
    ones = np.ones_like(AS)
    src = Source(api, M, M, IRP, JA, ones)
    try:
        got = _solve("bicgstab", src.dm, b, maxiter=30)
        _check("bicgstab", got, _ref("bicgstab", M, IRP, JA, ones, None, b, np.zeros(M), 1e-8, 30), "pattern handle")
    finally:
        src.free()
    for adopt in (4, 8):
        src = Source(api, M, M, IRP, JA, AS, adopt=adopt)
        P = Source(api, M, M, IRP, JA, AS, adopt=adopt)
        try:
            P.dm.ilu0()
            F = ilu0_levels(M, IRP, JA, AS)
            got = _solve("bicgstab", src.dm, b, precond=P.dm, tol=1e-10)
            _check("bicgstab", got, _ref("bicgstab", M, IRP, JA, AS, F, b, np.zeros(M), 1e-10, 1000), f"adopted {adopt}")
        finally:
            src.free()
            P.free()
    # Newton-style: new values on both handles, refactor, solve again from the last x
    IRP, JA, AS = laplacian7(n, n, n)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P, F = _factors(api, M, IRP, JA, AS)
    try:
        x1, _ = _solve("cg", A, b, precond=P)
        AS2 = np.where(AS > 0, AS + rng.random(AS.size), AS)
        A.update_values(AS2)
        P.update_values(AS2)
        P.ilu0()
        got = _solve("cg", A, b, x0=x1, precond=P)
        _check("cg", got, _ref("cg", M, IRP, JA, AS2, ilu0_levels(M, IRP, JA, AS2), b, x1, 1e-8, 1000), "after an update")
    finally:
        A.free()
        P.free()


def test_refusals_leave_x_untouched(api, capfd):
    torch = _torch()
    from spmv_openmp_cuda_amd import api as a
    n = 6
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    A = a.spMatCpyCSR(a.HostCSR(M, M, IRP, JA, AS))
    P = a.spMatCpyCSR(a.HostCSR(M, M, IRP, JA, AS))
    IRPs, JAs, ASs = laplacian7(5, 5, 5)
    S = a.spMatCpyCSR(a.HostCSR(125, 125, IRPs, JAs, ASs))
    rect = a.spMatCpyCSR(a.HostCSR(M, M + 1, IRP, JA, AS))
    nodiag_rows = np.repeat(np.arange(M), np.diff(IRP.astype(np.int64)))
    off = JA.astype(np.int64) != nodiag_rows                             # a matrix without its diagonal
    ND = a.spMatCpyCSR(a.HostCSR(M, M, *si.assemble(M, nodiag_rows[off], JA.astype(np.int64)[off], AS[off])))
    ell = a.spMatCpyELL(a.HostCSR(M, M, IRP, JA, AS).to_ell())
    b = torch.from_numpy(np.random.default_rng(3600).random(M)).cuda()
    x = torch.full((M,), 3.25, dtype=torch.float64).cuda()
    big = torch.zeros(2 * M, dtype=torch.float64).cuda()
    try:
        for fn in (a.lib.hipSpCGCSR, a.lib.hipSpBiCGStabCSR):
            def call(dA, dM, bp, xp, tol=1e-8, maxiter=10, hist=None):
                o = a.spmvKrylovOpts(tol, maxiter, hist)
                info = a.spmvKrylovInfo()
                return fn(C.byref(dA.handle) if dA is not None else None, C.byref(dM.handle) if dM is not None else None,
                          bp, xp, C.byref(o), C.byref(info))
            cases = [
                (None, None, b.data_ptr(), x.data_ptr(), {}),
                (A, None, None, x.data_ptr(), {}),
                (A, None, b.data_ptr(), None, {}),
                (ell, None, b.data_ptr(), x.data_ptr(), {}),
                (rect, None, b.data_ptr(), x.data_ptr(), {}),
                (A, S, b.data_ptr(), x.data_ptr(), {}),
                (A, ND, b.data_ptr(), x.data_ptr(), {}),
                (A, None, x.data_ptr(), x.data_ptr(), {}),
                (A, None, big.data_ptr(), big.data_ptr() + 8 * (M // 2), {}),
                (A, None, b.data_ptr(), x.data_ptr(), {"tol": -1.0}),
                (A, None, b.data_ptr(), x.data_ptr(), {"tol": float("nan")}),
                (A, None, b.data_ptr(), x.data_ptr(), {"maxiter": (1 << 64) - 1,
                                                       "hist": C.cast(C.c_void_p(8), C.POINTER(C.c_double))}),
            ]
            for i, (dA, dM, bp, xp, kw) in enumerate(cases):
                assert call(dA, dM, bp, xp, **kw) == 1, (fn.__name__, i)
                assert torch.all(x == 3.25).item(), (fn.__name__, i)
            assert fn(C.byref(A.handle), None, b.data_ptr(), x.data_ptr(), None, None) == 1
            assert torch.all(x == 3.25).item()
        assert "hipSpCGCSR" in capfd.readouterr().err
    finally:
        for m in (A, P, S, rect, ND, ell):
            m.free()


def test_non_default_stream(api):
    torch = _torch()
    n = 16
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    b = np.random.default_rng(3700).random(M)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P, F = _factors(api, M, IRP, JA, AS)
    s = torch.cuda.Stream()
    try:
        api.lib.spmvHipSetStream(C.c_void_p(s.cuda_stream))
        for kind in ("cg", "bicgstab"):
            got = _solve(kind, A, b, precond=P)
            _check(kind, got, _ref(kind, M, IRP, JA, AS, F, b, np.zeros(M), 1e-8, 1000), f"{kind} on a stream")
        bt = torch.from_numpy(b).cuda()
        torch.cuda.synchronize()
        d = api.dot(bt, bt)
        api.lib.spmvHipDeviceSynchronize()
        same_scalar(d.item(), dot_ref(b, b), "dot on a stream")
    finally:
        api.lib.spmvHipSetStream(None)
        A.free()
        P.free()


def test_device_memory_comes_back(api):
    torch = _torch()
    n = 24
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    b = torch.from_numpy(np.random.default_rng(3800).random(M)).cuda()
    free = []
    for _ in range(10):
        A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
        P, _ = _factors(api, M, IRP, JA, AS)
        A.cg(b, precond=P, history=True)
        A.bicgstab(b, precond=P)
        api.dot(b, b)
        A.free()
        P.free()
        api.spmvHipFinalize()
        api.spmvHipInit(0)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert np.median(free[2:]) >= free[1] - (8 << 20) and free[-1] >= free[1] - (8 << 20), free


# ------------------------------------------------------------------------------------------------- every exit
FN = {"cg": "hipSpCGCSR", "bicgstab": "hipSpBiCGStabCSR"}


def _poisoned(n):
    return np.full(n, POISON, dtype=np.uint64).view(np.float64)


def _raw(api, kind, A, P, b_ptr, x_ptr, tol, maxiter):
    """the solver through the C ABI with a history full of poison: (return code, info, history as handed back)"""
    hist = _poisoned(maxiter + 1)
    opts = api.spmvKrylovOpts(float(tol), int(maxiter), hist.ctypes.data_as(C.POINTER(C.c_double)))
    info = api.spmvKrylovInfo()
    rc = getattr(api.lib, FN[kind])(C.byref(A.handle), C.byref(P.handle) if P is not None else None, b_ptr, x_ptr,
                                    C.byref(opts), C.byref(info))
    return rc, info, hist


def _check_raw(info, hist, x, ref, what):
    rx, st, it, rhist, rr = ref
    assert (info.status, info.iterations) == (st, it), (what, info.status, info.iterations, st, it)
    same(x, rx, what + ": x")
    same(hist[:it + 1], rhist, what + ": history")
    assert (hist[it + 1:].view(np.uint64) == POISON).all(), what + ": history written past `iterations`"
    same_scalar(info.rr, rr, what + ": rr")


@pytest.mark.parametrize("name", exits.NAMES)
def test_every_exit(api, name):
    """each case of the exit table (tests/test_krylov_abi.py shows which `return` it takes) at three check intervals:
    status, iterations, x, history and rr are the reference's bits, the history past `iterations` is not written, and at a
    half-step exit x = x + alpha * phat was written after the stop"""
    torch = _torch()
    c = exits.case(name)
    with np.errstate(all="ignore"):
        F = ilu0_levels(c.M, c.IRP, c.JA, c.AS) if c.precond else None
    half = {}
    kw = {"half": half} if c.solver == "bicgstab" else {}
    ref = (cg_ref if c.solver == "cg" else bicgstab_ref)(Csr(c.M, c.IRP, c.JA, c.AS, F), c.b, c.x0, c.tol, c.maxiter, **kw)
    A = api.spMatCpyCSR(api.HostCSR(c.M, c.M, c.IRP, c.JA, c.AS))
    P = _factors(api, c.M, c.IRP, c.JA, c.AS)[0] if c.precond else None
    db = torch.from_numpy(c.b).cuda()
    xs = {}
    try:
        if name.endswith(":2I"):                                         # the case is there for the unit kernels
            v = C.c_double(0)
            assert api.lib.spmvHipUnitValue(C.byref(A.handle), C.byref(v)) == 1 and v.value == 2.0
        for K in (1, 16, 64):
            assert api.lib.spmvHipSetVariant(FN[c.solver].encode(), K) == 0
            got = _solve(c.solver, A, c.b, x0=c.x0, precond=P, tol=c.tol, maxiter=c.maxiter)
            _check(c.solver, got, ref, f"{name} K={K}")
            dx = torch.from_numpy(c.x0).cuda()
            rc, info, hist = _raw(api, c.solver, A, P, db.data_ptr(), dx.data_ptr(), c.tol, c.maxiter)
            assert rc == 0
            xs[K] = dx.cpu().numpy()
            _check_raw(info, hist, xs[K], ref, f"{name} K={K}, C ABI")
            same(got[0], xs[K], f"{name} K={K}: the two calls")
        for K in (16, 64):
            same(xs[K], xs[1], f"{name}: x at K={K} against K=1")
        if c.label in ("half_converged", "tt0"):
            assert not np.array_equal(xs[1], c.x0), name
            with np.errstate(all="ignore"):
                same(xs[1], half["x"] + half["alpha"] * half["phat"], f"{name}: x + alpha * phat")
    finally:
        A.free()
        if P is not None:
            P.free()


# ------------------------------------------------------------------------------------------------- alignment forms
ODD_GRID = (21, 19, 17)                 # n = 6 783: odd (the last pair is half) and one block of 4 096 plus a short one


@pytest.mark.parametrize("kind,precond", [("cg", False), ("cg", True), ("bicgstab", False), ("bicgstab", True)])
def test_b_and_x_at_odd_offsets(api, kind, precond):
    """dB / dX that are only 8-byte aligned send InitOp, CgUpdateOp / BiUpdateOp, the first SpMV and the triangular solves
    of dM down their scalar forms, alternating with the 16-byte forms of the passes on the workspace: the same bits, and
    nothing outside the views is touched"""
    torch = _torch()
    IRP, JA, AS = (laplacian7 if kind == "cg" else convdiff7)(*ODD_GRID)
    M = int(np.prod(ODD_GRID))
    assert M % 2 == 1 and M % 4096
    rng = np.random.default_rng(3900)
    b, x0 = rng.random(M), rng.uniform(-1, 1, M)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P, F = _factors(api, M, IRP, JA, AS) if precond else (None, None)
    ref = _ref(kind, M, IRP, JA, AS, F, b, x0, 1e-10, 40)
    try:
        for ob, ox in ((0, 0), (1, 0), (0, 1), (1, 1)):
            what = f"{kind} precond={precond} b+{ob} x+{ox}"
            bigb, vb = _carved(torch, b, ob)
            bigx, vx = _carved(torch, x0, ox)
            assert vb.data_ptr() % 16 == 8 * ob and vx.data_ptr() % 16 == 8 * ox
            rc, info, hist = _raw(api, kind, A, P, vb.data_ptr(), vx.data_ptr(), 1e-10, 40)
            assert rc == 0
            _check_raw(info, hist, vx.cpu().numpy(), ref, what)
            _outside_intact(bigb, ob, M, what + " (b)")
            _outside_intact(bigx, ox, M, what + " (x)")
            same(vb.cpu().numpy(), b, what + ": b is read only")
    finally:
        A.free()
        if P is not None:
            P.free()


def test_serial_order_spmv_reads_x_at_an_odd_offset(api):
    """the product inside a solve reads the caller's x0: the selected serial-order kernel on an 8-byte aligned x (and y)"""
    torch = _torch()
    n = 40
    IRP, JA, AS = convdiff7(n, n, n)
    M = n ** 3
    assert JA.size >= exits.AUTO_MIN_NNZ
    x = si.order_values(np.random.default_rng(3910), M, 8)
    y_ref = Csr(M, IRP, JA, AS).spmv(x)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    try:
        for ox, oy in ((1, 0), (1, 1), (0, 1), (0, 0)):
            bigx, vx = _carved(torch, x, ox)
            bigy, vy = _carved(torch, np.zeros(M), oy)
            vy.fill_(float("nan"))
            torch.cuda.synchronize()
            assert api.lib.spmvHipEnqueueAutoRows(C.byref(A.handle), C.c_void_p(vx.data_ptr()), C.c_void_p(vy.data_ptr()), None) == 0
            assert api.lib.spmvHipDeviceSynchronize() == 0
            assert_same_bits(vy.cpu().numpy(), y_ref, f"x+{ox} y+{oy}")
            _outside_intact(bigy, oy, M, f"x+{ox} y+{oy}")
        assert api.lib.spmvHipAutoChoiceRows(C.byref(A.handle), None) is not None
    finally:
        A.free()


# ------------------------------------------------------------------------------------------------- clauses on dM
def _tame(IRP, JA, AS, lower):
    """AS with the strictly lower (`lower`) or the strictly upper entries divided by 8: the other triangle dominates, and
    the raw triangles of the result are a mild preconditioner"""
    rows = si.row_of_entry(IRP)
    j = JA.astype(np.int64)
    return np.where((j < rows) if lower else (j > rows), AS / 8, AS)


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_dM_is_dA(api, kind):
    """"dM == dA is allowed": A used raw as its own preconditioner (M^-1 is its unit lower and its stored upper triangle,
    for a lower- and an upper-dominant A), and A holding ILU(0) factors as matrix and preconditioner at once"""
    n = 14
    IRP, JA, AS0 = convdiff7(n, n, n)
    M = n ** 3
    b = np.random.default_rng(3920).random(M)
    for what, AS, factor in (("upper-dominant, raw", _tame(IRP, JA, AS0, True), False),
                             ("lower-dominant, raw", _tame(IRP, JA, AS0, False), False), ("ILU(0) factors", AS0, True)):
        A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
        try:
            if factor:
                A.ilu0()
                AS = ilu0_levels(M, IRP, JA, AS)
            got = _solve(kind, A, b, precond=A, tol=1e-10, maxiter=12)
            _check(kind, got, _ref(kind, M, IRP, JA, AS, AS, b, np.zeros(M), 1e-10, 12), f"{kind} dM == dA, {what}")
        finally:
            A.free()


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_M_zero(api, kind):
    """"M = 0 succeeds: CONVERGED, 0": no read-back of a device state, x and its neighbours untouched, and of the history
    only hist[0 .. iterations] = hist[0] is written: dot(r, r) over no elements, +0.0"""
    torch = _torch()
    empty = (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    A, P = Source(api, 0, 0, *empty), Source(api, 0, 0, *empty)
    big = torch.from_numpy(_poisoned(4)).cuda()
    try:
        for pre in (None, P.dm):
            rc, info, hist = _raw(api, kind, A.dm, pre, big.data_ptr(), big.data_ptr() + 16, 1e-8, 5)
            assert rc == 0
            assert (info.status, info.iterations, info.hostChecks) == (CONVERGED, 0, 0)
            assert_same_bits(hist[:1], np.array([0.0]), "hist[0]")
            assert (hist[1:].view(np.uint64) == POISON).all()
            same_scalar(info.rr, 0.0, "rr")
            assert (big.cpu().numpy().view(np.uint64) == POISON).all()
    finally:
        A.free()
        P.free()


def test_dM_analysed_by_the_solve(api):
    """a dM that holds factors but has never been analysed: the first solve builds both schedules, the second keeps them"""
    n = 16
    IRP, JA, AS = convdiff7(n, n, n)
    M = n ** 3
    b = np.random.default_rng(3930).random(M)
    F = ilu0_levels(M, IRP, JA, AS)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, F))                  # the factors uploaded: no hipSpILU0CSR, no analysis
    try:
        assert [P.triangular_info(lo).analyses for lo in (True, False)] == [0, 0]
        assert [P.triangular_info(lo).levels for lo in (True, False)] == [0, 0]
        for kind in ("bicgstab", "cg"):
            got = _solve(kind, A, b, precond=P, tol=1e-10, maxiter=8)
            _check(kind, got, _ref(kind, M, IRP, JA, AS, F, b, np.zeros(M), 1e-10, 8), f"{kind}, dM not analysed before")
            infos = [P.triangular_info(lo) for lo in (True, False)]
            assert [i.analyses for i in infos] == [1, 1] and all(i.levels == 3 * n - 2 for i in infos)
    finally:
        A.free()
        P.free()


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_dM_updated_to_a_constant_and_not_refactored(api, kind):
    """dM factored, then every value set to 1.0 (a unit handle) and NOT factored again: M^-1 is the raw triangles of the
    constant matrix, the schedules stay, the loop runs on whatever that gives"""
    n = 10
    IRP, JA, AS = (laplacian7 if kind == "cg" else convdiff7)(n, n, n)
    M = n ** 3
    b = np.random.default_rng(3940).random(M)
    ones = np.ones_like(AS)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P, _ = _factors(api, M, IRP, JA, AS)
    try:
        P.update_values(ones)
        v = C.c_double(0)
        assert api.lib.spmvHipUnitValue(C.byref(P.handle), C.byref(v)) == 1 and v.value == 1.0
        got = _solve(kind, A, b, precond=P, tol=1e-10, maxiter=4)
        _check(kind, got, _ref(kind, M, IRP, JA, AS, ones, b, np.zeros(M), 1e-10, 4), f"{kind}, dM a unit handle")
        assert [P.triangular_info(lo).analyses for lo in (True, False)] == [1, 1]
        assert P.ilu0_info().factorisations == 1
    finally:
        A.free()
        P.free()
