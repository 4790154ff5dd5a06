"""The Chebyshev smoother of the multigrid cycle on the device (spmvHipAmgSetSmoother, spmvHipAmgSmoother, and such a
hierarchy under spmvHipAmgApply / Refresh and as dM of the Krylov solvers) against tests/amg_cheb_ref.py, bits throughout:
the cycle on plain, smoothed and strength hierarchies at both fuse thresholds and four degree triples (special values, an
odd M, misaligned vectors, one level, no rows), every level's table and view, the three solvers with CG's exact count, the
launch count of a cycle, the stop, a captured replay across a refresh at the table's address, switching back and forth,
every refusal with the cycle and the views compared as bytes, and device memory."""
import ctypes as C
import functools

import numpy as np
import pytest

import amg_cheb_ref as cr
import amg_ref as ar
import amg_sa_ref as sa
import filter_ref as fr
import spgemm_ref as sr
from amg_gpu import _same, _solve_and_compare, _up, cycle_launches
from bits import assert_same_bits
from gmres_ref import gmres_ref
from krylov_ref import bicgstab_ref, cg_ref
from test_amg_cheb_abi import COUNTS, KRYLOV_OPTS, KRYLOV_TOL, krylov_problem

pytestmark = pytest.mark.gpu

LAP = sr.laplacian7(12, 10, 8)                                  # 960 rows, three levels at coarseRows = 8
ANISO = fr.stencil7(12, 10, 8, (1.0, 0.01, 0.01))               # the strength filter drops entries of it
ODD = sa.with_one_diagonal(*(lambda a: (a[0], a[2], a[3]))(sr.laplacian7(5, 3, 3)), seed=41)       # 45 rows
GRAPHS = {name: sa.with_one_diagonal(*g, seed=n) for n, (name, g) in enumerate(ar.small_graphs().items())}
FUSED, NEVER = 64, 0
HIERARCHIES = {"plain": dict(), "smoothed": dict(smoothed=True), "strength": dict(smoothed=True, theta=0.0)}
DEGREES = [(2, 2, 8), (3, 1, 1), (1, 3, 0), (0, 2, 2)]          # (nu1, nu2, nuCoarse); 0: SPMV_AMG_NO_SWEEPS through the Python layer


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
    api.set_variant("spmvHipAmgApply", NEVER)
    api.set_variant("hipSpCGCSR", 16)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _matrix(hierarchy):
    return ANISO if hierarchy == "strength" else LAP


@functools.lru_cache(maxsize=None)
def _levels(hierarchy, depth=None):
    kw = dict(maxLevels=depth) if depth else {}
    levels, o = cr.setup_ref(_matrix(hierarchy), hierarchy, coarseRows=8, **kw)
    assert len(levels) == depth if depth else len(levels) >= 3
    return levels, o


def _special_r(M, seed=7):
    r = np.random.default_rng(seed).standard_normal(M)
    r[[3, M // 2]] = 0.0
    r[[4, M // 2 + 1]] = -0.0
    r[M // 3], r[M // 3 + 1], r[M - 2] = np.inf, -np.inf, np.nan
    return r


def _view_blob(h):
    """every level's view and table as bytes"""
    out = []
    for l in range(h.info.levels):
        v = h.smoother(l)
        out.append(repr([v[k] for k in ("kind", "nu1", "nu2", "nuCoarse", "dCoef")]).encode() +
                   np.array([v["rho"], v["lambdaMax"], v["lambdaMin"]]).tobytes() + v["coef"].tobytes())
    return b"|".join(out)


def _check_tables(h, levels, sm, what):
    tabs = cr.tables(levels, sm)
    total = 0
    for l, t in enumerate(tabs):
        v = h.smoother(l)
        assert (v["kind"], v["nu1"], v["nu2"], v["nuCoarse"]) == (cr.CHEBYSHEV, sm["nu1"], sm["nu2"], sm["nuCoarse"]), (what, l)
        for key, ref in (("rho", "rho"), ("lambdaMax", "lmax"), ("lambdaMin", "lmin")):
            assert _bits(v[key]) == _bits(t[ref]), (what, l, key, v[key], t[ref])
        assert v["coef"].shape == t["ab"].shape and np.array_equal(_bits(v["coef"]), _bits(t["ab"])), (what, l)
        assert (v["dCoef"] is None) == (t["ab"].shape[0] == 0)
        total += 16 * t["ab"].shape[0]
    return total


def test_device_memory_is_flat_across_twenty_calls(api):
    """(first in the file: no other test's handles are alive yet)  The tables are a few hundred bytes each, so the free
    memory can only show a gross leak; the bytes the hierarchy reports must come back exactly"""
    import torch
    da = _up(api, LAP)
    h = da.amg(coarseRows=8, smoothed=True)
    try:
        base = int(h.info.bytes)

        def once(i):
            if i % 2:
                h.set_smoother("jacobi", nu1=1 + i % 3, nu2=1, nuCoarse=8)
                assert int(h.info.bytes) == base
            else:
                h.set_smoother("chebyshev", nu1=1 + i % 5, nu2=2 + i % 7, nuCoarse=3 + i % 4)
                assert int(h.info.bytes) == base + 16 * ((h.info.levels - 1) * max(1 + i % 5, 2 + i % 7) + 3 + i % 4)
        once(0), once(1)
        h.apply(np.ones(LAP[0]))
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        for i in range(20):
            once(i)
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        assert after >= before - (8 << 20), (before, after)
        assert int(h.info.bytes) == base
    finally:
        h.free()
        da.free()


# --------------------------------------------------------------------------------------------------------------- cycle
@pytest.mark.parametrize("threshold", [NEVER, FUSED])
@pytest.mark.parametrize("nu", DEGREES)
@pytest.mark.parametrize("hierarchy", list(HIERARCHIES))
def test_cycle_bits_tables_and_views(api, hierarchy, nu, threshold):
    A = _matrix(hierarchy)
    levels, o = _levels(hierarchy)
    api.set_variant("spmvHipAmgApply", threshold)
    da = _up(api, A)
    h = da.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    try:
        before = int(h.info.bytes)
        never = h.smoother(0)
        assert (never["kind"], never["nu1"], never["nu2"], never["nuCoarse"]) == (cr.JACOBI, 1, 1, 8)
        assert (never["rho"], never["lambdaMax"], never["lambdaMin"], never["dCoef"], never["coef"].size) == (0.0, 0.0, 0.0, None, 0)
        for kw, ref_kw in ((dict(), dict()), (dict(eig_ratio=4.0, lambda_scale=1.1), dict(eigRatio=4.0, lambdaScale=1.1))):
            h.set_smoother("chebyshev", nu1=nu[0], nu2=nu[1], nuCoarse=nu[2], **kw)
            sm = cr.smoother(o, nu1=nu[0], nu2=nu[1], nuCoarse=nu[2], **ref_kw)
            what = f"{hierarchy}, degrees {nu}, threshold {threshold}, {kw}"
            assert int(h.info.bytes) == before + _check_tables(h, levels, sm, what)
            for name, r in (("random", np.random.default_rng(8).standard_normal(A[0])), ("special", _special_r(A[0]))):
                _same(h.apply(r), cr.cycle_ref(levels, o, r, sm), f"{name} r, {what}")
    finally:
        h.free()
        da.free()


def test_the_strength_hierarchy_takes_rho_from_a_not_f(api):
    levels, o = _levels("strength")
    sm = cr.smoother(o, nu1=2, nu2=2)
    assert _bits(cr.tables(levels, sm)[0]["rho"]) != _bits(cr.tables(levels, dict(sm, rho_from_F=True))[0]["rho"])
    da = _up(api, ANISO)
    h = da.amg(coarseRows=8, smoothed=True, theta=0.0)
    try:
        h.set_smoother(nu1=2, nu2=2)
        assert _bits(h.smoother(0)["rho"]) == _bits(cr.tables(levels, sm)[0]["rho"])
    finally:
        h.free()
        da.free()


@pytest.mark.parametrize("threshold", [NEVER, FUSED])
def test_odd_rows_and_vectors_at_odd_eight_byte_offsets(api, threshold):
    import torch
    M = ODD[0]
    levels, o = sa.setup_ref(ODD, coarseRows=4)
    assert M % 2 == 1 and len(levels) >= 2
    sm = cr.smoother(o, nu1=3, nu2=2, nuCoarse=4)
    r = _special_r(M)
    want = cr.cycle_ref(levels, o, r, sm)
    api.set_variant("spmvHipAmgApply", threshold)
    da = _up(api, ODD)
    h = da.amg(coarseRows=4, smoothed=True)
    try:
        h.set_smoother(nu1=3, nu2=2, nuCoarse=4)
        _same(h.apply(r), want, "odd M")
        rb, zb = torch.zeros(M + 1, dtype=torch.float64, device="cuda"), torch.zeros(M + 1, dtype=torch.float64, device="cuda")
        rv, zv = rb[1:], zb[1:]
        assert rv.data_ptr() % 16 == 8 and zv.data_ptr() % 16 == 8
        rv.copy_(torch.from_numpy(r))
        h.apply(rv, out=zv)
        _same(zv.cpu().numpy(), want, "vectors at odd 8-byte offsets")
    finally:
        h.free()
        da.free()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_small_graphs(api, name):
    """no rows, one to three rows, a path, stars, a messy pattern: unsorted rows, repeats, isolated vertices"""
    A = GRAPHS[name]
    levels, o = sa.setup_ref(A, coarseRows=8)
    sm = cr.smoother(o, nu1=2, nu2=2, nuCoarse=3)
    da = _up(api, A)
    h = da.amg(coarseRows=8, smoothed=True)
    try:
        h.set_smoother(nu1=2, nu2=2, nuCoarse=3)
        _check_tables(h, levels, sm, name)
        r = np.random.default_rng(9).standard_normal(A[0])
        z = h.apply(r)
        assert z.shape == (A[0],)
        if A[0]:
            _same(z, cr.cycle_ref(levels, o, r, sm), name)
        else:
            assert h.smoother(0)["rho"] == 0.0 and not h.smoother(0)["coef"].any()
    finally:
        h.free()
        da.free()


@pytest.mark.parametrize("q", [1, 5])
def test_one_level_is_a_polynomial_preconditioner(api, q):
    levels, o = _levels("plain", 1)
    sm = cr.smoother(o, nuCoarse=q)
    r = np.random.default_rng(10).standard_normal(LAP[0])
    da = _up(api, LAP)
    h = da.amg(maxLevels=1)
    try:
        h.set_smoother(nuCoarse=q)
        assert h.info.levels == 1 and h.smoother(0)["coef"].shape == (q, 2)
        _same(h.apply(r), cr.cycle_ref(levels, o, r, sm), f"one level, degree {q}")
    finally:
        h.free()
        da.free()


# -------------------------------------------------------------------------------------------------------------- Krylov
NU = 2


@pytest.fixture(scope="module")
def krylov(api):
    """the Laplacian of the CPU test and its right-hand side; per hierarchy the reference with Chebyshev at nu1 = nu2 = 2 and
    the device hierarchy given the same smoother"""
    A, b = krylov_problem((12, 10, 8))
    da = _up(api, A)
    out = {}
    for hierarchy in ("plain", "smoothed"):
        ref = cr.ChebCsr(A, hierarchy, sm=dict(nu1=NU, nu2=NU), **KRYLOV_OPTS)
        h = da.amg(**KRYLOV_OPTS, **HIERARCHIES[hierarchy])
        h.set_smoother(nu1=NU, nu2=NU)
        out[hierarchy] = (ref, h)
    yield A, b, da, out
    for _, h in out.values():
        h.free()
    da.free()


@pytest.mark.parametrize("hierarchy", ["plain", "smoothed"])
def test_cg_takes_the_reference_count_and_a_cycle_the_launches_of_jacobi(api, krylov, hierarchy):
    A, b, da, hs = krylov
    ref, h = hs[hierarchy]
    want = cg_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200)
    assert want[2] == COUNTS[((12, 10, 8), hierarchy, NU)][2]
    info = _solve_and_compare(da, b, h, "cg", want, KRYLOV_TOL)
    assert info.iterations == want[2]
    # CG's own kernels: 4 before the loop and 6 per enqueued iteration (whole batches of K = 16); every M^-1 (one before the
    # loop, one per iteration) adds the cycle, a dot pass and its finish
    enq = lambda it: min(200, -(-it // 16) * 16)
    unfused = h.info.levels - 1 if hierarchy == "smoothed" else 0
    cycle = cycle_launches(NU, NU, 8, h.info.levels, unfused)
    assert info.launches == 4 + 6 * enq(want[2]) + (enq(want[2]) + 1) * (cycle + 2)
    h.set_smoother("jacobi")                                         # the same sweeps, the other kind
    try:
        jac = cg_ref(cr.ChebCsr(A, levels=ref.levels, o=ref.o, sm=dict(kind=cr.JACOBI, nu1=NU, nu2=NU)), b, np.zeros(A[0]), KRYLOV_TOL, 200)
        assert jac[2] == COUNTS[((12, 10, 8), hierarchy, NU)][0]
        info = _solve_and_compare(da, b, h, "cg", jac, KRYLOV_TOL)
        assert info.launches == 4 + 6 * enq(jac[2]) + (enq(jac[2]) + 1) * (cycle + 2), "Jacobi's cycle is as many kernels"
    finally:
        h.set_smoother(nu1=NU, nu2=NU)


@pytest.mark.parametrize("hierarchy", ["plain", "smoothed"])
def test_bicgstab_and_gmres(api, krylov, hierarchy):
    A, b, da, hs = krylov
    ref, h = hs[hierarchy]
    _solve_and_compare(da, b, h, "bicgstab", bicgstab_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200), KRYLOV_TOL)
    _solve_and_compare(da, b, h, "gmres", gmres_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200, 5), KRYLOV_TOL, restart=5)


def test_cycles_queued_past_the_stop_write_nothing(api, krylov):
    A, b, da, hs = krylov
    for hierarchy, (ref, h) in hs.items():
        want = cg_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200)
        assert want[2] % 16, "the stop falls inside a batch of K = 16: queued cycles run after it"
        xs = []
        for K in (1, 16):
            api.set_variant("hipSpCGCSR", K)
            x, info = da.cg(b, precond=h, tol=KRYLOV_TOL, maxiter=200)
            assert info.iterations == want[2]
            xs.append(x)
        assert_same_bits(xs[0], want[0], f"{hierarchy}: K = 1")
        assert_same_bits(xs[1], xs[0], f"{hierarchy}: K = 16 against K = 1")


# ------------------------------------------------------------------------------------------------- capture and refresh
def _new_values():
    """other values on LAP's pattern, the diagonal scaled row by row: rho moves on every level"""
    rng = np.random.default_rng(11)
    new = LAP[4] * (1.0 + 0.25 * rng.random(LAP[4].size))
    rows = sr.si.row_of_entry(LAP[2])
    diag = LAP[3].astype(np.int64) == rows
    new[diag] = new[diag] * (1.0 + rng.random(int(diag.sum())))
    return LAP[:4] + (new,)


@pytest.mark.parametrize("hierarchy", ["plain", "smoothed"])
def test_a_captured_cycle_replayed_after_a_refresh_uses_the_new_table(api, hierarchy):
    import torch
    M = LAP[0]
    B = _new_values()
    kw = dict(nu1=2, nu2=3, nuCoarse=4)
    old, o = cr.setup_ref(LAP, hierarchy, coarseRows=8)
    new, _ = cr.setup_ref(B, hierarchy, coarseRows=8)
    sm = cr.smoother(o, **kw)
    told, tnew = cr.tables(old, sm), cr.tables(new, sm)
    assert all(_bits(a["rho"]) != _bits(b["rho"]) for a, b in zip(told, tnew)), "every rho moves"
    r = np.random.default_rng(12).standard_normal(M)
    da, db = _up(api, LAP), _up(api, B)
    h = da.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    fresh = db.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    try:
        h.set_smoother(**kw)
        fresh.set_smoother(**kw)
        where = [h.smoother(l)["dCoef"] for l in range(h.info.levels)]
        api.lib.spmvHipSetSync(0)
        s = torch.cuda.Stream()
        api.lib.spmvHipSetStream(C.c_void_p(s.cuda_stream))
        rt, zt = torch.from_numpy(r).cuda(), torch.zeros(M, dtype=torch.float64, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                h.apply(rt, out=zt)
        g.replay()
        torch.cuda.synchronize()
        _same(zt.cpu().numpy(), cr.cycle_ref(old, o, r, sm), "captured replay")
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        da.update_values(B[4])
        h.refresh_from(da)
        assert [h.smoother(l)["dCoef"] for l in range(h.info.levels)] == where, "the tables stay where they are"
        _check_tables(h, new, sm, "refreshed")
        _check_tables(fresh, new, sm, "fresh")
        zt.zero_()
        g.replay()
        torch.cuda.synchronize()
        z = zt.cpu().numpy()
        _same(z, cr.cycle_ref(new, o, r, sm), "the same graph after the refresh")
        assert_same_bits(z, fresh.apply(r), "refreshed against a fresh setup and the same call")
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        fresh.free()
        h.free()
        db.free()
        da.free()


# ----------------------------------------------------------------------------------------------------------- switching
@pytest.mark.parametrize("hierarchy", list(HIERARCHIES))
def test_switching_back_and_forth(api, hierarchy):
    A = _matrix(hierarchy)
    r = _special_r(A[0], seed=13)
    da = _up(api, A)
    kw = dict(coarseRows=8, **HIERARCHIES[hierarchy])
    h, two = da.amg(**kw), da.amg(nu1=2, nu2=3, nuCoarse=5, **kw)
    second = da.amg(**kw)
    try:
        z0, bytes0, view0 = h.apply(r).tobytes(), int(h.info.bytes), _view_blob(h)
        h.set_smoother(nu1=3, nu2=2)
        assert h.apply(r).tobytes() != z0 and int(h.info.bytes) > bytes0
        h.set_smoother("jacobi", nu1=1, nu2=1, nuCoarse=8)
        assert (h.apply(r).tobytes(), int(h.info.bytes), _view_blob(h)) == (z0, bytes0, view0), "back to what the setup gave"
        h.set_smoother("jacobi", nu1=2, nu2=3, nuCoarse=5)
        assert h.apply(r).tobytes() == two.apply(r).tobytes(), "Jacobi with new sweeps is a fresh setup with those sweeps"
        assert lib_set(api, h, None) == 0 and h.apply(r).tobytes() == two.apply(r).tobytes(), "opts == NULL: Jacobi, the current sweeps"
        h.set_smoother("chebyshev", nu1=4, nu2=1, nuCoarse=2, eig_ratio=30.0)
        h.set_smoother("chebyshev", nu1=1, nu2=2, nuCoarse=3, eig_ratio=4.0)
        second.set_smoother("chebyshev", nu1=1, nu2=2, nuCoarse=3, eig_ratio=4.0)
        assert h.apply(r).tobytes() == second.apply(r).tobytes(), "two calls in a row equal the second alone"
        assert [h.smoother(l)["coef"].tobytes() for l in range(h.info.levels)] == [second.smoother(l)["coef"].tobytes() for l in range(h.info.levels)]
        assert int(h.info.bytes) == int(second.info.bytes)
    finally:
        for x in (h, two, second):
            x.free()
        da.free()


def lib_set(api, h, opts):
    return api.lib.spmvHipAmgSetSmoother(C.byref(h.handle), C.byref(h.source.handle), None if opts is None else C.byref(opts))


# ------------------------------------------------------------------------------------------------------------ refusals
def _raw(obj):
    return bytes(C.string_at(C.addressof(obj), C.sizeof(obj)))


def _nonfinite_row():
    """path(12) with one diagonal per row; row 5 gets a tiny diagonal and a huge neighbour: |dinv| * sum|a| overflows"""
    A = sa.with_one_diagonal(*ar.path(12), seed=50)
    AS = A[4].copy()
    irp = A[2].astype(np.int64)
    for p in range(irp[5], irp[6]):
        AS[p] = 1e-300 if int(A[3][p]) == 5 else 1e300
    return A[:4] + (AS,)


def test_refusals_leave_the_hierarchy_and_the_view_untouched(api, capfd):
    lib = api.lib
    r = np.random.default_rng(14).standard_normal(LAP[0])
    da, other = _up(api, LAP), _up(api, LAP)
    gone = _up(api, LAP)
    gone.free()
    h = da.amg(coarseRows=8, smoothed=True)
    h.set_smoother(nu1=2, nu2=2)
    info = api.spmvAmgSmootherInfo()
    C.memset(C.addressof(info), 0x5A, C.sizeof(info))
    try:
        z0, view0, bytes0, info0, hm0 = h.apply(r).tobytes(), _view_blob(h), int(h.info.bytes), _raw(info), _raw(h.handle)
        HM, HA, O = C.byref(h.handle), C.byref(da.handle), api.spmvAmgSmootherOpts
        cheb = api.SPMV_AMG_SMOOTHER_CHEBYSHEV
        good = O(cheb, 3, 3, 3, 4.0, 1.0)
        set_ = lib.spmvHipAmgSetSmoother
        capfd.readouterr()
        assert set_(None, HA, C.byref(good)) != 0 and set_(HM, None, C.byref(good)) != 0, "NULL"
        assert set_(C.byref(gone.handle), HA, C.byref(good)) != 0 and set_(HM, C.byref(gone.handle), C.byref(good)) != 0, "not live"
        assert set_(HA, HA, C.byref(good)) != 0, "dM is no hierarchy"
        assert set_(HM, C.byref(other.handle), C.byref(good)) != 0, "dA is not the source"
        assert set_(HM, HM, C.byref(good)) != 0, "dA is a hierarchy"
        capfd.readouterr()
        for kind in (2, -1, 99):
            assert set_(HM, HA, C.byref(O(kind, 0, 0, 0, 0.0, 0.0))) != 0, kind
        assert capfd.readouterr().err.count("kind") == 3
        for bad in (1.0, 0.5, -4.0, np.inf, -np.inf, np.nan):
            assert set_(HM, HA, C.byref(O(cheb, 0, 0, 0, bad, 0.0))) != 0, bad
        assert capfd.readouterr().err.count("eigRatio") == 6
        for bad in (-1.0, np.inf, -np.inf, np.nan):
            assert set_(HM, HA, C.byref(O(cheb, 0, 0, 0, 0.0, bad))) != 0, bad
        assert capfd.readouterr().err.count("lambdaScale") == 4
        for nus in ((65, 0, 0), (0, 65, 0), (0, 0, 65), (0xFFFFFFFE, 0, 0)):
            assert set_(HM, HA, C.byref(O(cheb, *nus, 0.0, 0.0))) != 0, nus
            assert set_(HM, HA, C.byref(O(api.SPMV_AMG_SMOOTHER_JACOBI, *nus, 0.0, 0.0))) != 0, nus
        assert capfd.readouterr().err.count("sweeps") == 8
        # the view
        view = lib.spmvHipAmgSmoother
        for level in (h.info.levels, 99, 0xFFFFFFFF):
            assert view(HM, level, C.byref(info)) != 0, level
        assert view(HA, 0, C.byref(info)) != 0 and view(C.byref(gone.handle), 0, C.byref(info)) != 0 and view(None, 0, C.byref(info)) != 0
        assert view(HM, 0, None) != 0
        assert _raw(info) == info0 and _raw(h.handle) == hm0
        _check = lib.spmvHipAmgInfo(HM, C.byref(h.info))
        assert _check == 0
        assert (h.apply(r).tobytes(), _view_blob(h), int(h.info.bytes)) == (z0, view0, bytes0), "nothing moved"
        # the largest degree is taken
        assert set_(HM, HA, C.byref(O(cheb, 64, 64, api.SPMV_AMG_NO_SWEEPS, 0.0, 0.0))) == 0
        assert h.smoother(0)["coef"].shape == (64, 2) and h.smoother(h.info.levels - 1)["coef"].shape == (0, 2)
    finally:
        h.free()
        other.free()
        da.free()


def test_a_level_without_a_finite_rho_is_refused_and_a_refresh_recovers(api, capfd):
    bad = _nonfinite_row()
    good = bad[:4] + (sa.with_one_diagonal(*ar.path(12), seed=50)[4],)
    r = np.random.default_rng(15).standard_normal(bad[0])
    # the call itself: a plain hierarchy never looked at its row sums
    dbad = _up(api, bad)
    hb = dbad.amg(coarseRows=2)
    try:
        z0, view0 = hb.apply(r).tobytes(), _view_blob(hb)
        capfd.readouterr()
        with pytest.raises(api.SpmvHipError):
            hb.set_smoother(nu1=2, nu2=2)
        assert "row 5 of level 0" in capfd.readouterr().err
        assert (hb.apply(r).tobytes(), _view_blob(hb)) == (z0, view0)
        hb.set_smoother("jacobi", nu1=2)                             # Jacobi needs no rho
    finally:
        hb.free()
        dbad.free()
    # the refresh
    levels, o = ar.setup_ref(good, coarseRows=2)
    sm = cr.smoother(o, nu1=2, nu2=2)
    da = _up(api, good)
    h = da.amg(coarseRows=2)
    try:
        h.set_smoother(nu1=2, nu2=2)
        da.update_values(bad[4])
        capfd.readouterr()
        with pytest.raises(api.SpmvHipError):
            h.refresh_from(da)
        assert "row 5 of level 0" in capfd.readouterr().err
        da.update_values(good[4])
        h.refresh_from(da)
        _check_tables(h, levels, sm, "refreshed back")
        _same(h.apply(r), cr.cycle_ref(levels, o, r, sm), "the cycle after the recovery")
    finally:
        h.free()
        da.free()
