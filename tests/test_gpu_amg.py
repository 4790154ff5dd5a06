"""Aggregation multigrid on the device (spmvHipAggregateCSR, spmvHipAmgSetup / Refresh / Apply, and the hierarchy as dM of
the Krylov solvers) against tests/amg_ref.py: aggregate ids word for word, every level's IRP / JA / AS / dinv as bits, the
cycle's z as bits (special values, -0.0, misaligned vectors, a captured replay), the three solvers with the hierarchy as
preconditioner as bits with the reference loops, the refresh against a fresh setup, every refusal, and device memory."""
import ctypes as C

import numpy as np
import pytest

import amg_ref as ar
import spgemm_ref as sr
from amg_gpu import _down, _same, _solve_and_compare, _special_r, _up, cycle_launches
from bits import assert_same_bits
from gmres_ref import gmres_ref
from ilu0_ref import ilu0_levels
from krylov_ref import Csr, bicgstab_ref, cg_ref
from test_amg_abi import GRAPHS, KRYLOV_OPTS, KRYLOV_TOL, krylov_problem

pytestmark = pytest.mark.gpu

LAP = sr.laplacian7(12, 10, 8)                                  # 960 rows
SEEDS = (0, 0x9E3779B9)


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
    api.set_variant("spmvHipAggregateCSR", 16)
    api.set_variant("hipSpCGCSR", 16)


@pytest.fixture(scope="module")
def krylov(api):
    """the Laplacian of the CPU test, its right-hand side, the reference hierarchy and the device one"""
    A, b = krylov_problem()
    ref = ar.AmgCsr(A, **KRYLOV_OPTS)
    da = _up(api, A)
    h = da.amg(**KRYLOV_OPTS)
    yield A, b, ref, da, h
    h.free()
    da.free()


def _with_values(M, IRP, JA):
    return M, M, IRP, JA, np.ones(JA.size)


def test_device_memory_comes_back(api):
    """(first in the file: the library is finalised here, and no other test's handles are alive yet)"""
    import torch
    A = sr.laplacian7(24, 24, 16)
    free = []
    for _ in range(5):
        da = _up(api, A)
        h = da.amg(coarseRows=64)
        h.refresh_from(da)
        h.apply(np.ones(A[0]))
        da.free()                                                   # the source first: a hierarchy keeps no pointer to it
        h.free()
        api.spmvHipFinalize()
        api.spmvHipInit(0)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert min(free[2:]) >= free[1] - (8 << 20) and free[-1] >= free[1] - (8 << 20), free


# --------------------------------------------------------------------------------------------------------- aggregation
@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_aggregate_ids_are_the_loops(api, name, seed, K):
    M, IRP, JA = GRAPHS[name]
    api.set_variant("spmvHipAggregateCSR", K)
    da = _up(api, _with_values(M, IRP, JA))
    try:
        ids, info = da.aggregate(seed)
        want, roots, _ = ar.aggregate_ref(M, IRP, JA, seed, detail=True)
        assert np.array_equal(ids, want), (name, np.flatnonzero(ids != want)[:8])
        assert info.aggregates == len(roots)
        sizes = np.bincount(want.astype(np.int64)) if M else np.zeros(1, dtype=np.int64)
        assert (info.maxAggRows, info.minAggRows) == (int(sizes.max()), int(sizes.min()))
        assert info.longRows == (1 if name.startswith("star") else 0)
        stored = set(zip(np.repeat(np.arange(M), np.diff(IRP.astype(np.int64))).tolist(), JA.astype(np.int64).tolist()))
        tried = M == 0 or int(np.diff(IRP.astype(np.int64)).max()) <= 64
        assert info.symmetric == int(tried and all((j, i) in stored for i, j in stored)), "the symmetry check, tried on short rows"
        if M:
            assert info.hostChecks == -(-info.rounds // K) and info.rounds >= 1
        if name == "path70":
            assert info.rounds > 1
    finally:
        da.free()


def test_distance_two_through_a_retired_vertex(api):
    seed = ar.middle_first_seed()
    M, IRP, JA = ar.path(5)
    da = _up(api, _with_values(M, IRP, JA))
    try:
        ids, info = da.aggregate(seed)
        assert ids.tolist() == ar.aggregate_ref(M, IRP, JA, seed).tolist() == [0, 0, 0, 1, 1]
        assert info.rounds == 2
    finally:
        da.free()


# ----------------------------------------------------------------------------------------------------------- hierarchy
def _check_levels(api, h, levels, what):
    assert h.info.levels == len(levels), what
    for l, lv in enumerate(levels):
        A = lv["A"]
        view, agg, dinv = h.level(l)
        assert (int(view.M), int(view.NZ)) == (A[0], A[3].size) == (h.info.rows[l], h.info.nnz[l]), (what, l)
        _same(_down(api, dinv, A[0], np.float64), lv["dinv"], f"{what}: dinv of level {l}")
        if l:
            got = (A[0], A[1], _down(api, view.IRP, A[0] + 1, np.uint32), _down(api, view.JA, A[3].size, np.uint32),
                   _down(api, view.AS, A[3].size, np.float64))
            sr.same_bits(got, A, f"{what}: level {l}")
        if "agg" in lv:
            assert np.array_equal(_down(api, agg, A[0], np.uint32), lv["agg"]), (what, l)
            assert h.info.aggregates[l] == int(lv["agg"].max()) + 1
        else:
            assert agg is None and h.info.aggregates[l] == 0
    nnz = [lv["A"][3].size for lv in levels]
    assert h.info.opComplexity == pytest.approx(sum(nnz) / max(nnz[0], 1))


def test_every_level_is_the_reference(api):
    levels, _ = ar.setup_ref(LAP, coarseRows=8)
    assert len(levels) >= 3
    da = _up(api, LAP)
    h = da.amg(coarseRows=8)
    try:
        _check_levels(api, h, levels, "laplacian")
        assert h.info.bytes > 0 and h.info.ms > 0
    finally:
        h.free()
        da.free()


def test_one_level_and_isolated_vertices_stop_the_build(api):
    da = _up(api, LAP)
    h = da.amg(maxLevels=1)
    try:
        assert h.info.levels == 1 and h.info.aggregates[0] == 0
    finally:
        h.free()
        da.free()
    M = 40
    D = (M, M, np.arange(M + 1, dtype=np.uint64), np.arange(M, dtype=np.uint64), np.arange(1.0, M + 1))
    dd = _up(api, D)
    h = dd.amg(coarseRows=8)
    try:
        assert h.info.levels == 1, "nAgg == M stops the build"
        r = np.arange(1.0, M + 1)
        levels, o = ar.setup_ref(D, coarseRows=8)
        assert len(levels) == 1
        _same(h.apply(r), ar.cycle_ref(levels, o, r), "diagonal matrix")
    finally:
        h.free()
        dd.free()


def test_adopted_eight_byte_row_pointers_and_unit_values(api):
    M, _, IRP, JA, AS = LAP
    unit = (M, M, IRP, JA, np.full(JA.size, 0.5))
    levels_u, _ = ar.setup_ref(unit, coarseRows=8)
    du = _up(api, unit)
    hu = du.amg(coarseRows=8)
    try:
        v = C.c_double()
        assert api.lib.spmvHipUnitValue(C.byref(du.handle), C.byref(v)) == 1 and v.value == 0.5, "the source is a unit-value handle"
        _check_levels(api, hu, levels_u, "unit values")
    finally:
        hu.free()
        du.free()
    bufs = [api.DeviceBuffer(8 * (M + 1)).up(IRP.astype(np.uint64)), api.DeviceBuffer(4 * JA.size).up(JA.astype(np.uint32)),
            api.DeviceBuffer(8 * JA.size).up(AS)]
    dm = api.DeviceMatrix()
    dm.keep = bufs
    assert api.lib.spmvHipAdoptCSR(C.byref(dm.handle), M, M, JA.size, bufs[0].ptr, 8, bufs[1].ptr, bufs[2].ptr, None) == 0
    h = dm.amg(coarseRows=8)
    try:
        _check_levels(api, h, ar.setup_ref(LAP, coarseRows=8)[0], "adopted, 8-byte row pointers")
    finally:
        h.free()
        dm.free()


# --------------------------------------------------------------------------------------------------------------- cycle
SWEEPS = [(0, 0, 1), (1, 1, 1), (2, 1, 3), (0, 2, 1)]
DEPTHS = {1: dict(maxLevels=1), 2: dict(coarseRows=8, maxLevels=2), 3: dict(coarseRows=8, maxLevels=3)}


@pytest.mark.parametrize("depth", list(DEPTHS))
@pytest.mark.parametrize("nu", SWEEPS)
def test_cycle_bits(api, nu, depth):
    kw = dict(DEPTHS[depth], nu1=nu[0], nu2=nu[1], nuCoarse=nu[2])
    levels, o = ar.setup_ref(LAP, **kw)
    assert len(levels) == depth
    da = _up(api, LAP)
    h = da.amg(**kw)
    try:
        for what, r in (("random", np.random.default_rng(8).standard_normal(LAP[0])), ("special", _special_r(LAP[0]))):
            _same(h.apply(r), ar.cycle_ref(levels, o, r), f"{what} r, sweeps {nu}, {depth} levels")
    finally:
        h.free()
        da.free()


def test_negative_zero_before_the_correction(api):
    """r = -0.0 everywhere: the pre-smoothed z is -0.0 in every row and the coarse e is +0.0 (a serial-order sum starts at
    +0.0), so the gather z + e[agg] gives +0.0 -- the bits the reference states"""
    r = np.full(LAP[0], -0.0)
    one, o1 = ar.setup_ref(LAP, maxLevels=1, nuCoarse=1)
    assert np.all(np.signbit(ar.cycle_ref(one, o1, r))), "z before the correction is -0.0"
    for kw in (dict(coarseRows=8, maxLevels=2, nu1=1, nu2=0, nuCoarse=1), dict(coarseRows=8, maxLevels=3, nu1=1, nu2=1, nuCoarse=2)):
        levels, o = ar.setup_ref(LAP, **kw)
        want = ar.cycle_ref(levels, o, r)
        da = _up(api, LAP)
        h = da.amg(**kw)
        try:
            _same(h.apply(r), want, f"-0.0, {kw}")
        finally:
            h.free()
            da.free()


def test_misaligned_vectors_and_a_captured_replay(api):
    import torch
    levels, o = ar.setup_ref(LAP, coarseRows=8)
    M = LAP[0]
    r = np.random.default_rng(9).standard_normal(M)
    want = ar.cycle_ref(levels, o, r)
    da = _up(api, LAP)
    h = da.amg(coarseRows=8)
    try:
        rb, zb = torch.zeros(M + 1, dtype=torch.float64, device="cuda"), torch.zeros(M + 1, dtype=torch.float64, device="cuda")
        rv, zv = rb[1:], zb[1:]
        assert rv.data_ptr() % 16 == 8
        rv.copy_(torch.from_numpy(r))
        h.apply(rv, out=zv)
        _same(zv.cpu().numpy(), want, "8-byte aligned vectors")
        # capture one Apply, replay it on another r
        api.lib.spmvHipSetSync(0)
        s = torch.cuda.Stream()
        api.lib.spmvHipSetStream(C.c_void_p(s.cuda_stream))
        rt, zt = torch.from_numpy(r).cuda(), torch.zeros(M, dtype=torch.float64, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                h.apply(rt, out=zt)
        r2 = np.random.default_rng(10).standard_normal(M)
        rt.copy_(torch.from_numpy(r2))
        g.replay()
        torch.cuda.synchronize()
        _same(zt.cpu().numpy(), ar.cycle_ref(levels, o, r2), "captured replay")
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        h.free()
        da.free()


# -------------------------------------------------------------------------------------------------------------- Krylov
def test_cg_with_the_hierarchy(api, krylov):
    A, b, ref, da, h = krylov
    want = cg_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200)
    info = _solve_and_compare(da, b, h, "cg", want, KRYLOV_TOL)
    plain = cg_ref(Csr(A[0], A[2], A[3], A[4]), b, np.zeros(A[0]), KRYLOV_TOL, 200)
    assert info.iterations == want[2] < plain[2]
    # CG's own kernels: 4 before the loop and 6 per enqueued iteration (whole batches of K = 16), as a solve without dM
    # shows; with dM every M^-1 (one before the loop, one per iteration) adds the cycle, a dot pass and its finish
    enq = lambda it: min(200, -(-it // 16) * 16)
    _, pinfo = da.cg(b, tol=KRYLOV_TOL, maxiter=200)
    assert pinfo.launches == 4 + 6 * enq(plain[2])
    cycle = cycle_launches(1, 1, 8, h.info.levels)                  # the default sweeps of KRYLOV_OPTS
    assert set(KRYLOV_OPTS) == {"coarseRows"} and h.info.levels >= 3
    assert info.launches == 4 + 6 * enq(want[2]) + (enq(want[2]) + 1) * (cycle + 2)


def test_bicgstab_with_the_hierarchy(api, krylov):
    A, b, ref, da, h = krylov
    _solve_and_compare(da, b, h, "bicgstab", bicgstab_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200), KRYLOV_TOL)


def test_gmres_with_the_hierarchy(api, krylov):
    A, b, ref, da, h = krylov
    _solve_and_compare(da, b, h, "gmres", gmres_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200, 5), KRYLOV_TOL, restart=5)


def test_cycles_queued_past_the_stop_change_nothing(api, krylov):
    A, b, ref, da, h = krylov
    want = cg_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200)
    assert want[2] % 16, "the stop falls inside a batch of K = 16: queued cycles run after it"
    xs = []
    for K in (1, 16):
        api.set_variant("hipSpCGCSR", K)
        x, info = da.cg(b, precond=h, tol=KRYLOV_TOL, maxiter=200)
        assert info.iterations == want[2]
        xs.append(x)
    assert_same_bits(xs[0], want[0], "K = 1")
    assert_same_bits(xs[1], xs[0], "K = 16 against K = 1")


SOLVERS = {"cg": (cg_ref, {}, ()), "bicgstab": (bicgstab_ref, {}, ()), "gmres": (gmres_ref, dict(restart=5), (5,))}


@pytest.mark.parametrize("method", list(SOLVERS))
def test_ilu0_and_no_preconditioner_keep_their_bits(api, krylov, method):
    """the solvers' dispatch on the kind of dM left the two older kinds alone: the bits of tests/krylov_ref.py and
    tests/gmres_ref.py, with the hierarchy of the same matrix alive beside them"""
    A, b, ref, da, h = krylov
    M = A[0]
    loop, kw, tail = SOLVERS[method]
    F = ilu0_levels(M, A[2].astype(np.int64), A[3].astype(np.int64), A[4])
    dm = _up(api, A)
    try:
        dm.ilu0()
        for what, precond, csr in (("no dM", None, Csr(M, A[2], A[3], A[4])), ("ILU(0)", dm, Csr(M, A[2], A[3], A[4], F=F))):
            want = loop(csr, b, np.zeros(M), KRYLOV_TOL, 200, *tail)
            x, info = getattr(da, method)(b, precond=precond, tol=KRYLOV_TOL, maxiter=200, history=True, **kw)
            assert (info.status, info.iterations) == (want[1], want[2]), (method, what)
            assert_same_bits(x, want[0], f"{method}, {what}: x")
            assert_same_bits(info.history, want[3], f"{method}, {what}: history")
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------------------- refresh
def test_refresh_equals_a_fresh_setup(api):
    M = LAP[0]
    new = LAP[4] * (1.0 + 0.25 * np.random.default_rng(11).random(LAP[4].size))
    B = LAP[:4] + (new,)
    levels, o = ar.setup_ref(B, coarseRows=8)
    da = _up(api, LAP)
    h = da.amg(coarseRows=8)
    other = _up(api, LAP)
    try:
        da.update_values(new)
        h.refresh_from(da)
        _check_levels(api, h, levels, "refreshed")
        r = np.random.default_rng(12).standard_normal(M)
        _same(h.apply(r), ar.cycle_ref(levels, o, r), "cycle after the refresh")
        with pytest.raises(api.SpmvHipError):
            h.refresh_from(other)
    finally:
        h.free()
        other.free()
        da.free()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(api, krylov, capfd):
    A, b, ref, da, h = krylov
    M = A[0]
    lib = api.lib
    other = _up(api, A)
    rect = _up(api, sr.random_csr(np.random.default_rng(13), 6, 5, 2))
    nodiag = _up(api, (3, 3, np.array([0, 1, 2, 3], np.uint64), np.array([1, 2, 0], np.uint64), np.ones(3)))
    twodiag = _up(api, (2, 2, np.array([0, 2, 3], np.uint64), np.array([0, 0, 1], np.uint64), np.ones(3)))
    ell = api.csr_to_ell_device(other, False)
    dx, dy = api.DeviceVector(M).up(b), api.DeviceVector(M)
    out, info = api.spmat(), api.spmvAmgInfo()
    agg = api.DeviceBuffer(4 * M)
    gone = _up(api, A)
    gone.free()
    try:
        HA, HM = C.byref(da.handle), C.byref(h.handle)
        assert lib.spmvHipAggregateCSR(C.byref(gone.handle), None, agg.ptr, None) != 0, "a freed handle"
        assert lib.spmvHipAmgSetup(C.byref(gone.handle), None, C.byref(out), C.byref(info)) != 0, "a freed handle"
        assert lib.spmvHipAmgApply(HM, C.byref(gone.handle), dx.ptr, dy.ptr) != 0, "a freed dA"
        assert lib.spmvHipAmgRefresh(HM, C.byref(gone.handle)) != 0, "a freed dA"
        for dm in (rect, ell):
            assert lib.spmvHipAggregateCSR(C.byref(dm.handle), None, agg.ptr, None) != 0
            assert lib.spmvHipAmgSetup(C.byref(dm.handle), None, C.byref(out), C.byref(info)) != 0
        assert lib.spmvHipAggregateCSR(HA, None, None, None) != 0, "NULL dAgg"
        assert lib.spmvHipAggregateCSR(HM, None, agg.ptr, None) != 0, "a hierarchy is no matrix"
        assert lib.spmvHipAmgSetup(HA, None, None, None) != 0 and lib.spmvHipAmgSetup(None, None, C.byref(out), None) != 0
        assert lib.spmvHipAmgSetup(HA, None, HA, None) != 0, "dM == dA"
        for dm in (nodiag, twodiag):
            assert lib.spmvHipAmgSetup(C.byref(dm.handle), None, C.byref(out), C.byref(info)) != 0, "STORED rule"
        bad = api.spmvAmgOpts(0, 0, 17, 0.0, 0, 0, 0)
        assert lib.spmvHipAmgSetup(HA, C.byref(bad), C.byref(out), None) != 0, "maxLevels"
        bad = api.spmvAmgOpts(0, 0, 0, -1.0, 0, 0, 0)
        assert lib.spmvHipAmgSetup(HA, C.byref(bad), C.byref(out), None) != 0, "omega"
        assert not out.dev and info.levels == 0, "outputs untouched"
        # Apply
        assert lib.spmvHipAmgApply(HM, C.byref(other.handle), dx.ptr, dy.ptr) != 0, "not the source"
        assert lib.spmvHipAmgApply(HA, HA, dx.ptr, dy.ptr) != 0, "not a hierarchy"
        assert lib.spmvHipAmgApply(HM, HA, None, dy.ptr) != 0 and lib.spmvHipAmgApply(HM, HA, dx.ptr, None) != 0
        assert lib.spmvHipAmgApply(None, HA, dx.ptr, dy.ptr) != 0 and lib.spmvHipAmgApply(HM, None, dx.ptr, dy.ptr) != 0
        assert lib.spmvHipAmgApply(HM, HA, dx.ptr, dx.ptr) != 0, "dR == dZ"
        assert lib.spmvHipAmgApply(HM, HA, dx.ptr, C.c_void_p(dx.ptr.value + 8)) != 0, "overlap"
        # sizes: the C entry point sees addresses only, so the lengths are refused where they are known
        import torch
        good = torch.zeros(M, dtype=torch.float64, device="cuda")
        for bad_r, bad_out in ((np.ones(M + 1), None), (np.ones(M - 1), None), (np.ones((M, 1)), None), (np.ones(M), good),
                               (torch.zeros(M + 1, dtype=torch.float64, device="cuda"), None),
                               (torch.zeros(M - 1, dtype=torch.float64, device="cuda"), good),
                               (good, torch.zeros(M - 1, dtype=torch.float64, device="cuda")),
                               (good, torch.zeros(M + 1, dtype=torch.float64, device="cuda")),
                               (good, torch.zeros(M, dtype=torch.float32, device="cuda")),
                               (good, torch.zeros(M, dtype=torch.float64)), (good, np.zeros(M)), (list(b), None), (None, None)):
            with pytest.raises(api.SpmvHipError):
                h.apply(bad_r, out=bad_out)
        assert not good.any().item(), "a refused Apply writes nothing"
        # refresh, level
        assert lib.spmvHipAmgRefresh(HA, HA) != 0 and lib.spmvHipAmgRefresh(HM, C.byref(other.handle)) != 0
        assert lib.spmvHipAmgLevel(HM, 99, None, None, None) != 0
        # a hierarchy is no matrix: SpMV, transposes, products and solves refuse it
        with pytest.raises(api.SpmvHipError):
            api.spmv("hipSpMVRowsCSR", h, dx, dy)
        assert lib.spmvHipEnqueueAutoRows(HM, dx.ptr, dy.ptr, None) != 0
        assert lib.spmvHipCsrTranspose(HM, C.byref(out)) != 0 and lib.spmvHipSpGEMM(HM, HA, None, C.byref(out), None) != 0
        assert lib.hipSpILU0CSR(HM) != 0
        # Krylov: a hierarchy of another source
        with pytest.raises(api.SpmvHipError):
            other.cg(b, precond=h, tol=1e-8, maxiter=5)
        with pytest.raises(api.SpmvHipError):
            other.gmres(b, precond=h, tol=1e-8, maxiter=5, restart=5)
        assert "multigrid hierarchy" in capfd.readouterr().err
    finally:
        for d in (other, rect, nodiag, twodiag, ell, dx, dy, agg):
            d.free()
