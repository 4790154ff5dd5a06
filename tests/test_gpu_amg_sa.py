"""Smoothed-aggregation multigrid on the device (spmvHipAmgSetupSmoothed, spmvHipAmgProlongator, and the smoothed hierarchy
under spmvHipAmgApply / Refresh and as dM of the Krylov solvers) against tests/amg_sa_ref.py, bits throughout: every level's
P / R / A / dinv / w, the cycle's z with the correction fused, split and mixed (special values, an odd M, misaligned vectors,
a captured replay), the launch count of a cycle, the three solvers, the stop, the refresh against a fresh setup with the
addresses kept, every refusal with its outputs compared as bytes, and device memory."""
import ctypes as C
import functools

import numpy as np
import pytest

import amg_ref as ar
import amg_sa_ref as sa
import spgemm_ref as sr
from amg_gpu import _bits, _blob, _down, _same, _solve_and_compare, _special_r, _up, cycle_launches
from bits import assert_same_bits
from gmres_ref import gmres_ref
from krylov_ref import Csr, bicgstab_ref, cg_ref
from test_amg_sa_abi import COUNTS, KRYLOV_OPTS, KRYLOV_TOL, krylov_problem

pytestmark = pytest.mark.gpu

LAP = sr.laplacian7(12, 10, 8)                                  # 960 rows; its P_0 has rows of 6 entries, its P_1 of 5
SEEDS = (0, 0x9E3779B9)
FUSED, MIXED, SPLIT_ABOVE_2, NEVER = 64, 5, 2, 0                # thresholds: all fused; P_0 split and P_1 fused; both split; both split
DEFAULT = NEVER                                                 # what the library starts with: the form that measured faster
THRESHOLDS = (FUSED, MIXED, SPLIT_ABOVE_2, NEVER)
GRAPHS = {name: sa.with_one_diagonal(*g, seed=n) for n, (name, g) in enumerate(ar.small_graphs().items())}
ODD = sa.with_one_diagonal(*(lambda a: (a[0], a[2], a[3]))(sr.laplacian7(11, 9, 7)), seed=40)      # 693 rows


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
    api.set_variant("spmvHipAmgApply", DEFAULT)
    api.set_variant("hipSpCGCSR", 16)


def _unfused(levels, threshold):
    """the levels whose correction takes two launches"""
    return sum(int(np.diff(lv["P"][2].astype(np.int64)).max()) > threshold for lv in levels[:-1])


def _level_arrays(api, h, l):
    """what the device holds for level l: A_l (below level 0), agg, dinv and, but for the last level, P, R, w"""
    view, agg, dinv = h.level(l)
    M, NZ = int(view.M), int(view.NZ)
    out = dict(M=M, NZ=NZ, dinv=_down(api, dinv, M, np.float64), agg=None if agg is None else _down(api, agg, M, np.uint32))
    if l:
        out["A"] = (M, M, _down(api, view.IRP, M + 1, np.uint32), _down(api, view.JA, NZ, np.uint32), _down(api, view.AS, NZ, np.float64))
    if l + 1 < h.info.levels:
        out["P"], out["R"], out["w"] = h.prolongator(l)
    return out


def _check_levels(api, h, levels, what):
    assert h.info.levels == len(levels), what
    for l, lv in enumerate(levels):
        A = lv["A"]
        got = _level_arrays(api, h, l)
        assert (got["M"], got["NZ"]) == (A[0], A[3].size) == (h.info.rows[l], h.info.nnz[l]), (what, l)
        _same(got["dinv"], lv["dinv"], f"{what}: dinv of level {l}")
        if l:
            sr.same_bits(got["A"], A, f"{what}: A of level {l}")
        if "agg" in lv:
            assert np.array_equal(got["agg"], lv["agg"]), (what, l)
            assert h.info.aggregates[l] == int(lv["agg"].max()) + 1
            sr.same_bits(got["P"], lv["P"], f"{what}: P of level {l}")
            sr.same_bits(got["R"], lv["R"], f"{what}: R of level {l}")
            assert _bits(got["w"]) == _bits(lv["w"]), (what, l, got["w"], lv["w"])
        else:
            assert got["agg"] is None and h.info.aggregates[l] == 0
    assert h.info.opComplexity == pytest.approx(sa.complexity(levels))


def test_device_memory_comes_back_after_twenty_setups(api):
    """(first in the file: no other test's handles are alive yet)"""
    import torch
    A = sr.laplacian7(20, 20, 16)
    da = _up(api, A)
    try:
        def once(use=False):
            h = da.amg(coarseRows=64, smoothed=True)
            kept = int(h.info.bytes)
            if use:
                h.refresh_from(da)
                h.apply(np.ones(A[0]))
            h.free()
            return kept
        once(True), once(True)                                       # (the library's own workspaces exist now)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        kept = [once() for _ in range(20)]
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        slack = 8 << 20
        assert sum(kept) > 2 * slack, "twenty leaked hierarchies would show"
        assert after >= before - slack, (before, after)
    finally:
        da.free()


# ----------------------------------------------------------------------------------------------------------- hierarchy
@pytest.mark.parametrize("omegaP", [None, 0.5])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["laplacian"] + list(GRAPHS))
def test_every_level_is_the_reference(api, name, seed, omegaP):
    A = LAP if name == "laplacian" else GRAPHS[name]
    levels, _ = sa.setup_ref(A, omegaP or 0.0, coarseRows=8, seed=seed)
    if name in ("laplacian", "laplacian12x10x8"):
        assert len(levels) >= 3
    da = _up(api, A)
    h = da.amg(coarseRows=8, seed=seed, smoothed=True, omegaP=omegaP)
    try:
        _check_levels(api, h, levels, name)
        assert (h.info.bytes > 0) == (A[0] > 0) and h.info.ms > 0
        if name == "laplacian" and omegaP is None:
            assert _bits(h.prolongator(0)[2]) == _bits(2.0 / 3.0)
    finally:
        h.free()
        da.free()


def test_adopted_eight_byte_row_pointers(api):
    M, _, IRP, JA, AS = LAP
    bufs = [api.DeviceBuffer(8 * (M + 1)).up(IRP.astype(np.uint64)), api.DeviceBuffer(4 * JA.size).up(JA.astype(np.uint32)),
            api.DeviceBuffer(8 * JA.size).up(AS)]
    dm = api.DeviceMatrix()
    dm.keep = bufs
    assert api.lib.spmvHipAdoptCSR(C.byref(dm.handle), M, M, JA.size, bufs[0].ptr, 8, bufs[1].ptr, bufs[2].ptr, None) == 0
    h = dm.amg(coarseRows=8, smoothed=True)
    try:
        levels, o = sa.setup_ref(LAP, coarseRows=8)
        _check_levels(api, h, levels, "adopted, 8-byte row pointers")
        r = np.random.default_rng(30).standard_normal(M)
        _same(h.apply(r), sa.cycle_ref(levels, o, r), "adopted: the cycle")
    finally:
        h.free()
        dm.free()


def test_bytes_count_the_kept_handles(api):
    da = _up(api, LAP)
    plain, smooth = da.amg(coarseRows=8), da.amg(coarseRows=8, smoothed=True)
    try:
        levels, _ = sa.setup_ref(LAP, coarseRows=8)
        extra = 0
        for lv in levels[:-1]:
            M, nAgg = lv["A"][0], lv["P"][1]
            AT = sr.spgemm_ref(lv["A"], lv["T"])
            extra += (M * 12 + (M + 1) * 4) * 2 + 2 * (AT[3].size * 12 + (M + 1) * 4)          # T and D; A T and D (A T)
        assert smooth.info.bytes >= extra and smooth.info.bytes > plain.info.bytes
        assert smooth.info.tempBytes > 0
    finally:
        plain.free()
        smooth.free()
        da.free()


# --------------------------------------------------------------------------------------------------------------- cycle
SWEEPS = [(0, 0, 1), (1, 1, 1), (2, 1, 3), (0, 2, 1)]
DEPTHS = {1: dict(maxLevels=1), 2: dict(coarseRows=8, maxLevels=2), 3: dict(coarseRows=8, maxLevels=3)}
CYCLE_CASES = [(d, t) for d in DEPTHS for t in (THRESHOLDS if d > 1 else (FUSED,))]


@functools.lru_cache(maxsize=None)
def _lap_levels(depth):
    levels, _ = sa.setup_ref(LAP, **DEPTHS[depth])
    assert len(levels) == depth
    return levels


def test_the_thresholds_split_the_levels_as_named():
    levels = _lap_levels(3)
    assert [_unfused(levels, t) for t in THRESHOLDS] == [0, 1, 2, 2]


@pytest.mark.parametrize("depth,threshold", CYCLE_CASES)
@pytest.mark.parametrize("nu", SWEEPS)
def test_cycle_bits(api, nu, depth, threshold):
    kw = dict(DEPTHS[depth], nu1=nu[0], nu2=nu[1], nuCoarse=nu[2])
    levels, o = _lap_levels(depth), ar._opts(kw)
    api.set_variant("spmvHipAmgApply", threshold)
    da = _up(api, LAP)
    h = da.amg(smoothed=True, **kw)
    api.set_variant("spmvHipAmgApply", FUSED if threshold != FUSED else NEVER)      # (read at the setup: this changes nothing for h)
    try:
        for what, r in (("random", np.random.default_rng(8).standard_normal(LAP[0])), ("special", _special_r(LAP[0]))):
            _same(h.apply(r), sa.cycle_ref(levels, o, r), f"{what} r, sweeps {nu}, {depth} levels, threshold {threshold}")
    finally:
        h.free()
        da.free()


def test_negative_zero_before_the_correction(api):
    """r = -0.0 everywhere: z before the correction is -0.0 in every row, P e is a serial-order sum from +0.0, and z + P e is
    +0.0 -- fused and split alike"""
    r = np.full(LAP[0], -0.0)
    kw = dict(coarseRows=8, maxLevels=3, nu1=1, nu2=0, nuCoarse=2)
    levels, o = sa.setup_ref(LAP, **kw)
    want = sa.cycle_ref(levels, o, r)
    assert not np.signbit(want).any()
    da = _up(api, LAP)
    try:
        for threshold in (FUSED, NEVER):
            api.set_variant("spmvHipAmgApply", threshold)
            h = da.amg(smoothed=True, **kw)
            try:
                _same(h.apply(r), want, f"-0.0, threshold {threshold}")
            finally:
                h.free()
    finally:
        da.free()


@pytest.mark.parametrize("threshold", [FUSED, NEVER])
def test_odd_rows_misaligned_vectors_and_a_captured_replay(api, threshold):
    import torch
    levels, o = sa.setup_ref(ODD, coarseRows=8)
    M = ODD[0]
    assert M % 2 == 1 and len(levels) >= 3 and any(lv["A"][0] % 2 for lv in levels[1:-1])
    r = _special_r(M)
    want = sa.cycle_ref(levels, o, r)
    api.set_variant("spmvHipAmgApply", threshold)
    da = _up(api, ODD)
    h = da.amg(coarseRows=8, smoothed=True)
    try:
        _same(h.apply(r), want, "odd M")
        rb, zb = torch.zeros(M + 1, dtype=torch.float64, device="cuda"), torch.zeros(M + 1, dtype=torch.float64, device="cuda")
        rv, zv = rb[1:], zb[1:]
        assert rv.data_ptr() % 16 == 8 and zv.data_ptr() % 16 == 8
        rv.copy_(torch.from_numpy(r))
        h.apply(rv, out=zv)
        _same(zv.cpu().numpy(), want, "vectors at odd 8-byte offsets")
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
        _same(zt.cpu().numpy(), sa.cycle_ref(levels, o, r2), "captured replay")
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        h.free()
        da.free()


# -------------------------------------------------------------------------------------------------------------- Krylov
@pytest.fixture(scope="module")
def krylov(api):
    """the Laplacian of the CPU test, its right-hand side, the reference hierarchy and the device ones: h fused, h0 set up
    with the library's default (never fused)"""
    A, b = krylov_problem((12, 10, 8))
    ref = sa.SaCsr(A, **KRYLOV_OPTS)
    da = _up(api, A)
    h0 = da.amg(smoothed=True, **KRYLOV_OPTS)
    api.set_variant("spmvHipAmgApply", FUSED)
    h = da.amg(smoothed=True, **KRYLOV_OPTS)
    api.set_variant("spmvHipAmgApply", DEFAULT)
    yield A, b, ref, da, h, h0
    h0.free()
    h.free()
    da.free()


def test_cg_with_the_smoothed_hierarchy_and_the_launches_of_a_cycle(api, krylov):
    A, b, ref, da, h, h0 = krylov
    want = cg_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200)
    assert want[2] == COUNTS[(12, 10, 8)][2] < COUNTS[(12, 10, 8)][1]
    assert h.info.levels == h0.info.levels == len(ref.levels) >= 3 and set(KRYLOV_OPTS) == {"coarseRows"}
    enq = lambda it: min(200, -(-it // 16) * 16)
    for hier, unfused in ((h, 0), (h0, len(ref.levels) - 1)):
        info = _solve_and_compare(da, b, hier, "cg", want, KRYLOV_TOL)
        assert info.iterations == want[2]
        # CG's own kernels: 4 before the loop and 6 per enqueued iteration (whole batches of K = 16); every M^-1 (one before
        # the loop, one per iteration) adds the cycle, a dot pass and its finish
        cycle = cycle_launches(1, 1, 8, hier.info.levels, unfused)
        assert info.launches == 4 + 6 * enq(want[2]) + (enq(want[2]) + 1) * (cycle + 2), (unfused, info.launches)


def test_bicgstab_with_the_smoothed_hierarchy(api, krylov):
    A, b, ref, da, h, h0 = krylov
    _solve_and_compare(da, b, h, "bicgstab", bicgstab_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200), KRYLOV_TOL)


def test_gmres_with_the_smoothed_hierarchy(api, krylov):
    A, b, ref, da, h, h0 = krylov
    _solve_and_compare(da, b, h0, "gmres", gmres_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200, 5), KRYLOV_TOL, restart=5)
    _solve_and_compare(da, b, h, "gmres", gmres_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200, 5), KRYLOV_TOL, restart=5)


def test_cycles_queued_past_the_stop_write_nothing(api, krylov):
    A, b, ref, da, h, h0 = krylov
    want = cg_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200)
    assert want[2] % 16, "the stop falls inside a batch of K = 16: queued cycles run after it"
    for hier in (h, h0):
        xs = []
        for K in (1, 16):
            api.set_variant("hipSpCGCSR", K)
            x, info = da.cg(b, precond=hier, tol=KRYLOV_TOL, maxiter=200)
            assert info.iterations == want[2]
            xs.append(x)
        assert_same_bits(xs[0], want[0], "K = 1")
        assert_same_bits(xs[1], xs[0], "K = 16 against K = 1")


def test_the_block_solvers_still_refuse_a_hierarchy(api, krylov, capfd):
    A, b, ref, da, h, h0 = krylov
    B = np.stack([b, 2.0 * b], axis=1)
    for method in ("cg_block", "bicgstab_block"):
        with pytest.raises(api.SpmvHipError):
            getattr(da, method)(B, precond=h, tol=1e-8, maxiter=5)
    assert "multigrid hierarchy" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------------------- refresh
def _addresses(api, h):
    out = []
    for l in range(h.info.levels):
        view, agg, dinv = h.level(l)
        out += [C.cast(p, C.c_void_p).value for p in (view.IRP, view.JA, view.AS)] + [agg, dinv]
        if l + 1 < h.info.levels:
            P, R = api.spmat(), api.spmat()
            assert api.lib.spmvHipAmgProlongator(C.byref(h.handle), l, C.byref(P), C.byref(R), None) == 0
            out += [C.cast(p, C.c_void_p).value for v in (P, R) for p in (v.IRP, v.JA, v.AS)]
    return out


def _new_values():
    """other values on LAP's pattern, the diagonal scaled row by row: rho, and with it w, moves on every level"""
    rng = np.random.default_rng(11)
    new = LAP[4] * (1.0 + 0.25 * rng.random(LAP[4].size))
    rows = sr.si.row_of_entry(LAP[2])
    diag = LAP[3].astype(np.int64) == rows
    new[diag] = new[diag] * (1.0 + rng.random(int(diag.sum())))
    return LAP[:4] + (new,)


@pytest.mark.parametrize("omegaP", [None, 0.5])
def test_refresh_equals_a_fresh_setup_at_the_same_addresses(api, omegaP):
    M = LAP[0]
    B = _new_values()
    old, _ = sa.setup_ref(LAP, omegaP or 0.0, coarseRows=8)
    levels, o = sa.setup_ref(B, omegaP or 0.0, coarseRows=8)
    if omegaP is None:
        assert all(_bits(a["w"]) != _bits(b["w"]) for a, b in zip(old[:-1], levels[:-1])), "w moves"
    da, db = _up(api, LAP), _up(api, B)
    h = da.amg(coarseRows=8, smoothed=True, omegaP=omegaP)
    fresh = db.amg(coarseRows=8, smoothed=True, omegaP=omegaP)
    try:
        where = _addresses(api, h)
        da.update_values(B[4])
        h.refresh_from(da)
        assert _addresses(api, h) == where
        _check_levels(api, h, levels, "refreshed")
        _check_levels(api, fresh, levels, "fresh")
        r = np.random.default_rng(12).standard_normal(M)
        z = h.apply(r)
        _same(z, sa.cycle_ref(levels, o, r), "cycle after the refresh")
        assert_same_bits(z, fresh.apply(r), "refreshed against fresh")
        with pytest.raises(api.SpmvHipError):
            h.refresh_from(db)
    finally:
        fresh.free()
        h.free()
        db.free()
        da.free()


def test_refresh_of_a_plain_hierarchy_is_unchanged_and_its_view_is_the_unit_prolongator(api):
    B = _new_values()
    levels, o = ar.setup_ref(B, coarseRows=8)
    da = _up(api, LAP)
    h = da.amg(coarseRows=8)
    try:
        da.update_values(B[4])
        h.refresh_from(da)
        r = np.random.default_rng(13).standard_normal(LAP[0])
        _same(h.apply(r), ar.cycle_ref(levels, o, r), "plain hierarchy after its refresh")
        for l, lv in enumerate(levels[:-1]):
            P, R, w = h.prolongator(l)
            sr.same_bits(P, lv["P"], f"unit P of level {l}")
            sr.same_bits(R, lv["R"], f"its R of level {l}")
            assert _bits(w) == _bits(0.0)
            got = _level_arrays(api, h, l + 1)["A"]
            sr.same_bits(got, levels[l + 1]["A"], f"A of level {l + 1}")
    finally:
        h.free()
        da.free()


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


def test_refusals_leave_their_outputs_untouched(api, krylov, capfd):
    A, b, ref, da, h, h0 = krylov
    lib = api.lib
    other = _up(api, A)
    rect = _up(api, sr.random_csr(np.random.default_rng(13), 6, 5, 2))
    nodiag = _up(api, (3, 3, np.array([0, 1, 2, 3], np.uint64), np.array([1, 2, 0], np.uint64), np.ones(3)))
    twodiag = _up(api, (2, 2, np.array([0, 2, 3], np.uint64), np.array([0, 0, 1], np.uint64), np.ones(3)))
    overflow = _up(api, _nonfinite_row())
    ell = api.csr_to_ell_device(other, False)
    gone = _up(api, A)
    gone.free()
    out, info, P, R, w = api.spmat(), api.spmvAmgInfo(), api.spmat(), api.spmat(), C.c_double(123.0)
    for obj in (out, info, P, R):
        C.memset(C.addressof(obj), 0x5A, C.sizeof(obj))
    before = [_raw(x) for x in (out, info, P, R, w)]
    hm_before = _raw(h.handle)
    try:
        HA, HM, OUT, INFO = C.byref(da.handle), C.byref(h.handle), C.byref(out), C.byref(info)
        setup = lib.spmvHipAmgSetupSmoothed
        # those of spmvHipAmgSetup
        assert setup(C.byref(gone.handle), None, None, OUT, INFO) != 0, "a freed handle"
        for dm in (rect, ell, h):
            assert setup(C.byref(dm.handle), None, None, OUT, INFO) != 0, "not square, ELL, a hierarchy"
        assert setup(HA, None, None, None, INFO) != 0 and setup(None, None, None, OUT, INFO) != 0, "NULL"
        assert setup(HA, None, None, HA, INFO) != 0, "dM == dA"
        for dm in (nodiag, twodiag):
            assert setup(C.byref(dm.handle), None, None, OUT, INFO) != 0, "STORED rule"
        assert setup(HA, C.byref(api.spmvAmgOpts(0, 0, 17, 0.0, 0, 0, 0)), None, OUT, INFO) != 0, "maxLevels"
        assert setup(HA, C.byref(api.spmvAmgOpts(0, 0, 0, -1.0, 0, 0, 0)), None, OUT, INFO) != 0, "omega"
        capfd.readouterr()
        # its own
        for bad in (-0.5, np.inf, -np.inf, np.nan):
            assert setup(HA, None, C.byref(api.spmvAmgSmoothOpts(bad)), OUT, INFO) != 0, bad
        assert capfd.readouterr().err.count("omegaP") == 4
        opts = api.spmvAmgOpts(0, 2, 0, 0.0, 0, 0, 0)
        for smooth in (None, C.byref(api.spmvAmgSmoothOpts(0.5))):
            assert setup(C.byref(overflow.handle), C.byref(opts), smooth, OUT, INFO) != 0, "a row sum that is not finite"
            assert "row 5 of level 0" in capfd.readouterr().err
        # the view
        view = lib.spmvHipAmgProlongator
        last = h.info.levels - 1
        for level in (last, last + 1, 99, 0xFFFFFFFF):
            assert view(HM, level, C.byref(P), C.byref(R), C.byref(w)) != 0, level
        assert view(HA, 0, C.byref(P), C.byref(R), C.byref(w)) != 0, "not a hierarchy"
        assert view(C.byref(gone.handle), 0, C.byref(P), C.byref(R), C.byref(w)) != 0 and view(None, 0, None, None, None) != 0
        assert view(HM, 0, None, None, None) == 0, "every output may be NULL"
        assert [_raw(x) for x in (out, info, P, R, w)] == before, "outputs untouched"
        assert _raw(h.handle) == hm_before
        # a smoothed hierarchy is no matrix, and belongs to its source
        dx, dy = api.DeviceVector(A[0]).up(b), api.DeviceVector(A[0])
        try:
            assert lib.spmvHipEnqueueAutoRows(HM, dx.ptr, dy.ptr, None) != 0
            fresh = api.spmat()
            assert lib.spmvHipCsrTranspose(HM, C.byref(fresh)) != 0 and lib.spmvHipSpGEMM(HM, HA, None, C.byref(fresh), None) != 0
            assert lib.spmvHipCsrAdd(1.0, HM, 1.0, HA, None, C.byref(fresh), None) != 0 and lib.hipSpILU0CSR(HM) != 0
            assert not fresh.dev
            assert lib.spmvHipAmgApply(HM, C.byref(other.handle), dx.ptr, dy.ptr) != 0, "not the source"
            assert lib.spmvHipAmgRefresh(HM, C.byref(other.handle)) != 0
            with pytest.raises(api.SpmvHipError):
                other.cg(b, precond=h, tol=1e-8, maxiter=5)
        finally:
            dx.free()
            dy.free()
        with pytest.raises(api.SpmvHipError):
            da.amg(omegaP=0.5)
    finally:
        for d in (other, rect, nodiag, twodiag, overflow, ell):
            d.free()


def test_a_refresh_onto_a_row_sum_that_is_not_finite_is_refused(api, capfd):
    bad = _nonfinite_row()
    good = bad[:4] + (sa.with_one_diagonal(*ar.path(12), seed=50)[4],)
    da = _up(api, good)
    h = da.amg(coarseRows=2, smoothed=True)
    try:
        da.update_values(bad[4])
        capfd.readouterr()
        with pytest.raises(api.SpmvHipError):
            h.refresh_from(da)
        assert "row 5 of level 0" in capfd.readouterr().err
        da.update_values(good[4])
        h.refresh_from(da)
        _check_levels(api, h, sa.setup_ref(good, coarseRows=2)[0], "refreshed back")
    finally:
        h.free()
        da.free()


# ------------------------------------------------------------------------------------------------ shapes, housekeeping
def test_no_rows(api):
    E = (0, 0, np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    de = _up(api, E)
    h = de.amg(smoothed=True)
    try:
        assert h.info.levels == 1 and h.info.rows[0] == 0
        assert h.apply(np.zeros(0)).size == 0
        with pytest.raises(api.SpmvHipError):
            h.prolongator(0)
    finally:
        h.free()
        de.free()


def test_one_level_is_the_plain_hierarchys_cycle(api):
    A = GRAPHS["path70"]
    r = np.random.default_rng(14).standard_normal(A[0])
    levels, o = ar.setup_ref(A, coarseRows=70)
    assert len(levels) == 1
    da = _up(api, A)
    smooth, plain = da.amg(coarseRows=70, smoothed=True), da.amg(coarseRows=70)
    try:
        assert smooth.info.levels == plain.info.levels == 1
        z = smooth.apply(r)
        _same(z, ar.cycle_ref(levels, o, r), "M <= coarseRows")
        assert_same_bits(z, plain.apply(r), "smoothed against plain")
    finally:
        smooth.free()
        plain.free()
        da.free()


def test_two_setups_are_identical(api):
    da = _up(api, ODD)
    a, b = da.amg(coarseRows=8, smoothed=True), da.amg(coarseRows=8, smoothed=True)
    try:
        assert a.info.levels == b.info.levels >= 3
        for l in range(a.info.levels):
            x, y = _level_arrays(api, a, l), _level_arrays(api, b, l)
            assert x.keys() == y.keys()
            for k in x:
                assert _blob(x[k]) == _blob(y[k]), (l, k)
        r = np.random.default_rng(15).standard_normal(ODD[0])
        assert_same_bits(a.apply(r), b.apply(r), "two setups, one cycle")
        assert (a.info.bytes, a.info.opComplexity) == (b.info.bytes, b.info.opComplexity)
    finally:
        a.free()
        b.free()
        da.free()
