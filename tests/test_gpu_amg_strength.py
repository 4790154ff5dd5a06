"""Strength-filtered smoothed aggregation on the device (spmvHipAmgSetupStrength, spmvHipAmgStrength, and such a hierarchy under
spmvHipAmgApply / Refresh and as dM of the Krylov solvers) against tests/filter_ref.py's strength_setup_ref, bits throughout:
every level's F / agg / P / R / A / dinv / w / theta, a tiny theta against the smoothed setup, the cycle, the three solvers
with CG's exact count, the refresh with the kept sets of the build, the view and the refusals, and the two older setups
untouched."""
import ctypes as C

import numpy as np
import pytest

import amg_ref as ar
import amg_sa_ref as sa
import filter_ref as fr
import spgemm_ref as sr
from amg_gpu import _bits, _blob, _down, _same, _solve_and_compare, _special_r, _up
from bits import assert_same_bits
from gmres_ref import gmres_ref
from krylov_ref import bicgstab_ref, cg_ref
from test_filter_abi import ANISO, COUNTS, KRYLOV_OPTS, KRYLOV_TOL, krylov_problem

pytestmark = pytest.mark.gpu

ANISO_A = fr.stencil7(12, 10, 8, ANISO)
SEEDS = (0, 0x9E3779B9)
GRAPHS = {name: sa.with_one_diagonal(*g, seed=n) for n, (name, g) in enumerate(ar.small_graphs().items())}
THETAS = {"default": (None, None), "explicit": (0.25, 0.7)}


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


def _raw(obj):
    return bytes(C.string_at(C.addressof(obj), C.sizeof(obj)))


def _level_arrays(api, h, l, strength=True):
    view, agg, dinv = h.level(l)
    M, NZ = int(view.M), int(view.NZ)
    out = dict(M=M, NZ=NZ, dinv=_down(api, dinv, M, np.float64), agg=None if agg is None else _down(api, agg, M, np.uint32))
    if l:
        out["A"] = (M, M, _down(api, view.IRP, M + 1, np.uint32), _down(api, view.JA, NZ, np.uint32), _down(api, view.AS, NZ, np.float64))
    if l + 1 < h.info.levels:
        out["P"], out["R"], out["w"] = h.prolongator(l)
        if strength:
            out["F"], out["theta"] = h.strength(l)
    return out


def _check_levels(api, h, levels, what, strength=True):
    assert h.info.levels == len(levels), (what, h.info.levels, len(levels))
    for l, lv in enumerate(levels):
        A = lv["A"]
        got = _level_arrays(api, h, l, strength)
        assert (got["M"], got["NZ"]) == (A[0], A[3].size) == (h.info.rows[l], h.info.nnz[l]), (what, l)
        _same(got["dinv"], lv["dinv"], f"{what}: dinv of level {l}")
        if l:
            sr.same_bits(got["A"], A, f"{what}: A of level {l}")
        if "agg" in lv:
            if strength:
                fr.same_bits(got["F"], lv["F"], f"{what}: F of level {l}", lumped=True)
                assert _bits(got["theta"]) == _bits(lv["theta"]), (what, l, got["theta"], lv["theta"])
            assert np.array_equal(got["agg"], lv["agg"]), (what, l)
            assert h.info.aggregates[l] == int(lv["agg"].max()) + 1
            sr.same_bits(got["P"], lv["P"], f"{what}: P of level {l}")
            sr.same_bits(got["R"], lv["R"], f"{what}: R of level {l}")
            assert _bits(got["w"]) == _bits(lv["w"]), (what, l, got["w"], lv["w"])
        else:
            assert got["agg"] is None and h.info.aggregates[l] == 0
    assert h.info.opComplexity == pytest.approx(sa.complexity(levels))


def _amg(da, theta, scale, **kw):
    """the strength setup: None asks for the defaults through an explicit 0.0 (either argument given selects the setup)"""
    return da.amg(smoothed=True, theta=0.0 if theta is None else theta, thetaScale=scale, **kw)


# ----------------------------------------------------------------------------------------------------------- hierarchy
@pytest.mark.parametrize("thetas", list(THETAS))
@pytest.mark.parametrize("omegaP", [None, 0.5])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["anisotropic"] + list(GRAPHS))
def test_every_level_is_the_reference(api, name, seed, omegaP, thetas):
    A = ANISO_A if name == "anisotropic" else GRAPHS[name]
    theta, scale = THETAS[thetas]
    levels, _ = fr.strength_setup_ref(A, theta, scale, omegaP or 0.0, coarseRows=8, seed=seed)
    if name == "anisotropic":
        assert len(levels) >= 3 and all(lv["F"][3].size < lv["A"][3].size for lv in levels[:2]), "the filter drops entries"
    da = _up(api, A)
    h = _amg(da, theta, scale, coarseRows=8, seed=seed, omegaP=omegaP)
    try:
        _check_levels(api, h, levels, f"{name} {thetas}")
        assert (h.info.bytes > 0) == (A[0] > 0) and h.info.ms > 0
    finally:
        h.free()
        da.free()


def test_the_filters_of_the_small_graphs_are_not_all_trivial():
    dropped = 0
    for name, A in GRAPHS.items():
        levels, _ = fr.strength_setup_ref(A, 0.25, 0.7, coarseRows=8)
        dropped += sum(lv["A"][3].size - lv["F"][3].size for lv in levels[:-1])
    assert dropped > 100


def test_a_tiny_theta_gives_the_smoothed_setup(api):
    """theta = 1e-200: theta * theta is 0.0, every nonzero entry is kept"""
    for A in (sr.laplacian7(12, 10, 8), GRAPHS["messy"], GRAPHS["path70"]):
        assert np.all(A[4] != 0.0)
        levels, _ = sa.setup_ref(A, coarseRows=8)
        da = _up(api, A)
        h, smooth = da.amg(coarseRows=8, smoothed=True, theta=1e-200), da.amg(coarseRows=8, smoothed=True)
        try:
            _check_levels(api, h, levels, "tiny theta", strength=False)
            for l in range(h.info.levels):
                x, y = _level_arrays(api, h, l, False), _level_arrays(api, smooth, l, False)
                assert x.keys() == y.keys()
                for k in x:
                    assert _blob(x[k]) == _blob(y[k]), (l, k)
            for l in range(h.info.levels - 1):
                F, theta = h.strength(l)
                sr.same_bits(F, levels[l]["A"], f"F of level {l} is A")
                assert theta == 1e-200 * 0.5 ** l
        finally:
            smooth.free()
            h.free()
            da.free()


# --------------------------------------------------------------------------------------------------------------- cycle
@pytest.mark.parametrize("nu", [(0, 0, 1), (1, 1, 8), (2, 1, 3)])
def test_cycle_bits(api, nu):
    kw = dict(coarseRows=8, nu1=nu[0], nu2=nu[1], nuCoarse=nu[2])
    levels, o = fr.strength_setup_ref(ANISO_A, **kw)
    da = _up(api, ANISO_A)
    h = _amg(da, None, None, **kw)
    try:
        for what, r in (("random", np.random.default_rng(8).standard_normal(ANISO_A[0])), ("special", _special_r(ANISO_A[0]))):
            _same(h.apply(r), sa.cycle_ref(levels, o, r), f"{what} r, sweeps {nu}")
    finally:
        h.free()
        da.free()


# -------------------------------------------------------------------------------------------------------------- Krylov
@pytest.fixture(scope="module")
def krylov(api):
    A, b = krylov_problem(ANISO)
    ref = fr.StrengthCsr(A, **KRYLOV_OPTS)
    da = _up(api, A)
    h = _amg(da, None, None, **KRYLOV_OPTS)
    yield A, b, ref, da, h
    h.free()
    da.free()


def test_cg_takes_exactly_the_reference_count(api, krylov):
    A, b, ref, da, h = krylov
    want = cg_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200)
    assert want[2] == COUNTS[ANISO][2] < COUNTS[ANISO][1]
    assert h.info.levels == len(ref.levels) == 5
    assert _solve_and_compare(da, b, h, "cg", want, KRYLOV_TOL).iterations == COUNTS[ANISO][2]
    smooth = da.amg(smoothed=True, **KRYLOV_OPTS)
    try:
        x, info = da.cg(b, precond=smooth, tol=KRYLOV_TOL, maxiter=200)
        assert info.iterations == COUNTS[ANISO][1], "the smoothed hierarchy without the filter, on the same handle"
    finally:
        smooth.free()


def test_bicgstab_and_gmres(api, krylov):
    A, b, ref, da, h = krylov
    _solve_and_compare(da, b, h, "bicgstab", bicgstab_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200), KRYLOV_TOL)
    _solve_and_compare(da, b, h, "gmres", gmres_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200, 5), KRYLOV_TOL, restart=5)


def test_the_block_solvers_refuse_it(api, krylov, capfd):
    A, b, ref, da, h = krylov
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
            P, R, F = api.spmat(), api.spmat(), api.spmat()
            assert api.lib.spmvHipAmgProlongator(C.byref(h.handle), l, C.byref(P), C.byref(R), None) == 0
            assert api.lib.spmvHipAmgStrength(C.byref(h.handle), l, C.byref(F), None) == 0
            out += [C.cast(p, C.c_void_p).value for v in (P, R, F) for p in (v.IRP, v.JA, v.AS)]
    return out


def test_refresh_with_every_value_doubled_equals_a_fresh_setup_at_the_same_addresses(api):
    """every comparison of the filter scales by exactly 4, so a fresh setup keeps the same entries"""
    A = GRAPHS["laplacian12x10x8"]
    B = A[:4] + (A[4] * 2.0,)
    old, _ = fr.strength_setup_ref(A, 0.14, 0.5, coarseRows=8)
    levels, o = fr.strength_setup_ref(B, 0.14, 0.5, coarseRows=8)
    assert len(levels) == len(old) >= 3 and all(np.array_equal(a["kept"], b["kept"]) for a, b in zip(old[:-1], levels[:-1]))
    assert 0 < old[0]["F"][3].size - A[0] < A[3].size - A[0], "level 0 drops some entries and keeps some"
    da, db = _up(api, A), _up(api, B)
    h, fresh = _amg(da, 0.14, 0.5, coarseRows=8), _amg(db, 0.14, 0.5, coarseRows=8)
    try:
        _check_levels(api, h, old, "before")
        where = _addresses(api, h)
        da.update_values(B[4])
        h.refresh_from(da)
        assert _addresses(api, h) == where
        _check_levels(api, h, levels, "refreshed")
        _check_levels(api, fresh, levels, "fresh")
        r = np.random.default_rng(12).standard_normal(A[0])
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


def test_refresh_after_a_perturbation_keeps_the_kept_sets_of_the_build(api):
    A = GRAPHS["laplacian12x10x8"]
    rng = np.random.default_rng(2930)
    B = A[:4] + (A[4] * (1.0 + 0.3 * rng.random(A[4].size)),)
    old, o = fr.strength_setup_ref(A, 0.14, 0.5, coarseRows=8)
    fresh, _ = fr.strength_setup_ref(B, 0.14, 0.5, coarseRows=8)
    assert not np.array_equal(old[0]["kept"], fresh[0]["kept"]), "a fresh setup would keep other entries"
    want = fr.strength_refresh_ref(old, o, B)
    da = _up(api, A)
    h = _amg(da, 0.14, 0.5, coarseRows=8)
    try:
        where = _addresses(api, h)
        da.update_values(B[4])
        h.refresh_from(da)
        assert _addresses(api, h) == where
        _check_levels(api, h, want, "refreshed onto perturbed values")
        assert np.array_equal(want[0]["F"][3], old[0]["F"][3]) and np.array_equal(want[0]["agg"], old[0]["agg"])
        r = np.random.default_rng(13).standard_normal(A[0])
        _same(h.apply(r), sa.cycle_ref(want, o, r), "cycle after the refresh")
    finally:
        h.free()
        da.free()


# ------------------------------------------------------------------------------------------------- view and refusals
def test_the_view_and_the_refusals(api, krylov, capfd):
    A, b, ref, da, h = krylov
    lib = api.lib
    smooth, plain = da.amg(smoothed=True, **KRYLOV_OPTS), da.amg(**KRYLOV_OPTS)
    gone = _up(api, A)
    gone.free()
    out, info, F, theta = api.spmat(), api.spmvAmgInfo(), api.spmat(), C.c_double(123.0)
    for obj in (out, info, F):
        C.memset(C.addressof(obj), 0x5A, C.sizeof(obj))
    before = [_raw(x) for x in (out, info, F, theta)]
    hm_before = _raw(h.handle)
    try:
        HA, HM, OUT, INFO = C.byref(da.handle), C.byref(h.handle), C.byref(out), C.byref(info)
        setup = lib.spmvHipAmgSetupStrength
        capfd.readouterr()
        for t, s in ((-0.5, 0.5), (np.inf, 0.5), (np.nan, 0.5), (0.1, -0.5), (0.1, np.inf), (0.1, np.nan), (0.1, 1.5)):
            assert setup(HA, None, None, C.byref(api.spmvAmgStrengthOpts(t, s)), OUT, INFO) != 0, (t, s)
        err = capfd.readouterr().err
        assert err.count("spmvHipAmgSetupStrength") == 7 and err.count("thetaScale") == 4
        assert setup(HA, None, C.byref(api.spmvAmgSmoothOpts(-1.0)), None, OUT, INFO) != 0, "omegaP, as the smoothed setup"
        assert setup(HA, None, None, None, HA, INFO) != 0 and setup(None, None, None, None, OUT, INFO) != 0
        assert setup(C.byref(gone.handle), None, None, None, OUT, INFO) != 0 and setup(HM, None, None, None, OUT, INFO) != 0
        view = lib.spmvHipAmgStrength
        last = h.info.levels - 1
        for level in (last, last + 1, 99, 0xFFFFFFFF):
            assert view(HM, level, C.byref(F), C.byref(theta)) != 0, level
        for other in (smooth, plain, da):
            assert view(C.byref(other.handle), 0, C.byref(F), C.byref(theta)) != 0, "not a strength hierarchy"
        assert view(C.byref(gone.handle), 0, C.byref(F), C.byref(theta)) != 0 and view(None, 0, None, None) != 0
        assert view(HM, 0, None, None) == 0, "every output may be NULL"
        assert [_raw(x) for x in (out, info, F, theta)] == before, "outputs untouched"
        assert _raw(h.handle) == hm_before
        assert view(HM, 0, C.byref(F), C.byref(theta)) == 0 and not F.dev and theta.value == 0.08
        assert (int(F.M), int(F.N), int(F.NZ)) == (A[0], A[0], ref.levels[0]["F"][3].size)
        with pytest.raises(api.SpmvHipError):
            da.amg(theta=0.1)
        with pytest.raises(api.SpmvHipError):
            da.amg(thetaScale=0.5)
        with pytest.raises(api.SpmvHipError):
            smooth.strength(0)
    finally:
        smooth.free()
        plain.free()


def test_the_two_older_setups_give_the_bytes_they_gave(api):
    """before and after a strength setup on the same handle: their levels, their cycle, their views"""
    A = ANISO_A
    r = np.random.default_rng(14).standard_normal(A[0])
    da = _up(api, A)

    def snapshot(**kw):
        h = da.amg(coarseRows=8, **kw)
        try:
            parts = [h.apply(r).tobytes(), bytes([h.info.levels])]
            for l in range(h.info.levels):
                x = _level_arrays(api, h, l, False)
                parts += [_blob(x[k]) for k in sorted(x)]
            return b"|".join(parts)
        finally:
            h.free()
    try:
        before = [snapshot(), snapshot(smoothed=True), snapshot(smoothed=True, omegaP=0.5)]
        s = _amg(da, None, None, coarseRows=8)
        s.refresh_from(da)
        s.free()
        assert [snapshot(), snapshot(smoothed=True), snapshot(smoothed=True, omegaP=0.5)] == before
        lp, op = ar.setup_ref(A, coarseRows=8)
        ls, os_ = sa.setup_ref(A, coarseRows=8)
        plain, smooth = da.amg(coarseRows=8), da.amg(coarseRows=8, smoothed=True)
        try:
            _same(plain.apply(r), ar.cycle_ref(lp, op, r), "the plain hierarchy")
            _same(smooth.apply(r), sa.cycle_ref(ls, os_, r), "the smoothed hierarchy")
        finally:
            plain.free()
            smooth.free()
    finally:
        da.free()


def test_device_memory_comes_back(api):
    import torch
    A = sa.with_one_diagonal(*(lambda a: (a[0], a[2], a[3]))(fr.stencil7(40, 40, 20, ANISO)), seed=1)
    da = _up(api, A)
    try:
        def once(use=False):
            h = _amg(da, 0.1, None, coarseRows=64)
            kept = int(h.info.bytes)
            if use:
                h.refresh_from(da)
                h.apply(np.ones(A[0]))
            h.free()
            return kept
        once(True), once(True)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        kept = [once() for _ in range(10)]
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        slack = 8 << 20
        assert sum(kept) > 2 * slack, "ten leaked hierarchies would show"
        assert after >= before - slack, (before, after)
    finally:
        da.free()
