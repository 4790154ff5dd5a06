"""The approximate-inverse factor applied from single-precision storage (spmvHipFsaiSetStorage): the apply
and every solver that takes the factor as its preconditioner have the bits of the reference loops (tests/krylov_ref.py,
tests/gmres_ref.py) with M^-1 v = G~^T (G~ v), G~ the factor rounded through float32 -- x, history and iteration count --, a
refresh keeps the setting, and the way back to double storage gives the double bits again.  tests/test_values_f32_abi.py shows
on the host that the two storages give other bits of x on these inputs."""
import functools

import numpy as np
import pytest

import fsai_ref as fr
import values_f32_ref as vr
from bits import assert_same_bits
from gmres_ref import gmres_ref
from krylov_ref import bicgstab_ref, cg_ref
from spgemm_ref import laplacian7
from test_fsai_abi import random_spd, stencil

pytestmark = pytest.mark.gpu

TOL = 1e-10
SOLVERS = {"cg": (cg_ref, {}, ()), "bicgstab": (bicgstab_ref, {}, ()), "gmres": (gmres_ref, dict(restart=5), (5,))}
CASES = {
    "laplacian-10x9x8": lambda: tuple(laplacian7(10, 9, 8)[:5]),
    "stencil-9x8x7": lambda: stencil(np.random.default_rng(3820), 9, 8, 7),
    "random-spd-300": lambda: random_spd(np.random.default_rng(3803), 300, 4),
}


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(A, G, G~, b): computed once and shared"""
    A = CASES[name]()
    G = fr.fsai_vec(A)[0]
    return A, G, vr.rounded(G), np.random.default_rng(3821).standard_normal(A[0])


@pytest.fixture(params=list(CASES))
def factor(api, request):
    A, G, Gt, b = _case(request.param)
    da = api.spMatCpyCSR(api.HostCSR(*A))
    g = da.fsai(storage="f32")
    yield request.param, A, G, Gt, b, da, g
    g.free()
    da.free()


def test_apply_is_two_f32_products(api, factor):
    name, A, G, Gt, b, da, g = factor
    assert g.storage == "f32" and g.values_f32_info().built == 1
    assert_same_bits(g.apply(b), fr.Applied(Gt)(b), f"{name}: G~^T (G~ r)")
    g.set_storage("f32")                                                 # idempotent
    assert_same_bits(g.apply(b), fr.Applied(Gt)(b), f"{name}: set again")


@pytest.mark.parametrize("method", list(SOLVERS))
def test_the_solvers_apply_the_rounded_factor(api, factor, method):
    name, A, G, Gt, b, da, g = factor
    loop, kw, tail = SOLVERS[method]
    want = loop(fr.PrecondCsr(A, Gt), b, np.zeros(A[0]), TOL, 300, *tail)
    x, info = getattr(da, method)(b, precond=g, tol=TOL, maxiter=300, history=True, **kw)
    assert (info.status, info.iterations) == (want[1], want[2]), f"{name}, {method}"
    assert_same_bits(x, want[0], f"{name}, {method}: x")
    assert_same_bits(info.history, want[3], f"{name}, {method}: history")


def test_block_cg_applies_the_rounded_factor(api, factor):
    name, A, G, Gt, b, da, g = factor
    M = A[0]
    rng = np.random.default_rng(4300)
    B = np.ascontiguousarray(np.stack([b, rng.standard_normal(M), rng.standard_normal(M)], axis=1))
    X, info = da.cg_block(B, precond=g, tol=TOL, maxiter=300, history=True)
    ref = fr.PrecondCsr(A, Gt)
    for c in range(3):
        want = cg_ref(ref, np.ascontiguousarray(B[:, c]), np.zeros(M), TOL, 300)
        col = info.columns[c]
        assert (col.status, col.iterations) == (want[1], want[2]), f"{name}, column {c}"
        assert_same_bits(X[:, c], want[0], f"{name}, column {c}: x")
        assert_same_bits(info.history[c], want[3], f"{name}, column {c}: history")


def test_back_to_f64_gives_the_f64_bits(api, factor):
    name, A, G, Gt, b, da, g = factor
    live = api.alloc_stats().live
    g.set_storage("f64")
    assert g.storage == "f64" and g.values_f32_info().built == 0
    assert api.alloc_stats().live == live - (2 if G[4].size else 0), "both forms are released"
    assert_same_bits(g.apply(b), fr.Applied(G)(b), f"{name}: the apply")
    want = cg_ref(fr.PrecondCsr(A, G), b, np.zeros(A[0]), TOL, 300)
    x, info = da.cg(b, precond=g, tol=TOL, maxiter=300)
    assert info.iterations == want[2]
    assert_same_bits(x, want[0], f"{name}: CG")
    g.set_storage("f32")
    assert_same_bits(g.apply(b), fr.Applied(Gt)(b), f"{name}: and F32 again")


def test_a_refresh_keeps_the_storage(api):
    A, G, Gt, b = _case("random-spd-300")
    B = random_spd(np.random.default_rng(3803), 300, 4, e=1)             # the pattern of A, other values
    assert np.array_equal(B[3], A[3]) and not np.array_equal(B[4], A[4])
    da = api.spMatCpyCSR(api.HostCSR(*A))
    g = da.fsai(storage="f32")
    try:
        da.update_values(B[4])
        g.refresh_from(da)
        assert g.storage == "f32" and g.values_f32_info().refreshes == 1
        Ht = vr.rounded(fr.fsai_vec(B)[0])
        assert_same_bits(g.apply(b), fr.Applied(Ht)(b), "the apply after the refresh")
        want = cg_ref(fr.PrecondCsr(B, Ht), b, np.zeros(B[0]), TOL, 300)
        x, info = da.cg(b, precond=g, tol=TOL, maxiter=300, history=True)
        assert (info.status, info.iterations) == (want[1], want[2])
        assert_same_bits(x, want[0], "CG after the refresh")
        assert_same_bits(info.history, want[3], "its history")
    finally:
        g.free()
        da.free()


# ------------------------------------------------------------------------------------------------------- the hierarchy
# spmvHipAmgSetStorage: the cycle on levels whose A_l, R_l and P_l are rounded through float32 and whose dinv, rho_l and
# Chebyshev tables are the doubles' (values_f32_ref.rounded_levels) -- tests/test_values_f32_abi.py shows on the host that this
# gives other bits than the f64 cycle on these inputs.
import amg_block_ref as br  # noqa: E402
import amg_cheb_ref as cr  # noqa: E402

KINDS = {cr.JACOBI: "jacobi", cr.CHEBYSHEV: "chebyshev"}


def _hierarchy(api, config, da, storage="f32"):
    hierarchy, smoother, fuse = vr.AMG_CONFIGS[config]
    kind, nu1, nu2, nuCoarse = br.SMOOTHERS[smoother]
    api.set_variant("spmvHipAmgApply", fuse)                             # the longest row of P that the fused correction takes
    try:
        kw = dict(smoothed=True) if hierarchy != "plain" else {}
        if hierarchy == "strength":
            kw["theta"] = 0.0
        h = da.amg(coarseRows=8, **kw)
    finally:
        api.set_variant("spmvHipAmgApply", 0)
    h.set_smoother(KINDS[kind], nu1=nu1, nu2=nu2, nuCoarse=nuCoarse)
    if storage != "f64":
        h.set_storage(storage)
    return h


@pytest.fixture(params=list(vr.AMG_CONFIGS))
def hierarchy(api, request):
    levels, rounded, o, sm = vr.amg_reference(request.param)
    da = api.spMatCpyCSR(api.HostCSR(*vr.amg_matrix()))
    h = _hierarchy(api, request.param, da)
    yield request.param, levels, rounded, o, sm, da, h
    h.free()
    da.free()


def test_the_cycle_applies_the_rounded_levels(api, hierarchy):
    config, levels, rounded, o, sm, da, h = hierarchy
    M = levels[0]["A"][0]
    info = h.storage_info()
    assert info["storage"] == "f32" and info["levels"] == len(levels) == h.info.levels
    nnz = sum(lv["csr"].AS.size + (lv["Rcsr"].AS.size + (lv["Pcsr"].AS.size if "Pcsr" in lv else 0) if "Rcsr" in lv else 0) for lv in levels)
    nnzA = sum(lv["csr"].AS.size for lv in levels)                       # (a plain hierarchy's R_l and P_l are unit handles: no array)
    assert 4 * nnzA <= info["f32_bytes"] <= 4 * nnz + 48 * 3 * len(levels), "4 B per streamed entry, rounded up to 16, and the counters"
    r = si_values(M, 4520)
    want = cr.cycle_ref(rounded, o, r, sm)
    assert_same_bits(h.apply(r), want, f"{config}: spmvHipAmgApply")
    R = np.ascontiguousarray(np.stack([r, si_values(M, 4521), si_values(M, 4522)], axis=1))
    h.set_block_width(3)
    Z = h.apply_block(R)
    assert_same_bits(Z, br.block_cycle_ref(rounded, o, R, sm), f"{config}: the 3-column block cycle")
    assert_same_bits(Z[:, 0], want, f"{config}: column 0 is the single cycle")
    # and back: the f64 cycle's bits, the forms released
    h.set_storage("f64")
    assert h.storage_info() == {"storage": "f64", "levels": len(levels), "f32_bytes": 0} and da.values_f32_info().built == 0
    assert_same_bits(h.apply(r), cr.cycle_ref(levels, o, r, sm), f"{config}: back in F64")


def si_values(n, seed):
    import serial_order_inputs as si
    return si.order_values(np.random.default_rng(seed), n, 1)


def _kw(sm):
    return dict(kind=sm["kind"], nu1=sm["nu1"], nu2=sm["nu2"], nuCoarse=sm["nuCoarse"])


def test_cg_takes_the_f32_hierarchy(api, hierarchy):
    config, levels, rounded, o, sm, da, h = hierarchy
    A = vr.amg_matrix()
    b = np.random.default_rng(4530).standard_normal(A[0])
    want = cg_ref(cr.ChebCsr(A, levels=rounded, o=o, sm=_kw(sm)), b, np.zeros(A[0]), TOL, 300)
    x, info = da.cg(b, precond=h, tol=TOL, maxiter=300, history=True)
    assert (info.status, info.iterations) == (want[1], want[2]) and want[1] == 0, config
    assert_same_bits(x, want[0], f"{config}: x")
    assert_same_bits(info.history, want[3], f"{config}: history")


@pytest.mark.parametrize("config", ["plain-jacobi", "smoothed-chebyshev", "smoothed-chebyshev-fused"])
def test_a_hierarchy_refresh_keeps_the_storage(api, config):
    A, B = vr.amg_matrix(), vr.amg_matrix(1)
    assert np.array_equal(B[3], A[3]) and not np.array_equal(B[4], A[4])
    levels, rounded, o, sm = vr.amg_reference(config, 1)
    da = api.spMatCpyCSR(api.HostCSR(*A))
    h = _hierarchy(api, config, da)
    try:
        before = h.storage_info()
        da.update_values(B[4])
        h.refresh_from(da)
        assert h.storage_info() == before
        r = si_values(A[0], 4540)
        assert_same_bits(h.apply(r), cr.cycle_ref(rounded, o, r, sm), f"{config}: the cycle after the refresh")
    finally:
        h.free()
        da.free()
