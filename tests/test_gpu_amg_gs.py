"""The multicolour Gauss-Seidel smoother of the multigrid cycle on the device (spmvHipAmgSetGaussSeidel, spmvHipAmgGaussSeidel,
and such a hierarchy under spmvHipAmgApply / Refresh and as dM of the Krylov solvers) against tests/amg_gs_ref.py, bits
throughout: the cycle on plain, smoothed and strength hierarchies at both fuse thresholds, both orders, both directions, the
three level splits, four sweep triples and three small-level thresholds (special values, an odd M, misaligned vectors,
unsorted rows, rows for a wavefront, one level, no rows), every level's view, the three solvers with CG's exact count, the
launch count of a cycle, the stop, a captured replay across a refresh at the lists' addresses, switching between the three
smoothers, every refusal with the cycle and the views compared as bytes, and device memory."""
import ctypes as C
import functools

import numpy as np
import pytest

import amg_cheb_ref as cr
import amg_gs_ref as gr
import amg_ref as ar
import amg_sa_ref as sa
import colour_ref as cl
import filter_ref as fr
import spgemm_ref as sr
from amg_gpu import _same, _solve_and_compare, _up
from bits import assert_same_bits
from gmres_ref import gmres_ref
from krylov_ref import bicgstab_ref, cg_ref
from test_amg_gs_abi import COUNTS, KRYLOV_OPTS, KRYLOV_TOL, krylov_problem

pytestmark = pytest.mark.gpu

LAP = sr.laplacian7(12, 10, 8)                                  # 960 rows, three levels at coarseRows = 8
ANISO = fr.stencil7(12, 10, 8, (1.0, 0.01, 0.01))               # the strength filter drops entries of it
ODD = sa.with_one_diagonal(*(lambda a: (a[0], a[2], a[3]))(sr.laplacian7(5, 3, 3)), seed=41)       # 45 rows
GRAPHS = {name: sa.with_one_diagonal(*g, seed=n) for n, (name, g) in enumerate(ar.small_graphs().items())}
FUSED, NEVER = 64, 0
SMALL = {"never": 0, "mixed": 100, "default": gr.SMALL_ROWS}    # 100: level 0 (960) and level 1 by colour, the rest in one workgroup
HIERARCHIES = {"plain": dict(), "smoothed": dict(smoothed=True), "strength": dict(smoothed=True, theta=0.0)}
ORDERS = {gr.NATURAL: "natural", gr.HASH: "hash"}
SEED = 0x9E3779B9
LANES = (0, 1, 4, 8, 16, 32, 64)                                # lanes per row of the sweep kernels; 0: by the level's mean row, the default
# (order, seed, oneWay, levels, (nu1, nu2, nuCoarse)): every order, direction, level split and sweep triple at least twice;
# a count 0 is SPMV_AMG_NO_SWEEPS through the Python layer
CONFIGS = [(gr.NATURAL, 0, False, None, (2, 2, 8)), (gr.HASH, SEED, False, None, (3, 1, 1)), (gr.NATURAL, 0, True, None, (1, 3, 0)),
           (gr.HASH, 0, True, 1, (0, 2, 2)), (gr.NATURAL, 0, False, 1, (2, 2, 8)), (gr.NATURAL, 0, False, 2, (3, 1, 1)),
           (gr.HASH, 0, False, 2, (1, 3, 0)), (gr.NATURAL, 0, True, 2, (0, 2, 2))]


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
    api.set_variant("spmvHipAmgSetGaussSeidel", gr.SMALL_ROWS)
    api.set_variant("spmvHipAmgGaussSeidel", 0)
    api.set_variant("hipSpCGCSR", 16)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _matrix(hierarchy):
    return ANISO if hierarchy == "strength" else LAP


@functools.lru_cache(maxsize=None)
def _levels(hierarchy, depth=None):
    kw = dict(maxLevels=depth) if depth else {}
    levels, o = gr.setup_ref(_matrix(hierarchy), hierarchy, coarseRows=8, **kw)
    assert len(levels) == depth if depth else len(levels) >= 3
    return levels, o


def _special_r(M, seed=7):
    r = np.random.default_rng(seed).standard_normal(M)
    r[[3, M // 2]] = 0.0
    r[[4, M // 2 + 1]] = -0.0
    r[M // 3], r[M // 3 + 1], r[M - 2] = np.inf, -np.inf, np.nan
    return r


def _sm(o, config, **kw):
    order, seed, one_way, levels, nu = config
    return gr.smoother(o, order=order, seed=seed, oneWay=one_way, levels=levels, nu1=nu[0], nu2=nu[1], nuCoarse=nu[2], **kw)


def _set(h, config, **kw):
    order, seed, one_way, levels, nu = config
    h.set_gauss_seidel(order=ORDERS[order], seed=seed, one_way=one_way, levels=levels, nu1=nu[0], nu2=nu[1], nuCoarse=nu[2], **kw)


RS = {"random": lambda M: np.random.default_rng(8).standard_normal(M), "special": _special_r}


@functools.lru_cache(maxsize=None)
def _want(hierarchy, config, rname):
    """the reference's cycle, computed once: neither the fuse threshold nor the small-level threshold changes a bit"""
    levels, o = _levels(hierarchy)
    return gr.cycle_ref(levels, o, RS[rname](_matrix(hierarchy)[0]), _sm(o, config))


def _view_blob(h):
    """every level's two views and lists as bytes"""
    out = []
    for l in range(h.info.levels):
        v, s = h.gauss_seidel(l), h.smoother(l)
        out.append(repr([v[k] for k in ("active", "colours", "maxColourRows", "longRows", "small", "omega", "order", "seed", "oneWay", "dPerm",
                                        "dColourPtr")]).encode() +
                   (b"" if v["perm"] is None else v["perm"].tobytes() + v["colourPtr"].tobytes()) +
                   repr([s[k] for k in ("kind", "nu1", "nu2", "nuCoarse", "rho", "lambdaMax", "lambdaMin", "dCoef")]).encode() + s["coef"].tobytes())
    return b"|".join(out)


def _check_views(h, levels, sm, small_rows, what):
    """every level's view against the reference's colouring; returns the bytes the lists take"""
    cols = gr.colourings(levels, sm)
    total = 0
    for l, (lv, col) in enumerate(zip(levels, cols)):
        v, s = h.gauss_seidel(l), h.smoother(l)
        assert (s["kind"], s["nu1"], s["nu2"], s["nuCoarse"]) == (gr.GAUSS_SEIDEL, sm["nu1"], sm["nu2"], sm["nuCoarse"]), (what, l)
        assert (s["rho"], s["lambdaMax"], s["lambdaMin"], s["dCoef"], s["coef"].size) == (0.0, 0.0, 0.0, None, 0), (what, l)
        if col is None:
            assert (v["active"], v["colours"], v["maxColourRows"], v["longRows"], v["small"], v["dPerm"], v["dColourPtr"]) == (0, 0, 0, 0, 0, None, None)
            assert v["perm"] is None and v["colourPtr"] is None
            continue
        A = lv["A"]
        M, lens = A[0], np.diff(np.asarray(A[2], dtype=np.int64))
        assert v["active"] == 1 and v["colours"] == len(col["classes"]), (what, l)
        assert np.array_equal(v["perm"], col["perm"]) and np.array_equal(v["colourPtr"], col["ptr"]), (what, l)
        assert v["maxColourRows"] == (int(np.diff(col["ptr"].astype(np.int64)).max()) if M else 0), (what, l)
        assert v["longRows"] == int((lens > gr.LONG_ROW).sum()), (what, l)
        assert v["small"] == int(0 < M <= small_rows), (what, l, M)
        assert (_bits(v["omega"]), v["order"], v["seed"], v["oneWay"]) == (_bits(sm["omega"]), sm["order"], sm["seed"], int(sm["oneWay"])), (what, l)
        assert v["dPerm"] is not None and v["dColourPtr"] is not None
        total += 4 * M + 4 * (len(col["classes"]) + 1)
    return total


def test_device_memory_is_flat_across_twenty_calls(api):
    """(first in the file: no other test's handles are alive yet)  the bytes the hierarchy reports must come back exactly,
    and the free memory must not shrink by more than the allocator's granularity"""
    import torch
    da = _up(api, LAP)
    h = da.amg(coarseRows=8, smoothed=True)
    levels, o = _levels("smoothed")
    try:
        base = int(h.info.bytes)
        lists = {order: sum(4 * lv["A"][0] + 4 * (len(c["classes"]) + 1) for lv, c in zip(levels, gr.colourings(levels, gr.smoother(o, order=order))))
                 for order in ORDERS}

        def once(i):
            if i % 4 == 3:
                h.set_smoother("jacobi", nu1=1, nu2=1, nuCoarse=8)
                assert int(h.info.bytes) == base
            else:
                h.set_gauss_seidel(order=ORDERS[i % 2], nu1=1 + i % 3)
                assert int(h.info.bytes) == base + lists[i % 2]
        once(0), once(1), once(3)
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
@pytest.mark.parametrize("small", list(SMALL))
@pytest.mark.parametrize("hierarchy", list(HIERARCHIES))
def test_cycle_bits_and_views(api, hierarchy, small):
    A = _matrix(hierarchy)
    levels, o = _levels(hierarchy)
    api.set_variant("spmvHipAmgSetGaussSeidel", SMALL[small])
    for threshold in (NEVER, FUSED):
        api.set_variant("spmvHipAmgApply", threshold)
        da = _up(api, A)
        h = da.amg(coarseRows=8, **HIERARCHIES[hierarchy])
        try:
            before = int(h.info.bytes)
            never = h.gauss_seidel(0)
            assert (never["active"], never["colours"], never["dPerm"], never["dColourPtr"], never["omega"]) == (0, 0, None, None, 0.0)
            for config in CONFIGS:
                _set(h, config)
                what = f"{hierarchy}, {config}, fuse {threshold}, small {small}"
                assert int(h.info.bytes) == before + _check_views(h, levels, _sm(o, config), SMALL[small], what)
                for rname in RS:
                    _same(h.apply(RS[rname](A[0])), _want(hierarchy, config, rname), f"{rname} r, {what}")
        finally:
            h.free()
            da.free()


def test_omega_and_determinism(api):
    levels, o = _levels("smoothed")
    r = RS["random"](LAP[0])
    da = _up(api, LAP)
    h = da.amg(coarseRows=8, smoothed=True)
    try:
        for omega in (0.9, 1.3):
            h.set_gauss_seidel(omega=omega, nu1=2, nu2=2)
            z = h.apply(r)
            _same(z, gr.cycle_ref(levels, o, r, gr.smoother(o, omega=omega, nu1=2, nu2=2)), f"omega {omega}")
            for _ in range(5):
                assert_same_bits(h.apply(r), z, "repeated calls")
    finally:
        h.free()
        da.free()


def test_the_strength_hierarchy_takes_its_colours_from_a_not_f(api):
    levels, o = _levels("strength")
    sm = gr.smoother(o)
    ca, cf = gr.colourings(levels, sm), gr.colourings(levels, dict(sm, colours_from_F=True))
    assert not np.array_equal(ca[0]["perm"], cf[0]["perm"])
    da = _up(api, ANISO)
    h = da.amg(coarseRows=8, smoothed=True, theta=0.0)
    try:
        h.set_gauss_seidel()
        assert np.array_equal(h.gauss_seidel(0)["perm"], ca[0]["perm"])
    finally:
        h.free()
        da.free()


@pytest.mark.parametrize("small", ["never", "default"])
@pytest.mark.parametrize("threshold", [NEVER, FUSED])
def test_odd_rows_and_vectors_at_odd_eight_byte_offsets(api, threshold, small):
    import torch
    M = ODD[0]
    levels, o = sa.setup_ref(ODD, coarseRows=4)
    assert M % 2 == 1 and len(levels) >= 2
    sm = gr.smoother(o, nu1=3, nu2=2, nuCoarse=4)
    r = _special_r(M)
    want = gr.cycle_ref(levels, o, r, sm)
    api.set_variant("spmvHipAmgApply", threshold)
    api.set_variant("spmvHipAmgSetGaussSeidel", SMALL[small])
    da = _up(api, ODD)
    h = da.amg(coarseRows=4, smoothed=True)
    try:
        h.set_gauss_seidel(nu1=3, nu2=2, nuCoarse=4)
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


def _arrow(M=300, hubs=1, seed=3):
    """a diagonally dominant matrix whose first `hubs` rows and columns are dense (the hubs do not see each other when there
    are two: both then have the same colour and meet in one wavefront), the rest a chain"""
    rng = np.random.default_rng(seed)
    rest = np.arange(hubs, M)
    rows, cols = [np.arange(M)], [np.arange(M)]
    for hub in range(hubs):
        rows += [np.full(rest.size, hub), rest]
        cols += [rest, np.full(rest.size, hub)]
    if hubs == 1:
        rows += [rest[1:], rest[:-1]]
        cols += [rest[:-1], rest[1:]]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    p = rng.permutation(rows.size)                             # unsorted rows
    rows, cols = rows[p], cols[p]
    o = np.argsort(rows, kind="stable")
    rows, cols = rows[o], cols[o]
    vals = -(0.5 + rng.random(rows.size))
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    absum = np.bincount(rows, weights=np.abs(vals), minlength=M)
    diag = rows == cols
    vals[diag] = absum[rows[diag]] + 1.0
    return M, M, IRP, cols.astype(np.uint64), vals


@pytest.mark.parametrize("lanes", [1, 0, 4, 64])
@pytest.mark.parametrize("small", ["never", "default"])
@pytest.mark.parametrize("hubs", [1, 2])
def test_rows_for_a_wavefront(api, hubs, small, lanes):
    """300 rows, the hub rows of 300 and 299 entries: with a lane per row (lanes = 1) the wavefront-per-row path of both
    kernels, under both orders (the long row on lane 0 and elsewhere); with more lanes per row a row of many pieces"""
    A = _arrow(hubs=hubs)
    levels, o = ar.setup_ref(A, maxLevels=1)
    r = _special_r(A[0], seed=21)
    api.set_variant("spmvHipAmgSetGaussSeidel", SMALL[small])
    api.set_variant("spmvHipAmgGaussSeidel", lanes)
    da = _up(api, A)
    h = da.amg(maxLevels=1)
    try:
        for order, seed in ((gr.NATURAL, 0), (gr.HASH, 5)):
            sm = gr.smoother(o, order=order, seed=seed, omega=0.8, nuCoarse=3)
            h.set_gauss_seidel(omega=0.8, order=ORDERS[order], seed=seed, nuCoarse=3)
            v = h.gauss_seidel(0)
            assert v["longRows"] == hubs and v["small"] == int(small == "default")
            _check_views(h, levels, sm, SMALL[small], f"{hubs} hubs")
            for rr in (RS["random"](A[0]), r):
                _same(h.apply(rr), gr.cycle_ref(levels, o, rr, sm), f"{hubs} hubs, {ORDERS[order]}, small {small}")
    finally:
        h.free()
        da.free()


@pytest.mark.parametrize("lanes", LANES)
def test_every_number_of_lanes_per_row_gives_the_same_bits(api, lanes):
    """the smoothed hierarchy holds rows of 4 to 7 entries on level 0 and of 9 to 35 on level 1: under every setting a row is shorter than, as long
    as and longer than its lanes; both kernels; an odd M"""
    levels, o = _levels("smoothed")
    lens = [np.diff(lv["A"][2].astype(np.int64)) for lv in levels]
    assert min(int(x.min()) for x in lens) <= 4 and max(int(x.max()) for x in lens) > 32
    api.set_variant("spmvHipAmgGaussSeidel", lanes)
    for small in ("never", "default"):
        api.set_variant("spmvHipAmgSetGaussSeidel", SMALL[small])
        da = _up(api, LAP)
        h = da.amg(coarseRows=8, smoothed=True)
        try:
            for config in CONFIGS[:2]:
                _set(h, config)
                for rname in RS:
                    _same(h.apply(RS[rname](LAP[0])), _want("smoothed", config, rname), f"{lanes} lanes, {config}, small {small}, {rname} r")
        finally:
            h.free()
            da.free()
        olev, oo = sa.setup_ref(ODD, coarseRows=4)
        r = _special_r(ODD[0])
        da = _up(api, ODD)
        h = da.amg(coarseRows=4, smoothed=True)
        try:
            h.set_gauss_seidel(nu1=3, nu2=2, nuCoarse=4)
            _same(h.apply(r), gr.cycle_ref(olev, oo, r, gr.smoother(oo, nu1=3, nu2=2, nuCoarse=4)), f"odd M, {lanes} lanes, small {small}")
        finally:
            h.free()
            da.free()
    with pytest.raises(api.SpmvHipError):
        api.set_variant("spmvHipAmgGaussSeidel", 2)


def test_unsorted_rows_with_a_repeated_column(api):
    A = sa.with_one_diagonal(*cl.unsorted_repeats(), seed=17)
    irp, ja = A[2].astype(np.int64), A[3].astype(np.int64)
    assert any(np.unique(ja[irp[i]:irp[i + 1]]).size < irp[i + 1] - irp[i] for i in range(A[0])), "a repeated column"
    assert any(np.any(np.diff(ja[irp[i]:irp[i + 1]]) < 0) for i in range(A[0])), "an unsorted row"
    levels, o = sa.setup_ref(A, coarseRows=8)
    r = RS["random"](A[0])
    for small in ("never", "default"):
        api.set_variant("spmvHipAmgSetGaussSeidel", SMALL[small])
        da = _up(api, A)
        h = da.amg(coarseRows=8, smoothed=True)
        try:
            for config in CONFIGS[:4]:
                _set(h, config)
                _check_views(h, levels, _sm(o, config), SMALL[small], "unsorted")
                _same(h.apply(r), gr.cycle_ref(levels, o, r, _sm(o, config)), f"unsorted, {config}, small {small}")
        finally:
            h.free()
            da.free()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_small_graphs(api, name):
    """no rows, one to three rows, a path, stars, a messy pattern: unsorted rows, repeats, isolated vertices"""
    A = GRAPHS[name]
    levels, o = sa.setup_ref(A, coarseRows=8)
    r = np.random.default_rng(9).standard_normal(A[0])
    for small in ("never", "default"):
        api.set_variant("spmvHipAmgSetGaussSeidel", SMALL[small])
        da = _up(api, A)
        h = da.amg(coarseRows=8, smoothed=True)
        try:
            for config in (CONFIGS[0], CONFIGS[1], CONFIGS[3]):
                sm = _sm(o, config)
                _set(h, config)
                _check_views(h, levels, sm, SMALL[small], name)
                z = h.apply(r)
                assert z.shape == (A[0],)
                if A[0]:
                    _same(z, gr.cycle_ref(levels, o, r, sm), f"{name}, {config}, small {small}")
                else:
                    v = h.gauss_seidel(0)
                    assert (v["active"], v["colours"], v["small"]) == (1, 0, 0) and v["colourPtr"].tolist() == [0]
        finally:
            h.free()
            da.free()


@pytest.mark.parametrize("q", [1, 5])
def test_one_level(api, q):
    levels, o = _levels("plain", 1)
    r = np.random.default_rng(10).standard_normal(LAP[0])
    da = _up(api, LAP)
    h = da.amg(maxLevels=1)
    try:
        for one_way in (False, True):
            h.set_gauss_seidel(nuCoarse=q, one_way=one_way)
            assert h.info.levels == 1 and h.gauss_seidel(0)["colours"] == 2
            _same(h.apply(r), gr.cycle_ref(levels, o, r, gr.smoother(o, nuCoarse=q, oneWay=one_way)), f"one level, {q} sweeps, one-way {one_way}")
    finally:
        h.free()
        da.free()


# -------------------------------------------------------------------------------------------------------------- Krylov
NU = 2


@pytest.fixture(scope="module")
def krylov(api):
    """the Laplacian of the CPU test and its right-hand side; per hierarchy the reference with Gauss-Seidel at nu1 = nu2 = 2
    and the device hierarchy given the same smoother"""
    A, b = krylov_problem((12, 10, 8))
    da = _up(api, A)
    out = {}
    for hierarchy in ("plain", "smoothed"):
        ref = gr.GsCsr(A, hierarchy, sm=dict(nu1=NU, nu2=NU), **KRYLOV_OPTS)
        h = da.amg(**KRYLOV_OPTS, **HIERARCHIES[hierarchy])
        h.set_gauss_seidel(nu1=NU, nu2=NU)
        out[hierarchy] = (ref, h)
    yield A, b, da, out
    for _, h in out.values():
        h.free()
    da.free()


@pytest.mark.parametrize("small", ["never", "mixed", "default"])
@pytest.mark.parametrize("hierarchy", ["plain", "smoothed"])
def test_cg_takes_the_reference_count_and_a_cycle_the_launches_of_the_formula(api, krylov, hierarchy, small):
    A, b, da, hs = krylov
    ref, h = hs[hierarchy]
    want = cg_ref(ref, b, np.zeros(A[0]), KRYLOV_TOL, 200)
    assert want[2] == COUNTS[((12, 10, 8), hierarchy, NU)][1]
    api.set_variant("spmvHipAmgSetGaussSeidel", SMALL[small])
    try:
        for levels in (None, 1):
            h.set_gauss_seidel(nu1=NU, nu2=NU, levels=levels)
            sm = gr.smoother(ref.o, nu1=NU, nu2=NU, levels=levels)
            cols = gr.colourings(ref.levels, sm)
            if levels is None:
                info = _solve_and_compare(da, b, h, "cg", want, KRYLOV_TOL)
                assert info.iterations == want[2]
            else:
                x, info = da.cg(b, precond=h, tol=KRYLOV_TOL, maxiter=200)
            # CG's own kernels: 4 before the loop and 6 per enqueued iteration (whole batches of K = 16); every M^-1 (one before
            # the loop, one per iteration) adds the cycle, a dot pass and its finish
            enq = min(200, -(-info.iterations // 16) * 16)
            unfused = 1 if hierarchy == "smoothed" else 0
            cycle = gr.cycle_launches(ref.levels, sm, cols, unfused, SMALL[small])
            if small == "never" and levels is None:
                assert cycle > gr.cycle_launches(ref.levels, sm, cols, unfused, gr.SMALL_ROWS), "a launch per colour costs launches"
            assert info.launches == 4 + 6 * enq + (enq + 1) * (cycle + 2), (levels, small)
    finally:
        api.set_variant("spmvHipAmgSetGaussSeidel", gr.SMALL_ROWS)
        h.set_gauss_seidel(nu1=NU, nu2=NU)


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
        for small in ("never", "default"):
            api.set_variant("spmvHipAmgSetGaussSeidel", SMALL[small])
            h.set_gauss_seidel(nu1=NU, nu2=NU)
            xs = []
            for K in (1, 16):
                api.set_variant("hipSpCGCSR", K)
                x, info = da.cg(b, precond=h, tol=KRYLOV_TOL, maxiter=200)
                assert info.iterations == want[2]
                xs.append(x)
            assert_same_bits(xs[0], want[0], f"{hierarchy}: K = 1")
            assert_same_bits(xs[1], xs[0], f"{hierarchy}: K = 16 against K = 1")


def test_the_block_solvers_still_refuse_the_hierarchy(api, krylov, capfd):
    A, b, da, hs = krylov
    B = np.stack([b, b[::-1]], axis=1)
    capfd.readouterr()
    for method in ("cg_block", "bicgstab_block"):
        with pytest.raises(api.SpmvHipError):
            getattr(da, method)(B, precond=hs["plain"][1], tol=KRYLOV_TOL, maxiter=10)
    assert capfd.readouterr().err.count("hierarchy") >= 2


# ------------------------------------------------------------------------------------------------- capture and refresh
def _new_values():
    """other values on LAP's pattern, every one changed"""
    rng = np.random.default_rng(11)
    new = LAP[4] * (1.0 + 0.25 * rng.random(LAP[4].size))
    rows = sr.si.row_of_entry(LAP[2])
    diag = LAP[3].astype(np.int64) == rows
    new[diag] = new[diag] * (1.0 + rng.random(int(diag.sum())))
    assert np.all(new != LAP[4])
    return LAP[:4] + (new,)


@pytest.mark.parametrize("small", ["never", "default"])
@pytest.mark.parametrize("hierarchy", ["plain", "smoothed"])
def test_a_captured_cycle_replayed_after_a_refresh(api, hierarchy, small):
    import torch
    M = LAP[0]
    B = _new_values()
    kw = dict(nu1=2, nu2=3, nuCoarse=4)
    old, o = gr.setup_ref(LAP, hierarchy, coarseRows=8)
    new, _ = gr.setup_ref(B, hierarchy, coarseRows=8)
    sm = gr.smoother(o, **kw)
    r = np.random.default_rng(12).standard_normal(M)
    api.set_variant("spmvHipAmgSetGaussSeidel", SMALL[small])
    da, db = _up(api, LAP), _up(api, B)
    h = da.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    fresh = db.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    try:
        h.set_gauss_seidel(**kw)
        fresh.set_gauss_seidel(**kw)
        where = [(h.gauss_seidel(l)["dPerm"], h.gauss_seidel(l)["dColourPtr"]) for l in range(h.info.levels)]
        bytes0 = int(h.info.bytes)
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
        _same(zt.cpu().numpy(), gr.cycle_ref(old, o, r, sm), "captured replay")
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        da.update_values(B[4])
        h.refresh_from(da)
        assert [(h.gauss_seidel(l)["dPerm"], h.gauss_seidel(l)["dColourPtr"]) for l in range(h.info.levels)] == where, "the lists stay where they are"
        assert int(h.info.bytes) == bytes0 == int(fresh.info.bytes)
        _check_views(h, new, sm, SMALL[small], "refreshed")
        _check_views(fresh, new, sm, SMALL[small], "fresh")
        zt.zero_()
        g.replay()
        torch.cuda.synchronize()
        z = zt.cpu().numpy()
        _same(z, gr.cycle_ref(new, o, r, sm), "the same graph after the refresh")
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
def test_switching_between_the_three_smoothers(api, hierarchy):
    A = _matrix(hierarchy)
    r = _special_r(A[0], seed=13)
    da = _up(api, A)
    kw = dict(coarseRows=8, **HIERARCHIES[hierarchy])
    h, jac, che, gs = da.amg(**kw), da.amg(**kw), da.amg(**kw), da.amg(**kw)
    try:
        z0, bytes0, view0 = h.apply(r).tobytes(), int(h.info.bytes), _view_blob(h)
        jac.set_smoother("jacobi", nu1=2, nu2=3, nuCoarse=5)
        che.set_smoother("chebyshev", nu1=1, nu2=2, nuCoarse=3, eig_ratio=4.0)
        gs.set_gauss_seidel(order="hash", seed=4, omega=0.9, nu1=2, nu2=1, nuCoarse=3)

        def state(x):
            blob = _view_blob(x)                               # (device addresses differ between two hierarchies)
            views = [(x.gauss_seidel(l), x.smoother(l)) for l in range(x.info.levels)]
            clean = [[(k, (None if v is None else np.asarray(v).tobytes()) if k in ("perm", "colourPtr", "coef") else v)
                      for k, v in sorted({**a, **b}.items()) if k not in ("dPerm", "dColourPtr", "dCoef")] for a, b in views]
            assert blob
            return x.apply(r).tobytes(), int(x.info.bytes), repr(clean)
        h.set_gauss_seidel(order="natural", nu1=1, nu2=1)
        assert h.apply(r).tobytes() != z0 and int(h.info.bytes) > bytes0
        h.set_smoother("jacobi", nu1=1, nu2=1, nuCoarse=8)
        assert (h.apply(r).tobytes(), int(h.info.bytes), _view_blob(h)) == (z0, bytes0, view0), "back to what the setup gave"
        h.set_gauss_seidel(order="natural", nu1=4)
        h.set_smoother("jacobi", nu1=2, nu2=3, nuCoarse=5)
        assert state(h) == state(jac), "Gauss-Seidel -> Jacobi"
        h.set_smoother("chebyshev", nu1=1, nu2=2, nuCoarse=3, eig_ratio=4.0)
        assert state(h) == state(che), "-> Chebyshev"
        h.set_gauss_seidel(order="hash", seed=4, omega=0.9, nu1=2, nu2=1, nuCoarse=3)
        assert state(h) == state(gs), "-> Gauss-Seidel: the tables are gone"
        assert int(h.info.bytes) == bytes0 + sum(4 * len(v["perm"]) + 4 * len(v["colourPtr"]) for v in map(h.gauss_seidel, range(h.info.levels)))
        h.set_gauss_seidel(levels=1, nu1=2, nu2=1, nuCoarse=3)
        h.set_gauss_seidel(order="hash", seed=4, omega=0.9, nu1=2, nu2=1, nuCoarse=3)
        assert state(h) == state(gs), "two calls in a row equal the second alone"
        h.set_smoother("chebyshev", nu1=1, nu2=2, nuCoarse=3, eig_ratio=4.0)
        assert state(h) == state(che), "Gauss-Seidel -> Chebyshev"
        assert api.lib.spmvHipAmgSetGaussSeidel(C.byref(h.handle), C.byref(da.handle), None) == 0, "opts == NULL: the defaults, the current sweeps"
        gs.set_gauss_seidel(nu1=1, nu2=2, nuCoarse=3)
        api.lib.spmvHipAmgInfo(C.byref(h.handle), C.byref(h.info))
        assert state(h) == state(gs)
    finally:
        for x in (h, jac, che, gs):
            x.free()
        da.free()


# ------------------------------------------------------------------------------------------------------------ refusals
def _raw(obj):
    return bytes(C.string_at(C.addressof(obj), C.sizeof(obj)))


def test_refusals_leave_the_hierarchy_and_the_views_untouched(api, capfd):
    lib = api.lib
    r = np.random.default_rng(14).standard_normal(LAP[0])
    da, other = _up(api, LAP), _up(api, LAP)
    gone = _up(api, LAP)
    gone.free()
    info = api.spmvAmgGsInfo()
    C.memset(C.addressof(info), 0x5A, C.sizeof(info))
    hs = [da.amg(coarseRows=8, smoothed=True) for _ in range(3)]
    hs[0].set_gauss_seidel(order="hash", seed=9, omega=0.9, levels=2, nu1=2, nu2=2)
    hs[1].set_smoother("chebyshev", nu1=2, nu2=2)
    try:
        for h in hs:                                           # a Gauss-Seidel, a Chebyshev and an untouched hierarchy
            z0, view0, bytes0, info0, hm0 = h.apply(r).tobytes(), _view_blob(h), int(h.info.bytes), _raw(info), _raw(h.handle)
            HM, HA, O = C.byref(h.handle), C.byref(da.handle), api.spmvAmgGsOpts
            good = O(0, 0, 1.0, 0, 0, 3, 3, 3)
            set_ = lib.spmvHipAmgSetGaussSeidel
            capfd.readouterr()
            assert set_(None, HA, C.byref(good)) != 0 and set_(HM, None, C.byref(good)) != 0, "NULL"
            assert set_(C.byref(gone.handle), HA, C.byref(good)) != 0 and set_(HM, C.byref(gone.handle), C.byref(good)) != 0, "not live"
            assert set_(HA, HA, C.byref(good)) != 0, "dM is no hierarchy"
            assert set_(HM, C.byref(other.handle), C.byref(good)) != 0, "dA is not the source"
            assert set_(HM, HM, C.byref(good)) != 0, "dA is a hierarchy"
            capfd.readouterr()
            for order in (2, -1, 99):
                assert set_(HM, HA, C.byref(O(order, 0, 0.0, 0, 0, 0, 0, 0))) != 0, order
            assert capfd.readouterr().err.count("order") == 3
            for bad in (-1.0, -1e-300, np.inf, -np.inf, np.nan):
                assert set_(HM, HA, C.byref(O(0, 0, bad, 0, 0, 0, 0, 0))) != 0, bad
            assert capfd.readouterr().err.count("omega") == 5
            for nus in ((65, 0, 0), (0, 65, 0), (0, 0, 65), (0xFFFFFFFE, 0, 0)):
                assert set_(HM, HA, C.byref(O(0, 0, 0.0, 0, 0, *nus))) != 0, nus
            assert capfd.readouterr().err.count("sweeps") == 4
            # spmvHipAmgSetSmoother still knows two kinds
            assert lib.spmvHipAmgSetSmoother(HM, HA, C.byref(api.spmvAmgSmootherOpts(api.SPMV_AMG_SMOOTHER_GAUSS_SEIDEL, 0, 0, 0, 0.0, 0.0))) != 0
            assert "kind" in capfd.readouterr().err
            # the view
            view = lib.spmvHipAmgGaussSeidel
            for level in (h.info.levels, 99, 0xFFFFFFFF):
                assert view(HM, level, C.byref(info)) != 0, level
            assert view(HA, 0, C.byref(info)) != 0 and view(C.byref(gone.handle), 0, C.byref(info)) != 0 and view(None, 0, C.byref(info)) != 0
            assert view(HM, 0, None) != 0
            assert _raw(info) == info0 and _raw(h.handle) == hm0
            assert lib.spmvHipAmgInfo(HM, C.byref(h.info)) == 0
            assert (h.apply(r).tobytes(), _view_blob(h), int(h.info.bytes)) == (z0, view0, bytes0), "nothing moved"
        # the largest counts are taken
        h = hs[2]
        assert lib.spmvHipAmgSetGaussSeidel(C.byref(h.handle), C.byref(da.handle), C.byref(api.spmvAmgGsOpts(1, 7, 0.5, 1, 99, 64, 64, api.SPMV_AMG_NO_SWEEPS))) == 0
        v, s = h.gauss_seidel(h.info.levels - 1), h.smoother(0)
        assert (v["active"], v["omega"], v["order"], v["seed"], v["oneWay"]) == (1, 0.5, 1, 7, 1), "levels beyond the last: all"
        assert (s["kind"], s["nu1"], s["nu2"], s["nuCoarse"]) == (2, 64, 64, 0)
    finally:
        for h in hs:
            h.free()
        other.free()
        da.free()


def test_the_python_layer(api):
    da = _up(api, LAP)
    h = da.amg(coarseRows=8)
    try:
        with pytest.raises(api.SpmvHipError):
            h.set_gauss_seidel(order="red-black")
        h.set_gauss_seidel(omega=0.75, order=api.SPMV_COLOUR_HASH, seed=3, one_way=True, levels=1, nu1=3, nu2=0, nuCoarse=2)
        v = h.gauss_seidel(0)
        assert (v["active"], v["omega"], v["order"], v["seed"], v["oneWay"]) == (1, 0.75, 1, 3, 1)
        assert v["perm"].dtype == np.uint32 and sorted(v["perm"].tolist()) == list(range(LAP[0])) and v["colourPtr"][-1] == LAP[0]
        assert h.gauss_seidel(1)["active"] == 0 and h.gauss_seidel(1)["perm"] is None
        s = h.smoother(0)
        assert (s["kind"], s["nu1"], s["nu2"], s["nuCoarse"]) == (api.SPMV_AMG_SMOOTHER_GAUSS_SEIDEL, 3, 0, 2)
        with pytest.raises(api.SpmvHipError):
            h.gauss_seidel(h.info.levels)
        with pytest.raises(api.SpmvHipError):
            h.set_smoother(2)
        assert h.smoother(0)["kind"] == 2
    finally:
        h.free()
        da.free()
