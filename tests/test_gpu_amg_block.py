"""The multigrid cycle for a block of vectors on the device (spmvHipAmgSetBlockWidth, spmvHipAmgBlock, spmvHipAmgApplyBlock)
and a hierarchy as dM of the block solvers, against tests/amg_block_ref.py and, device to device, against the single cycle
and the single solves, bits throughout: plain, smoothed and strength hierarchies with Jacobi and Chebyshev at two degree
triples each, on 960 and 7 680 rows (two 4 096-row blocks), k = 1, 2, 3, 16, 17, 33, both layouts with padded leading
dimensions and misaligned blocks between sentinels; special-value columns; the small graphs and one level; the workspace's
width and bytes; a captured cycle across a refresh; the smoother switched before and after the width; the Gauss-Seidel
refusal; the block solves with columns that stop at different iterations, their launch count, every refusal, device memory."""
import ctypes as C
import functools

import numpy as np
import pytest

import amg_block_ref as br
import amg_cheb_ref as cr
import amg_ref as ar
import amg_sa_ref as sa
import filter_ref as fr
import spgemm_ref as sr
from amg_gpu import _same, _up, cycle_launches
from bits import assert_same_bits
from test_amg_cheb_abi import KRYLOV_TOL, krylov_problem

pytestmark = pytest.mark.gpu

SHAPES = {"960": (12, 10, 8), "7680": (24, 20, 16)}
HIERARCHIES = {"plain": dict(), "smoothed": dict(smoothed=True), "strength": dict(smoothed=True, theta=0.0)}
KINDS = {cr.JACOBI: "jacobi", cr.CHEBYSHEV: "chebyshev"}
WIDTHS = (1, 2, 3, 16, 17, 33)
# (layout, columns or rows beyond the block in the leading dimension, offset of the block in 8-byte elements)
LAYOUTS = (("row", 0, 0), ("row", 3, 1), ("col", 0, 1), ("col", 1, 0))
SENTINEL = -7.25e77
GRAPHS = {name: sa.with_one_diagonal(*g, seed=n) for n, (name, g) in enumerate(ar.small_graphs().items())}


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
    for name in ("hipSpCGBlockCSR", "hipSpBiCGStabBlockCSR", "hipSpCGCSR", "hipSpBiCGStabCSR"):
        api.set_variant(name, 16)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _matrix(hierarchy, shape):
    return fr.stencil7(*shape, (1.0, 0.01, 0.01)) if hierarchy == "strength" else sr.laplacian7(*shape)


@functools.lru_cache(maxsize=None)
def _levels(hierarchy, size):
    levels, o = cr.setup_ref(_matrix(hierarchy, SHAPES[size]), hierarchy, coarseRows=8)
    assert len(levels) >= 3
    return levels, o


@functools.lru_cache(maxsize=None)
def _reference(hierarchy, size, smoother):
    """(R, Z) for the 33 columns of the cycle tests, computed once"""
    levels, o = _levels(hierarchy, size)
    R = br.ordinary_block(levels[0]["A"][0], max(WIDTHS))
    return R, br.block_cycle_ref(levels, o, R, br.smoother_of(o, smoother))


def _set_smoother(h, name):
    kind, nu1, nu2, nuCoarse = br.SMOOTHERS[name]
    h.set_smoother(KINDS[kind], nu1=nu1, nu2=nu2, nuCoarse=nuCoarse)


def _block(M, k, layout, extra, offset, fill=None):
    """(buffer, view): an (M, k) view in `layout` inside a buffer of sentinels"""
    import torch
    rows, cols = (M, k + extra) if layout == "row" else (k, M + extra)
    buf = torch.full((rows * cols + offset + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    full = buf[offset:offset + rows * cols].view(rows, cols)
    view = full[:, :k] if layout == "row" else full[:, :M].t()
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill)).cuda())
    return buf, view


def _sentinels_survive(buf, view, what):
    got = view.cpu().numpy().copy()
    view.fill_(SENTINEL)
    assert bool((buf == SENTINEL).all()), f"{what}: an element outside the block was written"
    return got


def _state(h):
    """what must not move: the bytes, the block workspace, every level's view and table addresses"""
    out = [int(h.info.bytes), repr(h.block_info())]
    for l in range(h.info.levels):
        view, agg, dinv = h.level(l)
        out.append((C.string_at(C.addressof(view), C.sizeof(view)), agg, dinv, h.smoother(l)["dCoef"]))
    return out


def _addresses(h):
    return [h.level(l)[1:] for l in range(h.info.levels)]


def _expected_bytes(h, width):
    kp = width + (width & 1)
    rows = [int(h.info.rows[l]) for l in range(h.info.levels)]
    return 8 * kp * (2 * rows[0] + 4 * sum(rows[1:]))


def _launches(h, hierarchy, smoother):
    _, nu1, nu2, nuCoarse = br.SMOOTHERS[smoother]
    return cycle_launches(nu1, nu2, nuCoarse, h.info.levels, h.info.levels - 1 if hierarchy != "plain" else 0)


def test_device_memory_is_flat_across_twenty_cycles_and_solves(api):
    """(first in the file: no other test's handles are alive yet)"""
    import torch
    A, b = krylov_problem(SHAPES["960"])
    da = _up(api, A)
    h = da.amg(coarseRows=8, smoothed=True)
    try:
        h.set_block_width(4)
        R = torch.from_numpy(br.ordinary_block(A[0], 4)).cuda()
        Z = torch.empty_like(R)
        B = torch.from_numpy(np.stack([b, 2.0 * b, 0.5 * b], axis=1)).cuda()

        def once():
            h.apply_block(R, out=Z)
            da.cg_block(B, precond=h, tol=KRYLOV_TOL, maxiter=50)
        once()
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        for _ in range(20):
            once()
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        assert after >= before - (8 << 20), (before, after)
    finally:
        h.free()
        da.free()


# --------------------------------------------------------------------------------------------------------------- cycle
@pytest.mark.parametrize("size", list(SHAPES))
@pytest.mark.parametrize("smoother", list(br.SMOOTHERS))
@pytest.mark.parametrize("hierarchy", list(HIERARCHIES))
def test_cycle_bits_for_every_width_and_layout(api, hierarchy, smoother, size):
    import torch
    A = _matrix(hierarchy, SHAPES[size])
    M = A[0]
    R, want = _reference(hierarchy, size, smoother)
    da = _up(api, A)
    h = da.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    try:
        _set_smoother(h, smoother)
        # the single cycle of every column, device to device, before the hierarchy has a width
        Rt = torch.from_numpy(R).cuda()
        single = torch.stack([h.apply(Rt[:, c].contiguous()) for c in range(R.shape[1])], dim=1).cpu().numpy()
        assert_same_bits(single, want, "the single cycles against the reference")
        h.set_block_width(max(WIDTHS))
        for n, k in enumerate(WIDTHS):
            for j, (layout, extra, offset) in enumerate(LAYOUTS):
                zl = LAYOUTS[(j + 1 + n) % len(LAYOUTS)]             # Z in another layout than R
                what = f"k = {k}, R {layout, extra, offset}, Z {zl}"
                rbuf, rv = _block(M, k, layout, extra, offset, fill=R[:, :k])
                zbuf, zv = _block(M, k, *zl)
                before = rbuf.clone()
                out = h.apply_block(rv, out=zv)
                assert out is zv
                assert torch.equal(rbuf.view(torch.int64), before.view(torch.int64)), f"{what}: R is only read"
                got = _sentinels_survive(zbuf, zv, what)
                assert_same_bits(got, single[:, :k], f"{what}: against the single cycle per column")
                assert_same_bits(got, want[:, :k], f"{what}: against the reference")
    finally:
        h.free()
        da.free()


@pytest.mark.parametrize("smoother", ["jacobi223", "cheb314"])
@pytest.mark.parametrize("hierarchy", list(HIERARCHIES))
def test_special_value_columns_stay_in_their_columns(api, hierarchy, smoother):
    A = _matrix(hierarchy, SHAPES["960"])
    levels, o = _levels(hierarchy, "960")
    sm = br.smoother_of(o, smoother)
    R = br.special_block(A[0])
    T = br.tamed(R)
    da = _up(api, A)
    h = da.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    try:
        _set_smoother(h, smoother)
        h.set_block_width(8)
        Z, ZT = h.apply_block(R), h.apply_block(T)
        want = br.block_cycle_ref(levels, o, R, sm)
        for c in range(8):
            _same(Z[:, c], want[:, c], f"column {c}")
            _same(Z[:, c], h.apply(np.ascontiguousarray(R[:, c])), f"column {c} against the single cycle")
            if c not in br.SPECIAL:
                assert_same_bits(Z[:, c], ZT[:, c], f"column {c}: the bits of a block without the special columns")
        assert np.isnan(Z[:, 4]).any() and not np.isfinite(Z[:, 6]).all()
        # seven columns: the odd last pair holds the padding column, which never reaches a real one
        Z7 = h.apply_block(np.ascontiguousarray(R[:, :7]))
        for c in range(7):
            _same(Z7[:, c], want[:, c], f"k = 7, column {c}")
    finally:
        h.free()
        da.free()


def test_the_gather_keeps_minus_zero_on_the_negated_laplacian(api):
    """the input of the planted fault of test_amg_block_abi.py: a column of zeros on a plain hierarchy whose dinv is negative"""
    LAP = sr.laplacian7(12, 10, 8)
    A = LAP[:4] + (-LAP[4],)
    levels, o = ar.setup_ref(A, coarseRows=8)
    R = br.ordinary_block(A[0], 3)
    R[:, 1] = 0.0
    da = _up(api, A)
    h = da.amg(coarseRows=8)
    try:
        h.set_block_width(3)
        Z = h.apply_block(R)
        want = br.block_cycle_ref(levels, o, R, cr.smoother(o, kind=cr.JACOBI))
        assert np.signbit(want[:, 1]).all() and not want[:, 1].any()
        assert_same_bits(Z, want, "z = z + e[agg]")
    finally:
        h.free()
        da.free()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_small_graphs(api, name):
    A = GRAPHS[name]
    levels, o = sa.setup_ref(A, coarseRows=8)
    sm = cr.smoother(o, nu1=2, nu2=2, nuCoarse=3)
    da = _up(api, A)
    h = da.amg(coarseRows=8, smoothed=True)
    try:
        h.set_smoother(nu1=2, nu2=2, nuCoarse=3)
        h.set_block_width(5)
        assert h.block_info() == dict(width=5, bytes=_expected_bytes(h, 5))
        R = br.ordinary_block(A[0], 5)
        Z = h.apply_block(R)
        assert Z.shape == (A[0], 5)
        if A[0]:
            assert_same_bits(Z, br.block_cycle_ref(levels, o, R, sm), name)
    finally:
        h.free()
        da.free()


@pytest.mark.parametrize("smoother", ["jacobi118", "cheb314"])
def test_one_level(api, smoother):
    A = sr.laplacian7(12, 10, 8)
    levels, o = cr.setup_ref(A, "plain", coarseRows=8, maxLevels=1)
    da = _up(api, A)
    h = da.amg(coarseRows=8, maxLevels=1)
    try:
        _set_smoother(h, smoother)
        h.set_block_width(3)
        assert h.info.levels == 1 and h.block_info()["bytes"] == 8 * 4 * 2 * A[0]
        R = br.ordinary_block(A[0], 3)
        assert_same_bits(h.apply_block(R), br.block_cycle_ref(levels, o, R, br.smoother_of(o, smoother)), "one level")
    finally:
        h.free()
        da.free()


# ------------------------------------------------------------------------------------------------------- the workspace
def test_width_bytes_and_the_single_cycle_untouched(api):
    A, b = krylov_problem(SHAPES["960"])
    levels, o = _levels("smoothed", "960")
    R = br.ordinary_block(A[0], 6)
    da = _up(api, A)
    h = da.amg(coarseRows=8, smoothed=True)
    never = da.amg(coarseRows=8, smoothed=True)                     # a hierarchy that never has a width
    try:
        base, where = int(h.info.bytes), _addresses(h)
        assert base == int(never.info.bytes) and h.block_info() == dict(width=0, bytes=0)
        z0 = h.apply(b)
        x0, i0 = da.cg(b, precond=h, tol=KRYLOV_TOL, maxiter=200, history=True)
        for width in (6, 9, 6):
            h.set_block_width(width)
            assert h.block_info() == dict(width=width, bytes=_expected_bytes(h, width))
            assert int(h.info.bytes) == base + _expected_bytes(h, width) and _addresses(h) == where
            want = br.block_cycle_ref(levels, o, R, cr.smoother(o, kind=cr.JACOBI))
            assert_same_bits(h.apply_block(R), want, f"width {width}, k = 6")          # k equal to the width, and below it
            assert_same_bits(h.apply_block(np.ascontiguousarray(R[:, :4])), want[:, :4], f"width {width}, k = 4")
            # the single cycle and the single solve: the bits and launches of the hierarchy that never had a width
            assert_same_bits(h.apply(b), z0, "the single cycle after a block cycle")
            assert_same_bits(never.apply(b), z0, "a hierarchy without a width")
            x1, i1 = da.cg(b, precond=h, tol=KRYLOV_TOL, maxiter=200, history=True)
            x2, i2 = da.cg(b, precond=never, tol=KRYLOV_TOL, maxiter=200, history=True)
            assert_same_bits(x1, x0, "the single solve")
            assert_same_bits(x2, x0, "the single solve without a width")
            assert (i1.iterations, i1.launches) == (i0.iterations, i0.launches) == (i2.iterations, i2.launches)
            assert_same_bits(i1.history, i0.history, "history")
        h.set_block_width(0)
        assert h.block_info() == dict(width=0, bytes=0) and int(h.info.bytes) == base and _addresses(h) == where
        with pytest.raises(api.SpmvHipError):
            h.apply_block(R)
    finally:
        never.free()
        h.free()
        da.free()


def _new_values(LAP):
    """other values on LAP's pattern, the diagonal scaled row by row: rho moves on every level"""
    rng = np.random.default_rng(11)
    new = LAP[4] * (1.0 + 0.25 * rng.random(LAP[4].size))
    rows = sr.si.row_of_entry(LAP[2])
    diag = LAP[3].astype(np.int64) == rows
    new[diag] = new[diag] * (1.0 + rng.random(int(diag.sum())))
    return LAP[:4] + (new,)


@pytest.mark.parametrize("smoother", ["jacobi223", "cheb314"])
@pytest.mark.parametrize("hierarchy", ["plain", "smoothed"])
def test_a_captured_block_cycle_replayed_after_a_refresh(api, hierarchy, smoother):
    import torch
    LAP = sr.laplacian7(12, 10, 8)
    B = _new_values(LAP)
    M, k = LAP[0], 5
    old, o = cr.setup_ref(LAP, hierarchy, coarseRows=8)
    new, _ = cr.setup_ref(B, hierarchy, coarseRows=8)
    sm = br.smoother_of(o, smoother)
    if sm["kind"] == cr.CHEBYSHEV:
        assert all(_bits(a["rho"]) != _bits(b["rho"]) for a, b in zip(cr.tables(old, sm), cr.tables(new, sm))), "every rho moves"
    R = br.ordinary_block(M, k)
    da, db = _up(api, LAP), _up(api, B)
    h = da.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    fresh = db.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    try:
        for x in (h, fresh):
            _set_smoother(x, smoother)
            x.set_block_width(k)
        where, block = [h.smoother(l)["dCoef"] for l in range(h.info.levels)], h.block_info()
        Rt, Zt = torch.from_numpy(R).cuda(), torch.zeros((M, k), dtype=torch.float64, device="cuda")
        h.apply_block(Rt, out=Zt)                                    # (every kernel has run once before the capture)
        Zt.zero_()
        api.lib.spmvHipSetSync(0)
        s = torch.cuda.Stream()
        api.lib.spmvHipSetStream(C.c_void_p(s.cuda_stream))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):                      # a single-stream chain: nothing parallel is replayed
                h.apply_block(Rt, out=Zt)
        g.replay()
        torch.cuda.synchronize()
        assert_same_bits(Zt.cpu().numpy(), br.block_cycle_ref(old, o, R, sm), "captured replay")
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        da.update_values(B[4])
        h.refresh_from(da)
        assert [h.smoother(l)["dCoef"] for l in range(h.info.levels)] == where and h.block_info() == block
        Zt.zero_()
        g.replay()
        torch.cuda.synchronize()
        Z = Zt.cpu().numpy()
        assert_same_bits(Z, br.block_cycle_ref(new, o, R, sm), "the same graph after the refresh")
        assert_same_bits(Z, fresh.apply_block(R), "refreshed against a fresh setup")
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        fresh.free()
        h.free()
        db.free()
        da.free()


def test_the_smoother_set_before_and_after_the_width(api):
    A = sr.laplacian7(12, 10, 8)
    levels, o = _levels("smoothed", "960")
    R = br.ordinary_block(A[0], 3)
    da = _up(api, A)
    first, then = da.amg(coarseRows=8, smoothed=True), da.amg(coarseRows=8, smoothed=True)
    try:
        first.set_block_width(3)
        for name in ("cheb222", "jacobi223", "cheb314"):
            _set_smoother(first, name)                               # the smoother after the width: the width is kept
            assert first.block_info()["width"] == 3
            then.set_block_width(0)
            _set_smoother(then, name)
            then.set_block_width(3)                                  # the width after the smoother
            want = br.block_cycle_ref(levels, o, R, br.smoother_of(o, name))
            assert_same_bits(first.apply_block(R), want, name)
            assert_same_bits(then.apply_block(R), want, name)
    finally:
        then.free()
        first.free()
        da.free()


def test_a_gauss_seidel_hierarchy_is_refused_and_works_again_as_jacobi(api, capfd):
    A, b = krylov_problem(SHAPES["960"])
    levels, o = _levels("plain", "960")
    R = br.ordinary_block(A[0], 2)
    da = _up(api, A)
    h = da.amg(coarseRows=8)
    try:
        h.set_block_width(2)
        h.set_gauss_seidel()
        assert h.block_info()["width"] == 2
        state = _state(h)
        capfd.readouterr()
        for call in (lambda: h.apply_block(R), lambda: da.cg_block(R, precond=h, maxiter=5), lambda: da.bicgstab_block(R, precond=h, maxiter=5)):
            with pytest.raises(api.SpmvHipError):
                call()
            err = capfd.readouterr().err
            assert "multigrid hierarchy" in err and "Gauss-Seidel" in err, err
        assert _state(h) == state
        h.set_smoother("jacobi")
        assert h.block_info()["width"] == 2
        assert_same_bits(h.apply_block(R), br.block_cycle_ref(levels, o, R, cr.smoother(o, kind=cr.JACOBI)), "Jacobi again")
    finally:
        h.free()
        da.free()


# -------------------------------------------------------------------------------------------------------------- solves
def _enqueued(iterations, K=16, maxiter=200):
    return min(maxiter, -(-iterations // K) * K)


def _solve_launches(method, enq, cycle):
    """the kernels of a block solve that enqueued `enq` iterations, M^-1 one cycle of `cycle` kernels.  CG: 4 before the loop
    and 6 per iteration, and every M^-1 (one before the loop, one per iteration) with a dot pass and its finish; BiCGStab: 3
    before the loop, 11 per iteration and two M^-1"""
    return 4 + 6 * enq + (enq + 1) * (cycle + 2) if method == "cg" else 3 + enq * (11 + 2 * cycle)


def _same_number(a, b):
    """the same bits, or both NaN (the device's NaN and numpy's may differ in sign and payload)"""
    return bool(_bits(a) == _bits(b)) or bool(np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("case", [("plain", "jacobi118"), ("smoothed", "cheb222"), ("strength", "jacobi223")])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_block_solves_with_the_hierarchy(api, method, case):
    hierarchy, smoother = case
    shape = SHAPES["960"]
    A = _matrix(hierarchy, shape)
    b = krylov_problem(shape)[1]
    levels, o = _levels(hierarchy, "960")
    kind, nu1, nu2, nuCoarse = br.SMOOTHERS[smoother]
    ref = cr.ChebCsr(A, levels=levels, o=o, sm=dict(kind=kind, nu1=nu1, nu2=nu2, nuCoarse=nuCoarse))
    nan = b.copy()
    nan[17] = np.nan
    B = np.stack([b, 3.0 * b + 1.0, np.zeros_like(b), nan, 0.5 * b], axis=1)      # columns that stop at different iterations
    X0 = np.zeros_like(B)
    cols, (status, iterations, rr, bb) = br.block_solve_ref(method, ref, B, X0, KRYLOV_TOL, 200)
    assert cols[2].iterations == 0 and cols[3].iterations == 0 and cols[0].iterations > 1
    da = _up(api, A)
    h = da.amg(coarseRows=8, **HIERARCHIES[hierarchy])
    try:
        _set_smoother(h, smoother)
        singles = [getattr(da, method)(np.ascontiguousarray(B[:, c]), precond=h, tol=KRYLOV_TOL, maxiter=200, history=True) for c in range(5)]
        h.set_block_width(6)
        for K in (1, 16):
            api.set_variant("hipSpCGBlockCSR" if method == "cg" else "hipSpBiCGStabBlockCSR", K)
            X, info = getattr(da, method + "_block")(B, precond=h, tol=KRYLOV_TOL, maxiter=200, history=True)
            assert (info.status, info.iterations) == (status, iterations)
            assert _same_number(info.rr, rr) and _same_number(info.bb, bb)
            for c, (col, want, (sx, si)) in enumerate(zip(info.columns, cols, singles)):
                what = f"{method}, K = {K}, column {c}"
                _same(X[:, c], want.x, what + ": x against the reference")
                _same(X[:, c], sx, what + ": x against the single solve")
                assert (col.status, col.iterations) == (want.status, want.iterations) == (si.status, si.iterations), what
                for got, a, s in ((col.rr, want.rr, si.rr), (col.bb, want.bb, si.bb)):
                    assert _same_number(got, a) and _same_number(got, s), what
                _same(info.history[c], np.asarray(want.history), what + ": history")
                _same(info.history[c], si.history, what + ": history against the single solve")
        # launches: whole batches of K = 16 iterations, every M^-1 one block cycle whatever k is
        cycle = _launches(h, hierarchy, smoother)
        enq = _enqueued(iterations)
        formula = _solve_launches(method, enq, cycle)
        assert info.launches == formula, (info.launches, formula, cycle, enq)
        h.set_block_width(33)
        for k in (2, 16, 33):
            Bk = np.stack([b * 2.0 ** (c % 5 - 2) for c in range(k)], axis=1)
            Xk, ik = getattr(da, method + "_block")(Bk, precond=h, tol=KRYLOV_TOL, maxiter=200)
            assert ik.launches == _solve_launches(method, _enqueued(ik.iterations), cycle), (k, ik.launches)
            assert ik.iterations == cols[0].iterations, "scaling by a power of two changes no count"
            for c in range(k):
                assert_same_bits(Xk[:, c], singles[0][0] * 2.0 ** (c % 5 - 2), f"k = {k}, column {c}")
        # k = 1: one column as a block
        X1, i1 = getattr(da, method + "_block")(np.ascontiguousarray(B[:, :1]), precond=h, tol=KRYLOV_TOL, maxiter=200)
        assert_same_bits(X1[:, 0], singles[0][0], "k = 1")
        assert i1.iterations == singles[0][1].iterations
    finally:
        h.free()
        da.free()


def test_refusals_leave_everything_as_it_was(api, capfd):
    import torch
    lib = api.lib
    A, b = krylov_problem(SHAPES["960"])
    M, k = A[0], 4
    other = _up(api, sr.laplacian7(12, 10, 8))
    ell = api.spMatCpyELL(api.HostCSR(*A).to_ell())
    da = _up(api, A)
    h = da.amg(coarseRows=8, smoothed=True)
    none = da.amg(coarseRows=8, smoothed=True)
    try:
        h.set_block_width(k)
        big = torch.full((2 * M * (k + 2),), SENTINEL, dtype=torch.float64, device="cuda")
        R = torch.from_numpy(br.ordinary_block(M, k)).cuda()
        Z = torch.full((M, k), SENTINEL, dtype=torch.float64, device="cuda")
        HM, HA, HN = C.byref(h.handle), C.byref(da.handle), C.byref(none.handle)
        ROW, COL = api.SPMV_DENSE_ROW_MAJOR, api.SPMV_DENSE_COL_MAJOR
        opts = api.spmvKrylovOpts(1e-8, 5, None)

        def apply(m=HM, a=HA, kk=k, r=R.data_ptr(), ldr=k, rl=ROW, z=Z.data_ptr(), ldz=k, zl=ROW):
            return lib.spmvHipAmgApplyBlock(m, a, kk, r, ldr, rl, z, ldz, zl)

        def solve(fn, m=HM, a=HA, kk=k):
            return fn(a, m, kk, R.data_ptr(), k, ROW, Z.data_ptr(), k, ROW, C.byref(opts), None, None)
        calls = {
            "no width": (lambda: apply(m=HN), "spmvHipAmgSetBlockWidth"),
            "width < k": (lambda: apply(kk=k + 1, r=big.data_ptr(), ldr=k + 1, z=big.data_ptr() + 8 * M * (k + 1), ldz=k + 1), "width 4, k = 5"),
            "another matrix": (lambda: apply(a=C.byref(other.handle)), "dA is not the handle"),
            "an ELL dA": (lambda: apply(a=C.byref(ell.handle)), "ELL"),
            "not a hierarchy": (lambda: apply(m=HA), "was not made by"),
            "k = 0": (lambda: apply(kk=0), "k = 0"),
            "layout": (lambda: apply(zl=7), "layout"),
            "ldr": (lambda: apply(ldr=k - 1), "ldr"),
            "ldz": (lambda: apply(zl=COL, ldz=M - 1), "ldz"),
            "NULL R": (lambda: apply(r=None), "dR is NULL"),
            "NULL Z": (lambda: apply(z=None), "dZ is NULL"),
            "same block": (lambda: apply(r=Z.data_ptr()), "overlap"),
            "spans": (lambda: apply(r=big.data_ptr(), ldr=k + 1, z=big.data_ptr() + 8 * k, ldz=k + 1), "overlap"),
            "cg: no width": (lambda: solve(lib.hipSpCGBlockCSR, m=HN), "multigrid hierarchy"),
            "bicgstab: no width": (lambda: solve(lib.hipSpBiCGStabBlockCSR, m=HN), "multigrid hierarchy"),
            "cg: another matrix": (lambda: solve(lib.hipSpCGBlockCSR, a=C.byref(other.handle)), "dA is not the handle"),
            "width: another matrix": (lambda: lib.spmvHipAmgSetBlockWidth(HM, C.byref(other.handle), 8), "dA is not the handle"),
            "width: not a hierarchy": (lambda: lib.spmvHipAmgSetBlockWidth(HA, HA, 8), "was not made by"),
            "width: NULL": (lambda: lib.spmvHipAmgSetBlockWidth(None, HA, 8), "NULL"),
            "width: too much memory": (lambda: lib.spmvHipAmgSetBlockWidth(HM, HA, 0xFFFFFFFE), "allocation"),
            "block: NULL info": (lambda: lib.spmvHipAmgBlock(HM, None), "info is NULL"),
        }
        state = (_state(h), _state(none))
        zb, bb = Z.clone(), big.clone()
        for name, (call, text) in calls.items():
            capfd.readouterr()
            assert call() != 0, name
            err = capfd.readouterr().err
            assert text in err, (name, err)
            if "width" in name and name.split(":")[0] in ("no width", "width < k", "cg", "bicgstab"):
                assert "multigrid hierarchy" in err, (name, err)
            assert torch.equal(Z.view(torch.int64), zb.view(torch.int64)) and torch.equal(big.view(torch.int64), bb.view(torch.int64)), name
            assert (_state(h), _state(none)) == state, name
        # and everything still works
        assert_same_bits(h.apply_block(R).cpu().numpy(), np.stack([h.apply(R[:, c].contiguous()).cpu().numpy() for c in range(k)], axis=1), "after the refusals")
    finally:
        none.free()
        h.free()
        da.free()
        ell.free()
        other.free()
