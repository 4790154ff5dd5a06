"""hipSpCGBlockCSR / hipSpBiCGStabBlockCSR on the device against the block reference (tests/block_krylov_ref.py: column by
column the single loops of tests/krylov_ref.py), bit for bit: every column's x, status, iterations, rr, bb and history.
The sums of tests/block_exit_inputs.py send the columns of one block through different exits at different iterations,
at K = 1, 16 and 64 iterations per host check: a column that has stopped must stay frozen while its neighbours run on and
while the host enqueues far past its stop.  X and the history start as a sentinel bit pattern, padding included; nothing
past `iterations_c` and nothing outside the block may be written."""
import ctypes as C
import functools

import numpy as np
import pytest

import block_exit_inputs as sums
import serial_order_inputs as si
from bits import assert_same_bits
from block_krylov_ref import block_ref, block_x
from ilu0_ref import ilu0_levels
from krylov_ref import CONVERGED, MAXITER, NONFINITE, Csr
from test_gpu_trsm import COL, ROW, SENTINEL, Block, layouts_of
from test_gpu_trsv import Source, same
from test_krylov_abi import convdiff7
from test_trsv_abi import laplacian7
from transpose_ref import stable_transpose

pytestmark = pytest.mark.gpu

FN = {"cg": "hipSpCGBlockCSR", "bicgstab": "hipSpBiCGStabBlockCSR"}
SINGLE = {"cg": "hipSpCGCSR", "bicgstab": "hipSpBiCGStabCSR"}
LAYOUTS = ("row", "row+3", "col", "col+5")
ODD_GRID = (21, 19, 17)                 # n = 6 783: one whole block of 4 096 and a short one, an odd count of rows


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.lib.spmvHipSetStream(None)
    api.lib.spmvHipSetSync(1)
    for name in list(FN.values()) + list(SINGLE.values()):
        api.lib.spmvHipSetVariant(name.encode(), 16)


def set_k(api, kind, K):
    assert api.lib.spmvHipSetVariant(FN[kind].encode(), K) == 0


def raw(api, kind, A, P, k, B, X, tol, maxiter, history=True, want_cols=True):
    """the C call on two Blocks with a history full of sentinels: (return code, info, columns, history (k, maxiter + 1))"""
    hist = np.full((k, maxiter + 1), SENTINEL, dtype=np.uint64).view(np.float64)
    opts = api.spmvKrylovOpts(float(tol), int(maxiter), hist.ctypes.data_as(C.POINTER(C.c_double)) if history else None)
    info = api.spmvKrylovInfo()
    cols = (api.spmvKrylovColumn * k)()
    rc = getattr(api.lib, FN[kind])(C.byref(A.handle), C.byref(P.handle) if P is not None else None, k, C.c_void_p(B.ptr), B.ld,
                                    B.layout, C.c_void_p(X.ptr), X.ld, X.layout, C.byref(opts), cols if want_cols else None,
                                    C.byref(info))
    return rc, info, cols, hist


def check(got, ref, Xh, what):
    """every column and the block's info against the reference; the history past iterations_c is not written"""
    rc, info, cols, hist = got
    rcols, rinfo = ref
    assert rc == 0, what
    for c, r in enumerate(rcols):
        w = f"{what}, column {c} ({r.label})"
        assert (cols[c].status, cols[c].iterations) == (r.status, r.iterations), (w, cols[c].status, cols[c].iterations, r.status, r.iterations)
        same(Xh[:, c], r.x, w + ": x")
        same(hist[c, :r.iterations + 1], r.history, w + ": history")
        assert (hist[c, r.iterations + 1:].view(np.uint64) == SENTINEL).all(), w + ": history written past `iterations`"
        same(np.array([cols[c].rr, cols[c].bb]), np.array([r.rr, r.bb]), w + ": rr, bb")
    assert (info.status, info.iterations) == rinfo[:2], (what, info.status, info.iterations, rinfo[:2])
    same(np.array([info.rr, info.bb]), np.array(rinfo[2:]), what + ": info.rr, info.bb")
    assert info.launches > 0 and info.hostChecks > 0


def solve(api, torch, kind, A, P, Bh, X0h, tol, maxiter, bl="row", xl="row", off=0, what=""):
    """B and X in the named layouts at element offset `off`, X from X0 in a field of sentinels; returns (the C call's
    results, X's block) after checking the padding of both and that B was only read"""
    M, k = Bh.shape
    lay = layouts_of(M, k)
    B = Block(torch, M, k, *lay[bl], off=off, host=Bh)
    X = Block(torch, M, k, *lay[xl], off=off, host=X0h)
    got = raw(api, kind, A, P, k, B, X, tol, maxiter)
    torch.cuda.synchronize()
    X.padding_intact(what)
    B.padding_intact(what + " (B)")
    assert_same_bits(B.down(), Bh, what + ": B is read only")
    return got, X.down()


def factored(api, M, IRP, JA, AS):
    P = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P.ilu0()
    return P


# ------------------------------------------------------------------------------------------------- 1. the sums and their twins
@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("kind,precond", sums.KINDS)
def test_columns_leave_by_different_exits(api, torch, kind, precond, large):
    s = sums.block_sum(kind, precond, large)
    _, rcols, rinfo = sums.reference(kind, precond, large)
    M, k = s.B.shape
    A = api.spMatCpyCSR(api.HostCSR(M, M, s.IRP, s.JA, s.AS))
    P = factored(api, M, s.IRP, s.JA, s.AS) if precond else None
    B = Block(torch, M, k, ROW, k, host=s.B)
    X = Block(torch, M, k, ROW, k + (0 if large else 3), host=s.X0)
    start = X.flat.clone()
    xs = {}
    try:
        for K in (1, 16, 64):
            set_k(api, kind, K)
            X.flat.copy_(start)
            got = raw(api, kind, A, P, k, B, X, sums.TOL, sums.MAXITER)
            torch.cuda.synchronize()
            xs[K] = X.down()
            check(got, (rcols, rinfo), xs[K], f"{s.name} K={K}")
            X.padding_intact(f"{s.name} K={K}")
        for K in (16, 64):
            assert_same_bits(xs[K], xs[1], f"{s.name}: X at K={K} against K=1")
        for c, r in enumerate(rcols):                                    # x = x + alpha*phat, written after the stop word was set
            if r.label in ("half_converged", "tt0"):
                assert not np.array_equal(xs[1][:, c], s.X0[:, c]), (s.name, c)
                with np.errstate(all="ignore"):
                    same(xs[1][:, c], r.half["x"] + r.half["alpha"] * r.half["phat"], f"{s.name}, column {c}: x + alpha * phat")
        assert_same_bits(B.down(), s.B, s.name + ": B is read only")
    finally:
        A.free()
        if P is not None:
            P.free()


@pytest.mark.parametrize("kind,precond", sums.KINDS)
def test_max_iter_zero(api, torch, kind, precond):
    """init_maxiter, the exit the sums cannot take at maxIter = 6: every column stops at the init, no further kernel"""
    s = sums.block_sum(kind, precond)
    A_ref = sums.reference(kind, precond)[0]
    ref = block_ref(kind, A_ref, s.B, s.X0, sums.TOL, 0)
    assert "init_maxiter" in {c.label for c in ref[0]}
    M, k = s.B.shape
    A = api.spMatCpyCSR(api.HostCSR(M, M, s.IRP, s.JA, s.AS))
    P = factored(api, M, s.IRP, s.JA, s.AS) if precond else None
    try:
        got, Xh = solve(api, torch, kind, A, P, s.B, s.X0, sums.TOL, 0, what=s.name + " maxIter=0")
        check(got, ref, Xh, s.name + " maxIter=0")
        assert got[1].hostChecks == 1 and got[1].launches == 3           # the product, the init pass and its finish
        assert_same_bits(Xh, s.X0, "x is x0")
    finally:
        A.free()
        if P is not None:
            P.free()


# ------------------------------------------------------------------------------------------------- 2. a grid of 6 783 rows
@functools.lru_cache(maxsize=None)
def grid_case(kind, mode):
    """the 21 x 19 x 17 Laplacian (BiCGStab: its upwind twin), k = 5: columns of different scales, one zero column and one
    A * 1 column; mode: "none", "ilu0" or "dM==dA" (A holds its own ILU(0) factors); the reference, computed once"""
    IRP, JA, AS = (laplacian7 if kind == "cg" else convdiff7)(*ODD_GRID)
    M = int(np.prod(ODD_GRID))
    rng = np.random.default_rng(2900)
    F = ilu0_levels(M, IRP, JA, AS) if mode != "none" else None
    if mode == "dM==dA":
        AS = F
    B = np.stack([rng.random(M), 1e6 * rng.random(M), np.zeros(M), Csr(M, IRP, JA, AS).spmv(np.ones(M)), 1e-7 * rng.random(M)], axis=1)
    X0 = np.zeros((M, 5))
    X0[:, 4] = rng.uniform(-1, 1, M)
    ref = block_ref(kind, Csr(M, IRP, JA, AS, F), B, X0, 1e-6, 200)
    for a in (B, X0):
        a.setflags(write=False)
    return M, IRP, JA, AS, B, X0, ref


@pytest.mark.parametrize("mode", ["none", "ilu0", "dM==dA"])
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_layouts_offsets_and_check_intervals(api, torch, kind, mode):
    M, IRP, JA, AS, B, X0, ref = grid_case(kind, mode)
    assert M % 2 == 1 and M > 4096 and len({c.iterations for c in ref[0]}) >= 2
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P = A if mode == "dM==dA" else factored(api, M, *((laplacian7 if kind == "cg" else convdiff7)(*ODD_GRID))) if mode == "ilu0" else None
    try:
        first = None
        for bl in LAYOUTS:                                               # all four layouts for B and X, independently
            for xl in LAYOUTS:
                what = f"{kind} {mode} B {bl} X {xl}"
                got, Xh = solve(api, torch, kind, A, P, B, X0, 1e-6, 200, bl, xl, off=0, what=what)
                check(got, ref, Xh, what)
                first = Xh if first is None else first
        for bl, xl in (("row", "row"), ("row+3", "col"), ("col+5", "row+3")):     # an odd element offset: 8-byte aligned only
            what = f"{kind} {mode} B {bl} X {xl} at offset 1"
            got, Xh = solve(api, torch, kind, A, P, B, X0, 1e-6, 200, bl, xl, off=1, what=what)
            check(got, ref, Xh, what)
        for K in (1, 64):                                                # (16 is the default of the calls above)
            set_k(api, kind, K)
            got, Xh = solve(api, torch, kind, A, P, B, X0, 1e-6, 200, what=f"{kind} {mode} K={K}")
            check(got, ref, Xh, f"{kind} {mode} K={K}")
            assert_same_bits(Xh, first, f"{kind} {mode}: X at K={K} against K=16")
    finally:
        A.free()
        if P is not None and P is not A:
            P.free()


# ------------------------------------------------------------------------------------------------- 3. panel edges
@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_panel_edges_against_the_single_solve_on_the_device(api, torch, kind, precond):
    """k = 1, 17 and 33 on an 8^3 Laplacian: column c equals hipSpCGCSR / hipSpBiCGStabCSR on a contiguous copy of column c,
    device against device; info.launches does not depend on k"""
    n = 8
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    rng = np.random.default_rng(2910)
    base = np.stack([rng.random(M) * 10.0 ** rng.integers(-3, 4) for _ in range(33)], axis=1)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P = factored(api, M, IRP, JA, AS) if precond else None
    try:
        singles = {}
        for k in (1, 17, 33):
            (rc, info, cols, hist), Xh = solve(api, torch, kind, A, P, base[:, :k], np.zeros((M, k)), 1e-9, 60, "row+3", "col",
                                                what=f"k {k}")
            assert rc == 0
            for c in range(k):
                if c not in singles:
                    b = torch.from_numpy(np.ascontiguousarray(base[:, c])).cuda()
                    x, si_ = getattr(A, kind)(b, precond=P, tol=1e-9, maxiter=60, history=True)
                    singles[c] = (x.cpu().numpy(), si_)
                x, si_ = singles[c]
                w = f"{kind} k {k}, column {c}"
                assert_same_bits(Xh[:, c], x, w + ": x")
                assert (cols[c].status, cols[c].iterations) == (si_.status, si_.iterations), w
                assert_same_bits(np.array([cols[c].rr, cols[c].bb]), np.array([si_.rr, si_.bb]), w + ": rr, bb")
                assert_same_bits(hist[c, :si_.iterations + 1], si_.history, w + ": history")
        Bh = np.ascontiguousarray(base[:, :1])                           # k = 1 with unit strides: the single solve's kernels
        for bl, xl in (("row", "row"), ("col", "col+5")):
            (rc, info, cols, hist), Xh = solve(api, torch, kind, A, P, Bh, np.zeros((M, 1)), 1e-9, 60, bl, xl, what="k 1, unit strides")
            x, si_ = singles[0]
            assert rc == 0 and (cols[0].status, cols[0].iterations, info.iterations) == (si_.status, si_.iterations, si_.iterations)
            assert_same_bits(Xh[:, 0], x, "k 1, unit strides: x")
            assert_same_bits(hist[0, :si_.iterations + 1], si_.history, "k 1, unit strides: history")
        launches = []
        for k in (2, 16, 33):                                            # the same two columns repeated: the same count of iterations
            Bh = np.ascontiguousarray(base[:, np.arange(k) % 2])
            (rc, info, cols, _), _ = solve(api, torch, kind, A, P, Bh, np.zeros((M, k)), 1e-9, 60, what=f"launches, k {k}")
            assert rc == 0
            launches.append(info.launches)
        assert launches[0] == launches[1] == launches[2], launches
    finally:
        A.free()
        if P is not None:
            P.free()


# ------------------------------------------------------------------------------------------------- 4. columns are independent
@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_huge_and_nan_columns_stay_in_their_column(api, torch, kind, precond):
    n = 10
    IRP, JA, AS = (laplacian7 if kind == "cg" else convdiff7)(n, n, n)
    M = n ** 3
    rng = np.random.default_rng(2920)
    clean = np.stack([rng.random(M) for _ in range(5)], axis=1)
    dirty = clean.copy()
    dirty[:, 1] = 1e308 * (0.5 + 0.25 * rng.random(M))
    dirty[:, 3] = np.nan
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P = factored(api, M, IRP, JA, AS) if precond else None
    F = ilu0_levels(M, IRP, JA, AS) if precond else None
    try:
        (rc0, _, cols0, hist0), X0 = solve(api, torch, kind, A, P, clean, np.zeros((M, 5)), 1e-10, 80, what="clean")
        got, X1 = solve(api, torch, kind, A, P, dirty, np.zeros((M, 5)), 1e-10, 80, what="dirty")
        assert rc0 == 0
        check(got, block_ref(kind, Csr(M, IRP, JA, AS, F), dirty, np.zeros((M, 5)), 1e-10, 80), X1, f"{kind} precond={precond}")
        cols1, hist1 = got[2], got[3]
        assert cols1[3].status == NONFINITE and cols1[3].iterations == 0 and np.isinf(cols1[1].rr)
        for c in (0, 2, 4):                                              # the neighbours: the bits they have without them
            assert_same_bits(X1[:, c], X0[:, c], f"column {c}: x")
            assert (cols1[c].status, cols1[c].iterations) == (cols0[c].status, cols0[c].iterations) and cols1[c].status == CONVERGED
            assert_same_bits(hist1[c].view(np.uint64), hist0[c].view(np.uint64), f"column {c}: history")
    finally:
        A.free()
        if P is not None:
            P.free()


# ------------------------------------------------------------------------------------------------- 5. handle kinds
def test_unit_value_adopted_and_transpose_handles(api, torch):
    n = 9
    IRP, JA, AS = convdiff7(n, n, n)
    M = n ** 3
    rng = np.random.default_rng(2930)
    Bh = np.stack([rng.random(M) * s for s in (1.0, 100.0, 0.01)], axis=1)
    Z = np.zeros((M, 3))
    ones = np.ones_like(AS)
    src = Source(api, M, M, IRP, JA, ones)                               # every value 1.0: a unit-value handle
    try:
        v = C.c_double(0)
        assert api.lib.spmvHipUnitValue(C.byref(src.dm.handle), C.byref(v)) == 1
        got, Xh = solve(api, torch, "bicgstab", src.dm, None, Bh, Z, 1e-8, 20, what="unit-value")
        check(got, block_ref("bicgstab", Csr(M, IRP, JA, ones), Bh, Z, 1e-8, 20), Xh, "unit-value handle")
    finally:
        src.free()
    F = ilu0_levels(M, IRP, JA, AS)
    for adopt in (4, 8):
        src, pre = Source(api, M, M, IRP, JA, AS, adopt=adopt), Source(api, M, M, IRP, JA, AS, adopt=adopt)
        try:
            pre.dm.ilu0()
            got, Xh = solve(api, torch, "bicgstab", src.dm, pre.dm, Bh, Z, 1e-10, 100, "col", "row+3", what=f"adopted {adopt}")
            check(got, block_ref("bicgstab", Csr(M, IRP, JA, AS, F), Bh, Z, 1e-10, 100), Xh, f"adopted {adopt}")
        finally:
            src.free()
            pre.free()
    src = Source(api, M, M, IRP, JA, AS)
    t = src.dm.transpose()
    try:
        IRPt, JAt, ASt, _ = stable_transpose(M, IRP, JA, AS)
        got, Xh = solve(api, torch, "bicgstab", t, None, Bh, Z, 1e-10, 100, what="transpose")
        check(got, block_ref("bicgstab", Csr(M, IRPt, JAt, ASt), Bh, Z, 1e-10, 100), Xh, "a transpose handle")
    finally:
        t.free()
        src.free()


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_x_untouched(api, torch, capfd):
    n = 6
    IRP, JA, AS = laplacian7(n, n, n)
    M, k = n ** 3, 3
    rng = np.random.default_rng(2940)
    keep = []
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    keep.append(A)
    B = Block(torch, M, k, ROW, k, host=rng.random((M, k)))
    X = Block(torch, M, k, ROW, k, host=np.full((M, k), 3.25))
    big = Block(torch, 2 * M, k, ROW, k)
    start = X.flat.clone()
    try:
        P = C.byref
        for kind in ("cg", "bicgstab"):
            fn = getattr(api.lib, FN[kind])

            def call(dA=A, dM=None, kk=k, b=B.ptr, ldb=k, bl=ROW, x=X.ptr, ldx=k, xl=ROW, tol=1e-8, maxiter=10, hist=None, opts=True):
                o = api.spmvKrylovOpts(tol, maxiter, hist)
                info = api.spmvKrylovInfo()
                return lambda: fn(P(dA.handle) if dA is not None else None, P(dM.handle) if dM is not None else None, kk,
                                  C.c_void_p(b) if b else None, ldb, bl, C.c_void_p(x) if x else None, ldx, xl,
                                  P(o) if opts else None, None, P(info))

            def refused(c, msg=None, x=X):
                torch.cuda.synchronize()
                before = x.flat.cpu().numpy().view(np.uint64).copy()
                capfd.readouterr()
                assert c() == 1
                err = capfd.readouterr().err
                assert FN[kind] in err, err
                if msg:
                    assert msg in err, err
                torch.cuda.synchronize()
                assert np.array_equal(x.flat.cpu().numpy().view(np.uint64), before)

            # those of the single solves
            refused(call(dA=None))
            refused(call(b=None), "NULL")
            refused(call(x=None), "NULL")
            refused(call(opts=False), "NULL")
            refused(call(tol=-1.0), "tol")
            refused(call(tol=float("nan")), "tol")
            refused(call(maxiter=(1 << 64) - 1, hist=C.cast(C.c_void_p(8), C.POINTER(C.c_double))), "history")
            refused(call(maxiter=(1 << 61), hist=C.cast(C.c_void_p(8), C.POINTER(C.c_double))), "history")
            if kind == "cg":
                rect = api.spMatCpyCSR(api.HostCSR(M, M + 1, IRP, JA, AS))
                ell = api.spMatCpyELL(api.HostCSR(M, M, IRP, JA, AS).to_ell())
                IRPs, JAs, ASs = laplacian7(5, 5, 5)
                other = api.spMatCpyCSR(api.HostCSR(125, 125, IRPs, JAs, ASs))
                rows = si.row_of_entry(IRP)
                off = JA.astype(np.int64) != rows
                nodiag = api.spMatCpyCSR(api.HostCSR(M, M, *si.assemble(M, rows[off], JA.astype(np.int64)[off], AS[off])))
                amg = A.amg(coarseRows=8)
                keep += [rect, ell, other, nodiag, amg]
            rect, ell, other, nodiag, amg = keep[1:6]
            refused(call(dA=rect), "square")
            refused(call(dA=ell), "ELL")
            refused(call(dM=other), "rows")
            refused(call(dM=nodiag), "diagonal")
            refused(call(dM=amg), "hierarchy")                           # its cycle is single-vector
            # those of hipSpTRSMCSR for k, the layouts, the leading dimensions and the spans
            refused(call(kk=0), "k = 0")
            refused(call(bl=2), "layout")
            refused(call(xl=-1), "layout")
            refused(call(ldb=k - 1), "ldb")
            refused(call(ldx=k - 1), "ldx")
            refused(call(bl=COL, ldb=M - 1), "ldb")
            refused(call(xl=COL, ldx=M - 1), "ldx")
            refused(call(b=X.ptr), "overlap")
            refused(call(b=X.ptr, bl=COL, ldb=M), "overlap")
            refused(call(b=big.ptr, x=big.ptr + 8 * (M * k // 2)), "overlap", x=big)
            refused(call(b=big.ptr + 8 * (M * k - 1), x=big.ptr), "overlap", x=big)
            # and the handle still solves
            assert call()() == 0
            torch.cuda.synchronize()
            assert not np.array_equal(X.down(), np.full((M, k), 3.25))
            X.padding_intact("after the refusals")
            X.flat.copy_(start)
    finally:
        for m in keep[::-1]:
            m.free()


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_M_zero(api, torch, kind):
    empty = (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    A = Source(api, 0, 0, *empty)
    big = Block(torch, 4, 3, ROW, 3)
    try:
        B = Block(torch, 0, 3, ROW, 3)
        B.flat, B.off = big.flat, 0
        X = Block(torch, 0, 3, ROW, 3)
        X.flat, X.off = big.flat, 6
        rc, info, cols, hist = raw(api, kind, A.dm, None, 3, B, X, 1e-8, 5)
        assert rc == 0 and (info.status, info.iterations, info.hostChecks, info.launches) == (CONVERGED, 0, 0, 0)
        for c in range(3):
            assert (cols[c].status, cols[c].iterations) == (CONVERGED, 0)
            assert_same_bits(hist[c, :1], np.array([0.0]), "hist[0]")
            assert (hist[c, 1:].view(np.uint64) == SENTINEL).all()
        big.padding_intact("M = 0")
        assert (big.down().view(np.uint64) == SENTINEL).all()
    finally:
        A.free()


# ------------------------------------------------------------------------------------------------- 7. the Python layer
def test_python_layer(api, torch):
    M, IRP, JA, AS, B, X0, ref = grid_case("cg", "ilu0")
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P = factored(api, M, IRP, JA, AS)
    try:
        X, info = A.cg_block(np.array(B), X0=np.array(X0), precond=P, tol=1e-6, maxiter=200, history=True)     # numpy in, numpy out
        assert isinstance(X, np.ndarray) and len(info.columns) == 5 and len(info.history) == 5
        for c, r in enumerate(ref[0]):
            same(X[:, c], r.x, f"host call, column {c}")
            assert (info.columns[c].status, info.columns[c].iterations) == (r.status, r.iterations)
            same(info.history[c], r.history, f"host call, column {c}: history")
        Bt = torch.from_numpy(np.ascontiguousarray(B.T)).cuda().t()                                            # column-major B
        X0t = torch.from_numpy(np.array(X0)).cuda()
        Xt, info = A.cg_block(Bt, X0=X0t, precond=P, tol=1e-6, maxiter=200)
        assert isinstance(Xt, torch.Tensor) and Xt.is_cuda and Xt.data_ptr() != X0t.data_ptr()
        same(Xt.cpu().numpy(), block_x(ref[0]), "device call")
        assert_same_bits(X0t.cpu().numpy(), X0, "X0 is not written")
        Xb, _ = A.bicgstab_block(Bt, tol=1e-6, maxiter=3)
        assert tuple(Xb.shape) == (M, 5)
        with pytest.raises(api.SpmvHipError):
            A.cg_block(Bt[:-1])
        with pytest.raises(api.SpmvHipError):
            A.cg_block(Bt, X0=X0t[:, :4])
        with pytest.raises(api.SpmvHipError):
            A.cg_block(torch.zeros((M, 6), dtype=torch.float64, device="cuda")[:, ::2])
    finally:
        A.free()
        P.free()


# ------------------------------------------------------------------------------------------------- 8. determinism and memory
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_determinism_and_device_memory(api, torch, kind):
    """two runs give the same bytes; device memory is the same before the first and after the twentieth solve"""
    n = 12
    IRP, JA, AS = (laplacian7 if kind == "cg" else convdiff7)(n, n, n)
    M, k = n ** 3, 17
    rng = np.random.default_rng(2950)
    Bh = rng.random((M, k))
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P = factored(api, M, IRP, JA, AS)
    try:
        B = Block(torch, M, k, ROW, k, host=Bh)
        X = Block(torch, M, k, COL, M + 5, host=np.zeros((M, k)))
        start = X.flat.clone()
        rc, info, cols, hist = raw(api, kind, A, P, k, B, X, 1e-10, 100)
        assert rc == 0 and info.status == CONVERGED
        torch.cuda.synchronize()
        first, hist1 = X.flat.cpu().numpy().view(np.uint64).copy(), hist.view(np.uint64).copy()
        before = torch.cuda.mem_get_info()[0]
        for _ in range(20):
            X.flat.copy_(start)
            rc, info, cols, hist = raw(api, kind, A, P, k, B, X, 1e-10, 100)
            assert rc == 0
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == before
        assert np.array_equal(X.flat.cpu().numpy().view(np.uint64), first) and np.array_equal(hist.view(np.uint64), hist1)
    finally:
        A.free()
        P.free()
