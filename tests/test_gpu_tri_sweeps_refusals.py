"""What the sweep entry points refuse, and what a refused device allocation leaves (modelled on tests/test_gpu_alloc_refusals.py).

Refusals: every one listed in include/spmvHip.h for hipSpTRSVSweepsCSR, hipSpTRSMSweepsCSR, spmvHipTriSetApply,
spmvHipTriSweepsPrepare and spmvHipTriSweepsInfo, and those of a Krylov solve whose dM is in SWEEPS mode: EXIT_FAILURE, a
"libspmvhip" line that says why, the poisoned output still poisoned, the handle's plan what it was.
Allocations: every allocation of spmvHipTriSweepsPrepare refused in turn, alone and from then on -- the first build, the
widening, and the first-call prepare of a solve.  After each: the handle has no plan or the complete one, the ledger holds
what it held, no sticky error, the exact solve still works, and the same call unarmed succeeds with the reference's bits."""
import ctypes as C

import numpy as np
import pytest

import sweeps_inputs
from sweeps_ref import sweeps_numpy
from test_gpu_trsv import LOWER, STORED, UNIT, UPPER, Source, same
from test_trsv_abi import laplacian7, random_square
from trsv_ref import diag_pos, trsv_levels

pytestmark = pytest.mark.gpu
ROW, COL = 0, 1
FILL = 0x7FF8DEADBEEF0001


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.alloc_refuse(-1)
    a.spmvHipInit(0)
    yield a
    a.alloc_refuse(-1)
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.alloc_refuse(-1)


def _plan(dm):
    i = dm.triangular_sweeps_info()
    return tuple(getattr(i, f[0]) for f in i._fields_)


def _poisoned(api, v):
    return (v.down().view(np.uint64) == api.POISON_NAN).all()


def _no_sticky_error(api):
    v = api.DeviceVector(8)
    try:
        assert api.lib.spmvHipVecFill(v.ptr, 8, FILL) == 0
        assert (v.down().view(np.uint64) == FILL).all()
    finally:
        v.free()


def test_refusals_leave_outputs_and_handle_untouched(api, capfd):
    lib, P = api.lib, C.byref
    M, IRP, JA, AS, b = sweeps_inputs.make("r65")
    src = Source(api, M, M, IRP, JA, AS)
    rng = np.random.default_rng(4500)
    nodiag = Source(api, 100, 100, *random_square(rng, 100, 4, diag="none"))
    tw = random_square(rng, 100, 4, diag="twice")
    twice, twice_bad = Source(api, 100, 100, *tw), diag_pos(100, tw[0], tw[1])[1]
    assert twice_bad > 0
    lap = Source(api, 120, 120, *laplacian7(6, 5, 4))
    wide = api.spMatCpyCSR(api.HostCSR(3, 4, np.array([0, 1, 2, 3], np.uint64), np.array([0, 1, 3], np.uint64), np.ones(3)))
    dead = Source(api, M, M, IRP, JA, AS)
    dead.free()
    ell = api.csr_to_ell_device(src.dm, False)
    hier = lap.dm.amg()
    g = lap.dm.fsai()
    db, dx = api.DeviceVector(20 * M).up(np.resize(b, 20 * M)), api.DeviceVector(20 * M)
    h = P(src.dm.handle)
    bp, xp = db.ptr, dx.ptr
    shifted = C.c_void_p(bp.value + 8)
    info = api.spmvTriSweepsInfo()
    try:
        src.dm.prepare_triangular_sweeps(4)
        src.dm.set_triangular_apply((2, 3))
        plan = _plan(src.dm)
        trsv = lib.hipSpTRSVSweepsCSR
        trsm = lib.hipSpTRSMSweepsCSR
        cases = [
            ("trsv: dA is NULL", lambda: trsv(None, LOWER, STORED, 1, bp, xp), "not a device handle"),
            ("trsv: a handle that is not live", lambda: trsv(P(dead.dm.handle), LOWER, STORED, 1, bp, xp), "not a device handle"),
            ("trsv: an ELL handle", lambda: trsv(P(ell.handle), LOWER, STORED, 1, bp, xp), "ELL"),
            ("trsv: a hierarchy", lambda: trsv(P(hier.handle), LOWER, STORED, 1, bp, xp), "multigrid hierarchy"),
            ("trsv: not square", lambda: trsv(P(wide.handle), LOWER, UNIT, 1, bp, xp), "not square"),
            ("trsv: dB is NULL", lambda: trsv(h, LOWER, STORED, 1, None, xp), "dB is NULL"),
            ("trsv: dX is NULL", lambda: trsv(h, LOWER, STORED, 1, bp, None), "dX is NULL"),
            ("trsv: unknown uplo", lambda: trsv(h, 2, STORED, 1, bp, xp), "unknown uplo 2"),
            ("trsv: unknown diag", lambda: trsv(h, LOWER, 7, 1, bp, xp), "unknown diag 7"),
            ("trsv: 4097 sweeps", lambda: trsv(h, LOWER, STORED, 4097, bp, xp), "4097 sweeps are above 4096"),
            ("trsv: an overlap", lambda: trsv(h, LOWER, STORED, 1, bp, shifted), "overlap"),
            ("trsv: STORED without a diagonal", lambda: trsv(P(nodiag.dm.handle), UPPER, STORED, 1, bp, xp), "row 0 does not hold exactly one"),
            ("trsv: STORED with a diagonal twice", lambda: trsv(P(twice.dm.handle), LOWER, STORED, 1, bp, xp), f"row {twice_bad} does not hold exactly one"),
            ("trsm: k = 0", lambda: trsm(h, LOWER, STORED, 1, 0, bp, 4, ROW, xp, 4, ROW), "k = 0"),
            ("trsm: 4097 sweeps", lambda: trsm(h, LOWER, STORED, 4097, 2, bp, 2, ROW, xp, 2, ROW), "4097 sweeps are above 4096"),
            ("trsm: unknown layout", lambda: trsm(h, LOWER, STORED, 1, 2, bp, 2, 5, xp, 2, ROW), "unknown layout 5"),
            ("trsm: ldb too small", lambda: trsm(h, LOWER, STORED, 1, 3, bp, 2, ROW, xp, 3, ROW), "ldb = 2 is below 3"),
            ("trsm: ldx too small", lambda: trsm(h, LOWER, STORED, 1, 3, bp, 3, ROW, xp, M - 1, COL), f"ldx = {M - 1} is below {M}"),
            ("trsm: the same pointer in another layout", lambda: trsm(h, LOWER, STORED, 1, 3, bp, 3, ROW, bp, M, COL), "overlap"),
            ("trsm: k above the prepared width", lambda: trsm(h, LOWER, STORED, 1, 5, bp, 5, ROW, xp, 5, ROW), "prepared for 4"),
            ("trsm: an ELL handle", lambda: trsm(P(ell.handle), LOWER, STORED, 1, 2, bp, 2, ROW, xp, 2, ROW), "ELL"),
            ("set: unknown mode", lambda: lib.spmvHipTriSetApply(h, 2, 1, 1, 0), "unknown mode 2"),
            ("set: 4097 lower sweeps", lambda: lib.spmvHipTriSetApply(h, 1, 4097, 1, 0), "above 4096"),
            ("set: 4097 upper sweeps", lambda: lib.spmvHipTriSetApply(h, 1, 1, 4097, 0), "above 4096"),
            ("set: dA is NULL", lambda: lib.spmvHipTriSetApply(None, 1, 1, 1, 0), "not a device handle"),
            ("set: an ELL handle", lambda: lib.spmvHipTriSetApply(P(ell.handle), 1, 1, 1, 0), "ELL"),
            ("set: a hierarchy", lambda: lib.spmvHipTriSetApply(P(hier.handle), 1, 1, 1, 0), "multigrid hierarchy"),
            ("set: an approximate-inverse factor", lambda: lib.spmvHipTriSetApply(P(g.handle), 1, 1, 1, 0), "approximate-inverse"),
            ("prepare: a hierarchy", lambda: lib.spmvHipTriSweepsPrepare(P(hier.handle), 2), "multigrid hierarchy"),
            ("prepare: not square", lambda: lib.spmvHipTriSweepsPrepare(P(wide.handle), 2), "not square"),
            ("info: info is NULL", lambda: lib.spmvHipTriSweepsInfo(h, None), "info is NULL"),
            ("info: a handle that is not live", lambda: lib.spmvHipTriSweepsInfo(P(dead.dm.handle), P(info)), "not a device handle"),
        ]
        for what, call, says in cases:
            dx.poison()
            capfd.readouterr()
            assert call() == 1, what
            err = capfd.readouterr().err
            assert "libspmvhip" in err and says in err, (what, err)
            assert _poisoned(api, dx), what + ": the output was written"
            assert _plan(src.dm) == plan, what + ": the handle's plan changed"
        for other in (nodiag, twice):
            assert other.dm.triangular_info(True).levels == 0, "a refused sweep solve analysed no level sets"
        # a Krylov solve with a dM in SWEEPS mode: a bad diagonal names the row; a block wider than the workspace is refused
        twice.dm.set_triangular_apply(2)
        A = Source(api, 100, 100, *random_square(rng, 100, 4))
        try:
            opts, kinfo = api.spmvKrylovOpts(1e-8, 10, None), api.spmvKrylovInfo()
            for fn in (lib.hipSpCGCSR, lib.hipSpBiCGStabCSR):
                dx.poison()
                capfd.readouterr()
                assert fn(P(A.dm.handle), P(twice.dm.handle), bp, xp, P(opts), P(kinfo)) == 1
                assert f"row {twice_bad} of dM" in capfd.readouterr().err and _poisoned(api, dx)
            gopts = api.spmvGmresOpts(1e-8, 10, 5, None)
            dx.poison()
            assert lib.hipSpGMRESCSR(P(A.dm.handle), P(twice.dm.handle), bp, xp, P(gopts), P(kinfo)) == 1
            assert f"row {twice_bad} of dM" in capfd.readouterr().err and _poisoned(api, dx)
            A.dm.set_triangular_apply(2, block_width=2)
            for fn in (lib.hipSpCGBlockCSR, lib.hipSpBiCGStabBlockCSR):
                dx.poison()
                capfd.readouterr()
                assert fn(P(A.dm.handle), P(A.dm.handle), 3, bp, 3, ROW, xp, 3, ROW, P(opts), None, P(kinfo)) == 1
                err = capfd.readouterr().err
                assert "workspace of width 2, k = 3" in err and _poisoned(api, dx), err
        finally:
            A.free()
        _no_sticky_error(api)
        # and the handle still solves, by sweeps and exactly
        same(src.dm.solve_triangular(b, lower=True, sweeps=2), sweeps_numpy(M, IRP, JA, AS, b, 2, True, False), "sweeps after the refusals")
        same(src.dm.solve_triangular(b, lower=True), trsv_levels(M, IRP, JA, AS, b, True, False), "the exact solve after the refusals")
    finally:
        for x in (db, dx, g, hier, ell, wide):
            x.free()
        for s in (src, nodiag, twice, lap):
            s.free()


# ------------------------------------------------------------------------------------------------- refused allocations
def _sweep(api, dm, M, call, allocations, before, check_after, what, capfd):
    """`call` with allocation n refused, alone and from then on, for every n below `allocations`"""
    live = int(api.alloc_stats().live)
    for n in range(allocations):
        for from_then_on in (False, True):
            tag = f"{what}, allocation {n}{' on' if from_then_on else ''}"
            capfd.readouterr()
            api.alloc_refuse(n, from_then_on)
            rc = call()
            st = api.alloc_stats()
            api.alloc_refuse(-1)
            assert rc == 1 and st.refused >= 1, tag
            assert "libspmvhip" in capfd.readouterr().err, tag
            assert int(st.live) == live and int(st.badFrees) == 0, tag + ": something was left behind or released twice"
            assert _plan(dm) == before, tag + ": the handle has neither no plan nor the complete one it had"
            _no_sticky_error(api)
            check_after(tag)


def test_every_allocation_of_prepare_refused_in_turn(api, capfd):
    lib, P = api.lib, C.byref
    M, IRP, JA, AS, b = sweeps_inputs.make("span_edge")
    ref2 = sweeps_numpy(M, IRP, JA, AS, b, 2, True, False)
    exact = trsv_levels(M, IRP, JA, AS, b, True, False)
    src = Source(api, M, M, IRP, JA, AS)
    db, dx = api.DeviceVector(M).up(b), api.DeviceVector(M)
    try:
        same(src.dm.solve_triangular(b, lower=True), exact, "the exact solve, analysed before")

        def exact_still_works(tag):
            same(src.dm.solve_triangular(b, lower=True), exact, tag + ": the exact solve afterwards")

        # how many allocations a first build and a widening ask for, on a twin
        twin = Source(api, M, M, IRP, JA, AS)
        try:
            api.alloc_refuse(-1)
            twin.dm.prepare_triangular_sweeps(2)
            n_build = int(api.alloc_stats().calls)
            api.alloc_refuse(-1)
            twin.dm.prepare_triangular_sweeps(9)
            n_widen = int(api.alloc_stats().calls)
        finally:
            twin.free()
        assert (n_build, n_widen) == (3, 1), "diagPos, the iterates and the flag word; the wider iterates"

        none = _plan(src.dm)
        assert none[3] == 0 and none[-1] is None, "no plan yet"
        # 1. the first build, through Prepare, SetApply and the first solve
        _sweep(api, src.dm, M, lambda: lib.spmvHipTriSweepsPrepare(P(src.dm.handle), 2), n_build, none, exact_still_works, "Prepare", capfd)
        _sweep(api, src.dm, M, lambda: lib.spmvHipTriSetApply(P(src.dm.handle), 1, 2, 2, 2), n_build, none, exact_still_works, "SetApply", capfd)

        def first_solve():
            dx.poison()
            rc = lib.hipSpTRSVSweepsCSR(P(src.dm.handle), LOWER, STORED, 2, db.ptr, dx.ptr)
            assert rc == 0 or _poisoned(api, dx), "a refused solve wrote x"
            return rc
        _sweep(api, src.dm, M, first_solve, n_build, none, exact_still_works, "the first solve", capfd)
        assert first_solve() == 0, "the same call, unarmed"
        same(dx.down(), ref2, "the first solve, unarmed")
        built = _plan(src.dm)
        assert built[3] == 1 and built[8] == 1
        # 2. the widening: the complete narrow plan stays, and still solves
        def narrow_still_works(tag):
            exact_still_works(tag)
            same(src.dm.solve_triangular(b, lower=True, sweeps=2), ref2, tag + ": the narrow plan afterwards")
        _sweep(api, src.dm, M, lambda: lib.spmvHipTriSweepsPrepare(P(src.dm.handle), 9), n_widen, _plan(src.dm), narrow_still_works, "widening", capfd)
        assert lib.spmvHipTriSweepsPrepare(P(src.dm.handle), 9) == 0
        wide = src.dm.triangular_sweeps_info()
        assert (wide.width, wide.prepares, wide.diagPos) == (9, 2, built[-2])
        narrow_still_works("after the widening")
    finally:
        db.free()
        dx.free()
        src.free()
