"""Triangular solves by Jacobi sweeps on the device (hipSpTRSVSweepsCSR, spmvHipTriSweepsPrepare, spmvHipTriSweepsInfo;
DeviceMatrix.solve_triangular(sweeps=S)): every case equals the test side's loop (tests/sweeps_ref.py) in all bits -- finite
rows by bits, infinities by sign, NaN as NaN -- on the matrices of tests/sweeps_inputs.py, both triangles, both diagonals,
S in {0, 1, 2, 3, levels - 1, levels + 1}, out of place and in place; device against device at S = levels - 1; values
read live; no allocation once prepared."""
import ctypes as C

import numpy as np
import pytest

import sweeps_inputs
from ilu0_ref import ilu0_levels
from sweeps_ref import sweeps_numpy
from test_gpu_trsv import LOWER, STORED, UNIT, UPPER, Source, same
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
    api.lib.spmvHipSetUnitValues(1)
    api.lib.spmvHipSetSync(1)
    api.alloc_refuse(-1)


def sweep_raw(api, dm, uplo, diag, S, b, in_place):
    """the C call on device vectors, x poisoned first unless it is b: (return code, x)"""
    n = max(b.size, 1)
    db = api.DeviceVector(n).up(np.resize(b, n) if b.size else np.zeros(1))
    dx = db if in_place else api.DeviceVector(n)
    try:
        if not in_place:
            dx.poison()
        rc = api.lib.hipSpTRSVSweepsCSR(C.byref(dm.handle), uplo, diag, S, db.ptr, dx.ptr)
        return rc, dx.down()[:b.size]
    finally:
        db.free()
        if not in_place:
            dx.free()


def check_all(api, dm, M, IRP, JA, AS, b, name, exact=True):
    """every (uplo, diag, S, placement) of one matrix against the reference; at S = levels - 1 against hipSpTRSVCSR too"""
    for lower in (True, False):
        counts, L = sweeps_inputs.sweep_counts(M, IRP, JA, lower)
        for unit in (False, True):
            for S in counts:
                ref = sweeps_numpy(M, IRP, JA, AS, b, S, lower, unit)
                for in_place in (False, True):
                    what = f"{name}, lower {lower}, unit {unit}, S = {S}, in place {in_place}"
                    rc, x = sweep_raw(api, dm, LOWER if lower else UPPER, UNIT if unit else STORED, S, b, in_place)
                    assert rc == 0, what
                    same(x, ref, what)
                if exact and S == max(L - 1, 0):
                    x_exact = dm.solve_triangular(b, lower=lower, unit_diagonal=unit)
                    assert dm.triangular_info(lower).levels == L
                    same(dm.solve_triangular(b, lower=lower, unit_diagonal=unit, sweeps=S), x_exact, f"{name}: device against device")


# ------------------------------------------------------------------------------------------------- 1. matrices
@pytest.mark.parametrize("name", sweeps_inputs.NAMES)
def test_matrix(api, name):
    M, IRP, JA, AS, b = sweeps_inputs.make(name)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        if name == "pattern":
            v = C.c_double()
            assert api.lib.spmvHipUnitValue(C.byref(src.dm.handle), C.byref(v)) == 1 and v.value == 0.5, "a unit-value handle"
        check_all(api, src.dm, M, IRP, JA, AS, b, name)
        info = src.dm.triangular_sweeps_info()
        assert (info.prepares, info.width, info.firstBadDiag, info.mode) == (1, 1, -1, 0)
        assert info.bytes == 4 * M + 16 * M
    finally:
        src.free()


@pytest.mark.parametrize("adopt", [4, 8])
def test_adopted_handles_with_both_row_pointer_widths(api, adopt):
    M, IRP, JA, AS, b = sweeps_inputs.make("span_edge")
    src = Source(api, M, M, IRP, JA, AS, adopt)
    try:
        check_all(api, src.dm, M, IRP, JA, AS, b, f"adopted {adopt}", exact=False)
    finally:
        src.free()


def test_pattern_handle_with_unit_values_off(api):
    """the same pattern matrix with the value stream read: the same bits"""
    api.lib.spmvHipSetUnitValues(0)
    M, IRP, JA, AS, b = sweeps_inputs.make("pattern")
    src = Source(api, M, M, IRP, JA, AS)
    try:
        check_all(api, src.dm, M, IRP, JA, AS, b, "pattern, values streamed", exact=False)
    finally:
        src.free()


def test_m0_and_launch_counts(api):
    src = Source(api, 0, 0, np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    try:
        dv = api.DeviceVector(1)
        dv.poison()
        for S in (0, 3):
            assert api.lib.hipSpTRSVSweepsCSR(C.byref(src.dm.handle), LOWER, STORED, S, dv.ptr, dv.ptr) == 0
        assert dv.down().view(np.uint64)[0] == api.POISON_NAN, "M = 0 writes nothing"
        assert api.lib.spmvHipLastKernelSeconds() == 0.0
        dv.free()
    finally:
        src.free()
    # launches of one solve: S (UNIT; S + 1 for S == 1 in place; S == 0: one copy, none in place), S + 1 (STORED)
    M, IRP, JA, AS, b = sweeps_inputs.make("r65")
    src = Source(api, M, M, IRP, JA, AS)
    try:
        for diag, S, in_place, want in ((UNIT, 0, False, 1), (UNIT, 0, True, 0), (UNIT, 1, False, 1), (UNIT, 1, True, 2), (UNIT, 4, True, 4),
                                        (UNIT, 4, False, 4), (STORED, 0, True, 1), (STORED, 1, True, 2), (STORED, 5, False, 6)):
            rc, _ = sweep_raw(api, src.dm, LOWER, diag, S, b, in_place)
            assert rc == 0 and src.dm.triangular_sweeps_info().solveLaunches == want, (diag, S, in_place)
        g, bl = api.spmvDim3(), api.spmvDim3()
        api.lib.spmvHipLastLaunch(C.byref(g), C.byref(bl))
        assert (bl.x, bl.y, bl.z) == (256, 1, 1) and g.x >= 1
        assert api.lib.spmvHipLastKernelSeconds() > 0.0
        assert src.dm.triangular_info(True).levels == 0, "a sweep solve builds no level sets"
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 2. values are live
def _addresses(api, dm):
    info = dm.triangular_sweeps_info()
    return (info.prepares, info.width, info.bytes, info.firstBadDiag, info.sorted, info.diagPos, info.workspace)


def test_values_are_read_live_after_ilu0_and_an_update(api):
    nx, ny, nz = 6, 5, 4
    IRP, JA, AS = laplacian7(nx, ny, nz)
    M = nx * ny * nz
    rng = np.random.default_rng(4100)
    b = rng.standard_normal(M)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        src.dm.prepare_triangular_sweeps()
        before = _addresses(api, src.dm)
        assert before[0] == 1 and before[4] == 1, "sorted rows with one diagonal: the ILU(0) precondition"
        same(src.dm.solve_triangular(b, lower=True, unit_diagonal=True, sweeps=2), sweeps_numpy(M, IRP, JA, AS, b, 2, True, True), "before")
        src.dm.ilu0()
        F = ilu0_levels(M, IRP, JA, AS)
        for lower, unit in ((True, True), (False, False)):
            same(src.dm.solve_triangular(b, lower=lower, unit_diagonal=unit, sweeps=3), sweeps_numpy(M, IRP, JA, F, b, 3, lower, unit),
                 "after hipSpILU0CSR")
        AS2 = np.where(AS == 6.0, 7.0 + rng.random(AS.size), -1.0 - rng.random(AS.size) / 8)
        src.dm.update_values(AS2)
        same(src.dm.solve_triangular(b, lower=False, unit_diagonal=False, sweeps=3), sweeps_numpy(M, IRP, JA, AS2, b, 3, False, False),
             "after spmvHipUpdateValues")
        src.dm.ilu0()
        F2 = ilu0_levels(M, IRP, JA, AS2)
        same(src.dm.solve_triangular(b, lower=False, unit_diagonal=False, sweeps=1), sweeps_numpy(M, IRP, JA, F2, b, 1, False, False),
             "after a re-factorisation")
        assert _addresses(api, src.dm) == before, "the plan was rebuilt"
    finally:
        src.free()


def test_a_prepared_solve_allocates_nothing(api):
    M, IRP, JA, AS, b = sweeps_inputs.make("span_edge")
    start = api.alloc_stats().live
    src = Source(api, M, M, IRP, JA, AS)
    db, dx = api.DeviceVector(M).up(b), api.DeviceVector(M)
    try:
        live0 = api.alloc_stats().live
        src.dm.prepare_triangular_sweeps()
        assert api.alloc_stats().live == live0 + 2, "the plan holds diagPos and the two iterates (one allocation)"
        api.alloc_refuse(-1)                                   # (calls and refused start at 0)
        for uplo, diag, S in ((LOWER, UNIT, 3), (UPPER, STORED, 2), (LOWER, STORED, 0)):
            assert api.lib.hipSpTRSVSweepsCSR(C.byref(src.dm.handle), uplo, diag, S, db.ptr, dx.ptr) == 0
        st = api.alloc_stats()
        assert (st.calls, st.live) == (0, live0 + 2), "a solve on a prepared handle allocated"
        src.dm.prepare_triangular_sweeps()                     # a no-op
        src.dm.prepare_triangular_sweeps(1)
        assert api.alloc_stats().calls == 0 and src.dm.triangular_sweeps_info().prepares == 1
    finally:
        db.free()
        dx.free()
        src.free()
    assert api.alloc_stats().live == start, "hipFreeSpmat frees the plan"


def test_enqueue_only_with_sync_off(api):
    """spmvHipSetSync(0): the call only enqueues; the result is there after the stream is drained"""
    M, IRP, JA, AS, b = sweeps_inputs.make("r64")
    src = Source(api, M, M, IRP, JA, AS)
    db, dx = api.DeviceVector(M).up(b), api.DeviceVector(M)
    try:
        src.dm.prepare_triangular_sweeps()
        api.lib.spmvHipSetSync(0)
        assert api.lib.hipSpTRSVSweepsCSR(C.byref(src.dm.handle), LOWER, STORED, 3, db.ptr, dx.ptr) == 0
        api.lib.spmvHipSetSync(1)
        same(dx.down(), sweeps_numpy(M, IRP, JA, AS, b, 3, True, False), "enqueue only")   # (the download drains the stream)
    finally:
        db.free()
        dx.free()
        src.free()
