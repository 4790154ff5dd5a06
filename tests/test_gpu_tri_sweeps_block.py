"""Block sweep solves on the device (hipSpTRSMSweepsCSR; DeviceMatrix.solve_triangular_block(sweeps=S)): every column has the
bits of the single sweep solve (tests/sweeps_ref.py), k in {1, 3, 16, 17, 33}, both layouts mixed between B and X, padded
leading dimensions whose sentinels survive, in place, a NaN column that stays alone, and a launch count that does not depend
on k."""
import ctypes as C
import functools

import numpy as np
import pytest

import sweeps_inputs
from bits import assert_same_bits
from sweeps_ref import sweeps_block
from test_gpu_trsm import ROW, SENTINEL, Block, layouts_of
from test_gpu_trsv import LOWER, STORED, Source, same
from test_trsm_abi import block_of_columns
from test_trsv_abi import random_square

pytestmark = pytest.mark.gpu
WIDTHS = (1, 3, 16, 17, 33)
SWEEPS = (0, 1, 3)


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@functools.lru_cache(maxsize=None)
def m300():
    """M = 300, unsorted rows with repeats, the whole matrix; 33 order-sensitive columns of B"""
    rng = np.random.default_rng(4200)
    M = 300
    IRP, JA, AS = random_square(rng, M, 9)
    B = block_of_columns(rng, M, 33)
    B.setflags(write=False)
    return M, IRP, JA, AS, B


@functools.lru_cache(maxsize=None)
def m300_ref(lower, unit, S):
    """columns are independent: the first k columns of the 33-column reference are the k-column solve"""
    M, IRP, JA, AS, B = m300()
    X = sweeps_block(M, IRP, JA, AS, B, S, lower, unit)
    X.setflags(write=False)
    return X


@pytest.fixture(scope="module")
def h300(api):
    M, IRP, JA, AS, _ = m300()
    src = Source(api, M, M, IRP, JA, AS)
    src.dm.prepare_triangular_sweeps(33)
    yield src.dm
    src.free()


def solve(torch, dm, Bh, lower, unit, S, bl, xl, what, in_place=False):
    """through the Python layer: B and X in the named layouts, X from sentinels (or B itself); X's block, its padding checked"""
    M, k = Bh.shape
    lay = layouts_of(M, k)
    B = Block(torch, M, k, *lay[bl], host=Bh)
    X = B if in_place else Block(torch, M, k, *lay[xl])
    out = dm.solve_triangular_block(B.view, lower=lower, unit_diagonal=unit, out=X.view, sweeps=S)
    assert out.data_ptr() == X.view.data_ptr()
    X.padding_intact(what)
    if not in_place:
        B.padding_intact(what + " (B)")
        assert_same_bits(B.down(), Bh, what + ": B is read only")
    return X.down()


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("unit", [False, True])
def test_widths_layouts_and_in_place(api, torch, h300, lower, unit):
    M, _, _, _, B = m300()
    for S in SWEEPS:
        ref = m300_ref(lower, unit, S)
        for k in WIDTHS:
            pairs = [("row", "row"), ("row+3", "col+5"), ("col", "row+3"), ("col+5", "col")] if k in (3, 17) else [("row", "col"), ("col+5", "row+3")]
            for bl, xl in pairs:
                what = f"lower {lower}, unit {unit}, S = {S}, k = {k}, B {bl}, X {xl}"
                same(solve(torch, h300, B[:, :k], lower, unit, S, bl, xl, what), ref[:, :k], what)
            for lay in ("row+3", "col+5"):
                what = f"lower {lower}, unit {unit}, S = {S}, k = {k}, in place {lay}"
                same(solve(torch, h300, B[:, :k], lower, unit, S, lay, lay, what, in_place=True), ref[:, :k], what)
    info = h300.triangular_sweeps_info()
    assert (info.width, info.prepares) == (33, 1)


@pytest.mark.parametrize("name", ["span_edge", "short_rows", "long_rows", "pattern", "bad_diagonals"])
def test_every_kernel_path_by_column(api, torch, name):
    """the matrices of the single solve with 5 columns (a panel of 8 lanes with 3 idle) and 17 (two panels): several spans,
    two rows per group, a row longer than the span in each triangle, a unit-value handle, 0 / NaN / Inf diagonals"""
    M, IRP, JA, AS, b = sweeps_inputs.make(name)
    rng = np.random.default_rng(4300)
    Bh = np.stack([b] + [b * 2.0 ** (c - 8) for c in range(1, 17)], axis=1)
    Bh[:, 3] = rng.standard_normal(M)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        for lower, unit, S in ((True, True, 2), (False, False, 3), (True, False, 1)):
            ref = sweeps_block(M, IRP, JA, AS, Bh, S, lower, unit)
            for k, bl, xl in ((5, "row+3", "col"), (17, "col+5", "row")):
                what = f"{name}, lower {lower}, unit {unit}, S = {S}, k = {k}"
                same(solve(torch, src.dm, Bh[:, :k], lower, unit, S, bl, xl, what), ref[:, :k], what)
                if src.dm.triangular_sweeps_info().prepares == 1:
                    assert src.dm.triangular_sweeps_info().width == 5, "the first sweep solve prepared the handle for its own width"
                    src.dm.prepare_triangular_sweeps(17)
        assert src.dm.triangular_sweeps_info().width == 17
    finally:
        src.free()


def test_widening_keeps_the_plan_and_a_wider_solve_is_refused_before(api, torch, capfd):
    M, IRP, JA, AS, B = m300()
    src = Source(api, M, M, IRP, JA, AS)
    try:
        src.dm.prepare_triangular_sweeps(3)
        first = src.dm.triangular_sweeps_info()
        lay = layouts_of(M, 16)
        Bd, X = Block(torch, M, 16, *lay["row"], host=B[:, :16]), Block(torch, M, 16, *lay["row"])
        capfd.readouterr()
        rc = api.lib.hipSpTRSMSweepsCSR(C.byref(src.dm.handle), LOWER, STORED, 2, 16, C.c_void_p(Bd.ptr), 16, ROW, C.c_void_p(X.ptr), 16, ROW)
        assert rc != 0 and "prepared for 3" in capfd.readouterr().err
        assert (X.flat.cpu().numpy().view(np.uint64) == SENTINEL).all(), "a refused solve wrote X"
        src.dm.prepare_triangular_sweeps(16)
        wide = src.dm.triangular_sweeps_info()
        assert (wide.width, wide.prepares, wide.diagPos) == (16, 2, first.diagPos) and wide.bytes == 4 * M + 16 * 16 * M
        same(src.dm.solve_triangular_block(B[:, :16].copy(), lower=True, sweeps=2), m300_ref(True, False, 2)[:, :16], "after widening")
    finally:
        src.free()


def test_a_nan_column_stays_alone(api, torch, h300):
    M, IRP, JA, AS, B = m300()
    Bh = B[:, :17].copy()
    Bh[:, 8] = np.nan
    Bh[5, 16] = np.inf
    ref = sweeps_block(M, IRP, JA, AS, Bh, 3, True, False)
    X = solve(torch, h300, Bh, True, False, 3, "row", "row+3", "NaN column")
    same(X, ref, "NaN column")
    assert np.isnan(X[:, 8]).all() and np.isfinite(X[:, [7, 9]]).all()


def test_launch_count_does_not_depend_on_k(api, torch, h300):
    M, _, _, _, B = m300()
    for S, unit, want in ((3, True, 3), (3, False, 4), (0, False, 1)):
        seen = set()
        for k in WIDTHS:
            solve(torch, h300, B[:, :k], True, unit, S, "row+3", "col+5", f"k = {k}")
            seen.add(h300.triangular_sweeps_info().solveLaunches)
        assert seen == {want}, (S, unit, seen)
    g, bl = api.spmvDim3(), api.spmvDim3()
    api.lib.spmvHipLastLaunch(C.byref(g), C.byref(bl))
    assert (bl.x, bl.y, bl.z) == (256, 1, 1)
