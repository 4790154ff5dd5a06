"""Block triangular solves on the device (hipSpTRSMCSR; DeviceMatrix.solve_triangular_block): every column of every case
equals the test side's reference (tests/trsm_ref.py, column by column the serial loop of tests/trsv_ref.py) in all bits --
finite values by bits, infinities by sign, NaN as NaN.  The columns of B are distinct order-sensitive vectors
(serial_order_inputs.order_values), so a swapped or shared column shows; X starts as a sentinel bit pattern, padding
included, and the padding is checked afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits
from test_gpu_trsv import Source, same
from test_ilu0_abi import random_ilu
from test_trsm_abi import block_of_columns
from test_trsv_abi import laplacian7, random_square
from transpose_ref import stable_transpose
from trsm_ref import trsm_levels
from trsv_ref import diag_pos

pytestmark = pytest.mark.gpu

LOWER, UPPER, STORED, UNIT = 0, 1, 0, 1
ROW, COL = 0, 1
SENTINEL = 0x7FF4DEADBEEF0001


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
    api.lib.spmvHipSetUnitValues(1)
    api.lib.spmvHipSetStream(None)
    api.lib.spmvHipSetSync(1)
    api.lib.spmvHipSetVariant(b"hipSpTRSVCSR", 256)


# ------------------------------------------------------------------------------------------------- blocks on the device
class Block:
    """an (M, k) block inside a flat device tensor of sentinels, at element offset `off`: row-major (i, c) at
    off + i*ld + c, column-major at off + c*ld + i.  `view` is the strided torch view the Python layer takes."""

    def __init__(self, torch, M, k, layout, ld, off=0, host=None):
        self.M, self.k, self.layout, self.ld, self.off = M, k, layout, ld, off
        n = off + (M * ld if layout == ROW else k * ld) + 1
        flat = np.full(n, SENTINEL, dtype=np.uint64).view(np.float64)
        self.index = (off + np.arange(M)[:, None] * ld + np.arange(k)[None, :]) if layout == ROW else \
                     (off + np.arange(k)[None, :] * ld + np.arange(M)[:, None])
        if host is not None:
            flat[self.index] = host
        self.flat = torch.from_numpy(flat).cuda()
        self.view = self.flat.as_strided((M, k), (ld, 1) if layout == ROW else (1, ld), off)

    @property
    def ptr(self):
        return self.flat.data_ptr() + 8 * self.off

    def down(self):
        return self.flat.cpu().numpy()[self.index]

    def padding_intact(self, what):
        host = self.flat.cpu().numpy().view(np.uint64)
        outside = np.ones(host.size, bool)
        outside[self.index] = False
        assert (host[outside] == SENTINEL).all(), what + ": an element outside the block was written"


def layouts_of(M, k):
    return {"row": (ROW, k), "row+3": (ROW, k + 3), "col": (COL, M), "col+5": (COL, M + 5)}


def solve(api, torch, dm, Bh, lower, unit, bl="row", xl="row", what="", off=0):
    """through the Python layer: B and X in the named layouts, X from sentinels; returns X's block after checking its padding
    and that B was only read"""
    M, k = Bh.shape
    lay = layouts_of(M, k)
    B = Block(torch, M, k, *lay[bl], off=off, host=Bh)
    X = Block(torch, M, k, *lay[xl], off=off)
    out = dm.solve_triangular_block(B.view, lower=lower, unit_diagonal=unit, out=X.view)
    assert out.data_ptr() == X.view.data_ptr()
    X.padding_intact(what)
    B.padding_intact(what + " (B)")
    assert_same_bits(B.down(), Bh, what + ": B is read only")
    return X.down()


def raw(api, dm, uplo, diag, k, b_ptr, ldb, bl, x_ptr, ldx, xl):
    return api.lib.hipSpTRSMCSR(C.byref(dm.handle), uplo, diag, k, C.c_void_p(b_ptr), ldb, bl, C.c_void_p(x_ptr), ldx, xl)


# ------------------------------------------------------------------------------------------------- shared inputs
@functools.lru_cache(maxsize=None)
def m300():
    """M = 300, unsorted rows with repeats, the whole matrix; 33 columns of B; the reference of every (lower, unit)"""
    rng = np.random.default_rng(2601)
    M = 300
    IRP, JA, AS = random_square(rng, M, 9)
    B = block_of_columns(rng, M, 33)
    B.setflags(write=False)
    return M, IRP, JA, AS, B


@functools.lru_cache(maxsize=None)
def m300_ref(lower, unit):
    M, IRP, JA, AS, B = m300()
    X = trsm_levels(M, IRP, JA, AS, B, lower, unit)           # columns are independent: the first k columns are the k-column solve
    X.setflags(write=False)
    return X


@pytest.fixture(scope="module")
def h300(api):
    M, IRP, JA, AS, _ = m300()
    src = Source(api, M, M, IRP, JA, AS)
    yield src.dm
    src.free()


# ------------------------------------------------------------------------------------------------- 1. widths and layouts
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("unit", [False, True])
def test_widths_and_layouts(api, torch, h300, lower, unit):
    M, _, _, _, B = m300()
    ref = m300_ref(lower, unit)
    for k in (1, 2, 3, 8, 15, 16, 17, 33):
        names = list(layouts_of(M, k)) if k in (3, 17) else ["row"]
        for bl in names:
            for xl in names:
                what = f"lower {lower}, unit {unit}, k {k}, B {bl}, X {xl}"
                same(solve(api, torch, h300, B[:, :k], lower, unit, bl, xl, what), ref[:, :k], what)
    info = h300.triangular_info(lower)
    assert info.analyses == 1


# ------------------------------------------------------------------------------------------------- 2. both kernel paths
def _runs_and_levels(info):
    """(launches that are runs, launches that are single levels) from spmvTriInfo"""
    singles = info.levels - info.fusedLevels
    return info.launches - singles, singles


def test_wide_levels_and_fused_runs(api, torch):
    """a matrix whose first levels exceed T = 256 rows (the level kernel, several workgroups) and whose tail fuses (the run
    kernel)"""
    rng = np.random.default_rng(2602)
    M = 6000
    IRP, JA, AS = random_square(rng, M, 3, shuffle=False)
    rows = si.row_of_entry(IRP)
    keep = JA.astype(np.int64) <= rows                                   # sorted lower triangle
    IRP, JA, AS = si.assemble(M, rows[keep], JA[keep].astype(np.int64), AS[keep])
    B = block_of_columns(rng, M, 17)
    ref = trsm_levels(M, IRP, JA, AS, B, True, False)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        for k in (3, 16, 17):
            same(solve(api, torch, src.dm, B[:, :k], True, False, what=f"wide + fused, k {k}"), ref[:, :k], f"wide + fused, k {k}")
        info = src.dm.triangular_info(True)
        runs, singles = _runs_and_levels(info)
        assert info.fusedLevels > 0 and runs > 0 and info.launches > runs and info.maxLevelRows > 256
    finally:
        src.free()


@pytest.mark.parametrize("T", [256, 0])
def test_thin_laplacian_in_runs_and_in_levels(api, torch, T):
    """960 rows in 28 thin levels: one run (T = 256), or every level through the level kernel (T = 0)"""
    try:
        api.set_variant("hipSpTRSVCSR", T)
        nx, ny, nz = 12, 10, 8
        IRP, JA, AS = laplacian7(nx, ny, nz)
        M = nx * ny * nz
        rng = np.random.default_rng(2603)
        AS = np.where(AS == 6.0, 6.0 + rng.random(AS.size), si.order_values(rng, AS.size, 1) / 7)
        B = block_of_columns(rng, M, 17)
        src = Source(api, M, M, IRP, JA, AS)                              # a fresh handle: T holds for later analyses
        try:
            for lower in (True, False):
                ref = trsm_levels(M, IRP, JA, AS, B, lower, False)
                for k in (3, 16, 17):
                    what = f"laplacian, T {T}, lower {lower}, k {k}"
                    same(solve(api, torch, src.dm, B[:, :k], lower, False, what=what), ref[:, :k], what)
                info = src.dm.triangular_info(lower)
                assert info.levels == nx + ny + nz - 2 == 28
                assert (info.fusedLevels, info.launches) == ((28, 1) if T else (0, 28))
        finally:
            src.free()
    finally:
        api.set_variant("hipSpTRSVCSR", 256)


# ------------------------------------------------------------------------------------------------- 3. chain
@pytest.mark.parametrize("T", [256, 0])
def test_chain_of_3000(api, torch, T):
    """a subdiagonal chain: 3 000 levels of one row -- one fused run (T = 256), or a launch per level (T = 0)"""
    try:
        api.set_variant("hipSpTRSVCSR", T)
        rng = np.random.default_rng(2604)
        M = 3000
        i = np.arange(M)
        rows, cols = np.concatenate([i, i[1:]]), np.concatenate([i, i[1:] - 1])
        vals = np.where(rows == cols, 1.0 + rng.random(rows.size), rng.uniform(-1, 1, rows.size))
        IRP, JA, AS = si.assemble(M, rows, cols, vals)
        B = block_of_columns(rng, M, 17)
        ref = trsm_levels(M, IRP, JA, AS, B, True, False)
        src = Source(api, M, M, IRP, JA, AS)
        try:
            for k in (16, 17):
                same(solve(api, torch, src.dm, B[:, :k], True, False, what=f"chain, T {T}, k {k}"), ref[:, :k], f"chain, T {T}, k {k}")
            info = src.dm.triangular_info(True)
            assert info.levels == M and (info.fusedLevels, info.launches) == ((M, 1) if T else (0, M))
        finally:
            src.free()
    finally:
        api.set_variant("hipSpTRSVCSR", 256)


# ------------------------------------------------------------------------------------------------- 4. long rows
def long_rows_matrix(rng):
    """level 0: 200 rows without a lower entry; level 1: 200 rows into them, short ones and three of 65, 130 and 200
    strict-triangle entries (with repeats, unsorted), the diagonal and some upper entries in between"""
    M, h = 400, 200
    rows, cols = [np.arange(M)], [np.arange(M)]
    lens = rng.integers(0, 9, h)
    lens[[7, 90, 199]] = [65, 130, 200]
    r = np.repeat(np.arange(h, M), lens)
    rows.append(r)
    cols.append(rng.integers(0, h, r.size))
    up = rng.integers(h, M - 1, 150)                                     # upper entries of the second half: skipped by a lower solve
    rows.append(up)
    cols.append(rng.integers(up + 1, M))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = np.where(rows == cols, 2.0 + rng.random(rows.size), si.order_values(rng, rows.size, 2) / 50)
    o = rng.permutation(rows.size)
    return M, si.assemble(M, rows[o], cols[o], vals[o])


@pytest.mark.parametrize("unit", [False, True])
def test_long_rows(api, torch, unit):
    rng = np.random.default_rng(2605)
    M, (IRP, JA, AS) = long_rows_matrix(rng)
    B = block_of_columns(rng, M, 17)
    ref = trsm_levels(M, IRP, JA, AS, B, True, unit)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        for k in (1, 3, 16, 17):
            for xl in ("row+3", "col"):
                what = f"long rows, unit {unit}, k {k}, X {xl}"
                same(solve(api, torch, src.dm, B[:, :k], True, unit, "row", xl, what), ref[:, :k], what)
        info = src.dm.triangular_info(True)
        assert info.longRows == 3 and info.levels == 2
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 5. small shapes
def test_small_shapes(api, torch):
    rng = np.random.default_rng(2606)
    # M = 0: success, nothing written
    src = Source(api, 0, 0, np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    try:
        X = Block(torch, 2, 3, ROW, 3)                                    # some sentinels to point at
        assert raw(api, src.dm, LOWER, STORED, 3, X.ptr, 3, ROW, X.ptr, 3, ROW) == 0
        torch.cuda.synchronize()
        assert (X.flat.cpu().numpy().view(np.uint64) == SENTINEL).all()
        assert src.dm.triangular_info(True).levels == 0
    finally:
        src.free()
    # 1 x 1
    src = Source(api, 1, 1, np.array([0, 1], np.uint64), np.array([0], np.uint64), np.array([3.0]))
    try:
        Bh = np.array([[-7.0, 2.0, 5.0]])
        same(solve(api, torch, src.dm, Bh, True, False, what="1 x 1"), Bh / 3.0, "1 x 1")
        same(solve(api, torch, src.dm, Bh, False, True, what="1 x 1, unit"), Bh, "1 x 1, unit")
    finally:
        src.free()
    # M = 5, and UNIT with no stored diagonal
    for diag, unit in (("one", False), ("none", True)):
        M = 5
        IRP, JA, AS = random_square(rng, M, 3, diag=diag)
        src = Source(api, M, M, IRP, JA, AS)
        try:
            for k in (1, 2, 17):
                Bh = block_of_columns(rng, M, k)
                for lower in (True, False):
                    what = f"M 5, diagonal {diag}, k {k}, lower {lower}"
                    same(solve(api, torch, src.dm, Bh, lower, unit, "col", "row", what),
                         trsm_levels(M, IRP, JA, AS, Bh, lower, unit), what)
        finally:
            src.free()
    M = 300
    IRP, JA, AS = random_square(rng, M, 6, diag="none")
    src = Source(api, M, M, IRP, JA, AS)
    try:
        Bh = block_of_columns(rng, M, 5)
        for lower in (True, False):
            same(solve(api, torch, src.dm, Bh, lower, True, what="no stored diagonal"), trsm_levels(M, IRP, JA, AS, Bh, lower, True),
                 "no stored diagonal")
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 6. special values
def test_zero_diagonals_stay_in_their_column(api, torch):
    """zero stored diagonals at three rows: +-Inf where b - acc is not zero, NaN where it is; a column of zeros gets NaN at
    those rows while its neighbours get infinities, and each propagates down its own column only"""
    M, IRP, JA, AS, B = m300()
    dpos, _ = diag_pos(M, IRP, JA)
    AS = AS.copy()
    AS[dpos[[3, 50, 120]]] = 0.0
    Bh = B[:, :17].copy()
    Bh[:, 4] = 0.0
    src = Source(api, M, M, IRP, JA, AS)
    try:
        for lower in (True, False):
            ref = trsm_levels(M, IRP, JA, AS, Bh, lower, False)
            assert np.isinf(ref).any() and np.isnan(ref[:, 4]).any()
            same(solve(api, torch, src.dm, Bh, lower, False, what=f"zero diagonals, lower {lower}"), ref, f"zero diagonals, lower {lower}")
    finally:
        src.free()


def test_nan_column_and_signed_zero_column(api, torch, h300):
    M, IRP, JA, AS, B = m300()
    Bh = B[:, :17].copy()
    Bh[:, 5] = np.nan
    Bh[:, 16] = np.where(np.arange(M) % 2, -0.0, 0.0)
    others = [c for c in range(17) if c not in (5, 16)]
    for lower in (True, False):
        for xl in ("row", "col"):
            what = f"NaN column, lower {lower}, X {xl}"
            X = solve(api, torch, h300, Bh, lower, False, "row", xl, what)
            same(X, trsm_levels(M, IRP, JA, AS, Bh, lower, False), what)
            assert np.isnan(X[:, 5]).all()
            assert_same_bits(X[:, others], m300_ref(lower, False)[:, others], what + ": the other columns")


@pytest.mark.parametrize("layout", ["row", "row+3", "col", "col+5"])
def test_in_place(api, torch, h300, layout):
    M, _, _, _, B = m300()
    for k in (3, 17):
        for lower, unit in ((True, False), (False, True)):
            blk = Block(torch, M, k, *layouts_of(M, k)[layout], host=B[:, :k])
            out = h300.solve_triangular_block(blk.view, lower=lower, unit_diagonal=unit, out=blk.view)
            assert out.data_ptr() == blk.view.data_ptr()
            same(blk.down(), m300_ref(lower, unit)[:, :k], f"in place, {layout}, k {k}")
            blk.padding_intact(f"in place, {layout}, k {k}")


def test_odd_offsets_and_odd_leading_dimensions(api, torch, h300):
    """B and X that are only 8-byte aligned (element offset 1) with odd leading dimensions, apart and in place"""
    M, _, _, _, B = m300()
    for k in (3, 16, 17):
        ref = m300_ref(True, False)[:, :k]
        for layout, ld in ((ROW, k + 1 + k % 2), (COL, M + 1)):
            assert ld % 2 == 1
            what = f"odd offset, k {k}, layout {layout}, ld {ld}"
            Bb, Xb = Block(torch, M, k, layout, ld, off=1, host=B[:, :k]), Block(torch, M, k, layout, ld, off=1)
            assert Bb.ptr % 16 == 8 and Xb.ptr % 16 == 8
            h300.solve_triangular_block(Bb.view, out=Xb.view)
            same(Xb.down(), ref, what)
            Xb.padding_intact(what)
            h300.solve_triangular_block(Bb.view, out=Bb.view)
            same(Bb.down(), ref, what + ", in place")
            Bb.padding_intact(what + ", in place")


# ------------------------------------------------------------------------------------------------- 7. handles
def test_unit_value_handle(api, torch):
    rng = np.random.default_rng(2607)
    M = 600
    IRP, JA, _ = random_square(rng, M, 8)
    AS = np.full(JA.size, 1.0)
    Bh = block_of_columns(rng, M, 17)
    xs = []
    for unit_values in (1, 0):
        api.lib.spmvHipSetUnitValues(unit_values)
        src = Source(api, M, M, IRP, JA, AS, 4)
        try:
            v = C.c_double(0)
            assert api.lib.spmvHipUnitValue(C.byref(src.dm.handle), C.byref(v)) == unit_values
            for lower, unit in ((True, True), (False, False)):
                what = f"pattern handle, unit values {unit_values}, lower {lower}"
                xs.append(solve(api, torch, src.dm, Bh, lower, unit, what=what))
                same(xs[-1], trsm_levels(M, IRP, JA, AS, Bh, lower, unit), what)
        finally:
            src.free()
    assert_same_bits(xs[0], xs[2], "unit-value lower")
    assert_same_bits(xs[1], xs[3], "unit-value upper")


def test_adopted_handle_with_8_byte_row_pointers(api, torch):
    M, IRP, JA, AS, B = m300()
    src = Source(api, M, M, IRP, JA, AS, 8)
    try:
        for k in (3, 17):
            for lower, unit in ((True, False), (False, True)):
                what = f"adopted (8-byte IRP), k {k}, lower {lower}"
                same(solve(api, torch, src.dm, B[:, :k], lower, unit, "row", "col", what), m300_ref(lower, unit)[:, :k], what)
    finally:
        src.free()


def test_upper_solve_on_a_transpose(api, torch):
    rng = np.random.default_rng(2608)
    M = 600
    IRP, JA, AS = random_square(rng, M, 8)
    rows = si.row_of_entry(IRP)
    keep = JA.astype(np.int64) <= rows
    IRP, JA, AS = si.assemble(M, rows[keep], JA[keep].astype(np.int64), AS[keep])
    src = Source(api, M, M, IRP, JA, AS)
    t = src.dm.transpose()
    try:
        IRPt, JAt, ASt, _ = stable_transpose(M, IRP, JA, AS)
        Bh = block_of_columns(rng, M, 17)
        same(solve(api, torch, t, Bh, False, False, what="upper solve on L^T"), trsm_levels(M, IRPt, JAt, ASt, Bh, False, False),
             "upper solve on L^T")
    finally:
        t.free()
        src.free()


def test_ilu0_pair_in_place_on_a_block_of_5(api, torch):
    """hipSpILU0CSR, then (LOWER, UNIT) and (UPPER, STORED) in place on a block of 5: five single applies"""
    rng = np.random.default_rng(2609)
    M = 800
    IRP, JA, AS = random_ilu(rng, M, 7)
    Bh = block_of_columns(rng, M, 5)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        assert src.dm.ilu0().zeroPivot == -1
        for layout in ("row", "col"):
            blk = Block(torch, M, 5, *layouts_of(M, 5)[layout], host=Bh)
            src.dm.solve_triangular_block(blk.view, lower=True, unit_diagonal=True, out=blk.view)
            src.dm.solve_triangular_block(blk.view, lower=False, unit_diagonal=False, out=blk.view)
            Z = blk.down()
            for c in range(5):
                y = src.dm.solve_triangular(np.ascontiguousarray(Bh[:, c]), lower=True, unit_diagonal=True)
                z = src.dm.solve_triangular(y, lower=False, unit_diagonal=False)
                assert np.isfinite(z).all()
                assert_same_bits(Z[:, c], z, f"ILU(0) pair, {layout}, column {c}")
            blk.padding_intact("ILU(0) pair")
        assert src.dm.triangular_info(True).analyses == 1 and src.dm.triangular_info(False).analyses == 1
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 8. schedule and values
@pytest.mark.parametrize("block_first", [True, False])
def test_schedule_is_shared_with_the_single_solve(api, torch, block_first):
    M, IRP, JA, AS, B = m300()
    Bh = B[:, :17]
    src = Source(api, M, M, IRP, JA, AS)
    try:
        for lower in (True, False):
            assert src.dm.triangular_info(lower).analyses == 0
            if block_first:
                X = solve(api, torch, src.dm, Bh, lower, False, what="block first")
                x0 = src.dm.solve_triangular(np.ascontiguousarray(Bh[:, 0]), lower=lower)
            else:
                x0 = src.dm.solve_triangular(np.ascontiguousarray(Bh[:, 0]), lower=lower)
                X = solve(api, torch, src.dm, Bh, lower, False, what="single first")
            assert_same_bits(X[:, 0], x0, "column 0 is the single solve")
            same(X, m300_ref(lower, False)[:, :17], "shared schedule")
            assert src.dm.triangular_info(lower).analyses == 1
    finally:
        src.free()


def test_values_are_read_live(api, torch):
    rng = np.random.default_rng(2610)
    M, IRP, JA, A, B = m300()
    A2 = A * (1 + si.order_values(rng, A.size, 1) * 1e-3)
    Bh = B[:, :17]
    src = Source(api, M, M, IRP, JA, A)
    try:
        same(solve(api, torch, src.dm, Bh, True, False, what="before"), m300_ref(True, False)[:, :17], "before")
        src.dm.update_values(torch.from_numpy(A2).cuda())
        same(solve(api, torch, src.dm, Bh, True, False, what="after"), trsm_levels(M, IRP, JA, A2, Bh, True, False), "after update_values")
        assert src.dm.triangular_info(True).analyses == 1
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 9. determinism, capture
def test_determinism(api, torch, h300):
    M, _, _, _, B = m300()
    for lower in (True, False):
        x1 = solve(api, torch, h300, B, lower, False, what="first")
        assert_same_bits(solve(api, torch, h300, B, lower, False, what="second"), x1, "repeated solve")


def test_graph_capture(api, torch):
    """captured after the analysis on one stream, replayed twice: the bits of the eager call (a linear chain of launches)"""
    nx, ny, nz = 16, 14, 12
    IRP, JA, AS = laplacian7(nx, ny, nz)
    M = nx * ny * nz
    rng = np.random.default_rng(2611)
    AS = np.where(AS == 6.0, 6.0 + rng.random(AS.size), si.order_values(rng, AS.size, 1) / 7)
    k = 17
    B1, B2 = block_of_columns(rng, M, k), block_of_columns(rng, M, k)
    src = Source(api, M, M, IRP, JA, AS)
    stream = torch.cuda.Stream()
    try:
        src.dm.triangular_analyse(True)
        eager = [solve(api, torch, src.dm, Bh, True, False, what="eager") for Bh in (B1, B2)]
        same(eager[0], trsm_levels(M, IRP, JA, AS, B1, True, False), "eager")
        with torch.cuda.stream(stream):
            b = torch.from_numpy(B1).cuda()
            x = torch.full((M, k), float("nan"), dtype=torch.float64, device="cuda")
            api.lib.spmvHipSetStream(C.c_void_p(stream.cuda_stream))
            torch.cuda.synchronize()
            api.lib.spmvHipSetSync(0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                assert raw(api, src.dm, LOWER, STORED, k, b.data_ptr(), k, ROW, x.data_ptr(), k, ROW) == 0
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert_same_bits(x.cpu().numpy(), eager[0], "replay 1")
            b.copy_(torch.from_numpy(B2))
            x.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert_same_bits(x.cpu().numpy(), eager[1], "replay with a new B")
        assert src.dm.triangular_info(True).analyses == 1
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        src.free()


def test_sync_reports_time_and_last_launch(api, torch, h300):
    M, _, _, _, B = m300()
    solve(api, torch, h300, B[:, :17], True, False, what="timed")
    assert api.lib.spmvHipLastKernelSeconds() > 0
    grid, block = api.last_launch()
    assert block[0] in (256, 1024) and grid[0] >= 1


# ------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals_leave_x_untouched(api, torch, capfd):
    rng = np.random.default_rng(2612)
    M, IRP, JA, AS, Bfull = m300()
    k = 3
    src = Source(api, M, M, IRP, JA, AS)
    keep = []
    B = Block(torch, M, k, ROW, k, host=Bfull[:, :k])
    X = Block(torch, M, k, ROW, k)
    big = Block(torch, 2 * M, k, ROW, k)
    try:
        lib, P = api.lib, C.byref
        h = P(src.dm.handle)

        def refused(call, msg=None, x=X):
            torch.cuda.synchronize()
            before = x.flat.cpu().numpy().view(np.uint64).copy()
            capfd.readouterr()
            assert call() != 0
            err = capfd.readouterr().err
            assert err, "no message"
            if msg:
                assert msg in err, err
            torch.cuda.synchronize()
            assert np.array_equal(x.flat.cpu().numpy().view(np.uint64), before)

        def call(handle=h, uplo=LOWER, diag=STORED, kk=k, b=B.ptr, ldb=k, bl=ROW, x=X.ptr, ldx=k, xl=ROW):
            return lambda: lib.hipSpTRSMCSR(handle, uplo, diag, kk, C.c_void_p(b) if b else None, ldb, bl,
                                            C.c_void_p(x) if x else None, ldx, xl)

        refused(call(handle=None))
        refused(call(b=None), "NULL")
        refused(call(x=None), "NULL")
        refused(call(uplo=2), "uplo")
        refused(call(uplo=-1), "uplo")
        refused(call(diag=2), "diag")
        refused(call(bl=2), "layout")
        refused(call(xl=-1), "layout")
        refused(call(kk=0), "k = 0")
        refused(call(ldb=k - 1), "ldb")
        refused(call(ldx=k - 1), "ldx")
        refused(call(bl=COL, ldb=M - 1), "ldb")
        refused(call(xl=COL, ldx=M - 1), "ldx")
        # overlaps: the same pointer with another layout or leading dimension, and spans that share memory
        refused(call(b=X.ptr, bl=COL, ldb=M), "overlap")
        refused(call(b=big.ptr, ldb=k + 1, x=big.ptr, ldx=k), "overlap", x=big)
        refused(call(b=big.ptr, x=big.ptr + 8 * (M * k // 2)), "overlap", x=big)
        refused(call(b=big.ptr + 8, x=big.ptr), "overlap", x=big)
        # non-square, ELL, ELL made on the device, a multigrid hierarchy
        IRPn, JAn, ASn = random_square(rng, M, 4)
        rect = api.spMatCpyCSR(api.HostCSR(M, M + 5, IRPn, JAn, ASn))
        ell = api.spMatCpyELL(api.HostCSR(M, M, IRP, JA, AS).to_ell())
        ell_dev = api.csr_to_ell_device(src.dm, True)
        keep += [rect, ell, ell_dev]
        refused(call(handle=P(rect.handle), diag=UNIT), "not square")
        refused(call(handle=P(ell.handle), diag=UNIT), "ELL")
        refused(call(handle=P(ell_dev.handle), diag=UNIT), "ELL")
        IRPl, JAl, ASl = laplacian7(8, 8, 8)
        lap = api.spMatCpyCSR(api.HostCSR(512, 512, IRPl, JAl, ASl))
        amg = lap.amg(coarseRows=8)
        keep += [amg, lap]
        refused(call(handle=P(amg.handle), diag=UNIT), "hierarchy")
        # a missing and a doubled diagonal: STORED refused naming the row, UNIT accepted
        for diag in ("none", "twice"):
            I2, J2, A2 = random_square(rng, M, 5, diag=diag)
            bad = diag_pos(M, I2, J2)[1]
            hb = Source(api, M, M, I2, J2, A2)
            keep.append(hb)
            refused(call(handle=P(hb.dm.handle)), f"row {bad} ")
            assert hb.dm.triangular_info(True).firstBadDiag == bad
            assert call(handle=P(hb.dm.handle), diag=UNIT)() == 0
        # NZ at the 32-bit limit: adopted with no value or column array (nothing is read)
        irp = api.DeviceBuffer(16)
        keep.append(irp)
        huge = api.DeviceMatrix()
        h_irp = np.array([0, (1 << 32) - 65536], dtype=np.uint64)
        assert lib.spmvHipAdoptCSR(P(huge.handle), 1, 1, int(h_irp[1]), irp.ptr, 8, None, None, h_irp.ctypes.data_as(C.c_void_p)) == 0
        keep.append(huge)
        refused(call(handle=P(huge.handle), diag=UNIT), "NZ")
        # entries, a column array, no value array, not unit-value
        ja = api.DeviceBuffer(4 * JA.size).up(JA.astype(np.uint32))
        irp4 = api.DeviceBuffer(4 * (M + 1)).up(IRP.astype(np.uint32))
        keep += [ja, irp4]
        noval = api.DeviceMatrix()
        h4 = IRP.astype(np.uint32)
        assert lib.spmvHipAdoptCSR(P(noval.handle), M, M, JA.size, irp4.ptr, 4, ja.ptr, None, h4.ctypes.data_as(C.c_void_p)) == 0
        keep.append(noval)
        refused(call(handle=P(noval.handle), diag=UNIT), "no value array")
        # a freed handle
        gone = Source(api, M, M, IRP, JA, AS)
        gone.free()
        refused(call(handle=P(gone.dm.handle)), "not a device handle")
        # and the handle still solves
        assert call()() == 0
        torch.cuda.synchronize()
        same(X.down(), m300_ref(True, False)[:, :k], "after the refusals")
    finally:
        src.free()
        for item in keep:
            item.free()


def test_python_layer_refuses_before_the_library(api, torch, h300):
    M, _, _, _, B = m300()
    good = torch.from_numpy(np.ascontiguousarray(B[:, :3])).cuda()
    with pytest.raises(api.SpmvHipError):
        h300.solve_triangular_block(good[:-1])                           # the wrong number of rows
    with pytest.raises(api.SpmvHipError):
        h300.solve_triangular_block(torch.zeros((M, 6), dtype=torch.float64, device="cuda")[:, ::2])   # no unit stride
    with pytest.raises(api.SpmvHipError):
        h300.solve_triangular_block(good, out=torch.zeros((M, 4), dtype=torch.float64, device="cuda"))
    with pytest.raises(api.SpmvHipError):
        h300.solve_triangular_block(B[:, :3].copy(), out=good)           # `out` is for device calls
    X = h300.solve_triangular_block(np.ascontiguousarray(B[:, :3]))      # a host call returns numpy
    assert isinstance(X, np.ndarray)
    same(X, m300_ref(True, False)[:, :3], "host call")
    same(h300.solve_triangular_block(good).cpu().numpy(), m300_ref(True, False)[:, :3], "device call, new tensor")


# ------------------------------------------------------------------------------------------------- 11. memory
def test_no_device_memory_is_taken_by_solves(api, torch):
    """an analysed handle: device memory is the same before the first and after the twentieth solve"""
    M, IRP, JA, AS, B = m300()
    src = Source(api, M, M, IRP, JA, AS)
    try:
        src.dm.triangular_analyse(True)
        b = torch.from_numpy(np.ascontiguousarray(B[:, :17])).cuda()
        x = torch.empty_like(b)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        for _ in range(20):
            src.dm.solve_triangular_block(b, out=x)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == before
        same(x.cpu().numpy(), m300_ref(True, False)[:, :17], "after twenty solves")
    finally:
        src.free()
