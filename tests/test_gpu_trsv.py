"""Triangular solves on the device (hipSpTRSVCSR, spmvHipTriAnalyse, spmvHipTriInfo; DeviceMatrix.solve_triangular):
every case equals the test side's serial loop (tests/trsv_ref.py) in all bits -- finite rows by bits, infinities by sign,
NaN as NaN.  The inputs are order-sensitive (tests/test_trsv_abi.py shows that on the host)."""
import ctypes as C

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits
from test_trsv_abi import laplacian7, random_square
from transpose_ref import stable_transpose
from trsv_ref import diag_pos, trsv_levels, trsv_loop

pytestmark = pytest.mark.gpu

LOWER, UPPER, STORED, UNIT = 0, 1, 0, 1
POISON = 0x7FF4DEADBEEF0001


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
    api.lib.spmvHipSetStream(None)
    api.lib.spmvHipSetSync(1)
    api.lib.spmvHipSetVariant(b"hipSpTRSVCSR", 256)


class Source:
    """an uploaded handle, or an adopted one (4- or 8-byte row pointers) over the test's own device arrays"""

    def __init__(self, api, M, N, IRP, JA, AS, adopt=0):
        self.bufs = []
        if adopt:
            irp, ja, a = IRP.astype(np.uint64 if adopt == 8 else np.uint32), JA.astype(np.uint32), np.ascontiguousarray(AS, np.float64)
            self.bufs = [api.DeviceBuffer(v.nbytes).up(v) for v in (irp, ja, a)]
            self.dm = api.DeviceMatrix()
            assert api.lib.spmvHipAdoptCSR(C.byref(self.dm.handle), M, N, JA.size, self.bufs[0].ptr, adopt, self.bufs[1].ptr,
                                           self.bufs[2].ptr, irp.ctypes.data_as(C.c_void_p)) == 0
        else:
            self.dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))

    def free(self):
        self.dm.free()
        for b in self.bufs:
            b.free()


def same(x, ref, what):
    """finite rows by bits, infinities by sign, NaN as NaN"""
    x, ref = np.asarray(x), np.asarray(ref)
    fin = np.isfinite(ref)
    assert_same_bits(x[fin], ref[fin], what)
    inf = np.isinf(ref)
    assert np.array_equal(x[inf], ref[inf]), what
    assert np.isnan(x[np.isnan(ref)]).all(), what


def check(api, dm, M, IRP, JA, AS, b, lower, unit, what):
    x = dm.solve_triangular(b, lower=lower, unit_diagonal=unit)
    same(x, trsv_levels(M, IRP, JA, AS, b, lower, unit), what)
    return x


def _solve_raw(api, dm, uplo, diag, b_ptr, x_ptr):
    return api.lib.hipSpTRSVCSR(C.byref(dm.handle), uplo, diag, b_ptr, x_ptr)


def _info_tuple(info):
    return tuple(getattr(info, f[0]) for f in info._fields_ if f[0] != "analysisMs")


def long_rows_matrix(rng):
    """level 0: 3000 diagonal-only rows; level 1: 3000 rows into them, short ones and five of more than 2 048 strict entries
    (with repeats, unsorted)"""
    M, h = 6000, 3000
    rows, cols = [np.arange(M)], [np.arange(M)]
    lens = rng.integers(0, 9, h)
    lens[[7, 500, 1400, 2222, 2999]] = [2100, 2500, 3000, 4100, 2049]
    r = np.repeat(np.arange(h, M), lens)
    rows.append(r)
    cols.append(rng.integers(0, h, r.size))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = np.where(rows == cols, 2.0 + rng.random(rows.size), si.order_values(rng, rows.size, 2) / 50)
    o = rng.permutation(rows.size)
    return M, si.assemble(M, rows[o], cols[o], vals[o])


# ------------------------------------------------------------------------------------------------- 1. matrices
def test_random_lower_sorted(api):
    rng = np.random.default_rng(1701)
    M = 2000
    IRP, JA, AS = random_square(rng, M, 10, shuffle=False)
    rows = si.row_of_entry(IRP)
    keep = JA.astype(np.int64) <= rows                                   # lower triangle only
    IRP, JA, AS = si.assemble(M, rows[keep], JA[keep].astype(np.int64), AS[keep])
    src = Source(api, M, M, IRP, JA, AS)
    try:
        b = si.order_values(rng, M)
        check(api, src.dm, M, IRP, JA, AS, b, True, False, "random lower, sorted")
        info = src.dm.triangular_info(True)
        assert info.analyses == 1 and info.levels > 1 and info.firstBadDiag == -1
    finally:
        src.free()


@pytest.mark.parametrize("adopt", [0, 4, 8])
def test_unsorted_whole_matrix_both_triangles(api, adopt):
    """unsorted rows, repeated strict and diagonal-side pairs, the whole matrix solved as lower and as upper"""
    rng = np.random.default_rng(1702 + adopt)
    M = 2500
    IRP, JA, AS = random_square(rng, M, 12)
    src = Source(api, M, M, IRP, JA, AS, adopt)
    try:
        b = si.order_values(rng, M)
        for lower in (True, False):
            for unit in (False, True):
                check(api, src.dm, M, IRP, JA, AS, b, lower, unit, f"adopt {adopt}, lower {lower}, unit {unit}")
    finally:
        src.free()


def test_laplacian_88_levels(api):
    nx, ny, nz = 40, 30, 20
    IRP, JA, AS = laplacian7(nx, ny, nz)
    M = nx * ny * nz
    rng = np.random.default_rng(1703)
    AS = np.where(AS == 6.0, 6.0 + rng.random(AS.size), si.order_values(rng, AS.size, 1) / 7)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        b = si.order_values(rng, M)
        for lower in (True, False):
            check(api, src.dm, M, IRP, JA, AS, b, lower, False, f"laplacian lower {lower}")
            info = src.dm.triangular_info(lower)
            assert info.levels == nx + ny + nz - 2 == 88
            assert info.maxLevelRows <= nx * ny and info.longRows == 0
    finally:
        src.free()


@pytest.mark.parametrize("T", [256, 0])
def test_chain_of_5000(api, T):
    """a bidiagonal chain: depth 5 000, every level one row -- all in runs (T = 256), or a launch per level (T = 0)"""
    api.lib.spmvHipSetVariant(b"hipSpTRSVCSR", T)
    rng = np.random.default_rng(1704)
    M = 5000
    i = np.arange(M)
    rows, cols = np.concatenate([i, i[1:]]), np.concatenate([i, i[1:] - 1])
    vals = np.where(rows == cols, 1.0 + rng.random(rows.size), rng.uniform(-1, 1, rows.size))
    IRP, JA, AS = si.assemble(M, rows, cols, vals)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        b = si.order_values(rng, M)
        check(api, src.dm, M, IRP, JA, AS, b, True, False, f"chain, T = {T}")
        info = src.dm.triangular_info(True)
        assert info.levels == M and info.maxLevelRows == 1
        if T:
            assert info.fusedLevels == M and info.launches == 1
        else:
            assert info.fusedLevels == 0 and info.launches == M
        same(src.dm.solve_triangular(b, lower=False), trsv_loop(M, IRP, JA, AS, b, False, False), "chain, upper (diagonal)")
        assert src.dm.triangular_info(False).levels == 1
    finally:
        src.free()


def test_long_rows(api):
    rng = np.random.default_rng(1705)
    M, (IRP, JA, AS) = long_rows_matrix(rng)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        b = si.order_values(rng, M)
        check(api, src.dm, M, IRP, JA, AS, b, True, False, "long rows")
        check(api, src.dm, M, IRP, JA, AS, b, True, True, "long rows, unit")
        info = src.dm.triangular_info(True)
        assert info.levels == 2 and info.longRows >= 5
    finally:
        src.free()


def test_unit_diagonal_stored_and_absent(api):
    rng = np.random.default_rng(1706)
    M = 3000
    for diag in ("one", "none", "twice"):
        IRP, JA, AS = random_square(rng, M, 8, diag=diag)
        src = Source(api, M, M, IRP, JA, AS)
        try:
            b = si.order_values(rng, M)
            for lower in (True, False):
                check(api, src.dm, M, IRP, JA, AS, b, lower, True, f"unit, diagonal {diag}")
        finally:
            src.free()


def test_ilu0_pair_on_one_handle(api):
    """a strictly lower L with unit diagonal and U with the diagonal in one CSR: (LOWER, UNIT) then (UPPER, STORED)"""
    rng = np.random.default_rng(1707)
    M = 4000
    IRP, JA, AS = random_square(rng, M, 9)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        b = si.order_values(rng, M)
        torch = pytest.importorskip("torch")
        bt = torch.from_numpy(b).cuda()
        y = src.dm.solve_triangular(bt, lower=True, unit_diagonal=True)
        z = src.dm.solve_triangular(y, lower=False, unit_diagonal=False, out=y)      # in place
        y_ref = trsv_levels(M, IRP, JA, AS, b, True, True)
        same(z.cpu().numpy(), trsv_levels(M, IRP, JA, AS, y_ref, False, False), "ILU(0) pair")
    finally:
        src.free()


def test_small_shapes(api):
    rng = np.random.default_rng(1708)
    # rows holding only the diagonal
    M = 700
    IRP, JA, AS = si.assemble(M, np.arange(M), np.arange(M), si.order_values(rng, M))
    src = Source(api, M, M, IRP, JA, AS)
    try:
        b = si.order_values(rng, M)
        for lower in (True, False):
            check(api, src.dm, M, IRP, JA, AS, b, lower, False, "diagonal only")
        assert src.dm.triangular_info(True).levels == 1
    finally:
        src.free()
    # M = 1
    src = Source(api, 1, 1, np.array([0, 1], np.uint64), np.array([0], np.uint64), np.array([3.0]))
    try:
        same(src.dm.solve_triangular(np.array([-7.0])), np.array([-7.0 / 3.0]), "M = 1")
    finally:
        src.free()
    # M = 0: success, nothing written
    src = Source(api, 0, 0, np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    try:
        dv = api.DeviceVector(1)
        assert _solve_raw(api, src.dm, LOWER, STORED, dv.ptr, dv.ptr) == 0
        assert src.dm.triangular_info(True).levels == 0
        dv.free()
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 2. handles
def test_unit_value_handle(api):
    rng = np.random.default_rng(1709)
    M = 3000
    IRP, JA, _ = random_square(rng, M, 8)
    AS = np.full(JA.size, 1.0)
    b = si.order_values(rng, M)
    xs = []
    for unit_values in (1, 0):
        api.lib.spmvHipSetUnitValues(unit_values)
        src = Source(api, M, M, IRP, JA, AS, 4)
        try:
            v = C.c_double(0)
            assert api.lib.spmvHipUnitValue(C.byref(src.dm.handle), C.byref(v)) == unit_values
            xs.append(check(api, src.dm, M, IRP, JA, AS, b, True, True, f"pattern handle, unit values {unit_values}"))
            xs.append(check(api, src.dm, M, IRP, JA, AS, b, False, False, f"pattern handle, unit values {unit_values}"))
        finally:
            src.free()
    assert_same_bits(xs[0], xs[2], "unit-value lower")
    assert_same_bits(xs[1], xs[3], "unit-value upper")


def test_upper_solve_on_a_transpose(api):
    rng = np.random.default_rng(1710)
    M = 3000
    IRP, JA, AS = random_square(rng, M, 8)
    rows = si.row_of_entry(IRP)
    keep = JA.astype(np.int64) <= rows
    IRP, JA, AS = si.assemble(M, rows[keep], JA[keep].astype(np.int64), AS[keep])
    src = Source(api, M, M, IRP, JA, AS)
    t = src.dm.transpose()
    try:
        IRPt, JAt, ASt, _ = stable_transpose(M, IRP, JA, AS)
        b = si.order_values(rng, M)
        check(api, t, M, IRPt, JAt, ASt, b, False, False, "upper solve on L^T")
    finally:
        t.free()
        src.free()


def test_zero_diagonals_and_in_place(api):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1711)
    M = 3000
    IRP, JA, AS = random_square(rng, M, 8)
    dpos, _ = diag_pos(M, IRP, JA)
    AS = AS.copy()
    AS[dpos[[10, 1500, 2900]]] = 0.0
    src = Source(api, M, M, IRP, JA, AS)
    try:
        b = si.order_values(rng, M)
        for lower in (True, False):
            x = check(api, src.dm, M, IRP, JA, AS, b, lower, False, f"zero diagonals, lower {lower}")
            assert not np.isfinite(x).all()
            bt = torch.from_numpy(b).cuda()
            out = src.dm.solve_triangular(bt, lower=lower, out=bt)
            assert out.data_ptr() == bt.data_ptr()
            same(bt.cpu().numpy(), x, f"in place, lower {lower}")
    finally:
        src.free()


def _carved(torch, v, off):
    """v inside a larger device tensor of poison, at element offset `off`: (the larger tensor, the view)"""
    host = np.full(v.size + 2, POISON, dtype=np.uint64).view(np.float64)
    host[off:off + v.size] = v
    big = torch.from_numpy(host).cuda()
    return big, big[off:off + v.size]


def _outside_intact(big, off, n, what):
    host = big.cpu().numpy().view(np.uint64)
    assert (host[:off] == POISON).all() and (host[off + n:] == POISON).all(), what + ": a neighbour of the view was written"


def test_b_and_x_at_odd_offsets(api):
    """b and x that are only 8-byte aligned (views at element offset 1 of larger tensors), apart and in place, M odd: the
    same bits, and the elements next to the views keep their poison"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1718)
    M = 5001
    IRP, JA, AS = random_square(rng, M, 9)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        b = si.order_values(rng, M)
        for uplo, diag in ((LOWER, UNIT), (UPPER, STORED), (LOWER, STORED)):
            ref = trsv_levels(M, IRP, JA, AS, b, uplo == LOWER, diag == UNIT)
            for ob, ox in ((0, 0), (1, 0), (0, 1), (1, 1)):
                what = f"uplo {uplo}, diag {diag}, b+{ob}, x+{ox}"
                bigb, vb = _carved(torch, b, ob)
                bigx, vx = _carved(torch, np.zeros(M), ox)
                vx.fill_(float("nan"))
                torch.cuda.synchronize()
                assert vb.data_ptr() % 16 == 8 * ob and vx.data_ptr() % 16 == 8 * ox
                assert _solve_raw(api, src.dm, uplo, diag, vb.data_ptr(), vx.data_ptr()) == 0
                same(vx.cpu().numpy(), ref, what)
                _outside_intact(bigx, ox, M, what)
                assert_same_bits(vb.cpu().numpy(), b, what + ": b is read only")
            for o in (0, 1):
                big, v = _carved(torch, b, o)
                assert _solve_raw(api, src.dm, uplo, diag, v.data_ptr(), v.data_ptr()) == 0
                same(v.cpu().numpy(), ref, f"uplo {uplo}, diag {diag}, in place at +{o}")
                _outside_intact(big, o, M, f"in place at +{o}")
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 3. values change
def test_values_change_pattern_stays(api):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1712)
    M = 3000
    IRP, JA, A = random_square(rng, M, 8)
    B = A * (1 + si.order_values(rng, A.size, 1) * 1e-3)
    C2 = A * (1 - si.order_values(rng, A.size, 1) * 1e-3)
    b = si.order_values(rng, M)
    for adopt in (0, 4):
        src = Source(api, M, M, IRP, JA, A, adopt)
        try:
            check(api, src.dm, M, IRP, JA, A, b, True, False, "before")
            before = src.dm.triangular_info(True)
            src.dm.update_values(torch.from_numpy(B).cuda())
            check(api, src.dm, M, IRP, JA, B, b, True, False, "after update_values")
            if adopt:
                src.bufs[2].up(np.ascontiguousarray(C2))
                src.dm.values_changed()
                check(api, src.dm, M, IRP, JA, C2, b, True, False, "after values_changed")
            after = src.dm.triangular_info(True)
            assert after.analyses == 1 and after.levels == before.levels
        finally:
            src.free()


def test_determinism(api):
    rng = np.random.default_rng(1713)
    M = 20000
    IRP, JA, AS = random_square(rng, M, 10)
    b = si.order_values(rng, M)
    s1, s2 = Source(api, M, M, IRP, JA, AS), Source(api, M, M, IRP, JA, AS, 8)
    try:
        for lower in (True, False):
            s1.dm.triangular_analyse(lower)
            s2.dm.triangular_analyse(lower)
            s1.dm.triangular_analyse(lower)                                   # a no-op: it exists
            i1, i2 = s1.dm.triangular_info(lower), s2.dm.triangular_info(lower)
            assert _info_tuple(i1) == _info_tuple(i2) and i1.analyses == 1
            x1 = s1.dm.solve_triangular(b, lower=lower)
            assert_same_bits(s1.dm.solve_triangular(b, lower=lower), x1, "repeated solve")
            assert_same_bits(s2.dm.solve_triangular(b, lower=lower), x1, "second handle")
    finally:
        s1.free()
        s2.free()


def test_graph_capture(api):
    torch = pytest.importorskip("torch")
    nx, ny, nz = 40, 30, 20
    IRP, JA, AS = laplacian7(nx, ny, nz)
    M = nx * ny * nz
    rng = np.random.default_rng(1714)
    src = Source(api, M, M, IRP, JA, AS)
    stream = torch.cuda.Stream()
    try:
        src.dm.triangular_analyse(True)
        b1, b2 = si.order_values(rng, M), si.order_values(rng, M)
        with torch.cuda.stream(stream):
            b = torch.from_numpy(b1).cuda()
            x = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
            api.lib.spmvHipSetStream(C.c_void_p(stream.cuda_stream))
            torch.cuda.synchronize()
            api.lib.spmvHipSetSync(0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                assert _solve_raw(api, src.dm, LOWER, STORED, b.data_ptr(), x.data_ptr()) == 0
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            same(x.cpu().numpy(), trsv_levels(M, IRP, JA, AS, b1, True, False), "replay 1")
            b.copy_(torch.from_numpy(b2))
            x.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            same(x.cpu().numpy(), trsv_levels(M, IRP, JA, AS, b2, True, False), "replay with a new b")
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        src.free()


# ------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_x_untouched(api, capfd):
    rng = np.random.default_rng(1715)
    M = 2000
    IRP, JA, AS = random_square(rng, M, 6)
    src = Source(api, M, M, IRP, JA, AS)
    keep = []
    dx, db = api.DeviceVector(M), api.DeviceVector(M).up(si.order_values(rng, M))
    big = api.DeviceVector(2 * M)
    try:
        lib, P = api.lib, C.byref

        def refused(call, msg=None, x=dx):
            x.poison()
            before = x.down().view(np.uint64).copy()
            capfd.readouterr()
            assert call() != 0
            err = capfd.readouterr().err
            assert err, "no message"
            if msg:
                assert msg in err, err
            assert np.array_equal(x.down().view(np.uint64), before)

        refused(lambda: lib.hipSpTRSVCSR(None, LOWER, STORED, db.ptr, dx.ptr))
        refused(lambda: lib.hipSpTRSVCSR(P(src.dm.handle), LOWER, STORED, None, dx.ptr))
        refused(lambda: lib.hipSpTRSVCSR(P(src.dm.handle), LOWER, STORED, db.ptr, None))
        refused(lambda: lib.hipSpTRSVCSR(P(src.dm.handle), 2, STORED, db.ptr, dx.ptr), "uplo")
        refused(lambda: lib.hipSpTRSVCSR(P(src.dm.handle), -1, STORED, db.ptr, dx.ptr), "uplo")
        refused(lambda: lib.hipSpTRSVCSR(P(src.dm.handle), LOWER, 2, db.ptr, dx.ptr), "diag")
        # b and x overlapping without being equal
        refused(lambda: lib.hipSpTRSVCSR(P(src.dm.handle), LOWER, STORED, big.ptr, C.c_void_p(big.ptr.value + 8 * (M // 2))),
                "overlap", x=big)
        # non-square, ELL, ELL made on the device
        IRPn, JAn, ASn = random_square(rng, M, 4)
        rect = api.spMatCpyCSR(api.HostCSR(M, M + 5, IRPn, JAn, ASn))
        ell = api.spMatCpyELL(api.HostCSR(M, M, IRP, JA, AS).to_ell())
        ell_dev = api.csr_to_ell_device(src.dm, True)
        keep += [rect, ell, ell_dev]
        refused(lambda: lib.hipSpTRSVCSR(P(rect.handle), LOWER, UNIT, db.ptr, dx.ptr), "not square")
        refused(lambda: lib.hipSpTRSVCSR(P(ell.handle), LOWER, UNIT, db.ptr, dx.ptr), "ELL")
        refused(lambda: lib.hipSpTRSVCSR(P(ell_dev.handle), LOWER, UNIT, db.ptr, dx.ptr), "ELL")
        refused(lambda: lib.spmvHipTriAnalyse(P(ell.handle), LOWER), "ELL")
        # a missing and a doubled diagonal: STORED refused naming the row, UNIT accepted
        for diag in ("none", "twice"):
            I2, J2, A2 = random_square(rng, M, 5, diag=diag)
            bad = diag_pos(M, I2, J2)[1]
            h = Source(api, M, M, I2, J2, A2)
            keep.append(h)
            refused(lambda: lib.hipSpTRSVCSR(P(h.dm.handle), LOWER, STORED, db.ptr, dx.ptr), f"row {bad} ")
            assert h.dm.triangular_info(True).firstBadDiag == bad
            assert lib.hipSpTRSVCSR(P(h.dm.handle), LOWER, UNIT, db.ptr, dx.ptr) == 0
        # NZ at the 32-bit limit: adopted with no value or column array (nothing is read)
        irp = api.DeviceBuffer(16)
        keep.append(irp)
        huge = api.DeviceMatrix()
        h_irp = np.array([0, (1 << 32) - 65536], dtype=np.uint64)
        assert lib.spmvHipAdoptCSR(P(huge.handle), 1, 1, int(h_irp[1]), irp.ptr, 8, None, None, h_irp.ctypes.data_as(C.c_void_p)) == 0
        keep.append(huge)
        refused(lambda: lib.hipSpTRSVCSR(P(huge.handle), LOWER, UNIT, db.ptr, dx.ptr), "NZ")
        # a freed handle
        gone = Source(api, M, M, IRP, JA, AS)
        gone.free()
        refused(lambda: lib.hipSpTRSVCSR(P(gone.dm.handle), LOWER, STORED, db.ptr, dx.ptr), "not a device handle")
        refused(lambda: lib.spmvHipTriAnalyse(P(gone.dm.handle), LOWER), "not a device handle")
        # and the handle still solves
        same(src.dm.solve_triangular(db.down()), trsv_levels(M, IRP, JA, AS, db.down(), True, False), "after the refusals")
    finally:
        src.free()
        for k in keep:
            k.free()
        for v in (dx, db, big):
            v.free()


# ------------------------------------------------------------------------------------------------- 5. SpMV unchanged
def test_spmv_unchanged_by_the_analysis(api):
    rng = np.random.default_rng(1716)
    M = 30000
    IRP, JA, AS = random_square(rng, M, 12)
    src = Source(api, M, M, IRP, JA, AS)
    dx, dy = api.DeviceVector(M).up(si.order_values(rng, M)), api.DeviceVector(M)
    try:
        api.spmv("hipSpMVRowsCSR", src.dm, dx, dy)
        y0 = dy.down()
        src.dm.triangular_analyse(True)
        src.dm.triangular_analyse(False)
        dy.poison()
        api.spmv("hipSpMVRowsCSR", src.dm, dx, dy)
        assert_same_bits(dy.down(), y0, "hipSpMVRowsCSR after the analysis")
    finally:
        dx.free()
        dy.free()
        src.free()


# ------------------------------------------------------------------------------------------------- 6. memory
def test_device_memory_comes_back(api):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1717)
    M = 200_000
    IRP, JA, AS = random_square(rng, M, 12)
    b = si.order_values(rng, M)
    free = []
    for _ in range(20):
        src = Source(api, M, M, IRP, JA, AS)
        src.dm.triangular_analyse(True)
        src.dm.solve_triangular(b, lower=True)
        src.dm.solve_triangular(b, lower=False, unit_diagonal=True)
        src.free()
        api.spmvHipFinalize()
        api.spmvHipInit(0)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    # free memory is the device's, shared with other processes: a leak shows as a decline that stays, so the median of the
    # later cycles and the last one are compared, not a single sample
    assert np.median(free[2:]) >= free[1] - (8 << 20) and free[-1] >= free[1] - (8 << 20), free
