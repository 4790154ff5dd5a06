"""Y = A X for a block of vectors (hipSpMMRowsCSR / DeviceMatrix.matmul): every column of Y is bit-identical to sgemvSerial
on the matching column of X, for every width, layout and leading dimension, every row shape, stored entry order, adopted
and pattern handles, updated values, streams and graphs; the ld padding of Y is never written; refusals leave Y as it was."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_csr

pytestmark = pytest.mark.gpu

ROW, COL = 0, 1
POISON = np.array([0x7FF8DEADDEADDEAD], dtype=np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    """every test starts (and leaves) with the default variants, unit detection, synchronous launches, default stream"""
    yield
    api.set_variant("hipSpMVRowsCSR", 2)
    api.lib.spmvHipSetUnitValues(1)
    api.lib.spmvHipSetStream(None)
    api.lib.spmvHipSetSync(1)


def _x(rng, shape):
    return np.sin(rng.uniform(0, 2 * np.pi, size=shape)) * 3e-5


@pytest.fixture(scope="module")
def mat():
    """~375 k entries, rows of 2..13, sorted distinct columns"""
    rng = np.random.default_rng(1601)
    M = N = 50_000
    IRP, JA, AS = random_csr(rng, M, N, rng.integers(2, 14, size=M))
    assert JA.size >= 350_000
    return M, N, IRP, JA, AS


def _pack(A, layout, ld):
    """(rows, k) -> flat buffer in `layout` with leading dimension ld, padding poisoned"""
    rows, k = A.shape
    if layout == ROW:
        buf = np.full(max(rows * ld, 1), POISON)
        if rows:
            buf[:rows * ld].reshape(rows, ld)[:, :k] = A
    else:
        buf = np.full(max(k * ld, 1), POISON)
        buf[:k * ld].reshape(k, ld)[:, :rows] = A.T
    return buf


def _unpack(buf, layout, ld, rows, k):
    if layout == ROW:
        return buf[:rows * ld].reshape(rows, ld)[:, :k].copy() if rows else np.empty((0, k))
    return buf[:k * ld].reshape(k, ld)[:, :rows].T.copy()


def _padding_poisoned(buf, layout, ld, rows, k):
    mask = np.ones(buf.size, dtype=bool)
    if layout == ROW and rows:
        mask[:rows * ld].reshape(rows, ld)[:, :k] = False
    elif layout == COL:
        mask[:k * ld].reshape(k, ld)[:, :rows] = False
    return np.array_equal(buf[mask].view(np.uint64), np.full(mask.sum(), POISON).view(np.uint64))


def _spmm(api, dm, X, M, xl=ROW, yl=ROW, ldx=None, ldy=None, full=False):
    """hipSpMMRowsCSR through raw device buffers; returns Y (M, k) [and the whole Y buffer]"""
    N, k = X.shape
    ldx = ldx if ldx is not None else (k if xl == ROW else N)
    ldy = ldy if ldy is not None else (k if yl == ROW else M)
    hx, hy = _pack(X, xl, ldx), _pack(np.zeros((M, k)), yl, ldy)
    hy[:] = POISON
    dx, dy = api.DeviceBuffer(hx.nbytes).up(hx), api.DeviceBuffer(hy.nbytes).up(hy)
    try:
        rc = api.lib.hipSpMMRowsCSR(C.byref(dm.handle), k, dx.ptr, ldx, xl, dy.ptr, ldy, yl)
        assert rc == 0
        out = dy.down(np.float64)
    finally:
        dx.free()
        dy.free()
    Y = _unpack(out, yl, ldy, M, k)
    return (Y, out, ldy) if full else Y


def _expect(oracle, IRP, JA, AS, X):
    return np.stack([oracle.csr_serial(IRP, JA, AS, X[:, c]) for c in range(X.shape[1])], axis=1) \
        if X.shape[1] else np.empty((IRP.size - 1, 0))


def _assert_bits(Y, Yref, what, equal_nan=False):
    for c in range(Yref.shape[1]):
        assert np.array_equal(Y[:, c], Yref[:, c], equal_nan=equal_nan), (what, c)
    if not equal_nan:
        assert np.array_equal(Y.view(np.uint64), Yref.view(np.uint64)), what          # signs of zeros too


# ------------------------------------------------------------------------------------------------- 1. widths and layouts
@pytest.mark.parametrize("k", [1, 2, 3, 4, 7, 8, 15, 16, 17, 33])
@pytest.mark.parametrize("xl,yl", [(ROW, ROW), (ROW, COL), (COL, ROW), (COL, COL)], ids=["XrYr", "XrYc", "XcYr", "XcYc"])
def test_widths_and_layouts(api, oracle, mat, k, xl, yl):
    """Every width (panels of 16 and a narrower rest), every layout pair, leading dimensions larger than needed: the
    columns have the oracle's bits and the padding of Y is still poison."""
    M, N, IRP, JA, AS = mat
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    try:
        X = _x(np.random.default_rng(k), (N, k))
        ldx = k + 3 if xl == ROW else N + 5
        ldy = k + 2 if yl == ROW else M + 7
        Y, buf, _ = _spmm(api, dm, X, M, xl, yl, ldx, ldy, full=True)
        _assert_bits(Y, _expect(oracle, IRP, JA, AS, X), (k, xl, yl))
        assert _padding_poisoned(buf, yl, ldy, M, k), "Y was written outside the M x k block"
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------- 2. shapes
def _long_rows_case(rng):
    """rows of more than 2048 and more than 65 536 entries among short and empty rows"""
    M, N = 400, 200_000
    lens = rng.integers(0, 40, size=M)
    lens[rng.random(M) < 0.2] = 0
    lens[3], lens[17], lens[100], lens[250] = 3000, 70_000, 2049, 9000
    IRP, JA, AS = random_csr(rng, M, N, lens)
    return M, N, IRP, JA, AS


@pytest.mark.parametrize("k", [1, 5, 16, 17])
def test_long_and_empty_rows(api, oracle, k):
    rng = np.random.default_rng(2049)
    M, N, IRP, JA, AS = _long_rows_case(rng)
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    try:
        X = _x(rng, (N, k))
        for xl, yl in ((ROW, ROW), (COL, COL)):
            _assert_bits(_spmm(api, dm, X, M, xl, yl), _expect(oracle, IRP, JA, AS, X), (k, xl, yl))
    finally:
        dm.free()


def test_matrix_without_entries(api):
    """no entries at all: every element of Y is +0.0"""
    M, N, k = 300, 50, 6
    dm = api.spMatCpyCSR(api.HostCSR(M, N, np.zeros(M + 1), np.zeros(0), np.zeros(0)))
    try:
        Y = _spmm(api, dm, _x(np.random.default_rng(0), (N, k)), M)
        assert np.array_equal(Y.view(np.uint64), np.zeros((M, k), dtype=np.uint64))
    finally:
        dm.free()


@pytest.mark.parametrize("M,N", [(40_000, 300), (300, 200_000)], ids=["tall", "wide"])
def test_rectangular(api, oracle, M, N):
    rng = np.random.default_rng(M + N)
    IRP, JA, AS = random_csr(rng, M, N, rng.integers(0, min(N, 60), size=M))
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    try:
        X = _x(rng, (N, 9))
        for xl, yl in ((ROW, ROW), (COL, ROW), (ROW, COL)):
            _assert_bits(_spmm(api, dm, X, M, xl, yl), _expect(oracle, IRP, JA, AS, X), (M, N, xl, yl))
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------- 3. entry order
def test_unsorted_and_repeated_columns(api, oracle):
    """Columns in random order, repeated inside rows, values over 16 decades: the bits are those of the stored-order walk
    (which a sorted-order sum would not give).  Short rows and two long ones."""
    rng = np.random.default_rng(77)
    M, N = 3000, 500
    lens = rng.integers(0, 60, size=M)
    lens[5], lens[2000] = 5000, 2100
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(lens)
    JA = rng.integers(0, N, size=int(IRP[-1])).astype(np.uint64)
    AS = rng.uniform(-1, 1, size=JA.size) * 10.0 ** rng.integers(-8, 8, size=JA.size)
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    try:
        X = _x(rng, (N, 12))
        Yref = _expect(oracle, IRP, JA, AS, X)
        # the check can tell the orders apart: a sorted walk differs somewhere
        order = np.concatenate([np.argsort(JA[int(IRP[r]):int(IRP[r + 1])], kind="stable") + int(IRP[r]) for r in range(M)])
        assert not np.array_equal(_expect(oracle, IRP, JA[order], AS[order], X), Yref)
        _assert_bits(_spmm(api, dm, X, M), Yref, "row-major")
        _assert_bits(_spmm(api, dm, X, M, COL, COL), Yref, "column-major")
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------- 4. adopted handles
@pytest.mark.parametrize("irp_bytes", [4, 8])
def test_adopted_handle(api, oracle, mat, irp_bytes):
    M, N, IRP, JA, AS = mat
    irp = IRP.astype(np.uint32 if irp_bytes == 4 else np.uint64)
    ja = JA.astype(np.uint32)
    bufs = [api.DeviceBuffer(irp.nbytes).up(irp), api.DeviceBuffer(ja.nbytes).up(ja), api.DeviceBuffer(AS.nbytes).up(AS)]
    dm = api.DeviceMatrix()
    try:
        assert api.lib.spmvHipAdoptCSR(C.byref(dm.handle), M, N, JA.size, bufs[0].ptr, irp_bytes, bufs[1].ptr, bufs[2].ptr,
                                       irp.ctypes.data_as(C.c_void_p)) == 0
        X = _x(np.random.default_rng(irp_bytes), (N, 10))
        _assert_bits(_spmm(api, dm, X, M), _expect(oracle, IRP, JA, AS, X), irp_bytes)
    finally:
        dm.free()
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------- 5. pattern handles
@pytest.mark.parametrize("value", [1.0, 2.5])
def test_pattern_handle(api, oracle, mat, value):
    """all values equal: the unit kernels (value from a register) give the same bits as the valued walk"""
    M, N, IRP, JA, _ = mat
    AS = np.full(JA.size, value)
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    try:
        v = C.c_double()
        assert api.lib.spmvHipUnitValue(C.byref(dm.handle), C.byref(v)) == 1 and v.value == value
        X = _x(np.random.default_rng(5), (N, 16))
        Yref = _expect(oracle, IRP, JA, AS, X)
        _assert_bits(_spmm(api, dm, X, M), Yref, value)
        _assert_bits(_spmm(api, dm, X[:, :3], M), Yref[:, :3], value)
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------- 6. value updates
@pytest.mark.parametrize("start", ["valued", "unit"])
def test_value_updates(api, oracle, mat, start):
    """after spmvHipUpdateValues (non-unit -> non-unit, unit -> non-unit) the next product has the new values' bits"""
    M, N, IRP, JA, AS = mat
    A = AS if start == "valued" else np.ones(JA.size)
    B = np.random.default_rng(6).uniform(-2, 2, size=JA.size)
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
    try:
        X = _x(np.random.default_rng(7), (N, 8))
        _assert_bits(_spmm(api, dm, X, M), _expect(oracle, IRP, JA, A, X), "before")
        dm.update_values(B)
        assert api.lib.spmvHipUnitValue(C.byref(dm.handle), None) == 0
        _assert_bits(_spmm(api, dm, X, M), _expect(oracle, IRP, JA, B, X), "after")
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------- 7. agreement with SpMV
def test_agrees_with_spmv_launcher(api, mat):
    M, N, IRP, JA, AS = mat
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    try:
        X = _x(np.random.default_rng(8), (N, 8))
        dx, dy = api.DeviceVector(N), api.DeviceVector(M)

        def spmv(x):
            dx.up(x)
            dy.poison()
            api.spmv("hipSpMVRowsCSR", dm, dx, dy)
            return dy.down()
        y1 = _spmm(api, dm, X[:, :1], M)
        assert np.array_equal(y1[:, 0].view(np.uint64), spmv(X[:, 0]).view(np.uint64))
        Y = _spmm(api, dm, X, M)
        for c in range(8):
            assert np.array_equal(Y[:, c].view(np.uint64), spmv(np.ascontiguousarray(X[:, c])).view(np.uint64)), c
        dx.free()
        dy.free()
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------- 8. special values
def test_nan_inf_and_zero_x(api, oracle, mat):
    M, N, IRP, JA, AS = mat
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    try:
        rng = np.random.default_rng(9)
        X = _x(rng, (N, 8))
        X[rng.integers(0, N, size=40), rng.integers(0, 8, size=40)] = np.nan
        X[rng.integers(0, N, size=40), rng.integers(0, 8, size=40)] = np.inf
        X[rng.integers(0, N, size=40), rng.integers(0, 8, size=40)] = -np.inf
        Yref = _expect(oracle, IRP, JA, AS, X)
        assert np.isnan(Yref).any() and np.isinf(Yref).any()
        _assert_bits(_spmm(api, dm, X, M), Yref, "nan/inf", equal_nan=True)
        Z = np.zeros((N, 5))
        _assert_bits(_spmm(api, dm, Z, M), _expect(oracle, IRP, JA, AS, Z), "zero X")
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------- 9. streams and graphs
def test_capture_into_a_hip_graph(api, oracle, mat):
    """With spmvHipSetSync(0) the call only enqueues on the library stream: captured into a graph, nothing runs at
    capture; replayed after X got new contents, Y has the new product's bits."""
    torch = pytest.importorskip("torch")
    M, N, IRP, JA, AS = mat
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    rng = np.random.default_rng(10)
    X0, X1 = _x(rng, (N, 12)), _x(rng, (N, 12))
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            x = torch.from_numpy(X0).cuda()
            y = torch.full((M, 12), float("nan"), dtype=torch.float64, device="cuda")
            api.lib.spmvHipSetStream(C.c_void_p(stream.cuda_stream))
            api.lib.spmvHipSetSync(0)

            def call():
                assert api.lib.hipSpMMRowsCSR(C.byref(dm.handle), 12, x.data_ptr(), 12, ROW, y.data_ptr(), 12, ROW) == 0
            call()
            torch.cuda.synchronize()
            _assert_bits(y.cpu().numpy(), _expect(oracle, IRP, JA, AS, X0), "enqueued")
            y.fill_(float("nan"))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                call()
            torch.cuda.synchronize()
            assert bool(torch.isnan(y).all())                       # capture ran nothing
            x.copy_(torch.from_numpy(X1))
            graph.replay()
            torch.cuda.synchronize()
            _assert_bits(y.cpu().numpy(), _expect(oracle, IRP, JA, AS, X1), "replayed")
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        dm.free()


# ------------------------------------------------------------------------------------------------- 10. torch / numpy path
def test_matmul_torch_and_numpy(api, oracle, mat):
    torch = pytest.importorskip("torch")
    M, N, IRP, JA, AS = mat
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    try:
        X = _x(np.random.default_rng(11), (N, 6))
        Yref = _expect(oracle, IRP, JA, AS, X)
        xr = torch.from_numpy(X).cuda()                              # contiguous (N, k): row-major
        _assert_bits(dm.matmul(xr).cpu().numpy(), Yref, "contiguous")
        xc = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()  # .t() of a contiguous (k, N): column-major
        assert xc.stride() == (1, N)
        _assert_bits(dm.matmul(xc).cpu().numpy(), Yref, ".t() view")
        out = torch.full((6, M), float("nan"), dtype=torch.float64, device="cuda").t()
        assert dm.matmul(xr, out=out) is out
        _assert_bits(out.cpu().numpy(), Yref, "out, column-major")
        _assert_bits(dm.matmul(X), Yref, "numpy")
        with pytest.raises(api.SpmvHipError):
            dm.matmul(xr.float())
        with pytest.raises(api.SpmvHipError):
            dm.matmul(xr[:-1])
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------- 11. no leak
def test_no_device_memory_leak(api, mat):
    torch = pytest.importorskip("torch")
    M, N, IRP, JA, AS = mat
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
    try:
        x = torch.from_numpy(_x(np.random.default_rng(12), (N, 16))).cuda()
        y = torch.empty((M, 16), dtype=torch.float64, device="cuda")
        dm.matmul(x, out=y)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(50):
            dm.matmul(x, out=y)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0
    finally:
        dm.free()


# ------------------------------------------------------------------------------------------------- 12. refusals
def test_refusals_leave_y_untouched(api, mat):
    M, N, IRP, JA, AS = mat
    host = api.HostCSR(M, N, IRP, JA, AS)
    dm = api.spMatCpyCSR(host)
    k = 4
    hx = _x(np.random.default_rng(13), (N, k)).ravel()
    dx = api.DeviceBuffer(hx.nbytes).up(hx)
    hy = np.full(M * k, POISON)
    dy = api.DeviceBuffer(hy.nbytes).up(hy)
    big = api.DeviceBuffer(8 * (N * k + M * k))                 # X and Y inside one allocation
    big.up(np.full(N * k + M * k, POISON))
    ell = api.spMatCpyELL(host.to_ell())
    ell_dev = api.csr_to_ell_device(dm, True)
    freed = api.spMatCpyCSR(host)
    freed.free()
    H = C.byref(dm.handle)
    call = api.lib.hipSpMMRowsCSR
    cases = {
        "NULL handle": lambda: call(None, k, dx.ptr, k, ROW, dy.ptr, k, ROW),
        "freed handle": lambda: call(C.byref(freed.handle), k, dx.ptr, k, ROW, dy.ptr, k, ROW),
        "NULL X": lambda: call(H, k, None, k, ROW, dy.ptr, k, ROW),
        "NULL Y": lambda: call(H, k, dx.ptr, k, ROW, None, k, ROW),
        "ELL handle": lambda: call(C.byref(ell.handle), k, dx.ptr, k, ROW, dy.ptr, k, ROW),
        "ELL from CSR": lambda: call(C.byref(ell_dev.handle), k, dx.ptr, k, ROW, dy.ptr, k, ROW),
        "k = 0": lambda: call(H, 0, dx.ptr, k, ROW, dy.ptr, k, ROW),
        "X layout 2": lambda: call(H, k, dx.ptr, k, 2, dy.ptr, k, ROW),
        "Y layout -1": lambda: call(H, k, dx.ptr, k, ROW, dy.ptr, k, -1),
        "ldx < k": lambda: call(H, k, dx.ptr, k - 1, ROW, dy.ptr, k, ROW),
        "ldy < k": lambda: call(H, k, dx.ptr, k, ROW, dy.ptr, k - 1, ROW),
        "ldx < N": lambda: call(H, k, dx.ptr, N - 1, COL, dy.ptr, k, ROW),
        "ldy < M": lambda: call(H, k, dx.ptr, k, ROW, dy.ptr, M - 1, COL),
        "Y = X": lambda: call(H, k, dx.ptr, k, ROW, dx.ptr, k, ROW),
    }
    try:
        for name, fn in cases.items():
            assert fn() == 1, name
            assert np.array_equal(dy.down(np.float64).view(np.uint64), hy.view(np.uint64)), name
            assert np.array_equal(dx.down(np.float64), hx), name
        # overlapping ranges inside one allocation: Y starts in the last row of X, or X starts in the last row of Y
        base = big.ptr.value
        before = big.down(np.float64).view(np.uint64).copy()
        assert call(H, k, C.c_void_p(base), k, ROW, C.c_void_p(base + 8 * (N * k - 1)), k, ROW) == 1
        assert call(H, k, C.c_void_p(base + 8 * (M * k - 1)), k, ROW, C.c_void_p(base), k, ROW) == 1
        assert np.array_equal(big.down(np.float64).view(np.uint64), before)
        # ... and adjacent ranges are not an overlap
        assert call(H, k, C.c_void_p(base), k, ROW, C.c_void_p(base + 8 * N * k), k, ROW) == 0
    finally:
        for o in (dx, dy, big, ell, ell_dev, dm):
            o.free()


# ------------------------------------------------------------------------------------------------- 13. full size
def test_full_size_c2(api, oracle):
    """c2 (1 M rows, 32 M entries, generated on the device) at k = 8: every row of every column checked"""
    from spmv_openmp_cuda_amd import synth
    w = synth.WORKLOADS["c2"]
    irp = synth.prefix(synth.row_lengths(w))
    dm = synth.device_csr(w, irp, 0, w.N)
    try:
        ja = dm.buffers["JA"].down(np.uint32)
        as_ = dm.buffers["AS"].down(np.float64)
        irp32 = irp.astype(np.uint32)
        X = _x(np.random.default_rng(14), (w.N, 8))
        Y = _spmm(api, dm, X, w.N)
        for c in range(8):
            ref = oracle.csr_serial_dev(irp32, ja, as_, np.ascontiguousarray(X[:, c]))
            assert np.array_equal(Y[:, c].view(np.uint64), ref.view(np.uint64)), c
    finally:
        dm.free()
