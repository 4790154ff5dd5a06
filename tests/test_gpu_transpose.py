"""A^T of a device CSR handle (spmvHipCsrTranspose, DeviceMatrix.transpose) and its value refresh
(spmvHipTransposeRefresh, DeviceMatrix.refresh_from).

The transpose's arrays equal the test side's stable transpose (tests/transpose_ref.py) exactly, and every serial-order
candidate of hipSpMVRowsCSR on it gives the bits of the oracle on that transpose -- the serial scatter loop of A.  The
inputs of the product tests are order-sensitive with repeated columns (tests/serial_order_inputs.py), so an unstable
transpose would show (tests/test_transpose_abi.py shows that on the host)."""
import ctypes as C

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits
from conftest import random_csr
from test_oracle import NAMES, load_golden
from transpose_ref import stable_transpose

pytestmark = pytest.mark.gpu

ROWS = "hipSpMVRowsCSR"
IRP32_LIMIT = (1 << 32) - 65536


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.set_variant(ROWS, 2)
    api.lib.spmvHipSetUnitValues(1)
    api.lib.spmvHipSetStream(None)
    api.lib.spmvHipSetSync(1)


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


def _down(api, ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
    return out


def _arrays(api, dm):
    h = dm.handle
    return (_down(api, h.IRP, h.M + 1, np.uint32), _down(api, h.JA, h.NZ, np.uint32), _down(api, h.AS, h.NZ, np.float64))


def _assert_arrays(api, dmt, M, N, IRP, JA, AS, what):
    IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, AS)
    h = dmt.handle
    assert (h.M, h.N, h.NZ) == (N, M, JA.size), what
    irp, ja, a = _arrays(api, dmt)
    assert np.array_equal(irp, IRPt.astype(np.uint32)), f"{what}: IRP"
    assert np.array_equal(ja, JAt.astype(np.uint32)), f"{what}: JA"
    assert np.array_equal(a.view(np.uint64), ASt.view(np.uint64)), f"{what}: AS"


def _run(api, launcher, dm, x, M):
    dx, dy = api.DeviceVector(x.size).up(x), api.DeviceVector(M)
    try:
        dy.poison()
        api.spmv(launcher, dm, dx, dy)
        return dy.down()
    finally:
        dx.free()
        dy.free()


def _choice(api, dm):
    return (api.lib.spmvHipAutoChoiceRows(C.byref(dm.handle), None) or b"-").decode()


def _struct_bytes(dm):
    return C.string_at(C.addressof(dm.handle), C.sizeof(dm.handle))


# ------------------------------------------------------------------------------------------------- 1. arrays
def _empty_lines(rng):
    """empty rows (first, last) and empty columns (first, a run, the last)"""
    M, N = 300, 200
    lens = rng.integers(0, 9, M)
    lens[[0, 150, M - 1]] = 0
    rows = np.repeat(np.arange(M), lens)
    cols = rng.integers(1, N - 1, rows.size)
    cols[(cols > 50) & (cols < 90)] = 5
    o = np.lexsort((cols, rows))
    return (M, N) + si.assemble(M, rows[o], cols[o], si.order_values(rng, rows.size))


def _cases():
    rng = np.random.default_rng(1602)
    out = []
    for name in NAMES:
        g = load_golden(name)
        out.append((f"golden {name}", g["M"], g["N"], g["IRP"], g["JA"], g["AS"], 0))
    for M, N in ((3000, 500), (500, 3000)):
        out.append((f"random {M}x{N}",) + (M, N) + random_csr(rng, M, N, rng.integers(0, 30, M)) + (0,))
    out.append(("empty rows and columns",) + _empty_lines(rng) + (0,))
    M, N, IRP, JA, AS, _ = si.shuffled()
    out.append(("unsorted rows, repeated columns", M, N, IRP, JA, AS, 0))
    out.append(("unsorted rows, adopted, 8-byte IRP", M, N, IRP, JA, AS, 8))
    out.append(("pattern source", M, N, IRP, JA, np.full(JA.size, 1.0), 4))
    z = np.zeros(0, np.uint64)
    out.append(("M = 0", 0, 7, np.zeros(1, np.uint64), z, np.zeros(0), 0))
    out.append(("N = 0", 5, 0, np.zeros(6, np.uint64), z, np.zeros(0), 0))
    out.append(("NZ = 0", 5, 7, np.zeros(6, np.uint64), z, np.zeros(0), 0))
    return out


def test_arrays_equal_the_stable_transpose(api):
    for what, M, N, IRP, JA, AS, adopt in _cases():
        src = Source(api, M, N, IRP, JA, AS, adopt)
        try:
            t = src.dm.transpose()
            try:
                _assert_arrays(api, t, M, N, IRP, JA, AS, what)
                unit = api.lib.spmvHipUnitValue(C.byref(t.handle), None)
                assert unit == (1 if JA.size and np.all(AS.view(np.uint64) == AS[:1].view(np.uint64)) else 0), what
            finally:
                t.free()
        finally:
            src.free()


# ------------------------------------------------------------------------------------------------- 2-4. products
def _product_inputs(kind):
    if kind == "shuffled":
        M, N, IRP, JA, AS, _ = si.shuffled()
        return M, N, IRP, JA, AS
    inp = si.make("mixed")
    if kind == "unit":
        inp = si.unit(inp)
    return inp.M, inp.N, inp.IRP, inp.JA, inp.AS


def _check_serial(api, oracle, t, IRPt, JAt, ASt, xt, tag):
    y_ref = oracle.csr_serial(IRPt, JAt, ASt, xt)
    Mt = IRPt.size - 1

    def twice(launcher, what):
        y = _run(api, launcher, t, xt, Mt)
        assert_same_bits(y, y_ref, f"{tag}: {what}")
        assert_same_bits(_run(api, launcher, t, xt, Mt), y_ref, f"{tag}: {what}, second call")

    twice(ROWS, "hipSpMVRowsCSR variant 2")
    print(f"{tag}: variant 2 chose {_choice(api, t)}")
    api.set_variant(ROWS, 1)
    twice(ROWS, "hipSpMVRowsCSR variant 1")
    api.set_variant(ROWS, 2)
    api.build_tiles(t, deterministic=True)
    twice("hipSpMVTilesCSR", "two-phase deterministic")
    for form in (1, 2):
        api.build_stripes(t, deterministic=form)
        twice("hipSpMVStripesCSR", f"stripes deterministic {form}")
    return y_ref


def _assert_rounding(IRPt, JAt, ASt, xt, y_ref, y):
    """|y - y_ref| <= max(1e-13, len * 2^-52) * sum_j |a_ij x_j| in every row: 1e-13 is the parity tests' bound
    (conftest.tight_error), and a reordered sum of len products may be off by about len * eps, which only the long rows
    of these inputs reach (a row of 70 000 entries, all of one magnitude)"""
    prod = np.abs(ASt * xt[JAt.astype(np.int64)])
    lens = np.diff(IRPt.astype(np.int64))
    scale = np.add.reduceat(np.concatenate([prod, [0.0]]), np.minimum(IRPt[:-1].astype(np.int64), prod.size))
    bound = np.maximum(1e-13, lens * 2.0 ** -52) * np.where(lens > 0, scale, 0.0)
    bad = np.flatnonzero(~(np.abs(y - y_ref) <= bound))
    assert bad.size == 0, f"{bad.size} rows beyond rounding; row {bad[0]}: {y[bad[0]]!r} vs {y_ref[bad[0]]!r}, length {lens[bad[0]]}"


@pytest.mark.parametrize("kind,adopt", [("mixed", 0), ("mixed", 8), ("unit", 0), ("shuffled", 0)])
def test_products_have_the_scatter_loop_bits(api, oracle, kind, adopt):
    M, N, IRP, JA, AS = _product_inputs(kind)
    assert JA.size >= si.AUTO_MIN_NNZ
    IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, AS)
    xt = si.order_values(np.random.default_rng(7), M)
    src = Source(api, M, N, IRP, JA, AS, adopt)
    t = src.dm.transpose()
    try:
        y_ref = _check_serial(api, oracle, t, IRPt, JAt, ASt, xt, f"{kind}/adopt{adopt}")
        # 3. the reduction-order name: to rounding
        y = _run(api, "hipSpMVWarpPerRowCSR", t, xt, N)
        assert not np.isnan(y).any()
        _assert_rounding(IRPt, JAt, ASt, xt, y_ref, y)
        # 4. blocks: every column the bits of the serial product
        rng = np.random.default_rng(8)
        for k in (1, 4, 16):
            X = si.order_values(rng, M * k).reshape(M, k)
            Y = t.matmul(X)
            for c in range(k):
                assert_same_bits(Y[:, c], oracle.csr_serial(IRPt, JAt, ASt, np.ascontiguousarray(X[:, c])), f"{kind}: k={k}, column {c}")
    finally:
        t.free()
        src.free()


# ------------------------------------------------------------------------------------------------- 5. long rows of A^T
def test_a_column_longer_than_65536_entries(api, oracle):
    rng = np.random.default_rng(1605)
    M, N = 100_000, 3_000
    lens = rng.integers(1, 5, M)
    rows = np.repeat(np.arange(M), lens)
    cols = rng.integers(0, N, rows.size)
    first = np.r_[True, rows[1:] != rows[:-1]]
    cols[first & (rng.random(rows.size) < 0.75)] = 17              # ~75 000 rows hold column 17
    o = np.lexsort((cols, rows))
    IRP, JA, AS = si.assemble(M, rows[o], cols[o], si.order_values(rng, rows.size))
    assert np.count_nonzero(JA == 17) > 65_536
    src = Source(api, M, N, IRP, JA, AS)
    t = src.dm.transpose()
    try:
        _assert_arrays(api, t, M, N, IRP, JA, AS, "long row")
        IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, AS)
        _check_serial(api, oracle, t, IRPt, JAt, ASt, si.order_values(rng, M), "long row")
    finally:
        t.free()
        src.free()


# ------------------------------------------------------------------------------------------------- 6. double transpose
def test_double_transpose(api):
    rng = np.random.default_rng(1606)
    M, N = 2_000, 1_500
    IRP, JA, AS = random_csr(rng, M, N, rng.integers(0, 20, M))
    Ms, Ns, IRPs, JAs, ASs, _ = si.shuffled()
    for what, (m, n, irp, ja, a), expect in (("ascending rows", (M, N, IRP, JA, AS), None),
                                              ("unsorted rows", (Ms, Ns, IRPs, JAs, ASs), si.stable_rows_by(IRPs, JAs.astype(np.int64)))):
        src = Source(api, m, n, irp, ja, a)
        t = src.dm.transpose()
        tt = t.transpose()
        try:
            ja_e, a_e = (ja, a) if expect is None else (ja[expect], a[expect])
            got = _arrays(api, tt)
            assert (tt.handle.M, tt.handle.N, tt.handle.NZ) == (m, n, ja.size)
            assert np.array_equal(got[0], irp.astype(np.uint32)), what
            assert np.array_equal(got[1], ja_e.astype(np.uint32)), what
            assert np.array_equal(got[2].view(np.uint64), np.ascontiguousarray(a_e).view(np.uint64)), what
        finally:
            tt.free()
            t.free()
            src.free()


# ------------------------------------------------------------------------------------------------- 7. refresh
def _fresh_bits(api, src, xt, Mt):
    f = src.dm.transpose()
    try:
        return _run(api, ROWS, f, xt, Mt)
    finally:
        f.free()


def test_refresh_after_a_chain_of_updates(api, oracle):
    """host update, device update, ValuesChanged on the adopted array: after each refresh dAT's products (the selection's
    pick and the explicit deterministic forms) equal a fresh transpose's bits, the pick stays, the update is in place"""
    torch = pytest.importorskip("torch")
    inp = si.make("mixed")
    M, N, IRP, JA = inp.M, inp.N, inp.IRP, inp.JA
    rng = np.random.default_rng(1607)
    vals = [si.order_values(rng, JA.size) for _ in range(3)]
    xt = si.order_values(rng, M)
    src = Source(api, M, N, IRP, JA, inp.AS, adopt=4)
    t = src.dm.transpose()
    try:
        _run(api, ROWS, t, xt, N)
        pick = _choice(api, t)
        api.build_tiles(t, deterministic=True)
        api.build_stripes(t, deterministic=2)
        for step, v in enumerate(vals):
            if step == 0:
                src.dm.update_values(v)
            elif step == 1:
                src.dm.update_values(torch.from_numpy(v).cuda())
            else:
                src.bufs[2].up(v)
                src.dm.values_changed()
            t.refresh_from(src.dm)
            info = t.update_info()
            assert info.inPlace == 1 and info.rebuilt == 0, step
            IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, v)
            y_ref = oracle.csr_serial(IRPt, JAt, ASt, xt)
            assert_same_bits(_run(api, ROWS, t, xt, N), y_ref, f"step {step}: hipSpMVRowsCSR ({pick})")
            assert_same_bits(_fresh_bits(api, src, xt, N), y_ref, f"step {step}: fresh transpose")
            assert_same_bits(_run(api, "hipSpMVTilesCSR", t, xt, N), y_ref, f"step {step}: two-phase deterministic")
            assert_same_bits(_run(api, "hipSpMVStripesCSR", t, xt, N), y_ref, f"step {step}: stripes ordered tickets")
            assert _choice(api, t) == pick, step
            _assert_arrays(api, t, M, N, IRP, JA, v, f"step {step}")
    finally:
        t.free()
        src.free()


def test_refresh_unit_transitions(api, oracle):
    """ones -> random -> twos: dAT follows as spmvHipValuesChanged would (section 14 of DESIGN.md)"""
    inp = si.make("mixed")
    M, N, IRP, JA = inp.M, inp.N, inp.IRP, inp.JA
    rng = np.random.default_rng(1608)
    xt = si.order_values(rng, M)
    src = Source(api, M, N, IRP, JA, np.ones(JA.size))
    t = src.dm.transpose()
    try:
        assert api.lib.spmvHipUnitValue(C.byref(t.handle), None) == 1
        _run(api, ROWS, t, xt, N)
        prev = True
        for vals, unit in ((si.order_values(rng, JA.size), None), (np.full(JA.size, 2.0), 2.0)):
            src.dm.update_values(vals)
            t.refresh_from(src.dm)
            info = t.update_info()
            assert info.unitBefore == prev and info.unitAfter == (unit is not None)
            assert info.inPlace == (not prev)
            v = C.c_double(0)
            assert api.lib.spmvHipUnitValue(C.byref(t.handle), C.byref(v)) == (1 if unit is not None else 0)
            if unit is not None:
                assert v.value == unit
            IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, vals)
            assert_same_bits(_run(api, ROWS, t, xt, N), oracle.csr_serial(IRPt, JAt, ASt, xt), f"unit -> {unit}")
            prev = unit is not None
    finally:
        t.free()
        src.free()


# ------------------------------------------------------------------------------------------------- 8. graph
def test_captured_graph_replays_with_refreshed_values(api, oracle):
    torch = pytest.importorskip("torch")
    inp = si.make("mixed")
    M, N, IRP, JA, A = inp.M, inp.N, inp.IRP, inp.JA, inp.AS
    B = si.order_values(np.random.default_rng(1609), JA.size)
    xt_host = si.order_values(np.random.default_rng(1610), M)
    src = Source(api, M, N, IRP, JA, A)
    t = src.dm.transpose()
    stream = torch.cuda.Stream()
    cfg = api.CONFIG()
    try:
        with torch.cuda.stream(stream):
            x = torch.from_numpy(xt_host).cuda()
            y = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
            api.lib.spmvHipSetStream(C.c_void_p(stream.cuda_stream))
            assert api.lib.hipSpMVRowsCSR(C.byref(t.handle), x.data_ptr(), cfg, y.data_ptr()) == 0       # the selection
            torch.cuda.synchronize()
            api.lib.spmvHipSetSync(0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                assert api.lib.hipSpMVRowsCSR(C.byref(t.handle), x.data_ptr(), cfg, y.data_ptr()) == 0
            torch.cuda.synchronize()
            y.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, A)
            assert_same_bits(y.cpu().numpy(), oracle.csr_serial(IRPt, JAt, ASt, xt_host), "before the refresh")
            src.dm.update_values(B)
            t.refresh_from(src.dm)
            assert t.update_info().inPlace == 1
            y.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, B)
            assert_same_bits(y.cpu().numpy(), oracle.csr_serial(IRPt, JAt, ASt, xt_host), "replayed after the refresh")
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        t.free()
        src.free()


# ------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_leave_dat_untouched(api, oracle, capfd):
    rng = np.random.default_rng(1611)
    M, N = 4_000, 3_000
    IRP, JA, AS = random_csr(rng, M, N, rng.integers(0, 12, M))
    xt = si.order_values(rng, M)
    src = Source(api, M, N, IRP, JA, AS)
    t = src.dm.transpose()
    other = Source(api, M, N, IRP, JA, AS)
    keep = []
    try:
        before = _run(api, ROWS, t, xt, N)
        snap = _struct_bytes(t)
        lib, P = api.lib, C.byref

        def refused(call, msg=None):
            capfd.readouterr()
            assert call() != 0
            err = capfd.readouterr().err
            assert err, "no message"
            if msg:
                assert msg in err, err
            assert _struct_bytes(t) == snap

        refused(lambda: lib.spmvHipCsrTranspose(None, P(t.handle)))
        refused(lambda: lib.spmvHipCsrTranspose(P(src.dm.handle), None))
        refused(lambda: lib.spmvHipCsrTranspose(P(t.handle), P(t.handle)))
        ell = api.spMatCpyELL(api.HostCSR(M, N, IRP, JA, AS).to_ell())
        ell_dev = api.csr_to_ell_device(src.dm, True)
        keep += [ell, ell_dev]
        refused(lambda: lib.spmvHipCsrTranspose(P(ell.handle), P(t.handle)), "ELL")
        refused(lambda: lib.spmvHipCsrTranspose(P(ell_dev.handle), P(t.handle)), "ELL")
        # NZ at the 32-bit limit and N = 2^32 - 1: adopted with no value or column array (nothing is ever read)
        irp = api.DeviceBuffer(16)
        keep.append(irp)
        for (m, n, nz) in ((1, 4, IRP32_LIMIT), (1, (1 << 32) - 1, 0)):
            big = api.DeviceMatrix()
            h_irp = np.array([0, nz], dtype=np.uint64)
            assert lib.spmvHipAdoptCSR(P(big.handle), m, n, nz, irp.ptr, 8, None, None, h_irp.ctypes.data_as(C.c_void_p)) == 0
            keep.append(big)
            refused(lambda: lib.spmvHipCsrTranspose(P(big.handle), P(t.handle)), "NZ" if nz else "N=")
        # refresh: not a transpose, not its source (live, same shape), NULLs, a freed source, a new handle after it
        refused(lambda: lib.spmvHipTransposeRefresh(P(other.dm.handle), P(src.dm.handle)), "not made by")
        refused(lambda: lib.spmvHipTransposeRefresh(P(t.handle), P(other.dm.handle)), "not the handle")
        refused(lambda: lib.spmvHipTransposeRefresh(None, P(src.dm.handle)))
        refused(lambda: lib.spmvHipTransposeRefresh(P(t.handle), None))
        assert lib.spmvHipTransposeRefresh(P(t.handle), P(src.dm.handle)) == 0      # (the source itself is accepted)
        snap = _struct_bytes(t)
        src.free()
        refused(lambda: lib.spmvHipTransposeRefresh(P(t.handle), P(src.dm.handle)), "not a device handle")
        again = Source(api, M, N, IRP, JA, AS)
        keep.append(again)
        refused(lambda: lib.spmvHipTransposeRefresh(P(t.handle), P(again.dm.handle)), "not the handle")
        # dAT outlived its source and still computes what it did
        assert_same_bits(_run(api, ROWS, t, xt, N), before, "after the refusals")
    finally:
        t.free()
        src.free()
        other.free()
        for k in keep:
            k.free()


# ------------------------------------------------------------------------------------------------- 10. memory
def test_device_memory_comes_back(api):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1612)
    M, N = 200_000, 150_000
    IRP, JA, AS = random_csr(rng, M, N, rng.integers(0, 17, M))
    B = rng.uniform(-1, 1, JA.size)
    xt = si.order_values(rng, M)
    free = []
    for _ in range(20):
        src = Source(api, M, N, IRP, JA, AS)
        t = src.dm.transpose()
        src.dm.update_values(B)
        t.refresh_from(src.dm)
        _run(api, ROWS, t, xt, N)
        src.free()                                       # the source first: the transpose keeps no pointer to it
        t.free()
        api.spmvHipFinalize()
        api.spmvHipInit(0)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert min(free[2:]) >= free[1] - (8 << 20) and free[-1] >= free[1] - (8 << 20), free


# ------------------------------------------------------------------------------------------------- 11. full size
def test_full_size_c2(api, oracle):
    """c2 (1 M x 1 M, 32 M entries, generated on the device): the transposed product bit for bit on 2 000 sampled rows
    and the 8 longest; the torch and numpy paths of transpose() / refresh_from() / matmul()"""
    torch = pytest.importorskip("torch")
    from spmv_openmp_cuda_amd import synth
    w = synth.WORKLOADS["c2"]
    irp = synth.prefix(synth.row_lengths(w))
    dm = synth.device_csr(w, irp, 0, w.N)
    t = None
    try:
        ja = dm.buffers["JA"].down(np.uint32)
        as_ = dm.buffers["AS"].down(np.float64)
        M, N = w.N, w.N
        t = dm.transpose()
        rng = np.random.default_rng(1613)
        lens_t = np.bincount(ja, minlength=N)
        rows = np.unique(np.concatenate([rng.choice(N, 2000, replace=False), np.argsort(lens_t, kind="stable")[-8:]]))

        def check(values, what):
            IRPt, JAt, ASt, _ = stable_transpose(N, irp, ja, values)
            xt = si.order_values(rng, M)
            y_ref = oracle.csr_serial(IRPt, JAt, ASt, xt)
            y = t.matmul(torch.from_numpy(xt).cuda().reshape(M, 1)).cpu().numpy()[:, 0]      # torch path, k = 1
            assert_same_bits(y[rows], y_ref[rows], f"{what}: matmul (torch)")
            assert_same_bits(_run(api, ROWS, t, xt, N)[rows], y_ref[rows], f"{what}: hipSpMVRowsCSR ({_choice(api, t)})")
            X = np.stack([xt, xt[::-1]], axis=1)
            Y = t.matmul(X)                                                                 # numpy path
            assert_same_bits(Y[rows, 0], y_ref[rows], f"{what}: matmul (numpy)")

        check(as_, "c2")
        B = rng.uniform(-1, 1, as_.size)
        dm.update_values(torch.from_numpy(B).cuda())                                        # torch values on the device
        t.refresh_from(dm)
        check(B, "c2, refreshed (torch)")
        Cv = rng.uniform(-1, 1, as_.size)
        dm.update_values(Cv)                                                                # numpy values from the host
        t.refresh_from(dm)
        check(Cv, "c2, refreshed (numpy)")
    finally:
        if t is not None:
            t.free()
        dm.free()
