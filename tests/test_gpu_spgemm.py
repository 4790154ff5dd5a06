"""C = A B on the device (spmvHipSpGEMM, spmvHipSpGEMMRefresh): C's IRP, JA and AS are downloaded and compared with
tests/spgemm_ref.py -- indices exact, values as bits, NaN as NaN -- on every class of rows (wavefront, workgroup, sorted
path), at the class edges, under lowered and default options, on every kind of source handle, after a refresh; NZ, IRP[M] and
the array lengths are compared (C's arrays are the library's own, so nothing past their ends can be poisoned).  Every refusal leaves dC and info untouched."""
import ctypes as C

import numpy as np
import pytest

import serial_order_inputs as si
import spgemm_ref as sr
from bits import assert_same_bits

pytestmark = pytest.mark.gpu

ROWS = "hipSpMVRowsCSR"
LOWERED = dict(waveMaxProducts=64, groupMaxProducts=256)
ALL_SORTED = dict(waveMaxProducts=1, groupMaxProducts=1)
WAVE_SLOTS, WAVE_MAX, GROUP_MAX = 1024, 512, 6144


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


def _down(api, ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
    return out


def _up(api, A):
    return api.spMatCpyCSR(api.HostCSR(*A))


def _arrays(api, dm):
    h = dm.handle
    return (int(h.M), int(h.N), _down(api, h.IRP, h.M + 1, np.uint32), _down(api, h.JA, h.NZ, np.uint32), _down(api, h.AS, h.NZ, np.float64))


def _check(api, dc, R, what):
    """C against the reference, and its info against the reference's counts"""
    got = _arrays(api, dc)
    assert int(dc.handle.NZ) == R[3].size, f"{what}: NZ"
    sr.same_bits(got, R, what)
    return got


def _multiply_and_check(api, A, B, what, R=None, **opts):
    da, db = _up(api, A), _up(api, B)
    try:
        dc = da.multiply(db, **opts)
        try:
            R = sr.spgemm_ref(A, B) if R is None else R
            _check(api, dc, R, what)
            info = dc.spgemm_info()
            ub = sr.row_products(A, B)
            assert (info.products, info.nnzC) == (int(ub.sum()), R[3].size), what
            assert info.rowsWave + info.rowsGroup + info.rowsSorted == np.count_nonzero(ub), what
            assert info.maxRowProducts == (int(ub.max()) if ub.size else 0)
            assert info.maxRowNnz == (int(np.diff(R[2].astype(np.int64)).max()) if R[0] else 0)
            return info
        finally:
            dc.free()
    finally:
        da.free()
        db.free()


# ------------------------------------------------------------------------------------------------------- small shapes
def _empty(M, N):
    return M, N, np.zeros(M + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0)


@pytest.mark.parametrize("name", ["A.M=0", "A.N=0", "B.N=0", "rows empty", "B empty"])
def test_empty_shapes(api, name):
    rng = np.random.default_rng(2220)
    A, B = {"A.M=0": (_empty(0, 5), sr.random_csr(rng, 5, 4, 2)), "A.N=0": (_empty(6, 0), _empty(0, 4)),
            "B.N=0": (sr.random_csr(rng, 6, 5, 2), _empty(5, 0)), "rows empty": (_empty(6, 5), sr.random_csr(rng, 5, 4, 2)),
            "B empty": (sr.random_csr(rng, 6, 5, 2), _empty(5, 4))}[name]
    da, db = _up(api, A), _up(api, B)
    dc = da.multiply(db)
    try:
        M, N, irp, ja, a = _arrays(api, dc)
        assert (M, N, int(dc.handle.NZ), ja.size) == (A[0], B[1], 0, 0) and not irp.any()
        info = dc.spgemm_info()
        assert (info.nnzC, info.rowsWave, info.rowsGroup, info.rowsSorted) == (0, 0, 0, 0)
        if M and N:
            dx, dy = api.DeviceVector(N).up(np.ones(N)), api.DeviceVector(M)
            dy.poison()
            api.spmv(ROWS, dc, dx, dy)
            assert not dy.down().view(np.uint64).any(), "SpMV on an empty product gives +0.0"
            dx.free()
            dy.free()
    finally:
        for d in (dc, da, db):
            d.free()


CASES = sr.small_cases()
CASES["nan"] = sr.nan_case()


@pytest.mark.parametrize("opts", [{}, LOWERED, ALL_SORTED], ids=["default", "lowered", "sorted"])
@pytest.mark.parametrize("name", list(CASES))
def test_small_cases(api, name, opts):
    A, B = CASES[name]
    _multiply_and_check(api, A, B, name, **opts)


# --------------------------------------------------------------------------------------------------------- class edges
def _edge_pair(rng):
    """rows of exactly 63, 64, 65, 255, 256 and 257 products (B: one entry per row, 300 columns), some twice, among short
    random rows; the rows above 64 entries also take the wavefront form of the bound"""
    lens = np.array([63, 64, 65, 255, 256, 257, 0, 5, 64, 257, 1, 130], dtype=np.int64)
    A = sr.random_csr(rng, lens.size, 300, lens)
    B = sr.random_csr(rng, 300, 300, 1)
    return A, B, lens


def test_class_edges_and_equal_bits_under_every_option(api):
    A, B, lens = _edge_pair(np.random.default_rng(2221))
    R = sr.spgemm_ref(A, B)
    assert np.array_equal(sr.row_products(A, B), lens)
    low = _multiply_and_check(api, A, B, "lowered", R, **LOWERED)
    assert (low.rowsWave, low.rowsGroup, low.rowsSorted) == (np.count_nonzero((lens > 0) & (lens <= 64)),
                                                             np.count_nonzero((lens > 64) & (lens <= 256)), np.count_nonzero(lens > 256))
    dflt = _multiply_and_check(api, A, B, "default", R)
    assert (dflt.rowsWave, dflt.rowsGroup, dflt.rowsSorted) == (np.count_nonzero(lens), 0, 0)
    srt = _multiply_and_check(api, A, B, "sorted", R, **ALL_SORTED)
    assert (srt.rowsWave, srt.rowsGroup, srt.rowsSorted) == (np.count_nonzero(lens == 1), 0, np.count_nonzero(lens > 1))
    assert srt.sortBatches == 1 and srt.tempBytes > 0 and dflt.tempBytes > 0


# ------------------------------------------------------------------------------------------------------------- probing
def test_columns_that_are_multiples_of_the_table_size(api):
    rng = np.random.default_rng(2222)
    N = WAVE_SLOTS * 40
    B = sr.random_csr(rng, 50, N, rng.integers(1, 9, 50))
    B = B[:3] + ((B[3] // WAVE_SLOTS) * WAVE_SLOTS,) + B[4:]
    A = sr.random_csr(rng, 30, 50, rng.integers(0, 12, 30))
    info = _multiply_and_check(api, A, B, "multiples of 1024")
    assert info.rowsSorted == 0


def test_tables_filled_to_their_exact_limit(api):
    """B: 96 rows of 64 entries, its columns a permutation of 0 .. 6143.  Row 0 of A takes all 96 rows (6 144 distinct
    columns: the workgroup table at its limit), row 1 eight of them (512: the wavefront table at its limit), row 2 nine
    (576: the first workgroup row), row 3 all 96 and one again (6 208 products: the sorted path)"""
    rng = np.random.default_rng(2223)
    N = GROUP_MAX + 100
    cols = rng.permutation(GROUP_MAX)
    B = sr.csr(96, N, np.repeat(np.arange(96), 64), cols, si.order_values(rng, GROUP_MAX))
    take = [rng.permutation(96), rng.permutation(96)[:8], rng.permutation(96)[:9], np.append(rng.permutation(96), 5)]
    A = sr.csr(4, 96, np.repeat(np.arange(4), [t.size for t in take]), np.concatenate(take), si.order_values(rng, sum(t.size for t in take)))
    assert np.array_equal(sr.row_products(A, B), [GROUP_MAX, WAVE_MAX, WAVE_MAX + 64, GROUP_MAX + 64])
    info = _multiply_and_check(api, A, B, "full tables")
    assert (info.rowsWave, info.rowsGroup, info.rowsSorted) == (1, 2, 1)
    assert info.maxRowNnz == GROUP_MAX


def test_a_row_that_reaches_every_column_many_times(api):
    """30 rows of B with all 300 columns each, in random stored order: ub = 9 000, nnz = 300, class from min(ub, B.N)"""
    rng = np.random.default_rng(2224)
    B = sr.distinct_csr(rng, 40, 300, 300)
    A = sr.distinct_csr(rng, 3, 40, [30, 2, 40])
    info = _multiply_and_check(api, A, B, "dense rows")
    assert info.maxRowProducts == 12000 and info.maxRowNnz == 300 and info.rowsWave == 3


# --------------------------------------------------------------------------------------------------------- sorted path
def test_sorted_path_in_several_batches(api):
    rng = np.random.default_rng(2225)
    lens = np.full(40, 5, dtype=np.int64)
    lens[17] = 70                                                   # 700 products: above the budget of 600, a batch of its own
    A = sr.random_csr(rng, 40, 30, lens)
    B = sr.random_csr(rng, 30, 50, 10)
    assert int(sr.row_products(A, B).sum()) >= 2000
    info = _multiply_and_check(api, A, B, "batches", sortBudgetBytes=32 * 600, **ALL_SORTED)
    assert info.rowsSorted == 40 and info.sortBatches >= 4
    one = _multiply_and_check(api, A, B, "one batch", **ALL_SORTED)
    assert one.sortBatches == 1


# ----------------------------------------------------------------------------------------------------------- Laplacian
@pytest.fixture(scope="module")
def lap():
    A = sr.laplacian7(12, 10, 8, sr.integer_values)
    Av = A[:4] + (si.order_values(np.random.default_rng(2226), A[3].size),)
    return A, Av, sr.spgemm_ref(Av, Av)


def test_laplacian_squared_with_one_handle(api, lap):
    _, Av, R = lap
    da = _up(api, Av)
    dc = da.multiply(da)
    try:
        _check(api, dc, R, "A A")
        again = da.multiply(da, **LOWERED)
        assert all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) for u, v in zip(_arrays(api, dc)[2:], _arrays(api, again)[2:]))
        again.free()
    finally:
        dc.free()
        da.free()


def test_a_times_its_transpose_handle(api, lap):
    _, Av, _ = lap
    da = _up(api, Av)
    dt = da.transpose()
    dc = da.multiply(dt)
    try:
        _check(api, dc, sr.spgemm_ref(Av, sr.transpose(Av)), "A A^T")
    finally:
        for d in (dc, dt, da):
            d.free()


def test_galerkin_product_is_the_dense_one(api, lap):
    A, _, _ = lap
    P = sr.aggregation(12, 10, 8)
    da, dp = _up(api, A), _up(api, P)
    dpt = dp.transpose()
    dap = da.multiply(dp)
    dc = dpt.multiply(dap)                                          # a product handle as a source, and a unit-value one
    try:
        AP = sr.spgemm_ref(A, P)
        R = sr.spgemm_ref(sr.transpose(P), AP)
        got = _check(api, dc, R, "P^T (A P)")
        assert np.array_equal(sr.dense(got), sr.dense(P).T @ sr.dense(A) @ sr.dense(P))
        assert (got[0], got[1]) == (P[1], P[1])
    finally:
        for d in (dc, dap, dpt, dp, da):
            d.free()


# -------------------------------------------------------------------------------------------------------------- sources
def test_adopted_source_with_8_byte_row_pointers_and_a_unit_source(api):
    rng = np.random.default_rng(2227)
    A, B = CASES["mixed37x53x29"]
    ones = B[:4] + (np.full(B[3].size, -2.5),)
    bufs = [api.DeviceBuffer(8 * (A[0] + 1)).up(A[2].astype(np.uint64)), api.DeviceBuffer(4 * A[3].size).up(A[3].astype(np.uint32)),
            api.DeviceBuffer(8 * A[3].size).up(A[4])]
    da = api.DeviceMatrix()
    assert api.lib.spmvHipAdoptCSR(C.byref(da.handle), A[0], A[1], A[3].size, bufs[0].ptr, 8, bufs[1].ptr, bufs[2].ptr, None) == 0
    db = _up(api, ones)
    unit = C.c_double()
    assert api.lib.spmvHipUnitValue(C.byref(db.handle), C.byref(unit)) == 1 and unit.value == -2.5
    try:
        dc = da.multiply(db, **LOWERED)
        _check(api, dc, sr.spgemm_ref(A, ones), "adopted x unit")
        dc.free()
        dbt = db.transpose()
        sq = sr.random_csr(rng, 29, 37, 4)
        dsq = _up(api, sq)
        dc = dsq.multiply(da)                                       # the adopted handle on the right
        _check(api, dc, sr.spgemm_ref(sq, A), "x adopted")
        dc.free()
        dc = da.multiply(db).multiply(dbt)                          # (A B) B^T with the unit transpose on the right
        _check(api, dc, sr.spgemm_ref(sr.spgemm_ref(A, ones), sr.transpose(ones)), "(A B) B^T")
        dc.free()
        dbt.free()
        dsq.free()
    finally:
        da.free()
        db.free()
        for b in bufs:
            b.free()


# ----------------------------------------------------------------------------------------------------------- downstream
def test_downstream_spmv_ilu0_and_distance_2_colouring(api, oracle, lap):
    A, Av, R = lap
    da = _up(api, Av)
    dc = da.multiply(da)
    try:
        M, N, irp, ja, a = _arrays(api, dc)
        x = si.order_values(np.random.default_rng(2228), N)
        dx, dy = api.DeviceVector(N).up(x), api.DeviceVector(M)
        dy.poison()
        api.spmv(ROWS, dc, dx, dy)
        assert_same_bits(dy.down(), oracle.csr_serial(irp.astype(np.uint64), ja.astype(np.uint64), a, x), "SpMV on C")
        dx.free()
        dy.free()
        col = dc.colour(want_colours=True)
        colour = col.colours.down(np.uint32)
        col.free()
        # distance 2 in A: i and j share a neighbour, or are neighbours = (i, j) is in the pattern of A A (A has its diagonal)
        r = si.row_of_entry(irp)
        off = r != ja
        assert np.all(colour[r[off]] != colour[ja[off]]), "a proper colouring of A A is a distance-2 colouring of A"
        D = sr.dense(Av) != 0
        two = (D.astype(np.int64) @ D.astype(np.int64)) > 0
        np.fill_diagonal(two, False)
        ii, jj = np.nonzero(two)
        assert np.all(colour[ii] != colour[jj])
        info = dc.ilu0()
        assert info.zeroPivot < 0 and info.firstBadRow < 0
    finally:
        dc.free()
        da.free()


# -------------------------------------------------------------------------------------------------------------- refresh
def test_refresh_equals_a_fresh_product_and_a_graph_replays_it(api, oracle):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(2229)
    A, B, _ = _edge_pair(rng)
    A1 = A[:4] + (si.order_values(rng, A[3].size),)
    B1 = B[:4] + (si.order_values(rng, B[3].size),)
    da, db = _up(api, A), _up(api, B)
    dc = da.multiply(db, **LOWERED)
    x = si.order_values(rng, B[1])
    stream = torch.cuda.Stream()
    try:
        addr = (C.cast(dc.handle.IRP, C.c_void_p).value, C.cast(dc.handle.JA, C.c_void_p).value, C.cast(dc.handle.AS, C.c_void_p).value)
        with torch.cuda.stream(stream):
            tx = torch.from_numpy(x).cuda()
            ty = torch.full((A[0],), float("nan"), dtype=torch.float64, device="cuda")
            api.lib.spmvHipSetStream(C.c_void_p(stream.cuda_stream))
            api.lib.spmvHipSetSync(0)

            def call():
                assert api.lib.hipSpMVRowsCSR(C.byref(dc.handle), C.c_void_p(tx.data_ptr()), api.CONFIG(), C.c_void_p(ty.data_ptr())) == 0
            call()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                call()
            torch.cuda.synchronize()
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        for (An, Bn), what in (((A1, B), "A only"), ((A1, B1), "then B"), ((A, B1), "A back"), ((A1, B1), "both")):
            da.update_values(An[4])
            db.update_values(Bn[4])
            dc.multiply_refresh(da, db)
            R = sr.spgemm_ref(An, Bn)
            M, N, irp, ja, a = _check(api, dc, R, what)
            assert addr == (C.cast(dc.handle.IRP, C.c_void_p).value, C.cast(dc.handle.JA, C.c_void_p).value, C.cast(dc.handle.AS, C.c_void_p).value)
            info = dc.spgemm_info()
            assert info.symbolicMs == 0 and info.nnzC == R[3].size
            with torch.cuda.stream(stream):
                ty.fill_(float("nan"))
                graph.replay()
                torch.cuda.synchronize()
                assert_same_bits(ty.cpu().numpy(), oracle.csr_serial(R[2], R[3], R[4], x), f"replay after {what}")
        # refused: swapped sources, a foreign handle, a handle that is no product
        other = _up(api, A)
        before = _arrays(api, dc)[4].copy()
        for c, a_, b_ in ((dc, db, da), (dc, other, db), (dc, da, other), (da, da, db)):
            assert api.lib.spmvHipSpGEMMRefresh(C.byref(c.handle), C.byref(a_.handle), C.byref(b_.handle), None) == 1
        assert np.array_equal(_arrays(api, dc)[4].view(np.uint64), before.view(np.uint64))
        other.free()
        del graph
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        for d in (dc, da, db):
            d.free()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_dc_and_info_untouched(api, capfd):
    rng = np.random.default_rng(2230)
    A, B = CASES["mixed37x53x29"]
    da, db = _up(api, A), _up(api, B)
    ell = api.csr_to_ell_device(da, False)
    wide = _up(api, (2, (1 << 32) - 1, np.array([0, 1, 1], dtype=np.uint64), np.array([(1 << 32) - 2], dtype=np.uint64), np.ones(1)))
    two = _up(api, sr.random_csr(rng, 5, 2, 1))
    # an adopted A whose column ids are not checked at upload: one is >= B.M
    ja = A[3].astype(np.uint32)
    ja[7] = B[0]
    bufs = [api.DeviceBuffer(4 * (A[0] + 1)).up(A[2].astype(np.uint32)), api.DeviceBuffer(4 * ja.size).up(ja), api.DeviceBuffer(8 * ja.size).up(A[4])]
    bad = api.DeviceMatrix()
    assert api.lib.spmvHipAdoptCSR(C.byref(bad.handle), A[0], A[1], ja.size, bufs[0].ptr, 4, bufs[1].ptr, bufs[2].ptr, None) == 0
    out, info = api.spmat(), api.spmvSpgemmInfo()
    out.M, info.products = 12345, 777
    image = C.string_at(C.addressof(out), C.sizeof(out)), C.string_at(C.addressof(info), C.sizeof(info))
    dead = api.spmat()
    P = C.byref
    try:
        for a_, b_, c_ in ((None, P(db.handle), P(out)), (P(da.handle), None, P(out)), (P(da.handle), P(db.handle), None),
                           (P(dead), P(db.handle), P(out)), (P(da.handle), P(dead), P(out)),
                           (P(ell.handle), P(db.handle), P(out)), (P(two.handle), P(ell.handle), P(out)),
                           (P(db.handle), P(da.handle), P(out)),                      # 29 != 37
                           (P(two.handle), P(wide.handle), P(out)),                   # B.N = 2^32 - 1
                           (P(bad.handle), P(db.handle), P(out))):
            assert api.lib.spmvHipSpGEMM(a_, b_, None, c_, P(info)) == 1
            assert (C.string_at(C.addressof(out), C.sizeof(out)), C.string_at(C.addressof(info), C.sizeof(info))) == image
        for h, o in ((da, db), (db, da)):                          # dC == dA, dC == dB (shapes that would otherwise be fine: A A^T)
            dt = h.transpose()
            before = C.string_at(C.addressof(h.handle), C.sizeof(h.handle))
            assert api.lib.spmvHipSpGEMM(P(h.handle), P(dt.handle), None, P(h.handle), P(info)) == 1
            assert api.lib.spmvHipSpGEMM(P(dt.handle), P(h.handle), None, P(h.handle), P(info)) == 1
            assert C.string_at(C.addressof(h.handle), C.sizeof(h.handle)) == before
            dt.free()
        assert C.string_at(C.addressof(info), C.sizeof(info)) == image[1]
        err = capfd.readouterr().err
        for text in ("is NULL", "ELL handle", "A.N=29 != B.M=37", "32-bit row and column ids", "a column id of A is >= B.M", "dC is a source handle itself"):
            assert text in err, text
        dc = da.multiply(db)                                        # the sources are untouched by all of it
        _check(api, dc, sr.spgemm_ref(A, B), "after the refusals")
        dc.free()
    finally:
        for d in (bad, two, wide, ell, da, db):
            d.free()
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------- determinism, memory
def test_two_builds_give_equal_bits_and_the_words_past_the_ends_stay(api):
    """C's arrays are the library's own allocations, so the words past their ends cannot be poisoned from outside; what
    can be checked is that two builds agree in every byte and that NZ, IRP[M] and the array lengths agree"""
    A, B, _ = _edge_pair(np.random.default_rng(2231))
    da, db = _up(api, A), _up(api, B)
    try:
        got = []
        for _ in range(2):
            dc = da.multiply(db, **LOWERED)
            got.append(_arrays(api, dc))
            assert int(got[-1][2][-1]) == int(dc.handle.NZ) == got[-1][3].size
            dc.free()
        assert all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) for u, v in zip(got[0][2:], got[1][2:]))
    finally:
        da.free()
        db.free()


def test_device_memory_comes_back(api):
    import torch
    A = sr.laplacian7(24, 24, 16)
    free = []
    for _ in range(6):
        da = _up(api, A)
        dc = da.multiply(da)
        d2 = dc.multiply(da, **ALL_SORTED)
        dc.multiply_refresh(da, da)
        da.free()                                                   # the source first: a product keeps no pointer to it
        d2.free()
        dc.free()
        api.spmvHipFinalize()
        api.spmvHipInit(0)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert min(free[2:]) >= free[1] - (8 << 20) and free[-1] >= free[1] - (8 << 20), free
