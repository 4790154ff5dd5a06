"""C = alpha A + beta B on the device (spmvHipCsrAdd, spmvHipCsrAddRefresh): C's IRP, JA and AS are downloaded and compared
with tests/add_ref.py -- indices exact, values as bits, NaN as NaN -- on every class of rows (lane, wavefront, sorted path),
at the class edges, under default, lowered and all-sorted options, on every kind of source handle, after a refresh; NZ,
IRP[M] and the array lengths are compared (C's arrays are the library's own, so nothing past their ends can be poisoned).
Every refusal leaves dC and info untouched."""
import ctypes as C

import numpy as np
import pytest

import add_ref as ar
import serial_order_inputs as si
import spgemm_ref as sr
from bits import assert_same_bits

pytestmark = pytest.mark.gpu

ROWS = "hipSpMVRowsCSR"
LANE_MAX, WAVE_MAX = 32, 2048                                       # the built-in defaults
LOWERED = dict(laneMaxTerms=4, waveMaxTerms=70)
ALL_SORTED = dict(allSorted=True)
SETTINGS = {"default": {}, "lowered": LOWERED, "sorted": ALL_SORTED}


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


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


def _addresses(dm):
    return tuple(C.cast(p, C.c_void_p).value for p in (dm.handle.IRP, dm.handle.JA, dm.handle.AS))


def _check(api, dc, R, what):
    got = _arrays(api, dc)
    assert int(dc.handle.NZ) == R[3].size == got[3].size == got[4].size, f"{what}: NZ"
    assert int(got[2][-1]) == R[3].size, f"{what}: IRP[M]"
    ar.same_bits(got, R, what)
    return got


def _expected_classes(A, B, opts):
    return ar.classes(A, B, laneMax=opts.get("laneMaxTerms", LANE_MAX), waveMax=opts.get("waveMaxTerms", WAVE_MAX),
                      allSorted=opts.get("allSorted", False))


def _check_info(info, A, B, R, opts, what):
    t = ar.row_terms(A, B)
    assert (info.terms, info.nnzC) == (int(t.sum()), R[3].size), what
    assert (info.rowsLane, info.rowsWave, info.rowsSorted) == _expected_classes(A, B, opts), what
    assert info.rowsLane + info.rowsWave + info.rowsSorted == np.count_nonzero(t), what
    assert info.maxRowTerms == (int(t.max()) if t.size else 0), what
    assert info.maxRowNnz == (int(np.diff(R[2].astype(np.int64)).max()) if R[0] else 0), what


def _add_and_check(api, alpha, A, beta, B, what, R=None, **opts):
    da, db = _up(api, A), _up(api, B)
    try:
        dc = da.add(db, alpha, beta, **opts)
        try:
            R = ar.add_ref(alpha, A, beta, B) if R is None else R
            _check(api, dc, R, what)
            info = dc.add_info()
            _check_info(info, A, B, R, opts, what)
            return info
        finally:
            dc.free()
    finally:
        da.free()
        db.free()


# ------------------------------------------------------------------------------------------------------- small shapes
def _empty(M, N):
    return M, N, np.zeros(M + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0)


@pytest.mark.parametrize("name", ["M=0", "N=0", "both empty", "A empty", "B empty"])
def test_empty_shapes(api, oracle, name):
    rng = np.random.default_rng(2520)
    A, B = {"M=0": (_empty(0, 5), _empty(0, 5)), "N=0": (_empty(6, 0), _empty(6, 0)), "both empty": (_empty(6, 5), _empty(6, 5)),
            "A empty": (_empty(6, 5), sr.random_csr(rng, 6, 5, 3)), "B empty": (sr.random_csr(rng, 6, 5, 3), _empty(6, 5))}[name]
    da, db = _up(api, A), _up(api, B)
    dc = da.add(db, 2.0, -3.0)
    try:
        R = ar.add_ref(2.0, A, -3.0, B)
        M, N, irp, ja, a = _check(api, dc, R, name)
        info = dc.add_info()
        _check_info(info, A, B, R, {}, name)
        if not R[3].size:
            assert (info.nnzC, info.rowsLane, info.rowsWave, info.rowsSorted, info.sortBatches) == (0, 0, 0, 0, 0) and not irp.any()
        if M and N:
            x = si.order_values(rng, N)
            dx, dy = api.DeviceVector(N).up(x), api.DeviceVector(M)
            dy.poison()
            api.spmv(ROWS, dc, dx, dy)
            assert_same_bits(dy.down(), oracle.csr_serial(R[2], R[3], R[4], x) if R[3].size else np.zeros(M), "SpMV on C")
            dx.free()
            dy.free()
    finally:
        for d in (dc, da, db):
            d.free()


CASES = ar.small_cases()
CASES["nan"] = ar.nan_case()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", list(CASES))
def test_small_cases(api, name, setting):
    """1 x 1, unsorted rows and repeats in both (37 x 53), the plain rows of at most 12 entries in every relative position,
    +-Inf / -0.0 alone / +0.0 / -Inf + Inf, alpha = 0 against an Inf, A + (-1) A, NaN inputs"""
    alpha, A, beta, B = CASES[name]
    _add_and_check(api, alpha, A, beta, B, f"{name} ({setting})", **SETTINGS[setting])


def test_special_places(api):
    da, db = _up(api, CASES["special"][1]), _up(api, CASES["special"][3])
    dc = da.add(db)
    zero = da.add(db, 0.0, 2.0)
    try:
        a = _arrays(api, dc)
        assert (int(a[3][0]), int(a[4].view(np.uint64)[0])) == (0, 0), "a -0.0 alone in its column gives +0.0"
        z = _arrays(api, zero)
        assert np.array_equal(z[3], a[3]) and np.isnan(z[4]).any(), "alpha = 0 keeps A's pattern; 0 * Inf is a NaN at its place"
        A = CASES["cancel"][1]
        dA = _up(api, A)
        dz = dA.add(dA, 1.0, -1.0)
        got = _arrays(api, dz)
        assert got[3].size == np.unique(si.row_of_entry(A[2]) * A[1] + A[3].astype(np.int64)).size
        T = ar.sorted_csr(np.random.default_rng(2521), 30, 50, 9)
        dT = _up(api, T)
        dzz = dT.add(dT, 1.0, -1.0)
        gz = _arrays(api, dzz)
        assert gz[3].size == T[3].size and not gz[4].view(np.uint64).any(), "sums that cancel are stored, as +0.0"
        for d in (dzz, dT, dz, dA):
            d.free()
    finally:
        for d in (zero, dc, da, db):
            d.free()


@pytest.mark.parametrize("alpha,beta", [(1.0, -1.0), (-1.0, 0.0), (0.0, 1.0), (2.0 / 3.0, 1e300), (1e300, 2.0 / 3.0), (1e300, 1e300), (0.0, 0.0)])
def test_scalars(api, alpha, beta):
    rng = np.random.default_rng(2522)
    A, B = ar.mixed_37x53(rng)
    P, Q = ar.plain_rows(rng)
    _add_and_check(api, alpha, A, beta, B, "repeats")
    _add_and_check(api, alpha, P, beta, Q, "plain")
    _add_and_check(api, alpha, P, beta, Q, "plain, wave", laneMaxTerms=1)


# --------------------------------------------------------------------------------------------------------- class edges
EDGE_TERMS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 69, 70, 71, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 0, 3, 4, 5]


def _edge_pair(rng, N=1500):
    """plain rows of exactly EDGE_TERMS terms, split between A and B (a row of one term has it in B), columns that partly meet"""
    t = np.array(EDGE_TERMS, dtype=np.int64)
    la = t // 2
    A = ar.sorted_csr(rng, t.size, N, la)
    B = ar.sorted_csr(rng, t.size, N, t - la)
    return A, B, t


@pytest.fixture(scope="module")
def edges():
    A, B, t = _edge_pair(np.random.default_rng(2523))
    return A, B, t, ar.add_ref(1.25, A, -0.75, B)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_class_edges_and_equal_bits_under_every_option(api, edges, setting):
    A, B, t, R = edges
    assert np.array_equal(ar.row_terms(A, B), t) and ar.row_plain(A).all() and ar.row_plain(B).all()
    info = _add_and_check(api, 1.25, A, -0.75, B, setting, R, **SETTINGS[setting])
    live = t > 0
    want = {"default": (np.count_nonzero(live & (t <= 32)), np.count_nonzero((t > 32) & (t <= WAVE_MAX)), np.count_nonzero(t > WAVE_MAX)),
            "lowered": (np.count_nonzero(live & (t <= 4)), np.count_nonzero((t > 4) & (t <= 70)), np.count_nonzero(t > 70)),
            "sorted": (0, 0, np.count_nonzero(live))}[setting]
    assert (info.rowsLane, info.rowsWave, info.rowsSorted) == want
    assert info.tempBytes > 0 and info.sortBatches == (1 if want[2] else 0)


def test_limits_above_the_built_in_ones_are_clamped(api, edges):
    A, B, t, R = edges
    info = _add_and_check(api, 1.25, A, -0.75, B, "clamped", R, laneMaxTerms=64, waveMaxTerms=WAVE_MAX)
    da, db = _up(api, A), _up(api, B)
    dc = da.add(db, 1.25, -0.75, laneMaxTerms=1 << 20, waveMaxTerms=1 << 40)
    try:
        _check(api, dc, R, "clamped")
        got = dc.add_info()
        assert (got.rowsLane, got.rowsWave, got.rowsSorted) == (info.rowsLane, info.rowsWave, info.rowsSorted)
        assert got.rowsLane == np.count_nonzero((t > 0) & (t <= 64)) and got.rowsSorted == np.count_nonzero(t > WAVE_MAX)
    finally:
        for d in (dc, da, db):
            d.free()


def test_rows_that_are_not_plain_only_at_their_end(api):
    """65 entries: the last two columns equal, and the last column below the one before it -- found by the wavefront form of
    the first pass; the same two ends at 9 entries -- found by its lane form; under the lowered limits a row that is plain
    in A and not in B"""
    rng = np.random.default_rng(2524)
    N = 400
    asc65, asc9 = np.sort(rng.choice(N - 1, 65, replace=False)) + 1, np.sort(rng.choice(N - 1, 9, replace=False)) + 1
    rep65, dsc65, rep9, dsc9 = asc65.copy(), asc65.copy(), asc9.copy(), asc9.copy()
    rep65[-1], rep9[-1] = rep65[-2], rep9[-2]
    dsc65[-1], dsc9[-1] = dsc65[-2] - 1, 0
    plain = [np.sort(rng.choice(N, 7, replace=False)) for _ in range(6)]
    A = ar.from_rows(N, [rep65, dsc65, rep9, dsc9, asc65, asc9], rng)
    B = ar.from_rows(N, plain, rng)
    for (X, Y), what in (((A, B), "not plain in A"), ((B, A), "not plain in B")):
        for setting, opts in SETTINGS.items():
            info = _add_and_check(api, 1.0, X, -2.0, Y, f"{what} ({setting})", **opts)
            if setting == "default":
                assert (info.rowsLane, info.rowsWave, info.rowsSorted) == (1, 1, 4), what
            if setting == "lowered":
                assert (info.rowsLane, info.rowsWave, info.rowsSorted) == (0, 1, 5), what


# --------------------------------------------------------------------------------------------------------- sorted path
def test_sorted_path_in_several_batches(api):
    rng = np.random.default_rng(2525)
    lens = np.full(40, 20, dtype=np.int64)
    lens[17] = 660                                                  # 700 terms: above the budget of 600, a batch of its own
    A = sr.random_csr(rng, 40, 90, lens)
    B = sr.random_csr(rng, 40, 90, 40)
    assert int(ar.row_terms(A, B).sum()) >= 2400
    info = _add_and_check(api, 1.0, A, 1.0, B, "batches", sortBudgetBytes=32 * 600, **ALL_SORTED)
    assert info.rowsSorted == 40 and info.sortBatches >= 4
    mixed = _add_and_check(api, 1.0, A, 1.0, B, "batches of the unsorted rows", sortBudgetBytes=32 * 600)
    assert mixed.rowsSorted >= 30 and mixed.sortBatches >= 3
    one = _add_and_check(api, 1.0, A, 1.0, B, "one batch", **ALL_SORTED)
    assert one.sortBatches == 1


# ----------------------------------------------------------------------------------------------------------- Laplacian
@pytest.fixture(scope="module")
def lap():
    A = sr.laplacian7(12, 10, 8)
    Av = A[:4] + (si.order_values(np.random.default_rng(2526), A[3].size),)
    return A, Av


def test_one_handle_twice_and_a_plus_its_transpose_handle(api, lap):
    _, Av = lap
    da = _up(api, Av)
    dt = da.transpose()
    try:
        dc = da.add(da, 0.5, 0.25)
        _check(api, dc, ar.add_ref(0.5, Av, 0.25, Av), "dA == dB")
        dc.free()
        for opts in SETTINGS.values():
            dc = da.add(dt, **opts)
            got = _check(api, dc, ar.add_ref(1.0, Av, 1.0, sr.transpose(Av)), "A + A^T")
            D = np.zeros((got[0], got[1]), dtype=np.uint64)
            P = np.zeros((got[0], got[1]), dtype=bool)
            r = si.row_of_entry(got[2])
            D[r, got[3]] = got[4].view(np.uint64)
            P[r, got[3]] = True
            assert np.array_equal(P, P.T) and np.array_equal(D, D.T), "pattern and bits are symmetric"
            dc.free()
    finally:
        dt.free()
        da.free()


def test_product_sum_adopted_and_unit_sources(api):
    rng = np.random.default_rng(2527)
    _, A, _, B = CASES["mixed37x53"]
    sq = sr.random_csr(rng, 37, 37, 4)
    ones = B[:4] + (np.full(B[3].size, -2.5),)
    bufs = [api.DeviceBuffer(8 * (A[0] + 1)).up(A[2].astype(np.uint64)), api.DeviceBuffer(4 * A[3].size).up(A[3].astype(np.uint32)),
            api.DeviceBuffer(8 * A[3].size).up(A[4])]
    dad = api.DeviceMatrix()
    assert api.lib.spmvHipAdoptCSR(C.byref(dad.handle), A[0], A[1], A[3].size, bufs[0].ptr, 8, bufs[1].ptr, bufs[2].ptr, None) == 0
    dsq, db, du = _up(api, sq), _up(api, B), _up(api, ones)
    unit = C.c_double()
    assert api.lib.spmvHipUnitValue(C.byref(du.handle), C.byref(unit)) == 1 and unit.value == -2.5
    dprod = dsq.multiply(db)                                        # 37 x 53, ascending rows
    try:
        prod = sr.spgemm_ref(sq, B)
        dsum = dprod.add(dad, 2.0, -1.0)                            # a product handle and an adopted one (8-byte row pointers)
        S = ar.add_ref(2.0, prod, -1.0, A)
        _check(api, dsum, S, "2 (Q B) - A")
        dc = dad.add(dsum, 1.0, 1.0, **LOWERED)                     # the adopted handle on the left, a sum handle on the right
        _check(api, dc, ar.add_ref(1.0, A, 1.0, S), "A + (2 (Q B) - A)")
        dc.free()
        dc = dsum.add(du, -1.0, 3.0)                                # a sum handle on the left, a unit-value handle on the right
        _check(api, dc, ar.add_ref(-1.0, S, 3.0, ones), "-(...) + 3 U")
        dc.free()
        dc = du.add(du, 1.0, 1.0)                                   # unit + unit: C is a unit-value handle itself
        _check(api, dc, ar.add_ref(1.0, ones, 1.0, ones), "U + U")
        dc.free()
        dsum.free()
    finally:
        for d in (dprod, du, db, dsq, dad):
            d.free()
        for b in bufs:
            b.free()


# ----------------------------------------------------------------------------------------------------------- downstream
def test_downstream_spmv_ilu0_and_cg_on_a_shifted_matrix(api, oracle, lap):
    A, _ = lap
    M = A[0]
    sigma = -0.5                                                    # A - sigma I = A + I / 2: symmetric positive definite
    da, di = _up(api, A), _up(api, ar.identity(M))
    dc = da.add(di, 1.0, -sigma)
    try:
        R = ar.add_ref(1.0, A, -sigma, ar.identity(M))
        _, N, irp, ja, a = _check(api, dc, R, "A - sigma I")
        assert np.array_equal(sr.dense(R), sr.dense(A) + 0.5 * np.eye(M))
        rng = np.random.default_rng(2528)
        x = si.order_values(rng, N)
        dx, dy = api.DeviceVector(N).up(x), api.DeviceVector(M)
        dy.poison()
        api.spmv(ROWS, dc, dx, dy)
        assert_same_bits(dy.down(), oracle.csr_serial(irp.astype(np.uint64), ja.astype(np.uint64), a, x), "SpMV on C")
        dx.free()
        dy.free()
        b = rng.standard_normal(M)
        sol, kinfo = dc.cg(b, tol=1e-10, maxiter=500)
        assert kinfo.iterations > 0 and np.allclose(sr.dense(R) @ sol, b, atol=1e-6)
        info = dc.ilu0()                                            # (in place: last)
        assert info.zeroPivot < 0 and info.firstBadRow < 0
    finally:
        for d in (dc, di, da):
            d.free()


def test_smoothed_prolongator_through_public_calls(api, lap):
    A, _ = lap
    T = sr.aggregation(12, 10, 8)
    omega = 2.0 / 3.0
    Dinv = ar.identity(A[0])[:4] + (1.0 / ar.diagonal(A),)
    da, dt, dd = _up(api, A), _up(api, T), _up(api, Dinv)
    dat = da.multiply(dt)
    ddat = dd.multiply(dat)
    dp = dt.add(ddat, 1.0, -omega)
    try:
        R = ar.smoothed_prolongator(A, T, omega)
        got = _check(api, dp, R, "T - omega D^-1 A T")
        dA, dT = sr.dense(A), sr.dense(T)
        assert np.allclose(sr.dense(got), dT - omega * (np.diag(1.0 / np.diag(dA)) @ dA @ dT))
        assert dp.add_info().rowsSorted == 0
    finally:
        for d in (dp, ddat, dat, dd, dt, da):
            d.free()


# -------------------------------------------------------------------------------------------------------------- refresh
def test_refresh_equals_a_fresh_sum(api, oracle, edges):
    rng = np.random.default_rng(2529)
    A, B, _, _ = edges
    extra = ar.mixed_37x53(rng)                                     # rows with repeats below the plain ones
    A, B = _stack(A, extra[0]), _stack(B, extra[1])
    A1 = A[:4] + (si.order_values(rng, A[3].size),)
    B1 = B[:4] + (si.order_values(rng, B[3].size),)
    da, db = _up(api, A), _up(api, B)
    dc = da.add(db, 1.0, 1.0, **LOWERED)
    x = si.order_values(rng, A[1])
    dx, dy = api.DeviceVector(A[1]).up(x), api.DeviceVector(A[0])
    try:
        first = dc.add_info()
        assert first.rowsLane and first.rowsWave and first.rowsSorted
        addr = _addresses(dc)
        for (alpha, An, beta, Bn), what in (((1.0, A1, 1.0, B), "A only"), ((1.0, A1, 1.0, B1), "then B"), ((1.0, A, 1.0, B1), "A back"),
                                            ((1.0, A1, 1.0, B1), "both"), ((-0.5, A1, 3.0, B1), "alpha and beta"), ((1.0, A1, 0.0, B1), "beta = 0")):
            da.update_values(An[4])
            db.update_values(Bn[4])
            dc.add_refresh(da, db, alpha, beta)
            R = ar.add_ref(alpha, An, beta, Bn)
            _, _, irp, ja, a = _check(api, dc, R, what)
            assert addr == _addresses(dc), what
            info = dc.add_info()
            assert info.symbolicMs == 0 and info.nnzC == R[3].size
            assert (info.rowsLane, info.rowsWave, info.rowsSorted) == (first.rowsLane, first.rowsWave, first.rowsSorted)
            dy.poison()
            api.spmv(ROWS, dc, dx, dy)
            assert_same_bits(dy.down(), oracle.csr_serial(R[2], R[3], R[4], x), f"SpMV after {what}")
    finally:
        for d in (dx, dy, dc, da, db):
            d.free()


def _stack(X, Y):
    """Y's rows below X's, Y's columns kept"""
    assert Y[1] <= X[1]
    return (X[0] + Y[0], X[1], np.concatenate([X[2], Y[2][1:] + X[2][-1]]), np.concatenate([X[3], Y[3]]), np.concatenate([X[4], Y[4]]))


def test_refresh_refusals(api, capfd):
    _, A, _, B = CASES["mixed37x53"]
    sq = sr.random_csr(np.random.default_rng(2530), 37, 37, 3)
    da, db, other, dsq = _up(api, A), _up(api, B), _up(api, A), _up(api, sq)
    dc = da.add(db, 2.0, 3.0)
    dprod = dsq.multiply(da)
    info = api.spmvAddInfo()
    info.terms = 777
    image = C.string_at(C.addressof(info), C.sizeof(info))
    P = C.byref
    try:
        before = _arrays(api, dc)[4].copy()
        capfd.readouterr()
        for c, a_, b_ in ((dc, db, da), (dc, other, db), (dc, da, other), (dprod, dsq, da), (da, da, db)):
            assert api.lib.spmvHipCsrAddRefresh(P(c.handle), 2.0, P(a_.handle), 3.0, P(b_.handle), P(info)) == 1
            assert C.string_at(C.addressof(info), C.sizeof(info)) == image
        assert api.lib.spmvHipCsrAddRefresh(None, 2.0, P(da.handle), 3.0, P(db.handle), P(info)) == 1
        err = capfd.readouterr().err
        assert err.count("spmvHipCsrAddRefresh: ") == 6, err
        assert err.count("alpha with the first") == 3 and err.count("dC was not made by spmvHipCsrAdd") == 2 and "dC is NULL" in err, err
        assert np.array_equal(_arrays(api, dc)[4].view(np.uint64), before.view(np.uint64))
        dc.add_refresh(da, db, 2.0, 3.0)                            # the pair itself is taken
        _check(api, dc, ar.add_ref(2.0, A, 3.0, B), "after the refusals")
    finally:
        for d in (dprod, dc, dsq, other, da, db):
            d.free()


def test_a_sum_handle_in_other_refreshes_and_an_update_of_its_values(api, capfd):
    rng = np.random.default_rng(2531)
    sq = sr.random_csr(rng, 30, 30, 4)
    da = _up(api, sq)
    ds = da.add(da, 1.0, 2.0)
    P = C.byref
    try:
        capfd.readouterr()
        assert api.lib.spmvHipTransposeRefresh(P(ds.handle), P(da.handle)) == 1
        assert api.lib.spmvHipPermuteRefresh(P(ds.handle), P(da.handle)) == 1
        assert api.lib.spmvHipSpGEMMRefresh(P(ds.handle), P(da.handle), P(da.handle), None) == 1
        err = capfd.readouterr().err
        for maker in ("spmvHipCsrTranspose", "spmvHipCsrPermute", "spmvHipSpGEMM"):
            assert f"was not made by {maker}" in err, err
        R = ar.add_ref(1.0, sq, 2.0, sq)
        _check(api, ds, R, "untouched by the refused refreshes")
        new = si.order_values(rng, R[3].size)
        ds.update_values(new)                                       # spmvHipUpdateValues on a sum handle
        _check(api, ds, R[:4] + (new,), "updated values")
        x = si.order_values(rng, 30)
        dx, dy = api.DeviceVector(30).up(x), api.DeviceVector(30)
        dy.poison()
        api.spmv(ROWS, ds, dx, dy)
        want = np.zeros(30)
        for i in range(30):
            acc = np.float64(0.0)
            for p in range(int(R[2][i]), int(R[2][i + 1])):
                acc = acc + new[p] * x[int(R[3][p])]
            want[i] = acc
        assert_same_bits(dy.down(), want, "SpMV sees the updated values")
        dx.free()
        dy.free()
        dt = ds.transpose()                                         # ... and a sum handle is a source like any other
        _check(api, dt, sr.transpose(R[:4] + (new,)), "transpose of a sum")
        dt.free()
    finally:
        ds.free()
        da.free()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_dc_and_info_untouched(api, capfd):
    rng = np.random.default_rng(2532)
    _, A, _, B = CASES["mixed37x53"]
    da, db = _up(api, A), _up(api, B)
    ell = api.csr_to_ell_device(da, False)
    rows38 = _up(api, sr.random_csr(rng, 38, 53, 2))
    cols54 = _up(api, sr.random_csr(rng, 37, 54, 2))
    wide = _up(api, (2, (1 << 32) - 1, np.array([0, 1, 1], dtype=np.uint64), np.array([(1 << 32) - 2], dtype=np.uint64), np.ones(1)))
    lapl = _up(api, sr.laplacian7(6, 5, 4))
    hier = lapl.amg()
    # adopted arrays are not checked at upload: a column id >= N, and a handle with entries and no column array
    ja = A[3].astype(np.uint32)
    ja[7] = A[1]
    bufs = [api.DeviceBuffer(4 * (A[0] + 1)).up(A[2].astype(np.uint32)), api.DeviceBuffer(4 * ja.size).up(ja), api.DeviceBuffer(8 * ja.size).up(A[4])]
    bad, bare = api.DeviceMatrix(), api.DeviceMatrix()
    assert api.lib.spmvHipAdoptCSR(C.byref(bad.handle), A[0], A[1], ja.size, bufs[0].ptr, 4, bufs[1].ptr, bufs[2].ptr, None) == 0
    assert api.lib.spmvHipAdoptCSR(C.byref(bare.handle), A[0], A[1], ja.size, bufs[0].ptr, 4, None, bufs[2].ptr, None) == 0
    out, info = api.spmat(), api.spmvAddInfo()
    out.M, info.terms = 12345, 777
    image = C.string_at(C.addressof(out), C.sizeof(out)), C.string_at(C.addressof(info), C.sizeof(info))
    dead = api.spmat()
    P = C.byref
    try:
        capfd.readouterr()
        calls = ((None, P(db.handle), P(out)), (P(da.handle), None, P(out)), (P(da.handle), P(db.handle), None),
                 (P(dead), P(db.handle), P(out)), (P(da.handle), P(dead), P(out)),
                 (P(ell.handle), P(db.handle), P(out)), (P(da.handle), P(ell.handle), P(out)),
                 (P(hier.handle), P(lapl.handle), P(out)), (P(lapl.handle), P(hier.handle), P(out)),
                 (P(da.handle), P(rows38.handle), P(out)), (P(cols54.handle), P(db.handle), P(out)),
                 (P(wide.handle), P(wide.handle), P(out)),                           # N = 2^32 - 1
                 (P(bad.handle), P(db.handle), P(out)), (P(da.handle), P(bad.handle), P(out)),
                 (P(bare.handle), P(db.handle), P(out)), (P(da.handle), P(bare.handle), P(out)))
        for a_, b_, c_ in calls:
            assert api.lib.spmvHipCsrAdd(1.0, a_, 1.0, b_, None, c_, P(info)) == 1
            assert (C.string_at(C.addressof(out), C.sizeof(out)), C.string_at(C.addressof(info), C.sizeof(info))) == image
        for h in (da, db):                                          # dC == dA, dC == dB
            before = C.string_at(C.addressof(h.handle), C.sizeof(h.handle))
            o = db if h is da else da
            assert api.lib.spmvHipCsrAdd(1.0, P(h.handle), 1.0, P(o.handle), None, P(h.handle), P(info)) == 1
            assert api.lib.spmvHipCsrAdd(1.0, P(o.handle), 1.0, P(h.handle), None, P(h.handle), P(info)) == 1
            assert C.string_at(C.addressof(h.handle), C.sizeof(h.handle)) == before
        assert C.string_at(C.addressof(info), C.sizeof(info)) == image[1]
        err = capfd.readouterr().err
        lines = [line for line in err.splitlines() if "spmvHipCsrAdd: " in line]
        assert len(lines) == len(calls) + 4, err
        for text in ("dA is NULL", "dB is NULL", "dC is NULL", "not a device handle", "dA is an ELL handle", "dB is an ELL handle",
                     "multigrid hierarchy", "A is 37 x 53, B is 38 x 53", "A is 37 x 54, B is 37 x 53", "32-bit row and column ids",
                     "a column id of a source is >= N", "a source has no column or value array", "dC is a source handle itself",
                     "building the sum failed"):
            assert text in err, text
        dc = da.add(db)                                             # the sources are untouched by all of it
        _check(api, dc, ar.add_ref(1.0, A, 1.0, B), "after the refusals")
        dc.free()
    finally:
        for d in (hier, lapl, bare, bad, wide, cols54, rows38, ell, da, db):
            d.free()
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------- determinism, memory
def test_two_builds_give_equal_bits(api, edges):
    A, B, _, _ = edges
    extra = ar.mixed_37x53(np.random.default_rng(2533))
    A, B = _stack(A, extra[0]), _stack(B, extra[1])
    da, db = _up(api, A), _up(api, B)
    try:
        got = []
        for _ in range(2):
            dc = da.add(db, 2.0 / 3.0, -1.0, **LOWERED)
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
        dt = da.transpose()
        dc = da.add(dt)
        d2 = dc.add(da, 1.0, -1.0, **ALL_SORTED)
        dc.add_refresh(da, dt, 2.0, 0.5)
        d2.add_refresh(dc, da)
        da.free()                                                   # the sources first: a sum keeps no pointer to them
        dt.free()
        d2.free()
        dc.free()
        api.spmvHipFinalize()
        api.spmvHipInit(0)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert min(free[2:]) >= free[1] - (8 << 20) and free[-1] >= free[1] - (8 << 20), free
