"""The entry filter on the device (spmvHipCsrFilter, spmvHipCsrFilterRefresh): C's IRP, JA and AS and info's nnzC / maxRowNnz /
lumpedRows are compared with tests/filter_ref.py -- indices exact, values as bits, a copied NaN with its payload -- in all
three modes, with and without lump where allowed, at the tile and wavefront edges, on every kind of source handle, after a
refresh; C then runs through SpMV, the triangular solve and the transpose; every refusal leaves dC and info untouched."""
import ctypes as C

import numpy as np
import pytest

import add_ref as ad
import amg_ref as ar
import amg_sa_ref as sa
import filter_ref as fr
import serial_order_inputs as si
import spgemm_ref as sr
from bits import assert_same_bits
from trsv_ref import trsv_levels

pytestmark = pytest.mark.gpu

ROWS = "hipSpMVRowsCSR"
TILE = 1024                                                        # entries of a workgroup's tile (filter.hip)
IRP32_LIMIT = (1 << 32) - 65536
P = C.byref


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


def _raw(obj):
    return bytes(C.string_at(C.addressof(obj), C.sizeof(obj)))


def _square_options(theta=0.25, cut=1.25):
    return [fr.opts(fr.ABS, theta=cut, lump=True), fr.opts(fr.STRENGTH, theta=theta), fr.opts(fr.STRENGTH, theta=theta, lump=True),
            fr.opts(fr.STRENGTH, theta=0.0, lump=True), fr.opts(fr.STRENGTH, theta=1e300, lump=True)]


def _any_options(cut=1.25):
    return [fr.opts(fr.BAND, -1, 2), fr.opts(fr.BAND, None, 0), fr.opts(fr.BAND, 0, None), fr.opts(fr.BAND, 0, 0), fr.opts(fr.BAND, 3, 1),
            fr.opts(fr.BAND, None, None), fr.opts(fr.ABS, theta=0.0), fr.opts(fr.ABS, theta=cut), fr.opts(fr.ABS, theta=1e300)]


def _filter(dm, o):
    return dm.filter(o["mode"], o["lo"], o["hi"], o["theta"], o["lump"])


def _check(api, dc, A, o, what):
    """dc against the reference of filter(A, o): arrays, NZ, info"""
    R, kept, lumped = fr.filter_ref(A, o, info=True)
    got = _arrays(api, dc)
    what = f"{what} {o}"
    assert int(dc.handle.NZ) == R[3].size == got[3].size == got[4].size, f"{what}: NZ"
    assert int(got[2][-1]) == R[3].size, f"{what}: IRP[M]"
    fr.same_bits(got, R, what, lumped=o["lump"])
    info = dc.filter_info()
    assert (info.nnzA, info.nnzC) == (A[3].size, R[3].size), what
    assert info.maxRowNnz == (int(np.diff(R[2].astype(np.int64)).max()) if R[0] else 0), what
    assert info.lumpedRows == lumped, what
    return R, kept


def _filter_and_check(api, A, options, what, dm=None):
    own = dm is None
    dm = _up(api, A) if own else dm
    try:
        for o in options:
            dc = _filter(dm, o)
            try:
                _check(api, dc, A, o, what)
            finally:
                dc.free()
    finally:
        if own:
            dm.free()


def test_device_memory_comes_back_after_twenty_builds(api):
    """(first in the file: no other test's handles are alive yet)"""
    import torch
    A = sa.with_one_diagonal(*(lambda a: (a[0], a[2], a[3]))(sr.laplacian7(40, 40, 40)), seed=1)
    da = _up(api, A)
    try:
        def once():
            c = da.filter("strength", theta=0.25, lump=True)
            c.filter_refresh(da)
            kept = int(c.handle.NZ) * 16 + A[3].size // 8
            c.free()
            return kept
        once(), once()
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        kept = [once() for _ in range(20)]
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        slack = 8 << 20
        assert sum(kept) > 2 * slack, "twenty leaked handles would show"
        assert after >= before - slack, (before, after)
    finally:
        da.free()


# ------------------------------------------------------------------------------------------------------- small shapes
GRAPHS = fr.lump_inputs(0)


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_every_small_graph_in_every_mode(api, name, special):
    """M = 0, 1, 2, 3, the path, the Laplacian, the stars, messy (unsorted rows, repeats, isolated vertices); special: the
    values seeded with -0.0, +-Inf, a NaN with a payload, denormals and a stored 0.0"""
    A = GRAPHS[name]
    if special:
        A = A[:4] + (fr.special_values(np.random.default_rng(2910), A[3].size),)
    _filter_and_check(api, A, _any_options() + _square_options() + [fr.opts(fr.STRENGTH, theta=0.35, lump=True)], name)


def _empty(M, N):
    return M, N, np.zeros(M + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0)


@pytest.mark.parametrize("shape", [(0, 0), (0, 5), (6, 0), (6, 5)])
def test_empty_sources(api, oracle, shape):
    A = _empty(*shape)
    da = _up(api, A)
    try:
        for o in _any_options() + ([fr.opts(fr.STRENGTH, theta=0.1, lump=True)] if shape == (0, 0) else []):
            dc = _filter(da, o)
            try:
                _check(api, dc, A, o, f"empty {shape}")
                if shape[0] and shape[1]:
                    dx, dy = api.DeviceVector(shape[1]).up(np.ones(shape[1])), api.DeviceVector(shape[0])
                    dy.poison()
                    api.spmv(ROWS, dc, dx, dy)
                    assert_same_bits(dy.down(), np.zeros(shape[0]), "SpMV on an empty C")
                    dx.free()
                    dy.free()
            finally:
                dc.free()
    finally:
        da.free()


def _square_with_lengths(rng, lens, N, values=None):
    """row i holds lens[i] >= 1 entries in random stored order, exactly one of them (i, i); repeats of other columns allowed"""
    rows, cols = [], []
    for i, n in enumerate(lens):
        c = rng.integers(0, N - 1, int(n))
        c[c >= i] += 1                                            # never i
        c[rng.integers(0, int(n))] = i
        rows += [i] * int(n)
        cols += c.tolist()
    vals = (si.order_values if values is None else values)(rng, len(rows))
    return sr.csr(len(lens), N, rows, cols, vals)


ROW_LENGTHS = [1, 63, 64, 65, 127, 128, 129, 1, 2, 200, 64, 1]


@pytest.mark.parametrize("special", [False, True])
def test_rows_at_the_wavefront_edges(api, special):
    """rows of 1, 63, 64, 65, 127, 128 and 129 entries (the lump takes a lane up to 64 entries, a wavefront above)"""
    rng = np.random.default_rng(2911)
    M = len(ROW_LENGTHS)
    A = _square_with_lengths(rng, ROW_LENGTHS, M, fr.special_values if special else None)
    A = (M, M) + A[2:]
    assert np.array_equal(np.diff(A[2].astype(np.int64)), ROW_LENGTHS)
    _filter_and_check(api, A, _any_options(0.5) + _square_options(0.5, 0.5), "row lengths")


def test_rows_of_no_entry(api):
    """rows of 0, 1, 63, 64, 65, 127, 128, 129 entries, no diagonal rule: BAND and ABS"""
    rng = np.random.default_rng(2912)
    lens = np.array([0, 1, 63, 0, 0, 64, 65, 127, 0, 128, 129, 0], dtype=np.int64)
    A = sr.random_csr(rng, lens.size, 150, lens, fr.special_values)
    _filter_and_check(api, A, _any_options(0.5), "rows with no entry")


@pytest.mark.parametrize("nnz", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049])
def test_entry_counts_at_the_tile_and_wavefront_edges(api, nnz):
    rng = np.random.default_rng(nnz)
    M = 40
    lens = np.ones(M, dtype=np.int64)
    extra = rng.multinomial(nnz - M, np.ones(M) / M)
    A = _square_with_lengths(rng, lens + extra, M)
    A = (M, M) + A[2:]
    assert A[3].size == nnz
    _filter_and_check(api, A, _any_options(0.5) + _square_options(0.5, 0.5), f"{nnz} entries")


def test_first_and_last_entry_of_a_tile_dropped(api):
    """ABS on 3 tiles and a part: exactly the entries at the tile edges are small; then exactly those are kept"""
    rng = np.random.default_rng(2913)
    M, per = 25, 130
    A = sr.random_csr(rng, M, 300, per)
    assert A[3].size == 3 * TILE + 178
    edges = np.array([0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 3 * TILE - 1, 3 * TILE, A[3].size - 1])
    for small in (True, False):
        v = np.where(rng.random(A[3].size) < 0.5, 2.0, -3.0)
        v[edges] = 0.25
        if not small:
            v = np.where(np.isin(np.arange(v.size), edges), 5.0, 0.25)
        X = A[:4] + (v,)
        R, kept = fr.filter_ref(X, fr.opts(fr.ABS, theta=1.0))
        assert (not np.isin(edges, kept).any()) if small else np.array_equal(kept, edges)
        _filter_and_check(api, X, [fr.opts(fr.ABS, theta=1.0)], "tile edges")


def test_five_thousand_empty_rows_between_two_entries(api):
    """the slice of row pointers a tile stages is bounded: these tiles span 5 000 rows"""
    rng = np.random.default_rng(2914)
    for first, last in ((1, 1), (10, 700), (1500, 3)):
        M = 5002
        lens = np.zeros(M, dtype=np.int64)
        lens[0], lens[-1] = first, last
        A = sr.random_csr(rng, M, M, lens)
        A[3][0], A[3][-1] = 0, M - 1
        _filter_and_check(api, A, [fr.opts(fr.BAND, 0, 0), fr.opts(fr.BAND, None, 0), fr.opts(fr.BAND, None, None), fr.opts(fr.ABS, theta=0.5),
                                   fr.opts(fr.BAND, 1, 0)], f"empty rows {first}/{last}")
    # ... and with a diagonal in every row of the two blocks around the gap the strength filter cannot run (a row without
    # a diagonal is refused): the same gap of rows that hold their diagonal alone
    M = 5300
    lens = np.ones(M, dtype=np.int64)
    lens[:100], lens[-200:] = 9, 7
    A = _square_with_lengths(rng, lens, M)
    _filter_and_check(api, A, _square_options(0.5, 0.5), "a gap of diagonal-only rows")


def test_one_row_of_three_thousand_entries_lumped(api):
    """star with 3 000 leaves: the hub's row takes a wavefront, the leaf rows a lane; at this theta every off-diagonal goes"""
    A = sa.with_one_diagonal(*ar.star(3000), seed=4)
    special = A[:4] + (fr.special_values(np.random.default_rng(2915), A[3].size),)
    for X, what in ((A, "star3000"), (special, "star3000 special")):
        R, kept = fr.filter_ref(X, fr.opts(fr.STRENGTH, theta=0.25, lump=True))
        if X is A:
            assert kept.size == A[0], "every off-diagonal entry is dropped"
        _filter_and_check(api, X, _square_options() + [fr.opts(fr.ABS, theta=1.2, lump=True), fr.opts(fr.ABS, theta=1.2)], what)
    rev = sr.reverse_rows(A)
    _filter_and_check(api, rev, [fr.opts(fr.STRENGTH, theta=0.25, lump=True)], "star3000 reversed")


@pytest.mark.parametrize("shape", [(40, 90), (90, 40)])
def test_rectangular(api, shape):
    rng = np.random.default_rng(2916)
    A = sr.random_csr(rng, shape[0], shape[1], rng.integers(0, 30, shape[0]), fr.special_values)
    _filter_and_check(api, A, _any_options(0.5) + [fr.opts(fr.BAND, -50, -45), fr.opts(fr.BAND, 45, 60)], f"{shape}")


# ----------------------------------------------------------------------------------------------------- kinds of source
def test_adopted_source_with_eight_byte_row_pointers(api):
    A = GRAPHS["messy"]
    M, _, IRP, JA, AS = A
    bufs = [api.DeviceBuffer(8 * (M + 1)).up(IRP.astype(np.uint64)), api.DeviceBuffer(4 * JA.size).up(JA.astype(np.uint32)),
            api.DeviceBuffer(8 * JA.size).up(AS)]
    dm = api.DeviceMatrix()
    dm.keep = bufs
    assert api.lib.spmvHipAdoptCSR(P(dm.handle), M, M, JA.size, bufs[0].ptr, 8, bufs[1].ptr, bufs[2].ptr, None) == 0
    try:
        _filter_and_check(api, A, _any_options() + _square_options(), "adopted", dm)
    finally:
        dm.free()


def test_unit_value_source(api):
    lap = sr.laplacian7(7, 6, 5)
    A = lap[:4] + (np.full(lap[3].size, -1.5),)
    da = _up(api, A)
    try:
        v = C.c_double()
        assert api.lib.spmvHipUnitValue(P(da.handle), P(v)) == 1 and v.value == -1.5
        _filter_and_check(api, A, _any_options() + _square_options(0.9, 1.0), "unit values", da)
        dc = da.tril()
        assert api.lib.spmvHipUnitValue(P(dc.handle), P(v)) == 1 and v.value == -1.5, "C has its own unit detection"
        dc.free()
    finally:
        da.free()


def test_sources_that_are_transposes_products_and_sums(api):
    A = GRAPHS["messy"]
    B = sa.with_one_diagonal(*ar.messy(40, seed=6), seed=7)
    da, db = _up(api, A), _up(api, B)
    made = {"transpose": (da.transpose(), sr.transpose(A)), "product": (da.multiply(db), sr.spgemm_ref(A, B)),
            "sum": (da.add(db, 1.0, -0.5), ad.add_ref(1.0, A, -0.5, B))}
    made["filtered"] = (made["sum"][0].filter("abs", theta=0.5), fr.filter_ref(made["sum"][1], fr.opts(fr.ABS, theta=0.5))[0])
    try:
        for kind, (dm, X) in made.items():
            options = _any_options() + (_square_options() if kind == "transpose" else [fr.opts(fr.STRENGTH, theta=0.25)])
            usable = []
            for o in options:
                try:
                    fr.filter_ref(X, o)
                    usable.append(o)
                except ValueError:
                    pass
            assert len(usable) >= len(_any_options())
            _filter_and_check(api, X, usable, kind, dm)
    finally:
        for dm, _ in made.values():
            dm.free()
        da.free()
        db.free()


# ------------------------------------------------------------------------------------------------- C as a CSR handle
def test_spmv_trsv_and_transpose_run_on_c(api, oracle):
    rng = np.random.default_rng(2917)
    A = sa.with_one_diagonal(*ar.small_graphs()["laplacian12x10x8"], seed=8)
    M = A[0]
    da = _up(api, A)
    dc = da.filter("strength", theta=0.14, lump=True)
    lower, upper, diag = dc.tril(), dc.triu(1), dc.diagonal_matrix()
    ct = dc.transpose()
    try:
        Cr, _ = fr.filter_ref(A, fr.opts(fr.STRENGTH, theta=0.14, lump=True))
        assert M < Cr[3].size < A[3].size
        x = si.order_values(rng, M)
        dx, dy = api.DeviceVector(M).up(x), api.DeviceVector(M)
        dy.poison()
        api.spmv(ROWS, dc, dx, dy)
        assert_same_bits(dy.down(), oracle.csr_serial(Cr[2], Cr[3], Cr[4], x), "SpMV on C")
        L, _ = fr.filter_ref(Cr, fr.opts(fr.BAND, None, 0))
        fr.same_bits(_arrays(api, lower), L, "tril of C")
        fr.same_bits(_arrays(api, upper), fr.filter_ref(Cr, fr.opts(fr.BAND, 1, None))[0], "triu(1) of C")
        D = _arrays(api, diag)
        assert np.array_equal(D[3], np.arange(M)) and np.array_equal(D[2], np.arange(M + 1))
        b = rng.standard_normal(M)
        assert_same_bits(lower.solve_triangular(b), trsv_levels(M, L[2], L[3], L[4], b, True, False), "hipSpTRSVCSR on tril(C)")
        assert_same_bits(dc.solve_triangular(b, lower=False), trsv_levels(M, Cr[2], Cr[3], Cr[4], b, False, False), "... on C, upper")
        sr.same_bits(_arrays(api, ct), sr.transpose(Cr), "transpose of C")
        api.spmv(ROWS, ct, dx, dy)
        T = sr.transpose(Cr)
        assert_same_bits(dy.down(), oracle.csr_serial(T[2], T[3], T[4], x), "SpMV on the transpose of C")
        dx.free()
        dy.free()
    finally:
        for d in (ct, diag, upper, lower, dc, da):
            d.free()


# ------------------------------------------------------------------------------------------------------------- refresh
@pytest.mark.parametrize("o", [fr.opts(fr.STRENGTH, theta=0.25, lump=True), fr.opts(fr.STRENGTH, theta=0.25), fr.opts(fr.ABS, theta=1.25),
                               fr.opts(fr.ABS, theta=1.25, lump=True), fr.opts(fr.BAND, None, 0)],
                         ids=["strength-lump", "strength", "abs", "abs-lump", "tril"])
@pytest.mark.parametrize("name", ["messy", "star200", "rows"])
def test_refresh_keeps_the_pattern_and_takes_the_new_values(api, oracle, name, o):
    rng = np.random.default_rng(2918)
    if name == "rows":
        A = _square_with_lengths(rng, ROW_LENGTHS, len(ROW_LENGTHS))
        A = (len(ROW_LENGTHS), len(ROW_LENGTHS)) + A[2:]
        o = dict(o, theta=0.5)
    else:
        A = GRAPHS[name]
    M = A[0]
    da = _up(api, A)
    dc = _filter(da, o)
    try:
        R, kept = _check(api, dc, A, o, name)
        where = _addresses(dc)
        x = si.order_values(rng, M)
        dx, dy = api.DeviceVector(M).up(x), api.DeviceVector(M)
        assert api.lib.spmvHipBuildSell(P(dc.handle)) == 0        # a private format built on C before the refresh
        new = A[4] * (1.0 + rng.random(A[4].size)) * np.where(rng.random(A[4].size) < 0.2, -1.0, 1.0)
        new[rng.integers(0, new.size, 3)] = [np.inf, -0.0, np.uint64(0x7FF8000000000321).view(np.float64)]
        B = A[:4] + (new,)
        if o["mode"] != fr.BAND:
            assert not np.array_equal(fr.filter_ref(B, o)[1], kept), "a fresh filter of the new values would keep other entries"
        da.update_values(new)
        dc.filter_refresh(da)
        want = fr.filter_refresh_ref(kept, B, o)
        assert np.array_equal(want[2], R[2]) and np.array_equal(want[3], R[3])
        got = _arrays(api, dc)
        fr.same_bits(got, want, f"{name} refreshed {o}", lumped=o["lump"])
        assert _addresses(dc) == where and int(dc.handle.NZ) == R[3].size
        info = dc.filter_info()
        assert (info.nnzA, info.nnzC) == (A[3].size, R[3].size)
        finite = np.where(np.isfinite(got[4]), got[4], 1.0)       # (SELL pads with 0.0: 0 * Inf would be a NaN of its own)
        if np.array_equal(finite.view(np.uint64), got[4].view(np.uint64)):
            dy.poison()
            api.spmv("hipSpMVRowsSELL", dc, dx, dy)
            assert_same_bits(dy.down(), oracle.csr_serial(want[2], want[3], got[4], x), "SELL after the refresh")
        dy.poison()
        api.spmv(ROWS, dc, dx, dy)
        y, yr = dy.down(), oracle.csr_serial(want[2], want[3], got[4], x)
        nan = np.isnan(yr)
        assert np.array_equal(np.isnan(y), nan)
        assert_same_bits(np.where(nan, 0.0, y), np.where(nan, 0.0, yr), "SpMV after the refresh")
        dx.free()
        dy.free()
    finally:
        dc.free()
        da.free()


def test_sell_built_before_the_refresh_gives_the_new_y(api, oracle):
    rng = np.random.default_rng(2919)
    A = GRAPHS["laplacian12x10x8"]
    M = A[0]
    o = fr.opts(fr.STRENGTH, theta=0.14, lump=True)
    da = _up(api, A)
    dc = _filter(da, o)
    try:
        R, kept = _check(api, dc, A, o, "laplacian")
        assert M < kept.size < A[3].size
        x = si.order_values(rng, M)
        dx, dy = api.DeviceVector(M).up(x), api.DeviceVector(M)
        api.spmv("hipSpMVRowsSELL", dc, dx, dy)
        assert_same_bits(dy.down(), oracle.csr_serial(R[2], R[3], R[4], x), "SELL before")
        B = A[:4] + (A[4] * (0.5 + rng.random(A[4].size)),)
        da.update_values(B[4])
        dc.filter_refresh(da)
        want = fr.filter_refresh_ref(kept, B, o)
        fr.same_bits(_arrays(api, dc), want, "refreshed", lumped=True)
        dy.poison()
        api.spmv("hipSpMVRowsSELL", dc, dx, dy)
        assert_same_bits(dy.down(), oracle.csr_serial(want[2], want[3], want[4], x), "SELL after")
        dx.free()
        dy.free()
    finally:
        dc.free()
        da.free()


def test_two_identical_builds_give_identical_bytes(api):
    A = sa.with_one_diagonal(*ar.star(3000), seed=9)
    A = A[:4] + (fr.special_values(np.random.default_rng(2920), A[3].size),)
    da = _up(api, A)
    try:
        for o in (fr.opts(fr.STRENGTH, theta=0.25, lump=True), fr.opts(fr.ABS, theta=1.2)):
            a, b = _filter(da, o), _filter(da, o)
            try:
                for x, y in zip(_arrays(api, a)[2:], _arrays(api, b)[2:]):
                    assert x.tobytes() == y.tobytes()
            finally:
                a.free()
                b.free()
    finally:
        da.free()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_dc_and_info_untouched(api, capfd):
    lib = api.lib
    A = GRAPHS["messy"]
    M = A[0]
    da, other = _up(api, A), _up(api, A)
    rect = _up(api, sr.random_csr(np.random.default_rng(2921), 6, 5, 2))
    nodiag = _up(api, (3, 3, np.array([0, 2, 3, 4], np.uint64), np.array([0, 1, 2, 0], np.uint64), np.ones(4)))
    twodiag = _up(api, (3, 3, np.array([0, 1, 3, 4], np.uint64), np.array([0, 1, 1, 2], np.uint64), np.ones(4)))
    ell = api.csr_to_ell_device(other, False)
    hier = da.amg(coarseRows=8)
    gone = _up(api, A)
    gone.free()
    good = da.filter("abs", theta=1.25)
    keep = []
    out, info = api.spmat(), api.spmvFilterInfo()
    for obj in (out, info):
        C.memset(C.addressof(obj), 0x5A, C.sizeof(obj))
    before = [_raw(out), _raw(info)]
    band, strength = api.spmvFilterOpts(0, 0, 0, 0.0, 0), api.spmvFilterOpts(2, 0, 0, 0.25, 0)
    try:
        def refused(call, msg=None):
            capfd.readouterr()
            assert call() != 0
            err = capfd.readouterr().err
            assert "spmvHipCsrFilter" in err, err
            if msg:
                assert msg in err, err
            assert [_raw(out), _raw(info)] == before, "dC and info untouched"

        flt = lib.spmvHipCsrFilter
        HA, OUT, INFO = P(da.handle), P(out), P(info)
        refused(lambda: flt(None, P(band), OUT, INFO), "NULL")
        refused(lambda: flt(HA, None, OUT, INFO), "NULL")
        refused(lambda: flt(HA, P(band), None, INFO), "NULL")
        refused(lambda: flt(P(gone.handle), P(band), OUT, INFO), "not a device handle")
        refused(lambda: flt(P(ell.handle), P(band), OUT, INFO), "ELL")
        refused(lambda: flt(P(hier.handle), P(band), OUT, INFO), "hierarchy")
        snap = _raw(da.handle)
        refused(lambda: flt(HA, P(band), HA, INFO), "source handle itself")
        assert _raw(da.handle) == snap
        for mode in (3, -1, 99):
            refused(lambda: flt(HA, P(api.spmvFilterOpts(mode, 0, 0, 0.0, 0)), OUT, INFO), "mode")
        for theta in (-0.5, np.inf, -np.inf, np.nan):
            for mode in (0, 1, 2):
                refused(lambda: flt(HA, P(api.spmvFilterOpts(mode, 0, 0, theta, 0)), OUT, INFO), "theta")
        refused(lambda: flt(HA, P(api.spmvFilterOpts(0, 0, 0, 0.0, 1)), OUT, INFO), "lump")
        refused(lambda: flt(P(rect.handle), P(strength), OUT, INFO), "square")
        refused(lambda: flt(P(rect.handle), P(api.spmvFilterOpts(1, 0, 0, 0.5, 1)), OUT, INFO), "square")
        refused(lambda: flt(P(nodiag.handle), P(strength), OUT, INFO), "row 1 does not hold exactly one")
        refused(lambda: flt(P(twodiag.handle), P(api.spmvFilterOpts(1, 0, 0, 0.5, 1)), OUT, INFO), "row 1 does not hold exactly one")
        # NZ at the 32-bit limit: adopted with no value or column array (nothing is ever read); entries but no arrays
        irp = api.DeviceBuffer(16)
        keep.append(irp)
        for nz, msg in ((IRP32_LIMIT, "NZ="), (3, "no column or value array")):
            big = api.DeviceMatrix()
            h_irp = np.array([0, nz], dtype=np.uint64)
            assert lib.spmvHipAdoptCSR(P(big.handle), 1, 4, nz, irp.ptr, 8, None, None, h_irp.ctypes.data_as(C.c_void_p)) == 0
            keep.append(big)
            refused(lambda: flt(P(big.handle), P(band), OUT, INFO), msg)
        # a column id >= N in an adopted array
        h_irp = np.array([0, 2, 4], dtype=np.uint32)               # (each row holds its diagonal: the STORED rule is met)
        bufs = [api.DeviceBuffer(12).up(h_irp), api.DeviceBuffer(16).up(np.array([0, 1, 1, 7], np.uint32)), api.DeviceBuffer(32).up(np.ones(4))]
        wide = api.DeviceMatrix()
        wide.keep = bufs
        assert lib.spmvHipAdoptCSR(P(wide.handle), 2, 2, 4, bufs[0].ptr, 4, bufs[1].ptr, bufs[2].ptr, h_irp.ctypes.data_as(C.c_void_p)) == 0
        keep.append(wide)
        for o in (band, api.spmvFilterOpts(1, 0, 0, 0.5, 0), strength):
            refused(lambda: flt(P(wide.handle), P(o), OUT, INFO), "column id")
        # the refresh
        ref = lib.spmvHipCsrFilterRefresh
        snap = _raw(good.handle)
        refused(lambda: ref(P(other.handle), HA, INFO), "not made by spmvHipCsrFilter")
        refused(lambda: ref(P(good.handle), P(other.handle), INFO), "not the handle")
        refused(lambda: ref(None, HA, INFO), "NULL")
        refused(lambda: ref(P(good.handle), None, INFO), "NULL")
        refused(lambda: ref(P(good.handle), P(gone.handle), INFO), "not a device handle")
        assert _raw(good.handle) == snap
        assert ref(P(good.handle), HA, None) == 0, "info may be NULL"
        _check(api, good, A, fr.opts(fr.ABS, theta=1.25), "after the refusals")
        with pytest.raises(api.SpmvHipError):
            da.filter("no such mode")
        with pytest.raises(api.SpmvHipError):
            da.filter_info()
    finally:
        for d in [good, hier, ell, twodiag, nodiag, rect, other, da] + keep[1:]:
            d.free()
        keep[0].free() if keep else None
