"""The COO assembly on the device (spmvHipCooAssemble, spmvHipCooAssembleRefresh, spmvHipCsrToCoo): C's IRP and JA exact, AS
as bits and every field of info against tests/coo_ref.py, under SUM and LAST -- run lengths at the wavefront and tile
edges, gaps of empty rows, the width edges of the 64-bit key, skips, input orders, special values, a Q1 element assembly that
then runs through SpMV, ILU(0) + CG and the derived handles, the refresh with built formats and derived handles, to_coo on
every kind of handle, two streams, and every refusal with dC and info untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import add_ref as ad
import coo_ref as cr
import filter_ref as fr
import serial_order_inputs as si
import spgemm_ref as sr
from bits import assert_same_bits

pytestmark = pytest.mark.gpu

ROWS = "hipSpMVRowsCSR"
TILE = 1024                                                        # sorted entries of a workgroup's tile (coo.hip)
IRP32_LIMIT = (1 << 32) - 65536
MODES = ["sum", "last"]
INFO_FIELDS = ("nEntries", "skipped", "nnzC", "duplicates", "maxRun", "maxRowNnz")
P = C.byref


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.lib.spmvHipSetStream(None)
    a.spmvHipFinalize()


def _down(api, ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
    return out


def _arrays(api, dm, irp=np.uint32):
    h = dm.handle
    return (int(h.M), int(h.N), _down(api, h.IRP, h.M + 1, irp), _down(api, h.JA, h.NZ, np.uint32), _down(api, h.AS, h.NZ, np.float64))


def _addresses(dm):
    return tuple(C.cast(p, C.c_void_p).value for p in (dm.handle.IRP, dm.handle.JA, dm.handle.AS))


def _raw(obj):
    return bytes(C.string_at(C.addressof(obj), C.sizeof(obj)))


def _up(api, A):
    return api.spMatCpyCSR(api.HostCSR(*A))


def _compare(api, dc, ref, what, refreshed=False):
    """dc against (C, info, runs) of the reference: arrays, NZ, every count of info"""
    R, info, runs = ref
    got = _arrays(api, dc)
    assert int(dc.handle.NZ) == R[3].size == got[3].size == got[4].size, f"{what}: NZ"
    assert int(got[2][-1]) == R[3].size, f"{what}: IRP[M]"
    cr.same_bits(got, R, what, nan_sums=cr.nan_sums_of(R, runs))
    di = dc.assemble_info()
    for f in INFO_FIELDS:
        assert getattr(di, f) == info[f], f"{what}: info.{f} = {getattr(di, f)}, expected {info[f]}"
    assert di.ms >= 0.0 and (di.tempBytes == 0 if refreshed else di.tempBytes >= 24 * info["nEntries"])


def _assemble_and_check(api, M, N, rows, cols, vals, what, modes=MODES, keep=False):
    out = []
    for mode in modes:
        ref = cr.assemble_ref(M, N, rows, cols, vals, mode)
        dc = api.assemble_coo(M, N, np.asarray(rows), np.asarray(cols), np.asarray(vals, dtype=np.float64), duplicates=mode)
        try:
            _compare(api, dc, ref, f"{what} ({mode})")
        except BaseException:
            dc.free()
            raise
        if keep:
            out.append((dc, ref))
        else:
            dc.free()
    return out


def _spmv(api, dm, x):
    dx, dy = api.DeviceVector(x.size).up(x), api.DeviceVector(int(dm.handle.M))
    try:
        dy.poison()
        api.spmv(ROWS, dm, dx, dy)
        return dy.down()
    finally:
        dx.free()
        dy.free()


def _random_list(rng, M, N, n, skip=0.05):
    rows, cols = rng.integers(0, M, n), rng.integers(0, N, n)
    rows[rng.random(n) < skip] = -1
    cols[rng.random(n) < skip] = -1
    return rows, cols, si.order_values(rng, n)


# ---------------------------------------------------------------------------------------------------------- 1 memory
def test_device_memory_comes_back_after_twenty_builds_and_refreshes(api):
    """(first in the file: no other test's handles are alive yet)"""
    import torch
    rng = np.random.default_rng(3700)
    n, M = 500_000, 50_000
    rows, cols = rng.integers(0, M, n), rng.integers(0, M, n)
    vals = rng.uniform(-1, 1, n)
    t = [torch.from_numpy(a.astype(np.int32)).cuda() for a in (rows, cols)] + [torch.from_numpy(vals).cuda()]

    def once():
        c = api.assemble_coo(M, M, *t)
        c.assemble_refresh(t[2])
        held = int(c.handle.NZ) * 16 + n * 4
        c.free()
        return held
    once(), once()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    held = [once() for _ in range(20)]
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    slack = 8 << 20
    assert sum(held) > 2 * slack, "twenty leaked handles would show"
    assert after >= before - slack, (before, after)


# ------------------------------------------------------------------------------------------------------ 2 run lengths
RUN_LENGTHS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 5000]


@pytest.mark.parametrize("shift", [0, 62, 959])
def test_run_lengths_across_the_wavefront_and_tile_edges(api, shift):
    """row 1 holds one run per length on columns 10, 11, ...: in sorted order the runs start at 0, 1, 3, 66, 130, 195, 1218,
    2242, 3267 (+ shift single entries of row 0 before them), so they straddle the 64-entry and the 1024-entry borders; the
    input is shuffled, so only a stable sort adds them in input order"""
    rng = np.random.default_rng(3701 + shift)
    cols = np.concatenate([np.arange(shift)] + [np.full(L, 10 + k) for k, L in enumerate(RUN_LENGTHS)])
    rows = np.concatenate([np.zeros(shift, np.int64), np.ones(sum(RUN_LENGTHS), np.int64)])
    o = rng.permutation(rows.size)
    vals = si.order_values(rng, rows.size)
    starts = shift + np.cumsum([0] + RUN_LENGTHS[:-1])
    assert any(s // TILE != (s + L - 1) // TILE for s, L in zip(starts, RUN_LENGTHS)) and any(s % 64 + L > 64 for s, L in zip(starts, RUN_LENGTHS))
    (dc, ref), = _assemble_and_check(api, 3, 1000, rows[o], cols[o], vals, f"runs shift {shift}", ["sum"], keep=True)
    dc.free()
    assert ref[1]["maxRun"] == 5000 and np.array_equal(np.diff(ref[2][1])[shift:], RUN_LENGTHS)
    rev = cr.assemble_ref(3, 1000, rows[o][::-1], cols[o][::-1], vals[::-1])[0]
    long_runs = shift + np.flatnonzero(np.array(RUN_LENGTHS) >= 63)
    assert np.count_nonzero(rev[4][long_runs].view(np.uint64) != ref[0][4][long_runs].view(np.uint64)) >= 4, "the order shows in the bits"
    _assemble_and_check(api, 3, 1000, rows[o], cols[o], vals, f"runs shift {shift}", ["last"])


# ------------------------------------------------------------------------------------------------- 3 row-pointer gaps
def _gap_cases():
    rng = np.random.default_rng(3702)
    cases = {}
    r = np.array([3, 4, 9, 17, 9, 3]); cases["empty rows first, last and between"] = (20, 30, r, rng.integers(0, 30, r.size))
    r = np.array([3005, 2, 2, 3005, 3005]); cases["3000 consecutive empty rows"] = (3010, 50, r, rng.integers(0, 50, r.size))
    cases["one row holds everything"] = (5, 400, np.full(3000, 2), rng.integers(0, 400, 3000))
    cases["every row holds one entry"] = (2500, 2500, rng.permutation(2500), rng.permutation(2500))
    cases["1 x 1"] = (1, 1, np.zeros(3, np.int64), np.zeros(3, np.int64))
    cases["last row alone"] = (2050, 7, np.array([2049]), np.array([6]))
    cases["first row alone"] = (2050, 7, np.array([0, 0]), np.array([0, 6]))
    return {k: v + (si.order_values(rng, v[2].size),) for k, v in cases.items()}


GAPS = _gap_cases()


@pytest.mark.parametrize("name", list(GAPS))
def test_row_pointer_gaps(api, oracle, name):
    M, N, rows, cols, vals = GAPS[name]
    for dc, ref in _assemble_and_check(api, M, N, rows, cols, vals, name, keep=True):
        try:
            x = si.order_values(np.random.default_rng(5), N)
            assert_same_bits(_spmv(api, dc, x), oracle.csr_serial(ref[0][2], ref[0][3], ref[0][4], x), f"SpMV on {name}")
        finally:
            dc.free()


# ------------------------------------------------------------------------------------------------------ 4 width edges
@pytest.mark.parametrize("M", [32, 33, 64, 65])
def test_row_counts_at_a_power_of_two(api, M):
    rng = np.random.default_rng(3703 + M)
    rows, cols, vals = _random_list(rng, M, M, 40 * M)
    rows[:4], cols[:4] = [M - 1, M - 1, 0, 0], [M - 1, 0, M - 1, 0]
    _assemble_and_check(api, M, M, rows, cols, vals, f"M = N = {M}")


def test_the_top_of_the_64_bit_key(api):
    """N = 2^32 - 2: columns take 32 key bits, the last column is 2^32 - 3, and it costs no memory"""
    N = (1 << 32) - 2
    rows = np.array([4, 0, 4, 2, 4, 0, -1, 6], dtype=np.int64)
    cols = np.array([N - 1, N - 1, 0, N - 2, N - 1, 1 << 31, N - 1, N - 1], dtype=np.int64)
    vals = si.order_values(np.random.default_rng(3704), rows.size)
    _assemble_and_check(api, 7, N, rows, cols, vals, "N = 2^32 - 2")
    _assemble_and_check(api, 7, N, rows.astype(np.uint32), cols.astype(np.uint32), vals, "N = 2^32 - 2, uint32 input")


def test_a_million_rows_and_ten_entries(api):
    M = (1 << 20) + 1
    rng = np.random.default_rng(3705)
    rows = np.concatenate([[0, M - 1, M - 1, 1 << 19], rng.integers(0, M, 6)])
    _assemble_and_check(api, M, 9, rows, rng.integers(0, 9, 10), si.order_values(rng, 10), "M = 2^20 + 1")


# ------------------------------------------------------------------------------------------------------------ 5 skips
def test_skipped_rows_columns_both_and_all(api):
    nan = np.uint64(0x7FF8000000000ABC).view(np.float64)
    rng = np.random.default_rng(3706)
    rows, cols, vals = _random_list(rng, 60, 70, 5000, skip=0.2)
    rows[:3], cols[:3] = [-1, 5, -1], [5, -1, -1]
    skipped = (rows == -1) | (cols == -1)
    assert skipped[:3].all() and 1000 < skipped.sum() < 3000
    poisoned = np.where(skipped, nan, vals)
    for mode, (dc, ref) in zip(MODES, _assemble_and_check(api, 60, 70, rows, cols, poisoned, "a NaN at every skipped place", keep=True)):
        dc.free()
        assert not np.isnan(ref[0][4]).any() and ref[1]["skipped"] == skipped.sum()
        cr.same_bits(ref[0], cr.assemble_ref(60, 70, rows, cols, vals, mode)[0], "the reference does not read a skipped place either")
    # a skipped place may hold any index besides the marker: it is not range-checked
    rows2, cols2 = rows.copy(), cols.copy()
    rows2[1], cols2[0] = 4_000_000, 4_000_000
    _assemble_and_check(api, 60, 70, rows2, cols2, poisoned, "an index out of range beside a marker")
    for M, N in ((60, 70), (0, 0), (0, 5), (6, 0)):
        every = np.full(100, -1)
        for dc, ref in _assemble_and_check(api, M, N, every, every, np.full(100, nan), f"every entry skipped {M}x{N}", keep=True):
            try:
                assert int(dc.handle.NZ) == 0 and ref[1]["skipped"] == 100
                if M and N:
                    assert_same_bits(_spmv(api, dc, np.ones(N)), np.zeros(M), "SpMV on an empty C")
            finally:
                dc.free()
        none = np.zeros(0, np.int64)
        _assemble_and_check(api, M, N, none, none, np.zeros(0), f"no entry {M}x{N}")


def test_null_arrays_with_no_entry_and_device_tensors_in_place(api):
    import torch
    out, info = api.spmat(), api.spmvCooInfo()
    assert api.lib.spmvHipCooAssemble(6, 5, 0, None, None, None, None, P(out), P(info)) == 0
    assert (out.M, out.N, out.NZ, info.nEntries, info.nnzC) == (6, 5, 0, 0, 0)
    assert api.lib.spmvHipCooAssembleRefresh(P(out), 0, None, None) == 0, "NULL opts keeps the map"
    assert api.lib.hipFreeSpmat(P(out)) == 0
    rng = np.random.default_rng(3707)
    rows, cols, vals = _random_list(rng, 90, 40, 3000)
    new = si.order_values(rng, 3000)
    t = [torch.from_numpy(a.astype(np.int32)).cuda() for a in (rows, cols)] + [torch.from_numpy(vals).cuda()]
    for mode in MODES:
        dc = api.assemble_coo(90, 40, *t, duplicates=mode)
        try:
            ref = cr.assemble_ref(90, 40, rows, cols, vals, mode)
            _compare(api, dc, ref, f"torch operands ({mode})")
            dc.assemble_refresh(torch.from_numpy(new).cuda())
            _compare(api, dc, (cr.refresh_ref(ref[0], ref[2], new, mode),) + ref[1:], f"torch refresh ({mode})", refreshed=True)
            tr = dc.to_coo(as_torch=True)
            want = cr.to_coo_ref(_arrays(api, dc))
            assert [x.dtype for x in tr] == [torch.int32, torch.int32, torch.float64]
            assert np.array_equal(tr[0].cpu().numpy().view(np.uint32), want[0]) and np.array_equal(tr[1].cpu().numpy().view(np.uint32), want[1])
            assert_same_bits(tr[2].cpu().numpy(), want[2], "to_coo(as_torch=True)")
        finally:
            dc.free()
    with pytest.raises(api.SpmvHipError):
        api.assemble_coo(90, 40, rows, t[1], vals)
    with pytest.raises(api.SpmvHipError):
        api.assemble_coo(90, 40, rows.astype(np.float64), cols, vals)
    with pytest.raises(api.SpmvHipError):
        api.assemble_coo(90, 40, np.where(rows == -1, -2, rows), cols, vals)
    with pytest.raises(api.SpmvHipError):
        api.assemble_coo(90, 40, rows, cols[:-1], vals)


# ------------------------------------------------------------------------------------------------------ 6 input orders
def test_the_same_multiset_in_three_orders(api):
    """a matrix with runs of 3 to 6 mixed-magnitude duplicates, listed in CSR order, reversed and shuffled: one pattern,
    three sets of value bits, each the reference's for its order"""
    rng = np.random.default_rng(3708)
    M, N = 70, 50
    base_r, base_c = rng.integers(0, M, 900), rng.integers(0, N, 900)
    rep = rng.integers(1, 7, 900)
    rows, cols = np.repeat(base_r, rep), np.repeat(base_c, rep)
    vals = si.order_values(rng, rows.size)
    o = np.lexsort((cols, rows))
    orders = {"csr order": o, "reversed": o[::-1], "shuffled": rng.permutation(rows.size)}
    refs = {}
    for name, p in orders.items():
        for dc, ref in _assemble_and_check(api, M, N, rows[p], cols[p], vals[p], name, ["sum"], keep=True):
            dc.free()
            refs[name] = ref
        _assemble_and_check(api, M, N, rows[p], cols[p], vals[p], name, ["last"])
    a, b, c = (refs[k][0] for k in orders)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[2], c[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[3], c[3])
    long_runs = np.diff(refs["csr order"][2][1]) >= 3
    assert long_runs.sum() > 100
    for x, y in ((a, b), (a, c), (b, c)):
        assert np.count_nonzero(x[4][long_runs].view(np.uint64) != y[4][long_runs].view(np.uint64)) > 30, "the orders show in the bits"


# ----------------------------------------------------------------------------------------------------------- 7 values
def test_signed_zeros_nan_payloads_infinities_and_explicit_zeros(api):
    nan = np.uint64(0x7FF8000000000123).view(np.float64)
    snan = np.uint64(0x7FF0000000000001).view(np.float64)
    rows = np.array([2, 0, 2, 0, 1, 2, 2, 3, 3, 3, 1, 0, 0])
    cols = np.array([1, 3, 3, 3, 0, 1, 0, 0, 1, 1, 2, 0, 0])
    vals = np.array([np.inf, -0.0, 0.0, 0.0, nan, -np.inf, -0.0, snan, -0.0, -0.0, 0.0, 1.5, -1.5])
    for dc, ref in _assemble_and_check(api, 4, 4, rows, cols, vals, "special values", keep=True):
        try:
            R, info = ref[0], ref[1]
            assert info["nnzC"] == 9 and int(dc.handle.NZ) == 9, "explicit zeros and cancelled sums stay entries"
            got = _arrays(api, dc)[4]
            assert got[2].view(np.uint64) == np.uint64(0x7FF8000000000123), "a single NaN keeps its payload"
            assert got[7].view(np.uint64) == np.uint64(0x7FF0000000000001), "... a signalling one too: it is copied, not computed with"
            assert np.signbit(got[4]) and got[4] == 0.0, "a single -0.0 stays"
            assert np.signbit(got[8]), "-0.0 + -0.0 and the last -0.0"
        finally:
            dc.free()


# ---------------------------------------------------------------------------------------------------- 8 Q1 assembly
def _q1_element(d):
    """the Q1 stiffness matrix of the unit d-cube by 2-point Gauss quadrature, nodes in binary order"""
    g = np.array([0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0)])
    corners = np.array([[(k >> a) & 1 for a in range(d)] for k in range(1 << d)])
    K = np.zeros((1 << d, 1 << d))
    for q in np.ndindex(*([2] * d)):
        x = g[list(q)]
        grad = np.empty((1 << d, d))
        for k, cnr in enumerate(corners):
            for a in range(d):
                f = [(x[b] if cnr[b] else 1.0 - x[b]) for b in range(d)]
                f[a] = 1.0 if cnr[a] else -1.0
                grad[k, a] = np.prod(f)
        K += grad @ grad.T / (1 << d)
    return K, corners


@functools.lru_cache(maxsize=None)
def _q1_triplets(shape):
    """the element-by-element triplets of the Q1 Laplacian on a grid of shape nodes, boundary rows and columns masked with
    the skip marker, then the identity on the boundary"""
    d = len(shape)
    K, corners = _q1_element(d)
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    first = idx[tuple(slice(0, s - 1) for s in shape)].ravel()
    strides = np.array([idx[tuple(1 if b == a else 0 for b in range(d))] for a in range(d)])
    nodes = first[:, None] + (corners @ strides)[None, :]                       # elements x 2^d
    rows = np.repeat(nodes, 1 << d, axis=1).ravel()
    cols = np.tile(nodes, (1, 1 << d)).ravel()
    vals = np.tile(K.ravel(), first.size)
    inner = np.ones(shape, dtype=bool)
    for a in range(d):
        inner[tuple(slice(None) if b != a else [0, -1] for b in range(d))] = False
    boundary = np.flatnonzero(~inner.ravel())
    rows = np.where(inner.ravel()[rows], rows, -1)
    cols = np.where(inner.ravel()[cols], cols, -1)
    return (idx.size, np.concatenate([rows, boundary]), np.concatenate([cols, boundary]), np.concatenate([vals, np.ones(boundary.size)]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(5, 5), (12, 12, 12)])
def test_q1_element_assembly_then_spmv_solves_and_derived_handles(api, oracle, shape, mode):
    M, rows, cols, vals = _q1_triplets(shape)
    ref = cr.assemble_ref(M, M, rows, cols, vals, mode)
    R = ref[0]
    assert ref[1]["skipped"] > 0 and ref[1]["maxRun"] == 1 << len(shape) and ref[1]["maxRowNnz"] == 3 ** len(shape)
    dc = api.assemble_coo(M, M, rows, cols, vals, duplicates=mode)
    made = []
    try:
        _compare(api, dc, ref, f"Q1 {shape} ({mode})")
        rng = np.random.default_rng(3709)
        x = si.order_values(rng, M)
        assert_same_bits(_spmv(api, dc, x), oracle.csr_serial(R[2], R[3], R[4], x), "SpMV on the assembled matrix")
        t = dc.transpose(); made.append(t)
        sr.same_bits(_arrays(api, t), sr.transpose(R), "transpose of C")
        band = dc.filter("band", lo=-1, hi=1); made.append(band)
        fr.same_bits(_arrays(api, band), fr.filter_ref(R, fr.opts(fr.BAND, -1, 1))[0], "band of C")
        s = dc.add(t, 1.0, 0.5); made.append(s)
        sr.same_bits(_arrays(api, s), ad.add_ref(1.0, R, 0.5, sr.transpose(R)), "C + C^T / 2")
        if mode == "sum":                                            # (the last duplicate alone is no stiffness matrix)
            b = rng.standard_normal(M)
            pre = api.assemble_coo(M, M, rows, cols, vals, duplicates=mode); made.append(pre)
            assert pre.ilu0().zeroPivot < 0
            xs, info = dc.cg(b, precond=pre, tol=1e-10, maxiter=200)
            assert info.status == api.SPMV_KRYLOV_CONVERGED and info.iterations < 60
            dense = sr.dense(R)
            assert np.linalg.norm(dense @ xs - b) <= 1e-8 * np.linalg.norm(b)
            h = dc.amg(coarseRows=8); made.append(h)
            xa, ia = dc.cg(b, precond=h, tol=1e-10, maxiter=200)
            assert ia.status == api.SPMV_KRYLOV_CONVERGED and np.linalg.norm(dense @ xa - b) <= 1e-8 * np.linalg.norm(b)
    finally:
        for m in made[::-1]:
            m.free()
        dc.free()


# ---------------------------------------------------------------------------------------------------------- 9 refresh
@functools.lru_cache(maxsize=None)
def _big_list():
    """600 000 triplets on 60 000 rows, 17 columns around the diagonal: more than 2^18 distinct entries, so the formats
    are eligible"""
    rng = np.random.default_rng(3710)
    M, n = 60_000, 600_000
    rows = rng.integers(0, M, n)
    cols = (rows + rng.integers(-8, 9, n)) % M
    rows[rng.random(n) < 0.02] = -1
    return M, rows, cols, si.order_values(rng, n), si.order_values(rng, n)


@pytest.mark.parametrize("mode", MODES)
def test_refresh_gives_reference_bits_in_place_and_the_built_formats_follow(api, oracle, mode):
    import torch
    M, rows, cols, vals, new = _big_list()
    ref = cr.assemble_ref(M, M, rows, cols, vals, mode)
    assert ref[1]["nnzC"] >= si.AUTO_MIN_NNZ and ref[1]["duplicates"] > 50_000 and ref[1]["maxRun"] >= 4
    dc = api.assemble_coo(M, M, rows, cols, vals, duplicates=mode)
    try:
        _compare(api, dc, ref, f"big ({mode})")
        where = _addresses(dc)
        x = si.order_values(np.random.default_rng(6), M)
        dx, dy = api.DeviceVector(M).up(x), api.DeviceVector(M)
        api.build_stripes(dc, deterministic=1)
        api.build_tiles(dc, deterministic=True)
        R = ref[0]
        for launcher in ("hipSpMVStripesCSR", "hipSpMVTilesCSR", ROWS):
            dy.poison()
            api.spmv(launcher, dc, dx, dy)
            assert_same_bits(dy.down(), oracle.csr_serial(R[2], R[3], R[4], x), f"{launcher} before the refresh")
        # the assembly allocates nothing at a refresh: the ledger counts what values_changed() alone asks for
        tv = torch.from_numpy(new).cuda()
        dc.values_changed()                                          # (a format builds its value map at its first refresh)
        api.alloc_refuse(-1)
        dc.values_changed()
        plain = int(api.alloc_stats().calls)
        api.alloc_refuse(-1)
        dc.assemble_refresh(tv)
        assert int(api.alloc_stats().calls) == plain
        want = cr.refresh_ref(R, ref[2], new, mode)
        _compare(api, dc, (want,) + ref[1:], f"big refreshed ({mode})", refreshed=True)
        assert _addresses(dc) == where
        for launcher in ("hipSpMVStripesCSR", "hipSpMVTilesCSR", ROWS):
            dy.poison()
            api.spmv(launcher, dc, dx, dy)
            assert_same_bits(dy.down(), oracle.csr_serial(want[2], want[3], want[4], x), f"{launcher} after the refresh")
        dx.free()
        dy.free()
    finally:
        dc.free()


@pytest.mark.parametrize("mode", MODES)
def test_a_transpose_and_a_hierarchy_refresh_from_a_refreshed_assembly(api, mode):
    M, rows, cols, vals = _q1_triplets((9, 8, 7))
    new = vals * np.random.default_rng(3711).uniform(1.0, 2.0, vals.size)
    ref = cr.assemble_ref(M, M, rows, cols, vals, mode)
    dc = api.assemble_coo(M, M, rows, cols, vals, duplicates=mode)
    fresh = api.assemble_coo(M, M, rows, cols, new, duplicates=mode, keep_map=False)
    t, h, hf = dc.transpose(), dc.amg(coarseRows=8), fresh.amg(coarseRows=8)
    try:
        dc.assemble_refresh(new)
        want = cr.refresh_ref(ref[0], ref[2], new, mode)
        _compare(api, dc, (want,) + ref[1:], f"refreshed ({mode})", refreshed=True)
        cr.same_bits(_arrays(api, fresh), want, "a fresh assembly of the new values")
        t.refresh_from(dc)
        sr.same_bits(_arrays(api, t), sr.transpose(want), "the transpose refreshed from C")
        h.refresh_from(dc)
        r = np.random.default_rng(7).standard_normal(M)
        assert_same_bits(h.apply(r), hf.apply(r), "the refreshed hierarchy's cycle is a fresh hierarchy's")
        # the plain value calls work as on any derived handle
        dc.update_values(ref[0][4])
        cr.same_bits(_arrays(api, dc), ref[0], "update_values on an assembled handle")
    finally:
        for m in (hf, h, t, fresh, dc):
            m.free()


# ---------------------------------------------------------------------------------------------------------- 10 to_coo
def _adopt(api, A, irp_bytes):
    M, N, IRP, JA, AS = A
    bufs = [api.DeviceBuffer(irp_bytes * (M + 1)).up(IRP.astype(np.uint64 if irp_bytes == 8 else np.uint32)),
            api.DeviceBuffer(4 * JA.size).up(JA.astype(np.uint32)), api.DeviceBuffer(8 * JA.size).up(AS)]
    dm = api.DeviceMatrix()
    dm.keep = bufs
    assert api.lib.spmvHipAdoptCSR(P(dm.handle), M, N, JA.size, bufs[0].ptr, irp_bytes, bufs[1].ptr, bufs[2].ptr, None) == 0
    return dm


@pytest.mark.parametrize("mode", MODES)
def test_to_coo_of_every_kind_of_handle_and_back(api, mode):
    rng = np.random.default_rng(3712)
    lap = sr.laplacian7(7, 6, 5, lambda r, n: si.order_values(r, n))
    unit = lap[:4] + (np.full(lap[3].size, -1.5),)
    messy = sr.random_csr(rng, 80, 60, rng.integers(0, 40, 80))                 # unsorted rows, repeats
    handles = {"uploaded": (_up(api, lap), lap), "adopted 4": (_adopt(api, lap, 4), lap), "adopted 8": (_adopt(api, messy, 8), messy),
               "unit": (_up(api, unit), unit), "unsorted": (_up(api, messy), messy), "empty": (_up(api, (3, 4, np.zeros(4, np.uint64), np.zeros(0, np.uint64), np.zeros(0))),
                                                                                         (3, 4, np.zeros(4, np.uint64), np.zeros(0, np.uint64), np.zeros(0)))}
    da, db = handles["unsorted"][0], _up(api, sr.random_csr(rng, 60, 30, 5))
    prod = da.multiply(db)
    handles["product"] = (prod, _arrays(api, prod))
    try:
        v = C.c_double()
        assert api.lib.spmvHipUnitValue(P(handles["unit"][0].handle), P(v)) == 1
        for kind, (dm, A) in handles.items():
            got, want = dm.to_coo(), cr.to_coo_ref(A)
            assert [g.dtype for g in got] == [np.uint32, np.uint32, np.float64]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{kind}: indices"
            assert_same_bits(got[2], want[2], f"{kind}: values")
            dc = api.assemble_coo(A[0], A[1], *got, duplicates=mode)
            try:
                ref = cr.assemble_ref(A[0], A[1], *want, mode)
                _compare(api, dc, ref, f"assemble o to_coo, {kind} ({mode})")
                if kind in ("uploaded", "adopted 4", "unit", "product", "empty"):
                    cr.same_bits(_arrays(api, dc), A, f"{kind}: the identity on a handle whose rows ascend strictly")
                else:
                    assert ref[1]["duplicates"] > 0 and int(dc.handle.NZ) < A[3].size
            finally:
                dc.free()
        rows_only = [api.DeviceBuffer(4 * lap[3].size), api.DeviceBuffer(4 * lap[3].size)]
        assert api.lib.spmvHipCsrToCoo(P(handles["uploaded"][0].handle), rows_only[0].ptr, rows_only[1].ptr, None) == 0, "dVal may be NULL"
        assert np.array_equal(rows_only[0].down(np.uint32), cr.to_coo_ref(lap)[0])
        for b in rows_only:
            b.free()
    finally:
        db.free()
        for dm, _ in handles.values():
            dm.free()


# ----------------------------------------------------------------------------------------------------- 11 determinism
def test_two_builds_on_two_streams_give_identical_bytes(api):
    import torch
    rng = np.random.default_rng(3713)
    rows, cols, vals = _random_list(rng, 3000, 2000, 200_000)
    vals[rng.integers(0, vals.size, 50)] = np.nan
    got = []
    try:
        for mode in MODES:
            for _ in range(2):
                s = torch.cuda.Stream()
                api.lib.spmvHipSetStream(C.c_void_p(s.cuda_stream))
                dc = api.assemble_coo(3000, 2000, rows, cols, vals, duplicates=mode)
                dc.assemble_refresh(vals)
                api.lib.spmvHipSetStream(None)
                got.append(tuple(a.tobytes() for a in _arrays(api, dc)[2:]))
                dc.free()
            assert got[-1] == got[-2], mode
    finally:
        api.lib.spmvHipSetStream(None)


# --------------------------------------------------------------------------------------------------------- 12 refusals
def test_refusals_leave_dc_and_info_untouched_and_hold_nothing(api, capfd):
    lib = api.lib
    rng = np.random.default_rng(3714)
    n = 1000
    rows, cols, vals = _random_list(rng, 50, 40, n)
    bufs = [api.DeviceBuffer(4 * n).up(cr.as_index(rows).astype(np.uint32)), api.DeviceBuffer(4 * n).up(cr.as_index(cols).astype(np.uint32)),
            api.DeviceBuffer(8 * n).up(vals)]
    dr, dc_, dv = (b.ptr for b in bufs)
    good = api.assemble_coo(50, 40, rows, cols, vals)
    nomap = api.assemble_coo(50, 40, rows, cols, vals, keep_map=False)
    plain = _up(api, sr.laplacian7(4, 4, 4))
    ell = api.csr_to_ell_device(plain, False)
    hier = plain.amg(coarseRows=8)
    out, info = api.spmat(), api.spmvCooInfo()
    for obj in (out, info):
        C.memset(C.addressof(obj), 0x5A, C.sizeof(obj))
    before = [_raw(out), _raw(info)]
    OUT, INFO = P(out), P(info)
    live = int(api.alloc_stats().live)
    try:
        def refused(call, who, *msgs, handle=None):
            snap = _raw(handle.handle) if handle is not None else None
            capfd.readouterr()
            assert call() == 1
            err = capfd.readouterr().err
            lines = [l for l in err.splitlines() if l.strip()]
            assert len(lines) == 1 and "libspmvhip" in lines[0], err
            for m in (who,) + msgs:
                assert m in err, (m, err)
            assert [_raw(out), _raw(info)] == before, "dC and info untouched"
            assert snap is None or _raw(handle.handle) == snap, "the handle untouched"
            assert int(api.alloc_stats().live) == live, "nothing held"

        asm, who = lib.spmvHipCooAssemble, "spmvHipCooAssemble"
        sums = api.spmvCooOpts(api.SPMV_COO_SUM, 1)
        refused(lambda: asm(50, 40, n, dr, dc_, dv, P(sums), None, INFO), who, "dC is NULL")
        refused(lambda: asm(50, 40, n, None, dc_, dv, P(sums), OUT, INFO), who, "dRow is NULL")
        refused(lambda: asm(50, 40, n, dr, None, dv, P(sums), OUT, INFO), who, "dCol is NULL")
        refused(lambda: asm(50, 40, n, dr, dc_, None, P(sums), OUT, INFO), who, "dVal is NULL")
        for d in (2, -1, 99):
            refused(lambda: asm(50, 40, n, dr, dc_, dv, P(api.spmvCooOpts(d, 1)), OUT, INFO), who, "duplicates")
        refused(lambda: asm((1 << 32) - 1, 40, n, dr, dc_, dv, P(sums), OUT, INFO), who, "32-bit")
        refused(lambda: asm(50, (1 << 32) - 1, n, dr, dc_, dv, P(sums), OUT, INFO), who, "32-bit")
        refused(lambda: asm(50, 1 << 33, n, dr, dc_, dv, P(sums), OUT, INFO), who, "32-bit")
        refused(lambda: asm(50, 40, IRP32_LIMIT, dr, dc_, dv, P(sums), OUT, INFO), who, "nEntries")
        # out of range, found on the device: two offenders planted, the line names the smaller e with its row and column
        for (e1, r1, c1), (e2, r2, c2) in (((700, 50, 3), (300, 7, 40)), ((5, 1 << 20, 0), (999, 0, 41)), ((998, 49, 40), (999, 50, 39))):
            br, bc = cr.as_index(rows).astype(np.uint32), cr.as_index(cols).astype(np.uint32)
            br[[e1, e2]], bc[[e1, e2]] = [r1, r2], [c1, c2]
            with pytest.raises(IndexError, match=f"^{min(e1, e2)}$"):
                cr.assemble_ref(50, 40, br, bc, vals)
            tmp = [api.DeviceBuffer(4 * n).up(br), api.DeviceBuffer(4 * n).up(bc)]
            live += 2
            e, r, c = min((e1, r1, c1), (e2, r2, c2))
            for mode in (api.SPMV_COO_SUM, api.SPMV_COO_LAST):
                refused(lambda: asm(50, 40, n, tmp[0].ptr, tmp[1].ptr, dv, P(api.spmvCooOpts(mode, 1)), OUT, INFO), "coo", f"entry {e} is ({r}, {c})")
            for b in tmp:
                b.free()
            live -= 2
        ref, who = lib.spmvHipCooAssembleRefresh, "spmvHipCooAssembleRefresh"
        refused(lambda: ref(None, n, dv, INFO), who, "NULL")
        refused(lambda: ref(P(plain.handle), plain.handle.NZ, dv, INFO), who, "was not made by spmvHipCooAssemble", handle=plain)
        refused(lambda: ref(P(hier.handle), n, dv, INFO), who, "hierarchy", handle=hier)
        refused(lambda: ref(P(nomap.handle), n, dv, INFO), who, "keepMap = 0", handle=nomap)
        refused(lambda: ref(P(good.handle), n - 1, dv, INFO), who, "nEntries", handle=good)
        refused(lambda: ref(P(good.handle), n + 1, dv, INFO), who, "nEntries", handle=good)
        refused(lambda: ref(P(good.handle), n, None, INFO), who, "dVal is NULL", handle=good)
        coo, who = lib.spmvHipCsrToCoo, "spmvHipCsrToCoo"
        refused(lambda: coo(P(ell.handle), dr, dc_, dv), who, "ELL", handle=ell)
        refused(lambda: coo(P(hier.handle), dr, dc_, dv), who, "hierarchy", handle=hier)
        refused(lambda: coo(P(good.handle), None, dc_, dv), who, "dRow is NULL", handle=good)
        refused(lambda: coo(P(good.handle), dr, None, dv), who, "dCol is NULL", handle=good)
        refused(lambda: coo(None, dr, dc_, dv), who)
        # (its M >= 2^32 - 1 refusal cannot be reached from here: no maker of a handle accepts that many rows)
        # the handles that were refused are as they were: the good one still refreshes to the reference's bits
        good.assemble_refresh(vals)
        _compare(api, good, cr.assemble_ref(50, 40, rows, cols, vals), "after the refusals", refreshed=True)
    finally:
        for m in (hier, ell, plain, nomap, good):
            m.free()
        for b in bufs:
            b.free()
