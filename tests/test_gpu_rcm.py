"""spmvHipRcmCSR on the device: dPerm is, word for word, the permutation of the serial queue loop of include/spmvHip.h
(tests/rcm_ref.py) -- a function of the pattern and the options alone -- for both starts, forward and reversed, at
T = 0, 4, 64 and 1024, on every small case: empty, tiny, around a workgroup's size, one-directional, without a diagonal,
unsorted with repeats, a clique and a star on the wavefront path, a shuffled path, two shuffled grids, several components
with isolated vertices, a random graph.  The launches and read-backs of the path pinned at both ends of T, and a longer
path whose run passes the step limit of one launch.  The figures of spmvRcmInfo against the reference, the outputs in poisoned
buffers, the permutation through spmvHipCsrPermute / hipSpMVRowsCSR / hipSpILU0CSR, the Python layer, every refusal, and
the ledger after twenty calls."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as cr
import rcm_ref as rr
from exact_ref import check_any_order

pytestmark = pytest.mark.gpu

POISON = 0xA5A5A5A5
PAD = 7
NAME = "spmvHipRcmCSR"
ROWS = "hipSpMVRowsCSR"
THRESHOLDS = (0, 4, 64, 1024)
SMALL = rr.small_cases()
NOT_SYMMETRIC = ("bidiagonal", "no_diagonal", "unsorted_repeats", "clique_star")
_REF = {}


def _ref(name, start, forward, passes=0):
    """the loop's (perm, info), computed once per (case, start, passes): the forward order is the reversed one read backwards"""
    key = (name, start, passes)
    if key not in _REF:
        M, IRP, JA = SMALL[name]
        _REF[key] = rr.rcm_loop(M, IRP, JA, start, passes, False)
    perm, info = _REF[key]
    return (perm[::-1] if forward else perm), info


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.set_variant(NAME, 1024)


def _upload(api, M, IRP, JA, AS=None):
    return api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, np.ones(JA.size) if AS is None else AS))


def _rcm(api, dm, M, start, forward, passes=0, want_perm=True, opts=True):
    """(rc, perm, info): the output lives in a poisoned buffer PAD words longer than M"""
    buf = api.DeviceBuffer(4 * (M + PAD)).up(np.full(M + PAD, POISON, dtype=np.uint32)) if want_perm else None
    o, info = api.spmvRcmOpts(start, passes, int(forward)), api.spmvRcmInfo()
    try:
        rc = api.lib.spmvHipRcmCSR(C.byref(dm.handle), C.byref(o) if opts else None, buf.ptr if buf else None, C.byref(info))
        got = buf.down(np.uint32) if buf else None
    finally:
        if buf:
            buf.free()
    if got is not None:
        assert np.all(got[M:] == POISON), "a word past M was written"
        got = got[:M]
    return rc, got, info


def _info_tuple(i):
    return (i.components, i.levels, i.startBfs, i.maxFrontier, i.longRows, i.symmetric, i.bandwidthBefore, i.bandwidthAfter)


def _check_info(name, info, ref_info, perm_ref, start):
    M, IRP, JA = SMALL[name]
    deg = np.array([len(a) for a in rr.adjacency(M, IRP, JA)], dtype=np.int64)
    assert (info.components, info.levels, info.maxFrontier) == (ref_info["components"], ref_info["levels"], ref_info["maxFrontier"]), name
    assert info.startBfs == (ref_info["startBfs"] if start == rr.PERIPHERAL else 0), name
    assert info.longRows == int((deg > 64).sum()), name
    assert info.symmetric == (0 if name in NOT_SYMMETRIC else 1), name
    assert info.bandwidthBefore == rr.bandwidth(M, IRP, JA) and info.bandwidthAfter == rr.bandwidth(M, IRP, JA, perm_ref), name


@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("name", list(SMALL))
def test_small_cases_equal_the_loop(api, name, T):
    M, IRP, JA = SMALL[name]
    api.set_variant(NAME, T)
    dm = _upload(api, M, IRP, JA)
    try:
        for start, forward in rr.CONFIGS:
            perm_ref, ref_info = _ref(name, start, forward)
            rc, perm, info = _rcm(api, dm, M, start, forward)
            what = f"{name} T={T} start={start} forward={forward}"
            assert rc == 0, what
            assert np.array_equal(perm, perm_ref), what
            _check_info(name, info, ref_info, perm_ref, start)
            print(f"{what}: levels {info.levels}, launches {info.launches}, checks {info.hostChecks}, long rows {info.longRows}, "
                  f"bandwidth {info.bandwidthBefore} -> {info.bandwidthAfter}, {info.ms:.2f} ms")
            if M:
                assert info.launches >= 1 and info.hostChecks >= 1
            if name == "path3000" and T == 1024:
                assert info.launches < info.levels / 8, "the thin levels run inside one launch"
            if name in ("star1500", "clique_star"):                # (counted from the degrees: that these vertices' neighbours come out
                assert info.longRows >= 1                          # right, which only the wavefront walk visits, is the equality above)
    finally:
        dm.free()


@pytest.mark.parametrize("name", ["grid40x30", "three_components", "star1500", "path3000"])
def test_the_threshold_moves_levels_between_the_paths_and_no_word(api, name):
    """launches and hostChecks are the two figures that may depend on T: more of both the fewer levels run in the workgroup"""
    M, IRP, JA = SMALL[name]
    dm = _upload(api, M, IRP, JA)
    try:
        seen = {}
        for T in THRESHOLDS:
            api.set_variant(NAME, T)
            rc, perm, info = _rcm(api, dm, M, rr.PERIPHERAL, False)
            assert rc == 0
            seen[T] = (perm, _info_tuple(info), info.launches, info.hostChecks)
        for T in THRESHOLDS[1:]:
            assert np.array_equal(seen[T][0], seen[0][0]) and seen[T][1] == seen[0][1], T
        print(name, {T: seen[T][2:] for T in THRESHOLDS})
        assert seen[0][3] >= seen[4][3] >= seen[64][3] >= seen[1024][3]
        if name != "star1500":
            assert seen[0][3] > seen[1024][3]
        if name == "grid40x30":                                   # levels of up to 30 vertices: 4 < some of them <= 64
            assert seen[4][3] > seen[64][3]
        if name == "path3000":                                    # 3 000 levels of one vertex, two search runs and the ordering
            for T in THRESHOLDS[1:]:                              # one launch of the workgroup, and the read-back of the figures
                assert seen[T][2:] == (11, 2), T
            assert seen[0][3] == 4 * 3000 + 2, "a read-back per search level, two per ordering level"
            assert seen[0][2] > 8 * 3000
    finally:
        dm.free()


def test_a_run_that_reaches_its_step_limit_is_launched_again(api):
    """a path of 25 000 vertices is 75 000 thin levels, two search runs and the ordering: more than the 65 536 steps one launch
    of the workgroup takes, so the launch returns with its state and a second one carries on from it"""
    M, IRP, JA = rr.path(25000, seed=35)
    perm_ref, ref_info = rr.rcm_levels(M, IRP, JA)
    dm = _upload(api, M, IRP, JA)
    try:
        rc, perm, info = _rcm(api, dm, M, rr.PERIPHERAL, False)
        assert rc == 0 and np.array_equal(perm, perm_ref)
        assert (info.levels, info.startBfs, info.bandwidthAfter) == (M, 2, 1) and ref_info["levels"] == M
        print(f"path25000: launches {info.launches}, checks {info.hostChecks}, {info.ms:.2f} ms")
        assert info.hostChecks == 3 and info.launches == 12, "two launches of the workgroup where the path of 3 000 takes one"
    finally:
        dm.free()


@pytest.mark.parametrize("passes", [1, 2, 8])
def test_the_passes_of_the_start_search(api, passes):
    for name in ("random2000", "no_diagonal", "grid12x10x8"):
        M, IRP, JA = SMALL[name]
        perm_ref, ref_info = _ref(name, rr.PERIPHERAL, False, passes)
        dm = _upload(api, M, IRP, JA)
        try:
            rc, perm, info = _rcm(api, dm, M, rr.PERIPHERAL, False, passes)
            assert rc == 0 and np.array_equal(perm, perm_ref), (name, passes)
            assert info.startBfs == ref_info["startBfs"], (name, passes)
        finally:
            dm.free()


def test_a_second_call_null_outputs_and_null_options(api):
    for name in ("three_components", "unsorted_repeats", "random0", "random1"):
        M, IRP, JA = SMALL[name]
        perm_ref, _ = _ref(name, rr.PERIPHERAL, False)
        dm = _upload(api, M, IRP, JA)
        try:
            rc, perm, info = _rcm(api, dm, M, rr.PERIPHERAL, False)
            rc2, perm2, info2 = _rcm(api, dm, M, rr.PERIPHERAL, False)
            assert rc == 0 and rc2 == 0 and np.array_equal(perm, perm2) and np.array_equal(perm, perm_ref), name
            rc3, none, info3 = _rcm(api, dm, M, rr.PERIPHERAL, False, want_perm=False)
            assert rc3 == 0 and none is None and _info_tuple(info3) == _info_tuple(info) == _info_tuple(info2), name
            rc4, perm4, info4 = _rcm(api, dm, M, rr.MIN_DEGREE, True, opts=False)        # opts == NULL: PERIPHERAL, reversed
            assert rc4 == 0 and np.array_equal(perm4, perm_ref) and _info_tuple(info4) == _info_tuple(info), name
            if M == 0:
                assert _info_tuple(info)[:5] == (0, 0, 0, 0, 0) and info.launches == 0
        finally:
            dm.free()


def test_column_ids_past_m_of_an_adopted_array_are_no_vertices(api):
    M, IRP, JA = SMALL["random257"]
    rng = np.random.default_rng(61)
    rows = np.repeat(np.arange(M), np.diff(IRP.astype(np.int64)))
    extra = rng.integers(0, M, 40)
    rows2, cols2 = np.r_[rows, extra], np.r_[JA.astype(np.int64), M + rng.integers(0, 1000, 40)]
    o = np.lexsort((cols2, rows2))
    IRP2, JA2 = cr.csr_of(M, rows2[o], cols2[o])
    perm_ref, ref_info = rr.rcm_loop(M, IRP2, JA2)
    assert np.array_equal(perm_ref, rr.rcm_loop(M, IRP, JA)[0]), "the reference skips them"
    arrays = (IRP2.astype(np.uint32), JA2.astype(np.uint32), np.ones(JA2.size))
    bufs = [api.DeviceBuffer(v.nbytes).up(v) for v in arrays]
    dm = api.DeviceMatrix()
    try:
        assert api.lib.spmvHipAdoptCSR(C.byref(dm.handle), M, M, JA2.size, bufs[0].ptr, 4, bufs[1].ptr, bufs[2].ptr, None) == 0
        for T in (0, 1024):
            api.set_variant(NAME, T)
            rc, perm, info = _rcm(api, dm, M, rr.PERIPHERAL, False)
            assert rc == 0 and np.array_equal(perm, perm_ref)
            assert info.symmetric == 0 and info.components == ref_info["components"]
            assert info.bandwidthBefore == rr.bandwidth(M, IRP2, JA2) and info.bandwidthAfter == rr.bandwidth(M, IRP2, JA2, perm_ref)
    finally:
        dm.free()
        for b in bufs:
            b.free()


@pytest.mark.parametrize("name", ["laplacian12x10x8", "grid40x30", "unsorted_repeats", "no_diagonal"])
def test_the_permutation_through_permute_spmv_and_ilu0(api, name):
    """rcm -> permute -> SpMV on B with the permuted x -> y permuted back: the rows' sums of A x in another order"""
    M, IRP, JA = SMALL[name]
    rng = np.random.default_rng(62)
    laplacian = name in ("laplacian12x10x8", "grid40x30")
    rows = np.repeat(np.arange(M), np.diff(IRP.astype(np.int64)))
    AS = np.where(rows == JA.astype(np.int64), 8.0, -1.0) if laplacian else rng.uniform(-1, 1, JA.size)
    x = rng.uniform(-1, 1, M)
    dm = _upload(api, M, IRP, JA, AS)
    ordering = dm.rcm()
    b = dm.permute(ordering)
    try:
        perm = ordering.perm.down(np.uint32)
        assert np.array_equal(np.sort(perm), np.arange(M)) and np.array_equal(perm, _ref(name, rr.PERIPHERAL, False)[0])
        xb = api.permute_vector(ordering, x)
        assert np.array_equal(xb, x[perm])
        dx, dy = api.DeviceVector(M).up(xb), api.DeviceVector(M)
        dy.poison()
        api.spmv(ROWS, b, dx, dy)
        y = api.permute_vector(ordering, dy.down(), inverse=True)
        dx.free()
        dy.free()
        check_any_order(IRP, JA, AS, x, y, name)
        hb = b.handle
        assert rr.bandwidth(M, _down(api, hb.IRP, M + 1), _down(api, hb.JA, int(hb.NZ))) == ordering.info.bandwidthAfter, \
            "B's own bandwidth is the figure of the call"
        if laplacian:
            assert b.ilu0().zeroPivot < 0, "a sorted, repeat-free source gives a B that hipSpILU0CSR accepts"
    finally:
        b.free()
        ordering.free()
        dm.free()


def _down(api, ptr, n):
    out = np.empty(n, dtype=np.uint32)
    if n:
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
    return out


def test_python_rcm(api):
    import torch
    M, IRP, JA = SMALL["three_components"]
    dm = _upload(api, M, IRP, JA)
    try:
        o = dm.rcm()
        assert np.array_equal(o.perm.down(np.uint32), _ref("three_components", rr.PERIPHERAL, False)[0]) and o.info.components == 9
        o.free()
        assert o.perm is None
        o = dm.rcm(start="min_degree", forward=True, as_torch=True)
        assert o.perm.dtype == torch.int32 and o.perm.is_cuda
        assert np.array_equal(o.perm.cpu().numpy().view(np.uint32), _ref("three_components", rr.MIN_DEGREE, True)[0])
        assert o.info.startBfs == 0
        b = dm.permute(o)
        assert int(b.handle.M) == M
        b.free()
        o.free()
        o = dm.rcm(max_passes=1)
        assert np.array_equal(o.perm.down(np.uint32), _ref("three_components", rr.PERIPHERAL, False, 1)[0])
        o.free()
        with pytest.raises(api.SpmvHipError):
            dm.rcm(start="colour")
    finally:
        dm.free()


def test_refusals_leave_the_outputs_untouched(api, capfd):
    M, IRP, JA = SMALL["random257"]
    dm = _upload(api, M, IRP, JA)
    rect = api.spMatCpyCSR(api.HostCSR(3, 4, np.array([0, 1, 2, 3], dtype=np.uint64), np.array([0, 1, 3], dtype=np.uint64), np.ones(3)))
    ell = api.csr_to_ell_device(dm, False)
    buf = api.DeviceBuffer(4 * M).up(np.full(M, POISON, dtype=np.uint32))
    info = api.spmvRcmInfo()
    C.memset(C.addressof(info), 0xA5, C.sizeof(info))
    before = C.string_at(C.addressof(info), C.sizeof(info))
    try:
        bad_start, good, empty = api.spmvRcmOpts(2, 0, 0), api.spmvRcmOpts(rr.PERIPHERAL, 0, 0), api.spmat()
        capfd.readouterr()
        for handle, opts in ((dm.handle, bad_start), (rect.handle, good), (ell.handle, good), (empty, good)):
            assert api.lib.spmvHipRcmCSR(C.byref(handle), C.byref(opts), buf.ptr, C.byref(info)) == 1
        assert api.lib.spmvHipRcmCSR(None, C.byref(good), buf.ptr, C.byref(info)) == 1
        err = capfd.readouterr().err
        assert "unknown start" in err and "not square" in err and "ELL" in err
        assert C.string_at(C.addressof(info), C.sizeof(info)) == before, "info was written"
        assert buf.down(np.uint32).tobytes() == np.full(M, POISON, dtype=np.uint32).tobytes(), "dPerm was written"
        assert api.lib.spmvHipSetVariant(NAME.encode(), -1) == 1
        assert api.lib.spmvHipSetVariant(NAME.encode(), 5000) == 0, "clamped to 1024"
        rc, perm, _ = _rcm(api, dm, M, rr.PERIPHERAL, False)
        assert rc == 0 and np.array_equal(perm, _ref("random257", rr.PERIPHERAL, False)[0])
    finally:
        buf.free()
        for d in (ell, rect, dm):
            d.free()


def test_twenty_calls_leave_the_ledger_where_it_was(api):
    M, IRP, JA = SMALL["no_diagonal"]
    dm = _upload(api, M, IRP, JA)
    try:
        for T in (0, 1024):
            api.set_variant(NAME, T)
            _rcm(api, dm, M, rr.PERIPHERAL, False)                   # (the library's own workspaces, if any, are made here)
            st = api.alloc_stats()
            before = (int(st.live), int(st.liveBytes), int(st.badFrees))
            for k in range(20):
                rc, _, _ = _rcm(api, dm, M, k % 2, bool(k & 2), want_perm=False)
                assert rc == 0
            st = api.alloc_stats()
            assert (int(st.live), int(st.liveBytes), int(st.badFrees)) == before
    finally:
        dm.free()
