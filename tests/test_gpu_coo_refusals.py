"""Every device allocation of spmvHipCooAssemble, spmvHipCooAssembleRefresh and spmvHipCsrToCoo refused in turn
(spmvHipAllocRefuse), and what the call leaves each time -- what include/spmvHip.h promises for the families "makes a handle"
and "refreshes", by the method of tests/test_gpu_alloc_refusals.py on a 200-row case.

The call runs unarmed once (N = the allocations it asks for; its result is compared with tests/coo_ref.py).  Then, for every
n in [0, N), once with that allocation alone refused and once with every allocation from it on:

  1 refusal     refused >= 1, EXIT_FAILURE, a "libspmvhip" line on stderr
  2 ledger      no bad release; a build holds nothing of what it allocated; a refresh holds what it held
  3 outputs     a zeroed destination handle is still zero, a patterned info still holds the pattern; a refreshed handle keeps
                its pattern and its addresses
  4 no sticky   spmvHipVecFill on a scratch vector and a download succeed and show the fill
  5 retry       the same call, unarmed, succeeds with the reference's bits, and the handle is live and complete: SpMV on it
                gives the oracle's bits

The triplet arrays are uploaded before the sweep and the C entry points are called directly, so the only allocations counted
are the library's own."""
import ctypes as C

import numpy as np
import pytest

import coo_ref as cr
import serial_order_inputs as si
from bits import assert_same_bits

pytestmark = pytest.mark.gpu

ROWS = "hipSpMVRowsCSR"
PATTERN = 0xA5
FILL = 0x7FF8DEADBEEF0001
M, N, ENTRIES = 200, 180, 6000
P = C.byref


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.alloc_refuse(-1)
    a.spmvHipInit(0)
    yield a
    a.alloc_refuse(-1)
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _disarm(api):
    yield
    api.alloc_refuse(-1)
    if api.lib.spmvHipDeviceSynchronize() != 0:                      # a device error is a finding: nothing more runs on it
        pytest.exit("the device reports an error after this case: the remaining cases are not run", returncode=3)


def _level(api):
    st = api.alloc_stats()
    return int(st.live), int(st.liveBytes)


def _down(api, ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
    return out


def _arrays(api, h):
    return (int(h.M), int(h.N), _down(api, h.IRP, h.M + 1, np.uint32), _down(api, h.JA, h.NZ, np.uint32), _down(api, h.AS, h.NZ, np.float64))


def _addresses(h):
    return tuple(C.cast(p, C.c_void_p).value for p in (h.IRP, h.JA, h.AS)) + (int(h.M), int(h.N), int(h.NZ))


def _patterned(kind):
    s = kind()
    C.memset(C.addressof(s), PATTERN, C.sizeof(s))
    return s


def _is_patterned(s):
    return C.string_at(C.addressof(s), C.sizeof(s)) == bytes([PATTERN]) * C.sizeof(s)


def _is_zero(s):
    return C.string_at(C.addressof(s), C.sizeof(s)) == bytes(C.sizeof(s))


def _no_sticky_error(api, scratch):
    assert api.lib.spmvHipVecFill(scratch.ptr, scratch.n, FILL) == 0, "the next, unrelated call is judged on its own"
    assert np.all(scratch.down().view(np.uint64) == FILL)


def _live_and_complete(api, oracle, h, R, what):
    dm = api.DeviceMatrix()
    dm.handle = h
    x = si.order_values(np.random.default_rng(8), int(h.N))
    dx, dy = api.DeviceVector(x.size).up(x), api.DeviceVector(int(h.M))
    try:
        dy.poison()
        api.spmv(ROWS, dm, dx, dy)
        assert_same_bits(dy.down(), oracle.csr_serial(R[2], R[3], R[4], x), what)
    finally:
        dm.handle = api.spmat()                                      # (the caller frees h)
        dx.free()
        dy.free()


@pytest.fixture(scope="module")
def case(api):
    rng = np.random.default_rng(3800)
    rows, cols = rng.integers(0, M, ENTRIES), rng.integers(0, N, ENTRIES)
    rows[rng.random(ENTRIES) < 0.05] = -1
    rows[rows == 0] = 1                                              # (an empty first row)
    vals, new = si.order_values(rng, ENTRIES), si.order_values(rng, ENTRIES)
    bufs = dict(rows=api.DeviceBuffer(4 * ENTRIES).up(cr.as_index(rows).astype(np.uint32)),
                cols=api.DeviceBuffer(4 * ENTRIES).up(cr.as_index(cols).astype(np.uint32)),
                vals=api.DeviceBuffer(8 * ENTRIES).up(vals), new=api.DeviceBuffer(8 * ENTRIES).up(new))
    scratch = api.DeviceVector(64)
    yield dict(rows=rows, cols=cols, vals=vals, new=new, bufs=bufs, scratch=scratch)
    scratch.free()
    for b in bufs.values():
        b.free()


def _armed(n, from_then_on):
    return f"allocation {n}" + (" and every later one" if from_then_on else "") + " refused"


@pytest.mark.parametrize("keep_map", [1, 0])
@pytest.mark.parametrize("mode", ["sum", "last"])
def test_every_allocation_of_the_assembly_refused_in_turn(api, oracle, capfd, case, mode, keep_map):
    lib, b = api.lib, case["bufs"]
    opts = api.spmvCooOpts(cr.MODES[mode], keep_map)
    ref = cr.assemble_ref(M, N, case["rows"], case["cols"], case["vals"], mode)

    def call(out, info):
        return lib.spmvHipCooAssemble(M, N, ENTRIES, b["rows"].ptr, b["cols"].ptr, b["vals"].ptr, P(opts), P(out), P(info))

    level = _level(api)
    twin, info = api.spmat(), api.spmvCooInfo()
    api.alloc_refuse(-1)
    assert call(twin, info) == 0
    total = int(api.alloc_stats().calls)
    cr.same_bits(_arrays(api, twin), ref[0], "unarmed")
    assert lib.hipFreeSpmat(P(twin)) == 0 and _level(api) == level
    assert total >= 12, "the row pointers, the keys, the sort, the counts, the arrays, the row blocks, the unit flag"
    print(f"spmvHipCooAssemble {mode} keepMap={keep_map}: {total} allocations")
    for n in range(total):
        for from_then_on in (False, True):
            what = _armed(n, from_then_on)
            out, info = api.spmat(), _patterned(api.spmvCooInfo)
            capfd.readouterr()
            with api.alloc_refused(n, from_then_on):
                rc = call(out, info)
                st = api.alloc_stats()
            err = capfd.readouterr().err
            assert st.refused >= 1 and rc == 1 and "libspmvhip" in err, (what, rc, err)
            assert st.badFrees == 0 and _level(api) == level, f"{what}: nothing the call allocated is still held"
            assert _is_zero(out) and _is_patterned(info), f"{what}: dC and info are not written"
            _no_sticky_error(api, case["scratch"])
            assert call(out, info) == 0, f"{what}: the same call made again succeeds"
            try:
                cr.same_bits(_arrays(api, out), ref[0], f"{what}: retry")
                assert (info.nnzC, info.skipped, info.maxRun) == (ref[1]["nnzC"], ref[1]["skipped"], ref[1]["maxRun"])
                if n == total - 1:
                    _live_and_complete(api, oracle, out, ref[0], f"{what}: SpMV on the retried handle")
            finally:
                assert lib.hipFreeSpmat(P(out)) == 0
            assert _level(api) == level


@pytest.mark.parametrize("mode", ["sum", "last"])
def test_every_allocation_of_the_refresh_refused_in_turn(api, oracle, capfd, case, mode):
    lib, b = api.lib, case["bufs"]
    opts = api.spmvCooOpts(cr.MODES[mode], 1)
    ref = cr.assemble_ref(M, N, case["rows"], case["cols"], case["vals"], mode)
    values = {"vals": ref[0], "new": cr.refresh_ref(ref[0], ref[2], case["new"], mode)}
    h, first = api.spmat(), api.spmvCooInfo()
    assert lib.spmvHipCooAssemble(M, N, ENTRIES, b["rows"].ptr, b["cols"].ptr, b["vals"].ptr, P(opts), P(h), P(first)) == 0
    assert lib.spmvHipBuildSell(P(h)) == 0                            # a built format rides along
    try:
        level, where = _level(api), _addresses(h)
        api.alloc_refuse(-1)
        assert lib.spmvHipCooAssembleRefresh(P(h), ENTRIES, b["new"].ptr, None) == 0
        total = int(api.alloc_stats().calls)
        cr.same_bits(_arrays(api, h), values["new"], "unarmed")
        assert total >= 1 and _level(api) == level, "the unit flag of the new values; the assembly itself asks for nothing"
        print(f"spmvHipCooAssembleRefresh {mode}: {total} allocations")
        now = "new"
        for n in range(total):
            for from_then_on in (False, True):
                what = _armed(n, from_then_on)
                nxt = "vals" if now == "new" else "new"
                info = _patterned(api.spmvCooInfo)
                capfd.readouterr()
                with api.alloc_refused(n, from_then_on):
                    rc = lib.spmvHipCooAssembleRefresh(P(h), ENTRIES, b[nxt].ptr, P(info))
                    st = api.alloc_stats()
                err = capfd.readouterr().err
                assert st.refused >= 1 and rc == 1 and "libspmvhip" in err, (what, rc, err)
                assert st.badFrees == 0 and _level(api) == level, f"{what}: the handle holds what it held"
                assert _is_patterned(info) and _addresses(h) == where, f"{what}: info is not written, pattern and addresses stay"
                got = _arrays(api, h)
                assert np.array_equal(got[2], ref[0][2]) and np.array_equal(got[3], ref[0][3]), f"{what}: the pattern"
                _no_sticky_error(api, case["scratch"])
                assert lib.spmvHipCooAssembleRefresh(P(h), ENTRIES, b[nxt].ptr, P(info)) == 0, f"{what}: the repeated call completes it"
                cr.same_bits(_arrays(api, h), values[nxt], f"{what}: retry")
                assert info.nnzC == ref[1]["nnzC"] and _addresses(h) == where and _level(api) == level
                now = nxt
        _live_and_complete(api, oracle, h, values[now], "SpMV after the sweep")
        x = si.order_values(np.random.default_rng(9), N)
        dm = api.DeviceMatrix()
        dm.handle = h
        dx, dy = api.DeviceVector(N).up(x), api.DeviceVector(M)
        try:
            dy.poison()
            api.spmv("hipSpMVRowsSELL", dm, dx, dy)
            assert_same_bits(dy.down(), oracle.csr_serial(values[now][2], values[now][3], values[now][4], x), "the built format followed")
        finally:
            dm.handle = api.spmat()
            dx.free()
            dy.free()
    finally:
        assert lib.hipFreeSpmat(P(h)) == 0


def test_to_coo_asks_for_no_allocation(api, capfd, case):
    """with every allocation refused from the first on the call still succeeds: it has none to make"""
    lib, b = api.lib, case["bufs"]
    ref = cr.assemble_ref(M, N, case["rows"], case["cols"], case["vals"])
    h = api.spmat()
    assert lib.spmvHipCooAssemble(M, N, ENTRIES, b["rows"].ptr, b["cols"].ptr, b["vals"].ptr, None, P(h), None) == 0
    nz = int(h.NZ)
    out = [api.DeviceBuffer(4 * nz), api.DeviceBuffer(4 * nz), api.DeviceBuffer(8 * nz)]
    try:
        level = _level(api)
        capfd.readouterr()
        with api.alloc_refused(0, True):
            rc = lib.spmvHipCsrToCoo(P(h), out[0].ptr, out[1].ptr, out[2].ptr)
            st = api.alloc_stats()
        assert rc == 0 and st.calls == 0 and st.refused == 0 and "libspmvhip" not in capfd.readouterr().err
        assert _level(api) == level
        want = cr.to_coo_ref(ref[0])
        assert np.array_equal(out[0].down(np.uint32), want[0]) and np.array_equal(out[1].down(np.uint32), want[1])
        assert_same_bits(out[2].down(np.float64), want[2], "the triplets")
        _no_sticky_error(api, case["scratch"])
    finally:
        for o in out:
            o.free()
        assert lib.hipFreeSpmat(P(h)) == 0
