"""Every device allocation of spmvHipRcmCSR refused in turn (spmvHipAllocRefuse), at T = 0 and T = 1024, on the case of
three components with isolated vertices -- by the method of tests/test_gpu_alloc_refusals.py.

The call runs unarmed once (N = the allocations it asks for; its words are the reference's).  Then, for every n in [0, N),
once with that allocation alone refused and once with every allocation from it on:

  1 refusal     refused >= 1, EXIT_FAILURE, a "libspmvhip" line on stderr
  2 ledger      no bad release; the library holds what it held before the call
  3 outputs     a patterned info still holds the pattern (dPerm holds nothing to rely on, the header says)
  4 no sticky   spmvHipVecFill on a scratch vector and a download succeed and show the fill
  5 retry       the same call, unarmed, succeeds with the reference's words

A symmetric, sorted pattern walks A's own arrays; the same graph stored one way only builds the pattern of A + A^T, whose
allocations are swept as well."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as cr
import rcm_ref as rr

pytestmark = pytest.mark.gpu

NAME = "spmvHipRcmCSR"
PATTERN = 0xA5
FILL = 0x7FF8DEADBEEF0001
POISON = 0xA5A5A5A5


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.alloc_refuse(-1)
    a.spmvHipInit(0)
    yield a
    a.alloc_refuse(-1)
    a.set_variant(NAME, 1024)
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


def _patterned(kind):
    s = kind()
    C.memset(C.addressof(s), PATTERN, C.sizeof(s))
    return s


def _is_patterned(s):
    return C.string_at(C.addressof(s), C.sizeof(s)) == bytes([PATTERN]) * C.sizeof(s)


def _one_way(case):
    """the same graph with only the entries on and above the diagonal stored"""
    M, IRP, JA = case
    rows = np.repeat(np.arange(M), np.diff(IRP.astype(np.int64)))
    keep = JA.astype(np.int64) >= rows
    return (M,) + cr.csr_of(M, rows[keep], JA.astype(np.int64)[keep])


@pytest.mark.parametrize("T", [0, 1024])
@pytest.mark.parametrize("stored", ["symmetric", "one_way"])
def test_every_allocation_refused_in_turn(api, capfd, stored, T):
    case = rr.three_components()
    M, IRP, JA = case if stored == "symmetric" else _one_way(case)
    perm_ref, ref_info = rr.rcm_loop(*case)
    assert np.array_equal(perm_ref, rr.rcm_loop(M, IRP, JA)[0])
    api.set_variant(NAME, T)
    dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, np.ones(JA.size)))
    buf, scratch = api.DeviceBuffer(4 * M), api.DeviceVector(64)
    opts = api.spmvRcmOpts(rr.PERIPHERAL, 0, 0)

    def call(info):
        buf.up(np.full(M, POISON, dtype=np.uint32))
        return api.lib.spmvHipRcmCSR(C.byref(dm.handle), C.byref(opts), buf.ptr, C.byref(info))

    try:
        level = _level(api)
        info = api.spmvRcmInfo()
        api.alloc_refuse(-1)
        assert call(info) == 0
        total = int(api.alloc_stats().calls)
        assert np.array_equal(buf.down(np.uint32), perm_ref) and info.components == ref_info["components"]
        assert info.symmetric == (1 if stored == "symmetric" else 0)
        assert total >= 8 and _level(api) == level, "the rows of the entries, the degrees, the flags, the lists, the state, the sorts"
        print(f"spmvHipRcmCSR {stored} T={T}: {total} allocations, {info.launches} launches, {info.hostChecks} read-backs")
        for n in range(total):
            for from_then_on in (False, True):
                what = f"allocation {n}" + (" and every later one" if from_then_on else "") + " refused"
                info = _patterned(api.spmvRcmInfo)
                capfd.readouterr()
                buf.up(np.full(M, POISON, dtype=np.uint32))
                with api.alloc_refused(n, from_then_on):
                    rc = api.lib.spmvHipRcmCSR(C.byref(dm.handle), C.byref(opts), buf.ptr, C.byref(info))
                    st = api.alloc_stats()
                err = capfd.readouterr().err
                assert st.refused >= 1 and rc == 1 and "libspmvhip" in err, (what, rc, err)
                assert st.badFrees == 0 and _level(api) == level, f"{what}: nothing the call allocated is still held"
                assert _is_patterned(info), f"{what}: info is not written"
                assert api.lib.spmvHipVecFill(scratch.ptr, scratch.n, FILL) == 0, f"{what}: the next, unrelated call is judged on its own"
                assert np.all(scratch.down().view(np.uint64) == FILL)
                assert call(info) == 0, f"{what}: the same call made again succeeds"
                assert np.array_equal(buf.down(np.uint32), perm_ref), f"{what}: retry"
                assert info.components == ref_info["components"] and info.levels == ref_info["levels"]
                assert _level(api) == level
    finally:
        scratch.free()
        buf.free()
        dm.free()
