"""The single-precision value form on the device (spmvHipValuesF32, the f32 products): every serial-order
f32 product has the bits of sgemvSerial on A~ = (double)(float)A -- against the host oracle and against hipSpMVRowsCSR on a
handle that was uploaded with the roundings --, the form reports what its rounding did, follows every change of the values,
and leaves every f64 call as it was.  Finite values are compared by bits, infinities by sign, NaN as NaN.  The inputs
(tests/values_f32_ref.py) tell the two storages apart and are order-sensitive: tests/test_values_f32_abi.py shows it."""
import ctypes as C

import numpy as np
import pytest

import serial_order_inputs as si
import values_f32_ref as vr
from conftest import tight_error
from test_gpu_spmm import COL, POISON, ROW, _pack, _padding_poisoned, _unpack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.set_variant("hipSpMVRowsCSR", 2)
    api.lib.spmvHipSetSync(1)


class Handle:
    """a case on the device, uploaded or adopted with 8-byte row pointers; free() gives back what it holds"""

    def __init__(self, api, A, origin="uploaded"):
        M, N, IRP, JA, AS = A[:5]
        self.api, self.bufs = api, []
        if origin == "uploaded":
            self.dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
        else:
            irp, ja, a = IRP.astype(np.uint64), JA.astype(np.uint32), np.ascontiguousarray(AS, dtype=np.float64)
            self.bufs = [api.DeviceBuffer(h.nbytes).up(h) for h in (irp, ja, a)]
            self.dm = api.DeviceMatrix()
            assert api.lib.spmvHipAdoptCSR(C.byref(self.dm.handle), M, N, JA.size, self.bufs[0].ptr, 8, self.bufs[1].ptr, self.bufs[2].ptr,
                                           irp.ctypes.data_as(C.c_void_p)) == 0

    def free(self):
        self.dm.free()
        for b in self.bufs:
            b.free()


def _run(api, launcher, dm, x, M):
    """y of one launcher call, y poisoned before it (vectors of at least one element: an empty one has no address)"""
    dx, dy = api.DeviceVector(max(x.size, 1)), api.DeviceVector(max(M, 1))
    try:
        dx.up(np.r_[x, np.zeros(1)][:max(x.size, 1)])
        dy.poison()
        api.spmv(launcher, dm, dx, dy)
        return dy.down()[:M]
    finally:
        dx.free()
        dy.free()


def _want(oracle, A):
    """sgemvSerial on the roundings"""
    M, N, IRP, JA, AS, x = A
    return oracle.csr_serial(IRP, JA, vr.round32(AS), x) if M else np.zeros(0)


# ---------------------------------------------------------------------------------------------------------- products
@pytest.mark.parametrize("origin", ["uploaded", "adopted-8"])
@pytest.mark.parametrize("name", list(vr.CASES))
def test_rows_f32_is_the_serial_loop_on_the_roundings(api, oracle, name, origin):
    A = vr.case(name)
    M, N, IRP, JA, AS, x = A
    want = _want(oracle, A)
    h = Handle(api, A, origin)
    pre = Handle(api, (M, N, IRP, JA, vr.round32(AS)))                   # uploaded with the roundings: the f64 kernels on A~
    try:
        y64 = _run(api, "hipSpMVRowsCSR", h.dm, x, M)
        pick = api.lib.spmvHipAutoChoiceRows(C.byref(h.dm.handle), None)
        h.dm.values_f32()
        vr.same(_run(api, "hipSpMVRowsCSRf32", h.dm, x, M), want, f"{name}, {origin}: against the oracle on the roundings")
        vr.same(_run(api, "hipSpMVRowsCSR", pre.dm, x, M), want, f"{name}: hipSpMVRowsCSR on the rounded upload")
        # the f64 side is what it was: the same bits, the same pick
        vr.same(_run(api, "hipSpMVRowsCSR", h.dm, x, M), y64, f"{name}, {origin}: the f64 product after the build")
        vr.same(y64, oracle.csr_serial(IRP, JA, AS, x) if M else np.zeros(0), f"{name}, {origin}: the f64 product")
        assert api.lib.spmvHipAutoChoiceRows(C.byref(h.dm.handle), None) == pick
        info = h.dm.values_f32_info()
        assert info.built == 1 and info.unit == 0 and info.refreshes == 0
        assert info.bytes == ((JA.size * 4 + 15) // 16 * 16 + 32 if JA.size else 0)
        assert (info.inexact, info.overflowed, info.flushed, info.firstOverflow) == vr.counts(AS), name
        # released and built again: the same bits
        h.dm.values_f32(False)
        assert h.dm.values_f32_info().built == 0
        h.dm.values_f32()
        h.dm.values_f32()                                                # idempotent
        vr.same(_run(api, "hipSpMVRowsCSRf32", h.dm, x, M), want, f"{name}, {origin}: built again")
    finally:
        h.free()
        pre.free()


@pytest.mark.parametrize("value", [1.0, 0.1])
def test_a_unit_handle_rounds_its_register_value(api, oracle, value):
    A = vr.unit_case(value)
    M, N, IRP, JA, AS, x = A
    h = Handle(api, A)
    try:
        v = C.c_double()
        assert api.lib.spmvHipUnitValue(C.byref(h.dm.handle), C.byref(v)) == 1 and v.value == value
        live = api.alloc_stats().live
        h.dm.values_f32()
        assert api.alloc_stats().live == live, "a unit handle gets no array"
        info = h.dm.values_f32_info()
        assert (info.built, info.unit, info.bytes) == (1, 1, 0)
        assert (info.inexact, info.overflowed, info.flushed, info.firstOverflow) == vr.counts(AS)
        vr.same(_run(api, "hipSpMVRowsCSRf32", h.dm, x, M), _want(oracle, A), f"all {value}")
        Y = h.dm.matmul(np.ascontiguousarray(np.stack([x, 2 * x, -x], axis=1)), values="f32")
        vr.same(Y[:, 0], _want(oracle, A), f"all {value}: SpMM")
    finally:
        h.free()


@pytest.mark.parametrize("name", list(vr.ORDINARY))
def test_warp_per_row_f32_is_the_same_sums_in_another_order(api, oracle, name):
    """the reduction-order contract under the project's tight check (conftest.tight_error): two orders of the same n rounded
    products differ by at most 2 (n - 1) 2^-53 sum |a x|; an empty row is +0.0 exactly"""
    A = vr.case(name)
    M, N, IRP, JA, AS, x = A
    h = Handle(api, A)
    try:
        h.dm.values_f32()
        y = _run(api, "hipSpMVWarpPerRowCSRf32", h.dm, x, M)
        assert not np.isnan(y).any()
        n = int(np.diff(IRP.astype(np.int64)).max())
        err = tight_error(IRP, JA, vr.round32(AS), x, _want(oracle, A), y)
        print(f"{name}: tight error {err:.3e}, bound {2 * n * 2.0 ** -53:.3e}")
        assert err <= 2 * n * 2.0 ** -53
    finally:
        h.free()


def _spmm32(api, dm, X, M, xl, yl, ldx, ldy):
    N, k = X.shape
    hx, hy = _pack(X, xl, ldx), _pack(np.zeros((M, k)), yl, ldy)
    hy[:] = POISON
    dx, dy = api.DeviceBuffer(hx.nbytes).up(hx), api.DeviceBuffer(hy.nbytes).up(hy)
    try:
        assert api.lib.hipSpMMRowsCSRf32(C.byref(dm.handle), k, dx.ptr, ldx, xl, dy.ptr, ldy, yl) == 0
        out = dy.down(np.float64)
    finally:
        dx.free()
        dy.free()
    assert _padding_poisoned(out, yl, ldy, M, k), "the ld padding of Y is never written"
    return _unpack(out, yl, ldy, M, k)


@pytest.mark.parametrize("k", [1, 3, 16, 17])
@pytest.mark.parametrize("name", ["three-rows-4100", "random-300", "short-1300", "boundary"])
def test_spmm_f32_columns_are_the_f32_spmv(api, oracle, name, k):
    M, N, IRP, JA, AS, x = vr.case(name)
    rng = np.random.default_rng(4200 + k)
    X = np.stack([x] + [x[rng.permutation(N)] for _ in range(k - 1)], axis=1)
    h = Handle(api, (M, N, IRP, JA, AS), "adopted-8" if k == 3 else "uploaded")
    try:
        h.dm.values_f32()
        cols = [_run(api, "hipSpMVRowsCSRf32", h.dm, X[:, c].copy(), M) for c in range(k)]
        vr.same(cols[0], oracle.csr_serial(IRP, JA, vr.round32(AS), x), name)
        for xl, yl in ((ROW, ROW), (COL, COL), (ROW, COL)):
            ldx, ldy = (k if xl == ROW else N) + 3, (k if yl == ROW else M) + 5        # leading dimensions larger than needed
            Y = _spmm32(api, h.dm, X, M, xl, yl, ldx, ldy)
            for c in range(k):
                vr.same(Y[:, c], cols[c], f"{name}, k = {k}, layouts {xl}{yl}, column {c}")
        if k == 1:                                                       # one plain vector: the SpMV kernel itself
            vr.same(_spmm32(api, h.dm, X, M, COL, COL, N, M)[:, 0], cols[0], f"{name}: unit strides")
    finally:
        h.free()


# ------------------------------------------------------------------------------------------------- following the values
def _calls(api, fn):
    before = api.alloc_stats().calls
    fn()
    return api.alloc_stats().calls - before


def test_the_form_follows_update_values_in_place(api, oracle):
    M, N, IRP, JA, AS, x = vr.case("random-300")
    new = si.order_values(np.random.default_rng(4210), JA.size)
    h, plain = Handle(api, (M, N, IRP, JA, AS)), Handle(api, (M, N, IRP, JA, AS))
    try:
        h.dm.values_f32()
        stats = api.alloc_stats()
        # the update allocates what it allocates without the form (the unit detection's word): the array stays where it is
        assert _calls(api, lambda: h.dm.update_values(new)) == _calls(api, lambda: plain.dm.update_values(new))
        after = api.alloc_stats()
        assert (after.live, after.liveBytes) == (stats.live, stats.liveBytes)
        info = h.dm.values_f32_info()
        assert (info.built, info.refreshes) == (1, 1) and (info.inexact, info.overflowed, info.flushed, info.firstOverflow) == vr.counts(new)
        vr.same(_run(api, "hipSpMVRowsCSRf32", h.dm, x, M), oracle.csr_serial(IRP, JA, vr.round32(new), x), "after update_values")
        vr.same(_run(api, "hipSpMVRowsCSR", h.dm, x, M), oracle.csr_serial(IRP, JA, new, x), "the f64 product after update_values")
        # an adopted array rewritten on the device
        ad = Handle(api, (M, N, IRP, JA, AS), "adopted-8")
        try:
            ad.dm.values_f32()
            ad.bufs[2].up(new)
            ad.dm.values_changed()
            vr.same(_run(api, "hipSpMVRowsCSRf32", ad.dm, x, M), oracle.csr_serial(IRP, JA, vr.round32(new), x), "after values_changed")
        finally:
            ad.free()
    finally:
        h.free()
        plain.free()


def test_unit_transitions_make_and_free_the_array(api, oracle):
    M, N, IRP, JA, AS, x = vr.case("random-300")
    ones = np.full(JA.size, 0.1)
    h = Handle(api, (M, N, IRP, JA, ones))
    try:
        h.dm.values_f32()
        live = api.alloc_stats()
        h.dm.update_values(AS)                                           # unit -> non-unit: the array is made
        info = h.dm.values_f32_info()
        assert (info.built, info.unit, info.refreshes) == (1, 0, 1) and info.bytes == (JA.size * 4 + 15) // 16 * 16 + 32
        assert api.alloc_stats().live == live.live + 1 and api.alloc_stats().liveBytes == live.liveBytes + info.bytes
        vr.same(_run(api, "hipSpMVRowsCSRf32", h.dm, x, M), oracle.csr_serial(IRP, JA, vr.round32(AS), x), "unit -> non-unit")
        h.dm.update_values(ones)                                         # and back: it is freed
        info = h.dm.values_f32_info()
        assert (info.built, info.unit, info.bytes, info.refreshes) == (1, 1, 0, 2)
        assert (api.alloc_stats().live, api.alloc_stats().liveBytes) == (live.live, live.liveBytes)
        vr.same(_run(api, "hipSpMVRowsCSRf32", h.dm, x, M), oracle.csr_serial(IRP, JA, vr.round32(ones), x), "non-unit -> unit")
    finally:
        h.free()


def _square(seed):
    """a 300-row matrix with sorted distinct columns and a dominant diagonal (ILU(0) takes it)"""
    from test_fsai_abi import random_spd
    return random_spd(np.random.default_rng(seed), 300, 4)


def _host(api, dm):
    h = dm.handle
    M, NZ = int(h.M), int(h.NZ)

    def down(ptr, n, dtype):
        out = np.empty(n, dtype=dtype)
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
        return out
    return M, int(h.N), down(h.IRP, M + 1, np.uint32).astype(np.uint64), down(h.JA, NZ, np.uint32).astype(np.uint64), down(h.AS, NZ, np.float64)


def test_the_form_follows_the_refresh_of_a_transpose_and_a_product(api, oracle):
    A = _square(4220)
    M, _, IRP, JA, AS = A
    new = _square(4220)[4] * (1.0 + 0.25 * np.random.default_rng(4221).random(JA.size))
    x = si.order_values(np.random.default_rng(4222), M)
    da = api.spMatCpyCSR(api.HostCSR(*A))
    t, p = da.transpose(), da.multiply(da)
    try:
        t.values_f32()
        p.values_f32()
        da.update_values(new)
        t.refresh_from(da)
        p.multiply_refresh(da, da)
        for what, d in (("the transpose", t), ("the product", p)):
            Mh, Nh, I, J, V = _host(api, d)                              # the refreshed doubles, checked elsewhere; here: their roundings
            assert d.values_f32_info().refreshes == 1
            vr.same(_run(api, "hipSpMVRowsCSRf32", d, x, Mh), oracle.csr_serial(I, J, vr.round32(V), x), what)
    finally:
        for m in (p, t, da):
            m.free()


def test_the_form_follows_an_ilu0_factorisation(api, oracle):
    A = _square(4230)
    M, _, IRP, JA, AS = A
    x = si.order_values(np.random.default_rng(4231), M)
    da = api.spMatCpyCSR(api.HostCSR(*A))
    try:
        da.values_f32()
        da.ilu0()
        LU = _host(api, da)[4]
        assert not np.array_equal(LU, AS), "the handle holds the factors now"
        assert da.values_f32_info().refreshes == 1
        vr.same(_run(api, "hipSpMVRowsCSRf32", da, x, M), oracle.csr_serial(IRP, JA, vr.round32(LU), x), "the L\\U handle's f32 product")
    finally:
        da.free()
