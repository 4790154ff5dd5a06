"""What the single-precision value storage refuses, and what a refused device allocation leaves: a
launcher before the form is built, handles that have no such form, and every allocation of spmvHipValuesF32, of an update that
crosses unit -> non-unit and of spmvHipFsaiSetStorage refused in turn -- the f64 handle goes on answering, no partly built
form stays, and the allocation ledger balances."""
import ctypes as C

import numpy as np
import pytest

import fsai_ref as fr
import serial_order_inputs as si
import values_f32_ref as vr
from bits import assert_same_bits
from test_fsai_abi import random_spd
from test_gpu_values_f32 import Handle, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.alloc_refuse(-1)
    a.spmvHipFinalize()


def _ledger(api):
    st = api.alloc_stats()
    return st.live, st.liveBytes, st.badFrees


def test_a_launcher_before_the_form_is_built_is_refused(api, capfd):
    M, N, IRP, JA, AS, x = vr.case("random-300")
    h = Handle(api, (M, N, IRP, JA, AS))
    dx, dy = api.DeviceVector(N).up(x), api.DeviceVector(M)
    H, cfg = C.byref(h.dm.handle), api.CONFIG()
    calls = {
        "hipSpMVRowsCSRf32": lambda: api.lib.hipSpMVRowsCSRf32(H, dx.ptr, cfg, dy.ptr),
        "hipSpMVWarpPerRowCSRf32": lambda: api.lib.hipSpMVWarpPerRowCSRf32(H, dx.ptr, cfg, dy.ptr),
        "spmvHipEnqueueRowsF32": lambda: api.lib.spmvHipEnqueueRowsF32(H, dx.ptr, dy.ptr, None),
        "hipSpMMRowsCSRf32": lambda: api.lib.hipSpMMRowsCSRf32(H, 1, dx.ptr, N, 1, dy.ptr, M, 1),
    }
    try:
        before = _ledger(api)
        for name, call in calls.items():
            dy.poison()
            capfd.readouterr()
            assert call() != 0, name
            err = capfd.readouterr().err
            assert name in err and "spmvHipValuesF32" in err, err
            assert np.isnan(dy.down()).all(), f"{name}: y is untouched"
        assert _ledger(api) == before, "a launcher never allocates"
        with pytest.raises(api.SpmvHipError):
            h.dm.matmul(np.ones((N, 2)), values="f32")
        with pytest.raises(api.SpmvHipError):
            h.dm.matmul(np.ones((N, 2)), values="f16")
        # built, released: refused again
        h.dm.values_f32()
        assert calls["hipSpMVRowsCSRf32"]() == 0
        h.dm.values_f32(False)
        assert calls["hipSpMVRowsCSRf32"]() != 0
    finally:
        dx.free()
        dy.free()
        h.free()


def test_handles_without_such_a_form_are_refused(api, capfd):
    A = random_spd(np.random.default_rng(4400), 300, 4)
    host = api.HostCSR(*A)
    da = api.spMatCpyCSR(host)
    ell = api.spMatCpyELL(host.to_ell())
    amg = da.amg()
    info = api.spmvF32Info()
    try:
        for what, handle, text in (("an ELL handle", ell.handle, "ELL"), ("a hierarchy", amg.handle, "hierarchy")):
            for fn, arg in ((api.lib.spmvHipValuesF32, 1), (api.lib.spmvHipValuesF32Info, C.byref(info))):
                capfd.readouterr()
                assert fn(C.byref(handle), arg) != 0, what
                assert text in capfd.readouterr().err, what
        capfd.readouterr()
        assert api.lib.spmvHipValuesF32(None, 1) != 0 and api.lib.spmvHipValuesF32Info(None, C.byref(info)) != 0
        assert "NULL" in capfd.readouterr().err
        assert api.lib.spmvHipValuesF32Info(C.byref(da.handle), None) != 0
        freed = api.spMatCpyCSR(host)
        freed.values_f32()
        freed.free()                                                     # frees the form with the handle ...
        capfd.readouterr()
        assert api.lib.spmvHipValuesF32(C.byref(freed.handle), 1) != 0   # ... and the zeroed handle is no device handle
        assert "not a device handle" in capfd.readouterr().err
        # a factor: a storage that is neither constant, and a handle that is no factor
        g = da.fsai()
        try:
            capfd.readouterr()
            assert api.lib.spmvHipFsaiSetStorage(C.byref(g.handle), 2) != 0 and g.storage == "f64"
            assert "SPMV_STORAGE" in capfd.readouterr().err
            assert api.lib.spmvHipFsaiSetStorage(C.byref(da.handle), 1) != 0
            assert "spmvHipFsaiSetup" in capfd.readouterr().err
            with pytest.raises(api.SpmvHipError):
                g.set_storage("f16")
        finally:
            g.free()
    finally:
        amg.free()
        ell.free()
        da.free()


def _refuse_in_turn(api, call, after_failure, limit=8):
    """the call with its n-th allocation refused, n = 0, 1, ... until it succeeds; returns how many refusals it met"""
    for n in range(limit):
        try:
            with api.alloc_refused(n):
                call()
        except api.SpmvHipError:
            after_failure(n)
            continue
        return n
    raise AssertionError("the call never succeeded")


def test_the_allocation_of_the_build_refused(api, oracle):
    M, N, IRP, JA, AS, x = vr.case("random-300")
    h = Handle(api, (M, N, IRP, JA, AS))
    try:
        y64 = _run(api, "hipSpMVRowsCSR", h.dm, x, M)
        base = _ledger(api)

        def after(n):
            assert h.dm.values_f32_info().built == 0 and _ledger(api) == base
            assert_same_bits(_run(api, "hipSpMVRowsCSR", h.dm, x, M), y64, "the f64 product after the refusal")
        assert _refuse_in_turn(api, h.dm.values_f32, after) == 1, "one allocation"
        vr.same(_run(api, "hipSpMVRowsCSRf32", h.dm, x, M), oracle.csr_serial(IRP, JA, vr.round32(AS), x), "built after the refusals")
    finally:
        h.free()


def test_the_allocations_of_a_unit_to_non_unit_update_refused(api, oracle):
    M, N, IRP, JA, AS, x = vr.case("random-300")
    ones = np.full(JA.size, 0.1)
    want64 = oracle.csr_serial(IRP, JA, AS, x)
    h = Handle(api, (M, N, IRP, JA, ones))
    try:
        h.dm.values_f32()
        base = _ledger(api)                                              # a unit handle: the form holds no array

        def after(n):
            # the new doubles are in place (the copy comes first) and the handle answers with them; the form is gone, whole
            assert h.dm.values_f32_info().built == 0 and _ledger(api) == base
            assert_same_bits(_run(api, "hipSpMVRowsCSR", h.dm, x, M), want64, f"the f64 product after refusal {n}")
            h.dm.update_values(ones)
            h.dm.values_f32()
            assert _ledger(api) == base
        met = _refuse_in_turn(api, lambda: h.dm.update_values(AS), after)
        assert met == 2, "the unit detection's word and the form's array"
        info = h.dm.values_f32_info()
        assert (info.built, info.unit) == (1, 0)
        vr.same(_run(api, "hipSpMVRowsCSRf32", h.dm, x, M), oracle.csr_serial(IRP, JA, vr.round32(AS), x), "after the update that went through")
    finally:
        h.free()


def test_the_allocations_of_the_factor_storage_refused(api):
    A = random_spd(np.random.default_rng(3803), 300, 4)
    G = fr.fsai_vec(A)[0]
    b = si.order_values(np.random.default_rng(4410), A[0])
    da = api.spMatCpyCSR(api.HostCSR(*A))
    g = da.fsai()
    try:
        want = fr.Applied(G)(b)
        assert_same_bits(g.apply(b), want, "the f64 apply")
        base = _ledger(api)

        def after(n):
            assert g.storage == "f64" and g.values_f32_info().built == 0 and _ledger(api) == base
            assert_same_bits(g.apply(b), want, f"the f64 apply after refusal {n}")
        assert _refuse_in_turn(api, lambda: g.set_storage("f32"), after) == 2, "the form of G and the form of G^T"
        assert g.storage == "f32"
        assert_same_bits(g.apply(b), fr.Applied(vr.rounded(G))(b), "F32 after the refusals")
    finally:
        g.free()
        da.free()


# ------------------------------------------------------------------------------------------------------- the hierarchy
def test_gauss_seidel_and_single_precision_refuse_each_other(api, capfd):
    da = api.spMatCpyCSR(api.HostCSR(*vr.amg_matrix()))
    h = da.amg(coarseRows=8)
    r = si.order_values(np.random.default_rng(4420), int(da.handle.M), 1)
    try:
        h.set_gauss_seidel()
        z = h.apply(r)
        base = _ledger(api)
        capfd.readouterr()
        with pytest.raises(api.SpmvHipError):
            h.set_storage("f32")
        assert "Gauss-Seidel" in capfd.readouterr().err
        assert h.storage_info()["storage"] == "f64" and da.values_f32_info().built == 0 and _ledger(api) == base
        assert_same_bits(h.apply(r), z, "the Gauss-Seidel cycle after the refusal")
        h.set_smoother("jacobi")
        h.set_storage("f32")
        z32 = h.apply(r)
        base = _ledger(api)
        capfd.readouterr()
        with pytest.raises(api.SpmvHipError):
            h.set_gauss_seidel()
        assert "spmvHipAmgSetStorage" in capfd.readouterr().err
        assert h.storage_info()["storage"] == "f32" and _ledger(api) == base
        assert_same_bits(h.apply(r), z32, "the F32 cycle after the refusal")
        capfd.readouterr()
        assert api.lib.spmvHipAmgSetStorage(C.byref(h.handle), C.byref(da.handle), 2) != 0
        assert "SPMV_STORAGE" in capfd.readouterr().err
        assert api.lib.spmvHipAmgStorage(C.byref(da.handle), C.byref(api.spmvAmgStorageInfo())) != 0, "a matrix is no hierarchy"
        assert api.lib.spmvHipAmgStorage(C.byref(h.handle), None) != 0
    finally:
        h.free()
        da.free()


@pytest.mark.parametrize("smoothed", [False, True])
def test_the_allocations_of_the_hierarchy_storage_refused(api, smoothed):
    da = api.spMatCpyCSR(api.HostCSR(*vr.amg_matrix()))
    h = da.amg(coarseRows=8, smoothed=smoothed)
    r = si.order_values(np.random.default_rng(4430), int(da.handle.M), 1)
    try:
        z = h.apply(r)
        base = _ledger(api)

        def after(n):
            assert h.storage_info() == {"storage": "f64", "levels": h.info.levels, "f32_bytes": 0}
            assert da.values_f32_info().built == 0 and _ledger(api) == base
            assert_same_bits(h.apply(r), z, f"the f64 cycle after refusal {n}")
        levels = h.info.levels
        met = _refuse_in_turn(api, lambda: h.set_storage("f32"), after, limit=64)
        # one array per matrix with distinct values: A_0 .. A_last, every P_l of a smoothed hierarchy; a plain hierarchy's P_l
        # and R_l are unit handles and get none, a smoothed one's R_l = P_l^T has one
        assert met == levels + (2 * (levels - 1) if smoothed else 0)
        assert h.storage_info()["storage"] == "f32"
    finally:
        h.free()
        da.free()


def test_a_sharded_matrix_is_refused(api, capfd):
    M, N, IRP, JA, AS, x = vr.case("random-300")
    host = api.HostCSR(M, N, IRP, JA, AS)
    shard = C.c_void_p()
    assert api.lib.spmvHipShardCSR(C.byref(host.struct), 1, C.byref(shard)) == 0
    try:
        base = _ledger(api)
        for fn, arg in ((api.lib.spmvHipValuesF32, 1), (api.lib.spmvHipValuesF32Info, C.byref(api.spmvF32Info()))):
            capfd.readouterr()
            assert fn(C.cast(shard, C.POINTER(api.spmat)), arg) != 0
            assert "sharded" in capfd.readouterr().err
        assert _ledger(api) == base
    finally:
        assert api.lib.spmvHipShardFree(shard) == 0
