"""B = P A P^T of a device CSR handle (spmvHipCsrPermute, spmvHipPermuteRefresh) and the permutation of a vector
(spmvHipVecPermute): B's arrays equal tests/colour_ref.py's permutation exactly -- the stable order of repeats and the
special values included --, every downstream contract (SpMV, level sets, ILU(0)-PCG, GMRES) holds on B's downloaded arrays
bit for bit, and every refusal leaves its outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as cr
import serial_order_inputs as si
from bits import assert_same_bits
from gmres_ref import gmres_ref
from ilu0_ref import ilu0_levels
from krylov_ref import Csr, cg_ref

pytestmark = pytest.mark.gpu

ROWS = "hipSpMVRowsCSR"
POISON = 0xA5A5A5A5


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


def _arrays(api, dm):
    h = dm.handle
    return (_down(api, h.IRP, h.M + 1, np.uint32), _down(api, h.JA, h.NZ, np.uint32), _down(api, h.AS, h.NZ, np.float64))


def _assert_permuted(api, db, M, IRP, JA, AS, perm, what):
    irp_ref, ja_ref, as_ref, _ = cr.permute_ref(M, IRP, JA, AS, perm)
    h = db.handle
    assert (h.M, h.N, h.NZ) == (M, M, JA.size), what
    irp, ja, a = _arrays(api, db)
    assert np.array_equal(irp, irp_ref), f"{what}: IRP"
    assert np.array_equal(ja, ja_ref), f"{what}: JA"
    assert np.array_equal(a.view(np.uint64), as_ref.view(np.uint64)), f"{what}: AS"
    return irp, ja, a


def _special_values(rng, n):
    """order-sensitive values with NaNs of two payloads, both infinities and both zeros among them"""
    v = si.order_values(rng, n)
    bits = v.view(np.uint64)
    special = np.array([0x7FF8000000000001, 0xFFF800000000BEEF, 0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 0],
                       dtype=np.uint64)
    if n:
        at = rng.choice(n, size=min(n, 24), replace=False)
        bits[at] = special[np.arange(at.size) % special.size]
    return v


def _perms(M, IRP, JA, rng):
    out = {"identity": np.arange(M), "reversal": np.arange(M)[::-1].copy(), "random": rng.permutation(M)}
    for order, seed in cr.CONFIGS:
        out[f"colour{order}:{seed:#x}"] = cr.perm_of(cr.colour_ref(M, IRP, JA, order, seed)[0])
    return out


CASES = cr.small_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_arrays_equal_the_reference(api, name):
    M, IRP, JA = CASES[name]
    rng = np.random.default_rng(2100)
    AS = _special_values(rng, JA.size)
    dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    try:
        for pname, perm in _perms(M, IRP, JA, rng).items():
            db = dm.permute(perm.astype(np.uint32))
            try:
                _assert_permuted(api, db, M, IRP, JA, AS, perm, f"{name} {pname}")
            finally:
                db.free()
    finally:
        dm.free()


def test_device_perm_from_colour_and_spmv(api, oracle):
    """colour on the device, permute with its perm, and multiply: the bits of the oracle on B's arrays, and P (A x) on
    integer-valued inputs (every sum exact, so the order inside a row cannot show)"""
    M, IRP, JA = CASES["unsorted_repeats"]
    rng = np.random.default_rng(2101)
    AS = rng.integers(-8, 9, JA.size).astype(np.float64)
    x = rng.integers(-8, 9, M).astype(np.float64)
    dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    col = dm.colour(order="hash", seed=3)
    db = dm.permute(col)
    try:
        perm = col.perm.down(np.uint32)
        irp, ja, a = _assert_permuted(api, db, M, IRP, JA, AS, perm, "device perm")
        px = api.permute_vector(col, x)
        assert np.array_equal(px, x[perm])
        dx, dy = api.DeviceVector(M).up(px), api.DeviceVector(M)
        dy.poison()
        api.spmv(ROWS, db, dx, dy)
        y = dy.down()
        assert_same_bits(y, oracle.csr_serial(irp, ja, a, px), "oracle on B")
        assert np.array_equal(y, oracle.csr_serial(IRP, JA, AS, x)[perm])
        assert np.array_equal(api.permute_vector(col, y, inverse=True), oracle.csr_serial(IRP, JA, AS, x))
        dx.free()
        dy.free()
    finally:
        col.free()
        db.free()
        dm.free()


@pytest.fixture(scope="module")
def red_black(api):
    """the 12x10x8 Laplacian permuted by its NATURAL colouring twice: B, and M factored in place by ILU(0)"""
    M, IRP, JA, AS = cr.laplacian7(12, 10, 8)
    dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    col = dm.colour()
    B, F = dm.permute(col), dm.permute(col)
    perm = col.perm.down(np.uint32)
    irp, ja, a = _arrays(api, B)
    F.ilu0()
    yield M, B, F, perm, irp, ja, a
    for d in (B, F, dm):
        d.free()
    col.free()


def test_red_black_has_two_levels(api, red_black):
    M, B, F, perm, irp, ja, a = red_black
    for lower in (True, False):
        B.triangular_analyse(lower)
        info = B.triangular_info(lower)
        assert (info.levels, info.launches) == (2, 2), (lower, info.levels, info.launches)
    assert F.ilu0_info().levels == 2 and F.ilu0_info().zeroPivot < 0


def test_pcg_and_gmres_on_the_permuted_pair(api, red_black):
    M, B, F, perm, irp, ja, a = red_black
    fac = ilu0_levels(M, irp, ja, a)
    assert_same_bits(_arrays(api, F)[2], fac, "ILU(0) of B")
    pbuf = api.DeviceBuffer(4 * M).up(perm)
    b = api.permute_vector(pbuf, np.random.default_rng(2102).random(M))
    pbuf.free()
    A = Csr(M, irp, ja, a, fac)
    x, info = B.cg(b, precond=F, tol=1e-8, maxiter=200, history=True)
    xr, st, it, hist, rr = cg_ref(A, b, np.zeros(M), 1e-8, 200)
    assert (info.status, info.iterations) == (st, it) and st == 0
    assert_same_bits(x, xr, "PCG x")
    assert_same_bits(info.history, hist, "PCG history")
    x, info = B.gmres(b, precond=F, tol=1e-8, maxiter=200, restart=10, history=True)
    xr, st, it, hist, rr = gmres_ref(A, b, np.zeros(M), 1e-8, 200, 10)
    assert (info.status, info.iterations) == (st, it) and st == 0
    assert_same_bits(x, xr, "GMRES x")
    assert_same_bits(info.history, hist, "GMRES history")


def test_vector_round_trip_at_odd_offsets(api):
    import torch
    n = 1000
    rng = np.random.default_rng(2103)
    perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
    v_host = _special_values(rng, n)
    nan = float("nan")
    src = torch.full((n + 8,), nan, dtype=torch.float64, device="cuda")
    mid = torch.full((n + 8,), nan, dtype=torch.float64, device="cuda")
    dst = torch.full((n + 8,), nan, dtype=torch.float64, device="cuda")
    src[3:3 + n] = torch.from_numpy(v_host).cuda()
    poison = mid.clone().view(torch.int64)
    api.permute_vector(perm, src[3:3 + n], out=mid[1:1 + n])
    api.permute_vector(perm, mid[1:1 + n], inverse=True, out=dst[5:5 + n])
    torch.cuda.synchronize()
    got_mid, got = mid.cpu().numpy(), dst.cpu().numpy()
    assert np.array_equal(got_mid[1:1 + n].view(np.uint64), v_host[perm.cpu().numpy()].view(np.uint64))
    assert np.array_equal(got[5:5 + n].view(np.uint64), v_host.view(np.uint64))
    p = poison.cpu().numpy()
    assert np.array_equal(got_mid.view(np.int64)[[0] + list(range(n + 1, n + 8))], p[[0] + list(range(n + 1, n + 8))])
    assert np.array_equal(got.view(np.int64)[list(range(5)) + list(range(n + 5, n + 8))], p[list(range(5)) + list(range(n + 5, n + 8))])


def test_refresh_equals_a_fresh_permute(api):
    M, IRP, JA = CASES["unsorted_repeats"]
    rng = np.random.default_rng(2104)
    A0, A1 = si.order_values(rng, JA.size), _special_values(rng, JA.size)
    perm = rng.permutation(M).astype(np.uint32)
    dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, A0))
    other = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, A1))
    db = dm.permute(perm)
    dt = dm.transpose()
    try:
        dm.update_values(A1)
        db.permute_refresh(dm)
        _assert_permuted(api, db, M, IRP, JA, A1, perm, "refreshed")
        fresh = dm.permute(perm)
        assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(_arrays(api, db), _arrays(api, fresh)))
        fresh.free()
        before = _arrays(api, db)[2].copy()
        for dst, src in ((db, other), (dm, dm), (dt, dm)):            # a wrong source; no permutation; a transpose
            assert api.lib.spmvHipPermuteRefresh(C.byref(dst.handle), C.byref(src.handle)) == 1
        assert api.lib.spmvHipTransposeRefresh(C.byref(db.handle), C.byref(dm.handle)) == 1
        assert np.array_equal(_arrays(api, db)[2].view(np.uint64), before.view(np.uint64))
    finally:
        for d in (dt, db, other, dm):
            d.free()


def test_graph_replay_of_vec_permute(api):
    import torch
    n = 4099
    rng = np.random.default_rng(2105)
    perm_host = rng.permutation(n)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        perm = torch.from_numpy(perm_host.astype(np.int32)).cuda()
        v = torch.from_numpy(rng.random(n)).cuda()
        out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        api.lib.spmvHipSetStream(C.c_void_p(stream.cuda_stream))
        api.lib.spmvHipSetSync(0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            assert api.lib.spmvHipVecPermute(n, perm.data_ptr(), v.data_ptr(), out.data_ptr(), 0) == 0
        torch.cuda.synchronize()
        v.copy_(torch.from_numpy(np.arange(n, dtype=np.float64)).cuda())
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), perm_host.astype(np.float64))
    api.lib.spmvHipSetStream(None)
    api.lib.spmvHipSetSync(1)
    del graph


def test_refusals_leave_outputs_untouched(api, capfd):
    M, IRP, JA = CASES["random257"]
    AS = np.ones(JA.size)
    dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    rect = api.spMatCpyCSR(api.HostCSR(3, 4, np.array([0, 1, 2, 3], dtype=np.uint64), np.array([0, 1, 3], dtype=np.uint64), np.ones(3)))
    ell = api.csr_to_ell_device(dm, False)
    good = np.arange(M, dtype=np.uint32)
    too_big, repeated = good.copy(), good.copy()
    too_big[100] = M
    repeated[200] = 7
    bufs = {k: api.DeviceBuffer(4 * M).up(v) for k, v in (("good", good), ("too_big", too_big), ("repeated", repeated))}
    out = api.spmat()
    out.M = 12345
    image = C.string_at(C.addressof(out), C.sizeof(out))
    empty = api.spmat()
    try:
        for handle, perm in ((dm.handle, bufs["too_big"].ptr), (dm.handle, bufs["repeated"].ptr), (dm.handle, None),
                             (rect.handle, bufs["good"].ptr), (ell.handle, bufs["good"].ptr), (empty, bufs["good"].ptr)):
            assert api.lib.spmvHipCsrPermute(C.byref(handle), perm, C.byref(out)) == 1
            assert C.string_at(C.addressof(out), C.sizeof(out)) == image
        assert api.lib.spmvHipCsrPermute(None, bufs["good"].ptr, C.byref(out)) == 1
        assert api.lib.spmvHipCsrPermute(C.byref(dm.handle), bufs["good"].ptr, None) == 1
        before = C.string_at(C.addressof(dm.handle), C.sizeof(dm.handle))
        assert api.lib.spmvHipCsrPermute(C.byref(dm.handle), bufs["good"].ptr, C.byref(dm.handle)) == 1
        assert C.string_at(C.addressof(dm.handle), C.sizeof(dm.handle)) == before
        err = capfd.readouterr().err
        assert "a value >= M" in err and "a repeated value" in err
        # the vector permutation: NULLs and dIn == dOut
        dv = api.DeviceVector(M).up(np.arange(M, dtype=np.float64))
        for args in ((None, dv.ptr, dv.ptr), (bufs["good"].ptr, None, dv.ptr), (bufs["good"].ptr, dv.ptr, None),
                     (bufs["good"].ptr, dv.ptr, dv.ptr)):
            assert api.lib.spmvHipVecPermute(M, *args, 0) == 1
        assert np.array_equal(dv.down(), np.arange(M, dtype=np.float64))
        dv.free()
        # the source is untouched by all of it
        db = dm.permute(bufs["good"])
        _assert_permuted(api, db, M, IRP, JA, AS, good, "identity after the refusals")
        db.free()
    finally:
        for b in bufs.values():
            b.free()
        for d in (ell, rect, dm):
            d.free()


def test_device_memory_comes_back(api):
    import torch
    M, IRP, JA, AS = cr.laplacian7(64, 64, 16)
    free = []
    for _ in range(8):
        dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
        col = dm.colour(order="hash", want_colours=True)
        db = dm.permute(col)
        dm.update_values(AS * 2)
        db.permute_refresh(dm)
        dm.free()                                        # the source first: B keeps no pointer to it
        db.free()
        col.free()
        api.spmvHipFinalize()
        api.spmvHipInit(0)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert min(free[2:]) >= free[1] - (8 << 20) and free[-1] >= free[1] - (8 << 20), free
