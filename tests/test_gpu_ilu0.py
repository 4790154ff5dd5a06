"""ILU(0) on the device (hipSpILU0CSR, spmvHipIlu0Info; DeviceMatrix.ilu0): every case compares AS after the factorisation
with the test side's serial loop (tests/ilu0_ref.py) in all bits -- finite values by bits, infinities by sign, NaN as NaN.
The inputs are order-sensitive (tests/test_ilu0_abi.py shows that on the host)."""
import ctypes as C

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits
from conftest import tight_error
from ilu0_ref import check_pattern, ilu0_levels, ilu0_loop
from test_gpu_trsv import Source, same
from test_ilu0_abi import chain, random_ilu, stencil
from test_trsv_abi import laplacian7
from trsv_ref import trsv_levels

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
    api.lib.spmvHipSetUnitValues(1)
    api.lib.spmvHipSetSync(1)
    api.lib.spmvHipSetVariant(b"hipSpILU0CSR", 16)
    api.lib.spmvHipSetVariant(b"hipSpTRSVCSR", 256)


def _down_as(dm):
    """the handle's AS as it is on the device"""
    from spmv_openmp_cuda_amd import api
    out = np.empty(int(dm.handle.NZ), np.float64)
    if out.size:
        assert api.lib.spmvHipVecDown(out.ctypes.data_as(C.c_void_p), C.cast(dm.handle.AS, C.c_void_p), out.size) == 0
    return out


def factor(api, src, M, IRP, JA, AS, what, ref=None):
    info = src.dm.ilu0()
    got = _down_as(src.dm)
    if ref is None:
        ref = ilu0_loop(M, IRP, JA, AS) if JA.size < 20_000 else ilu0_levels(M, IRP, JA, AS)
    same(got, ref, what)
    return info, ref


def _spmv(api, name, dm, x):
    M = int(dm.handle.M)
    dx, dy = api.DeviceVector(x.size).up(x), api.DeviceVector(M)
    try:
        dy.poison()
        api.spmv(name, dm, dx, dy)
        return dy.down()
    finally:
        dx.free()
        dy.free()


# ------------------------------------------------------------------------------------------------- 1. matrices
def test_small_hand_made(api):
    cases = [
        (1, [0, 1], [0], [2.5]),
        (2, [0, 2, 4], [0, 1, 0, 1], [4.0, 1.0, 3.0, 5.0]),
        (3, [0, 2, 5, 7], [0, 2, 0, 1, 2, 1, 2], [2.0, -1.0, 0.5, 3.0, 0.25, -2.0, 7.0]),
        (4, [0, 1, 3, 6, 10], [0, 0, 1, 0, 1, 2, 0, 1, 2, 3], [3.0, 0.1, 2.0, 0.7, 0.3, 5.0, 1 / 3, 0.2, 0.9, 4.0]),
    ]
    for M, IRP, JA, AS in cases:
        IRP, JA, AS = np.array(IRP, np.uint64), np.array(JA, np.uint64), np.array(AS)
        src = Source(api, M, M, IRP, JA, AS)
        try:
            info, _ = factor(api, src, M, IRP, JA, AS, f"hand-made {M}")
            assert info.zeroPivot == -1 and info.firstBadRow == -1 and info.factorisations == 1
        finally:
            src.free()


@pytest.mark.parametrize("adopt", [0, 4, 8])
@pytest.mark.parametrize("M,per_row,seed", [(700, 6, 1), (3000, 12, 2)])
def test_random_sorted(api, adopt, M, per_row, seed):
    rng = np.random.default_rng(1800 + seed + adopt)
    IRP, JA, AS = random_ilu(rng, M, per_row, e=4)
    src = Source(api, M, M, IRP, JA, AS, adopt)
    try:
        info, ref = factor(api, src, M, IRP, JA, AS, f"random, adopt {adopt}")
        assert info.levels == src.dm.triangular_info(True).levels > 1
        if adopt:                                            # the caller's dAS is the factored array
            same(src.bufs[2].down(np.float64), ref, "adopted dAS")
    finally:
        src.free()


@pytest.mark.parametrize("width", [8, 16, 64])
def test_laplacian_64_cubed_wide_levels(api, width):
    rng = np.random.default_rng(1810)
    n = 64
    IRP, JA, AS = stencil(rng, n, n, n)
    M = n ** 3
    api.set_variant("hipSpILU0CSR", width)
    src = Source(api, M, M, IRP, JA, AS)
    try:
        info, _ = factor(api, src, M, IRP, JA, AS, f"laplacian 64^3, width {width}")
        assert info.levels == 3 * n - 2 and info.longRows == 0
    finally:
        src.free()


def test_chain_thin_runs(api):
    rng = np.random.default_rng(1811)
    M = 5000
    IRP, JA, AS = chain(rng, M)
    src = Source(api, M, M, IRP, JA, AS, 8)
    try:
        info, _ = factor(api, src, M, IRP, JA, AS, "chain")
        tri = src.dm.triangular_info(True)
        assert info.levels == M and tri.fusedLevels == M and info.launches == tri.launches + 1
    finally:
        src.free()


def long_rows(rng):
    """a banded matrix with a row of 100 lower entries (more than 64), rows of 300 and 900 lower entries and one of 300
    upper entries (more than the 256 entries a wavefront stages in LDS; the last in a run of thin levels), and the
    transposed entries of each, so that the updates reach them"""
    M = 1200
    rows, cols = [np.arange(M)], [np.arange(M)]
    for i in range(1, M):
        for j in (i - 1, i - 2):
            if j >= 0:
                rows.append([i, j])
                cols.append([j, i])
    for i, lo in ((500, 100), (800, 300), (1100, 900)):
        c = np.arange(i - lo, i)
        rows.append(np.full(c.size, i))
        cols.append(c)
        rows.append(c)                                       # and the transposed entries: fill the updates reach
        cols.append(np.full(c.size, i))
    c = np.arange(51, 351)
    rows += [np.full(c.size, 50), c]
    cols += [c, np.full(c.size, 50)]
    rows, cols = np.concatenate([np.ravel(r) for r in rows]), np.concatenate([np.ravel(c) for c in cols])
    key = np.unique(rows * M + cols)
    rows, cols = key // M, key % M
    vals = np.where(rows == cols, 40.0 + rng.random(rows.size), si.order_values(rng, rows.size, 2) / 30)
    return M, si.assemble(M, rows, cols, vals)


@pytest.mark.parametrize("width", [8, 64])
@pytest.mark.parametrize("adopt", [0, 8])
def test_long_rows(api, width, adopt):
    rng = np.random.default_rng(1812)
    M, (IRP, JA, AS) = long_rows(rng)
    assert np.diff(IRP.astype(np.int64)).max() > 900
    api.set_variant("hipSpILU0CSR", width)
    src = Source(api, M, M, IRP, JA, AS, adopt)
    try:
        info, _ = factor(api, src, M, IRP, JA, AS, f"long rows, width {width}")
        assert info.longRows >= 3
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 2. the handle after
def test_pattern_handle_stops_being_unit(api, oracle):
    nx, ny, nz = 20, 16, 12
    IRP, JA, _ = laplacian7(nx, ny, nz)
    M = nx * ny * nz
    AS = np.ones(JA.size)
    src = Source(api, M, M, IRP, JA, AS)
    v = C.c_double()
    try:
        assert api.lib.spmvHipUnitValue(C.byref(src.dm.handle), C.byref(v)) == 1
        x = si.order_values(np.random.default_rng(1820), M)
        _spmv(api, "hipSpMVRowsCSR", src.dm, x)                  # the serial-order selection measured on the unit matrix
        _, ref = factor(api, src, M, IRP, JA, AS, "pattern")
        assert api.lib.spmvHipUnitValue(C.byref(src.dm.handle), C.byref(v)) == 0
        assert src.dm.update_info().unitBefore == 1 and src.dm.update_info().unitAfter == 0
        assert_same_bits(_spmv(api, "hipSpMVRowsCSR", src.dm, x), oracle.csr_serial(IRP, JA, ref, x))
    finally:
        src.free()


def test_formats_built_before_factoring(api, oracle):
    rng = np.random.default_rng(1821)
    n = 40
    IRP, JA, AS = stencil(rng, 2 * n, n, n)
    M = 2 * n ** 3
    assert JA.size >= 1 << 18
    src = Source(api, M, M, IRP, JA, AS)
    x = si.order_values(rng, M)
    try:
        for det in (False, True):
            api.build_tiles(src.dm, deterministic=det)
            api.build_stripes(src.dm, deterministic=det)
        for name in ("hipSpMVRowsCSR", "hipSpMVWarpPerRowCSR"):
            _spmv(api, name, src.dm, x)
        _, ref = factor(api, src, M, IRP, JA, AS, "formats built")
        y_ref = oracle.csr_serial(IRP, JA, ref, x)
        assert_same_bits(_spmv(api, "hipSpMVRowsCSR", src.dm, x), y_ref)
        assert tight_error(IRP, JA, ref, x, y_ref, _spmv(api, "hipSpMVWarpPerRowCSR", src.dm, x)) <= 1e-13
        for name in ("hipSpMVTilesCSR", "hipSpMVStripesCSR", "hipSpMVRowsSELL"):
            assert tight_error(IRP, JA, ref, x, y_ref, _spmv(api, name, src.dm, x)) <= 1e-13, name
    finally:
        src.free()


def test_zero_pivot(api):
    rng = np.random.default_rng(1830)
    M = 1500
    IRP, JA, AS = random_ilu(rng, M, 8)
    dpos, _, _ = check_pattern(M, IRP, JA)
    AS = AS.copy()
    AS[dpos[[40, 700]]] = [0.0, -0.0]
    src = Source(api, M, M, IRP, JA, AS)
    try:
        info, ref = factor(api, src, M, IRP, JA, AS, "zero pivot")
        assert not np.isfinite(ref).all()
        zero = np.flatnonzero(ref[dpos] == 0.0)
        assert info.zeroPivot == zero[0] <= 40
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_leave_as_untouched(api, capfd):
    from spmv_openmp_cuda_amd import api as a
    lib = a.lib
    P = C.byref

    def refused(dm, msg, bad_row=None):
        before = _down_as(dm) if dm is not None else None
        assert lib.hipSpILU0CSR(P(dm.handle) if dm is not None else None) != 0
        err = capfd.readouterr().err
        assert msg in err, err
        if dm is not None:
            assert_same_bits(_down_as(dm), before, msg)
            if bad_row is not None:
                assert dm.ilu0_info().firstBadRow == bad_row

    refused(None, "not a device handle")
    rng = np.random.default_rng(1840)
    M = 300
    IRP, JA, AS = random_ilu(rng, M, 6)
    rows = si.row_of_entry(IRP).astype(np.int64)
    starts = IRP[:-1].astype(np.int64)
    lens = np.diff(IRP.astype(np.int64))
    cases = []
    r = int(np.flatnonzero(lens >= 3)[5])                   # unsorted row r
    ja = JA.copy()
    ja[starts[r]], ja[starts[r] + 1] = ja[starts[r] + 1], ja[starts[r]]
    cases.append((ja, "not strictly ascending", r))
    r2 = int(np.flatnonzero(lens >= 3)[9])                  # a repeated column in row r2: its first column twice
    ja = JA.copy()
    ja[starts[r2] + 1] = ja[starts[r2]]
    cases.append((ja, "not strictly ascending", r2))
    for ja, msg, row in cases:
        src = Source(api, M, M, IRP, ja, AS)
        try:
            refused(src.dm, msg, row)
            refused(src.dm, msg, row)                        # the cached answer
        finally:
            src.free()
    # a missing diagonal (row 7) and a doubled one (row 11, sorted: the diagonal repeated is also a repeated column)
    keep = ~((rows == 7) & (JA.astype(np.int64) == 7))
    I2, J2, A2 = si.assemble(M, rows[keep], JA[keep].astype(np.int64), AS[keep])
    src = Source(api, M, M, I2, J2, A2)
    try:
        refused(src.dm, "row 7 does not hold exactly one stored diagonal", 7)
    finally:
        src.free()
    # not square, ELL
    rect = a.spMatCpyCSR(a.HostCSR(M, M + 1, IRP, JA, AS))
    try:
        refused(rect, "not square")
    finally:
        rect.free()
    host = Source(api, M, M, IRP, JA, AS)
    ells = [a.spMatCpyELL(a.HostCSR(M, M, IRP, JA, AS).to_ell()), a.csr_to_ell_device(host.dm, False)]
    try:
        for ell in ells:
            assert lib.hipSpILU0CSR(P(ell.handle)) != 0
            assert "ELL" in capfd.readouterr().err
        assert_same_bits(_down_as(host.dm), AS, "the source of the device ELL")
    finally:
        for ell in ells:
            ell.free()
        host.free()
    gone = Source(api, M, M, IRP, JA, AS)
    h = gone.dm.handle
    gone.free()
    assert lib.hipSpILU0CSR(P(h)) != 0
    assert "not a device handle" in capfd.readouterr().err
    # and a good matrix still factors after all that
    src = Source(api, M, M, IRP, JA, AS)
    try:
        factor(api, src, M, IRP, JA, AS, "after the refusals")
    finally:
        src.free()


# ------------------------------------------------------------------------------------------------- 4. reuse and solves
def test_schedule_reuse_and_refactorisation(api):
    rng = np.random.default_rng(1850)
    nx, ny, nz = 30, 20, 10
    IRP, JA, A = stencil(rng, nx, ny, nz)
    M = nx * ny * nz
    _, _, B = stencil(rng, nx, ny, nz)
    src = Source(api, M, M, IRP, JA, A)
    try:
        src.dm.triangular_analyse(True)
        factor(api, src, M, IRP, JA, A, "first")
        src.dm.update_values(B)
        info, ref_b = factor(api, src, M, IRP, JA, B, "second")
        assert src.dm.triangular_info(True).analyses == 1 and info.factorisations == 2
        fresh = Source(api, M, M, IRP, JA, B)
        try:
            fresh.dm.ilu0()
            assert_same_bits(_down_as(src.dm), _down_as(fresh.dm), "refactorised vs fresh")
        finally:
            fresh.free()
    finally:
        src.free()


def test_factor_then_solve(api):
    rng = np.random.default_rng(1860)
    nx, ny, nz = 24, 20, 16
    IRP, JA, AS = stencil(rng, nx, ny, nz)
    M = nx * ny * nz
    src = Source(api, M, M, IRP, JA, AS)
    try:
        _, F = factor(api, src, M, IRP, JA, AS, "factors")
        b = si.order_values(rng, M)
        y = src.dm.solve_triangular(b, lower=True, unit_diagonal=True)
        same(y, trsv_levels(M, IRP, JA, F, b, True, True), "L y = b")
        x = src.dm.solve_triangular(y, lower=False)
        same(x, trsv_levels(M, IRP, JA, F, y, False, False), "U x = y")
    finally:
        src.free()


def test_pcg_converges_faster(api):
    """preconditioned CG on a Laplacian with torch vector ops: ILU(0) by the two solves on a second handle"""
    torch = pytest.importorskip("torch")
    n = 32
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    dx, dy = api.DeviceVector(M), api.DeviceVector(M)
    try:
        P.ilu0()
        b = torch.from_numpy(np.random.default_rng(1870).random(M)).cuda()

        def matvec(v):
            dx.up(v.cpu().numpy())
            api.spmv("hipSpMVRowsCSR", A, dx, dy)
            return torch.from_numpy(dy.down()).cuda()

        def cg(precond):
            x = torch.zeros_like(b)
            r = b.clone()
            z = precond(r)
            p = z.clone()
            rz = torch.dot(r, z)
            bn = torch.linalg.norm(b)
            for it in range(1, 500):
                q = matvec(p)
                alpha = rz / torch.dot(p, q)
                x += alpha * p
                r -= alpha * q
                if torch.linalg.norm(r) / bn < 1e-8:
                    return it, x
                z = precond(r)
                rz, rz_old = torch.dot(r, z), rz
                p = z + (rz / rz_old) * p
            return 500, x

        def ilu(r):
            return P.solve_triangular(P.solve_triangular(r, lower=True, unit_diagonal=True), lower=False)

        it_plain, _ = cg(lambda r: r.clone())
        it_ilu, x = cg(ilu)
        res = torch.linalg.norm(b - matvec(x)) / torch.linalg.norm(b)
        assert res < 1e-7 and it_ilu < 500
        assert it_ilu <= 0.75 * it_plain, (it_ilu, it_plain)
    finally:
        dx.free()
        dy.free()
        A.free()
        P.free()


def test_device_memory_comes_back(api):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1880)
    n = 40
    IRP, JA, AS = stencil(rng, n, n, n)
    M = n ** 3
    free = []
    for _ in range(12):
        src = Source(api, M, M, IRP, JA, AS)
        src.dm.ilu0()
        src.dm.update_values(AS)
        src.dm.ilu0()
        src.free()
        api.spmvHipFinalize()
        api.spmvHipInit(0)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert np.median(free[2:]) >= free[1] - (8 << 20) and free[-1] >= free[1] - (8 << 20), free
