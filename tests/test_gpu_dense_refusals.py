"""What the six entry points that take dense blocks say when they refuse one: hipSpMMRowsCSR, hipSpTRSMCSR, spmvHipBlockDot,
spmvHipAmgApplyBlock, hipSpCGBlockCSR and hipSpBiCGStabBlockCSR on the 3 x 3 x 3 Laplacian, one call per single fault --
k = 0, an unknown layout in either operand, a leading dimension one below the need in either operand and either layout,
two blocks that share one element -- with the whole line after "libspmvhip: " literally and the output block untouched;
and the one thing that shares memory and is accepted, the triangular solve in place.  (The refusals happen on the host;
the library needs a device to start.)"""
import ctypes as C

import numpy as np
import pytest

from amg_gpu import _up
from spgemm_ref import laplacian7

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF4DEADBEEF0001
ROW, COL = 0, 1
M, K = 27, 3
END = "\33[0m\n"                        # what closes the library's error line


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(scope="module")
def setup(api):
    """the matrix, its hierarchy with a block workspace of K columns, an input field `src` whose two halves are two
    blocks that touch, and an output block `out`, both of sentinels"""
    da = _up(api, laplacian7(3, 3, 3))
    h = da.amg()
    h.set_block_width(K)
    field = np.full(2 * M * K, SENTINEL, dtype=np.uint64)
    src = api.DeviceBuffer(field.nbytes).up(field)
    out = api.DeviceBuffer(field.nbytes // 2).up(field[:M * K])
    yield da, h, src, out
    for item in (src, out, h, da):
        item.free()


def entry_points(api, da, h):
    """name -> (call(k, p, ldp, pl, q, ldq, ql), the names of the two leading dimensions, the overlap line or None)"""
    lib, A, H = api.lib, C.byref(da.handle), C.byref(h.handle)
    opts = api.spmvKrylovOpts(1e-8, 5, None)

    def krylov(fn):
        return lambda k, p, ldp, pl, q, ldq, ql: fn(A, None, k, p, ldp, pl, q, ldq, ql, C.byref(opts), None, None)
    return {
        "hipSpMMRowsCSR": (lambda k, p, ldp, pl, q, ldq, ql: lib.hipSpMMRowsCSR(A, k, p, ldp, pl, q, ldq, ql), ("ldx", "ldy"), "X and Y overlap"),
        "hipSpTRSMCSR": (lambda k, p, ldp, pl, q, ldq, ql: lib.hipSpTRSMCSR(A, 0, 0, k, p, ldp, pl, q, ldq, ql), ("ldb", "ldx"),
                         "dB and dX overlap without being the same block (same pointer, layout and leading dimension)"),
        "spmvHipBlockDot": (lambda k, p, ldp, pl, q, ldq, ql: lib.spmvHipBlockDot(M, k, p, ldp, pl, p + 8 * M * K, ldq, ql, q), ("ldu", "ldv"), None),
        "spmvHipAmgApplyBlock": (lambda k, p, ldp, pl, q, ldq, ql: lib.spmvHipAmgApplyBlock(H, A, k, p, ldp, pl, q, ldq, ql), ("ldr", "ldz"),
                                 "dR and dZ overlap"),
        "hipSpCGBlockCSR": (krylov(lib.hipSpCGBlockCSR), ("ldb", "ldx"), "dB and dX overlap"),
        "hipSpBiCGStabBlockCSR": (krylov(lib.hipSpBiCGStabBlockCSR), ("ldb", "ldx"), "dB and dX overlap"),
    }


NAMES = ("hipSpMMRowsCSR", "hipSpTRSMCSR", "spmvHipBlockDot", "spmvHipAmgApplyBlock", "hipSpCGBlockCSR", "hipSpBiCGStabBlockCSR")


@pytest.mark.parametrize("who", NAMES)
def test_one_fault_one_line(api, setup, capfd, who):
    da, h, src, out = setup
    call, (ld0, ld1), overlap = entry_points(api, da, h)[who]
    p, q = src.ptr.value, out.ptr.value
    good = dict(k=K, p=p, ldp=K, pl=ROW, q=q, ldq=K, ql=ROW)
    faults = [
        (dict(k=0), "k = 0 columns"),
        (dict(pl=2), "unknown layout 2"),
        (dict(ql=-1), "unknown layout -1"),
        (dict(ldp=K - 1), f"leading dimension {ld0} = {K - 1} is below {K}"),
        (dict(ldq=K - 1), f"leading dimension {ld1} = {K - 1} is below {K}"),
        (dict(pl=COL, ldp=M - 1), f"leading dimension {ld0} = {M - 1} is below {M}"),
        (dict(ql=COL, ldq=M - 1), f"leading dimension {ld1} = {M - 1} is below {M}"),
    ]
    if overlap:                                         # the second block begins at the first one's last element, both ways round
        faults += [(dict(q=p + 8 * (M * K - 1)), overlap), (dict(p=p + 8 * (M * K - 1), q=p), overlap)]
    before = (src.down(np.uint64), out.down(np.uint64))
    for change, text in faults:
        capfd.readouterr()
        assert call(**{**good, **change}) != 0, (who, change)
        err = capfd.readouterr().err
        assert err.count("libspmvhip: ") == 1 and err.split("libspmvhip: ", 1)[1] == f"{who}: {text}" + END, (who, change, err)
        assert np.array_equal(src.down(np.uint64), before[0]) and np.array_equal(out.down(np.uint64), before[1]), (who, change)


def test_the_triangular_solve_in_place_is_accepted(api, setup, capfd):
    da, h, src, out = setup
    call = entry_points(api, da, h)["hipSpTRSMCSR"][0]
    rhs = np.arange(1.0, M * K + 1).reshape(M, K)
    buf = api.DeviceBuffer(rhs.nbytes).up(rhs)
    try:
        for layout, ld in ((ROW, K), (COL, M)):
            capfd.readouterr()
            assert call(K, buf.ptr.value, ld, layout, buf.ptr.value, ld, layout) == 0
            assert capfd.readouterr().err == ""
        assert not np.array_equal(buf.down(np.float64), rhs.ravel()), "the solve wrote its block"
    finally:
        buf.free()
