"""spmvHipBlockDot on the device: dH[c] is, bit for bit, the fixed-order dot of column c (krylov_ref.dot_ref) and what
spmvHipDot gives on a contiguous copy of that column -- whatever k, the layouts, the leading dimensions and the alignment
are.  The columns are distinct order-sensitive vectors (serial_order_inputs.order_values), so a swapped or shared column
shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits
from block_krylov_ref import block_dot_ref
from test_gpu_trsm import SENTINEL, Block, layouts_of

pytestmark = pytest.mark.gpu

KB = 4096
SMALL_N = (0, 1, 2, 511, 512, 513, KB - 1, KB, KB + 1, 2 * KB + 3)
BIG_N = 257 * KB + 5                    # more block partials than the second level has lanes
LAYOUTS = ("row", "row+3", "col", "col+5")


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@functools.lru_cache(maxsize=None)
def inputs(n, k):
    """U, V (n, k) and the reference of every column, computed once"""
    rng = np.random.default_rng(2800 + n % 997 + k)
    U = np.stack([si.order_values(rng, n, 8) for _ in range(k)], axis=1) if n else np.zeros((0, k))
    V = np.stack([si.order_values(rng, n, 8) for _ in range(k)], axis=1) if n else np.zeros((0, k))
    ref, ref_uu = block_dot_ref(U, V), block_dot_ref(U, U)
    for a in (U, V, ref, ref_uu):
        a.setflags(write=False)
    return U, V, ref, ref_uu


def run(api, torch, U, V, k, out_off=0):
    """the C call on two Blocks (V may be U); returns the k results after checking that nothing else was written"""
    out = torch.from_numpy(np.full(k + 2 + out_off, SENTINEL, dtype=np.uint64).view(np.float64)).cuda()
    rc = api.lib.spmvHipBlockDot(U.M, k, C.c_void_p(U.ptr), U.ld, U.layout, C.c_void_p(V.ptr), V.ld, V.layout,
                                 C.c_void_p(out.data_ptr() + 8 * out_off))
    assert rc == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (np.delete(host, np.arange(out_off, out_off + k)).view(np.uint64) == SENTINEL).all(), "written outside dH"
    return host[out_off:out_off + k]


@pytest.mark.parametrize("n", SMALL_N)
def test_widths_layouts_and_offsets(api, torch, n):
    for k in (1, 2, 3, 16, 17, 33):
        Uh, Vh, ref, ref_uu = inputs(n, k)
        lay = layouts_of(n, k)
        pairs = [(u, v) for u in LAYOUTS for v in LAYOUTS] if k in (3, 16) else [(u, LAYOUTS[(i + k) % 4]) for i, u in enumerate(LAYOUTS)]
        for ul, vl in pairs:
            for off in ((0, 1) if ul == vl else (0,)):                   # views at element offset 1: 8-byte aligned only
                what = f"n {n}, k {k}, U {ul}, V {vl}, offset {off}"
                U = Block(torch, n, k, *lay[ul], off=off, host=Uh)
                V = Block(torch, n, k, *lay[vl], off=off, host=Vh)
                assert_same_bits(run(api, torch, U, V, k, out_off=off), ref, what)
                U.padding_intact(what)
                V.padding_intact(what)
                if ul == vl:
                    assert_same_bits(run(api, torch, U, U, k), ref_uu, what + ", U == V")
    if n == 0:
        assert not np.signbit(inputs(0, 3)[2]).any()                    # k times +0.0


@pytest.mark.parametrize("k", [1, 3])
def test_more_block_partials_than_lanes(api, torch, k):
    Uh, Vh, ref, ref_uu = inputs(BIG_N, k)
    lay = layouts_of(BIG_N, k)
    for ul, vl, off in (("row", "row", 0), ("row+3", "col", 1), ("col+5", "col+5", 1)):
        U = Block(torch, BIG_N, k, *lay[ul], off=off, host=Uh)
        V = Block(torch, BIG_N, k, *lay[vl], off=off, host=Vh)
        assert_same_bits(run(api, torch, U, V, k), ref, f"k {k}, U {ul}, V {vl}, offset {off}")
    assert_same_bits(run(api, torch, U, U, k), ref_uu, "U == V")


@pytest.mark.parametrize("n,k", [(2 * KB + 3, 17), (BIG_N, 3)])
def test_against_the_single_dot_on_the_device(api, torch, n, k):
    Uh, Vh, ref, _ = inputs(n, k)
    lay = layouts_of(n, k)
    U = Block(torch, n, k, *lay["row+3"], off=1, host=Uh)
    V = Block(torch, n, k, *lay["col"], host=Vh)
    got = run(api, torch, U, V, k)
    single = [api.dot(U.view[:, c].contiguous(), V.view[:, c].contiguous()).item() for c in range(k)]
    assert_same_bits(got, np.array(single), "against spmvHipDot")
    assert_same_bits(got, ref, "against dot_ref")


def test_python_layer_and_refusals(api, torch, capfd):
    n, k = 513, 3
    Uh, Vh, ref, ref_uu = inputs(n, k)
    U, V = torch.from_numpy(np.array(Uh)).cuda(), torch.from_numpy(np.array(Vh).T.copy()).cuda().t()
    h = api.block_dot(U, V)                                              # row-major U, column-major V
    assert h.is_cuda and tuple(h.shape) == (k,)
    assert_same_bits(h.cpu().numpy(), ref, "device call")
    assert_same_bits(api.block_dot(U, U).cpu().numpy(), ref_uu, "U == V")
    hn = api.block_dot(np.array(Uh), np.array(Vh))
    assert isinstance(hn, np.ndarray)
    assert_same_bits(hn, ref, "host call")
    with pytest.raises(api.SpmvHipError):
        api.block_dot(U, V[:, :2])
    out = torch.zeros(k, dtype=torch.float64).cuda()
    lib = api.lib
    up, vp, op = C.c_void_p(U.data_ptr()), C.c_void_p(V.data_ptr()), C.c_void_p(out.data_ptr())
    capfd.readouterr()
    for call in (lambda: lib.spmvHipBlockDot(n, k, None, k, 0, vp, n, 1, op), lambda: lib.spmvHipBlockDot(n, k, up, k, 0, None, n, 1, op),
                 lambda: lib.spmvHipBlockDot(n, k, up, k, 0, vp, n, 1, None), lambda: lib.spmvHipBlockDot(n, 0, up, k, 0, vp, n, 1, op),
                 lambda: lib.spmvHipBlockDot(n, k, up, k, 2, vp, n, 1, op), lambda: lib.spmvHipBlockDot(n, k, up, k - 1, 0, vp, n, 1, op),
                 lambda: lib.spmvHipBlockDot(n, k, up, k, 0, vp, n - 1, 1, op)):
        assert call() == 1
        assert "spmvHipBlockDot" in capfd.readouterr().err
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()
