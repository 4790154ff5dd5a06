"""spmvHipBlockCombine on the device against tests/lanczos_ref.combine_ref, bit for bit: at the workgroup boundaries of
both forms, for m at and around the four register widths, for the 16-byte and the 8-byte form (even and odd leading
dimensions, pointers at element offset 1), in place at k < m and k = m, with poisoned neighbours, signed zeros and a NaN
that stay in their row, n = 0, the refusals, the Python entry and one graph capture."""
import ctypes as C

import numpy as np
import pytest

import serial_order_inputs as si
from lanczos_ref import combine_ref
from test_gpu_trsv import POISON, same

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 4097)
MKS = ((1, 1), (2, 1), (3, 3), (17, 5), (64, 64), (64, 1))


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


def _torch():
    return pytest.importorskip("torch")


def _poison(count):
    return np.full(count, POISON, dtype=np.uint64).view(np.float64)


def _block(values, rows, cols, ld, off):
    """a column-major rows x cols block of leading dimension ld at element offset `off` of a poisoned host buffer"""
    host = _poison(off + max(cols - 1, 0) * ld + rows + 5)
    for c in range(cols):
        host[off + c * ld:off + c * ld + rows] = values[:, c]
    return host


def _unblock(host, rows, cols, ld, off):
    return np.stack([host[off + c * ld:off + c * ld + rows] for c in range(cols)], axis=1) if cols else np.zeros((rows, 0))


def _untouched(host, rows, cols, ld, off, what):
    mask = np.ones(host.size, bool)
    for c in range(cols):
        mask[off + c * ld:off + c * ld + rows] = False
    assert (host.view(np.uint64)[mask] == POISON).all(), what + ": written outside the n x k block"


def _run(api, torch, V, S, ldv, ldy, offv, offy, lds=None, spare=2):
    n, m = V.shape
    k = S.shape[1]
    lds = m + 1 if lds is None else lds
    dV = torch.from_numpy(_block(V, n, m, ldv, offv)).cuda()
    dS = torch.from_numpy(_block(S, m, k, lds, 0)).cuda()
    hostY = _poison(offy + (k + spare - 1) * ldy + n + 5)
    dY = torch.from_numpy(hostY).cuda()
    rc = api.lib.spmvHipBlockCombine(n, m, k, dV.data_ptr() + 8 * offv, ldv, dS.data_ptr(), lds, dY.data_ptr() + 8 * offy, ldy)
    assert rc == 0
    out = dY.cpu().numpy()
    return _unblock(out, n, k, ldy, offy), out


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("mk", MKS, ids=[f"m{m}k{k}" for m, k in MKS])
def test_combine_bits(api, n, mk):
    torch = _torch()
    m, k = mk
    rng = np.random.default_rng(9000 + 131 * n + 7 * m + k)
    V = si.order_values(rng, n * m, 8).reshape(n, m)
    S = si.order_values(rng, m * k, 8).reshape(m, k)
    ref = combine_ref(V, S)
    ev = n + (n & 1)
    # (ldv, ldy, offset of V, offset of Y): the 16-byte form where m <= 32; an odd ldv, an odd ldy, 8-byte aligned pointers
    for ldv, ldy, offv, offy in ((ev, ev + 2, 0, 0), (ev + 1, ev, 0, 0), (ev, ev + 1, 0, 0), (ev, ev, 1, 0), (ev, ev, 0, 1), (n, n, 1, 1)):
        what = f"n={n} m={m} k={k} ldv={ldv} ldy={ldy} offsets {offv}, {offy}"
        Y, raw = _run(api, torch, V, S, ldv, ldy, offv, offy)
        same(Y, ref, what)
        _untouched(raw, n, k, ldy, offy, what)


def test_combine_register_widths(api):
    """m at and next to 8, 16 and 32, where another instance of the kernel takes over; k above m"""
    torch = _torch()
    n = 515
    for m in (7, 8, 9, 15, 16, 17, 31, 32, 33, 63):
        rng = np.random.default_rng(9100 + m)
        V, S = si.order_values(rng, n * m, 8).reshape(n, m), si.order_values(rng, m * (m + 1), 8).reshape(m, m + 1)
        for ld, off in ((516, 0), (517, 1)):
            Y, raw = _run(api, torch, V, S, ld, ld, off, off)
            same(Y, combine_ref(V, S), f"m={m} ld={ld}")
            _untouched(raw, n, m + 1, ld, off, f"m={m} ld={ld}")


@pytest.mark.parametrize("mk", [(20, 12), (5, 5), (64, 64), (64, 32), (33, 1)], ids=str)
def test_combine_in_place(api, mk):
    """dY == dV: columns 0 .. k-1 of V become Y, columns k .. m-1 and everything around the block stay"""
    torch = _torch()
    m, k = mk
    for n, ld, off in ((4097, 4098, 0), (4097, 4099, 1), (65, 65, 0)):
        rng = np.random.default_rng(9200 + m + k + n)
        V, S = si.order_values(rng, n * m, 8).reshape(n, m), si.order_values(rng, m * k, 8).reshape(m, k)
        host = _block(V, n, m, ld, off)
        dV = torch.from_numpy(host).cuda()
        dS = torch.from_numpy(np.asfortranarray(S).ravel(order="F")).cuda()
        p = dV.data_ptr() + 8 * off
        assert api.lib.spmvHipBlockCombine(n, m, k, p, ld, dS.data_ptr(), m, p, ld) == 0
        out = dV.cpu().numpy()
        got = _unblock(out, n, m, ld, off)
        what = f"in place n={n} m={m} k={k} ld={ld}"
        same(got[:, :k], combine_ref(V, S), what)
        same(got[:, k:], V[:, k:], what + ": the columns past k")
        _untouched(out, n, m, ld, off, what)


def test_combine_special_values_stay_in_their_row(api):
    torch = _torch()
    n, m, k = 130, 6, 4
    rng = np.random.default_rng(9300)
    V, S = si.order_values(rng, n * m, 8).reshape(n, m), si.order_values(rng, m * k, 8).reshape(m, k)
    V[5, :] = -0.0
    V[6, 2], V[77, 0], V[78, 5] = np.nan, np.inf, -np.inf
    S[1, 3] = -0.0
    S[0, :] = np.abs(S[0, :]) + 1.0
    with np.errstate(all="ignore"):
        ref = combine_ref(V, S)
    for ld, off in ((130, 0), (131, 1)):
        Y, _ = _run(api, torch, V, S, ld, ld, off, off)
        same(Y, ref, f"ld={ld}")
        assert (Y[5].view(np.uint64) == 0).all(), "a row of -0.0 sums to +0.0"
        assert np.isnan(Y[6]).all() and np.isfinite(np.delete(Y, (6, 77, 78), axis=0)).all()
        assert (Y[77] == np.inf).all()


def test_combine_n_zero_and_refusals(api, capfd):
    torch = _torch()
    f = api.lib.spmvHipBlockCombine
    x = torch.ones(4000, dtype=torch.float64).cuda()
    s = torch.ones(64 * 64, dtype=torch.float64).cuda()
    y = torch.from_numpy(_poison(4000)).cuda()
    X, S_, Y = x.data_ptr(), s.data_ptr(), y.data_ptr()
    assert f(0, 3, 2, None, 0, None, 3, None, 0) == 0                    # n = 0: nothing to do, nothing read
    assert f(0, 3, 2, X, 0, S_, 3, Y, 0) == 0
    refused = [
        (10, 3, 2, None, 10, S_, 3, Y, 10), (10, 3, 2, X, 10, None, 3, Y, 10), (10, 3, 2, X, 10, S_, 3, None, 10),
        (10, 0, 2, X, 10, S_, 3, Y, 10), (10, 3, 0, X, 10, S_, 3, Y, 10), (10, 65, 2, X, 10, S_, 65, Y, 10), (10, 3, 65, X, 10, S_, 3, Y, 10),
        (10, 3, 2, X, 9, S_, 3, Y, 10), (10, 3, 2, X, 10, S_, 3, Y, 9), (10, 3, 2, X, 10, S_, 2, Y, 10),
        (10, 2, 3, Y, 10, S_, 2, Y, 10),                                 # in place with k > m
        (10, 3, 2, Y, 12, S_, 3, Y, 10),                                 # in place with another leading dimension
        (10, 3, 2, Y + 8, 10, S_, 3, Y, 10),                             # overlapping without being the same block
        (10, 3, 2, X, 10, Y + 16, 3, Y, 10),                             # S inside Y
    ]
    for i, args in enumerate(refused):
        assert f(*args) == 1, i
    assert (y.cpu().numpy().view(np.uint64) == POISON).all()
    assert "spmvHipBlockCombine" in capfd.readouterr().err


def test_combine_through_python(api):
    torch = _torch()
    n, m, k = 6783, 20, 12
    rng = np.random.default_rng(9400)
    V, S = si.order_values(rng, n * m, 8).reshape(n, m), si.order_values(rng, m * k, 8).reshape(m, k)
    ref = combine_ref(V, S)
    same(api.block_combine(V, S), ref, "numpy")
    got = api.block_combine(torch.from_numpy(V.T.copy()).cuda().T, torch.from_numpy(S.T.copy()).cuda().T)
    assert got.is_cuda and got.shape == (n, k) and got.stride(0) == 1
    same(got.cpu().numpy(), ref, "torch")
    with pytest.raises(api.SpmvHipError):
        api.block_combine(torch.from_numpy(V).cuda(), torch.from_numpy(S.T.copy()).cuda().T)   # rows contiguous, not columns
    with pytest.raises(api.SpmvHipError):
        api.block_combine(V, S[:-1])


def test_combine_capture_and_replay(api):
    """kernels only: captured once, replayed on new values"""
    torch = _torch()
    n, m, k = 5000, 9, 4
    rng = np.random.default_rng(9500)
    V, S = si.order_values(rng, n * m, 8).reshape(n, m), si.order_values(rng, m * k, 8).reshape(m, k)
    dV = torch.from_numpy(np.asfortranarray(V).ravel(order="F")).cuda()
    dS = torch.from_numpy(np.asfortranarray(S).ravel(order="F")).cuda()
    dY = torch.zeros(n * k, dtype=torch.float64).cuda()
    s = torch.cuda.Stream()
    try:
        api.lib.spmvHipSetStream(C.c_void_p(s.cuda_stream))
        api.lib.spmvHipSetSync(0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert api.lib.spmvHipBlockCombine(n, m, k, dV.data_ptr(), n, dS.data_ptr(), m, dY.data_ptr(), n) == 0
        S2 = si.order_values(rng, m * k, 8).reshape(m, k)
        dS.copy_(torch.from_numpy(np.asfortranarray(S2).ravel(order="F")))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(dY.cpu().numpy().reshape(k, n).T, combine_ref(V, S2), "replayed")
    finally:
        api.lib.spmvHipSetSync(1)
        api.lib.spmvHipSetStream(None)
