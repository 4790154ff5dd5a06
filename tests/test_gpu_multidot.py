"""spmvHipMultiDot on the device: every entry is the bits of tests/gmres_ref.multi_dot_ref and of spmvHipDot on its column,
at the block boundaries, for k below, at and above the panel width, for leading dimensions that leave every second column
8-byte aligned, with special values, refusals and one graph capture; and the square root of the bit-for-bit path
through 1 x 1 GMRES solves."""
import ctypes as C

import numpy as np
import pytest

import serial_order_inputs as si
from gmres_ref import gmres_ref, multi_dot_ref
from krylov_ref import Csr
from test_gpu_trsv import POISON, same

pytestmark = pytest.mark.gpu

BIG = 256 * 4096 + 4097                 # 258 block partials: two lanes of the second level add two


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


def _torch():
    return pytest.importorskip("torch")


def _values(rng, n, k, ldv):
    """V as (k, ldv) rows = columns of the device matrix, w with one spare element in front"""
    V = si.order_values(rng, k * ldv, 8).reshape(k, ldv) if k * ldv else np.zeros((k, ldv))
    w = si.order_values(rng, n + 1, 8)
    return V, w


def _run(api, torch, V, w, n, k, ldv, spare=3):
    dV = torch.from_numpy(V.ravel()).cuda()
    dw = torch.from_numpy(w).cuda()[1:]                                  # a view at element offset 1
    out = torch.from_numpy(np.full(k + spare, POISON, np.uint64).view(np.float64)).cuda()
    assert api.lib.spmvHipMultiDot(n, k, dV.data_ptr(), ldv, dw.data_ptr(), out.data_ptr()) == 0
    h = out.cpu().numpy()
    assert (h[k:].view(np.uint64) == POISON).all(), "dH written past k"
    dots = torch.empty(k, dtype=torch.float64).cuda()
    for i in range(k):
        assert api.lib.spmvHipDot(n, dV.data_ptr() + 8 * i * ldv, dw.data_ptr(), dots.data_ptr() + 8 * i) == 0
    return h[:k], dots.cpu().numpy()


@pytest.mark.parametrize("n", [0, 1, 2, 4095, 4096, 4097, 21 * 19 * 17])
@pytest.mark.parametrize("k", [1, 2, 3, 16, 17, 64, 65])
def test_multidot_bits(api, n, k):
    torch = _torch()
    for pad in (0, 1, 7):
        ldv = n + pad
        rng = np.random.default_rng(7000 + n % 997 + 31 * k + pad)
        V, w = _values(rng, n, k, ldv)
        h, dots = _run(api, torch, V, w, n, k, ldv)
        ref = multi_dot_ref(V[:, :n].T, w[1:]) if n else np.zeros(k)
        same(h, ref, f"n={n} k={k} ldv=n+{pad}: the reference")
        same(h, dots, f"n={n} k={k} ldv=n+{pad}: k calls of spmvHipDot")


def test_multidot_second_level_adds_two(api):
    torch = _torch()
    n, k = BIG, 3
    for pad in (0, 1):
        V, w = _values(np.random.default_rng(7100 + pad), n, k, n + pad)
        h, dots = _run(api, torch, V, w, n, k, n + pad)
        same(h, multi_dot_ref(V[:, :n].T, w[1:]), f"ldv=n+{pad}: the reference")
        same(h, dots, f"ldv=n+{pad}: k calls of spmvHipDot")


def test_multidot_special_values(api):
    """+-0.0, subnormals, +-Inf and NaN in single positions, compared as bit patterns (NaN where NaN is)"""
    torch = _torch()
    n, k = 2 * 4096 + 5, 5
    for pad in (0, 1):
        ldv = n + pad
        V, w = _values(np.random.default_rng(7200 + pad), n, k, ldv)
        V[0, 7], V[0, 4100], w[1 + 9] = -0.0, 5e-324, 2.2e-308
        V[1, 100], V[2, 4097], V[3, 8000] = np.inf, -np.inf, np.nan
        V[4, :] = -0.0
        for i in (100, 4097):                                            # w > 0 there: the infinities keep their signs
            w[1 + i] = abs(w[1 + i]) + 1.0
        h, dots = _run(api, torch, V, w, n, k, ldv)
        with np.errstate(all="ignore"):
            ref = multi_dot_ref(V[:, :n].T, w[1:])
        same(h, ref, f"ldv=n+{pad}")
        same(h, dots, f"ldv=n+{pad}: spmvHipDot")
        assert h[1] == np.inf and h[2] == -np.inf and np.isnan(h[3])
        assert h[4] == 0.0 and not np.signbit(h[4])


def test_multidot_through_python(api):
    torch = _torch()
    n, k = 6783, 5
    rng = np.random.default_rng(7300)
    V, w = si.order_values(rng, n * k, 8).reshape(k, n), si.order_values(rng, n, 8)
    ref = multi_dot_ref(V.T, w)
    got = api.multi_dot(torch.from_numpy(V).cuda().T, torch.from_numpy(w).cuda())
    assert got.is_cuda and got.shape == (k,)
    same(got.cpu().numpy(), ref, "torch")
    same(api.multi_dot(np.asfortranarray(V.T), w), ref, "numpy")
    with pytest.raises(api.SpmvHipError):
        api.multi_dot(torch.from_numpy(V).cuda(), torch.from_numpy(w).cuda()[:k])   # rows contiguous, not columns


def test_multidot_refusals_leave_dH_untouched(api, capfd):
    torch = _torch()
    x = torch.ones(40, dtype=torch.float64).cuda()
    out = torch.from_numpy(np.full(4, POISON, np.uint64).view(np.float64)).cuda()
    f = api.lib.spmvHipMultiDot
    assert f(10, 2, x.data_ptr(), 10, x.data_ptr(), None) == 1
    assert f(10, 2, None, 10, x.data_ptr(), out.data_ptr()) == 1
    assert f(10, 2, x.data_ptr(), 10, None, out.data_ptr()) == 1
    assert f(10, 0, x.data_ptr(), 10, x.data_ptr(), out.data_ptr()) == 1
    assert f(10, 2, x.data_ptr(), 9, x.data_ptr(), out.data_ptr()) == 1
    assert (out.cpu().numpy().view(np.uint64) == POISON).all()
    assert "spmvHipMultiDot" in capfd.readouterr().err
    assert f(0, 2, None, 0, None, out.data_ptr()) == 0                   # n = 0: k times +0.0
    h = out.cpu().numpy()
    assert (h[:2].view(np.uint64) == 0).all() and (h[2:].view(np.uint64) == POISON).all()


def test_multidot_capture_and_replay(api):
    """a call that needs no growth of the workspace only enqueues: captured once, replayed on new values"""
    torch = _torch()
    n, k, ldv = 3 * 4096 + 5, 6, 3 * 4096 + 6
    rng = np.random.default_rng(7400)
    V, w = _values(rng, n, k, ldv)
    dV, dw = torch.from_numpy(V.ravel()).cuda(), torch.from_numpy(w[1:].copy()).cuda()
    out = torch.zeros(k, dtype=torch.float64).cuda()
    s = torch.cuda.Stream()
    try:
        assert api.lib.spmvHipMultiDot(n, k, dV.data_ptr(), ldv, dw.data_ptr(), out.data_ptr()) == 0   # grows the workspace
        api.lib.spmvHipSetStream(C.c_void_p(s.cuda_stream))
        api.lib.spmvHipSetSync(0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert api.lib.spmvHipMultiDot(n, k, dV.data_ptr(), ldv, dw.data_ptr(), out.data_ptr()) == 0
        w2 = si.order_values(rng, n, 8)
        dw.copy_(torch.from_numpy(w2))
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(out.cpu().numpy(), multi_dot_ref(V[:, :n].T, w2), "replayed")
    finally:
        api.lib.spmvHipSetSync(1)
        api.lib.spmvHipSetStream(None)


def _sweep():
    """some hundred values of c whose squares cover subnormal results, odd and even exponents and the neighbours of
    powers of two"""
    vals = []
    for e in (-537, -520, -511, -510, -100, -1, 0, 1, 2, 51, 100, 300, 511):
        for m in (1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 1.5, 1.4142135623730951, 1.4142135623730949, 1.75, 1.1):
            vals.append(m * 2.0 ** e)
    vals += list(np.random.default_rng(7500).uniform(0.5, 2.0, 60) * 2.0 ** np.random.default_rng(7501).integers(-530, 500, 60))
    return [float(v) for v in vals]


def test_sqrt_is_correctly_rounded_through_gmres(api):
    """A = [a], b = [c]: beta = sqrt(c^2), v[0] = c / beta, hn = sqrt(0) and d = sqrt(h^2): info.rr, the history and x
    equal the reference (np.sqrt is IEEE's correctly rounded root)"""
    cs = _sweep()
    assert len(cs) >= 150
    one = np.array([0, 1], np.uint64)
    for a in (1.0, 3.0):
        A = api.spMatCpyCSR(api.HostCSR(1, 1, one, np.zeros(1, np.uint64), np.array([a])))
        try:
            for c in cs:
                b = np.array([c])
                with np.errstate(all="ignore"):
                    rx, st, it, rh, rrr = gmres_ref(Csr(1, one, np.zeros(1, np.uint64), np.array([a])), b, np.zeros(1), 0.0, 3, 2)
                x, info = A.gmres(b, tol=0.0, maxiter=3, restart=2, history=True)
                what = f"a={a} c={c!r}"
                assert (info.status, info.iterations) == (st, it), what
                same(x, rx, what + ": x")
                same(info.history, rh, what + ": history")
                same(np.array([info.rr]), np.array([rrr]), what + ": rr")
        finally:
            A.free()
