"""spmvHipBlockResidual on the device against tests/davidson_ref.residual_ref, bit for bit: R and the squared norms at the
edges of a wave and of a dot block and at two blocks plus one row, for m around the load chunk and k on each side of every
instance's cap, in the 16-byte and the 8-byte form (even and odd leading dimensions, pointers at element offset 1), R's u
part against api.block_combine and the norms against api.dot, with poisoned neighbours, a NaN and an Inf that stay in their
row, n = 0, every refusal and the Python entry."""
import numpy as np
import pytest

import serial_order_inputs as si
from davidson_ref import residual_ref
from lanczos_ref import combine_ref
from test_gpu_block_combine import _block, _poison, _unblock, _untouched
from test_gpu_trsv import POISON, same

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
# every m of {1, 2, 8, 9, 33, 64} and every k of {1, 3, 4, 5, 8, 9, 16}: each side of the caps 4, 8 and 16 of the instances
MKS = ((1, 1), (2, 3), (8, 4), (9, 5), (33, 8), (64, 9), (64, 16), (1, 16), (2, 9), (8, 8), (9, 1), (33, 3), (20, 4))


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


def _torch():
    return pytest.importorskip("torch")


def _run(api, torch, V, W, S, theta, ldv, ldw, ldr, offv, offw, offr, spare=2):
    """-> (R, norm2, the whole host copy of R's buffer, that of norm2's)"""
    n, m = V.shape
    k = S.shape[1]
    dV = torch.from_numpy(_block(V, n, m, ldv, offv)).cuda()
    dW = torch.from_numpy(_block(W, n, m, ldw, offw)).cuda()
    dS = torch.from_numpy(_block(S, m, k, m + 1, 0)).cuda()
    dT = torch.from_numpy(theta.copy()).cuda()
    dR = torch.from_numpy(_poison(offr + (k + spare - 1) * ldr + n + 5)).cuda()
    dN = torch.from_numpy(_poison(k + 3)).cuda()
    rc = api.lib.spmvHipBlockResidual(n, m, k, dV.data_ptr() + 8 * offv, ldv, dW.data_ptr() + 8 * offw, ldw, dS.data_ptr(), m + 1,
                                      dT.data_ptr(), dR.data_ptr() + 8 * offr, ldr, dN.data_ptr() + 8)
    assert rc == 0
    raw, rawn = dR.cpu().numpy(), dN.cpu().numpy()
    return _unblock(raw, n, k, ldr, offr), rawn[1:1 + k], raw, rawn


def _norms_untouched(rawn, k, what):
    assert rawn.view(np.uint64)[0] == POISON and (rawn.view(np.uint64)[1 + k:] == POISON).all(), what + ": written outside dNorm2[0 .. k-1]"


@pytest.mark.parametrize("n", NS)
def test_residual_bits(api, n):
    torch = _torch()
    ev = n + (n & 1)
    # (ldv, ldw, ldr, offsets of V, W, R): the 16-byte form; an odd ldv; an odd ldr; 8-byte aligned pointers; R alone off
    layouts = ((ev, ev + 2, ev, 0, 0, 0), (ev + 1, ev, ev, 0, 0, 0), (ev, ev, ev + 1, 0, 0, 0), (n, n, n, 1, 1, 1), (ev, ev, ev, 0, 0, 1))
    for m, k in MKS:
        rng = np.random.default_rng(9600 + 131 * n + 7 * m + k)
        V, W = si.order_values(rng, n * m, 8).reshape(n, m), si.order_values(rng, n * m, 8).reshape(n, m)
        S, theta = si.order_values(rng, m * k, 8).reshape(m, k), si.order_values(rng, k, 8)
        refR, refN = residual_ref(V, W, S, theta)
        for ldv, ldw, ldr, offv, offw, offr in layouts:
            what = f"n={n} m={m} k={k} ld={ldv},{ldw},{ldr} offsets {offv},{offw},{offr}"
            R, n2, raw, rawn = _run(api, torch, V, W, S, theta, ldv, ldw, ldr, offv, offw, offr)
            same(R, refR, what + ": R")
            same(n2, refN, what + ": norm2")
            _untouched(raw, n, k, ldr, offr, what)
            _norms_untouched(rawn, k, what)


@pytest.mark.parametrize("n", [65, 4097])
def test_u_part_is_block_combine_and_the_norms_are_dot(api, n):
    """W = 0 and theta = -1 leave R = u, which is api.block_combine(V, S) on the device; norm2[c] is api.dot of R's column"""
    torch = _torch()
    for m, k in ((9, 5), (33, 16)):
        rng = np.random.default_rng(9700 + n + m)
        V, S = si.order_values(rng, n * m, 8).reshape(n, m), si.order_values(rng, m * k, 8).reshape(m, k)
        dV, dS = torch.from_numpy(V.T.copy()).cuda().T, torch.from_numpy(S.T.copy()).cuda().T
        R, n2 = api.block_residual(dV, torch.zeros_like(dV), dS, torch.full((k,), -1.0, dtype=torch.float64).cuda())
        Y = api.block_combine(dV, dS)
        same(R.cpu().numpy(), Y.cpu().numpy(), f"n={n} m={m} k={k}: u")
        same(R.cpu().numpy(), combine_ref(V, S), f"n={n} m={m} k={k}: u against the reference")
        for c in range(k):
            same(n2[c].cpu().numpy(), api.dot(R[:, c].contiguous(), R[:, c].contiguous()).cpu().numpy(), f"norm2[{c}]")


def test_special_values_stay_in_their_row(api):
    torch = _torch()
    n, m, k = 4100, 6, 4
    rng = np.random.default_rng(9800)
    V, W = si.order_values(rng, n * m, 8).reshape(n, m), si.order_values(rng, n * m, 8).reshape(n, m)
    S, theta = si.order_values(rng, m * k, 8).reshape(m, k), si.order_values(rng, k, 8)
    V[6, 2], W[77, 0], W[4099, 5], V[4098, 1] = np.nan, np.inf, np.nan, -np.inf
    V[5, :], W[5, :] = -0.0, -0.0
    with np.errstate(all="ignore"):
        refR, refN = residual_ref(V, W, S, theta)
    bad = np.zeros(n, bool)
    bad[[6, 77, 4098, 4099]] = True
    for ld, off in ((4100, 0), (4101, 1)):
        R, n2, _, _ = _run(api, torch, V, W, S, theta, ld, ld, ld, off, off, off)
        same(R, refR, f"ld={ld}")
        assert not np.isfinite(R[bad]).any() and np.isfinite(R[~bad]).all(), "a NaN or an Inf stays in its row"
        assert np.isnan(n2).all() and np.isnan(refN).all(), "and reaches every norm"


def test_n_zero_and_refusals(api, capfd):
    torch = _torch()
    f = api.lib.spmvHipBlockResidual
    x = torch.ones(4000, dtype=torch.float64).cuda()
    w = torch.ones(4000, dtype=torch.float64).cuda()
    s = torch.ones(64 * 16, dtype=torch.float64).cuda()
    t = torch.ones(16, dtype=torch.float64).cuda()
    r = torch.from_numpy(_poison(4000)).cuda()
    q = torch.from_numpy(_poison(16)).cuda()
    X, W, S_, T, R, Q = (a.data_ptr() for a in (x, w, s, t, r, q))
    assert f(0, 3, 2, None, 0, None, 0, None, 3, None, None, 0, None) == 0          # n = 0: nothing to do, nothing read or written
    assert f(0, 3, 2, X, 0, W, 0, S_, 3, T, R, 0, Q) == 0
    ok = (10, 3, 2, X, 10, W, 10, S_, 3, T, R, 10, Q)
    refused = [ok[:i] + (None,) + ok[i + 1:] for i in (3, 5, 7, 9, 10, 12)]            # every NULL pointer
    refused += [
        (10, 0, 2) + ok[3:], (10, 65, 2, X, 10, W, 10, S_, 65, T, R, 10, Q), (10, 3, 0) + ok[3:], (10, 3, 17) + ok[3:],
        (10, 3, 2, X, 9, W, 10, S_, 3, T, R, 10, Q), (10, 3, 2, X, 10, W, 9, S_, 3, T, R, 10, Q), (10, 3, 2, X, 10, W, 10, S_, 2, T, R, 10, Q),
        (10, 3, 2, X, 10, W, 10, S_, 3, T, R, 9, Q),
        (10, 3, 2, R, 10, W, 10, S_, 3, T, R, 10, Q),                    # R is V
        (10, 3, 2, X, 10, R + 8, 10, S_, 3, T, R, 10, Q),                # W overlaps R
        (10, 3, 2, X, 10, W, 10, R + 16, 3, T, R, 10, Q),                # S inside R
        (10, 3, 2, X, 10, W, 10, S_, 3, R + 8, R, 10, Q),                # theta inside R
        (10, 3, 2, X, 10, W, 10, S_, 3, T, R, 10, R + 8 * 12),           # norm2 inside R
        (10, 3, 2, X, 10, W, 10, S_, 3, Q, R, 10, Q),                    # norm2 is theta
        (10, 3, 2, Q, 10, W, 10, S_, 3, T, R, 10, Q + 8),                # norm2 inside V
    ]
    for i, args in enumerate(refused):
        assert f(*args) == 1, i
    assert (r.cpu().numpy().view(np.uint64) == POISON).all() and (q.cpu().numpy().view(np.uint64) == POISON).all()
    assert "spmvHipBlockResidual" in capfd.readouterr().err
    assert f(10, 3, 2, X, 10, X, 10, S_, 3, T, R, 10, Q) == 0                        # V and W may be one block


def test_residual_through_python(api):
    torch = _torch()
    n, m, k = 6783, 20, 4
    rng = np.random.default_rng(9900)
    V, W = si.order_values(rng, n * m, 8).reshape(n, m), si.order_values(rng, n * m, 8).reshape(n, m)
    S, theta = si.order_values(rng, m * k, 8).reshape(m, k), si.order_values(rng, k, 8)
    refR, refN = residual_ref(V, W, S, theta)
    R, n2 = api.block_residual(V, W, S, theta)
    same(R, refR, "numpy: R")
    same(n2, refN, "numpy: norm2")
    cols = lambda a: torch.from_numpy(a.T.copy()).cuda().T               # noqa: E731  (contiguous columns)
    Rt, nt = api.block_residual(cols(V), cols(W), cols(S), torch.from_numpy(theta).cuda())
    assert Rt.is_cuda and Rt.shape == (n, k) and Rt.stride(0) == 1 and nt.shape == (k,)
    same(Rt.cpu().numpy(), refR, "torch: R")
    same(nt.cpu().numpy(), refN, "torch: norm2")
    with pytest.raises(api.SpmvHipError):
        api.block_residual(V, W[:, :-1], S, theta)
    with pytest.raises(api.SpmvHipError):
        api.block_residual(V, W, S[:-1], theta)
    with pytest.raises(api.SpmvHipError):
        api.block_residual(V, W, S, theta[:-1])
