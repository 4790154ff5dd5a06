"""What the GPU tests of the multigrid hierarchies share (test_gpu_amg.py, test_gpu_amg_sa.py, test_gpu_amg_strength.py,
test_gpu_amg_cheb.py): moving matrices and arrays, comparing bits, the solve against a reference loop, and the launch
count of a cycle.  A plain module: the fixtures stay in the test files, where they differ."""
import ctypes as C

import numpy as np

from bits import assert_same_bits


def _up(api, A):
    return api.spMatCpyCSR(api.HostCSR(*A))


def _down(api, ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
    return out


def _same(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN places"
    assert_same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what)


def _bits(x):
    return np.float64(x).view(np.uint64)


def _blob(v):
    """the bytes of a downloaded piece: an array, a number, None, or a tuple of them"""
    if isinstance(v, tuple):
        return b"|".join(_blob(t) for t in v)
    return b"" if v is None else np.asarray(v).tobytes()


def _special_r(M):
    r = np.random.default_rng(7).standard_normal(M)
    r[[3, 100, 511]] = 0.0
    r[[4, 101]] = -0.0
    r[200], r[201], r[300] = np.inf, -np.inf, np.nan
    return r


def _solve_and_compare(da, b, precond, method, want, tol, **kw):
    """da.<method>(b) with the hierarchy `precond` against the reference loop's (x, status, iterations, history, _)"""
    x, info = getattr(da, method)(b, precond=precond, tol=tol, maxiter=200, history=True, **kw)
    wx, wstatus, wit, whist, _ = want
    assert (info.status, info.iterations) == (wstatus, wit), method
    assert_same_bits(x, wx, f"{method}: x")
    assert_same_bits(info.history, whist, f"{method}: history")
    return info


def cycle_launches(nu1, nu2, nuCoarse, levels, unfused=0):
    """the kernels one cycle enqueues, an SpMV counted as one (include/spmvHip.h), whatever the smoother: n sweeps from
    nothing are one pass and two kernels per further sweep; above the last level come the residual's SpMV and pass, the
    restriction, the correction and two kernels per post-sweep; a smoothed level whose correction is an SpMV and an add
    (`unfused` of them) takes one more"""
    def start(n):
        return 1 + 2 * (max(n, 1) - 1)
    return (levels - 1) * (start(nu1) + 3 + 1 + 2 * nu2) + start(nuCoarse) + unfused
