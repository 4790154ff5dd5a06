"""The test side's reference for spmvHipBlockCombine and hipSpLanczosCSR (include/spmvHip.h): `combine_ref` is the
in-order rounded sum Y = V S, `jacobi_ref` the cyclic-by-row Jacobi method with the header's conventions, `lanczos_ref`
the thick-restart Lanczos loop with CGS2 written out as the header writes it, on krylov_ref.Csr (serial-order SpMV) and
krylov_ref.dot_ref.  numpy rounds every product, add, division and square root on its own, as IEEE double does with no
FMA, so the bits are the library's."""
import numpy as np

from krylov_ref import BREAKDOWN, CONVERGED, MAXITER, NONFINITE, dot_ref

LARGEST, SMALLEST = 0, 1
MAX_NCV = 64
JACOBI_SWEEPS = 30
# one label per `return` of the loop
LANCZOS_EXITS = ("v0_nonfinite", "v0_zero", "init_maxiter", "step_nonfinite", "jacobi_nonfinite", "converged", "breakdown",
                 "maxiter")


def default_keep(nev, m):
    """columns a restart keeps when opts.keep == 0"""
    return min(m - 1, nev + (m - nev) // 2)


def combine_ref(V, S):
    """Y[:, c] = sum_j V[:, j] * S[j, c], j ascending from +0.0, every product and every add rounded on its own"""
    V, S = np.asarray(V, dtype=np.float64), np.asarray(S, dtype=np.float64)
    Y = np.zeros((V.shape[0], S.shape[1]))
    with np.errstate(all="ignore"):
        for c in range(S.shape[1]):
            acc = np.zeros(V.shape[0])
            for j in range(S.shape[0]):
                acc = acc + V[:, j] * S[j, c]
            Y[:, c] = acc
    return Y


def jacobi_ref(T):
    """cyclic-by-row Jacobi on the symmetric T.  Returns (diagonal, S, sweeps), S accumulated from the identity (column i
    goes with diagonal[i], unsorted), or None when JACOBI_SWEEPS sweeps did not end with a sweep without a rotation."""
    n = T.shape[0]
    A = np.array(T, dtype=np.float64, copy=True)
    S = np.eye(n)
    one, two = np.float64(1.0), np.float64(2.0)
    with np.errstate(all="ignore"):
        for sweep in range(1, JACOBI_SWEEPS + 1):
            rotated = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[p, q]
                    if apq == 0:
                        continue
                    app, aqq, g = A[p, p], A[q, q], abs(apq)
                    if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):    # negligible: zeroed, no rotation
                        A[p, q] = A[q, p] = 0.0
                        continue
                    rotated = True
                    th = (aqq - app) / (two * apq)
                    t = one / (abs(th) + np.sqrt(th * th + one))
                    if th < 0:
                        t = -t
                    c = one / np.sqrt(t * t + one)
                    s = t * c
                    tau = s / (one + c)
                    h = t * apq
                    ap, aq = A[:, p].copy(), A[:, q].copy()
                    A[:, p] = ap - s * (aq + tau * ap)
                    A[:, q] = aq + s * (ap - tau * aq)
                    A[p, :] = A[:, p]
                    A[q, :] = A[:, q]
                    A[p, p], A[q, q] = app - h, aqq + h
                    A[p, q] = A[q, p] = 0.0
                    sp, sq = S[:, p].copy(), S[:, q].copy()
                    S[:, p] = sp - s * (sq + tau * sp)
                    S[:, q] = sq + s * (sp - tau * sq)
            if not rotated:
                return np.diag(A).copy(), S, sweep
    return None


def ritz_order(d, which):
    """the columns of a Jacobi result in the order of the wanted end: ascending for SMALLEST, descending for LARGEST,
    equal values by ascending index"""
    return np.argsort(d if which == SMALLEST else -d, kind="stable")


def lanczos_ref(A, v0, nev, ncv, which, tol, maxiter, keep=0, trace=None, stats=None, one_pass=False):
    """hipSpLanczosCSR's loop.  Returns (theta[found], res[found], X (n x found), status, found, iterations, cycles);
    appends the exit's label (LANCZOS_EXITS) to `trace`; `stats` (a dict, or None) receives scale, sweeps (the most
    sweeps a Jacobi call took), steps (the Lanczos steps of each cycle) and exact.  one_pass plants the fault of a
    single projection pass (tests only)."""
    n, m = A.M, ncv
    none = (np.zeros(0), np.zeros(0), np.zeros((n, 0)))
    info = dict(scale=0.0, sweeps=0, steps=[], exact=False)
    if stats is not None:
        stats.update(info)
        info = stats

    def leave(label, status, out=none, it=0, cycles=0):
        if trace is not None:
            trace.append(label)
        return out + (status, out[0].size, it, cycles)

    with np.errstate(all="ignore"):
        v0 = np.asarray(v0, dtype=np.float64)
        nn = dot_ref(v0, v0)
        if not np.isfinite(nn):
            return leave("v0_nonfinite", NONFINITE)
        if nn == 0:
            return leave("v0_zero", BREAKDOWN)
        if maxiter == 0:
            return leave("init_maxiter", MAXITER)
        V = np.zeros((n, m + 1))
        V[:, 0] = v0 / np.sqrt(nn)
        T = np.zeros((m, m))
        k, it, cycles = 0, 0, 0
        kk = keep if keep else default_keep(nev, m)
        while True:
            cycles += 1
            cols, exact, beta = m, False, None
            for j in range(k, m):
                w = A.spmv(V[:, j])
                it += 1
                h = np.array([dot_ref(V[:, i], w) for i in range(j + 1)])
                for i in range(j + 1):
                    w = w - h[i] * V[:, i]
                c = np.zeros(j + 1) if one_pass else np.array([dot_ref(V[:, i], w) for i in range(j + 1)])
                if not one_pass:
                    for i in range(j + 1):
                        w = w - c[i] * V[:, i]
                alpha = h[j] + c[j]
                T[j, j] = alpha
                beta = np.sqrt(dot_ref(w, w))
                if not (np.isfinite(alpha) and np.isfinite(beta)):
                    info["steps"].append(j + 1 - k)
                    return leave("step_nonfinite", NONFINITE, none, it, cycles)
                if beta == 0:
                    cols, exact = j + 1, True
                    break
                V[:, j + 1] = w / beta
                if j + 1 < m:
                    T[j, j + 1] = T[j + 1, j] = beta
                if it == maxiter:
                    cols = j + 1
                    break
            info["steps"].append(cols - k)
            info["exact"] = exact
            jac = jacobi_ref(T[:cols, :cols])
            if jac is None or not np.all(np.isfinite(jac[0])):
                info["sweeps"] = JACOBI_SWEEPS if jac is None else max(info["sweeps"], jac[2])
                return leave("jacobi_nonfinite", NONFINITE, none, it, cycles)
            d, S, sweeps = jac
            info["sweeps"] = max(info["sweeps"], sweeps)
            order = ritz_order(d, which)
            theta, S = d[order], S[:, order]
            res = np.zeros(cols) if exact else np.abs(beta * S[cols - 1, :])
            scale = np.max(np.abs(theta))
            info["scale"] = float(scale)
            found = min(nev, cols)
            done = cols >= nev and bool(np.all(res[:nev] <= np.float64(tol) * scale))
            if done or exact or it == maxiter:
                out = (theta[:found].copy(), res[:found].copy(), combine_ref(V[:, :cols], S[:, :found]))
                if done:
                    return leave("converged", CONVERGED, out, it, cycles)
                if exact:
                    return leave("breakdown", BREAKDOWN, out, it, cycles)
                return leave("maxiter", MAXITER, out, it, cycles)
            V[:, :kk] = combine_ref(V[:, :m], S[:, :kk])
            V[:, kk] = V[:, m]
            T[:] = 0.0
            for i in range(kk):
                T[i, i] = theta[i]
                T[kk, i] = T[i, kk] = beta * S[m - 1, i]
            k = kk
