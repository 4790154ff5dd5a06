"""The test side's reference for spmvHipMultiDot and hipSpGMRESCSR (include/spmvHip.h): `multi_dot_ref` is k calls of
krylov_ref.dot_ref, `gmres_ref` the restarted GMRES(m) loop with CGS2 written out as the header writes it, on
krylov_ref.Csr (serial-order SpMV, the ILU(0) pair).  numpy rounds every product, add, division and square root on its
own, as IEEE double does with no FMA, so the bits are the library's."""
import numpy as np

from krylov_ref import BREAKDOWN, CONVERGED, MAXITER, NONFINITE, _exit, _first_exit, _init, dot_ref

# one label per `return` of the loop: the three of the init, the dropped step (d == 0) at j == 0, and the four of a cycle's
# end.  What ended each cycle goes to stats["ends"]: "d0", or every condition of CYCLE_ENDS that held, joined by "+".
GMRES_EXITS = ("init_converged", "init_nonfinite", "init_maxiter", "d0_cols0", "converged", "nonfinite", "breakdown", "maxiter")
CYCLE_ENDS = ("est", "estnf", "hn0", "restart", "maxiter")


def multi_dot_ref(V, w):
    """h[i] = dot_ref(V[:, i], w)"""
    V = np.asarray(V, dtype=np.float64)
    return np.array([dot_ref(V[:, i], w) for i in range(V.shape[1])], dtype=np.float64)


def gmres_ref(A, b, x0, tol, maxiter, restart, trace=None, stats=None):
    """hipSpGMRESCSR's loop.  Returns (x, status, iterations, history, rr); appends the exit's label (GMRES_EXITS) to
    `trace`; `stats` (a dict, or None) receives cycles (the number of cycles begun) and ends (what ended each)."""
    with np.errstate(all="ignore"):
        x = np.array(x0, dtype=np.float64, copy=True)
        b = np.asarray(b, dtype=np.float64)
        r, rr, bb, thresh = _init(A, b, x, tol)
        hist = [rr]
        ends = []
        if stats is not None:
            stats.update(cycles=0, ends=ends)
        st = _first_exit(rr, thresh, maxiter, trace)
        if st is not None:
            return x, st, 0, np.array(hist), rr
        m = restart
        k = 0
        while True:
            if stats is not None:
                stats["cycles"] += 1
            beta = np.sqrt(rr)
            v = [r / beta]
            g = np.zeros(m + 1)
            g[0] = beta
            cs, sn = np.zeros(m), np.zeros(m)
            R = np.zeros((m, m))
            cols, why = None, None
            for j in range(m):
                z = A.precond(v[j])
                w = A.spmv(z)
                h = np.array([dot_ref(v[i], w) for i in range(j + 1)])
                for i in range(j + 1):
                    w = w - h[i] * v[i]
                c = np.array([dot_ref(v[i], w) for i in range(j + 1)])
                for i in range(j + 1):
                    w = w - c[i] * v[i]
                h = h + c
                ww = dot_ref(w, w)
                hn = np.sqrt(ww)
                for i in range(j):
                    t = cs[i] * h[i] + sn[i] * h[i + 1]
                    h[i + 1] = cs[i] * h[i + 1] - sn[i] * h[i]
                    h[i] = t
                d = np.sqrt(h[j] * h[j] + hn * hn)
                if d == 0:
                    if j == 0:
                        ends.append("d0")
                        return x, _exit(trace, "d0_cols0", BREAKDOWN), k, np.array(hist), rr
                    cols, why = j, "d0"
                    break
                k += 1
                cs[j], sn[j] = h[j] / d, hn / d
                h[j] = d
                R[:j + 1, j] = h
                g[j + 1] = -(sn[j] * g[j])
                g[j] = cs[j] * g[j]
                est = g[j + 1] * g[j + 1]
                hist.append(est)
                why = "+".join(name for name, hit in (("est", est <= thresh), ("estnf", not np.isfinite(est)), ("hn0", hn == 0),
                                                      ("restart", j == m - 1), ("maxiter", k == maxiter)) if hit) or None
                if why is not None:
                    cols = j + 1
                    brk = hn == 0
                    break
                v.append(w / hn)
            if why == "d0":
                brk = True
            ends.append(why)
            y = np.zeros(cols)
            for i in range(cols - 1, -1, -1):
                s = g[i]
                for l in range(i + 1, cols):
                    s = s - R[i, l] * y[l]
                y[i] = s / R[i, i]
            u = y[0] * v[0]
            for i in range(1, cols):
                u = u + y[i] * v[i]
            x = x + A.precond(u)
            q = A.spmv(x)
            r = b - q
            rr = dot_ref(r, r)
            hist[k] = rr
            if rr <= thresh:
                return x, _exit(trace, "converged", CONVERGED), k, np.array(hist), rr
            if not np.isfinite(rr):
                return x, _exit(trace, "nonfinite", NONFINITE), k, np.array(hist), rr
            if brk:
                return x, _exit(trace, "breakdown", BREAKDOWN), k, np.array(hist), rr
            if k == maxiter:
                return x, _exit(trace, "maxiter", MAXITER), k, np.array(hist), rr
