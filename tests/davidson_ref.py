"""The test side's reference for spmvHipBlockResidual and hipSpDavidsonCSR (include/spmvHip.h): `residual_ref` is the
residual block R = W S - (V S) diag(theta) with the squared norms of its columns, `davidson_ref` the generalised Davidson
loop with CGS2 and thick restart written out as the header writes it, on krylov_ref.Csr (serial-order SpMV),
krylov_ref.dot_ref and the Jacobi method, the rotation and the ordering of lanczos_ref.  M^-1 is a callable -- the
`precond` method of any of the references the Krylov tests use (krylov_ref.Csr with ILU(0) factors, sweeps_ref.SweepCsr,
fsai_ref.PrecondCsr, amg_ref.AmgCsr and its smoother and storage variants).  numpy rounds every product, add, division and
square root on its own, as IEEE double does with no FMA, so the bits are the library's."""
import numpy as np

from krylov_ref import BREAKDOWN, CONVERGED, MAXITER, NONFINITE, dot_ref
from lanczos_ref import JACOBI_SWEEPS, LARGEST, SMALLEST, combine_ref, default_keep, jacobi_ref, ritz_order

MAX_NEV = 16
# one label per `return` of the loop
DAVIDSON_EXITS = ("v0_nonfinite", "v0_zero", "init_maxiter", "h_nonfinite", "jacobi_nonfinite", "res_nonfinite", "beta_nonfinite",
                  "converged", "maxiter", "breakdown")
# the mistakes the exit table must tell apart (tests only)
FAULTS = ("one pass", "target 0", "descending", "rounding", "full H")


def residual_ref(V, W, S, theta, fault=None):
    """(R, norm2): R[:, c] = (W S)[:, c] - theta[c] * (V S)[:, c], both sums in ascending j from +0.0, the product rounded
    before the subtraction; norm2[c] = dot_ref(R[:, c], R[:, c])"""
    V, W, S = (np.asarray(a, dtype=np.float64) for a in (V, W, S))
    theta = np.asarray(theta, dtype=np.float64)
    with np.errstate(all="ignore"):
        if fault == "rounding":                                  # R = (W - theta V) S
            R = np.stack([combine_ref(W - theta[c] * V, S[:, c:c + 1])[:, 0] for c in range(S.shape[1])], axis=1)
        elif fault == "descending":
            u, q = combine_ref(V[:, ::-1], S[::-1]), combine_ref(W[:, ::-1], S[::-1])
            R = q - theta[None, :] * u
        else:
            R = combine_ref(W, S) - theta[None, :] * combine_ref(V, S)
    return R, np.array([dot_ref(R[:, c], R[:, c]) for c in range(R.shape[1])])


def launches(stats, precond_launches=0):
    """info.launches by the header's formula from the counts a davidson_ref run leaves in `stats`"""
    return (3 + 3 * stats["products"] + 2 * stats["residuals"] + (8 + precond_launches) * stats["expansions"] + 2 * stats["restarts"]
            + stats["x"])


def davidson_ref(A, v0, nev, ncv, which, tol, maxiter, keep=0, precond=None, trace=None, stats=None, fault=None):
    """hipSpDavidsonCSR's loop.  Returns (theta[found], res[found], X (n x found), status, found, iterations, restarts);
    appends the exit's label (DAVIDSON_EXITS) to `trace`; `stats` (a dict, or None) receives scale, sweeps (the most sweeps a
    Jacobi call took), the counts of the launch formula (products and expansions ENQUEUED, residuals, restarts, x),
    applies, checks (the read-backs), targets (the l of every expansion) and cols (the columns at every residual)."""
    n, m = A.M, ncv
    none = (np.zeros(0), np.zeros(0), np.zeros((n, 0)))
    info = dict(scale=0.0, sweeps=0, products=0, residuals=0, expansions=0, restarts=0, x=0, applies=0, checks=0, targets=[], cols=[])
    if stats is not None:
        stats.update(info)
        info = stats

    def leave(label, status, out=none, it=0):
        if trace is not None:
            trace.append(label)
        info["x"] = 1 if out[0].size else 0
        return out + (status, out[0].size, it, info["restarts"])

    with np.errstate(all="ignore"):
        v0 = np.asarray(v0, dtype=np.float64)
        nn = dot_ref(v0, v0)
        if not np.isfinite(nn):
            return leave("v0_nonfinite", NONFINITE)
        if nn == 0:
            return leave("v0_zero", BREAKDOWN)
        if maxiter == 0:
            return leave("init_maxiter", MAXITER)
        V, W = np.zeros((n, m)), np.zeros((n, m))
        V[:, 0] = v0 / np.sqrt(nn)
        H = np.zeros((m, m))
        cols = it = 0
        kk = keep if keep else default_keep(nev, m)
        tolerance = np.float64(tol)
        while True:
            j = cols
            W[:, j] = A.spmv(V[:, j])
            it += 1
            info["products"] += 1
            info["checks"] += 1
            for i in range(j + 1):
                H[i, j] = H[j, i] = dot_ref(V[:, i], W[:, j])
            cols = j + 1
            if not np.all(np.isfinite(H[:cols, j])):
                return leave("h_nonfinite", NONFINITE, none, it)
            jac = jacobi_ref(H[:cols, :cols])
            if jac is None or not np.all(np.isfinite(jac[0])):
                info["sweeps"] = JACOBI_SWEEPS if jac is None else max(info["sweeps"], jac[2])
                return leave("jacobi_nonfinite", NONFINITE, none, it)
            d, S, sweeps = jac
            info["sweeps"] = max(info["sweeps"], sweeps)
            order = ritz_order(d, which)
            theta, S = d[order], S[:, order]
            scale = np.max(np.abs(theta))
            info["scale"] = float(scale)
            c = min(nev, cols)
            R, n2 = residual_ref(V[:, :cols], W[:, :cols], S[:, :c], theta[:c], fault)
            info["residuals"] += 1
            info["checks"] += 1
            info["cols"].append(cols)
            res = np.sqrt(n2)
            if not np.all(np.isfinite(res)):
                return leave("res_nonfinite", NONFINITE, none, it)
            done = cols >= nev and bool(np.all(res[:nev] <= tolerance * scale))
            if done or it == maxiter:
                out = (theta[:c].copy(), res.copy(), combine_ref(V[:, :cols], S[:, :c]))
                return leave("converged", CONVERGED, out, it) if done else leave("maxiter", MAXITER, out, it)
            late = np.flatnonzero(res > tolerance * scale)
            l = int(late[0]) if late.size else c - 1
            if fault == "target 0":
                l = 0
            X = None
            if cols == m:
                X = combine_ref(V, S[:, :c])                     # (the first c columns of the rotated basis)
                V[:, :kk] = combine_ref(V, S[:, :kk])
                W[:, :kk] = combine_ref(W, S[:, :kk])
                if fault == "full H":                            # the rotated H kept whole: S^T H S with its rounding noise
                    H[:kk, :kk] = S[:, :kk].T @ H @ S[:, :kk]
                    H[kk:, :] = H[:, kk:] = 0.0
                else:
                    H[:] = 0.0
                    H[np.arange(kk), np.arange(kk)] = theta[:kk]
                cols = kk
                info["restarts"] += 1
            info["targets"].append(l)
            info["expansions"] += 1
            info["products"] += 1                                # (enqueued with the expansion, whatever beta turns out to be)
            t = R[:, l].copy()
            if precond is not None:
                t = np.asarray(precond(t), dtype=np.float64).copy()
                info["applies"] += 1
            for _ in range(1 if fault == "one pass" else 2):
                h = [dot_ref(V[:, i], t) for i in range(cols)]
                for i in range(cols):
                    t = t - h[i] * V[:, i]
            beta = np.sqrt(dot_ref(t, t))
            if not np.isfinite(beta):
                info["checks"] += 1
                return leave("beta_nonfinite", NONFINITE, none, it)
            if beta == 0:
                info["checks"] += 1
                out = (theta[:c].copy(), res.copy(), combine_ref(V[:, :j + 1], S[:, :c]) if X is None else X)
                return leave("breakdown", BREAKDOWN, out, it)
            info["products"] -= 1                                # (the next step counts it)
            V[:, cols] = t / beta
