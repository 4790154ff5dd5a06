"""The test side's reference for spmvHipDot, hipSpCGCSR and hipSpBiCGStabCSR (include/spmvHip.h): the fixed-order dot
product vectorised over blocks and lanes (`dot_ref`), the serial-order SpMV as a stored-order walk (`Csr.spmv`, the bits of
sgemvSerial), the ILU(0) preconditioner by the level-vectorised triangular solves of trsv_ref, and the two loops written
out as the header writes them (`cg_ref`, `bicgstab_ref`).  numpy rounds every product and every add on its own, as IEEE
double does with no FMA, so the bits are the library's."""
import numpy as np

from trsv_ref import levels, trsv_levels

KB, KT = 4096, 256                  # indices of a block, lanes of a block
CONVERGED, MAXITER, BREAKDOWN, NONFINITE = 0, 1, 2, 3


def tree(a):
    """the fixed tree over the last axis (256 lanes): a[t] += a[t + h], h = 128, ..., 1; returns a[..., 0]"""
    a = a.copy()
    h = a.shape[-1] // 2
    while h >= 1:
        a[..., :h] = a[..., :h] + a[..., h:2 * h]
        h //= 2
    return a[..., 0]


def dot_ref(u, v):
    """u . v in the order of spmvHipDot: per block of 4096, lane t adds the products of 512 s + 2 t, 512 s + 2 t + 1,
    s = 0..7, from +0.0; the tree over the lanes; the block partials by the same rule"""
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    n = u.size
    nb = -(-n // KB)
    if nb == 0:
        return np.float64(0.0)
    prod = np.zeros(nb * KB)
    with np.errstate(all="ignore"):
        prod[:n] = u * v
        lanes = prod.reshape(nb, KB // (2 * KT), KT, 2).transpose(0, 2, 1, 3).reshape(nb, KT, KB // KT)
        acc = np.zeros((nb, KT))
        for j in range(KB // KT):
            acc = acc + lanes[:, :, j]
        part = tree(acc)
        m = -(-nb // KT)
        pp = np.zeros(m * KT)
        pp[:nb] = part
        pp = pp.reshape(m, KT)
        acc = np.zeros(KT)
        for i in range(m):
            acc = acc + pp[i]
        return np.float64(tree(acc))


class Csr:
    """a CSR matrix with its serial-order SpMV and, when given the ILU(0) factors F (same pattern), M^-1 v"""

    def __init__(self, M, IRP, JA, AS, F=None):
        self.M = M
        self.IRP = np.asarray(IRP, dtype=np.int64)
        self.JA = np.asarray(JA, dtype=np.int64)
        self.AS = np.asarray(AS, dtype=np.float64)
        lens = np.diff(self.IRP)
        self.steps = [np.flatnonzero(lens > k) for k in range(int(lens.max()) if M else 0)]
        self.F = None if F is None else np.asarray(F, dtype=np.float64)
        if F is not None:
            self.lvl = (levels(M, self.IRP, self.JA, True), levels(M, self.IRP, self.JA, False))

    def spmv(self, x):
        """y[i] = +0.0, then += AS[p] * x[JA[p]] in stored order (sgemvSerial)"""
        y = np.zeros(self.M)
        with np.errstate(all="ignore"):
            for k, live in enumerate(self.steps):
                p = self.IRP[live] + k
                y[live] = y[live] + self.AS[p] * x[self.JA[p]]
        return y

    def precond(self, v):
        """U^-1 (L^-1 v) with the unit lower and the stored upper triangle of F; v itself without F"""
        if self.F is None:
            return v
        w = trsv_levels(self.M, self.IRP, self.JA, self.F, v, True, True, self.lvl[0])
        return trsv_levels(self.M, self.IRP, self.JA, self.F, w, False, False, self.lvl[1])


def _init(A, b, x, tol):
    q = A.spmv(x)
    r = b - q
    rr, bb = dot_ref(r, r), dot_ref(b, b)
    tol = np.float64(tol)
    thresh = (tol * tol) * bb
    return r, rr, bb, thresh


def _first_exit(rr, thresh, maxiter, trace):
    if rr <= thresh:
        return _exit(trace, "init_converged", CONVERGED)
    if not np.isfinite(rr):
        return _exit(trace, "init_nonfinite", NONFINITE)
    if maxiter == 0:
        return _exit(trace, "init_maxiter", MAXITER)
    return None


# one label per `return` of the two loops.  BiCGStab's `rho == 0` straight after the init needs rr == 0, which
# `rr <= thresh` catches first (thresh >= 0 or NaN; with a NaN thresh rr = 0 is impossible, bb being a term of it): that
# return is unreachable and has no label.
CG_EXITS = ("init_converged", "init_nonfinite", "init_maxiter", "pq0", "converged", "nonfinite", "maxiter")
BICGSTAB_EXITS = ("init_converged", "init_nonfinite", "init_maxiter", "rv0", "half_converged", "tt0", "converged",
                  "nonfinite", "omega0", "maxiter", "rho0")


def _exit(trace, label, status, half=None, **state):
    """the loop ends here: `trace` (a list, or None) learns which line it was; at BiCGStab's two half-step exits `half`
    (a dict, or None) also receives the x the iteration started from, alpha and phat"""
    if trace is not None:
        trace.append(label)
    if half is not None:
        half.update(state)
    return status


def cg_ref(A, b, x0, tol, maxiter, trace=None):
    """hipSpCGCSR's loop.  Returns (x, status, iterations, history, rr); appends the exit's label (CG_EXITS) to `trace`."""
    with np.errstate(all="ignore"):
        x = np.array(x0, dtype=np.float64, copy=True)
        b = np.asarray(b, dtype=np.float64)
        r, rr, bb, thresh = _init(A, b, x, tol)
        hist = [rr]
        st = _first_exit(rr, thresh, maxiter, trace)
        if st is not None:
            return x, st, 0, np.array(hist), rr
        z = A.precond(r)
        rz = dot_ref(r, z) if A.F is not None else rr
        p = z.copy()
        for k in range(1, maxiter + 1):
            q = A.spmv(p)
            pq = dot_ref(p, q)
            if pq == 0:
                return x, _exit(trace, "pq0", BREAKDOWN), k - 1, np.array(hist), rr
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            rr = dot_ref(r, r)
            hist.append(rr)
            if rr <= thresh:
                return x, _exit(trace, "converged", CONVERGED), k, np.array(hist), rr
            if not np.isfinite(rr):
                return x, _exit(trace, "nonfinite", NONFINITE), k, np.array(hist), rr
            if k == maxiter:
                return x, _exit(trace, "maxiter", MAXITER), k, np.array(hist), rr
            if A.F is not None:
                z = A.precond(r)
                rzn = dot_ref(r, z)
            else:
                z, rzn = r, rr
            beta = rzn / rz
            rz = rzn
            p = z + beta * p
    raise AssertionError("unreachable")


def bicgstab_ref(A, b, x0, tol, maxiter, trace=None, half=None):
    """hipSpBiCGStabCSR's loop (right-preconditioned).  Returns (x, status, iterations, history, rr); appends the exit's
    label (BICGSTAB_EXITS) to `trace`; `half` as in _exit."""
    with np.errstate(all="ignore"):
        x = np.array(x0, dtype=np.float64, copy=True)
        b = np.asarray(b, dtype=np.float64)
        r, rr, bb, thresh = _init(A, b, x, tol)
        hist = [rr]
        st = _first_exit(rr, thresh, maxiter, trace)
        if st is not None:
            return x, st, 0, np.array(hist), rr
        rhat = r.copy()
        rho = rr
        rho_old = alpha = omega = np.float64(1.0)
        if rho == 0:
            return x, BREAKDOWN, 0, np.array(hist), rr
        beta = p = v = None
        for k in range(1, maxiter + 1):
            p = r.copy() if k == 1 else r + beta * (p - omega * v)
            phat = A.precond(p)
            v = A.spmv(phat)
            rv = dot_ref(rhat, v)
            if rv == 0:
                return x, _exit(trace, "rv0", BREAKDOWN), k - 1, np.array(hist), rr
            alpha = rho / rv
            s = r - alpha * v
            rr = dot_ref(s, s)
            hist.append(rr)
            if rr <= thresh:
                st = _exit(trace, "half_converged", CONVERGED, half, x=x, alpha=alpha, phat=phat)
                return x + alpha * phat, st, k, np.array(hist), rr
            shat = A.precond(s)
            t = A.spmv(shat)
            tt, ts = dot_ref(t, t), dot_ref(t, s)
            if tt == 0:
                st = _exit(trace, "tt0", BREAKDOWN, half, x=x, alpha=alpha, phat=phat)
                return x + alpha * phat, st, k, np.array(hist), rr
            omega = ts / tt
            x = (x + alpha * phat) + omega * shat
            r = s - omega * t
            rr = dot_ref(r, r)
            hist[k] = rr
            rhon = dot_ref(rhat, r)
            if rr <= thresh:
                return x, _exit(trace, "converged", CONVERGED), k, np.array(hist), rr
            if not np.isfinite(rr):
                return x, _exit(trace, "nonfinite", NONFINITE), k, np.array(hist), rr
            if omega == 0:
                return x, _exit(trace, "omega0", BREAKDOWN), k, np.array(hist), rr
            if k == maxiter:
                return x, _exit(trace, "maxiter", MAXITER), k, np.array(hist), rr
            rho_old, rho = rho, rhon
            if rho == 0:
                return x, _exit(trace, "rho0", BREAKDOWN), k, np.array(hist), rr
            beta = (rho / rho_old) * (alpha / omega)
    raise AssertionError("unreachable")
