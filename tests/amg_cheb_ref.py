"""The test side's reference of the Chebyshev smoother of include/spmvHip.h (spmvHipAmgSetSmoother): the coefficient
recurrence in numpy float64 in the header's order (coefficients), every level's rho from A_l and dinv_l and its table
(tables), and the cycle with the smoother in both smoothing places (cycle_ref) over the levels of amg_ref.setup_ref (the
gather), amg_sa_ref.setup_ref or filter_ref.strength_setup_ref (P e).  ChebCsr is the cycle as the preconditioner of the
Krylov reference loops.  Three faults can be planted: the step's a d + b x as one fused multiply-add, a post-smoother that
continues the pre-smoother's recurrence, and rho taken from the strength-filtered F_l.  numpy rounds every product and add
on its own, as IEEE double does with no FMA."""
from fractions import Fraction

import numpy as np

import amg_ref as ar
import amg_sa_ref as sa
from krylov_ref import Csr

JACOBI, CHEBYSHEV = 0, 1
MAX_DEGREE = 64
F = np.float64


def coefficients(rho, eigRatio, lambdaScale, q):
    """(lmax, lmin, ab): the interval and the (q, 2) array of the pairs (a_k, b_k), a_0 = 0.0, in the header's order"""
    with np.errstate(all="ignore"):
        lmax = F(lambdaScale) * F(rho)
        lmin = lmax / F(eigRatio)
        ab = np.zeros((q, 2))
        if q == 0:
            return lmax, lmin, ab
        theta = (lmax + lmin) / F(2.0)
        delta = (lmax - lmin) / F(2.0)
        sigma = theta / delta
        s = F(1.0) / sigma
        ab[0] = (0.0, F(1.0) / theta)
        for k in range(1, q):
            sk = F(1.0) / (F(2.0) * sigma - s)
            ab[k] = (sk * s, (F(2.0) * sk) / delta)
            s = sk
    return lmax, lmin, ab


def smoother(o, kind=CHEBYSHEV, nu1=None, nu2=None, nuCoarse=None, eigRatio=10.0, lambdaScale=1.0, **faults):
    """what spmvHipAmgSetSmoother leaves in force on a hierarchy set up with the options o: a count None keeps o's.
    faults: fma, carry_on, rho_from_F (False)"""
    keep = lambda v, k: o[k] if v is None else v
    out = dict(kind=kind, nu1=keep(nu1, "nu1"), nu2=keep(nu2, "nu2"), nuCoarse=keep(nuCoarse, "nuCoarse"), eigRatio=eigRatio,
               lambdaScale=lambdaScale, fma=False, carry_on=False, rho_from_F=False)
    out.update(faults)
    return out


def pairs(levels, sm, l):
    """the length of level l's table"""
    return sm["nuCoarse"] if l + 1 == len(levels) else max(sm["nu1"], sm["nu2"])


def level_rho(lv, from_F=False):
    """rho of a level from A_l's stored rows and dinv_l (the planted fault: F_l's rows and dF_l where the level has them)"""
    if from_F and "F" in lv:
        return sa.rho_of(lv["F"], lv["dF"])[0]
    return sa.rho_of(lv["A"], lv["dinv"])[0] if lv["A"][0] else F(0.0)


def tables(levels, sm, extra=0):
    """per level dict(rho, lmax, lmin, ab) of a Chebyshev smoother (extra: more pairs than the table holds, for carry_on)"""
    out = []
    for l, lv in enumerate(levels):
        rho = level_rho(lv, sm["rho_from_F"])
        if lv["A"][0] == 0:
            out.append(dict(rho=F(0.0), lmax=F(0.0), lmin=F(0.0), ab=np.zeros((pairs(levels, sm, l), 2))))
            continue
        assert 0.0 < rho < np.inf, "the call refuses this level"
        lmax, lmin, ab = coefficients(rho, sm["eigRatio"], sm["lambdaScale"], pairs(levels, sm, l) + extra)
        out.append(dict(rho=rho, lmax=lmax, lmin=lmin, ab=ab))
    return out


def _fma(a, d, p):
    """a * d + p with one rounding, elementwise, in exact rational arithmetic (finite values)"""
    return np.array([float(Fraction(float(a)) * Fraction(float(x)) + Fraction(float(y))) for x, y in zip(d, p)])


def cheb(A, dinv, r, z, ab, ks, from_nothing, d=None, fma=False):
    """the steps k in ks of Cheb(l, r, z, q, fromNothing) of the header; returns (z, d)"""
    with np.errstate(all="ignore"):
        for k in ks:
            a, b = F(ab[k, 0]), F(ab[k, 1])
            if k == 0 and from_nothing:
                d = b * (dinv * r)
                z = d.copy()
                continue
            x = dinv * (r - A.spmv(z))
            if k == 0:
                d = b * x
            elif fma:
                d = _fma(a, d, b * x)
            else:
                d = a * d + b * x
            z = z + d
    return z, d


def cycle_ref(levels, o, r, sm, l=0, tabs=None):
    """V(l, r) of the header with the smoother sm (smoother()): Jacobi with sm's counts, or Chebyshev.  The correction is
    P e on a level that holds a smoothed prolongator, else the gather."""
    lv = levels[l]
    last = l + 1 == len(levels)
    A, dinv, omega = lv["csr"], lv["dinv"], F(o["omega"])
    sweeps = sm["nuCoarse"] if last else sm["nu1"]
    chebyshev = sm["kind"] == CHEBYSHEV
    if chebyshev and tabs is None:
        tabs = tables(levels, sm, extra=sm["nu2"] if sm["carry_on"] else 0)
    ab = tabs[l]["ab"] if chebyshev else None
    with np.errstate(all="ignore"):
        d = None
        if sweeps == 0:
            z = np.zeros(A.M)
        elif chebyshev:
            z, d = cheb(A, dinv, r, None, ab, range(sweeps), True, fma=sm["fma"])
        else:
            z = omega * (dinv * r)
            for _ in range(sweeps - 1):
                z = z + omega * (dinv * (r - A.spmv(z)))
        if last:
            return z
        e = cycle_ref(levels, o, lv["Rcsr"].spmv(r - A.spmv(z)), sm, l + 1, tabs)
        z = z + (lv["Pcsr"].spmv(e) if "Pcsr" in lv else e[lv["agg"].astype(np.int64)])
        if chebyshev and sm["carry_on"] and d is not None:
            z, _ = cheb(A, dinv, r, z, ab, range(sweeps, sweeps + sm["nu2"]), False, d=d, fma=sm["fma"])
        elif chebyshev:
            z, _ = cheb(A, dinv, r, z, ab, range(sm["nu2"]), False, fma=sm["fma"])
        else:
            for _ in range(sm["nu2"]):
                z = z + omega * (dinv * (r - A.spmv(z)))
        return z


def setup_ref(A, hierarchy="plain", **kw):
    """(levels, o) of one of the three setups: "plain", "smoothed" or "strength" (theta / thetaScale / omegaP in kw)"""
    if hierarchy == "plain":
        return ar.setup_ref(A, **kw)
    omegaP = kw.pop("omegaP", 0.0) or 0.0
    if hierarchy == "smoothed":
        return sa.setup_ref(A, omegaP, **kw)
    import filter_ref as fr
    return fr.strength_setup_ref(A, kw.pop("theta", None), kw.pop("thetaScale", None), omegaP, **kw)


class ChebCsr(Csr):
    """krylov_ref.Csr whose M^-1 v is the cycle with the given smoother (keywords of smoother())"""

    def __init__(self, A, hierarchy="plain", levels=None, o=None, sm=None, **kw):
        super().__init__(A[0], A[2], A[3], A[4])
        self.levels, self.o = (levels, o) if levels is not None else setup_ref(A, hierarchy, **kw)
        self.sm = smoother(self.o, **(sm or {}))
        self.tabs = tables(self.levels, self.sm) if self.sm["kind"] == CHEBYSHEV else None
        self.F = self.levels                                   # (not None: the loops then call precond)

    def precond(self, v):
        return cycle_ref(self.levels, self.o, np.asarray(v, dtype=np.float64), self.sm, tabs=self.tabs)
