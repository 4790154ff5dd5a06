"""The test side's reference of the multicolour Gauss-Seidel smoother of include/spmvHip.h (spmvHipAmgSetGaussSeidel): every
Gauss-Seidel level's colouring from colour_ref (colourings), the sweep GS(l, r, z, q, fromNothing, backward_k) in numpy
float64 one colour at a time (gs), and the cycle with it in both smoothing places (cycle_ref) over the levels of
amg_ref.setup_ref (the gather), amg_sa_ref.setup_ref or filter_ref.strength_setup_ref (P e).  GsCsr is the cycle as the
preconditioner of the Krylov reference loops.  Four faults can be planted: the row update as one fused multiply-add, a
symmetric cycle whose post-sweep runs forward, colours taken from the strength-filtered F_l, and a Jacobi within the sweep
(the row sums from the z of the sweep's start).  numpy rounds every product and add on its own, as IEEE double does with no
FMA."""
from fractions import Fraction

import numpy as np

import colour_ref as cl
from amg_cheb_ref import setup_ref                              # noqa: F401  (the three setups by name)
from krylov_ref import Csr

JACOBI, CHEBYSHEV, GAUSS_SEIDEL = 0, 1, 2
NATURAL, HASH = cl.NATURAL, cl.HASH
MAX_DEGREE = 64
SMALL_ROWS = 1024                                              # the one-workgroup sweep's default threshold
LONG_ROW = 64                                                  # rows above it take a wavefront
F = np.float64


def smoother(o, omega=1.0, order=NATURAL, seed=0, oneWay=False, levels=None, nu1=None, nu2=None, nuCoarse=None, **faults):
    """what spmvHipAmgSetGaussSeidel leaves in force on a hierarchy set up with the options o: a count None keeps o's,
    levels None is all.  faults: fma, post_forward, colours_from_F, jacobi_within (False)"""
    keep = lambda v, k: o[k] if v is None else v
    out = dict(kind=GAUSS_SEIDEL, omega=omega, order=order, seed=seed, oneWay=bool(oneWay), levels=levels, nu1=keep(nu1, "nu1"),
               nu2=keep(nu2, "nu2"), nuCoarse=keep(nuCoarse, "nuCoarse"), fma=False, post_forward=False, colours_from_F=False,
               jacobi_within=False)
    out.update(faults)
    return out


def gs_levels(levels, sm):
    """how many levels, from 0, smooth with Gauss-Seidel"""
    return len(levels) if not sm["levels"] else min(sm["levels"], len(levels))


def level_colouring(lv, sm):
    """dict(colour, perm, ptr, classes) of one level: the colours of A_l (the planted fault: of F_l where the level has
    one), the rows by (colour, id), the C + 1 class offsets, and per class (rows, the rows of A_l as a Csr)"""
    A = lv["A"]
    P = lv["F"] if sm["colours_from_F"] and "F" in lv else A
    M = A[0]
    colour, _ = cl.colour_ref(M, P[2], P[3], sm["order"], sm["seed"])
    perm = cl.perm_of(colour)
    C = int(colour.max()) + 1 if M else 0
    ptr = np.searchsorted(colour[perm.astype(np.int64)], np.arange(C + 1)).astype(np.uint32)
    irp, ja, vals = np.asarray(A[2], dtype=np.int64), np.asarray(A[3], dtype=np.int64), np.asarray(A[4], dtype=np.float64)
    classes = []
    for c in range(C):
        rows = perm[ptr[c]:ptr[c + 1]].astype(np.int64)
        lens = irp[rows + 1] - irp[rows]
        sub = np.zeros(rows.size + 1, dtype=np.int64)
        sub[1:] = np.cumsum(lens)
        pos = np.repeat(irp[rows] - sub[:-1], lens) + np.arange(int(sub[-1]))
        classes.append((rows, Csr(rows.size, sub, ja[pos], vals[pos])))
    return dict(colour=colour, perm=perm, ptr=ptr, classes=classes)


def colourings(levels, sm):
    """per level the colouring of a Gauss-Seidel level, None of a Jacobi level"""
    n = gs_levels(levels, sm)
    return [level_colouring(lv, sm) if l < n else None for l, lv in enumerate(levels)]


def _fma(a, x, z):
    """a * x + z with one rounding, elementwise, in exact rational arithmetic (finite values)"""
    return np.array([float(Fraction(float(a)) * Fraction(float(u)) + Fraction(float(v))) for u, v in zip(x, z)])


def gs(col, dinv, r, z, q, from_nothing, backward, omega, fma=False, jacobi_within=False):
    """GS(l, r, z, q, fromNothing, backward_k) of the header; backward(k) says which way sweep k runs"""
    omega = F(omega)
    z = np.zeros(r.size) if from_nothing else z.copy()
    with np.errstate(all="ignore"):
        for k in range(q):
            src = z.copy() if jacobi_within else z
            for rows, sub in (col["classes"][::-1] if backward(k) else col["classes"]):
                x = dinv[rows] * (r[rows] - sub.spmv(src))
                z[rows] = _fma(omega, x, z[rows]) if fma else z[rows] + omega * x
    return z


def cycle_ref(levels, o, r, sm, l=0, cols=None):
    """V(l, r) of the header with the Gauss-Seidel smoother sm (smoother()) on the levels below sm's `levels` and the Jacobi
    lines with o's omega from there on.  The correction is P e on a level that holds a smoothed prolongator, else the gather."""
    if cols is None:
        cols = colourings(levels, sm)
    lv = levels[l]
    last = l + 1 == len(levels)
    A, dinv, omega = lv["csr"], lv["dinv"], F(o["omega"])
    sweeps = sm["nuCoarse"] if last else sm["nu1"]
    col = cols[l]
    kw = dict(omega=sm["omega"], fma=sm["fma"], jacobi_within=sm["jacobi_within"])
    with np.errstate(all="ignore"):
        if col is not None:
            z = gs(col, dinv, r, None, sweeps, True, (lambda k: not sm["oneWay"] and k % 2 == 1) if last else (lambda k: False), **kw)
        elif sweeps == 0:
            z = np.zeros(A.M)
        else:
            z = omega * (dinv * r)
            for _ in range(sweeps - 1):
                z = z + omega * (dinv * (r - A.spmv(z)))
        if last:
            return z
        e = cycle_ref(levels, o, lv["Rcsr"].spmv(r - A.spmv(z)), sm, l + 1, cols)
        z = z + (lv["Pcsr"].spmv(e) if "Pcsr" in lv else e[lv["agg"].astype(np.int64)])
        if col is not None:
            back = not sm["oneWay"] and not sm["post_forward"]
            z = gs(col, dinv, r, z, sm["nu2"], False, lambda k: back, **kw)
        else:
            for _ in range(sm["nu2"]):
                z = z + omega * (dinv * (r - A.spmv(z)))
        return z


def sweep_launches(col, M, small_rows=SMALL_ROWS):
    """K_l of the header: the kernels of one sweep of a Gauss-Seidel level"""
    if M == 0:
        return 0
    return 1 if small_rows and M <= small_rows else len(col["classes"])


def cycle_launches(levels, sm, cols, unfused=0, small_rows=SMALL_ROWS):
    """the kernels one cycle enqueues (include/spmvHip.h): per Gauss-Seidel level above the last the zero pass, nu1 sweeps, the
    residual's SpMV and pass, the restriction, the correction (one more when it is `unfused`: an SpMV and an add) and nu2
    sweeps; on the last the zero pass and nuCoarse sweeps; a Jacobi level keeps its term"""
    start = lambda n: 1 + 2 * (max(n, 1) - 1)
    total = 0
    for l, lv in enumerate(levels):
        last = l + 1 == len(levels)
        if cols[l] is None:
            total += start(sm["nuCoarse"]) if last else start(sm["nu1"]) + 3 + 1 + 2 * sm["nu2"] + unfused
            continue
        K = sweep_launches(cols[l], lv["A"][0], small_rows)
        total += 1 + sm["nuCoarse"] * K if last else 1 + sm["nu1"] * K + 3 + 1 + unfused + sm["nu2"] * K
    return total


class GsCsr(Csr):
    """krylov_ref.Csr whose M^-1 v is the cycle with the given smoother (keywords of smoother(); kind JACOBI: the Jacobi
    cycle with sm's counts, for the comparison at the same sweeps)"""

    def __init__(self, A, hierarchy="plain", levels=None, o=None, sm=None, **kw):
        super().__init__(A[0], A[2], A[3], A[4])
        self.levels, self.o = (levels, o) if levels is not None else setup_ref(A, hierarchy, **kw)
        sm = dict(sm or {})
        self.jacobi = sm.pop("kind", GAUSS_SEIDEL) == JACOBI
        self.sm = smoother(self.o, **sm)
        if self.jacobi:
            self.sm["levels"], self.cols = None, [None] * len(self.levels)
        else:
            self.cols = colourings(self.levels, self.sm)
        self.F = self.levels                                   # (not None: the loops then call precond)

    def precond(self, v):
        return cycle_ref(self.levels, self.o, np.asarray(v, dtype=np.float64), self.sm, cols=self.cols)
