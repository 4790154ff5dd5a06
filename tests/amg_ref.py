"""The test side's reference of the aggregation multigrid of include/spmvHip.h: the aggregation loop (aggregate_ref), the
hierarchy (setup_ref: stable transpose and serial-loop products from transpose_ref / spgemm_ref), the V-cycle (cycle_ref,
on krylov_ref.Csr's serial-order SpMV) and the cycle as the preconditioner of the CG / BiCGStab / GMRES reference loops
(AmgCsr).  numpy rounds every product and add on its own, as IEEE double does with no FMA."""
import numpy as np

import spgemm_ref as sr
from colour_ref import fmix32
from krylov_ref import Csr

DEFAULTS = dict(seed=0, coarseRows=512, maxLevels=16, omega=2.0 / 3.0, nu1=1, nu2=1, nuCoarse=8)


def adjacency(M, IRP, JA):
    """adj(i) of the header: the pattern of A + A^T, no diagonal, repeats once, column ids >= M skipped"""
    adj = [set() for _ in range(M)]
    for i in range(M):
        for p in range(int(IRP[i]), int(IRP[i + 1])):
            j = int(JA[p])
            if j != i and j < M:
                adj[i].add(j)
                adj[j].add(i)
    return adj


def within2(adj, i):
    out = set(adj[i])
    for k in adj[i]:
        out |= adj[k]
    out.discard(i)
    return out


def aggregate_ref(M, IRP, JA, seed=0, detail=False):
    """the loop of the header.  Returns agg (uint32); with detail also (roots, ring) -- ring[i] in {0, 1, 2}"""
    adj = adjacency(M, IRP, JA)
    pri = [(fmix32(i ^ seed), i) for i in range(M)]
    root = [False] * M
    for i in sorted(range(M), key=lambda v: pri[v], reverse=True):
        root[i] = not any(root[j] for j in within2(adj, i))
    roots = [i for i in range(M) if root[i]]
    number = {r: n for n, r in enumerate(roots)}
    agg, ring = [None] * M, [None] * M
    for r in roots:
        agg[r], ring[r] = number[r], 0
    for i in range(M):
        if not root[i]:
            near = [k for k in adj[i] if root[k]]
            if near:
                assert len(near) == 1
                agg[i], ring[i] = number[near[0]], 1
    for i in range(M):
        if agg[i] is None:
            k = max((k for k in adj[i] if ring[k] == 1), key=lambda v: pri[v])
            agg[i] = agg[k]
    for i in range(M):
        if ring[i] is None:
            ring[i] = 2
    out = np.array(agg, dtype=np.uint32).reshape(M)
    return (out, roots, ring) if detail else out


def _opts(kw):
    o = dict(DEFAULTS)
    o.update({k: v for k, v in kw.items() if v is not None})
    return o


def dinv_of(A):
    M, _, IRP, JA, AS = A
    rows = np.repeat(np.arange(M), np.diff(IRP.astype(np.int64)))
    d = np.flatnonzero(JA.astype(np.int64) == rows)
    assert np.array_equal(rows[d], np.arange(M)), "every row holds exactly one stored diagonal entry"
    with np.errstate(all="ignore"):
        return 1.0 / AS[d]


def prolongator(M, agg, nAgg):
    return M, nAgg, np.arange(M + 1, dtype=np.uint64), agg.astype(np.uint64), np.ones(M)


def setup_ref(A, **kw):
    """A = (M, M, IRP, JA, AS).  Returns the list of levels: dicts with A, dinv and, but for the last, agg, P, R, AP"""
    o = _opts(kw)
    levels = []
    while True:
        M = A[0]
        lv = dict(A=A, dinv=dinv_of(A), csr=Csr(M, A[2], A[3], A[4]))
        levels.append(lv)
        if M <= o["coarseRows"] or len(levels) == o["maxLevels"]:
            break
        agg = aggregate_ref(M, A[2], A[3], o["seed"])
        nAgg = int(agg.max()) + 1
        if nAgg == M:
            break
        P = prolongator(M, agg, nAgg)
        R = sr.transpose(P)
        AP = sr.spgemm_ref(A, P)
        lv.update(agg=agg, P=P, R=R, AP=AP, Rcsr=Csr(R[0], R[2], R[3], R[4]))
        A = sr.spgemm_ref(R, AP)
    return levels, o


def cycle_ref(levels, o, r, l=0):
    """V(l, r) of the header"""
    lv = levels[l]
    last = l + 1 == len(levels)
    A, dinv, omega = lv["csr"], lv["dinv"], np.float64(o["omega"])
    with np.errstate(all="ignore"):
        sweeps = o["nuCoarse"] if last else o["nu1"]
        if sweeps == 0:
            z = np.zeros(A.M)
        else:
            z = omega * (dinv * r)
            for _ in range(sweeps - 1):
                t = A.spmv(z)
                z = z + omega * (dinv * (r - t))
        if last:
            return z
        d = r - A.spmv(z)
        e = cycle_ref(levels, o, lv["Rcsr"].spmv(d), l + 1)
        z = z + e[lv["agg"].astype(np.int64)]
        for _ in range(o["nu2"]):
            t = A.spmv(z)
            z = z + omega * (dinv * (r - t))
        return z


class AmgCsr(Csr):
    """krylov_ref.Csr whose M^-1 v is the cycle: what cg_ref / bicgstab_ref / gmres_ref take as A"""

    def __init__(self, A, **kw):
        super().__init__(A[0], A[2], A[3], A[4])
        self.levels, self.o = setup_ref(A, **kw)
        self.F = self.levels                                   # (not None: the loops then call precond)

    def precond(self, v):
        return cycle_ref(self.levels, self.o, np.asarray(v, dtype=np.float64))


# ------------------------------------------------------------------------------------------------------------- inputs
def pattern(M, rows, cols):
    """(M, IRP, JA) of the (row, col) list, in the given order inside each row"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    o = np.argsort(rows, kind="stable")
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return M, IRP, cols[o].astype(np.uint64)


def path(M, diagonal=True):
    rows = np.r_[np.arange(M) if diagonal else [], np.arange(1, M), np.arange(0, M - 1)].astype(np.int64)
    cols = np.r_[np.arange(M) if diagonal else [], np.arange(0, M - 1), np.arange(1, M)].astype(np.int64)
    o = np.lexsort((cols, rows))
    return pattern(M, rows[o], cols[o])


def star(leaves, upper_only=False):
    """vertex 0 is the hub; upper_only stores (0, leaf) alone: the other direction comes from A^T"""
    M = leaves + 1
    leaf = np.arange(1, M)
    rows, cols = np.r_[np.arange(M), np.zeros(leaves, dtype=np.int64)], np.r_[np.arange(M), leaf]
    if not upper_only:
        rows, cols = np.r_[rows, leaf], np.r_[cols, np.zeros(leaves, dtype=np.int64)]
    o = np.lexsort((cols, rows))
    return pattern(M, rows[o], cols[o])


def messy(M=40, seed=5):
    """isolated vertices (with and without a diagonal entry), repeated entries, unsorted rows, one-directional edges"""
    rng = np.random.default_rng(seed)
    live = np.arange(M)[np.arange(M) % 7 != 3]
    rows = np.repeat(live, 2)
    cols = rng.choice(live, rows.size)
    rows, cols = np.r_[rows, rows[:20], np.arange(0, M, 2)], np.r_[cols, cols[:20], np.arange(0, M, 2)]
    o = rng.permutation(rows.size)
    return pattern(M, rows[o], cols[o])


def small_graphs():
    """name -> (M, IRP, JA): every small graph of the two test files"""
    from colour_ref import laplacian7
    out = {f"M{M}": path(M) for M in (0, 1, 2, 3)}
    out["path70"] = path(70)
    out["laplacian12x10x8"] = laplacian7(12, 10, 8)[:3]
    out["star200"] = star(200)
    out["star200_upper"] = star(200, upper_only=True)
    out["messy"] = messy()
    return out


def middle_first_seed():
    """the smallest seed under which, on the 5-vertex path, a root retires the middle vertex 2 in the first round while an
    end vertex is still undecided: the case "distance 2 through a retired vertex" decides.  Root 1 (or 3) beats 0..3 (1..4)
    in round one and retires 0, 2, 3; vertex 4 then has only the retired 3 and 2 within distance 2 and becomes a root in
    round two -- an implementation that lets the retired 2, 3 still compete, or that stops walking at a retired vertex,
    gives other ids."""
    M, IRP, JA = path(5)
    for seed in range(1 << 16):
        pri = [(fmix32(i ^ seed), i) for i in range(5)]
        if pri[1] > max(pri[0], pri[2], pri[3]) and pri[3] > pri[4] and pri[2] > pri[4]:
            agg, roots, _ = aggregate_ref(M, IRP, JA, seed, detail=True)
            if roots == [1, 4]:
                return seed
    raise AssertionError("no seed found")


def laplacian(nx, ny, nz, values=None):
    """(M, M, IRP, JA, AS) of the 7-point Laplacian (spgemm_ref.laplacian7)"""
    return sr.laplacian7(nx, ny, nz) if values is None else sr.laplacian7(nx, ny, nz, values)
