"""The host model of a pool of derived device handles and the seeded generator of operation sequences on it
(tests/test_derived_model.py runs it dry, tests/test_gpu_derived_sequences.py against the device).

The pool is a small graph: three sources -- A, the SPD five-point matrix of a 23 x 19 grid (437 rows: no multiple of 4 or
64); N, nonsymmetric of the same size with a full diagonal and three rows past 64 entries, adopted with 8-byte row pointers;
R, 150 x 437 with empty rows and one row of a few hundred entries -- and the nodes derived from them and from each other:
transposes, permutations by a colouring, products, sums and filters.  A node's model holds its pattern and the values the
device handle must hold NOW, composed from the per-feature references (spgemm_ref, colour_ref, add_ref, filter_ref,
ilu0_ref) on its sources' model values at its build or last refresh: a node whose source changed since then is stale and
keeps its old values.  The model also carries what the value-update tail of the library keeps per handle: the unit flag
and value, the formats built and whether while unit, the two kernel selections, whether the node holds ILU(0) factors.
Multigrid hierarchies stand on the square nodes (Hier): their levels as amg_ref / amg_sa_ref / filter_ref build and refresh
them, the smoother in force as amg_cheb_ref / amg_gs_ref state it, the width of the block workspace.

Every draw comes from numpy.random.default_rng(seed) and from the model alone, never from a device result: a seed gives
the same trace with and without a GPU.  Generator.run() yields one record (a dict) per operation, AFTER the model has
taken it; a backend executes the record and compares the device with the model.  `stats` counts what happened, for the
coverage conditions of tests/test_derived_model.py."""
import collections
import functools

import numpy as np

import add_ref as ad
import amg_block_ref as abr
import amg_cheb_ref as acr
import amg_gs_ref as ags
import colour_ref as cr
import filter_ref as fr
import spgemm_ref as sr
from exact_ref import HI, LO
from gmres_ref import gmres_ref
from ilu0_ref import check_pattern, ilu0_levels
from krylov_ref import Csr, bicgstab_ref, cg_ref
from sequence_inputs import CONSTANTS, KINDS, unit_of, values

SEEDS = tuple(range(20))
STEPS = 50
MAX_LIVE = 10                          # live nodes, the three sources among them
MAX_NNZ = 30_000                       # of a product (a seed must run in seconds)
GRID = (23, 19)
DERIVED = ("transpose", "permute", "multiply", "add", "filter")
PRODUCTS = ("rows", "warp", "auto", "enq_auto", "enq_auto_rows", "enq_csr0", "enq_csr1", "tiles", "stripes", "sell")
# (operation, weight)
OPS = (("set_values", 12), ("update_derived", 5), ("derive", 12), ("refresh", 22), ("refresh_refused", 4), ("free", 2),
       ("reupload", 2), ("build", 13), ("product", 12), ("matmul", 4), ("solve", 5), ("ilu0", 5), ("krylov", 4), ("hierarchy", 18))
HIERARCHIES = ("plain", "smoothed", "strength")
THETA = 0.25                           # of the strength setup


def _csr(M, rows, cols):
    """sorted distinct columns per row"""
    key = np.unique(np.asarray(rows, dtype=np.int64) * (1 << 32) + np.asarray(cols, dtype=np.int64))
    rows, cols = key >> 32, key & 0xFFFFFFFF
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return IRP, cols.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def sources():
    """name -> (M, N, IRP, JA, AS): the three source matrices with their first values"""
    rng = np.random.default_rng(4300)
    nx, ny = GRID
    M = nx * ny
    ids = np.arange(M)
    x, y = ids % nx, ids // nx
    rows, cols = [ids], [ids]
    for ok, d in ((y > 0, -nx), (x > 0, -1), (x < nx - 1, 1), (y < ny - 1, nx)):
        rows.append(ids[ok])
        cols.append(ids[ok] + d)
    IRP, JA = _csr(M, np.concatenate(rows), np.concatenate(cols))
    A = (M, M, IRP, JA, np.where(sr.si.row_of_entry(IRP) == JA.astype(np.int64), 4.0, -1.0))
    lens = rng.integers(3, 9, M)
    lens[[5, 200, M - 1]] = [80, 120, 90]
    IRP, JA = _csr(M, np.concatenate([np.repeat(ids, lens), ids]), np.concatenate([rng.integers(0, M, lens.sum()), ids]))
    v = rng.uniform(-1.0, 1.0, JA.size)
    r = sr.si.row_of_entry(IRP)
    diag = r == JA.astype(np.int64)
    v[diag] = np.bincount(r, weights=np.abs(v) * ~diag, minlength=M) + 1.0
    N = (M, M, IRP, JA, v)
    assert np.sort(np.diff(IRP.astype(np.int64)))[-3] > 64
    Mr = 150
    lens = rng.integers(0, 7, Mr)
    lens[[0, 17, Mr - 1]] = 0
    lens[40] = 300
    IRP, JA = _csr(Mr, np.repeat(np.arange(Mr), lens), rng.integers(0, M, lens.sum()))
    R = (Mr, M, IRP, JA, rng.uniform(-1.0, 1.0, JA.size))
    assert np.diff(IRP.astype(np.int64)).max() > 200
    return {"A": A, "N": N, "R": R}


@functools.lru_cache(maxsize=None)
def xs(n):
    """the two x vectors of every node with n columns (as sequence_inputs makes them)"""
    rng = np.random.default_rng(4400 + n)
    x0 = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.0, n) * 2.0 ** rng.integers(-8, 9, n)
    x1 = np.sin(rng.uniform(0.1, 3.0, n)) * 3e-5 * rng.choice([-1.0, 1.0], n)
    return x0, x1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def in_exact_range(v):
    """exact_ref's sums are exact on these values (finite, nonzero magnitudes in [2^-200, 2^200])"""
    v = np.abs(v)
    nz = v[v != 0.0]
    return bool(np.isfinite(v).all() and (nz.size == 0 or (nz.min() >= LO and nz.max() <= HI)))


# ------------------------------------------------------------------------------------ what a derived node is made of
def build_node(kind, params, S):
    """(matrix, aux) of `kind` made from the source matrices S (tuples (M, N, IRP, JA, AS)); aux is what a refresh needs"""
    if kind == "transpose":
        T = sr.transpose(S[0])
        return T, np.argsort(S[0][3].astype(np.int64), kind="stable")
    if kind == "permute":
        M, _, IRP, JA, AS = S[0]
        perm = permutation(S[0], params)
        irp, ja, val, o = cr.permute_ref(M, IRP, JA, AS, perm)
        return (M, M, irp.astype(np.uint64), ja.astype(np.uint64), val), o.astype(np.int64)
    if kind == "multiply":
        return sr.spgemm_ref(S[0], S[1]), None
    if kind == "add":
        return ad.add_ref(params["alpha"], S[0], params["beta"], S[1]), None
    if kind == "filter":
        C, kept = fr.filter_ref(S[0], params)
        return C, kept
    if kind == "fsai":                                   # (tests/state_model.py: the factor G of S[0] on the pattern S[1], or its own)
        import fsai_ref
        G, info = fsai_ref.fsai_loop(S[0], S[1] if len(S) > 1 else None)
        return G, (S[1][:4] + (None,) if len(S) > 1 else None)
    raise KeyError(kind)


def refresh_values(kind, params, aux, S):
    """the values a refresh of the node gives from the sources' values now"""
    if kind in ("transpose", "permute"):
        return S[0][4][aux].copy()
    if kind == "multiply":
        return sr.spgemm_ref(S[0], S[1])[4]
    if kind == "add":
        return ad.add_ref(params["alpha"], S[0], params["beta"], S[1])[4]
    if kind == "filter":
        return fr.filter_refresh_ref(aux, S[0], params)[4]
    if kind == "fsai":
        import fsai_ref
        return fsai_ref.fsai_loop(S[0], aux)[0][4]
    raise KeyError(kind)


def permutation(A, params):
    """perm[new] = old of X.colour(order, seed), or of X.rcm(start, max_passes, forward) for the order "rcm" (a hook of
    tests/state_model.py: this module's own generator never draws it)"""
    if params["order"] == "rcm":
        import rcm_ref
        start = {"peripheral": rcm_ref.PERIPHERAL, "min_degree": rcm_ref.MIN_DEGREE}[params["start"]]
        return np.asarray(rcm_ref.rcm_loop(A[0], A[2], A[3], start, params["max_passes"], params["forward"])[0], dtype=np.int64)
    colour, _ = cr.colour_ref(A[0], A[2], A[3], {"natural": cr.NATURAL, "hash": cr.HASH}[params["order"]], params["seed"])
    return cr.perm_of(colour)


class Node:
    """one handle of the pool: what the model knows about it"""

    def __init__(self, nid, uid, kind, srcs, params, mat, aux, label, depth):
        self.id, self.uid, self.kind, self.srcs, self.params, self.aux, self.label, self.depth = nid, uid, kind, srcs, params, aux, label, depth
        self.M, self.N, self.IRP, self.JA, self.vals = mat
        self.alive, self.version, self.factored = True, 0, False
        self.seen = ()                  # the (uid, version) of every source at the build or the last refresh
        self.unit = unit_of(self.vals)
        self.tiles = None               # the two-phase form in use: None, or deterministic (bool)
        self.stripes, self.stripes_det = {}, 0      # layout ("shared" / "owner") -> built while unit; what the launcher runs
        self.sell = False
        self.dirty = set()              # the formats built whose values changed since the last product through them
        self.selected = [False, False]  # the reduction-order / serial-order selection has run (None: it may have)
        self.last_update = None
        r = sr.si.row_of_entry(self.IRP)
        j = self.JA.astype(np.int64)
        self.square = self.M == self.N
        diag = np.bincount(r[r == j], minlength=self.M) if self.M else np.zeros(0, dtype=np.int64)
        self.one_diagonal = bool(self.square and (diag == 1).all())
        self.ilu_ok = bool(self.one_diagonal and check_pattern(self.M, self.IRP, self.JA)[1] < 0)
        self.dpos = check_pattern(self.M, self.IRP, self.JA)[0] if self.ilu_ok else None

    @property
    def mat(self):
        return self.M, self.N, self.IRP, self.JA, self.vals

    @property
    def derived(self):
        return self.kind != "source"


class Hier:
    """one multigrid hierarchy: its levels as the reference holds them, the smoother in force, the block width"""

    def __init__(self, hid, src, kind, kw, levels, o):
        self.id, self.label, self.src, self.uid, self.version = hid, f"H{hid}", src.id, src.uid, src.version
        self.kind, self.kw, self.levels, self.o = kind, kw, levels, o
        self.sm, self.set_call = acr.smoother(o, kind=acr.JACOBI), None      # set_call: the last set_* call, for a twin
        self.width, self.alive, self.refreshed = 0, True, False
        self.storage, self.a0form = "f64", False             # (tests/state_model.py switches the storage; here it stays f64)

    def active(self):
        """the levels a cycle streams: in F32 storage their roundings (values_f32_ref.rounded_levels)"""
        if self.storage == "f64":
            return self.levels
        import values_f32_ref
        return values_f32_ref.rounded_levels(self.levels)

    def cycle(self, r):
        ref = ags if self.sm["kind"] == ags.GAUSS_SEIDEL else acr
        return ref.cycle_ref(self.active(), self.o, np.asarray(r, dtype=np.float64), self.sm)


class Generator:
    HIER_ACTIONS = ("set_smoother", "set_gauss_seidel", "set_block_width", "refresh", "apply", "apply_block", "apply_block", "set_block_width",
                    "set_smoother", "apply", "free")
    OPS = OPS                           # hooks of a subclass (tests/state_model.py): its own table of operations ...
    sources = staticmethod(sources)     # ... and its own source matrices

    def __init__(self, seed, steps=STEPS):
        self.hiers = []
        self.seed, self.steps = seed, steps
        self.rng = np.random.default_rng(seed)
        self.nodes, self.trace, self.stats = {}, [], collections.Counter()
        self.skips = collections.Counter()
        self._id = self._uid = 0

    def where(self):
        return f"seed {self.seed}, step {len(self.trace)}; trace:\n  " + "\n  ".join(self.trace)

    # ------------------------------------------------------------------------------------------------------ the pool
    def live(self, derived=None, **need):
        out = [n for n in self.nodes.values() if n.alive and (derived is None or n.derived == derived)]
        return [n for n in out if all(getattr(n, k) == v for k, v in need.items())]

    def pick(self, nodes, prefer_derived=0.0):
        """one of the nodes, or None: a derived one with that probability when there is one"""
        if not nodes:
            return None
        d = [n for n in nodes if n.derived]
        if d and len(d) < len(nodes) and self.rng.random() < prefer_derived:
            nodes = d
        return nodes[int(self.rng.integers(len(nodes)))]

    def _uid_next(self):
        self._uid += 1
        return self._uid

    def _add(self, kind, srcs, params, mat, aux, label):
        depth = 1 + max([self.nodes[s].depth for s in srcs], default=-1)
        n = Node(self._id, self._uid_next(), kind, tuple(srcs), params, mat, aux, label, depth)
        n.seen = tuple((self.nodes[s].uid, self.nodes[s].version) for s in srcs)
        self.nodes[n.id] = n
        self._id += 1
        return n

    def stale(self, n):
        """the node's own sources changed since its build or last refresh"""
        return n.derived and n.seen != tuple((self.nodes[s].uid, self.nodes[s].version) for s in n.srcs)

    def refreshable(self, n):
        return n.derived and all(self.nodes[s].alive and self.nodes[s].uid == u for s, (u, _) in zip(n.srcs, n.seen))

    def fresh_values(self, n):
        """what the node would hold had every node above it been refreshed in order (dead sources keep their last values)"""
        if not n.derived:
            return n.vals
        S = [self.nodes[s].mat[:4] + (self.fresh_values(self.nodes[s]),) for s in n.srcs]
        with np.errstate(all="ignore"):
            return refresh_values(n.kind, n.params, n.aux, S)

    # ------------------------------------------------------------------------------- the tail of every value update
    def _set(self, n, vals, factored=False):
        before = n.unit
        n.vals = np.ascontiguousarray(vals, dtype=np.float64)
        n.version += 1
        n.factored = factored
        n.unit = unit_of(n.vals)
        same = before[0] and n.unit[0] and np.float64(before[1]).tobytes() == np.float64(n.unit[1]).tobytes()
        if n.derived and n.stripes:
            if not before[0] and n.unit[0]:
                self.stats["stripes: non-unit -> unit"] += 1
            elif before[0] and n.unit[0] and not same:
                self.stats["stripes: unit -> unit of another value"] += 1
            elif before[0] and not n.unit[0]:
                self.stats["stripes: unit -> non-unit"] += 1
        n.dirty |= {f for f, held in (("tiles", n.tiles is not None), ("stripes", bool(n.stripes)), ("sell", n.sell)) if held}
        rebuilt = not n.unit[0] and any(n.stripes.values())
        if rebuilt:
            n.stripes = {k: False for k in n.stripes}
        if before[0] and not n.unit[0]:
            n.selected = [False, False]
        n.last_update = dict(unitBefore=int(before[0]), unitAfter=int(n.unit[0]), rebuilt=int(rebuilt),
                             inPlace=int(not rebuilt and (not before[0] or same)))

    def _log(self, op, text, **rec):
        self.trace.append(text)
        self.stats[op] += 1
        return dict(rec, op=op, text=text)

    # --------------------------------------------------------------------------------------------------- operations
    def run(self):
        for name, mat in self.sources().items():
            n = self._add("source", (), {"adopted": name == "N"}, mat, None, name)
            yield self._log("upload", f"upload {name}" + (" (adopted, 8-byte row pointers)" if name == "N" else ""), node=n.id)
        w = np.array([x for _, x in self.OPS], dtype=np.float64)
        for _ in range(self.steps):
            op = self.OPS[int(self.rng.choice(len(self.OPS), p=w / w.sum()))][0]
            rec = getattr(self, "op_" + op)()
            if rec is None:                              # nothing to do it on yet: the pool grows instead
                rec = self.op_derive()
            yield rec
        for H in self.hiers:
            n = self.nodes[H.src]
            if H.alive and n.alive and (n.uid, n.version) == (H.uid, H.version):
                yield self._cycle(H, n, f"final cycle of {H.label}", "apply", twin=False)
        for n in self.live():
            x = xs(n.N)[0]
            n.selected[1] = True
            yield self._log("final", f"final hipSpMVRowsCSR({n.label})", node=n.id, x=x)

    # ---- hierarchies
    def hier_ok(self, n):
        """the setups take it and the cycle stays specified: one sorted diagonal per row, finite values, no zero diagonal"""
        return n.alive and n.ilu_ok and bool(np.isfinite(n.vals).all() and (n.vals[n.dpos] != 0.0).all())

    def _levels(self, kind, kw, A, old=None):
        """the levels of a setup, or of a refresh of `old`; None where the reference says the library refuses a level"""
        try:
            with np.errstate(all="ignore"):
                if old is not None and kind == "strength":
                    return fr.strength_refresh_ref(old.levels, old.o, A), old.o
                extra = dict(theta=THETA) if kind == "strength" else {}
                return acr.setup_ref(A, kind, **kw, **extra)
        except AssertionError:
            return None

    def op_hierarchy(self):
        rng = self.rng
        live = [H for H in self.hiers if H.alive]
        if not live or (len(live) < 3 and rng.random() < 0.15):
            cand = [c for c in self.live() if self.hier_ok(c)]
            spd = [c for c in cand if self.is_spd(c)]
            if not cand:
                return None
            kind = HIERARCHIES[int(rng.integers(3))]
            kw = dict(seed=int(rng.integers(1 << 16)), coarseRows=int(rng.choice([8, 40, 120])))
            for _ in range(3):                           # mostly a matrix that gives more than one level
                n = self.pick(spd if spd and rng.random() < 0.8 else cand)
                made = self._levels(kind, kw, n.mat)
                if made is not None and len(made[0]) > 1:
                    break
            self.skips["hierarchy draws"] += 1
            if made is None:
                self.skips["hierarchy skipped"] += 1
                return self._log("hierarchy", f"amg({n.label}, {kind}) skipped: the reference refuses a level", node=n.id, action="skip")
            H = Hier(len(self.hiers), n, kind, kw, *made)
            self.hiers.append(H)
            self.stats[f"hierarchy setup {kind}"] += 1
            return self._cycle(H, n, f"{H.label} = amg({n.label}, {kind}, {kw}): {len(H.levels)} levels", "setup")
        H = live[int(rng.integers(len(live)))]
        n = self.nodes[H.src]
        self.skips["hierarchy draws"] += 1
        if not n.alive or n.uid != H.uid:
            H.alive = False
            return self._log("hierarchy", f"free {H.label}: its source {n.label} is gone", node=n.id, hier=H.id, action="free")
        stale = n.version != H.version
        action = self.HIER_ACTIONS[int(rng.integers(len(self.HIER_ACTIONS)))]
        if action == "apply_block" and H.width == 0 and rng.random() < 0.6:
            action = "set_block_width"                   # a workspace first: mostly a block cycle is one that is taken
        if stale:                                        # the cycle of a stale hierarchy is not specified: refresh it, or let it go
            action = "refresh"
        nu = dict(nu1=int(rng.integers(1, 4)), nu2=int(rng.integers(1, 4)), nuCoarse=int(rng.integers(1, 5)))
        if action == "set_storage":                          # (a subclass's action)
            return self._hier_storage(H, n)
        if action == "free":
            H.alive = False
            return self._log("hierarchy", f"free {H.label}", node=n.id, hier=H.id, action="free")
        if action == "refresh":
            made = self._levels(H.kind, H.kw, n.mat, H) if self.hier_ok(n) else None
            if made is None:
                H.alive = False
                self.skips["hierarchy skipped"] += 1
                return self._log("hierarchy", f"free {H.label}: {n.label}'s new values are not for a hierarchy", node=n.id, hier=H.id, action="free")
            H.levels, H.version, H.refreshed = made[0], n.version, True
            self.stats["hierarchy refresh" + (" while stale" if stale else "")] += 1
            return self._cycle(H, n, f"{H.label}.refresh_from({n.label})", "refresh")
        if action == "set_smoother":
            cheb = bool(rng.integers(2))
            args = dict(kind="chebyshev" if cheb else "jacobi", eig_ratio=float(rng.choice([4.0, 10.0])), **nu)
            H.sm = acr.smoother(H.o, kind=acr.CHEBYSHEV if cheb else acr.JACOBI, eigRatio=args["eig_ratio"], **nu)
            H.set_call = ("set_smoother", args)
            self.stats[f"hierarchy {args['kind']}"] += 1
            return self._cycle(H, n, f"{H.label}.set_smoother({args})", action, args=args)
        if action == "set_gauss_seidel":
            args = dict(omega=float(rng.choice([1.0, 0.9])), order=("natural", "hash")[int(rng.integers(2))], seed=int(rng.integers(1 << 16)),
                        one_way=bool(rng.integers(2)), levels=(None, 1)[int(rng.integers(2))], **nu)
            if H.storage == "f32":                           # refused: the sweeps read the double values; the smoother stays
                self.stats["hierarchy gauss_seidel refused in F32"] += 1
                return self._cycle(H, n, f"{H.label}.set_gauss_seidel({args}) refused: the hierarchy is stored in F32", action, args=args, refused=True)
            H.sm = ags.smoother(H.o, omega=args["omega"], order=ags.HASH if args["order"] == "hash" else ags.NATURAL, seed=args["seed"],
                                oneWay=args["one_way"], levels=args["levels"], **nu)
            H.set_call = ("set_gauss_seidel", args)
            self.stats["hierarchy gauss_seidel"] += 1
            return self._cycle(H, n, f"{H.label}.set_gauss_seidel({args})", action, args=args)
        if action == "set_block_width":
            H.width = int(rng.choice([0, 1, 3, 3, 16, 16] if H.width else [1, 3, 16]))
            self.stats["hierarchy set_block_width"] += 1
            return self._cycle(H, n, f"{H.label}.set_block_width({H.width})", action, args=dict(width=H.width))
        if action == "apply":
            self.stats["hierarchy apply"] += 1
            return self._cycle(H, n, f"{H.label}.apply, and a twin set up with the same settings", action, twin=not (H.kind == "strength" and H.refreshed) and H.storage == "f64")
        k = int(rng.choice([1, 3, 16]))
        if k > H.width > 0 and rng.random() < 0.7:       # mostly a block the workspace takes
            k = H.width
        R = rng.standard_normal((n.M, k))
        if H.sm["kind"] == ags.GAUSS_SEIDEL or k > H.width:
            why = "a Gauss-Seidel hierarchy" if H.sm["kind"] == ags.GAUSS_SEIDEL else f"the width is {H.width}"
            self.stats["hierarchy apply_block refused"] += 1
            return self._cycle(H, n, f"{H.label}.apply_block(k={k}) refused: {why}", "apply_block", R=R, Z=None)
        with np.errstate(all="ignore"):
            Z = abr.block_cycle_ref(H.active(), H.o, R, H.sm)
        self.stats["hierarchy apply_block"] += 1
        return self._cycle(H, n, f"{H.label}.apply_block(k={k})", "apply_block", R=R, Z=Z)

    def _cycle(self, H, n, text, action, **rec):
        """every hierarchy step ends in one cycle on a fresh r: the bits of the reference for the settings in force.
        (The twin of an `apply` step replays only the last set_* call: every count and option is passed explicitly, so a
        set_* call replaces the whole smoother state, and the width does not enter a single cycle.  A strength hierarchy has
        no twin after a refresh: the refresh keeps the kept sets of its setup, a fresh setup judges the new values again.)"""
        r = self.rng.standard_normal(n.M)
        with np.errstate(all="ignore"):
            z = H.cycle(r)
        self.stats["hierarchy cycles"] += 1
        if not n.selected[1]:                            # a cycle with an SpMV on level 0 runs the serial-order selection of the
            n.selected[1] = None                         # source, one of a single pass does not: not modelled until the next product
        if "R" not in rec and H.width and H.sm["kind"] != ags.GAUSS_SEIDEL:      # ... and, where a workspace stands, a block cycle
            k = min(H.width, int(self.rng.choice([1, 3, 16])))
            rec["R"] = self.rng.standard_normal((n.M, k))
            with np.errstate(all="ignore"):
                rec["Z"] = abr.block_cycle_ref(H.active(), H.o, rec["R"], H.sm)
            self.stats["hierarchy apply_block"] += 1
            text += f"; apply_block(k={k})"
        return self._log("hierarchy", text, node=n.id, hier=H.id, action=action, r=r, z=z, **rec)

    def _kind_values(self, n, kinds=KINDS):
        kind = kinds[int(self.rng.integers(len(kinds)))]
        return kind, values(self.rng, kind, n.IRP, n.JA, xs(n.N)[0])

    def op_set_values(self):
        n = self.pick(self.live(derived=False))
        how = "in place" if n.params["adopted"] and self.rng.random() < 0.5 else ("host", "device tensor")[int(self.rng.integers(2))]
        kind, v = self._kind_values(n)
        self._set(n, v)
        return self._log("set_values", f"new values for {n.label} ({kind}, {how})", node=n.id, how=how)

    def op_update_derived(self):
        cand = self.live(derived=True)
        holding = [c for c in cand if c.stripes]
        n = self.pick(holding if holding and self.rng.random() < 0.8 else cand)
        if n is None:
            return None
        holds = bool(n.stripes)                          # a node with a stripes format: the unit transitions are what counts
        kinds = ("constant", "constant", "constant", "constant_but_one", "uniform") if holds else KINDS
        kind, v = self._kind_values(n, kinds)
        if holds and n.unit[0] and self.rng.random() < 0.6:                  # unit values of ANOTHER value: only a register changes
            others = [c for c in CONSTANTS if np.float64(c).tobytes() != np.float64(n.unit[1]).tobytes()]
            kind, v = "constant", np.full(n.JA.size, others[int(self.rng.integers(len(others)))])
        self._set(n, v)
        return self._log("update_derived", f"update_values directly on {n.label} ({kind})", node=n.id, how="host")

    def op_reupload(self):
        n = self.pick(self.live(derived=False))
        kind, v = self._kind_values(n)
        old = n.id
        n.alive = False
        new = self._add("source", (), n.params, n.mat[:4] + (v,), None, n.label)
        return self._log("reupload", f"free + upload {n.label} again ({kind})", node=new.id, freed=old)

    def op_free(self):
        cand = self.live(derived=True)
        n = self.pick([c for c in cand if any(c.id in d.srcs for d in cand)]) or self.pick(cand)
        if n is None:
            return None
        n.alive = False
        users = [d.label for d in cand if n.id in d.srcs]
        return self._log("free", f"free {n.label}" + (f" (a source of {', '.join(users)})" if users else ""), node=n.id)

    # ---- new nodes
    def op_derive(self):
        if len(self.live()) >= MAX_LIVE:
            return self.op_free()
        rng = self.rng
        live = self.live()
        w = np.array([1.0 / (1.0 + sum(n.kind == k for n in live)) for k in DERIVED])       # the kinds the pool holds fewer of
        kind = DERIVED[int(rng.choice(len(DERIVED), p=w / w.sum()))]
        deep = 0.65
        srcs = params = None
        if kind == "permute":
            x = self.pick(self.live(square=True), deep)
            srcs, params = (x.id,), self._permute_params(x)
        elif kind == "multiply":
            x = self.pick(live, deep)
            own = [t for t in live if t.kind == "transpose" and t.srcs == (x.id,)]
            if own and rng.random() < 0.5:               # a matrix times its own transpose handle, either way round
                pair = (x, own[0]) if rng.integers(2) else (own[0], x)
            else:
                pair = (x, self.pick([y for y in live if y.M == x.N], deep))
            if pair[1] is not None and sr.products(pair[0].mat, pair[1].mat)[3].sum() <= 8 * MAX_NNZ:
                srcs, params = (pair[0].id, pair[1].id), {}
        elif kind == "add":
            x = self.pick(live, deep)
            y = self.pick([y for y in live if (y.M, y.N) == (x.M, x.N)], deep)      # (x itself among them)
            r = rng.integers(4)
            own = [t for t in live if t.kind == "transpose" and t.srcs == (x.id,) and t.square]
            diag = [f for f in live if f.kind == "filter" and f.srcs == (x.id,) and f.params == fr.opts(fr.BAND, 0, 0)]
            alpha, beta = [float(c) for c in rng.choice([1.0, -1.0, 0.0, 0.5, -2.5, 3.0], 2)]
            if own and r == 0:                           # X + X^T
                y, alpha, beta = own[0], 1.0, 1.0
            elif diag and r == 1:                        # X - sigma diag(X)
                y, alpha, beta = diag[0], 1.0, -float(rng.uniform(0.05, 0.6))
            srcs, params = (x.id, y.id), dict(alpha=alpha, beta=beta)
        elif kind == "filter":
            x = self.pick(live, deep)
            srcs, params = (x.id,), self._filter_opts(x)
        if srcs is None:
            kind, srcs, params = "transpose", (self.pick(live, deep).id,), {}
        S = [self.nodes[s].mat for s in srcs]
        with np.errstate(all="ignore"):
            mat, aux = build_node(kind, params, S)
        if mat[3].size == 0 or mat[3].size > MAX_NNZ:    # nothing kept, or too large for a seed of seconds: the transpose instead
            kind, srcs, params = "transpose", srcs[:1], {}
            mat, aux = build_node(kind, params, S[:1])
        names = ", ".join(self.nodes[s].label for s in srcs)
        label = f"n{self._id}"
        n = self._add(kind, srcs, params, mat, aux, label)
        self.stats["derive " + kind] += 1
        self.stats["depth"] = max(self.stats["depth"], n.depth)
        text = f"{label} = {kind}({names}{self._show(kind, params)}): {n.M} x {n.N}, {n.JA.size} entries, depth {n.depth}"
        return self._log("derive", text, node=n.id, kind=kind, srcs=srcs, params=params)

    def _permute_params(self, x):
        return dict(order=("natural", "hash")[int(self.rng.integers(2))], seed=int(self.rng.integers(1 << 16)))

    def _situations(self, c):
        """further (name, holds) pairs of a node about to be refreshed, for the weights and the counts (a subclass's hook)"""
        return []

    @staticmethod
    def _show(kind, p):
        if kind == "filter":
            mode = ("band", "abs", "strength")[p["mode"]]
            lo = "" if p["lo"] == fr.INT64_MIN else p["lo"]
            hi = "" if p["hi"] == fr.INT64_MAX else p["hi"]
            return f"; {mode}, [{lo}..{hi}], theta={p['theta']:.6g}, lump={int(p['lump'])}"
        return "; " + ", ".join(f"{k}={v}" for k, v in p.items()) if p else ""

    def _filter_opts(self, x):
        rng = self.rng
        r = int(rng.integers(8))
        mag = np.abs(x.vals[np.isfinite(x.vals)])
        theta = float(np.quantile(mag, rng.uniform(0.2, 0.7))) if mag.size else 0.5
        lump = bool(rng.integers(2))
        if r == 0:
            return fr.opts(fr.BAND, None, int(rng.integers(-1, 2)))          # tril(k)
        if r == 1:
            return fr.opts(fr.BAND, int(rng.integers(-1, 2)), None)          # triu(k)
        if r == 2:
            return fr.opts(fr.BAND, 0, 0)                                    # diagonal_matrix()
        if r == 3:
            return fr.opts(fr.BAND, -int(rng.integers(1, 25)), int(rng.integers(1, 25)))
        if r in (4, 5) or not x.one_diagonal:
            return fr.opts(fr.ABS, theta=theta, lump=lump and x.one_diagonal)
        return fr.opts(fr.STRENGTH, theta=float(rng.uniform(0.05, 0.6)), lump=lump)

    # ---- refreshes
    def op_refresh(self):
        cand = [c for c in self.live(derived=True) if self.refreshable(c)]
        if not cand:
            return None
        # a node with formats of its own or a stale source is what a refresh can get wrong: those are drawn more often, and
        # most of all in a situation this seed has not had yet for the node's kind
        def weight(c):
            here = [("source stale", any(self.stale(self.nodes[s]) for s in c.srcs)), ("two-phase built before", c.tiles is not None),
                    ("stripes built before", bool(c.stripes)), ("SELL built before", c.sell)] + self._situations(c)
            return 0.2 + 0.5 / (1.0 + self.stats[f"refresh {c.kind}"]) + sum((1.0 + 2.0 * (what == "source stale")) / (1.0 + self.stats[f"refresh {c.kind}: {what}"]) for what, on in here if on)
        w = np.array([weight(c) for c in cand])
        n = cand[int(self.rng.choice(len(cand), p=w / w.sum()))]
        S = [self.nodes[s] for s in n.srcs]
        params = n.params
        if n.kind == "add" and self.rng.random() < 0.3:                      # alpha and beta may be new
            a, b = [float(c) for c in self.rng.choice([1.0, -1.0, 0.0, 0.5, -2.5, 3.0], 2)]
            params = dict(alpha=a, beta=b)
        k = n.kind
        self.stats[f"refresh {k}"] += 1
        stale = [s for s in S if self.stale(s)]
        if stale:
            self.stats[f"refresh {k}: source stale"] += 1
            self.stats["stale refresh"] += 1
            if any(not same_bits(s.vals, self.fresh_values(s)) for s in stale):
                self.stats["stale refresh: the source's values differ from a fresh build"] += 1
        if n.tiles is not None:
            self.stats[f"refresh {k}: two-phase built before"] += 1
        if n.stripes:
            self.stats[f"refresh {k}: stripes built before"] += 1
        if n.sell:
            self.stats[f"refresh {k}: SELL built before"] += 1
        if n.factored:
            self.stats["ilu0, later a refresh of the node"] += 1
        for what, on in self._situations(n):
            if on:
                self.stats[f"refresh {k}: {what}"] += 1
        n.params = params
        with np.errstate(all="ignore"):
            self._set(n, refresh_values(k, params, n.aux, [s.mat for s in S]))
        n.seen = tuple((s.uid, s.version) for s in S)
        text = f"refresh {n.label} from {', '.join(s.label for s in S)}" + (f" (stale: {', '.join(s.label for s in stale)})" if stale else "")
        if n.kind == "add":
            text += f" alpha={params['alpha']}, beta={params['beta']}"
        return self._log("refresh", text, node=n.id, params=params)

    def op_refresh_refused(self):
        cand = self.live(derived=True)
        broken = [c for c in cand if not self.refreshable(c)]
        if broken and self.rng.random() < 0.7:
            n = self.pick(broken)
            use, why = [], []
            for s, (u, _) in zip(n.srcs, n.seen):
                src = self.nodes[s]
                if src.alive:
                    use.append(s)
                    continue
                again = [m for m in self.live(derived=False) if m.label == src.label] if not src.derived else []
                use.append(again[0].id if again else s)                      # the re-uploaded source, or the freed handle
                why.append(f"{src.label} was " + ("uploaded again" if again else "freed"))
            return self._log("refresh_refused", f"refresh {n.label}: refused, {' and '.join(why)}", node=n.id, use=tuple(use))
        n = self.pick(cand)
        if n is None:
            return None
        wrong = self.pick([m for m in self.live() if m.id != n.id and m.id not in n.srcs])
        use = list(n.srcs)
        at = int(self.rng.integers(len(use)))
        use[at] = wrong.id
        if len(use) == 2 and self.rng.random() < 0.3 and n.srcs[0] != n.srcs[1]:
            use, wrong = [n.srcs[1], n.srcs[0]], None                        # the pair in the other order
        if any(not self.nodes[s].alive for s in use):
            return None
        text = f"refresh {n.label}: refused, " + (f"{wrong.label} is not its source" if wrong else "its pair in the other order")
        return self._log("refresh_refused", text, node=n.id, use=tuple(use))

    # ---- formats and products
    def op_build(self):
        rng = self.rng
        cand = self.live(derived=True)
        if cand and rng.random() < 0.85:                 # mostly a derived node, of a kind that had fewer builds
            w = np.array([1.0 / (1.0 + self.stats[f"build {c.kind}"]) for c in cand])
            n = cand[int(rng.choice(len(cand), p=w / w.sum()))]
        else:
            n = self.pick(self.live())
        self.stats[f"build {n.kind}"] += 1
        r = (self.seed + self.stats[f"build {n.kind}"]) % 3                 # the three formats in turn for every kind of node
        if r == 0:
            det = bool(rng.integers(2))
            n.tiles = det
            return self._log("build", f"build_tiles({n.label}, deterministic={int(det)})", node=n.id, what="tiles", det=det)
        if r == 1:
            det = int(rng.integers(3))
            opts = dict(spread=int(rng.choice([-1, 0, 1, 4, 64])), grid=int(rng.choice([0, 0, 7, 32])), rowsPerBin=int(rng.choice([0, 0, 256, 1024])))
            n.stripes_det = det
            n.stripes["owner" if det == 1 else "shared"] = bool(n.unit[0])
            return self._log("build", f"build_stripes({n.label}, deterministic={det}, {opts})", node=n.id, what="stripes", det=det, opts=opts)
        n.sell = True
        return self._log("build", f"spmvHipBuildSell({n.label})", node=n.id, what="sell")

    def op_product(self):
        n = self.pick(self.live(), 0.8)
        which = PRODUCTS[int(self.rng.integers(len(PRODUCTS)))]
        dirty = [c for c in self.live() if c.dirty]
        if dirty and self.rng.random() < 0.6:            # mostly through a format whose values a refresh or an update has changed:
            n = self.pick(dirty, 0.8)                    # the product that shows whether the tail refreshed it
            which = sorted(n.dirty)[int(self.rng.integers(len(n.dirty)))]
        if which in n.dirty:
            self.stats[f"product through {which} after its values changed"] += 1
            n.dirty.discard(which)
        nx = int(self.rng.integers(2))
        user = bool(self.rng.integers(2)) or which.startswith("enq_csr")
        x = xs(n.N)[nx]
        any_ok = in_exact_range(n.vals)
        serial = which in ("rows", "enq_auto_rows", "enq_csr0") or (which == "tiles" and bool(n.tiles)) or (which == "stripes" and n.stripes_det > 0)
        if which == "tiles" and n.tiles is None:
            n.tiles = False
        if which == "stripes":
            n.stripes.setdefault("owner" if n.stripes_det == 1 else "shared", bool(n.unit[0]))
        if which == "sell":
            n.sell = True
        if which in ("warp", "auto", "enq_auto"):
            n.selected[0] = True
        if which in ("rows", "enq_auto_rows"):
            n.selected[1] = True
        self.skips["product draws"] += 1
        if not serial and not any_ok:
            self.skips["product skipped"] += 1
        text = f"{which}({n.label}, x{nx})" + (f" on the {'user' if user else 'null'} stream" if which.startswith("enq_") else "")
        return self._log("product", text, node=n.id, which=which, x=x, user=user, serial=serial, check=serial or any_ok)

    def op_matmul(self):
        n = self.pick(self.live(), 0.8)
        k = int(self.rng.choice([1, 3, 16]))
        xl, yl = int(self.rng.integers(2)), int(self.rng.integers(2))
        x0, x1 = xs(n.N)
        X = np.stack([(x0, x1)[c % 2] * (1.0 + c) for c in range(k)], axis=1)
        text = f"matmul({n.label}, k={k}, X {'col' if xl else 'row'}-major, Y {'col' if yl else 'row'}-major)"
        return self._log("matmul", text, node=n.id, X=X, xl=xl, yl=yl)

    # ---- solves
    def op_solve(self):
        n = self.pick(self.live(one_diagonal=True), 0.85)
        lower, unit = bool(self.rng.integers(2)), bool(self.rng.integers(2))
        k = int(self.rng.choice([0, 0, 1, 3, 16]))                           # 0: solve_triangular, else the block solve
        B = self.rng.uniform(-1.0, 1.0, (n.M, max(k, 1)))
        self.skips["solve draws"] += 1
        check = bool(np.isfinite(n.vals).all())
        if not check:
            self.skips["solve skipped"] += 1
        call = "solve_triangular" if k == 0 else f"solve_triangular_block k={k}"
        text = f"{call}({n.label}, lower={int(lower)}, unit_diagonal={int(unit)})" + ("" if check else " skipped: a non-finite value")
        return self._log("solve", text, node=n.id, lower=lower, unit=unit, k=k, B=B, check=check)

    def op_ilu0(self):
        cand = self.live(derived=True, ilu_ok=True)
        with np.errstate(all="ignore"):                  # mostly a node whose factors are finite: the solves that follow count
            sound = [c for c in cand if np.isfinite(c.vals).all() and np.isfinite(ilu0_levels(c.M, c.IRP, c.JA, c.vals)).all()]
        if not sound and self.rng.random() < 0.8:        # a non-finite factor now and then, not as a rule
            return None
        n = self.pick(sound if sound and self.rng.random() < 0.97 else cand)
        if n is None:
            return None
        F = ilu0_levels(n.M, n.IRP, n.JA, n.vals)
        zero = np.flatnonzero(F[n.dpos] == 0.0)
        again = n.factored
        self._set(n, F, factored=True)
        b = self.rng.uniform(-1.0, 1.0, n.M)
        self.skips["ilu0 solve draws"] += 1
        check = bool(np.isfinite(F).all())
        if not check:
            self.skips["ilu0 solve skipped"] += 1
        text = f"ilu0({n.label})" + (" again, on the factors" if again else "") + (", then L and U solves" if check else ", a non-finite factor: no solves")
        return self._log("ilu0", text, node=n.id, zeroPivot=int(zero[0]) if zero.size else -1, b=b, solves=check)

    def op_krylov(self):
        cand = [c for c in self.live(ilu_ok=True) if np.isfinite(c.vals).all()]
        spd = [c for c in cand if self.is_spd(c)]
        n = self.pick(spd if spd and self.rng.random() < 0.8 else cand)
        if n is None:
            return None
        rng = self.rng
        method = ("cg", "bicgstab", "gmres")[int(rng.integers(3))]
        maxiter = int(rng.choice([2, 5, 12, 30]))
        tol = float(rng.choice([1e-3, 1e-8]))
        restart = int(rng.choice([4, 10])) if method == "gmres" else None
        b = rng.uniform(-1.0, 1.0, n.M)
        F = None
        if rng.integers(2):
            F = ilu0_levels(n.M, n.IRP, n.JA, n.vals)
            F = F if np.isfinite(F).all() and (F[n.dpos] != 0.0).all() else None
        A = Csr(n.M, n.IRP, n.JA, n.vals, F)
        x0 = np.zeros(n.M)
        if method == "cg":
            want = cg_ref(A, b, x0, tol, maxiter)
        elif method == "bicgstab":
            want = bicgstab_ref(A, b, x0, tol, maxiter)
        else:
            want = gmres_ref(A, b, x0, tol, maxiter, restart)
        n.selected[1] = True                             # the solvers' SpMV is the serial-order launcher: its selection runs
        self.skips["krylov draws"] += 1
        check = bool(np.isfinite(want[0]).all())
        if not check:
            self.skips["krylov skipped"] += 1
        self.stats[f"krylov status {want[1]}"] += 1
        text = (f"{method}({n.label}, precond={'a factored copy' if F is not None else None}, tol={tol}, maxiter={maxiter}"
                + (f", restart={restart}" if restart else "") + f"): status {want[1]} after {want[2]}" + ("" if check else " skipped: x is not finite"))
        return self._log("krylov", text, node=n.id, method=method, maxiter=maxiter, tol=tol, restart=restart, b=b, F=F, want=want, check=check)

    def is_spd(self, n):
        """symmetric as bits and strictly diagonally dominant with a positive diagonal: enough for SPD"""
        if not n.ilu_ok:
            return False
        T = sr.transpose(n.mat)
        if not (np.array_equal(T[2], n.IRP) and np.array_equal(T[3], n.JA) and same_bits(T[4], n.vals)):
            return False
        d = n.vals[n.dpos]
        off = np.bincount(sr.si.row_of_entry(n.IRP), weights=np.abs(n.vals), minlength=n.M) - np.abs(d)
        return bool((d > 0).all() and (d >= off).all())
