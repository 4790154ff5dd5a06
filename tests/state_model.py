"""The second seeded generator of operation sequences: derived_model.Generator with the per-handle state of the later
features (tests/test_state_model.py runs it dry, tests/test_gpu_state_sequences.py against the device).

It takes every operation of derived_model and adds, composed from the references that exist (no arithmetic of its own):
  * a fourth source Q, the 23 x 19 grid operator assembled from shuffled element triplets (coo_ref; every stored entry the
    sum of 1 to 4 triplets, duplicates "sum" or "last" by the seed), whose value update is assemble_refresh;
  * permutations by reverse Cuthill-McKee (rcm_ref.rcm_loop) beside those by a colouring;
  * the single-precision value form of a node (values_f32_ref): built and released, followed through every value update,
    refresh and ILU(0), its products refused without it; the value kind `f32_edges` plants the rounding's boundary values;
  * the sweep plan and the apply mode of a node with one diagonal per row (sweeps_ref): prepared, widened, set and reset,
    sweep solves single and block, and both kept across every write into the node;
  * Krylov solves (single and block, k = 3) whose preconditioner is a live factored node of the pool in its apply mode, or a
    live `fsai` node in its storage;
  * the derived kind `fsai` (fsai_ref.fsai_loop): the factor of a node on its own pattern or a band filter's, refreshed also
    while its source is stale, switched between F64 and F32 storage, a source of further nodes, never written into and never
    the source of a hierarchy;
  * hierarchy set_storage (values_f32_ref.rounded_levels), with its two mutual refusals with Gauss-Seidel and the form it
    builds on, and releases from, the source node;
  * eigsh by lanczos_ref / davidson_ref on SPD nodes, Davidson also preconditioned by a live hierarchy or fsai node.
A node's state is part of every record (`state`): a backend compares it after every step.  SEEDS and OPS are this module's
own; derived_model's seeds draw exactly what they drew before (it gained hooks, no draw)."""
import functools

import numpy as np

import coo_ref as co
import fsai_ref
import derived_model as dm
import sweeps_ref as sw
import values_f32_ref as vr
from block_krylov_ref import block_ref
from derived_model import in_exact_range, same_bits, xs
from davidson_ref import davidson_ref
from gmres_ref import gmres_ref
from ilu0_ref import ilu0_levels
from krylov_ref import Csr, bicgstab_ref, cg_ref
from lanczos_ref import SMALLEST, lanczos_ref
from sequence_inputs import CONSTANTS, KINDS, values
from trsv_ref import levels, trsv_levels

SEEDS = tuple(range(100, 140))
STEPS = 50
NEW_OPS = ("values_f32", "product_f32", "sweeps_prepare", "sweeps_apply", "sweeps_solve", "fsai", "eigsh")
OPS = (("set_values", 12), ("update_derived", 13), ("derive", 12), ("refresh", 26), ("refresh_refused", 3), ("free", 2), ("reupload", 2),
       ("build", 9), ("product", 8), ("matmul", 3), ("solve", 3), ("ilu0", 9), ("krylov", 12), ("hierarchy", 21),
       ("values_f32", 15), ("product_f32", 14), ("sweeps_prepare", 4), ("sweeps_apply", 9), ("sweeps_solve", 8), ("fsai", 9), ("eigsh", 6))
F32_PRODUCTS = ("rows_f32", "warp_f32", "enq_rows_f32", "matmul_f32")
WIDTHS = (0, 1, 3, 16)
SWEEPS = (0, 1, 2, 5)
MAX_SWEEPS = 96                         # of a solve with S = levels - 1 (a longer chain costs the dry run seconds)
Q_KINDS = ("uniform", "uniform", "wide", "constant", "constant_but_one")
DIAG_W, OFF_W = 1.6, -0.25              # an element's share of a diagonal / an off-diagonal entry (see q_values)


# ------------------------------------------------------------------------------------------------------- the source Q
@functools.lru_cache(maxsize=None)
def q_triplets():
    """(rows, cols, slot, weight) of Q's triplet list: every cell of the grid gives its four corners a share of their
    diagonal entry and its four edges a share of both off-diagonal entries (so a diagonal entry is the sum of 1, 2 or 4
    triplets, an off-diagonal one of 1 or 2), the (cell, item) pairs shuffled; slot: the pair's number -- both directions of
    an edge share one, so they get the same value and stand next to each other in the list"""
    rng = np.random.default_rng(4310)
    nx, ny = dm.GRID
    items = []
    for cy in range(ny - 1):
        for cx in range(nx - 1):
            c = (cy * nx + cx, cy * nx + cx + 1, (cy + 1) * nx + cx, (cy + 1) * nx + cx + 1)
            items += [((v, v),) for v in c]
            items += [((a, b), (b, a)) for a, b in ((c[0], c[1]), (c[2], c[3]), (c[0], c[2]), (c[1], c[3]))]
    rows, cols, slot, w = [], [], [], []
    for s, u in enumerate(rng.permutation(len(items))):
        for i, j in items[u]:
            rows.append(i), cols.append(j), slot.append(s), w.append(DIAG_W if i == j else OFF_W)
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(slot, dtype=np.int64), np.array(w)


def q_values(rng, kind):
    """the triplet values of one kind, scaled onto the stencil: weight * (1 + 0.2 u) for `uniform` (u in [-1, 1] per slot),
    weight * value for the others.  For `uniform` Q is SPD in both duplicate modes: its two triangles get the same bits (the
    two directions of an edge share their values, and a sum of two is commutative; "last" takes both from the same cell),
    a diagonal entry is at least 1.6 * 0.8 = 1.28 per contributing cell, and the off-diagonal entries of a row of c cells
    sum to at most 0.25 * 1.2 * 2 c <= 1.28 c in "sum" mode and to at most 4 * 0.3 = 1.2 in "last" mode."""
    rows, cols, slot, w = q_triplets()
    k = values(rng, kind, None, np.empty(int(slot.max()) + 1), None)
    return w * (1.0 + 0.2 * k[slot]) if kind == "uniform" else w * k[slot]


@functools.lru_cache(maxsize=None)
def q_source(mode):
    """(matrix, runs, first triplet values) of Q assembled with the duplicate mode"""
    rows, cols, _, _ = q_triplets()
    vals = q_values(np.random.default_rng(4311), "uniform")
    M = dm.GRID[0] * dm.GRID[1]
    C, info, runs = co.assemble_ref(M, M, rows, cols, vals, mode)
    return C, runs, vals


# ----------------------------------------------------------------------------------------------------- node state
def f32_bytes(n):
    return 0 if n.unit[0] or n.JA.size == 0 else (4 * n.JA.size + 15) // 16 * 16 + 32


def apply_launches(apply):
    """spmvTriSweepsInfo.applyLaunches by the header's rule: S_L + S_U, + 1 when one of them is 0; EXACT: 0"""
    if apply[0] == "exact":
        return 0
    return apply[1] + apply[2] + (0 if apply[1] and apply[2] else 1)


class Pooled(Csr):
    """krylov_ref.Csr of the operator with M^-1 v = U^-1 (L^-1 v) from the factors a pooled node P holds (its own pattern), by
    the exact solves (trsv_ref) or by P's sweep counts (sweeps_ref), as P's apply mode says"""

    def __init__(self, n, P):
        super().__init__(n.M, n.IRP, n.JA, n.vals)
        self.P, self.apply = (P.M, P.IRP, P.JA, P.vals), P.apply
        self.F = P.vals                                      # (the reference loops take `F is not None` for "preconditioned")
        self.lvl = (levels(P.M, P.IRP, P.JA, True), levels(P.M, P.IRP, P.JA, False))
        self.applications = 0

    def precond(self, v):
        self.applications += 1
        if self.apply[0] == "exact":
            w = trsv_levels(*self.P, v, True, True, self.lvl[0])
            return trsv_levels(*self.P, w, False, False, self.lvl[1])
        w = sw.sweeps_numpy(*self.P, v, self.apply[1], True, True)
        return sw.sweeps_numpy(*self.P, w, self.apply[2], False, False)


class Generator(dm.Generator):
    OPS = OPS
    HIER_ACTIONS = dm.Generator.HIER_ACTIONS + ("set_storage",) * 6 + ("set_gauss_seidel", "set_gauss_seidel") + ("refresh",) * 5

    def __init__(self, seed, steps=STEPS):
        super().__init__(seed, steps)
        self.q_mode = ("sum", "last")[seed % 2]
        self.q = None                   # Q's triplet values now (rows and cols: q_triplets())

    def sources(self):
        C, runs, vals = q_source(self.q_mode)
        self.q = vals
        return dict(dm.sources(), Q=C)

    # ------------------------------------------------------------------------------------------------------ the pool
    def _add(self, kind, srcs, params, mat, aux, label):
        n = super()._add(kind, srcs, params, mat, aux, label)
        n.f32 = None                    # the single-precision form: None, or dict(refreshes)
        n.f32_changed = False           # the values changed since the last f32 product
        n.plan = None                   # the sweep plan: None, or dict(width, prepares)
        n.apply = ("exact",)            # or ("sweeps", S_L, S_U)
        n.storage = n.setups = n.fsai_info = None           # of an `fsai` node: "f64" / "f32", spmvFsaiInfo.setups, the reference's info
        if any(self.nodes[s].kind == "fsai" for s in srcs):
            self.stats["an fsai node used as a source"] += 1
        return n

    def state_of(self, n):
        """what the device must report for the node now: values_f32_info() and triangular_sweeps_info()"""
        f32 = None
        if n.f32 is not None:
            f32 = dict(built=1, unit=int(n.unit[0]), bytes=f32_bytes(n), refreshes=n.f32["refreshes"], counts=vr.counts(n.vals))
        plan = None if n.plan is None else dict(n.plan, bytes=4 * n.M + 16 * n.M * n.plan["width"])
        fsai = None if n.kind != "fsai" else dict(storage=n.storage, setups=n.setups)
        return dict(f32=f32, plan=plan, apply=n.apply, applyLaunches=apply_launches(n.apply), fsai=fsai)

    def _log(self, op, text, **rec):
        rec = super()._log(op, text, **rec)
        n = self.nodes.get(rec.get("node"))
        if n is not None and n.alive:
            rec["state"], rec["vals"] = self.state_of(n), n.vals         # (vals: the node's values now -- no write mutates an array)
            if n.kind == "fsai":
                rec["fsai_info"] = n.fsai_info
        return rec

    def _set(self, n, vals, factored=False):
        before, pattern = n.unit, (n.IRP, n.JA)
        super()._set(n, vals, factored)
        assert n.IRP is pattern[0] and n.JA is pattern[1]    # no write changes a pattern: a plan's diagPos stays valid
        if n.kind == "fsai":                                 # (the only writer of a factor is its refresh)
            with np.errstate(all="ignore"):
                n.fsai_info = fsai_ref.fsai_loop(self.nodes[n.srcs[0]].mat, n.aux)[1]
            n.setups += 1
        if n.f32 is not None:
            n.f32["refreshes"] += 1
            n.f32_changed = True
            same = before[0] and n.unit[0] and np.float64(before[1]).tobytes() == np.float64(n.unit[1]).tobytes()
            if not before[0] and n.unit[0]:
                self.stats["f32: non-unit -> unit"] += 1
            elif before[0] and n.unit[0] and not same:
                self.stats["f32: unit -> unit of another value"] += 1
            elif before[0] and not n.unit[0]:
                self.stats["f32: unit -> non-unit"] += 1

    def _situations(self, c):
        if c.kind == "fsai":
            return [("F32 storage", c.storage == "f32")]
        return [("f32 form built", c.f32 is not None), ("plan in SWEEPS mode", c.apply[0] == "sweeps")]

    def below(self, n):
        """the live derived nodes made, directly or not, from n"""
        out, grew = {n.id}, True
        while grew:
            grew = False
            for d in self.live(derived=True):
                if d.id not in out and any(s in out for s in d.srcs):
                    out.add(d.id)
                    grew = True
        return len(out) - 1

    # ---------------------------------------------------------------------------------------------------- values
    def _kind_values(self, n, kinds=KINDS):
        if n.f32 is not None and self.rng.random() < 0.2:    # the rounding's boundary values among ordinary ones
            v = values(self.rng, "uniform", n.IRP, n.JA, xs(n.N)[0])
            at = self.rng.choice(v.size, min(5, v.size), replace=False)
            v[at] = self.rng.choice(vr.boundary_values(), at.size)
            self.stats["f32_edges"] += 1
            return "f32_edges", v
        return super()._kind_values(n, kinds)

    def op_set_values(self):
        n = self.pick(self.live(derived=False))
        if n.label != "Q":
            how = "in place" if n.params["adopted"] and self.rng.random() < 0.5 else ("host", "device tensor")[int(self.rng.integers(2))]
            kind, v = self._kind_values(n)
            self._set(n, v)
            return self._log("set_values", f"new values for {n.label} ({kind}, {how})", node=n.id, how=how)
        how = ("host", "device tensor")[int(self.rng.integers(2))]
        kind = Q_KINDS[int(self.rng.integers(len(Q_KINDS)))]
        self.q = q_values(self.rng, kind)
        C, runs, _ = q_source(self.q_mode)
        with np.errstate(all="ignore"):
            self._set(n, co.refresh_ref(C, runs, self.q, self.q_mode)[4])
        below = self.below(n)
        self.stats["assemble_refresh"] += 1
        if below >= 2:
            self.stats["assemble_refresh with two or more derived nodes below"] += 1
        if n.f32 is not None:
            self.stats["assemble_refresh with the f32 form built"] += 1
        return self._log("set_values", f"assemble_refresh of Q (triplet values: {kind}, {how}; {below} derived nodes below)", node=n.id, how=how,
                         triplets=self.q.copy())

    def op_update_derived(self):
        cand = [c for c in self.live(derived=True) if c.kind != "fsai"]
        holding = [c for c in cand if c.f32 is not None] if self.rng.random() < 0.6 else []
        holding = holding or [c for c in cand if c.stripes or c.f32 is not None]
        n = self.pick(holding if holding and self.rng.random() < 0.8 else cand)
        if n is None:
            return None
        holds = bool(n.stripes) or n.f32 is not None         # a stripes format or an f32 form: the unit transitions are what counts
        kinds = ("constant", "constant", "constant", "constant_but_one", "uniform") if holds else KINDS
        kind, v = self._kind_values(n, kinds)
        if holds and n.unit[0] and self.rng.random() < 0.6 and kind != "f32_edges":
            others = [c for c in CONSTANTS if np.float64(c).tobytes() != np.float64(n.unit[1]).tobytes()]
            kind, v = "constant", np.full(n.JA.size, others[int(self.rng.integers(len(others)))])
        self._set(n, v)
        return self._log("update_derived", f"update_values directly on {n.label} ({kind})", node=n.id, how="host")

    def op_reupload(self):
        n = self.pick([s for s in self.live(derived=False) if s.label != "Q"])
        kind, v = self._kind_values(n)
        old = n.id
        n.alive = False
        new = self._add("source", (), n.params, n.mat[:4] + (v,), None, n.label)
        return self._log("reupload", f"free + upload {n.label} again ({kind})", node=new.id, freed=old)

    def _permute_params(self, x):
        if self.rng.random() < 0.5:
            self.stats["permute by rcm"] += 1
            return dict(order="rcm", start=("peripheral", "min_degree")[int(self.rng.integers(2))], max_passes=int(self.rng.choice([0, 1, 3])),
                        forward=bool(self.rng.integers(2)))
        return super()._permute_params(x)

    # ------------------------------------------------------------------------------------------------- the f32 form
    @staticmethod
    def _applied(g):
        """an fsai node was applied as M^-1: the first application chooses the kernels of G and G^T (spmvHipFsaiApply in
        spmvHip.h), which is G's serial-order selection; the f32 products have no selection, so in F32 storage it may or may
        not have run"""
        if g.storage == "f64":
            g.selected[1] = True
        elif not g.selected[1]:
            g.selected[1] = None

    def hier_ok(self, n):
        """no hierarchy stands on a factor: its set_storage would build a form on G outside spmvHipFsaiSetStorage"""
        return n.kind != "fsai" and super().hier_ok(n)

    def _f32_hiers(self, n):
        """the live hierarchies on n stored in F32: their cycles stream n's form"""
        return [H for H in self.hiers if H.alive and H.src == n.id and H.uid == n.uid and H.storage == "f32"]

    def _hier_storage(self, H, n):
        """spmvHipAmgSetStorage: F32 builds the form on the source (if it has none: then F64 releases it again) and on the levels;
        refused on a Gauss-Seidel hierarchy.  A second F32 hierarchy on one node is not drawn: the first one's F64 could take
        the node's form from under it."""
        storage = ("f32", "f64")[H.storage == "f32"] if self.rng.random() < 0.85 else H.storage
        if H.sm["kind"] == dm.ags.GAUSS_SEIDEL and self.rng.random() < 0.7:      # the refusal is what a Gauss-Seidel hierarchy has to show
            storage = "f32"
        if storage == "f32" and [X for X in self._f32_hiers(n) if X is not H]:
            storage = H.storage
        args = dict(storage=storage)
        if storage == "f32" and H.sm["kind"] == dm.ags.GAUSS_SEIDEL:
            self.stats["hierarchy F32 refused on Gauss-Seidel"] += 1
            return self._cycle(H, n, f"{H.label}.set_storage(f32) refused: a Gauss-Seidel hierarchy", "set_storage", args=args, refused=True)
        if storage == "f32":
            if n.f32 is None:
                n.f32, n.f32_changed, H.a0form = dict(refreshes=0), False, True
        else:
            if H.a0form:
                n.f32 = None
            H.a0form = False
        if storage != H.storage:
            self.stats[f"hierarchy set_storage {storage}"] += 1
        H.storage = storage
        return self._cycle(H, n, f"{H.label}.set_storage({storage})", "set_storage", args=args)

    def _cycle(self, H, n, text, action, **rec):
        if action == "refresh" and H.storage == "f32":
            self.stats["hierarchy refresh in F32"] += 1
        rec = super()._cycle(H, n, text, action, **rec)
        rec["hstate"] = dict(storage=H.storage, levels=len(H.levels))
        rec["state"] = self.state_of(n)                      # (set_storage may have built or released the node's form)
        return rec

    def op_values_f32(self):
        cand = [c for c in self.live() if c.kind != "fsai" and not self._f32_hiers(c)]       # (a form a hierarchy streams is left alone)
        w = np.array([1.0 + 2.0 * c.derived + 2.0 * bool(c.stripes or c.sell or c.tiles is not None) + 3.0 * (c.label == "Q") + 6.0 * (c.derived and not self.stats[f"refresh {c.kind}: f32 form built"])
                      + 8.0 / (1.0 + self.stats[f"values_f32 on {c.kind}"]) for c in cand])
        n = cand[int(self.rng.choice(len(cand), p=w / w.sum()))]
        on = n.f32 is None or self.rng.random() < 0.75
        again = on and n.f32 is not None
        if on and n.f32 is None:
            n.f32, n.f32_changed = dict(refreshes=0), False
            self.stats[f"values_f32 on {n.kind}"] += 1
        elif not on:
            n.f32 = None
        text = f"values_f32({n.label}, {on})" + (" again: nothing changes" if again else "")
        return self._log("values_f32", text, node=n.id, on=on)

    def op_product_f32(self):
        rng = self.rng
        built = [c for c in self.live() if c.f32 is not None]
        changed = [c for c in built if c.f32_changed]
        if not built:                                        # nothing to multiply by: a form is built instead, for the next product
            return self.op_values_f32()
        if rng.random() < 0.8:
            n = self.pick(changed if changed and rng.random() < 0.7 else built, 0.7)
        else:                                                # now and then a node without the form: the product is refused
            n = self.pick([c for c in self.live() if c.f32 is None] or self.live(), 0.7)
        which = F32_PRODUCTS[int(rng.integers(len(F32_PRODUCTS)))]
        nx, k, user = int(rng.integers(2)), int(rng.choice([1, 3, 16])), bool(rng.integers(2))
        x0, x1 = xs(n.N)
        X = np.stack([(x0, x1)[(c + nx) % 2] * (1.0 + c) for c in range(k)], axis=1) if which == "matmul_f32" else (x0, x1)[nx][:, None]
        text = f"{which}({n.label}, x{nx}" + (f", k={k}" if which == "matmul_f32" else "") + ")"
        if n.f32 is None:
            self.stats["f32 product refused"] += 1
            return self._log("product_f32", text + " refused: the form is not built", node=n.id, which=which, X=X, user=user, vals32=None, check=True)
        if n.f32_changed:
            self.stats["f32 product after the values changed"] += 1
            n.f32_changed = False
        vals32 = vr.round32(n.vals)
        serial = which != "warp_f32"
        check = serial or in_exact_range(vals32)
        self.skips["product_f32 draws"] += 1
        if not check:
            self.skips["product_f32 skipped"] += 1
        return self._log("product_f32", text, node=n.id, which=which, X=X, user=user, vals32=vals32, check=check)

    # ------------------------------------------------------------------------------------- sweep plans and apply modes
    def _prepare(self, n, width):
        """spmvHipTriSweepsPrepare's rule: width 0 is one column; a larger width than the plan's widens it, a smaller is a no-op"""
        width = max(int(width), 1)
        if n.plan is None:
            n.plan = dict(width=width, prepares=1)
        elif width > n.plan["width"]:
            n.plan = dict(width=width, prepares=n.plan["prepares"] + 1)
            self.stats["plan widened"] += 1

    def _sweep_nodes(self):
        return [c for c in self.live(one_diagonal=True) if c.kind != "fsai"]

    def op_sweeps_prepare(self):
        n = self.pick(self._sweep_nodes(), 0.8)
        width = int(self.rng.choice(WIDTHS))
        self._prepare(n, width)
        return self._log("sweeps_prepare", f"prepare_triangular_sweeps({n.label}, {width})", node=n.id, width=width)

    def op_sweeps_apply(self):
        rng = self.rng
        cand = self._sweep_nodes()
        fact = [c for c in cand if c.factored]
        rare = [c for c in cand if c.derived and not self.stats[f"refresh {c.kind}: plan in SWEEPS mode"]]      # a kind not yet refreshed in SWEEPS mode
        n = self.pick(rare if rare and rng.random() < 0.6 else fact if fact and rng.random() < 0.6 else cand, 0.85)
        r = rng.random()
        width = int(rng.choice([0, 0, 3, 16]))
        if r < 0.2:
            sweeps = None
            n.apply = ("exact",)
        else:
            a = int(rng.choice(SWEEPS + (3,)))
            b = a if r < 0.7 else int(rng.choice(SWEEPS + (3,)))
            sweeps = a if r < 0.7 else (a, b)
            self._prepare(n, width)
            n.apply = ("sweeps", a, b)
        self.stats["set_triangular_apply " + n.apply[0]] += 1
        return self._log("sweeps_apply", f"set_triangular_apply({n.label}, sweeps={sweeps}, block_width={width})", node=n.id, sweeps=sweeps, width=width)

    def op_sweeps_solve(self):
        rng = self.rng
        cand = self._sweep_nodes()
        planned = [c for c in cand if c.plan is not None]
        n = self.pick(planned if planned and rng.random() < 0.6 else cand, 0.85)
        lower, unit = bool(rng.integers(2)), bool(rng.integers(2))
        k = int(rng.choice([0, 0, 1, 3, 16]))
        B = rng.uniform(-1.0, 1.0, (n.M, max(k, 1)))
        top = int(levels(n.M, n.IRP.astype(np.int64), n.JA.astype(np.int64), lower).max())      # levels - 1
        S = (SWEEPS + ((top, top) if top <= MAX_SWEEPS else ()))[int(rng.integers(len(SWEEPS) + 2 * (top <= MAX_SWEEPS)))]
        call = f"solve_triangular(sweeps={S})" if k == 0 else f"solve_triangular_block(k={k}, sweeps={S})"
        text = f"{call}({n.label}, lower={int(lower)}, unit_diagonal={int(unit)})"
        if n.plan is not None and k > n.plan["width"]:       # refused: k above the prepared width
            self.stats["sweep solve refused"] += 1
            return self._log("sweeps_solve", text + f" refused: the plan holds {n.plan['width']} columns", node=n.id, lower=lower, unit=unit, k=k, S=S,
                             B=B, want=None, exact=False, check=True)
        self.skips["sweeps_solve draws"] += 1
        check = bool(np.isfinite(n.vals).all())
        want = None
        if check:                                            # (a skipped solve is not run: it prepares nothing either)
            self._prepare(n, max(k, 1) if n.plan is None else 0)
            with np.errstate(all="ignore"):
                want = sw.sweeps_block(n.M, n.IRP, n.JA, n.vals, B, S, lower, unit)
                if S == top:                                 # the header's consequence 4: the exact solve's bits
                    exact = np.stack([trsv_levels(n.M, n.IRP, n.JA, n.vals, B[:, c], lower=lower, unit=unit) for c in range(B.shape[1])], axis=1)
                    nan = np.isnan(exact)
                    assert np.array_equal(np.isnan(want), nan) and same_bits(np.where(nan, 0.0, want), np.where(nan, 0.0, exact)), self.where()
                    self.stats["sweep solve at levels - 1"] += 1
        else:
            self.skips["sweeps_solve skipped"] += 1
        return self._log("sweeps_solve", text + ("" if check else " skipped: a non-finite value"), node=n.id, lower=lower, unit=unit, k=k, S=S, B=B,
                         want=want, exact=S == top, check=check)

    def op_ilu0(self):
        """as derived_model's, but mostly on a node whose apply mode is SWEEPS when there is one: the mode must survive it"""
        cand = [c for c in self.live(derived=True, ilu_ok=True) if c.kind != "fsai"]
        with np.errstate(all="ignore"):
            sound = [c for c in cand if np.isfinite(c.vals).all() and np.isfinite(ilu0_levels(c.M, c.IRP, c.JA, c.vals)).all()]
        if not sound and self.rng.random() < 0.8:
            return None
        sweeping = [c for c in sound if c.apply[0] == "sweeps"]
        n = self.pick(sweeping if sweeping and self.rng.random() < 0.6 else sound if sound and self.rng.random() < 0.97 else cand)
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

    # ------------------------------------------------------------------------------------------ approximate inverses
    def op_fsai(self):
        """a factor G of a pool node as a node of its own (never written into directly: the header defines nothing for that),
        or the storage of a live one switched"""
        rng = self.rng
        mine = self.live(kind="fsai")
        if mine and (len(mine) >= 2 or len(self.live()) >= dm.MAX_LIVE or rng.random() < 0.55):
            n = self.pick(mine)
            storage = ("f32", "f64")[n.storage == "f32"] if rng.random() < 0.85 else n.storage
            if storage == "f32" and n.f32 is None:           # the form on G (and on G^T) is built, as by values_f32
                n.f32, n.f32_changed = dict(refreshes=0), False
            elif storage == "f64":
                n.f32 = None
            self.stats[f"fsai set_storage {storage}"] += 1
            n.storage = storage
            return self._log("fsai", f"{n.label}.set_storage({storage})", node=n.id, action="set_storage", storage=storage)
        if len(self.live()) >= dm.MAX_LIVE:
            return None
        cand = [c for c in self.live(ilu_ok=True) if c.kind != "fsai" and np.isfinite(c.vals).all()]
        spd = [c for c in cand if self.is_spd(c)]
        x = self.pick(spd if spd and rng.random() < 0.75 else cand, 0.5)
        if x is None:
            return None
        bands = [f for f in self.live(kind="filter") if (f.M, f.N) == (x.M, x.N) and f.params["mode"] == dm.fr.BAND and f.id != x.id]
        pat = self.pick(bands) if bands and rng.random() < 0.5 else None
        for S in ((pat,) if pat is not None else ()) + (None,):
            IRPg, _ = fsai_ref.pattern(x.M, (S or x).IRP, (S or x).JA)
            if int(np.diff(IRPg).max()) <= fsai_ref.MAX_ROW:
                break
        else:
            return None                                      # (a row above SPMV_FSAI_MAX_ROW: the library refuses the pattern)
        with np.errstate(all="ignore"):
            G, aux = dm.build_node("fsai", {}, [x.mat] + ([S.mat] if S is not None else []))
            info = fsai_ref.fsai_loop(x.mat, aux)[1]
        if not (self.is_spd(x) or info["badRows"] < x.M):
            return None
        label = f"n{self._id}"
        n = self._add("fsai", (x.id,), dict(pattern=None if S is None else S.label), G, aux, label)
        n.storage, n.setups, n.fsai_info = "f64", 1, info
        self.stats["derive fsai"] += 1
        text = f"{label} = fsai({x.label}, pattern={'its own' if S is None else S.label}): {G[3].size} entries, {info['badRows']} bad rows"
        return self._log("fsai", text, node=n.id, action="setup", src=x.id, pattern=None if S is None else S.id)

    # ------------------------------------------------------------------------------------------------ eigenpairs
    def op_eigsh(self):
        """the two smallest eigenpairs of an SPD node by Lanczos or Davidson; Davidson also with a live hierarchy of the node
        (Jacobi or Chebyshev smoother) or a live fsai node of its size as M^-1"""
        rng = self.rng
        spd = [c for c in self.live() if c.kind != "fsai" and np.isfinite(c.vals).all() and self.is_spd(c)]
        n = self.pick(spd, 0.5)
        if n is None:
            return None
        method = ("lanczos", "davidson", "davidson")[int(rng.integers(3))]
        ncv, maxiter = int(rng.choice([6, 10])), int(rng.choice([8, 30]))
        v0 = rng.standard_normal(n.M)
        pre, apply, what = None, None, None
        if method == "davidson" and rng.random() < 0.65:
            hs = [H for H in self.hiers if H.alive and H.src == n.id and (H.uid, H.version) == (n.uid, n.version) and H.sm["kind"] != dm.ags.GAUSS_SEIDEL]
            gs = [g for g in self.live(kind="fsai") if g.M == n.M and np.isfinite(g.vals).all()]
            if hs and (not gs or rng.random() < 0.5):
                H = hs[int(rng.integers(len(hs)))]
                pre, apply, what = ("hier", H.id), H.cycle, f"{H.label} ({H.storage})"
            elif gs:
                g = self.pick(gs)
                G = g.mat[:4] + (vr.round32(g.vals) if g.storage == "f32" else g.vals,)
                pre, apply, what = ("node", g.id), fsai_ref.Applied(G), f"{g.label} (fsai, {g.storage})"
        A = Csr(n.M, n.IRP, n.JA, n.vals)
        with np.errstate(all="ignore"):
            if method == "lanczos":
                want = lanczos_ref(A, v0, 2, ncv, SMALLEST, 1e-8, maxiter)
            else:
                counts = {}
                want = davidson_ref(A, v0, 2, ncv, SMALLEST, 1e-8, maxiter, 0, apply, None, counts)
                if pre is not None and pre[0] == "node" and counts["applies"]:
                    self._applied(self.nodes[pre[1]])
        n.selected[1] = True                                 # the solvers' SpMV is the serial-order launcher
        self.skips["eigsh draws"] += 1
        check = bool(np.isfinite(want[0]).all() and np.isfinite(want[2]).all())
        if not check:
            self.skips["eigsh skipped"] += 1
        self.stats[f"eigsh {method} " + ("with" if pre else "without") + " a preconditioner"] += 1
        text = f"eigsh({n.label}, k=2, SA, {method}, ncv={ncv}, maxiter={maxiter}, precond={what}): status {want[3]}, {want[4]} found after {want[5]}"
        return self._log("eigsh", text, node=n.id, method=method, ncv=ncv, maxiter=maxiter, v0=v0, pre=pre, want=want, check=check)

    # --------------------------------------------------------------------------------------------------- Krylov
    def op_krylov(self):
        rng = self.rng
        cand = [c for c in self.live(ilu_ok=True) if np.isfinite(c.vals).all()]
        spd = [c for c in cand if self.is_spd(c)]
        n = self.pick(spd if spd and rng.random() < 0.8 else cand)
        if n is None:
            return None
        method = ("cg", "bicgstab", "gmres")[int(rng.integers(3))]
        k = 3 if method != "gmres" and rng.random() < 0.35 else 0
        maxiter = int(rng.choice([2, 5, 12, 30]))
        tol = float(rng.choice([1e-3, 1e-8]))
        restart = int(rng.choice([4, 10])) if method == "gmres" else None
        B = rng.uniform(-1.0, 1.0, (n.M, max(k, 1)))
        pooled = [p for p in self.live(factored=True) if p.id != n.id and p.M == n.M and np.isfinite(p.vals).all() and (p.vals[p.dpos] != 0.0).all()]
        choice = ("none", "copy", "pooled", "pooled", "pooled", "fsai", "fsai")[int(rng.integers(7))]
        factors = [g for g in self.live(kind="fsai") if g.M == n.M and g.id != n.id and np.isfinite(g.vals).all()]
        if choice == "fsai" and not factors:
            choice = "pooled"
        if choice == "pooled" and not pooled:                # no factored node to take: one is made instead, for the next solve
            rec = self.op_ilu0()
            if rec is not None:
                return rec
            choice = "copy"
        F = P = None
        if choice == "copy":
            F = ilu0_levels(n.M, n.IRP, n.JA, n.vals)
            F = F if np.isfinite(F).all() and (F[n.dpos] != 0.0).all() else None
            A, pre = Csr(n.M, n.IRP, n.JA, n.vals, F), "a factored copy" if F is not None else None
        elif choice == "pooled":
            sweeping = [p for p in pooled if p.apply[0] == "sweeps"]
            P = self.pick(sweeping if sweeping and rng.random() < 0.6 else pooled)
            A, pre = Pooled(n, P), f"{P.label} ({' '.join(str(a) for a in P.apply)})"
        elif choice == "fsai":
            single = [g for g in factors if g.storage == "f32"]
            P = self.pick(single if single and rng.random() < 0.6 else factors)
            G = P.mat[:4] + (vr.round32(P.vals) if P.storage == "f32" else P.vals,)
            A, pre = fsai_ref.PrecondCsr(n.mat, G), f"{P.label} (fsai, {P.storage})"
        else:
            A, pre = Csr(n.M, n.IRP, n.JA, n.vals), None
        name = method + ("_block" if k else "")
        text = f"{name}({n.label}, precond={pre}, tol={tol}, maxiter={maxiter}" + (f", k={k}" if k else "") + (f", restart={restart}" if restart else "")
        if k and P is not None and P.kind != "fsai" and P.apply[0] == "sweeps" and P.plan["width"] < k:
            self.stats["krylov block refused"] += 1
            return self._log("krylov", text + f"): refused, {P.label}'s plan holds {P.plan['width']} columns", node=n.id, method=method, k=k,
                             maxiter=maxiter, tol=tol, restart=restart, B=B, F=F, pre=P.id, pre_state=self.state_of(P), want=None, check=True)
        X0 = np.zeros_like(B)
        with np.errstate(all="ignore"):
            if k:
                cols, (status, its, _, _) = block_ref(method, A, B, X0, tol, maxiter)
                want = (np.stack([c.x for c in cols], axis=1), status, its, [(c.status, c.iterations) for c in cols])
            elif method == "gmres":
                want = gmres_ref(A, B[:, 0], X0[:, 0], tol, maxiter, restart)[:3]
            else:
                want = (cg_ref if method == "cg" else bicgstab_ref)(A, B[:, 0], X0[:, 0], tol, maxiter)[:3]
        if not k:                                            # the single solvers' SpMV is the serial-order launcher: its selection runs
            n.selected[1] = True                             # (a block solve multiplies by hipSpMMRowsCSR, which selects nothing)
        self.skips["krylov draws"] += 1
        check = bool(np.isfinite(want[0]).all())
        if not check:
            self.skips["krylov skipped"] += 1
        self.stats[f"krylov status {want[1]}"] += 1
        if P is not None and P.kind == "fsai":
            if not k:                                        # (a block solve applies G and G^T by hipSpMMRowsCSR, which selects nothing)
                self._applied(P)
            self.stats[f"krylov with a pooled fsai node, {P.storage}"] += 1
        elif P is not None:
            self.stats[f"krylov with a pooled factored node, {P.apply[0]}"] += 1
        if k:
            self.stats["krylov block"] += 1
        text += f"): status {want[1]} after {want[2]}" + ("" if check else " skipped: x is not finite")
        return self._log("krylov", text, node=n.id, method=method, k=k, maxiter=maxiter, tol=tol, restart=restart, B=B, F=F,
                         pre=None if P is None else P.id, pre_state=None if P is None else self.state_of(P), want=want, check=check)
