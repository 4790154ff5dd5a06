"""The host model of tests/test_gpu_state_sequences.py, run dry (no GPU): every seed of state_model.Generator against the
model alone, and against a host stand-in of the new per-handle state with planted faults.  It shows that the sequences test
what they claim:
  * the new sources and node kinds are the bits of the per-feature references (coo_ref, rcm_ref, values_f32_ref, sweeps_ref, fsai_ref, the amg cycle on rounded levels),
    and a chain done by the model is the same chain done by hand through them;
  * over all seeds together every new operation and every situation in which the new state can be lost occurs (conditions,
    not measurements: if a seed set misses one, the weights or the seeds change);
  * the steps the model marks as unspecified stay at most 10 % of their kind's draws;
  * a stand-in that keeps, per node, an f32 array, the apply mode, the plan's counters, a factor's G^T and storage, and per
    hierarchy its storage, passes every seed, and fails at
    least two seeds with any one of its faults switched on."""
import collections

import numpy as np
import pytest

import colour_ref as cr
import coo_ref as co
import derived_model as dm
import rcm_ref
import state_model as sm
import sweeps_inputs
import sweeps_ref as sw
import values_f32_ref as vr
from ilu0_ref import ilu0_levels
from krylov_ref import cg_ref
from sequence_inputs import unit_of


@pytest.fixture(scope="module")
def runs():
    """every seed run dry: (stats summed, skips summed, the generators, the records per seed)"""
    stats, skips, gens, recs = collections.Counter(), collections.Counter(), [], []
    for seed in sm.SEEDS:
        g = sm.Generator(seed)
        records = list(g.run())
        assert len(records) == len(g.trace) and all(r["text"] == t for r, t in zip(records, g.trace))
        depth = g.stats.pop("depth")
        stats.update(g.stats)
        stats["depth"] = max(stats["depth"], depth)
        skips.update(g.skips)
        gens.append(g)
        recs.append(records)
    return stats, skips, gens, recs


# ------------------------------------------------------------------------------------- agreement with the references
def _node(mat, label="X"):
    g = sm.Generator(0)
    return g, g._add("source", (), {"adopted": False}, mat, None, label)


@pytest.mark.parametrize("mode", ["sum", "last"])
def test_q_is_the_grid_operator_assembled_by_the_coo_reference_and_spd(mode):
    rows, cols, slot, w = sm.q_triplets()
    C, runs, vals = sm.q_source(mode)
    A = dm.sources()["A"]
    assert C[:2] == A[:2] and np.array_equal(C[2], A[2]) and np.array_equal(C[3], A[3]), "the pattern of the 23 x 19 five-point operator"
    lens = np.diff(runs[1])
    assert lens.min() == 1 and lens.max() == 4 and set(lens.tolist()) == {1, 2, 4}, "every stored entry: the sum of 1 to 4 triplets"
    assert not np.array_equal(np.lexsort((cols, rows)), np.arange(rows.size)), "a shuffled list"
    R, info, _ = co.assemble_ref(C[0], C[1], rows, cols, vals, mode)
    co.same_bits(C, R, "Q")
    g, n = _node(C, "Q")
    assert g.is_spd(n) and n.ilu_ok
    rng = np.random.default_rng(5200)
    for _ in range(3):                                       # and after a refresh with `uniform` triplet values
        g._set(n, co.refresh_ref(C, runs, sm.q_values(rng, "uniform"), mode)[4])
        assert g.is_spd(n)
    v = sm.q_values(rng, "wide")
    assert dm.same_bits(co.refresh_ref(C, runs, v, mode)[4], co.assemble_ref(C[0], C[1], rows, cols, v, mode)[0][4]), "a refresh is the assembly"


@pytest.mark.parametrize("mode", ["sum", "last"])
def test_an_assembled_node_on_the_q1_fixture_of_the_coo_test(mode):
    """tests/test_gpu_coo.py's element triplets (skip markers on the boundary, up to four duplicates an entry): a node made
    as Q is made, and its value update as the model does it, are the assembly of the new values"""
    from test_gpu_coo import _q1_triplets
    M, rows, cols, vals = _q1_triplets((5, 5))
    C, info, runs = co.assemble_ref(M, M, rows, cols, vals, mode)
    assert info["skipped"] > 0 and info["maxRun"] == 4
    g, n = _node(C, "Q")
    n.f32 = dict(refreshes=0)
    new = vals * np.random.default_rng(5207).uniform(0.5, 1.5, vals.size)
    g._set(n, co.refresh_ref(C, runs, new, mode)[4])
    co.same_bits(n.mat, co.assemble_ref(M, M, rows, cols, new, mode)[0], "the refreshed node")
    assert g.state_of(n)["f32"]["refreshes"] == 1 and g.state_of(n)["f32"]["counts"] == vr.counts(n.vals)


def test_the_sweep_solves_of_the_records_are_the_literal_loop(runs):
    """what op_sweeps_solve puts into a record, against sweeps_ref.sweeps_loop on the values the record carries"""
    done = 0
    for g, rs in zip(runs[2], runs[3]):
        for r in rs:
            if r["op"] == "sweeps_solve" and r["want"] is not None and r["S"] <= 2 and done < 6 and r["vals"].size < 4000:
                n = g.nodes[r["node"]]
                with np.errstate(all="ignore"):
                    ref = sw.sweeps_loop(n.M, n.IRP, n.JA, r["vals"], r["B"][:, 0], r["S"], r["lower"], r["unit"])
                nan = np.isnan(ref)
                assert np.array_equal(np.isnan(r["want"][:, 0]), nan) and dm.same_bits(np.where(nan, 0.0, r["want"][:, 0]), np.where(nan, 0.0, ref)), r["text"]
                done += 1
    assert done == 6


@pytest.mark.parametrize("name", ["random257", "laplacian12x10x8", "clique_star"])
@pytest.mark.parametrize("start, max_passes, forward", [("peripheral", 0, False), ("min_degree", 1, True), ("peripheral", 3, True)])
def test_rcm_permute_nodes_are_the_rcm_and_permutation_references(name, start, max_passes, forward):
    M, IRP, JA = cr.small_cases()[name]
    AS = np.random.default_rng(5201).uniform(-1, 1, JA.size)
    A = (M, M, IRP, JA, AS)
    p = dict(order="rcm", start=start, max_passes=max_passes, forward=forward)
    B, o = dm.build_node("permute", p, [A])
    perm, _ = rcm_ref.rcm_loop(M, IRP, JA, rcm_ref.PERIPHERAL if start == "peripheral" else rcm_ref.MIN_DEGREE, max_passes, forward)
    assert sorted(perm) == list(range(M))
    irp, ja, val, m = cr.permute_ref(M, IRP, JA, AS, np.asarray(perm, dtype=np.int64))
    assert np.array_equal(B[2], irp) and np.array_equal(B[3], ja) and dm.same_bits(B[4], val) and np.array_equal(o, m)
    assert dm.same_bits(dm.refresh_values("permute", p, o, [A[:4] + (-AS,)]), -val)


@pytest.mark.parametrize("name", ["random-300", "boundary", "empty-rows"])
def test_the_f32_state_of_a_node_is_the_values_f32_reference(name):
    M, N, IRP, JA, AS, x = vr.case(name)
    g, n = _node((M, N, IRP, JA, AS))
    assert g.state_of(n)["f32"] is None
    n.f32 = dict(refreshes=0)
    s = g.state_of(n)["f32"]
    assert (s["built"], s["unit"], s["refreshes"]) == (1, 0, 0) and s["bytes"] == (JA.size * 4 + 15) // 16 * 16 + 32 and s["counts"] == vr.counts(AS)
    g._set(n, np.full(JA.size, 0.1))                         # non-unit -> unit: the array goes, every entry inexact
    s = g.state_of(n)["f32"]
    assert (s["unit"], s["bytes"], s["refreshes"]) == (1, 0, 1) and s["counts"] == (JA.size, 0, 0, -1)
    g._set(n, AS)
    assert g.state_of(n)["f32"]["bytes"] == (JA.size * 4 + 15) // 16 * 16 + 32 and g.state_of(n)["f32"]["refreshes"] == 2
    assert g.stats["f32: non-unit -> unit"] == g.stats["f32: unit -> non-unit"] == 1


@pytest.mark.parametrize("name", ["r63", "r65", "pattern"])
def test_sweep_solves_of_the_model_are_the_literal_loop(name):
    M, IRP, JA, AS, b = sweeps_inputs.make(name)
    for lower in (True, False):
        counts, L = sweeps_inputs.sweep_counts(M, IRP, JA, lower)
        for S in counts[:4]:
            got = sw.sweeps_block(M, IRP, JA, AS, b[:, None], S, lower, False)[:, 0]
            assert dm.same_bits(got, sw.sweeps_loop(M, IRP, JA, AS, b, S, lower, False)), (name, lower, S)


def test_the_plan_and_the_apply_mode_of_the_model_follow_the_header():
    g, n = _node(dm.sources()["A"], "A")
    assert g.state_of(n)["plan"] is None and g.state_of(n)["applyLaunches"] == 0
    g._prepare(n, 0)
    assert n.plan == dict(width=1, prepares=1)
    g._prepare(n, 3), g._prepare(n, 1)                       # a larger width widens, a smaller is a no-op
    assert n.plan == dict(width=3, prepares=2) and g.state_of(n)["plan"]["bytes"] == 4 * n.M + 16 * n.M * 3
    for apply, c in ((("sweeps", 2, 2), 4), (("sweeps", 0, 3), 4), (("sweeps", 0, 0), 1), (("exact",), 0)):
        assert sm.apply_launches(apply) == c
    n.apply = ("sweeps", 2, 1)
    g._set(n, ilu0_levels(n.M, n.IRP, n.JA, n.vals), factored=True)
    assert n.apply == ("sweeps", 2, 1) and n.plan == dict(width=3, prepares=2), "a write keeps both"


def test_a_chain_by_the_model_is_the_chain_by_hand():
    """Q -> RCM permute (the operator o and the preconditioner p) -> ilu0(p) -> SWEEPS mode -> assemble_refresh -> both
    refreshed -> ilu0(p) -> cg(o, precond=p)"""
    g = sm.Generator(2)                                      # (an even seed: duplicates "sum")
    recs = g.run()
    for _ in range(4):
        next(recs)
    Q = g.nodes[3]
    assert Q.label == "Q"
    rows, cols, _, _ = sm.q_triplets()
    params = dict(order="rcm", start="peripheral", max_passes=0, forward=False)

    def permute():
        mat, aux = dm.build_node("permute", params, [Q.mat])
        return g._add("permute", [Q.id], params, mat, aux, f"n{g._id}")

    def refresh(n):
        g._set(n, dm.refresh_values(n.kind, n.params, n.aux, [Q.mat]))
        n.seen = ((Q.uid, Q.version),)

    o, p = permute(), permute()
    g._set(p, ilu0_levels(p.M, p.IRP, p.JA, p.vals), factored=True)
    g._prepare(p, 0)
    p.apply = ("sweeps", 2, 2)
    new = sm.q_values(np.random.default_rng(5202), "uniform")
    C, runs, _ = sm.q_source("sum")
    g._set(Q, co.refresh_ref(C, runs, new, "sum")[4])
    assert g.stale(o) and g.stale(p) and p.factored
    refresh(o), refresh(p)
    assert not p.factored and p.apply == ("sweeps", 2, 2) and p.plan == dict(width=1, prepares=1)
    g._set(p, ilu0_levels(p.M, p.IRP, p.JA, p.vals), factored=True)
    b = np.random.default_rng(5203).uniform(-1, 1, o.M)
    got = cg_ref(sm.Pooled(o, p), b, np.zeros(o.M), 1e-8, 30)
    # by hand
    M = Q.M
    A, _, _ = co.assemble_ref(M, M, rows, cols, new, "sum")
    perm, _ = rcm_ref.rcm_loop(M, A[2], A[3], rcm_ref.PERIPHERAL, 0, False)
    irp, ja, val, _ = cr.permute_ref(M, A[2], A[3], A[4], np.asarray(perm, dtype=np.int64))
    F = ilu0_levels(M, irp, ja, val)
    want = cg_ref(sw.SweepCsr(M, irp, ja, val, F, 2, 2), b, np.zeros(M), 1e-8, 30)
    assert dm.same_bits(got[0], want[0]) and got[1:3] == want[1:3] and got[2] > 2
    p.apply = ("exact",)
    from krylov_ref import Csr
    assert dm.same_bits(cg_ref(sm.Pooled(o, p), b, np.zeros(M), 1e-8, 30)[0], cg_ref(Csr(M, irp, ja, val, F), b, np.zeros(M), 1e-8, 30)[0])


# --------------------------------------------------------------------------------------------------------- coverage
def test_a_seed_gives_the_same_trace_twice():
    a, b = sm.Generator(sm.SEEDS[3]), sm.Generator(sm.SEEDS[3])
    ra, rb = list(a.run()), list(b.run())
    assert a.trace == b.trace and all(dm.same_bits(a.nodes[i].vals, b.nodes[i].vals) for i in a.nodes)
    assert [r.get("state") for r in ra] == [r.get("state") for r in rb]


def test_the_new_seeds_are_not_the_old_ones():
    assert len(sm.SEEDS) == 40 and not set(sm.SEEDS) & set(dm.SEEDS) and sm.STEPS == 50


def test_every_operation_kind_occurs(runs):
    stats = runs[0]
    for op, _ in sm.OPS:
        assert stats[op] >= 5, (op, stats[op])
    assert set(sm.NEW_OPS) <= {op for op, _ in sm.OPS} and {op for op, _ in dm.OPS} <= {op for op, _ in sm.OPS}
    for what in ("permute by rcm", "f32_edges", "assemble_refresh", "f32 product refused", "sweep solve at levels - 1", "krylov block",
                 "set_triangular_apply exact", "set_triangular_apply sweeps"):
        assert stats[what] >= 5, (what, stats[what])
    for which in sm.F32_PRODUCTS:
        assert sum(r["op"] == "product_f32" and r["which"] == which and r["vals32"] is not None for rs in runs[3] for r in rs) >= 5, which
    assert stats["plan widened"] >= 2 and stats["sweep solve refused"] >= 2


@pytest.mark.parametrize("what", ["f32 form built", "plan in SWEEPS mode"])
@pytest.mark.parametrize("kind", dm.DERIVED)
def test_every_derived_kind_is_refreshed_with_the_new_state(runs, kind, what):
    assert runs[0][f"refresh {kind}: {what}"] >= 1


def test_assemble_refresh_with_derived_nodes_below(runs):
    assert runs[0]["assemble_refresh with two or more derived nodes below"] >= 3
    assert runs[0]["assemble_refresh with the f32 form built"] >= 3


@pytest.mark.parametrize("what", ["non-unit -> unit", "unit -> unit of another value", "unit -> non-unit"])
def test_unit_transitions_on_a_node_with_an_f32_form(runs, what):
    assert runs[0]["f32: " + what] >= 1


def test_f32_products_after_the_values_changed(runs):
    assert runs[0]["f32 product after the values changed"] >= 5


@pytest.mark.parametrize("mode", ["exact", "sweeps"])
def test_krylov_solves_with_a_pooled_factored_node(runs, mode):
    assert runs[0][f"krylov with a pooled factored node, {mode}"] >= 2


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_krylov_solves_with_a_pooled_fsai_node(runs, storage):
    assert runs[0][f"krylov with a pooled fsai node, {storage}"] >= 2


def test_fsai_histories(runs):
    stats = runs[0]
    assert stats["derive fsai"] >= 5 and stats["fsai set_storage f32"] >= 2 and stats["fsai set_storage f64"] >= 2
    assert stats["refresh fsai: source stale"] >= 2 and stats["refresh fsai: F32 storage"] >= 2
    assert stats["an fsai node used as a source"] >= 3
    for g in runs[2]:                                        # no hierarchy stands on a factor (its set_storage would put a form on G)
        assert all(g.nodes[H.src].kind != "fsai" for H in g.hiers)
    for rs, g in zip(runs[3], runs[2]):                      # the generator never writes into a factor directly
        for r in rs:
            if r["op"] in ("update_derived", "ilu0", "values_f32", "sweeps_apply"):
                assert g.nodes[r["node"]].kind != "fsai", r["text"]


@pytest.mark.parametrize("lanes", [4])
def test_fsai_nodes_are_the_fsai_reference(lanes):
    """on a fixture of tests/test_gpu_fsai.py (random_spd) and its band pattern: the node, its refresh, the preconditioned cg"""
    import fsai_ref
    from test_fsai_abi import random_spd
    A = random_spd(np.random.default_rng(5204), 300, 4)
    S, _ = dm.build_node("filter", dm.fr.opts(dm.fr.BAND, -40, 0), [A])
    for pat in (None, S):
        G, aux = dm.build_node("fsai", {}, [A] + ([pat] if pat is not None else []))
        R, info = fsai_ref.fsai_loop(A, pat)
        assert info["badRows"] == 0 and dm.same_bits(G[4], R[4]) and np.array_equal(G[3], R[3]) and np.array_equal(G[2], R[2])
        assert dm.same_bits(G[4], fsai_ref.fsai_vec(A, pat)[0][4]), "the loop is the vectorised reference"
        B = A[:4] + (A[4] * 1.5,)
        assert dm.same_bits(dm.refresh_values("fsai", {}, aux, [B]), fsai_ref.fsai_loop(B, pat)[0][4])
    b = np.random.default_rng(5205).uniform(-1, 1, A[0])
    G32 = G[:4] + (vr.round32(G[4]),)
    x64, x32 = (cg_ref(fsai_ref.PrecondCsr(A, g), b, np.zeros(A[0]), 1e-8, 30) for g in (G, G32))
    assert x64[2] > 2 and not dm.same_bits(x64[0], x32[0]), "the two storages are told apart"


@pytest.mark.parametrize("what", ["set_storage f32", "set_storage f64", "refresh in F32", "F32 refused on Gauss-Seidel", "gauss_seidel refused in F32"])
def test_hierarchy_storage_histories(runs, what):
    """both directions and a refresh in F32 at least twice, each of the two mutual refusals at least once"""
    assert runs[0]["hierarchy " + what] >= (1 if "refused" in what else 2), runs[0]["hierarchy " + what]


def test_an_f32_hierarchy_of_the_model_is_the_cycle_on_the_rounded_levels():
    import amg_cheb_ref as acr
    g = sm.Generator(0)
    recs = g.run()
    next(recs)
    A = g.nodes[0]
    levels, o = g._levels("smoothed", dict(seed=3, coarseRows=40), A.mat)
    H = dm.Hier(0, A, "smoothed", dict(seed=3, coarseRows=40), levels, o)
    r = np.random.default_rng(5206).standard_normal(A.M)
    z64 = H.cycle(r)
    H.storage = "f32"
    z32 = H.cycle(r)
    assert dm.same_bits(z32, acr.cycle_ref(vr.rounded_levels(levels), o, r, H.sm)) and not dm.same_bits(z32, z64)
    H.storage = "f64"
    assert dm.same_bits(H.cycle(r), z64)


@pytest.mark.parametrize("method, pre", [("lanczos", "without"), ("davidson", "without"), ("davidson", "with")])
def test_eigsh_by_each_method(runs, method, pre):
    """(Lanczos takes no preconditioner)"""
    assert runs[0][f"eigsh {method} {pre} a preconditioner"] >= 2


def test_krylov_solves_stop_on_the_cap_and_before_it(runs):
    assert runs[0]["krylov status 0"] >= 1 and runs[0]["krylov status 1"] >= 1


def test_ilu0_on_a_node_in_sweeps_mode(runs):
    """(what the fault `apply mode reset by ilu0` needs)"""
    n = sum(r["op"] == "ilu0" and r["state"]["apply"][0] == "sweeps" for rs in runs[3] for r in rs)
    assert n >= 2, n


@pytest.mark.parametrize("kind", ["product", "product_f32", "solve", "ilu0 solve", "sweeps_solve", "krylov", "hierarchy", "eigsh"])
def test_skipped_steps_stay_below_a_tenth(runs, kind):
    skips = runs[1]
    assert skips[kind + " draws"] >= 5
    assert 10 * skips[kind + " skipped"] <= skips[kind + " draws"], (kind, skips[kind + " skipped"], skips[kind + " draws"])


def test_the_pool_stays_small(runs):
    for g in runs[2]:
        assert len(g.live()) <= dm.MAX_LIVE and max(n.JA.size for n in g.nodes.values()) <= dm.MAX_NNZ


# ----------------------------------------------------------------------------------------------------- planted faults
FAULTS = tuple(f"form not followed after a refresh of a {k}" for k in dm.DERIVED) + (
    "form not followed after assemble_refresh", "form kept across unit -> non-unit with the stale register value",
    "apply mode reset by ilu0", "apply mode reset by a refresh", "plan rebuilt on refresh", "refreshes not counted",
    "G^T not refreshed", "FSAI storage lost at refresh", "hierarchy storage lost at refresh")


class StandIn:
    """a host stand-in for the new state of the library alone: per node the doubles an f32 form was rounded from (so its
    array and what its info reports), the refresh count, the apply mode and the plan's counters, each updated when a record
    tells of the event -- by the library's rules, or, with `fault`, with one of them broken.  check() compares what it would
    answer with what the record expects and returns the first difference."""

    def __init__(self, gen, fault=None):
        self.gen, self.fault, self.s = gen, fault, {}
        self.h = {}                     # hierarchy id -> dict(storage, a0form)

    def _new(self, n, vals):
        self.s[n.id] = dict(unit=unit_of(vals), f32=None, plan=None, apply=("exact",), fsai=None, gt=None)
        if n.kind == "fsai":                                 # the factor after its setup: G^T made from these values
            self.s[n.id].update(fsai=dict(storage="f64", setups=1), gt=vals)

    def _round(self, st, vals):
        st["f32"]["src"] = np.array(vals, dtype=np.float64)

    def _write(self, n, vals, how):
        st = self.s[n.id]
        before, st["unit"] = st["unit"], unit_of(vals)
        f = st["f32"]
        if f is not None:
            lost = (self.fault == f"form not followed after a refresh of a {n.kind}" and how == "refresh") or \
                   (self.fault == "form not followed after assemble_refresh" and how == "assemble_refresh")
            if not lost:
                if self.fault == "form kept across unit -> non-unit with the stale register value" and before[0] and not st["unit"][0]:
                    self._round(st, np.full(n.JA.size, before[1]))
                else:
                    self._round(st, vals)
                f["refreshes"] += 0 if self.fault == "refreshes not counted" else 1
        if (self.fault == "apply mode reset by ilu0" and how == "ilu0") or (self.fault == "apply mode reset by a refresh" and how == "refresh"):
            st["apply"] = ("exact",)
        if self.fault == "plan rebuilt on refresh" and how == "refresh" and st["plan"] is not None:
            st["plan"]["prepares"] += 1
        if st["fsai"] is not None:                           # spmvHipFsaiRefresh: G^T takes G's new values, the storage stays
            st["fsai"]["setups"] += 1
            if self.fault != "G^T not refreshed":
                st["gt"] = vals
            if self.fault == "FSAI storage lost at refresh":
                st["fsai"]["storage"], st["f32"] = "f64", None

    def _prepare(self, st, width):
        width = max(int(width), 1)
        if st["plan"] is None:
            st["plan"] = dict(width=width, prepares=1)
        elif width > st["plan"]["width"]:
            st["plan"] = dict(width=width, prepares=st["plan"]["prepares"] + 1)

    def state(self, n):
        st = self.s[n.id]
        f32 = None
        if st["f32"] is not None:
            src = st["f32"]["src"]
            unit = unit_of(src)[0]
            f32 = dict(built=1, unit=int(unit), bytes=0 if unit else (4 * src.size + 15) // 16 * 16 + 32, refreshes=st["f32"]["refreshes"],
                       counts=vr.counts(src))
        plan = None if st["plan"] is None else dict(st["plan"], bytes=4 * n.M + 16 * n.M * st["plan"]["width"])
        return dict(f32=f32, plan=plan, apply=st["apply"], applyLaunches=sm.apply_launches(st["apply"]),
                    fsai=None if st["fsai"] is None else dict(st["fsai"]))

    def check(self, rec):
        op, n, vals = rec["op"], self.gen.nodes[rec["node"]], rec.get("vals")
        if op in ("upload", "reupload", "derive") or (op == "fsai" and rec["action"] == "setup"):
            self._new(n, vals)
        st = self.s[n.id]
        if op in ("set_values", "update_derived", "refresh", "ilu0"):
            self._write(n, vals, "assemble_refresh" if "triplets" in rec else op)
        elif op == "values_f32":
            if not rec["on"]:
                st["f32"] = None
            elif st["f32"] is None:
                st["f32"] = dict(refreshes=0)
                self._round(st, vals)
        elif op == "fsai" and rec["action"] == "set_storage":
            st["fsai"]["storage"] = rec["storage"]
            if rec["storage"] == "f64":
                st["f32"] = None
            elif st["f32"] is None:
                st["f32"] = dict(refreshes=0)
                self._round(st, vals)
        elif op == "hierarchy" and "hstate" in rec:
            h = self.h.setdefault(rec["hier"], dict(storage="f64", a0form=False))
            if rec["action"] == "refresh" and self.fault == "hierarchy storage lost at refresh":
                h["storage"] = "f64"
            if rec["action"] == "set_storage" and not rec.get("refused"):
                if rec["args"]["storage"] == "f32":
                    if st["f32"] is None:
                        st["f32"], h["a0form"] = dict(refreshes=0), True
                        self._round(st, vals)
                else:
                    if h["a0form"]:
                        st["f32"] = None
                    h["a0form"] = False
                h["storage"] = rec["args"]["storage"]
            if h["storage"] != rec["hstate"]["storage"]:
                return f"hierarchy {rec['hier']}: storage {h['storage']}, the model {rec['hstate']['storage']}"
        elif op == "sweeps_prepare":
            self._prepare(st, rec["width"])
        elif op == "sweeps_apply":
            if rec["sweeps"] is None:
                st["apply"] = ("exact",)
            else:
                self._prepare(st, rec["width"])
                lo, up = rec["sweeps"] if isinstance(rec["sweeps"], tuple) else (rec["sweeps"], rec["sweeps"])
                st["apply"] = ("sweeps", lo, up)
        elif op == "sweeps_solve" and st["plan"] is None and rec["check"]:
            self._prepare(st, max(rec["k"], 1))
        elif op == "product_f32":
            if (rec["vals32"] is None) != (st["f32"] is None):
                return "an f32 product taken or refused against the model"
            if rec["vals32"] is not None:
                got = vr.round32(st["f32"]["src"])
                nan = np.isnan(rec["vals32"])
                if not (np.array_equal(np.isnan(got), nan) and dm.same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, rec["vals32"]))):
                    return "the f32 array is not the rounding of the node's values"
        elif op == "krylov" and rec["pre"] is not None:
            P = self.gen.nodes[rec["pre"]]
            if self.state(P) != rec["pre_state"]:
                return f"the preconditioner's state {self.state(P)}, the model {rec['pre_state']}"
        if "state" in rec and st["gt"] is not None and not dm.same_bits(st["gt"], vals):
            return f"{n.label}: the owned G^T is not the transpose of the factor's values"
        if "state" in rec and self.state(n) != rec["state"]:
            return f"{n.label}: state {self.state(n)}, the model {rec['state']}"
        return None


def _first_failure(g, records, fault):
    """(step, why) of the first record the stand-in answers differently, or None (the records carry the values of their time)"""
    s = StandIn(g, fault)
    for step, rec in enumerate(records):
        why = s.check(rec)
        if why is not None:
            return step, why
    return None


def test_the_stand_in_passes_every_seed(runs):
    for g, records in zip(runs[2], runs[3]):
        bad = _first_failure(g, records, None)
        assert bad is None, f"seed {g.seed}, step {bad[0]} ({records[bad[0]]['text']}): {bad[1]}"


@pytest.mark.parametrize("fault", FAULTS)
def test_every_planted_fault_fails_at_least_two_seeds(runs, fault):
    bad = [g.seed for g, records in zip(runs[2], runs[3]) if _first_failure(g, records, fault) is not None]
    assert len(bad) >= 2, (fault, bad)
