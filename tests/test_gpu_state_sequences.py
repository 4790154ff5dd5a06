"""Seeded operation sequences on derived device handles that carry the per-handle state of the later features, checked step
by step against a host model.

tests/test_gpu_derived_sequences.py runs histories of transposes, permutations, products, sums and filters through the one
value-update tail of the library; its model predates the single-precision value form, the sweep plans with their apply mode,
the COO assembly, the RCM orderings, FSAI factors, the storage of a hierarchy and the eigensolvers.  tests/state_model.py holds a second generator that takes every operation of the
first and adds those (tests/test_state_model.py runs the same traces without a GPU, checks what they cover and shows with
planted faults that they discriminate); this file executes each record on the device with the backend of its sibling
(tests/derived_device.py) and, on top of what that one checks:
  * Q, assembled from shuffled element triplets with a kept map, is the bits of coo_ref and the root of derived nodes;
    assemble_refresh is its value update; a permutation by RCM is rcm_ref's;
  * after EVERY step the node's values_f32_info() (built, unit, bytes, refreshes, inexact, overflowed, flushed,
    firstOverflow) and triangular_sweeps_info() (mode, sweep counts, width, prepares, applyLaunches, bytes, and diagPos and
    the workspace at the addresses they had) are the model's: through direct updates, every kind of refresh, ILU(0) in
    place, the unit transitions that create and free the f32 array, and the rebuilds of formats;
  * the f32 products (rows, warp per row, enqueued rows, matmul k = 1, 3, 16) are the serial loop on the roundings bit for
    bit (the warp kernel by exact_ref.check_any_order and tight_error <= 1e-13 on the roundings); without the form they are
    refused and leave a poisoned y alone; with it every f64 check of the sibling still holds;
  * sweep solves (single and block, S in 0, 1, 2, 5, levels - 1) are sweeps_ref's bits, at levels - 1 also the exact solve's;
    a block wider than the plan is refused;
  * cg / bicgstab / gmres and the block forms (k = 3) with a LIVE factored node of the pool as the preconditioner, applied in
    the mode in force on it -- exact solves or its sweep counts --, have x, status and iteration count of the reference
    loops, and in SWEEPS mode the launch counters of tests/test_gpu_solver_counters.py's rule;
  * an `fsai` node is the bits of fsai_ref.fsai_loop on its own pattern or a band filter's, with badRows / firstBadRow, nnz,
    maxRow and setups of the reference; it is refreshed by Fsai.refresh_from, also while its source is stale, switched
    between F64 and F32 storage (the form on G then part of its modelled f32 state), never written into; after every step
    on it the owned G^T is downloaded and is the transpose of the G it holds, and the public transpose of the node equals
    Fsai.transposed(); as `precond` of the single and block solvers it is fsai_ref.PrecondCsr with G rounded through float in
    F32 storage;
  * hierarchy set_storage("f32" | "f64"): every cycle that follows a step, single and block, is the amg_*_ref cycle on
    values_f32_ref.rounded_levels; refresh_from keeps the storage; set_gauss_seidel on an F32 hierarchy and F32 on a
    Gauss-Seidel hierarchy are refused and leave the cycle's bits alone; storage_info() (storage, levels, f32_bytes zero in
    F64 and nonzero in F32) is compared after every step, and the form the call builds on the source node -- and releases
    again only if it built it -- is part of that node's state;
  * eigsh(k=2, "SA") by Lanczos and by Davidson, the latter also with a live hierarchy or a live fsai node as M^-1: theta, the
    residual norms, X, status, found and iterations of lanczos_ref / davidson_ref;
  * at the end of a seed every handle is freed and the allocation ledger (alloc_stats: live, liveBytes) is exactly where it
    was before the first upload.
A step whose result the model marks as unspecified is skipped (tests/test_state_model.py caps them); an unexpected refusal
is a failure.  Every failure names the seed and the whole trace up to the failing step; one seed runs alone by its id
(tests/test_gpu_state_sequences.py::test_state_sequence[107]).

40 seeds of 50 operations each, plus the uploads, a final cycle of every live hierarchy and a final serial-order product on
every live node; measured on one MI355X: 19 s for the module, 12 s of them the first test's start of the runtime, no seed
above 0.6 s (2 554 operations; 459 checked f64 products, 98 f32 products, 247 triangular solves, 65 sweep solves, 76 Krylov
solves, 67 eigsh solves, 272 cycles, 1 743 downloads of a node's arrays, 726 checks of a live sweep plan, 255 checks of a
factor with its owned transpose)."""
import ctypes as C

import numpy as np
import pytest

import derived_model as dm
import fsai_ref
import state_model as sm
import values_f32_ref as vr
from conftest import tight_error
from derived_device import TIGHT, Device, api, stream, torch  # noqa: F401  (the fixtures)
from exact_ref import check_any_order
from test_gpu_solver_counters import block_rule, single_rule

pytestmark = pytest.mark.gpu
CHECK_EVERY = 16                       # iterations between the host checks of a solve (the library's default)


class StateDevice(Device):
    """derived_device.Device plus the new sources, node kinds, operations and the state check after every step"""

    def __init__(self, *a):
        super().__init__(*a)
        self.addr = {}                  # node id -> (prepares, diagPos, workspace) of its sweep plan when last seen
        self.counts.update(f32_products=0, sweep_solves=0, states=0, eigsh=0, fsai=0)

    def same32(self, got, want, what):
        try:
            vr.same(got, want, what)
        except AssertionError as e:
            self.fail(e)

    # --------------------------------------------------------------------------------------------------- the state
    def execute(self, rec):
        super().execute(rec)
        if "state" in rec:
            try:
                self.check_state(self.node(rec), rec["state"])
            except AssertionError as e:
                if "-- seed" in str(e):
                    raise
                self.fail(e)

    def check_state(self, n, want):
        d = self.h[n.id]
        info = d.values_f32_info()
        got = None
        if info.built:
            got = dict(built=1, unit=info.unit, bytes=info.bytes, refreshes=info.refreshes,
                       counts=(info.inexact, info.overflowed, info.flushed, info.firstOverflow))
        else:
            assert (info.bytes, info.refreshes) == (0, 0), f"{n.label}: values_f32_info without a form: bytes {info.bytes}, refreshes {info.refreshes}"
        assert got == want["f32"], f"{n.label}: values_f32_info {got}, model {want['f32']}"
        if not n.square:
            return
        if want["fsai"] is not None:
            self.check_fsai(n, want["fsai"])
        p = d.triangular_sweeps_info()
        if want["plan"] is None:
            assert (p.width, p.prepares, p.bytes, p.diagPos, p.workspace, p.mode) == (0, 0, 0, None, None, 0), f"{n.label}: a sweep plan the model has not"
            return
        got = dict(width=p.width, prepares=p.prepares, bytes=p.bytes)
        assert got == want["plan"], f"{n.label}: triangular_sweeps_info {got}, model {want['plan']}"
        mode = ("sweeps", p.lowerSweeps, p.upperSweeps) if p.mode == self.api.SPMV_TRI_APPLY_SWEEPS else ("exact",)
        assert (mode, p.applyLaunches) == (want["apply"], want["applyLaunches"]), \
            f"{n.label}: apply mode {mode} with {p.applyLaunches} launches, model {want['apply']} with {want['applyLaunches']}"
        seen = self.addr.get(n.id)
        assert p.diagPos and p.workspace, f"{n.label}: the plan has no arrays"
        if seen is not None:
            assert p.diagPos == seen[1], f"{n.label}: diagPos moved"
            if seen[0] == p.prepares:
                assert p.workspace == seen[2], f"{n.label}: the workspace moved without a widening"
        self.addr[n.id] = (p.prepares, p.diagPos, p.workspace)
        self.counts["states"] += 1

    def check_fsai(self, n, want):
        """the factor's storage and counters, and its owned transpose: the transpose of the G it holds now, bit for bit"""
        d = self.h[n.id]
        info = d.info()
        ref = n.fsai_info
        got = (d.storage, info.setups, info.nnz, info.maxRow, info.badRows, info.firstBadRow)
        model = (want["storage"], want["setups"], ref["nnz"], ref["maxRow"], ref["badRows"], ref["firstBadRow"])
        assert got == model, f"{n.label}: storage, setups, nnz, maxRow, badRows, firstBadRow {got}, model {model}"
        M, N, IRP, JA, AS = d.transposed()
        T = fsai_ref.transposed(n.mat)
        assert (M, N) == T[:2] and np.array_equal(IRP, T[2]) and np.array_equal(JA, T[3]), f"{n.label}: the pattern of the owned G^T"
        self.same(AS, T[4], f"{n.label}: the owned G^T")
        self.counts["fsai"] += 1

    # ----------------------------------------------------------------------------------------------- sources and kinds
    def do_fsai(self, rec, n):
        if rec["action"] == "setup":
            pat = rec["pattern"]
            self.h[n.id] = self.h[rec["src"]].fsai(pattern=None if pat is None else self.h[pat])
        else:
            self.h[n.id].set_storage(rec["storage"])
        self.check_node(n)

    def do_hierarchy(self, rec, n):
        act = rec["action"]
        if act == "set_storage" or rec.get("refused"):
            h = self.hh[rec["hier"]]
            try:
                if act == "set_storage":
                    h.set_storage(rec["args"]["storage"])
                else:
                    getattr(h, act)(**rec["args"])
            except self.api.SpmvHipError:
                assert rec.get("refused"), f"{rec['text']}: refused"
            else:
                assert not rec.get("refused"), f"{rec['text']}: the call was taken"
            rec = dict(rec, action="cycle")                  # what is left for the sibling's backend: the cycles of the step
        super().do_hierarchy(rec, n)
        if "hstate" in rec and rec["hier"] in self.hh:
            got, want = self.hh[rec["hier"]].storage_info(), rec["hstate"]
            assert (got["storage"], got["levels"], got["f32_bytes"] > 0) == (want["storage"], want["levels"], want["storage"] == "f32"), \
                f"{rec['text']}: storage_info {got}, model {want}"

    def _refresh(self, n, use, params):
        if n.kind != "fsai":
            return super()._refresh(n, use, params)
        self.h[n.id].refresh_from(self.h[use[0]])

    def do_upload(self, rec, n):
        if n.label != "Q":
            return super().do_upload(rec, n)
        rows, cols, _, _ = sm.q_triplets()
        d = self.api.assemble_coo(n.M, n.N, rows, cols, self.gen.q, duplicates=self.gen.q_mode, keep_map=True)
        self.h[n.id] = d
        info = d.assemble_info()
        assert (info.nEntries, info.nnzC) == (rows.size, n.JA.size), f"Q: {info.nEntries} triplets, {info.nnzC} entries"
        self.check_node(n)

    def do_free(self, rec, n):
        super().do_free(rec, n)
        self.addr.pop(n.id, None)

    def do_set_values(self, rec, n):
        if "triplets" not in rec:
            return super().do_set_values(rec, n)
        v = rec["triplets"]
        self.h[n.id].assemble_refresh(v if rec["how"] == "host" else self.tensor(v.copy()))
        self.check_node(n, updated=True)

    def do_derive(self, rec, n):
        p = rec["params"]
        if rec["kind"] != "permute" or p["order"] != "rcm":
            super().do_derive(rec, n)
            if rec["kind"] == "transpose" and self.gen.nodes[rec["srcs"][0]].kind == "fsai":     # the public transpose of a factor: its owned G^T
                M, N, IRP, JA, AS = self.h[rec["srcs"][0]].transposed()
                assert np.array_equal(IRP, n.IRP) and np.array_equal(JA, n.JA), f"{n.label}: Fsai.transposed() has another pattern"
                self.same(AS, n.vals, f"{n.label}: Fsai.transposed()")
            return
        src = self.h[rec["srcs"][0]]
        o = src.rcm(start=p["start"], max_passes=p["max_passes"], forward=p["forward"])
        try:
            want = dm.permutation(self.gen.nodes[rec["srcs"][0]].mat, p)
            assert np.array_equal(o.perm.down(np.uint32), want), f"rcm({p}): the permutation differs from rcm_ref"
            self.h[n.id] = src.permute(o)
        finally:
            o.free()
        self.check_node(n)

    # --------------------------------------------------------------------------------------------------- the f32 form
    def do_values_f32(self, rec, n):
        self.h[n.id].values_f32(rec["on"])
        self.check_node(n)                                   # the doubles, the unit flag and both selections as they were

    def do_product_f32(self, rec, n):
        api, d, which, X, what = self.api, self.h[n.id], rec["which"], rec["X"], rec["text"]
        H = C.byref(d.handle)
        st = self.user_stream if rec["user"] else None
        want32 = rec["vals32"]
        if which == "matmul_f32":
            try:
                Y = d.matmul(np.ascontiguousarray(X), values="f32")
            except api.SpmvHipError:
                assert want32 is None, f"{what}: refused"
                return
            assert want32 is not None, f"{what}: taken without the form"
            for c in range(X.shape[1]):
                self.same32(Y[:, c], self.oracle.csr_serial(n.IRP, n.JA, want32, X[:, c].copy()), f"{what} column {c}")
            self.counts["f32_products"] += 1
            return
        x = X[:, 0].copy()
        dx, dy = api.DeviceVector(x.size).up(x), api.DeviceVector(n.M)
        try:
            dy.poison()
            api.lib.spmvHipDeviceSynchronize()
            if which == "enq_rows_f32":
                rc = api.lib.spmvHipEnqueueRowsF32(H, dx.ptr, dy.ptr, st)
            else:
                rc = api.SPMV_LAUNCHERS["hipSpMVRowsCSRf32" if which == "rows_f32" else "hipSpMVWarpPerRowCSRf32"](H, dx.ptr, api.CONFIG(), dy.ptr)
            assert api.lib.spmvHipDeviceSynchronize() == 0
            y = dy.down()
        finally:
            dx.free()
            dy.free()
        if want32 is None:
            assert rc not in (0, None), f"{what}: taken without the form"
            assert np.isnan(y).all(), f"{what}: the refused call wrote y"
            return
        assert rc in (0, None), f"{what}: launch failed ({rc})"
        if not rec["check"]:
            return
        self.counts["f32_products"] += 1
        want = self.oracle.csr_serial(n.IRP, n.JA, want32, x)
        if which != "warp_f32":
            return self.same32(y, want, what)
        assert not np.isnan(y).any(), f"{what}: NaN (poison survived?)"
        check_any_order(n.IRP, n.JA, want32, x, y, what)
        t = tight_error(n.IRP, n.JA, want32, x, want, y)
        assert t <= TIGHT, f"{what}: tight_error {t:.3e} > {TIGHT}"

    # ------------------------------------------------------------------------------------------- sweep plans and modes
    def do_sweeps_prepare(self, rec, n):
        self.h[n.id].prepare_triangular_sweeps(rec["width"])

    def do_sweeps_apply(self, rec, n):
        self.h[n.id].set_triangular_apply(rec["sweeps"], block_width=rec["width"])

    def do_sweeps_solve(self, rec, n):
        d, B, k, S, what = self.h[n.id], rec["B"], rec["k"], rec["S"], rec["text"]
        if not rec["check"]:
            return
        kw = dict(lower=rec["lower"], unit_diagonal=rec["unit"])
        if rec["want"] is None:                              # k above the prepared width
            try:
                d.solve_triangular_block(B, sweeps=S, **kw)
            except self.api.SpmvHipError:
                return
            self.fail(f"{what}: the solve was taken")
        if k == 0:
            got = d.solve_triangular(B[:, 0].copy(), sweeps=S, **kw)[:, None]
            exact = d.solve_triangular(B[:, 0].copy(), **kw)[:, None] if rec["exact"] else None
        else:
            got = d.solve_triangular_block(B, sweeps=S, **kw)
            exact = d.solve_triangular_block(B, **kw) if rec["exact"] else None
        for c in range(B.shape[1]):
            self.same(got[:, c], rec["want"][:, c], f"{what} column {c}")
            if exact is not None:
                self.same(exact[:, c], rec["want"][:, c], f"{what} column {c}: the exact solve")
        self.counts["sweep_solves"] += 1

    # --------------------------------------------------------------------------------------------------- eigenpairs
    def do_eigsh(self, rec, n):
        pre, what = rec["pre"], rec["text"]
        dM = None if pre is None else self.hh[pre[1]] if pre[0] == "hier" else self.h[pre[1]]
        theta, X, info = self.h[n.id].eigsh(k=2, which="SA", ncv=rec["ncv"], v0=rec["v0"], tol=1e-8, maxiter=rec["maxiter"], method=rec["method"], precond=dM)
        wtheta, wres, wX, status, found, its = rec["want"][:6]
        assert (info.status, info.found, info.iterations) == (status, found, its), f"{what}: status {info.status}, {info.found} found after {info.iterations}"
        if rec["check"]:
            self.same(theta, wtheta, f"{what}: theta")
            self.same(info.res, wres, f"{what}: the residual norms")
            for c in range(found):
                self.same(X[:, c], wX[:, c], f"{what}: X[:, {c}]")
            self.counts["eigsh"] += 1
        self.check_node(n)

    # ------------------------------------------------------------------------------------------------------- Krylov
    def do_krylov(self, rec, n):
        api, d, k, method, what = self.api, self.h[n.id], rec["k"], rec["method"], rec["text"]
        pre = own = None
        try:
            if rec["pre"] is not None:
                P = self.gen.nodes[rec["pre"]]
                pre = self.h[P.id]
                self.check_state(P, rec["pre_state"])
            elif rec["F"] is not None:
                pre = own = api.spMatCpyCSR(api.HostCSR(n.M, n.N, n.IRP, n.JA, n.vals))
                pre.ilu0()
                self.same(self.down(pre.handle.AS, n.JA.size, np.float64), rec["F"], "the factored copy")
            kw = dict(restart=rec["restart"]) if rec["restart"] else {}
            try:
                if k:
                    x, info = getattr(d, method + "_block")(rec["B"], precond=pre, tol=rec["tol"], maxiter=rec["maxiter"])
                else:
                    x, info = getattr(d, method)(rec["B"][:, 0].copy(), precond=pre, tol=rec["tol"], maxiter=rec["maxiter"], **kw)
            except api.SpmvHipError:
                if rec["want"] is None:                      # the preconditioner's plan is narrower than the block
                    return
                raise
            assert rec["want"] is not None, f"{what}: the solve was taken"
        finally:
            if own is not None:
                own.free()
        wx, wstatus, wit = rec["want"][:3]
        assert (info.status, info.iterations) == (wstatus, wit), f"{what}: status {info.status} after {info.iterations}"
        if k:
            got = [(c.status, c.iterations) for c in info.columns]
            assert got == rec["want"][3], f"{what}: the columns stopped at {got}"
        if rec["check"]:
            for c in range(rec["B"].shape[1]):
                self.same(x[:, c] if k else x, wx[:, c] if k else wx, f"{what}: x" + (f" column {c}" if k else ""))
            self.counts["krylov"] += 1
        st = rec["pre_state"]
        if st is not None and st["apply"][0] == "sweeps" and method != "gmres" and wit >= 1 and wstatus in (0, 1):
            rule = (block_rule if k else single_rule)(method, rec["maxiter"], CHECK_EVERY, wit, True, st["applyLaunches"])
            assert (info.launches, info.hostChecks) == rule, f"{what}: {info.launches} launches, {info.hostChecks} host checks; the rule: {rule}"
        self.check_node(n)
        if rec["pre"] is not None:                           # the preconditioner is what it was
            self.check_node(self.gen.nodes[rec["pre"]])
            self.check_state(self.gen.nodes[rec["pre"]], rec["pre_state"])


def _ledger_cold(api):
    """(live, liveBytes) of the allocation ledger with the library's own workspaces (product, dot, caches) given back, as
    tests/test_gpu_alloc_refusals.py does it: what is left belongs to handles"""
    api.lib.spmvHipDeviceSynchronize()
    api.spmvHipFinalize()
    api.spmvHipInit(0)
    st = api.alloc_stats()
    return int(st.live), int(st.liveBytes)


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_state_sequence(api, torch, oracle, stream, seed):
    torch.cuda.synchronize()
    before = _ledger_cold(api)
    gen = sm.Generator(seed)
    dev = StateDevice(api, torch, oracle, gen, stream)
    try:
        for rec in gen.run():
            dev.execute(rec)
        c = dev.counts
        print(f"seed {seed}: {len(gen.trace)} operations, {c['products']} checked products, {c['f32_products']} f32 products, {c['solves']} solves, "
              f"{c['sweep_solves']} sweep solves, {c['krylov']} Krylov solves, {c['eigsh']} eigsh solves, {c['cycles']} cycles, "
              f"{c['downloads']} node downloads, {c['states']} plan checks, {c['fsai']} factor checks")
    finally:
        api.lib.spmvHipDeviceSynchronize()
        for h in dev.hh.values():
            h.free()
        dev.hh.clear()
        for d in dev.h.values():
            d.free()
        dev.h.clear()
        dev.adopted.clear()
    after = _ledger_cold(api)
    assert after == before, f"seed {seed}: the allocation ledger (live, liveBytes) {after} after every free, {before} before the first upload"
