"""The device backend of the seeded sequence tests (tests/test_gpu_derived_sequences.py, tests/test_gpu_state_sequences.py):
the fixtures both modules use and `Device`, which executes the records of derived_model.Generator on the device and compares
every step with the host model.  tests/test_gpu_derived_sequences.py states what is checked."""
import ctypes as C

import numpy as np
import pytest

import derived_model as dm
import filter_ref as fr
from bits import assert_same_bits
from conftest import tight_error
from exact_ref import check_any_order
from serial_order_inputs import stripes_order, tiles_order
from trsm_ref import trsm_levels
from trsv_ref import trsv_levels

TIGHT = 1e-13
MEM_TOL = 8 << 20                      # as tests/test_gpu_sequences.py: the runtime's pools wobble by 4 MiB pieces
SERIAL_NAMES = {b"hipSpMVRowsCSR", b"hipSpMVTilesCSR(deterministic)", b"hipSpMVStripesCSR(owner wavefronts)",
                b"hipSpMVStripesCSR(ordered tickets)"}
REDUCTION_NAMES = {b"hipSpMVWarpPerRowCSR", b"hipSpMVTilesCSR", b"hipSpMVStripesCSR"}


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture
def stream(api, torch):
    """a user stream of the test's own, destroyed afterwards; every process-wide switch back to its default"""
    api.lib.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    api.lib.hipStreamDestroy.argtypes = [C.c_void_p]
    s = C.c_void_p()
    assert api.lib.hipStreamCreate(C.byref(s)) == 0
    yield s
    api.lib.spmvHipDeviceSynchronize()
    api.set_variant("hipSpMVRowsCSR", 2)
    api.set_variant("hipSpMVWarpPerRowCSR", 2)
    api.lib.spmvHipSetUnitValues(1)
    api.lib.spmvHipSetStream(None)
    api.lib.spmvHipSetSync(1)
    api.lib.spmvHipSetEllRowLens(1)
    assert api.lib.hipStreamDestroy(s) == 0


class Device:
    """executes the generator's records on the device and compares with its model"""

    def __init__(self, api, torch, oracle, gen, stream):
        self.api, self.torch, self.oracle, self.gen, self.user_stream = api, torch, oracle, gen, stream
        self.h = {}                     # node id -> DeviceMatrix (a freed one stays: what a refused refresh is given)
        self.adopted = {}               # node id -> the caller-owned tensors of an adopted handle
        self.hh = {}                    # hierarchy id -> AmgHierarchy
        self.counts = dict(products=0, solves=0, krylov=0, cycles=0, downloads=0)

    # ------------------------------------------------------------------------------------------------------ helpers
    def fail(self, e):
        raise AssertionError(f"{e} -- {self.gen.where()}") from None

    def same(self, got, want, what):
        try:
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), f"{what}: NaN places differ"
            assert_same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what)
        except AssertionError as e:
            self.fail(e)

    def down(self, ptr, n, dtype):
        out = np.empty(n, dtype=dtype)
        if n:
            assert self.api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
        return out

    def check_node(self, n, updated=False):
        """the handle holds the model's arrays, unit flag and selections; after a value update also its update_info"""
        api, h = self.api, self.h[n.id].handle
        assert api.lib.spmvHipDeviceSynchronize() == 0
        if (int(h.M), int(h.N), int(h.NZ)) != (n.M, n.N, n.JA.size):
            self.fail(f"{n.label}: shape {(int(h.M), int(h.N), int(h.NZ))}, model {(n.M, n.N, n.JA.size)}")
        if n.derived:                                    # (a derived handle has 4-byte row pointers)
            if not np.array_equal(self.down(h.IRP, n.M + 1, np.uint32), n.IRP):
                self.fail(f"{n.label}: IRP differs from the model")
            if not np.array_equal(self.down(h.JA, n.JA.size, np.uint32), n.JA):
                self.fail(f"{n.label}: JA differs from the model")
        self.same(self.down(h.AS, n.JA.size, np.float64), n.vals, f"{n.label}: AS")
        self.counts["downloads"] += 1
        c = C.c_double(12345.0)
        got = api.lib.spmvHipUnitValue(C.byref(h), C.byref(c))
        if got != int(n.unit[0]) or (n.unit[0] and np.float64(c.value).tobytes() != np.float64(n.unit[1]).tobytes()):
            self.fail(f"{n.label}: spmvHipUnitValue {got} ({c.value!r}), model {n.unit}")
        if updated:
            info = self.h[n.id].update_info()
            got = dict(unitBefore=info.unitBefore, unitAfter=info.unitAfter, rebuilt=info.rebuilt, inPlace=info.inPlace)
            if got != n.last_update:
                self.fail(f"{n.label}: update_info {got}, model {n.last_update} (stripes layouts {n.stripes})")
        self.check_choices(n)

    def check_choices(self, n):
        for k, (fn, names) in enumerate(((self.api.lib.spmvHipAutoChoice, REDUCTION_NAMES), (self.api.lib.spmvHipAutoChoiceRows, SERIAL_NAMES))):
            name = fn(C.byref(self.h[n.id].handle), None)
            if n.selected[k] is None:                    # a multigrid cycle may have run it
                continue
            if n.selected[k] and name not in names:
                self.fail(f"{n.label}: selection {k} chose {name}")
            if not n.selected[k] and name is not None:
                self.fail(f"{n.label}: selection {k} reports {name} before it ran (or after the values stopped being unit)")

    def tensor(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.torch.cuda.synchronize()
        return t

    def node(self, rec):
        return self.gen.nodes[rec["node"]]

    # --------------------------------------------------------------------------------------------------- operations
    def execute(self, rec):
        try:
            getattr(self, "do_" + rec["op"])(rec, self.node(rec))
        except AssertionError as e:
            if "-- seed" in str(e):
                raise
            self.fail(e)
        except self.api.SpmvHipError as e:
            self.fail(f"unexpected refusal: {e}")

    def do_upload(self, rec, n):
        api, torch = self.api, self.torch
        if n.params["adopted"]:
            t = (self.tensor(n.IRP.astype(np.int64)), self.tensor(n.JA.astype(np.int32)), self.tensor(n.vals.copy()))
            dmx = api.DeviceMatrix()
            assert api.lib.spmvHipAdoptCSR(C.byref(dmx.handle), n.M, n.N, n.JA.size, C.c_void_p(t[0].data_ptr()), 8,
                                           C.c_void_p(t[1].data_ptr()), C.c_void_p(t[2].data_ptr()), None) == 0
            dmx.rows = n.M
            self.adopted[n.id] = t
        else:
            dmx = api.spMatCpyCSR(api.HostCSR(n.M, n.N, n.IRP, n.JA, n.vals))
        self.h[n.id] = dmx
        self.check_node(n)

    def do_reupload(self, rec, n):
        self.do_free(rec, self.gen.nodes[rec["freed"]])
        self.do_upload(rec, n)

    def do_free(self, rec, n):
        self.h[n.id].free()
        self.adopted.pop(n.id, None)

    def do_set_values(self, rec, n):
        if rec["how"] == "host":
            self.h[n.id].update_values(n.vals)
        elif rec["how"] == "device tensor":
            self.h[n.id].update_values(self.tensor(n.vals.copy()))
        else:
            self.adopted[n.id][2].copy_(self.torch.from_numpy(n.vals))
            self.torch.cuda.synchronize()
            self.h[n.id].values_changed()
        self.check_node(n, updated=True)

    do_update_derived = do_set_values

    def do_derive(self, rec, n):
        S = [self.h[s] for s in rec["srcs"]]
        p, kind = rec["params"], rec["kind"]
        if kind == "transpose":
            d = S[0].transpose()
        elif kind == "permute":
            col = S[0].colour(order=p["order"], seed=p["seed"])
            try:
                perm = col.perm.down(np.uint32)
                want = dm.permutation(self.gen.nodes[rec["srcs"][0]].mat, p)
                assert np.array_equal(perm, want), f"colour({p}): the permutation differs from colour_ref"
                d = S[0].permute(col)
            finally:
                col.free()
        elif kind == "multiply":
            d = S[0].multiply(S[1])
        elif kind == "add":
            d = S[0].add(S[1], p["alpha"], p["beta"])
        elif p["mode"] == fr.BAND and (p["lo"], p["hi"]) == (0, 0):
            d = S[0].diagonal_matrix()
        elif p["mode"] == fr.BAND and p["lo"] == fr.INT64_MIN:
            d = S[0].tril(p["hi"])
        elif p["mode"] == fr.BAND and p["hi"] == fr.INT64_MAX:
            d = S[0].triu(p["lo"])
        else:
            d = S[0].filter(p["mode"], p["lo"], p["hi"], p["theta"], p["lump"])
        self.h[n.id] = d
        self.check_node(n)

    def _refresh(self, n, use, params):
        d, S = self.h[n.id], [self.h[s] for s in use]
        if n.kind == "transpose":
            d.refresh_from(S[0])
        elif n.kind == "permute":
            d.permute_refresh(S[0])
        elif n.kind == "multiply":
            d.multiply_refresh(S[0], S[1])
        elif n.kind == "add":
            d.add_refresh(S[0], S[1], params["alpha"], params["beta"])
        else:
            d.filter_refresh(S[0])

    def do_refresh(self, rec, n):
        self._refresh(n, n.srcs, rec["params"])
        self.check_node(n, updated=True)

    def do_refresh_refused(self, rec, n):
        """refused on the host, before any launch: the library compares the handles' identities first"""
        try:
            self._refresh(n, rec["use"], n.params)
        except self.api.SpmvHipError:
            pass
        else:
            self.fail(f"{n.label}: the refresh was taken")
        self.check_node(n)

    def do_build(self, rec, n):
        api, d = self.api, self.h[n.id]
        if rec["what"] == "tiles":
            api.build_tiles(d, deterministic=rec["det"])
        elif rec["what"] == "stripes":
            api.build_stripes(d, deterministic=rec["det"], **rec["opts"])
        else:
            assert api.lib.spmvHipBuildSell(C.byref(d.handle)) == 0
        self.check_choices(n)

    def run(self, rows, x, launch):
        api = self.api
        dx = api.DeviceVector(x.size).up(x)
        dy = api.DeviceVector(rows)
        dy.poison()
        api.lib.spmvHipDeviceSynchronize()
        try:
            rc = launch(dx, dy)
            assert rc in (0, None), f"launch failed ({rc})"
            assert api.lib.spmvHipDeviceSynchronize() == 0
            return dy.down()
        finally:
            dx.free()
            dy.free()

    def serial(self, n, x, y, what, order=None):
        ja, v = (n.JA, n.vals) if order is None else (n.JA[order], n.vals[order])
        self.same(y, self.oracle.csr_serial(n.IRP, ja, v, x), what)

    def any_order(self, n, x, y, what):
        assert not np.isnan(y).any(), f"{what}: NaN (poison survived?)"
        check_any_order(n.IRP, n.JA, n.vals, x, y, what)
        t = tight_error(n.IRP, n.JA, n.vals, x, self.oracle.csr_serial(n.IRP, n.JA, n.vals, x), y)
        assert t <= TIGHT, f"{what}: tight_error {t:.3e} > {TIGHT}"

    def do_product(self, rec, n):
        api, d, which, x, what = self.api, self.h[n.id], rec["which"], rec["x"], rec["text"]
        H = C.byref(d.handle)
        st = self.user_stream if rec["user"] else None
        name = {"rows": "hipSpMVRowsCSR", "warp": "hipSpMVWarpPerRowCSR", "auto": "hipSpMVAutoCSR", "tiles": "hipSpMVTilesCSR",
                "stripes": "hipSpMVStripesCSR", "sell": "hipSpMVRowsSELL"}.get(which)
        if name:
            y = self.run(n.M, x, lambda dx, dy: api.SPMV_LAUNCHERS[name](H, dx.ptr, api.CONFIG(), dy.ptr))
        elif which == "enq_auto":
            y = self.run(n.M, x, lambda dx, dy: api.lib.spmvHipEnqueueAuto(H, dx.ptr, dy.ptr, st))
        elif which == "enq_auto_rows":
            y = self.run(n.M, x, lambda dx, dy: api.lib.spmvHipEnqueueAutoRows(H, dx.ptr, dy.ptr, st))
        else:
            y = self.run(n.M, x, lambda dx, dy: api.lib.spmvHipEnqueueCSR(H, int(which[-1]), dx.ptr, dy.ptr, self.user_stream))
        self.check_choices(n)
        if not rec["check"]:
            return
        self.counts["products"] += 1
        if rec["serial"]:
            order = tiles_order(n.IRP, n.JA) if which == "tiles" else stripes_order(n.IRP, n.JA) if which == "stripes" else None
            self.serial(n, x, y, what, order)
        else:
            if which == "sell":
                short = np.diff(n.IRP.astype(np.int64)) <= 256
                self.same(y[short], self.oracle.csr_serial(n.IRP, n.JA, n.vals, x)[short], what + " rows <= 256")
            self.any_order(n, x, y, what)

    def do_final(self, rec, n):
        d = self.h[n.id]
        y = self.run(n.M, rec["x"], lambda dx, dy: self.api.SPMV_LAUNCHERS["hipSpMVRowsCSR"](C.byref(d.handle), dx.ptr, self.api.CONFIG(), dy.ptr))
        self.serial(n, rec["x"], y, rec["text"])
        self.counts["products"] += 1
        self.check_node(n)

    def do_matmul(self, rec, n):
        torch, X, k = self.torch, rec["X"], rec["X"].shape[1]
        dX = self.tensor(X) if not rec["xl"] else self.tensor(X.T).t()
        out = torch.full((n.M, k), float("nan"), dtype=torch.float64, device="cuda") if not rec["yl"] else \
            torch.full((k, n.M), float("nan"), dtype=torch.float64, device="cuda").t()
        torch.cuda.synchronize()
        self.h[n.id].matmul(dX, out=out)
        self.api.lib.spmvHipDeviceSynchronize()
        Y = out.cpu().numpy()
        for c in range(k):
            self.serial(n, X[:, c], Y[:, c], f"{rec['text']} column {c}")
        self.counts["products"] += 1

    def do_solve(self, rec, n):
        if not rec["check"]:
            return
        d, B, k = self.h[n.id], rec["B"], rec["k"]
        if k == 0:
            got = d.solve_triangular(self.tensor(B[:, 0].copy()), lower=rec["lower"], unit_diagonal=rec["unit"])
            self.api.lib.spmvHipDeviceSynchronize()
            self.same(got.cpu().numpy(), trsv_levels(n.M, n.IRP, n.JA, n.vals, B[:, 0], lower=rec["lower"], unit=rec["unit"]), rec["text"])
        else:
            got = d.solve_triangular_block(self.tensor(B), lower=rec["lower"], unit_diagonal=rec["unit"])
            self.api.lib.spmvHipDeviceSynchronize()
            want = trsm_levels(n.M, n.IRP, n.JA, n.vals, B, lower=rec["lower"], unit=rec["unit"])
            got = got.cpu().numpy()
            for c in range(k):
                self.same(got[:, c], want[:, c], f"{rec['text']} column {c}")
        self.counts["solves"] += 1

    def do_ilu0(self, rec, n):
        d = self.h[n.id]
        info = d.ilu0()
        assert (info.zeroPivot, info.firstBadRow) == (rec["zeroPivot"], -1), \
            f"ilu0({n.label}): zeroPivot {info.zeroPivot}, firstBadRow {info.firstBadRow}; the model: {rec['zeroPivot']}, -1"
        self.check_node(n, updated=True)
        if not rec["solves"]:
            return
        b = rec["b"]
        for lower, unit in ((True, True), (False, False)):
            got = d.solve_triangular(b, lower=lower, unit_diagonal=unit)
            self.same(got, trsv_levels(n.M, n.IRP, n.JA, n.vals, b, lower=lower, unit=unit), f"{'L' if lower else 'U'} solve on the factors of {n.label}")
            self.counts["solves"] += 1

    def do_krylov(self, rec, n):
        api, d = self.api, self.h[n.id]
        pre = None
        try:
            if rec["F"] is not None:
                pre = api.spMatCpyCSR(api.HostCSR(n.M, n.N, n.IRP, n.JA, n.vals))
                pre.ilu0()
                self.same(self.down(pre.handle.AS, n.JA.size, np.float64), rec["F"], "the factored copy")
            kw = dict(restart=rec["restart"]) if rec["restart"] else {}
            x, info = getattr(d, rec["method"])(rec["b"], precond=pre, tol=rec["tol"], maxiter=rec["maxiter"], **kw)
        finally:
            if pre is not None:
                pre.free()
        wx, wstatus, wit = rec["want"][:3]
        assert (info.status, info.iterations) == (wstatus, wit), f"{rec['text']}: status {info.status} after {info.iterations}"
        if rec["check"]:
            self.same(x, wx, f"{rec['text']}: x")
            self.counts["krylov"] += 1
        self.check_node(n)


    # ---- hierarchies
    def _amg(self, src, H):
        h = src.amg(seed=H.kw["seed"], coarseRows=H.kw["coarseRows"], smoothed=H.kind != "plain", theta=dm.THETA if H.kind == "strength" else None)
        assert h.info.levels == len(H.levels), f"{H.label}: {h.info.levels} levels, the reference {len(H.levels)}"
        return h

    def do_hierarchy(self, rec, n):
        act, what = rec["action"], rec["text"]
        if act == "skip":
            return
        H = self.gen.hiers[rec["hier"]]
        if act == "free":
            self.hh.pop(H.id).free()
            return
        src = self.h[n.id]
        if act == "setup":
            self.hh[H.id] = self._amg(src, H)
        h = self.hh[H.id]
        if act in ("set_smoother", "set_gauss_seidel"):
            getattr(h, act)(**rec["args"])
        elif act == "set_block_width":
            h.set_block_width(rec["args"]["width"])
            assert h.block_info()["width"] == rec["args"]["width"]
        elif act == "refresh":
            h.refresh_from(src)
        self.same(h.apply(rec["r"]), rec["z"], f"{what}: the cycle")
        self.counts["cycles"] += 1
        if "R" in rec and rec["Z"] is None:              # refused on the host: no workspace of that width, or Gauss-Seidel
            try:
                h.apply_block(rec["R"])
            except self.api.SpmvHipError:
                pass
            else:
                self.fail(f"{what}: the block cycle was taken")
            self.same(h.apply(rec["r"]), rec["z"], f"{what}: the cycle after the refusal")
        elif "R" in rec:
            Z = h.apply_block(rec["R"])
            for c in range(rec["R"].shape[1]):
                self.same(Z[:, c], rec["Z"][:, c], f"{what}: column {c} of the block cycle")
            self.counts["cycles"] += 1
        if rec.get("twin"):                              # a fresh hierarchy with the same settings gives the same bits
            twin = self._amg(src, H)
            try:
                if H.set_call:
                    getattr(twin, H.set_call[0])(**H.set_call[1])
                self.same(twin.apply(rec["r"]), rec["z"], f"{what}: the twin's cycle")
                self.counts["cycles"] += 1
            finally:
                twin.free()
