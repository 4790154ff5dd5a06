"""Seeded operation sequences on a pool of device handles, checked step by step against a host model.

A handle carries much state derived from its values (unit flag and value, both forms of the two-phase and the stripes
format, SELL, the two kernel selections, a transpose's link to its source, the triangular schedules), and the process
carries more (kernel variants, unit detection, stream, sync mode, ELL row lengths).  Every other GPU test checks one
feature on a fresh handle; this one keeps using the same handles the way an iterative caller does, and draws what it does
next from a seeded generator: new values of five kinds (from the host, from a device tensor, or written in place into an
adopted array), process-wide switches, format builds, every product, queries, transposes, re-uploads and ELL conversions.

After every product the result is compared with the model:
  * serial-order paths give the bits of sgemvSerial (in the stored order, or stably by column / by 16 Ki-column slice for
    the deterministic formats on unsorted rows), SpMM column by column, the transpose as the scatter loop, the triangular
    solves as the serial loop, a derived ELL handle with the values it was made from;
  * any-order paths meet exact_ref.check_any_order (a rigorous bound against the exactly rounded row sums) AND the
    suite's tight_error <= 1e-13;
  * y starts poisoned, and no poison survives.
Every failure names the seed and the trace of operations up to the failing step; one seed runs alone by its id
(tests/test_gpu_sequences.py::test_sequence[7]).

16 seeds of 40 operations each, plus a final serial-order product on every handle; measured on one MI355X: 24 s for
the module (704 operations, 305 of them checked products)."""
import ctypes as C

import numpy as np
import pytest

from bits import assert_same_bits
from conftest import tight_error
from exact_ref import check_any_order
from sequence_inputs import FAMILIES, KINDS, family, unit_of, values
from serial_order_inputs import stripes_order, tiles_order
from transpose_ref import stable_transpose
from trsv_ref import trsv_levels

pytestmark = pytest.mark.gpu

SEEDS = range(16)
STEPS = 40
TIGHT = 1e-13
MEM_TOL = 8 << 20                      # what test_device_memory_comes_back allows: the runtime's pools wobble by 4 MiB pieces
SERIAL_NAMES = {b"hipSpMVRowsCSR", b"hipSpMVTilesCSR(deterministic)", b"hipSpMVStripesCSR(owner wavefronts)",
                b"hipSpMVStripesCSR(ordered tickets)"}
REDUCTION_NAMES = {b"hipSpMVWarpPerRowCSR", b"hipSpMVTilesCSR", b"hipSpMVStripesCSR"}
# the stripes layout a selection's winner keeps: [selection][name] (shared stream: arrival order and ordered tickets)
WINNER_LAYOUT = ({b"hipSpMVStripesCSR": "shared"},
                 {b"hipSpMVStripesCSR(owner wavefronts)": "owner", b"hipSpMVStripesCSR(ordered tickets)": "shared"})
ELL_FAMILIES = ("uploaded", "square", "shuffled")     # short rows: a padded ELL copy stays small


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


class Handle:
    """one device handle of the pool and what the model knows about it"""

    def __init__(self, ctx, fam):
        self.fam = fam
        self.M, self.N, self.IRP, self.JA, self.x0, self.x1 = family(fam)
        self.vals = values(ctx.rng, "uniform", self.IRP, self.JA, self.x0)
        self.dm = None
        self.T = None                   # (transpose handle, source values at its last refresh, source handle id)
        self.ell = None                 # (derived ELL handle, the values it was made from)
        self.upload(ctx)

    def upload(self, ctx):
        api, torch = ctx.api, ctx.torch
        if self.fam == "adopted64":     # 64-bit row pointers, caller-owned AS
            self.d_irp = torch.from_numpy(self.IRP.astype(np.int64)).cuda()
            self.d_ja = torch.from_numpy(self.JA.astype(np.int32)).cuda()
            self.d_as = torch.from_numpy(self.vals.copy()).cuda()
            torch.cuda.synchronize()
            self.dm = api.DeviceMatrix()
            assert api.lib.spmvHipAdoptCSR(C.byref(self.dm.handle), self.M, self.N, self.JA.size,
                                           C.c_void_p(self.d_irp.data_ptr()), 8, C.c_void_p(self.d_ja.data_ptr()),
                                           C.c_void_p(self.d_as.data_ptr()), None) == 0
            self.dm.rows = self.M
        else:
            self.dm = api.spMatCpyCSR(api.HostCSR(self.M, self.N, self.IRP, self.JA, self.vals))
        self.gen = ctx.next_gen()
        self.tiles_det, self.stripes_det = False, 0      # what hipSpMVTilesCSR / hipSpMVStripesCSR run on a new handle
        # the stripes layouts the handle holds ("shared" / "owner") -> built while the values were unit (no value array:
        # rebuilt at the next update that makes them non-unit)
        self.stripes = {}
        self.selected = [False, False]                   # the reduction-order / serial-order selection has run
        self.unit = unit_of(self.vals) if ctx.unit_on else (False, None)

    def free(self):
        for part in (self.T, self.ell):
            if part:
                part[0].free()
        self.T = self.ell = None
        self.dm.free()
        self.d_irp = self.d_ja = self.d_as = None


class Ctx:
    def __init__(self, api, torch, oracle, seed, stream):
        self.api, self.torch, self.oracle, self.seed, self.user_stream = api, torch, oracle, seed, stream
        self.rng = np.random.default_rng(seed)
        self.trace = []
        self.unit_on, self.stream, self.sync, self.ell_rl = True, None, True, True
        self.variant = {"hipSpMVRowsCSR": 2, "hipSpMVWarpPerRowCSR": 2}
        self._gen = 0
        self.pool = {}

    def next_gen(self):
        self._gen += 1
        return self._gen

    def where(self):
        return f"seed {self.seed}, step {len(self.trace)}; trace:\n  " + "\n  ".join(self.trace)

    def x_of(self, h, n=None):
        return (h.x0, h.x1)[int(self.rng.integers(2))] if n is None else (h.x0, h.x1)[n]

    # ---------------------------------------------------------------- one product and its check
    def run(self, rows, x, launch):
        api = self.api
        dx = api.DeviceVector(x.size).up(x)
        dy = api.DeviceVector(rows)
        dy.poison()
        api.lib.spmvHipDeviceSynchronize()
        try:
            rc = launch(dx, dy)
            assert rc in (0, None), f"launch failed ({rc}) -- {self.where()}"
            assert api.lib.spmvHipDeviceSynchronize() == 0
            return dy.down()
        finally:
            dx.free()
            dy.free()

    def serial(self, y, y_ref, what, h=None):
        assert not np.isnan(y).any(), f"{what}: NaN (poison survived?) -- {self.where()}"
        lens = None if h is None else np.diff(h.IRP.astype(np.int64))
        try:
            assert_same_bits(y, y_ref, what, None if lens is None else (lambda r: f"length {lens[r]}"))
        except AssertionError as e:
            raise AssertionError(f"{e} -- {self.where()}") from None

    def any_order(self, h, vals, x, y, what):
        try:
            check_any_order(h.IRP, h.JA, vals, x, y, what)
            y_ref = self.oracle.csr_serial(h.IRP, h.JA, vals, x)
            t = tight_error(h.IRP, h.JA, vals, x, y_ref, y)
            assert t <= TIGHT, f"{what}: tight_error {t:.3e} > {TIGHT}"
        except AssertionError as e:
            raise AssertionError(f"{e} -- {self.where()}") from None


# -------------------------------------------------------------------- the operations
def op_update_host(ctx, h, kind):
    v = values(ctx.rng, kind, h.IRP, h.JA, h.x0)
    h.dm.update_values(v)
    return _after_update(ctx, h, v, f"update_values({h.fam}, {kind}, host)")


def op_update_device(ctx, h, kind):
    v = values(ctx.rng, kind, h.IRP, h.JA, h.x0)
    t = ctx.torch.from_numpy(v.copy()).cuda()
    ctx.torch.cuda.synchronize()
    h.dm.update_values(t)
    return _after_update(ctx, h, v, f"update_values({h.fam}, {kind}, device tensor)")


def op_adopted_in_place(ctx, h, kind):
    v = values(ctx.rng, kind, h.IRP, h.JA, h.x0)
    h.d_as.copy_(ctx.torch.from_numpy(v))
    ctx.torch.cuda.synchronize()
    h.dm.values_changed()
    return _after_update(ctx, h, v, f"write adopted AS + values_changed({h.fam}, {kind})")


def _after_update(ctx, h, v, label):
    ctx.trace.append(label)
    before = h.unit
    h.vals = v
    h.unit = unit_of(v) if ctx.unit_on else (False, None)
    info = h.dm.update_info()
    same = before[0] and h.unit[0] and np.float64(before[1]).tobytes() == np.float64(h.unit[1]).tobytes()
    got = (info.unitBefore, info.unitAfter)
    assert got == (int(before[0]), int(h.unit[0])), f"update_info unitBefore/After {got} -- {ctx.where()}"
    rebuilt = not h.unit[0] and any(h.stripes.values())
    assert info.rebuilt == int(rebuilt), \
        f"update_info rebuilt {info.rebuilt}, model {int(rebuilt)} (stripes layouts {h.stripes}) -- {ctx.where()}"
    if rebuilt:
        h.stripes = {k: False for k in h.stripes}
    assert info.inPlace == int(not rebuilt and (not before[0] or same)), f"update_info inPlace {info.inPlace} -- {ctx.where()}"
    if before[0] and not h.unit[0]:                      # the selections measured the unit kernels: both forgotten
        h.selected = [False, False]
    _check_unit(ctx, h)
    _check_choices(ctx, h)


def _check_choices(ctx, h):
    for k, (fn, names) in enumerate(((ctx.api.lib.spmvHipAutoChoice, REDUCTION_NAMES),
                                     (ctx.api.lib.spmvHipAutoChoiceRows, SERIAL_NAMES))):
        name = fn(C.byref(h.dm.handle), None)
        if h.selected[k]:
            assert name in names, f"selection {k} chose {name} -- {ctx.where()}"
        else:
            assert name is None, f"selection {k} reports {name} before it ran -- {ctx.where()}"


def _stripes_built(h, layout):
    """a stripes layout built now, if the handle does not hold it yet"""
    h.stripes.setdefault(layout, bool(h.unit[0]))


def _selection_ran(ctx, h, k):
    """after a call that runs selection k if it has not run: the winner's stripes layout stays (the losers' go)"""
    if h.selected[k]:
        return
    h.selected[k] = True
    fn = (ctx.api.lib.spmvHipAutoChoice, ctx.api.lib.spmvHipAutoChoiceRows)[k]
    layout = WINNER_LAYOUT[k].get(fn(C.byref(h.dm.handle), None))
    if layout:
        _stripes_built(h, layout)


def _check_unit(ctx, h):
    c = C.c_double(12345.0)
    got = ctx.api.lib.spmvHipUnitValue(C.byref(h.dm.handle), C.byref(c))
    assert got == int(h.unit[0]), f"spmvHipUnitValue {got}, model {h.unit} -- {ctx.where()}"
    if h.unit[0]:
        assert np.float64(c.value).tobytes() == np.float64(h.unit[1]).tobytes(), \
            f"unit value {c.value!r}, model {h.unit[1]!r} -- {ctx.where()}"


def op_switch(ctx, h, _):
    api, r = ctx.api, ctx.rng.integers(6)
    if r == 0:
        ctx.unit_on = bool(ctx.rng.integers(2))
        api.lib.spmvHipSetUnitValues(int(ctx.unit_on))
        ctx.trace.append(f"spmvHipSetUnitValues({int(ctx.unit_on)})")
    elif r in (1, 2):
        name = ("hipSpMVRowsCSR", "hipSpMVWarpPerRowCSR")[r - 1]
        ctx.variant[name] = int(ctx.rng.integers(3))
        api.set_variant(name, ctx.variant[name])
        ctx.trace.append(f"set_variant({name}, {ctx.variant[name]})")
    elif r == 3:
        ctx.stream = ctx.user_stream if ctx.rng.integers(2) else None
        api.lib.spmvHipDeviceSynchronize()
        api.lib.spmvHipSetStream(ctx.stream)
        ctx.trace.append(f"spmvHipSetStream({'user' if ctx.stream is not None else 'default'})")
    elif r == 4:
        ctx.sync = bool(ctx.rng.integers(2))
        api.lib.spmvHipSetSync(int(ctx.sync))
        ctx.trace.append(f"spmvHipSetSync({int(ctx.sync)})")
    else:
        ctx.ell_rl = bool(ctx.rng.integers(2))
        api.lib.spmvHipSetEllRowLens(int(ctx.ell_rl))
        ctx.trace.append(f"spmvHipSetEllRowLens({int(ctx.ell_rl)})")


def op_build(ctx, h, _):
    api, r = ctx.api, ctx.rng.integers(3)
    if r == 0:
        det = bool(ctx.rng.integers(2))
        api.build_tiles(h.dm, deterministic=det)
        h.tiles_det = det
        ctx.trace.append(f"build_tiles({h.fam}, deterministic={int(det)})")
    elif r == 1:
        det = int(ctx.rng.integers(3))
        spread = int(ctx.rng.choice([-1, 0, 1, 4, 64]))
        grid = int(ctx.rng.choice([0, 0, 7, 32]))
        rpb = int(ctx.rng.choice([0, 0, 256, 1024]))
        api.build_stripes(h.dm, rowsPerBin=rpb, grid=grid, spread=spread, deterministic=det)
        h.stripes_det = det
        h.stripes["owner" if det == 1 else "shared"] = bool(h.unit[0])      # explicit options replace that layout
        ctx.trace.append(f"build_stripes({h.fam}, deterministic={det}, spread={spread}, grid={grid}, rowsPerBin={rpb})")
    else:
        assert api.lib.spmvHipBuildSell(C.byref(h.dm.handle)) == 0
        ctx.trace.append(f"spmvHipBuildSell({h.fam})")


def _spmv(ctx, name, dm):
    return lambda dx, dy: ctx.api.SPMV_LAUNCHERS[name](C.byref(dm.handle), dx.ptr, ctx.api.CONFIG(), dy.ptr)


def op_product(ctx, h, _):
    api, rng = ctx.api, ctx.rng
    which = ["rows", "warp", "auto", "enq_auto", "enq_auto_rows", "enq_csr0", "enq_csr1", "tiles", "stripes", "sell",
             "matmul"][rng.integers(11)]
    nx = int(rng.integers(2))
    x = ctx.x_of(h, nx)
    label = f"{which}({h.fam}, x{nx})"
    if which in ("rows", "warp"):
        name = "hipSpMVRowsCSR" if which == "rows" else "hipSpMVWarpPerRowCSR"
        label = f"{name} v{ctx.variant[name]}({h.fam}, x{nx})"
    ctx.trace.append(label)
    serial_ref = lambda perm=None: ctx.oracle.csr_serial(h.IRP, h.JA[perm], h.vals[perm], x) if perm is not None \
        else ctx.oracle.csr_serial(h.IRP, h.JA, h.vals, x)
    # enqueue entry points: spmvHipEnqueueCSR on the user stream, the selections' on a stream drawn per call
    st = ctx.user_stream if which.startswith("enq_csr") or rng.integers(2) else None
    if which.startswith("enq_"):
        ctx.trace[-1] = label = f"{label} on the {'user' if st is not None else 'null'} stream"
    if which == "rows":
        y = ctx.run(h.M, x, _spmv(ctx, "hipSpMVRowsCSR", h.dm))
        if ctx.variant["hipSpMVRowsCSR"] == 2:
            _selection_ran(ctx, h, 1)
        ctx.serial(y, serial_ref(), label, h)
    elif which == "warp":
        y = ctx.run(h.M, x, _spmv(ctx, "hipSpMVWarpPerRowCSR", h.dm))
        if ctx.variant["hipSpMVWarpPerRowCSR"] == 2:
            _selection_ran(ctx, h, 0)
        ctx.any_order(h, h.vals, x, y, label)
    elif which == "auto":
        y = ctx.run(h.M, x, _spmv(ctx, "hipSpMVAutoCSR", h.dm))
        _selection_ran(ctx, h, 0)
        ctx.any_order(h, h.vals, x, y, label)
    elif which == "enq_auto":
        y = ctx.run(h.M, x, lambda dx, dy: api.lib.spmvHipEnqueueAuto(C.byref(h.dm.handle), dx.ptr, dy.ptr, st))
        _selection_ran(ctx, h, 0)
        ctx.any_order(h, h.vals, x, y, label)
    elif which == "enq_auto_rows":
        y = ctx.run(h.M, x, lambda dx, dy: api.lib.spmvHipEnqueueAutoRows(C.byref(h.dm.handle), dx.ptr, dy.ptr, st))
        _selection_ran(ctx, h, 1)
        ctx.serial(y, serial_ref(), label, h)
    elif which in ("enq_csr0", "enq_csr1"):
        wpr = int(which[-1])
        y = ctx.run(h.M, x, lambda dx, dy: api.lib.spmvHipEnqueueCSR(C.byref(h.dm.handle), wpr, dx.ptr, dy.ptr, st))
        if wpr:
            ctx.any_order(h, h.vals, x, y, label)
        else:
            ctx.serial(y, serial_ref(), label, h)
    elif which == "tiles":
        y = ctx.run(h.M, x, _spmv(ctx, "hipSpMVTilesCSR", h.dm))
        if h.tiles_det:
            ctx.serial(y, serial_ref(tiles_order(h.IRP, h.JA)), label + " deterministic", h)
        else:
            ctx.any_order(h, h.vals, x, y, label + " arrival order")
    elif which == "stripes":
        y = ctx.run(h.M, x, _spmv(ctx, "hipSpMVStripesCSR", h.dm))
        _stripes_built(h, "owner" if h.stripes_det == 1 else "shared")
        if h.stripes_det:
            ctx.serial(y, serial_ref(stripes_order(h.IRP, h.JA)), label + f" deterministic {h.stripes_det}", h)
        else:
            ctx.any_order(h, h.vals, x, y, label + " arrival order")
    elif which == "sell":
        y = ctx.run(h.M, x, _spmv(ctx, "hipSpMVRowsSELL", h.dm))
        short = np.diff(h.IRP.astype(np.int64)) <= 256
        ctx.serial(y[short], serial_ref()[short], label + " rows <= 256", None)
        ctx.any_order(h, h.vals, x, y, label)
    else:
        _matmul(ctx, h, label)


def _matmul(ctx, h, label):
    torch, rng = ctx.torch, ctx.rng
    k = int(rng.choice([1, 5, 16, 17]))
    xl, yl = int(rng.integers(2)), int(rng.integers(2))
    ctx.trace[-1] = label = f"matmul({h.fam}, k={k}, X {'col' if xl else 'row'}-major, Y {'col' if yl else 'row'}-major)"
    X = np.stack([(h.x0, h.x1)[c % 2] * (1.0 + c) for c in range(k)], axis=1)
    dX = torch.from_numpy(X).cuda() if not xl else torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
    out = torch.full((h.M, k), float("nan"), dtype=torch.float64, device="cuda") if not yl else \
        torch.full((k, h.M), float("nan"), dtype=torch.float64, device="cuda").t()
    torch.cuda.synchronize()
    h.dm.matmul(dX, out=out)
    ctx.api.lib.spmvHipDeviceSynchronize()
    Y = out.cpu().numpy()
    for c in range(k):
        ctx.serial(Y[:, c], ctx.oracle.csr_serial(h.IRP, h.JA, h.vals, X[:, c]), f"{label} column {c}", h)


def op_query(ctx, h, _):
    ctx.trace.append(f"queries({h.fam})")
    _check_unit(ctx, h)
    _check_choices(ctx, h)


def op_transpose(ctx, h, _):
    api = ctx.api
    if h.T is not None and ctx.rng.integers(2):
        t, _, src = h.T
        if src == h.gen:
            t.refresh_from(h.dm)
            h.T = (t, h.vals.copy(), src)
            ctx.trace.append(f"transpose({h.fam}).refresh_from(source)")
        else:                                            # the source was freed and uploaded again: a new handle
            ctx.trace.append(f"transpose({h.fam}).refresh_from(re-uploaded source) refused")
            with pytest.raises(api.SpmvHipError):
                t.refresh_from(h.dm)
    else:
        if h.T is not None:
            h.T[0].free()
        h.T = (h.dm.transpose(), h.vals.copy(), h.gen)
        ctx.trace.append(f"transpose({h.fam})")
    t, snap, _ = h.T
    u = unit_of(snap) if ctx.unit_on else (False, None)
    if ctx.trace[-1].endswith("refused"):
        return
    c = C.c_double(12345.0)
    assert api.lib.spmvHipUnitValue(C.byref(t.handle), C.byref(c)) == int(u[0]), f"transpose unit -- {ctx.where()}"
    if u[0]:
        assert np.float64(c.value).tobytes() == np.float64(u[1]).tobytes(), \
            f"transpose unit value {c.value!r}, model {u[1]!r} -- {ctx.where()}"


def op_transpose_product(ctx, h, _):
    if h.T is None:
        return op_transpose(ctx, h, _)
    t, snap, _ = h.T
    x = ctx.rng.uniform(-1, 1, h.M) * 2.0 ** ctx.rng.integers(-8, 9, h.M)
    ctx.trace.append(f"hipSpMVRowsCSR v{ctx.variant['hipSpMVRowsCSR']} on transpose({h.fam})")
    IRPt, JAt, ASt, _ = stable_transpose(h.N, h.IRP, h.JA, snap)
    y = ctx.run(h.N, x, _spmv(ctx, "hipSpMVRowsCSR", t))
    ctx.serial(y, ctx.oracle.csr_serial(IRPt, JAt, ASt, x), ctx.trace[-1])


def op_solve(ctx, h, _):
    h = ctx.pool["square"]
    torch, rng = ctx.torch, ctx.rng
    lower, unit = bool(rng.integers(2)), bool(rng.integers(2))
    b = rng.uniform(-1, 1, h.N)
    ctx.trace.append(f"solve_triangular(square, lower={int(lower)}, unit_diagonal={int(unit)})")
    db = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    out = h.dm.solve_triangular(db, lower=lower, unit_diagonal=unit)
    ctx.api.lib.spmvHipDeviceSynchronize()
    got = out.cpu().numpy()
    ref = trsv_levels(h.M, h.IRP, h.JA, h.vals, b, lower=lower, unit=unit)
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), f"solve: NaN rows differ -- {ctx.where()}"
    ctx.serial(np.where(nan, 0.0, got), np.where(nan, 0.0, ref), ctx.trace[-1])


def op_ell(ctx, h, _):
    api = ctx.api
    if h.fam not in ELL_FAMILIES:
        h = ctx.pool["uploaded"]
    if h.ell is None or ctx.rng.integers(2):
        if h.ell is not None:
            h.ell[0].free()
        h.ell = (api.csr_to_ell_device(h.dm, True), h.vals.copy())
        ctx.trace.append(f"csr_to_ell_device({h.fam}); update of the ELL handle refused")
        with pytest.raises(api.SpmvHipError):
            h.ell[0].update_values(h.vals)
        return
    e, snap = h.ell
    nx = int(ctx.rng.integers(2))
    x = ctx.x_of(h, nx)
    ctx.trace.append(f"hipSpMVRowsELL(ELL of {h.fam}, x{nx}, row lengths {int(ctx.ell_rl)})")
    y = ctx.run(h.M, x, _spmv(ctx, "hipSpMVRowsELL", e))
    ctx.serial(y, ctx.oracle.csr_serial(h.IRP, h.JA, snap, x) + 0.0, ctx.trace[-1], h)


def op_reupload(ctx, h, _):
    ctx.trace.append(f"free + upload({h.fam}) with new values")
    h.dm.free()
    h.vals = values(ctx.rng, KINDS[int(ctx.rng.integers(len(KINDS)))], h.IRP, h.JA, h.x0)
    h.upload(ctx)
    _check_unit(ctx, h)


# (operation, weight, needs a value kind)
OPS = [(op_update_host, 5, True), (op_update_device, 3, True), (op_adopted_in_place, 2, True), (op_switch, 5, False),
       (op_build, 4, False), (op_product, 14, False), (op_query, 2, False), (op_transpose, 2, False),
       (op_transpose_product, 2, False), (op_solve, 2, False), (op_ell, 2, False), (op_reupload, 1, False)]
_W = np.array([w for _, w, _ in OPS], dtype=np.float64)

_memory = {}
PRODUCTS = ("hipSpMV", "warp(", "rows(", "auto(", "enq_", "tiles(", "stripes(", "sell(", "matmul(", "solve_", "final ")


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence(api, torch, oracle, stream, seed):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    ctx = Ctx(api, torch, oracle, seed, stream)
    try:
        for fam in FAMILIES:
            ctx.pool[fam] = Handle(ctx, fam)
        for _ in range(STEPS):
            op, _, kinded = OPS[int(ctx.rng.choice(len(OPS), p=_W / _W.sum()))]
            h = ctx.pool[FAMILIES[int(ctx.rng.integers(len(FAMILIES)))]]
            if op is op_adopted_in_place:
                h = ctx.pool["adopted64"]
            kind = KINDS[int(ctx.rng.integers(len(KINDS)))] if kinded else None
            op(ctx, h, kind)
        # every handle once more through the serial-order launcher, after the whole history
        for h in ctx.pool.values():
            ctx.trace.append(f"final hipSpMVRowsCSR({h.fam})")
            x = h.x0
            ctx.serial(ctx.run(h.M, x, _spmv(ctx, "hipSpMVRowsCSR", h.dm)), oracle.csr_serial(h.IRP, h.JA, h.vals, x),
                       ctx.trace[-1], h)
        print(f"seed {seed}: {len(ctx.trace)} operations, {sum(t.startswith(P) for t in ctx.trace for P in PRODUCTS)} products")
    finally:
        api.lib.spmvHipDeviceSynchronize()
        for h in ctx.pool.values():
            h.free()
        ctx.pool.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1 = torch.cuda.mem_get_info()[0]
    # the first seed of the process may load code objects and the library's shared workspace: from the second seed on
    # free memory must come back to where the first one left it
    assert free1 >= free0 - (256 << 20), (seed, free0, free1)
    base = _memory.setdefault("after first seed", free1)
    assert free1 >= base - MEM_TOL, f"seed {seed}: {(base - free1) >> 20} MiB not given back"
