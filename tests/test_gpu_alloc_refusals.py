"""Every device allocation of a call refused in turn (spmvHipAllocRefuse), and what the call leaves each time.

One table of operations, one driver.  For an operation the driver makes the inputs, lets the call run unarmed on a twin
(N = the allocations it asks for; its result is compared once with the existing reference), and then, for EVERY n in
[0, N), once with that allocation alone refused and once with every allocation from it on, checks in this order:

  1 refusal      refused >= 1, EXIT_FAILURE, a "libspmvhip" line on stderr (a call the header says falls back may also
                 succeed with the reference's bits, and must with every allocation refused)
  2 ledger       no bad release; where nothing may be left behind, the library holds what it held before the call
  3 outputs      a zeroed destination handle is still zero, a patterned info struct still holds the pattern, a poisoned
                 output vector is still poisoned; an in-place call keeps what its header comment promises
  4 sources      the sources' hipSpMVRowsCSR products, selections, built formats and update records are what they were
  5 lawful       a handle the call leaves alive gives its old bits; one that is not live is refused by a launcher
  6 no sticky    spmvHipVecFill on a scratch vector and a download succeed and show the fill
  7 retry        the same call, unarmed, on the same handles succeeds with the twin's bits

No launch goes through a destination before 1-3 have passed for that call; an assertion that fails ends the case.  Before
every call of the sweep the library gives back its own workspaces (spmvHipFinalize, spmvHipInit), so the count of a call
does not depend on what ran before it and the allocations of the workspaces are swept too.  At the end of a case every
handle is freed and the ledger is back at the level it had before the case existed.  Leaks are the ledger's to measure,
never mem_get_info's: that sees every other process on the card."""
import ctypes as C
import time

import numpy as np
import pytest

import add_ref as adr
import amg_cheb_ref as cb
import amg_gs_ref as gr
import amg_ref as ar
import amg_sa_ref as sa
import colour_ref as cl
import filter_ref as fr
import ilu0_ref
import spgemm_ref as sr
import trsv_ref
from bits import assert_same_bits
from conftest import random_csr
from exact_ref import check_any_order
from block_krylov_ref import block_dot_ref
from gmres_ref import gmres_ref, multi_dot_ref
from krylov_ref import Csr, bicgstab_ref, cg_ref, dot_ref
from transpose_ref import stable_transpose

pytestmark = pytest.mark.gpu

ROWS, WARP = "hipSpMVRowsCSR", "hipSpMVWarpPerRowCSR"
PATTERN = 0xA5
FILL = 0x7FF8DEADBEEF0001                      # a NaN payload for the sticky-error check
MODULE_START = []                              # the ledger's (live, liveBytes, badFrees) before the module's first call
MEASURED = []                                  # (operation, N, armed calls, seconds) of every sweep, printed by the last test


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.alloc_refuse(-1)
    start = a.alloc_stats()
    a.spmvHipInit(0)
    MODULE_START[:] = [int(start.live), int(start.liveBytes), int(start.badFrees)]
    yield a
    a.alloc_refuse(-1)
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.alloc_refuse(-1)
    api.set_variant(ROWS, 2)
    api.set_variant(WARP, 2)
    if api.lib.spmvHipDeviceSynchronize() != 0:                      # a device error is a finding: nothing more runs on it
        pytest.exit("the device reports an error after this case: the remaining cases are not run", returncode=3)


# --------------------------------------------------------------------------------------------------------- small tools
def _level(api):
    st = api.alloc_stats()
    return int(st.live), int(st.liveBytes)


def _cold(api):
    """the library's own workspaces (product, dot, caches) go back: the next call starts from nothing of its own"""
    api.spmvHipFinalize()
    api.spmvHipInit(0)


def _patterned(kind):
    s = kind()
    C.memset(C.addressof(s), PATTERN, C.sizeof(s))
    return s


def _is_patterned(s):
    return C.string_at(C.addressof(s), C.sizeof(s)) == bytes([PATTERN]) * C.sizeof(s)


def _handle_bytes(dm):
    return C.string_at(C.addressof(dm.handle), C.sizeof(dm.handle))


def _down(api, ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
    return out


def _csr_arrays(api, dm, irp=np.uint32):
    h = dm.handle
    return (_down(api, h.IRP, int(h.M) + 1, irp).astype(np.uint64), _down(api, h.JA, int(h.NZ), np.uint32).astype(np.uint64),
            _down(api, h.AS, int(h.NZ), np.float64))


def _product(api, launcher, dm, x, M):
    dx, dy = api.DeviceVector(x.size).up(x), api.DeviceVector(M)
    try:
        dy.poison()
        api.spmv(launcher, dm, dx, dy)
        return dy.down()
    finally:
        dx.free()
        dy.free()


def _x(seed, n):
    return np.sin(np.random.default_rng(seed).uniform(0, 2 * np.pi, size=n)) * 3e-5


def _blob(parts):
    return tuple(np.ascontiguousarray(p).tobytes() for p in parts)


def _choice(api, dm, rows):
    fn = api.lib.spmvHipAutoChoiceRows if rows else api.lib.spmvHipAutoChoice
    return fn(C.byref(dm.handle), None) or b"-"


def _formats(api, dm):
    h = C.byref(dm.handle)
    return int(api.lib.spmvHipTilesBytes(h)), int(api.lib.spmvHipStripesBytes(h)), int(api.lib.spmvHipSellBytes(h))


def _source_state(api, dm, x):
    """what invariant 4 compares: the serial-order product, both selections, the built formats, the last update's record"""
    y = _product(api, ROWS, dm, x, int(dm.handle.M))
    u = dm.update_info()
    return (y.tobytes(), _choice(api, dm, True), _choice(api, dm, False), _formats(api, dm),
            (u.inPlace, u.rebuilt, u.mapsBuilt, u.unitBefore, u.unitAfter))


def _not_live_is_refused(api, dm, capfd):
    """a handle that is not live is refused loudly by a launcher, before anything is launched"""
    v = api.DeviceVector(8)
    try:
        capfd.readouterr()
        assert api.lib.hipSpMVRowsCSR(C.byref(dm.handle), v.ptr, api.CONFIG(), v.ptr) == 1
        assert "libspmvhip" in capfd.readouterr().err
    finally:
        v.free()


# --------------------------------------------------------------------------------------------------------------- inputs
def _long_rows():
    """3000 rows, one past 256 and one past 2048 entries: the row blocks of the LDS-stream kernel take their long-row
    path, the tiles / stripes / SELL builds their long-row lists"""
    rng = np.random.default_rng(4101)
    M = N = 3000
    lens = rng.integers(0, 9, M)
    lens[7], lens[1500] = 300, 2100
    IRP, JA, AS = random_csr(rng, M, N, lens)
    return M, N, IRP, JA, AS


def _selectable():
    """30 000 rows of 9 sorted entries: 270 000 entries, past the 2^18 below which the selections build no format"""
    rng = np.random.default_rng(4121)
    M = N = 30000
    JA = np.sort(rng.integers(0, N, size=(M, 9)), axis=1).astype(np.uint64).ravel()
    return M, N, np.arange(M + 1, dtype=np.uint64) * 9, JA, rng.uniform(-1, 1, JA.size)


def _small():
    """500 x 400 with short rows (two empty): what the ELL forms and the derived handles are made from"""
    rng = np.random.default_rng(4102)
    M, N = 500, 400
    lens = rng.integers(1, 9, M)
    lens[[0, 499]] = 0
    IRP, JA, AS = random_csr(rng, M, N, lens)
    return M, N, IRP, JA, AS


def _square(seed=4103, M=600):
    """square, a full diagonal, sorted columns, diagonally dominant: the triangles, ILU(0), the Krylov solves"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 7, M)
    rows = np.repeat(np.arange(M), lens)
    cols = rng.integers(0, M, rows.size)
    rows, cols = np.concatenate([rows, np.arange(M)]), np.concatenate([cols, np.arange(M)])
    key = np.unique(rows * M + cols)
    rows, cols = key // M, key % M
    AS = rng.uniform(-1, 1, rows.size)
    AS[rows == cols] = 8.0 + rng.uniform(0, 1, M)
    IRP = np.zeros(M + 1, np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return M, M, IRP, cols.astype(np.uint64), AS


def _triangle(A, lower):
    M, _, IRP, JA, AS = A
    rows = np.repeat(np.arange(M), np.diff(IRP.astype(np.int64)))
    keep = JA.astype(np.int64) <= rows if lower else JA.astype(np.int64) >= rows
    irp = np.zeros(M + 1, np.uint64)
    irp[1:] = np.cumsum(np.bincount(rows[keep], minlength=M))
    return M, M, irp, JA[keep], AS[keep]


def _spd():
    """the 7-point Laplacian on 8 x 7 x 6: symmetric positive definite, for CG"""
    return sr.laplacian7(8, 7, 6)


def _grid():
    """the 2-D Laplacian on 16 x 12: three levels with coarseRows = 8"""
    return sr.laplacian7(16, 12, 1)


AMG_OPTS = dict(coarseRows=8)


# ------------------------------------------------------------------------------------------------------- the operations
class Op:
    """One entry of the table.  make() builds the inputs and returns the sources [(DeviceMatrix, x)]; fresh() the
    destination of one call; call(dst) makes the call and returns its status; untouched(dst) is invariant 3 (no launch),
    still_lawful(dst) invariant 5; result(dst) the bytes a successful call left; reference(dst) compares them, once, with
    the existing reference; drop(dst) and free() give everything back."""
    name = path = ""
    fallback = False                     # the header says the call falls back: it may succeed under a refusal
    nothing_left = True                  # a refused call leaves the ledger where it was at once

    def __init__(self, api, oracle, capfd):
        self.api, self.lib, self.oracle, self.capfd = api, api.lib, oracle, capfd

    def make(self):
        return []

    def still_lawful(self, dst):
        pass

    def may_stay(self, dst):
        """what a refused call may leave on the ledger, as (allocations, bytes) above the level before the call"""
        return [(0, 0)]

    refusing = -1                        # the allocation the driver is refusing (for what an entry wants to report)

    def note(self):
        """what the entry measured besides N, for the line the driver prints"""
        return ""

    def free(self):
        pass


class NewHandle(Op):
    """a call that makes a new CSR handle: the destination is zeroed, the info struct (if any) patterned; a refusal leaves
    both as they were and nothing behind"""
    info_kind = None
    irp = np.uint32

    def fresh(self):
        return self.api.DeviceMatrix(), (_patterned(self.info_kind) if self.info_kind else None)

    def info_ref(self, dst):
        return C.byref(dst[1]) if dst[1] is not None else None

    def untouched(self, dst):
        assert _handle_bytes(dst[0]) == bytes(C.sizeof(dst[0].handle)), "the zeroed destination handle was written"
        assert dst[1] is None or _is_patterned(dst[1]), "info was written"

    def still_lawful(self, dst):
        _not_live_is_refused(self.api, dst[0], self.capfd)

    def result(self, dst):
        IRP, JA, AS = _csr_arrays(self.api, dst[0], self.irp)
        h = dst[0].handle
        y = _product(self.api, ROWS, dst[0], _x(11, int(h.N)), int(h.M))
        return _blob((np.array([h.M, h.N, h.NZ], np.uint64), IRP, JA, AS, y))

    def reference(self, dst):
        M, N, IRP, JA, AS = self.expected()
        want = _blob((np.array([M, N, JA.size], np.uint64), np.asarray(IRP, np.uint64), np.asarray(JA, np.uint64), np.asarray(AS, np.float64),
                      self.oracle.csr_serial(IRP, JA, AS, _x(11, N))))
        got = self.result(dst)
        for g, w, what in zip(got, want, ("shape", "IRP", "JA", "AS", "product")):
            assert g == w, f"{self.name}: {what} differs from the reference"

    def drop(self, dst):
        dst[0].free()


class CpyCSR(NewHandle):
    name, path = "spMatCpyCSR", "row pointers, columns, values, row lengths, the row blocks with two long rows"

    def make(self):
        self.A = _long_rows()
        self.host = self.api.HostCSR(*self.A)
        return []

    def call(self, dst):
        return self.lib.spMatCpyCSR(C.byref(self.host.struct), C.byref(dst[0].handle))

    def expected(self):
        return self.A


class Adopt(NewHandle):
    path = "the row blocks over the caller's arrays (row pointers read back from the device)"

    def __init__(self, width, *a):
        super().__init__(*a)
        self.width, self.name = width, f"spmvHipAdoptCSR[{width}-byte row pointers]"
        self.irp = np.uint64 if width == 8 else np.uint32

    def make(self):
        self.A = M, N, IRP, JA, AS = _long_rows()
        arrays = (IRP.astype(self.irp), JA.astype(np.uint32), np.ascontiguousarray(AS))
        self.bufs = [self.api.DeviceBuffer(v.nbytes).up(v) for v in arrays]
        return []

    def call(self, dst):
        M, N, IRP, JA, AS = self.A
        return self.lib.spmvHipAdoptCSR(C.byref(dst[0].handle), M, N, JA.size, self.bufs[0].ptr, self.width, self.bufs[1].ptr,
                                        self.bufs[2].ptr, None)

    def expected(self):
        return self.A

    def free(self):
        for b in self.bufs:
            b.free()


class Ell(Op):
    """the ELL forms: the product of the form's own serial-order launcher is the result (row lengths kept: sgemvSerial's
    bits but for the sign of an empty row's zero)"""
    def make(self):
        self.A = M, N, IRP, JA, AS = _small()
        self.x = _x(12, N)
        self.host = self.api.HostCSR(M, N, IRP, JA, AS)
        return self.more()

    def more(self):
        return []

    def fresh(self):
        return self.api.DeviceMatrix()

    def untouched(self, dst):
        assert _handle_bytes(dst) == bytes(C.sizeof(dst.handle)), "the zeroed destination handle was written"

    def still_lawful(self, dst):
        _not_live_is_refused(self.api, dst, self.capfd)

    def result(self, dst):
        return _blob((_product(self.api, self.launcher, dst, self.x, self.A[0]),))

    def reference(self, dst):
        M, N, IRP, JA, AS = self.A
        assert_same_bits(_product(self.api, self.launcher, dst, self.x, M), self.oracle.csr_serial(IRP, JA, AS, self.x) + 0.0, self.name)

    def drop(self, dst):
        dst.free()


class CpyELL(Ell):
    def __init__(self, transposed, *a):
        super().__init__(*a)
        self.transposed = transposed
        self.name = "spMatCpyELL[" + ("column-major" if transposed else "row-major") + "]"
        self.path = "columns, values, row lengths of the padded arrays"
        self.launcher = "hipSpMVRowsELL" if transposed else "hipSpMVRowsELLNNTransposed"

    def more(self):
        ell = self.host.to_ell(with_row_lens=True)
        self.ell = ell.transpose() if self.transposed else ell
        return []

    def call(self, dst):
        return self.lib.spMatCpyELL(C.byref(self.ell.struct), C.byref(dst.handle))


class CsrToEll(Ell):
    def __init__(self, transposed, *a):
        super().__init__(*a)
        self.transposed = transposed
        self.name = "spmvHipCsrToEll[" + ("column-major" if transposed else "row-major") + "]"
        self.path = "the three arrays of the device-side conversion"
        self.launcher = "hipSpMVRowsELL" if transposed else "hipSpMVRowsELLNNTransposed"

    def more(self):
        self.src = self.api.spMatCpyCSR(self.host)
        return [(self.src, self.x)]

    def call(self, dst):
        return self.lib.spmvHipCsrToEll(C.byref(self.src.handle), 1 if self.transposed else 0, C.byref(dst.handle))

    def free(self):
        self.src.free()


class Format(Op):
    """a private format built on a fresh handle: a refusal leaves the handle a lawful CSR handle without that format and
    nothing behind; the retry builds it and its launcher gives the oracle's bits (a deterministic form) or sums within the
    exact any-order bound"""
    exact = False

    def make(self):
        self.A = M, N, IRP, JA, AS = _long_rows()
        self.x = _x(13, N)
        self.host = self.api.HostCSR(M, N, IRP, JA, AS)
        self.y_ref = self.oracle.csr_serial(IRP, JA, AS, self.x)
        return []

    def fresh(self):
        return self.api.spMatCpyCSR(self.host)

    def untouched(self, dst):
        assert self.built(dst) == 0, "a refused build left a format on the handle"

    def still_lawful(self, dst):
        self.api.set_variant(ROWS, 0)                                  # the restatement: no format is built by asking
        assert_same_bits(_product(self.api, ROWS, dst, self.x, self.A[0]), self.y_ref, self.name + ": the CSR handle after a refused build")
        self.api.set_variant(ROWS, 2)

    def result(self, dst):
        assert self.built(dst) > 0
        y = _product(self.api, self.launcher, dst, self.x, self.A[0])
        M, N, IRP, JA, AS = self.A
        if self.exact:
            return _blob((y,))
        check_any_order(IRP, JA, AS, self.x, y, self.name)
        return ()

    def reference(self, dst):
        if self.exact:
            assert_same_bits(_product(self.api, self.launcher, dst, self.x, self.A[0]), self.y_ref, self.name)
        else:
            self.result(dst)

    def drop(self, dst):
        dst.free()


class Tiles(Format):
    launcher = "hipSpMVTilesCSR"

    def __init__(self, det, *a):
        super().__init__(*a)
        self.det, self.exact = det, bool(det)
        self.name = "spmvHipBuildTiles[" + ("deterministic" if det else "arrival order") + "]"
        self.path = "slab, payload, tile lists, work list, the long rows' runs, the product workspace" + (", the product index" if det else "")

    def call(self, dst):
        o = self.api.spmvTilesOpts(deterministic=self.det)
        return self.lib.spmvHipBuildTilesOpt(C.byref(dst.handle), C.byref(o))

    def built(self, dst):
        return _formats(self.api, dst)[0]

    def may_stay(self, dst):
        return [(0, 0), (1, 8 * self.A[3].size)]                   # the device's product workspace, once grown, is the library's


class Stripes(Format):
    launcher = "hipSpMVStripesCSR"

    def __init__(self, det, *a):
        super().__init__(*a)
        self.det, self.exact = det, bool(det)
        self.name = "spmvHipBuildStripes[" + ("owner wavefronts" if det else "arrival order") + "]"
        self.path = "bin rows, sub-streams, cells" + (", the owner layout" if det else "")

    def call(self, dst):
        o = self.api.spmvStripesOpts(deterministic=self.det)
        return self.lib.spmvHipBuildStripesOpt(C.byref(dst.handle), C.byref(o))

    def built(self, dst):
        return _formats(self.api, dst)[1]


class Sell(Format):
    launcher, name, path = "hipSpMVRowsSELL", "hipSpMVRowsSELL's build (spmvHipBuildSell)", "permutation, slice lengths and offsets, values, columns, long rows"

    def call(self, dst):
        return self.lib.spmvHipBuildSell(C.byref(dst.handle))

    def built(self, dst):
        return _formats(self.api, dst)[2]


class FirstCall(Op):
    """the first call of a reference-named launcher: its selection builds and times the candidates, skips a format it
    cannot build and falls back to the kernel that needs no memory of its own (the header's exception)"""
    fallback, nothing_left = True, False

    def __init__(self, launcher, *a):
        super().__init__(*a)
        self.launcher, self.name = launcher, f"the first {launcher}"
        self.path = "the candidates' formats of the selection, each of which may be skipped"

    def make(self):
        self.A = M, N, IRP, JA, AS = _selectable()
        self.x = _x(14, N)
        self.host = self.api.HostCSR(M, N, IRP, JA, AS)
        self.y_ref = self.oracle.csr_serial(IRP, JA, AS, self.x)
        self.dx, self.dy = self.api.DeviceVector(N).up(self.x), self.api.DeviceVector(M)
        return []

    def fresh(self):
        self.dy.poison()
        return self.api.spMatCpyCSR(self.host)

    def call(self, dst):
        return getattr(self.lib, self.launcher)(C.byref(dst.handle), self.dx.ptr, self.api.CONFIG(), self.dy.ptr)

    def untouched(self, dst):
        pass

    def check(self, y):
        M, N, IRP, JA, AS = self.A
        if self.launcher == ROWS:
            assert_same_bits(y, self.y_ref, self.name)
        else:
            check_any_order(IRP, JA, AS, self.x, y, self.name)

    def result(self, dst):
        self.check(self.dy.down())
        return ()

    def reference(self, dst):
        self.result(dst)

    def still_lawful(self, dst):
        self.dy.poison()

    def drop(self, dst):
        dst.free()

    def free(self):
        self.dx.free()
        self.dy.free()


class UpdateValues(Op):
    """spmvHipUpdateValues on a handle with every format built.  The header's promise for a failure: the handle stays
    live, its CSR values are the new ones or the old ones, a built format may hold either until the call is made again;
    the same call made again brings everything to the new values."""
    name, path, nothing_left = "spmvHipUpdateValues", "the value maps of both tile forms, both stripe layouts and SELL, the unit flag", False

    def make(self):
        self.A = M, N, IRP, JA, AS = _long_rows()
        self.x = _x(15, N)
        self.host = self.api.HostCSR(M, N, IRP, JA, AS)
        self.AS2 = np.ascontiguousarray(np.random.default_rng(4104).uniform(-1, 1, AS.size))
        self.y_new = self.oracle.csr_serial(IRP, JA, self.AS2, self.x)
        return []

    def fresh(self):
        d = self.api.spMatCpyCSR(self.host)
        for det in (0, 1):
            self.api.build_tiles(d, deterministic=det)
            self.api.build_stripes(d, deterministic=det)
        assert self.lib.spmvHipBuildSell(C.byref(d.handle)) == 0
        self.formats = _formats(self.api, d)
        return d

    def call(self, dst):
        return self.lib.spmvHipUpdateValues(C.byref(dst.handle), self.AS2.ctypes.data_as(C.c_void_p), 0)

    def untouched(self, dst):
        assert dst.handle.dev and all(v > 0 for v in _formats(self.api, dst)), "a refused update dropped the handle or a format"

    def result(self, dst):
        M, N, IRP, JA, AS = self.A
        out = [_csr_arrays(self.api, dst)[2]]
        for launcher in ("hipSpMVTilesCSR", "hipSpMVStripesCSR"):      # (the preferred form is the last one built: the deterministic one)
            out.append(_product(self.api, launcher, dst, self.x, M))
        check_any_order(IRP, JA, self.AS2, self.x, _product(self.api, "hipSpMVRowsSELL", dst, self.x, M), self.name + ": SELL")
        return _blob(out)

    def reference(self, dst):
        values, tiles, stripes = self.result(dst)
        assert values == self.AS2.tobytes()
        assert tiles == self.y_new.tobytes() and stripes == self.y_new.tobytes(), "a deterministic form after the update"

    def drop(self, dst):
        dst.free()


class Derived(NewHandle):
    """a handle made from other handles: the sources are the table's invariant-4 subjects"""
    def make(self):
        self.mats = self.inputs()
        self.src = [self.api.spMatCpyCSR(self.api.HostCSR(*A)) for A in self.mats]
        return [(d, _x(16 + i, A[1])) for i, (d, A) in enumerate(zip(self.src, self.mats))]

    def free(self):
        for d in self.src:
            d.free()


class Transpose(Derived):
    name, path = "spmvHipCsrTranspose", "the four arrays, the sort's keys and workspace, the row blocks"

    def inputs(self):
        return [_small()]

    def call(self, dst):
        return self.lib.spmvHipCsrTranspose(C.byref(self.src[0].handle), C.byref(dst[0].handle))

    def expected(self):
        M, N, IRP, JA, AS = self.mats[0]
        IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, AS)
        return N, M, IRPt, JAt, ASt


class Permute(Derived):
    name, path = "spmvHipCsrPermute", "the inverse permutation, the four arrays, the sort"

    def inputs(self):
        return [_square()]

    def make(self):
        out = super().make()
        M = self.mats[0][0]
        self.perm = np.random.default_rng(4105).permutation(M).astype(np.uint32)
        self.dperm = self.api.DeviceBuffer(4 * M).up(self.perm)
        return out

    def call(self, dst):
        return self.lib.spmvHipCsrPermute(C.byref(self.src[0].handle), self.dperm.ptr, C.byref(dst[0].handle))

    def expected(self):
        M, N, IRP, JA, AS = self.mats[0]
        irp, ja, a, _ = cl.permute_ref(M, IRP, JA, AS, self.perm)
        return M, M, irp, ja, a

    def free(self):
        super().free()
        self.dperm.free()


class Spgemm(Derived):
    name = "spmvHipSpGEMM"
    path = "rows in each class: wavefront table, workgroup table, the sorted longest rows (limits lowered to 8 and 64 products)"

    def __init__(self, *a):
        super().__init__(*a)
        self.info_kind = self.api.spmvSpgemmInfo

    def inputs(self):
        rng = np.random.default_rng(4106)
        M, K, N = 200, 150, 180
        lens = rng.integers(0, 5, M)
        lens[3], lens[90] = 30, 120                              # x rows of B of up to 6: past 8, past 64 products
        IRP, JA, AS = random_csr(rng, M, K, lens)
        IRPb, JAb, ASb = random_csr(rng, K, N, rng.integers(1, 7, K))
        return [(M, K, IRP, JA, AS), (K, N, IRPb, JAb, ASb)]

    def call(self, dst):
        o = self.api.spmvSpgemmOpts(8, 64, 0)
        return self.lib.spmvHipSpGEMM(C.byref(self.src[0].handle), C.byref(self.src[1].handle), C.byref(o), C.byref(dst[0].handle),
                                      self.info_ref(dst))

    def expected(self):
        return sr.spgemm_ref(*self.mats)

    def reference(self, dst):
        super().reference(dst)
        i = dst[1]
        assert i.rowsWave > 0 and i.rowsGroup > 0 and i.rowsSorted > 0, "the input is there for all three classes"


class Add(Derived):
    name = "spmvHipCsrAdd"
    path = "rows in each class: merge by lane, ranks by wavefront, the sorted path (limits lowered to 4 and 16 terms)"

    def __init__(self, *a):
        super().__init__(*a)
        self.info_kind = self.api.spmvAddInfo

    def inputs(self):
        rng = np.random.default_rng(4107)
        M, N = 300, 250
        la, lb = rng.integers(0, 3, M), rng.integers(0, 3, M)
        la[5], lb[5], la[200], lb[200] = 6, 6, 40, 30
        return [(M, N) + random_csr(rng, M, N, la), (M, N) + random_csr(rng, M, N, lb)]

    def call(self, dst):
        o = self.api.spmvAddOpts(4, 16, 0, 0)
        return self.lib.spmvHipCsrAdd(1.5, C.byref(self.src[0].handle), -0.25, C.byref(self.src[1].handle), C.byref(o), C.byref(dst[0].handle),
                                      self.info_ref(dst))

    def expected(self):
        return adr.add_ref(1.5, self.mats[0], -0.25, self.mats[1])

    def reference(self, dst):
        super().reference(dst)
        i = dst[1]
        assert i.rowsLane > 0 and i.rowsWave > 0 and i.rowsSorted > 0, "the input is there for all three classes"


class Filter(Derived):
    def __init__(self, mode, *a):
        super().__init__(*a)
        self.mode, self.info_kind = mode, self.api.spmvFilterInfo
        self.name = f"spmvHipCsrFilter[{mode}]"
        self.path = {"band": "the pattern-only predicate", "abs": "the tolerance", "strength": "the diagonal places, the keep mask, lumping"}[mode]
        self.o = {"band": fr.opts(fr.BAND, lo=-3, hi=40), "abs": fr.opts(fr.ABS, theta=0.4),
                  "strength": fr.opts(fr.STRENGTH, theta=0.1, lump=True)}[mode]

    def inputs(self):
        return [_square(4108)]

    def call(self, dst):
        o = self.o
        opts = self.api.spmvFilterOpts(o["mode"], o["lo"], o["hi"], o["theta"], int(o["lump"]))
        return self.lib.spmvHipCsrFilter(C.byref(self.src[0].handle), C.byref(opts), C.byref(dst[0].handle), self.info_ref(dst))

    def expected(self):
        return fr.filter_ref(self.mats[0], self.o)[0]


class Refresh(Op):
    """the value refresh of a derived handle.  The source gets new values AFTER the derived handle was made, so a refresh
    has something to bring over.  The header's promise for a failure: info untouched, the handle stays live with its
    pattern and addresses, its values may be the old or the new ones, and the same call made again completes it."""
    nothing_left = False

    def __init__(self, maker, *a):
        super().__init__(*a)
        self.m = maker
        self.name, self.path = maker.name + "'s refresh", "the unit flag, the numeric phase's temporaries"

    def make(self):
        out = self.m.make()
        rng = np.random.default_rng(4109)
        self.old = [A[4] for A in self.m.mats]
        self.new = [np.ascontiguousarray(np.where(A[4] > 7.0, A[4] + 1.0, rng.uniform(-1, 1, A[4].size))) for A in self.m.mats]
        for d, v in zip(self.m.src, self.new):
            d.update_values(v)
        return out

    def fresh(self):
        for d, v in zip(self.m.src, self.old):
            d.update_values(v)
        dst = self.m.fresh()
        assert self.m.call(dst) == 0
        for d, v in zip(self.m.src, self.new):
            d.update_values(v)
        info = _patterned(self.m.info_kind) if self.m.info_kind else None
        return dst[0], info, _handle_bytes(dst[0])

    def call(self, dst):
        d, info, _ = dst
        s = [C.byref(x.handle) for x in self.m.src]
        i = C.byref(info) if info is not None else None
        if isinstance(self.m, Transpose):
            return self.lib.spmvHipTransposeRefresh(C.byref(d.handle), s[0])
        if isinstance(self.m, Permute):
            return self.lib.spmvHipPermuteRefresh(C.byref(d.handle), s[0])
        if isinstance(self.m, Spgemm):
            return self.lib.spmvHipSpGEMMRefresh(C.byref(d.handle), s[0], s[1], i)
        if isinstance(self.m, Add):
            return self.lib.spmvHipCsrAddRefresh(C.byref(d.handle), 1.5, s[0], -0.25, s[1], i)
        return self.lib.spmvHipCsrFilterRefresh(C.byref(d.handle), s[0], i)

    def untouched(self, dst):
        d, info, before = dst
        assert _handle_bytes(d) == before, "a refused refresh changed the handle's pattern or addresses"
        assert info is None or isinstance(self.m, (Transpose, Permute)) or _is_patterned(info), "info was written"

    def result(self, dst):
        return self.m.result((dst[0], None))

    def reference(self, dst):
        mats = [A[:4] + (v,) for A, v in zip(self.m.mats, self.new)]
        keep, self.m.mats = self.m.mats, mats
        try:
            if isinstance(self.m, Filter):                          # the build's kept set on the new values
                kept = fr.filter_ref(keep[0], self.m.o)[1]
                want = fr.filter_refresh_ref(kept, mats[0], self.m.o)
                self.m.expected = lambda: want
            NewHandle.reference(self.m, (dst[0], None))
        finally:
            self.m.mats = keep
            if isinstance(self.m, Filter):
                del self.m.expected

    def drop(self, dst):
        dst[0].free()

    def free(self):
        self.m.free()


class Colour(Op):
    name, path = "spmvHipColourCSR", "the incoming pattern's sort, the rounds' state, the permutation's sort"

    def make(self):
        self.A = M, N, IRP, JA, AS = _square(4110)
        self.src = self.api.spMatCpyCSR(self.api.HostCSR(M, N, IRP, JA, AS))
        self.bufs = [self.api.DeviceBuffer(4 * M), self.api.DeviceBuffer(4 * M)]
        return [(self.src, _x(17, N))]

    def fresh(self):
        for b in self.bufs:
            b.up(np.full(self.A[0], 0xA5A5A5A5, np.uint32))
        return _patterned(self.api.spmvColourInfo)

    def call(self, dst):
        o = self.api.spmvColourOpts(self.api.SPMV_COLOUR_HASH, 5)
        return self.lib.spmvHipColourCSR(C.byref(self.src.handle), C.byref(o), self.bufs[0].ptr, self.bufs[1].ptr, C.byref(dst))

    written = None

    def untouched(self, dst):                                      # (the header: after a failed allocation dColour and dPerm hold nothing to rely on)
        assert _is_patterned(dst), "info was written"
        if self.written is None and any(np.any(b.down(np.uint32) != 0xA5A5A5A5) for b in self.bufs):
            self.written = self.refusing

    def note(self):
        return f" | the output arrays are first found written at n = {self.written}"

    def result(self, dst):
        return _blob((self.bufs[0].down(np.uint32), self.bufs[1].down(np.uint32), np.array([dst.colours])))

    def reference(self, dst):
        M, N, IRP, JA, AS = self.A
        colour, _ = cl.colour_ref(M, IRP, JA, self.api.SPMV_COLOUR_HASH, 5)
        assert np.array_equal(self.bufs[0].down(np.uint32), np.asarray(colour, np.uint32))
        assert np.array_equal(self.bufs[1].down(np.uint32), cl.perm_of(colour))

    def drop(self, dst):
        pass

    def free(self):
        self.src.free()
        for b in self.bufs:
            b.free()


class Trsv(Op):
    """the first hipSpTRSVCSR of a triangle: the analysis.  A refusal leaves x untouched and no schedule on the handle."""
    def __init__(self, lower, *a):
        super().__init__(*a)
        self.lower, self.name = lower, "the first hipSpTRSVCSR[" + ("lower" if lower else "upper") + "]"
        self.path = "permutation, diagonal places, level counts, the level table, the sorts"

    def make(self):
        self.T = M, N, IRP, JA, AS = _triangle(_square(4111, 500), self.lower)
        self.host = self.api.HostCSR(M, N, IRP, JA, AS)
        self.b = np.random.default_rng(4112).standard_normal(M)
        self.db, self.dx = self.api.DeviceVector(M).up(self.b), self.api.DeviceVector(M)
        return []

    def fresh(self):
        self.dx.poison()
        return self.api.spMatCpyCSR(self.host)

    def call(self, dst):
        uplo = self.api.SPMV_TRI_LOWER if self.lower else self.api.SPMV_TRI_UPPER
        return self.lib.hipSpTRSVCSR(C.byref(dst.handle), uplo, self.api.SPMV_DIAG_STORED, self.db.ptr, self.dx.ptr)

    def untouched(self, dst):
        assert np.isnan(self.dx.down()).all(), "x was written"
        assert dst.triangular_info(self.lower).analyses == 0, "a refused analysis left a schedule"

    def still_lawful(self, dst):
        M, N, IRP, JA, AS = self.T
        x = _x(18, N)
        assert_same_bits(_product(self.api, ROWS, dst, x, M), self.oracle.csr_serial(IRP, JA, AS, x), self.name + ": the handle's product")

    def result(self, dst):
        return _blob((self.dx.down(),))

    def reference(self, dst):
        M, N, IRP, JA, AS = self.T
        assert_same_bits(self.dx.down(), np.array(trsv_ref.trsv_loop(M, IRP, JA, AS, self.b, self.lower, False)), self.name)

    def drop(self, dst):
        dst.free()

    def free(self):
        self.db.free()
        self.dx.free()


class Ilu0(Op):
    """hipSpILU0CSR works in place.  The header's promise for a failure: AS untouched bit for bit -- or, when it was the
    last step that failed (the unit flag and the formats after the factorisation), the complete factors, never a mixture;
    the same call made again then only finishes the handle (the retry's bits would show a second factorisation)."""
    name, path = "hipSpILU0CSR", "the pattern check's flag, the lower triangle's analysis, the zero-pivot words, the unit flag after the factorisation"

    def make(self):
        self.A = M, N, IRP, JA, AS = _square(4113, 500)
        self.host = self.api.HostCSR(M, N, IRP, JA, AS)
        return []

    def fresh(self):
        return self.api.spMatCpyCSR(self.host)

    def call(self, dst):
        return self.lib.hipSpILU0CSR(C.byref(dst.handle))

    def untouched(self, dst):
        got = _csr_arrays(self.api, dst)[2].tobytes()
        if got != np.ascontiguousarray(self.A[4]).tobytes():
            assert got == self.factors.tobytes(), "a refused factorisation left AS neither as it was nor as the complete factors"

    def may_stay(self, dst):
        return [(0, 0), (3, int(dst.triangular_info(True).bytes))]   # the lower triangle's schedule, once made, stays on the handle

    def result(self, dst):
        return _blob((_csr_arrays(self.api, dst)[2],))

    def reference(self, dst):
        M, N, IRP, JA, AS = self.A
        self.factors = np.array(ilu0_ref.ilu0_loop(M, IRP, JA, AS))
        assert_same_bits(_csr_arrays(self.api, dst)[2], self.factors, self.name)

    def drop(self, dst):
        dst.free()


class Dot(Op):
    name, path = "spmvHipDot", "the dot workspace grows from nothing to the block partials of n"

    def make(self):
        rng = np.random.default_rng(4114)
        self.n = 3 * 4096 + 17
        self.u, self.v = rng.standard_normal(self.n), rng.standard_normal(self.n)
        self.du, self.dv = self.api.DeviceVector(self.n).up(self.u), self.api.DeviceVector(self.n).up(self.v)
        self.out = self.api.DeviceVector(1)
        return []

    def fresh(self):
        self.out.poison()
        return None

    def call(self, dst):
        return self.lib.spmvHipDot(self.n, self.du.ptr, self.dv.ptr, self.out.ptr)

    def untouched(self, dst):
        assert np.isnan(self.out.down()).all(), "the result was written"

    def result(self, dst):
        return _blob((self.out.down(),))

    def reference(self, dst):
        assert_same_bits(self.out.down(), np.array([dot_ref(self.u, self.v)]), self.name)

    def drop(self, dst):
        pass

    def free(self):
        for v in (self.du, self.dv, self.out):
            v.free()


class MultiDot(Dot):
    name, path = "spmvHipMultiDot", "the dot workspace grows from nothing to k blocks-of-n partials"

    def make(self):
        rng = np.random.default_rng(4122)
        self.n, self.k = 2 * 4096 + 5, 5
        self.V, self.w = rng.standard_normal((self.n, self.k)), rng.standard_normal(self.n)
        self.du = self.api.DeviceVector(self.n * self.k).up(np.asfortranarray(self.V).ravel(order="F"))
        self.dv = self.api.DeviceVector(self.n).up(self.w)
        self.out = self.api.DeviceVector(8)
        return []

    def call(self, dst):
        return self.lib.spmvHipMultiDot(self.n, self.k, self.du.ptr, self.n, self.dv.ptr, self.out.ptr)

    def reference(self, dst):
        assert_same_bits(self.out.down()[:self.k], multi_dot_ref(self.V, self.w), self.name)


class BlockDot(Dot):
    name, path = "spmvHipBlockDot", "the dot workspace grows from nothing to k blocks-of-n partials"

    def make(self):
        rng = np.random.default_rng(4123)
        self.n, self.k = 2 * 4096 + 5, 3
        self.U, self.V = rng.standard_normal((self.n, self.k)), rng.standard_normal((self.n, self.k))
        self.du = self.api.DeviceVector(self.n * self.k).up(self.U.ravel())                       # row-major
        self.dv = self.api.DeviceVector(self.n * self.k).up(np.asfortranarray(self.V).ravel(order="F"))   # column-major
        self.out = self.api.DeviceVector(8)
        return []

    def call(self, dst):
        return self.lib.spmvHipBlockDot(self.n, self.k, self.du.ptr, self.k, self.api.SPMV_DENSE_ROW_MAJOR, self.dv.ptr, self.n,
                                        self.api.SPMV_DENSE_COL_MAJOR, self.out.ptr)

    def reference(self, dst):
        assert_same_bits(self.out.down()[:self.k], block_dot_ref(self.U, self.V), self.name)


class Trsm(Trsv):
    """the first hipSpTRSMCSR of a triangle: the same analysis, X untouched by a refusal"""
    def __init__(self, *a):
        super().__init__(True, *a)
        self.name = "the first hipSpTRSMCSR[lower]"

    def make(self):
        out = super().make()
        M, self.k = self.T[0], 3
        self.B = np.random.default_rng(4124).standard_normal((M, self.k))
        self.db.free()
        self.dx.free()
        self.db, self.dx = self.api.DeviceVector(M * self.k).up(self.B.ravel()), self.api.DeviceVector(M * self.k)
        return out

    def call(self, dst):
        rm = self.api.SPMV_DENSE_ROW_MAJOR
        return self.lib.hipSpTRSMCSR(C.byref(dst.handle), self.api.SPMV_TRI_LOWER, self.api.SPMV_DIAG_STORED, self.k, self.db.ptr, self.k, rm,
                                     self.dx.ptr, self.k, rm)

    def reference(self, dst):
        M, N, IRP, JA, AS = self.T
        X = self.dx.down().reshape(M, self.k)
        for c in range(self.k):
            assert_same_bits(X[:, c], np.array(trsv_ref.trsv_loop(M, IRP, JA, AS, self.B[:, c], True, False)), f"{self.name}: column {c}")


class Krylov(Op):
    """a Krylov solve: every allocation comes before the loop.  A refusal leaves x and info untouched."""
    def __init__(self, method, precond, *a):
        super().__init__(*a)
        self.method, self.precond = method, precond
        self.name = {"cg": "hipSpCGCSR", "bicgstab": "hipSpBiCGStabCSR", "gmres": "hipSpGMRESCSR"}[method] + ("[dM = ILU(0)]" if precond else "")
        self.path = "the solver's workspace, the dot workspace" + (", the factors' two analyses" if precond else "")

    def make(self):
        self.A = M, N, IRP, JA, AS = _spd() if self.method == "cg" else _square(4115, 400)
        self.src = self.api.spMatCpyCSR(self.api.HostCSR(M, N, IRP, JA, AS))
        self.b = np.random.default_rng(4116).standard_normal(M)
        self.db, self.dx = self.api.DeviceVector(M).up(self.b), self.api.DeviceVector(M)
        self.x0 = np.zeros(M)
        return [(self.src, _x(19, N))]

    def fresh(self):
        self.dx.up(self.x0)
        m = None
        if self.precond:                                              # a fresh factor handle: its analyses are part of the call
            m = self.api.spMatCpyCSR(self.api.HostCSR(*self.A))
            m.ilu0()
        return _patterned(self.api.spmvKrylovInfo), m

    def call(self, dst):
        info, m = dst
        mh = C.byref(m.handle) if m is not None else None
        if self.method == "gmres":
            o = self.api.spmvGmresOpts(1e-10, 200, 20, None)
            return self.lib.hipSpGMRESCSR(C.byref(self.src.handle), mh, self.db.ptr, self.dx.ptr, C.byref(o), C.byref(info))
        o = self.api.spmvKrylovOpts(1e-10, 200, None)
        fn = self.lib.hipSpCGCSR if self.method == "cg" else self.lib.hipSpBiCGStabCSR
        return fn(C.byref(self.src.handle), mh, self.db.ptr, self.dx.ptr, C.byref(o), C.byref(info))

    def untouched(self, dst):
        assert _is_patterned(dst[0]), "info was written"
        assert self.dx.down().tobytes() == self.x0.tobytes(), "x was written"

    def may_stay(self, dst):
        if dst[1] is None:
            return [(0, 0)]
        lo, up = (int(dst[1].triangular_info(w).bytes) for w in (True, False))     # a schedule that was made stays on the factor handle
        return [(0, 0)] + [(3, b) for b in (lo, up) if b] + ([(6, lo + up)] if lo and up else [])

    def result(self, dst):
        i = dst[0]
        return _blob((self.dx.down(), np.array([i.status, i.iterations]), np.array([i.rr, i.bb])))

    def reference(self, dst):
        M, N, IRP, JA, AS = self.A
        F = np.array(ilu0_ref.ilu0_loop(M, IRP, JA, AS)) if self.precond else None
        A = Csr(M, IRP, JA, AS, F)
        if self.method == "gmres":
            x, status, it, _, rr = gmres_ref(A, self.b, self.x0, 1e-10, 200, 20)
        else:
            x, status, it, _, rr = (cg_ref if self.method == "cg" else bicgstab_ref)(A, self.b, self.x0, 1e-10, 200)
        assert (dst[0].status, dst[0].iterations) == (status, it), self.name
        assert_same_bits(self.dx.down(), x, self.name)

    def drop(self, dst):
        if dst[1] is not None:
            dst[1].free()

    def free(self):
        self.src.free()
        self.db.free()
        self.dx.free()


class KrylovBlock(Krylov):
    """the two block solvers: k columns in lock step, column c with the single solve's bits"""
    def __init__(self, method, *a):
        super().__init__(method, False, *a)
        self.name = {"cg": "hipSpCGBlockCSR", "bicgstab": "hipSpBiCGStabBlockCSR"}[method]
        self.path = "the block workspace of k columns, the dot workspace"

    def make(self):
        out = super().make()
        M, self.k = self.A[0], 3
        self.B = np.random.default_rng(4125).standard_normal((M, self.k))
        self.db.free()
        self.dx.free()
        self.db, self.dx = self.api.DeviceVector(M * self.k).up(self.B.ravel()), self.api.DeviceVector(M * self.k)
        self.x0 = np.zeros(M * self.k)
        return out

    def fresh(self):
        self.dx.up(self.x0)
        cols = (self.api.spmvKrylovColumn * self.k)()
        C.memset(cols, PATTERN, C.sizeof(cols))
        return _patterned(self.api.spmvKrylovInfo), None, cols

    def call(self, dst):
        info, _, cols = dst
        o, rm = self.api.spmvKrylovOpts(1e-10, 200, None), self.api.SPMV_DENSE_ROW_MAJOR
        fn = self.lib.hipSpCGBlockCSR if self.method == "cg" else self.lib.hipSpBiCGStabBlockCSR
        return fn(C.byref(self.src.handle), None, self.k, self.db.ptr, self.k, rm, self.dx.ptr, self.k, rm, C.byref(o), cols, C.byref(info))

    def untouched(self, dst):
        super().untouched(dst)
        assert C.string_at(dst[2], C.sizeof(dst[2])) == bytes([PATTERN]) * C.sizeof(dst[2]), "the columns' records were written"

    def result(self, dst):
        i = dst[0]
        per = np.array([[c.status, c.iterations] for c in dst[2]])
        return _blob((self.dx.down(), np.array([i.status, i.iterations]), per))

    def reference(self, dst):
        M, N, IRP, JA, AS = self.A
        A = Csr(M, IRP, JA, AS)
        X = self.dx.down().reshape(M, self.k)
        for c in range(self.k):
            x, status, it, _, _ = (cg_ref if self.method == "cg" else bicgstab_ref)(A, self.B[:, c], np.zeros(M), 1e-10, 200)
            assert (dst[2][c].status, dst[2][c].iterations) == (status, it), f"{self.name}: column {c}"
            assert_same_bits(X[:, c], x, f"{self.name}: column {c}")


class Aggregate(Op):
    name, path = "spmvHipAggregateCSR", "the incoming pattern, the rounds' state"

    def make(self):
        self.A = M, N, IRP, JA, AS = _grid()
        self.src = self.api.spMatCpyCSR(self.api.HostCSR(M, N, IRP, JA, AS))
        self.buf = self.api.DeviceBuffer(4 * M)
        return [(self.src, _x(20, N))]

    def fresh(self):
        self.buf.up(np.full(self.A[0], 0xA5A5A5A5, np.uint32))
        return _patterned(self.api.spmvAggInfo)

    def call(self, dst):
        o = self.api.spmvAggOpts(3)
        return self.lib.spmvHipAggregateCSR(C.byref(self.src.handle), C.byref(o), self.buf.ptr, C.byref(dst))

    written = None

    def untouched(self, dst):                                      # (the header: after a failed allocation dAgg holds nothing to rely on)
        assert _is_patterned(dst), "info was written"
        if self.written is None and np.any(self.buf.down(np.uint32) != 0xA5A5A5A5):
            self.written = self.refusing

    def note(self):
        return f" | the ids are first found written at n = {self.written}"

    def result(self, dst):
        return _blob((self.buf.down(np.uint32), np.array([dst.aggregates])))

    def reference(self, dst):
        M, N, IRP, JA, AS = self.A
        assert np.array_equal(self.buf.down(np.uint32), ar.aggregate_ref(M, IRP, JA, 3))

    def drop(self, dst):
        pass

    def free(self):
        self.src.free()
        self.buf.free()


class AmgSetup(Op):
    """the three setups: a refusal leaves dM zeroed, info untouched and nothing behind; the retry's cycle has the
    reference's bits"""
    def __init__(self, kind, *a):
        super().__init__(*a)
        self.kind = kind
        self.name = {"plain": "spmvHipAmgSetup", "smoothed": "spmvHipAmgSetupSmoothed", "strength": "spmvHipAmgSetupStrength"}[kind]
        self.path = "three levels of the 16 x 12 Laplacian: aggregation, P, R, the two products per level, the level vectors" + \
            {"plain": "", "smoothed": ", the smoothed prolongator's sums", "strength": ", the filtered matrices"}[kind]

    def make(self):
        self.A = M, N, IRP, JA, AS = _grid()
        self.src = self.api.spMatCpyCSR(self.api.HostCSR(M, N, IRP, JA, AS))
        self.r = np.random.default_rng(4117).standard_normal(M)
        return [(self.src, _x(21, N))]

    def fresh(self):
        h = self.api.AmgHierarchy(self.src)
        C.memset(C.addressof(h.info), PATTERN, C.sizeof(h.info))
        return h

    def call(self, dst):
        o = self.api.spmvAmgOpts(0, AMG_OPTS["coarseRows"], 0, 0.0, 0, 0, 0)
        s, st = self.api.spmvAmgSmoothOpts(0.0), self.api.spmvAmgStrengthOpts(0.0, 0.0)
        a, d, i = C.byref(self.src.handle), C.byref(dst.handle), C.byref(dst.info)
        if self.kind == "plain":
            return self.lib.spmvHipAmgSetup(a, C.byref(o), d, i)
        if self.kind == "smoothed":
            return self.lib.spmvHipAmgSetupSmoothed(a, C.byref(o), C.byref(s), d, i)
        return self.lib.spmvHipAmgSetupStrength(a, C.byref(o), C.byref(s), C.byref(st), d, i)

    def untouched(self, dst):
        assert _handle_bytes(dst) == bytes(C.sizeof(dst.handle)), "the zeroed hierarchy handle was written"
        assert _is_patterned(dst.info), "info was written"

    def still_lawful(self, dst):
        _not_live_is_refused(self.api, dst, self.capfd)

    def result(self, dst):
        return _blob((dst.apply(self.r), np.array([dst.info.levels])))

    def cycle(self):
        if self.kind == "plain":
            levels, o = ar.setup_ref(self.A, **AMG_OPTS)
            return levels, ar.cycle_ref(levels, o, self.r)
        if self.kind == "smoothed":
            levels, o = sa.setup_ref(self.A, **AMG_OPTS)
            return levels, sa.cycle_ref(levels, o, self.r)
        levels, o = fr.strength_setup_ref(self.A, **AMG_OPTS)
        return levels, sa.cycle_ref(levels, o, self.r)

    def reference(self, dst):
        levels, z = self.cycle()
        assert dst.info.levels == len(levels) >= 3, "the input is there for three levels"
        assert_same_bits(dst.apply(self.r), z, self.name)

    def drop(self, dst):
        dst.free()

    def free(self):
        self.src.free()


class AmgChange(Op):
    """a call that changes a hierarchy in place.  The setters make everything new before anything old is dropped: after a
    refusal the cycle gives the bits it gave before.  The refresh's promise: the hierarchy stays live, and the same call
    made again completes it."""
    def __init__(self, what, *a):
        super().__init__(*a)
        self.what = what
        self.name = {"refresh": "spmvHipAmgRefresh", "chebyshev": "spmvHipAmgSetSmoother[Chebyshev]", "gs": "spmvHipAmgSetGaussSeidel",
                     "width": "spmvHipAmgSetBlockWidth[none -> 3]", "rewidth": "spmvHipAmgSetBlockWidth[2 -> 5]"}[what]
        self.path = {"refresh": "the products' numeric phases, the unit flags", "chebyshev": "the spectral radii's vectors, the coefficient tables",
                     "gs": "the colourings and colour lists of every level", "width": "the block workspace of every level",
                     "rewidth": "a new block workspace beside the old one"}[what]
        self.keeps_old = what != "refresh"
        self.nothing_left = self.keeps_old

    def make(self):
        self.A = M, N, IRP, JA, AS = _grid()
        self.src = self.api.spMatCpyCSR(self.api.HostCSR(M, N, IRP, JA, AS))
        self.r = np.random.default_rng(4118).standard_normal(M)
        self.R = np.random.default_rng(4119).standard_normal((M, 3))
        self.levels, self.o = ar.setup_ref(self.A, **AMG_OPTS)
        self.old = ar.cycle_ref(self.levels, self.o, self.r)
        if self.what == "refresh":
            self.AS2 = np.ascontiguousarray(AS * np.random.default_rng(4120).uniform(1.0, 1.5, 1)[0])
            self.src.update_values(self.AS2)
        return [(self.src, _x(22, N))]

    def fresh(self):
        if self.what == "refresh":
            self.src.update_values(self.A[4])
        h = self.src.amg(**AMG_OPTS)
        if self.what == "rewidth":
            h.set_block_width(2)
        if self.what == "refresh":
            self.src.update_values(self.AS2)
        return h

    def call(self, dst):
        a, d = C.byref(self.src.handle), C.byref(dst.handle)
        if self.what == "refresh":
            return self.lib.spmvHipAmgRefresh(d, a)
        if self.what == "chebyshev":
            o = self.api.spmvAmgSmootherOpts(self.api.SPMV_AMG_SMOOTHER_CHEBYSHEV, 0, 0, 0, 0.0, 0.0)
            return self.lib.spmvHipAmgSetSmoother(d, a, C.byref(o))
        if self.what == "gs":
            o = self.api.spmvAmgGsOpts(self.api.SPMV_COLOUR_NATURAL, 0, 0.0, 0, 0, 0, 0, 0)
            return self.lib.spmvHipAmgSetGaussSeidel(d, a, C.byref(o))
        return self.lib.spmvHipAmgSetBlockWidth(d, a, 3 if self.what == "width" else 5)

    def untouched(self, dst):
        assert dst.handle.dev, "a refused call dropped the hierarchy"
        if self.what in ("width", "rewidth"):
            assert dst.block_info()["width"] == (0 if self.what == "width" else 2), "a refused width change changed the width"

    def still_lawful(self, dst):
        if self.keeps_old:
            assert_same_bits(dst.apply(self.r), self.old, self.name + ": the cycle after a refused setter")
        if self.what == "rewidth":
            Z = dst.apply_block(self.R[:, :2].copy())
            for c in range(2):
                assert_same_bits(Z[:, c], dst.apply(self.R[:, c].copy()), self.name + ": the old workspace's block cycle")

    def result(self, dst):
        if self.what in ("width", "rewidth"):
            return _blob((dst.apply_block(self.R), np.array([dst.block_info()["width"]])))
        return _blob((dst.apply(self.r),))

    def reference(self, dst):
        if self.what == "refresh":
            levels, o = ar.setup_ref(self.A[:4] + (self.AS2,), **AMG_OPTS)
            want = ar.cycle_ref(levels, o, self.r)
        elif self.what == "chebyshev":
            levels, o = cb.setup_ref(self.A, "plain", **AMG_OPTS)
            want = cb.cycle_ref(levels, o, self.r, cb.smoother(o))
        elif self.what == "gs":
            levels, o = gr.setup_ref(self.A, "plain", **AMG_OPTS)
            want = gr.cycle_ref(levels, o, self.r, gr.smoother(o))
        else:
            Z = dst.apply_block(self.R)
            for c in range(3):
                assert_same_bits(Z[:, c], ar.cycle_ref(self.levels, self.o, self.R[:, c].copy()), f"{self.name}: column {c}")
            return
        assert_same_bits(dst.apply(self.r), want, self.name)

    def drop(self, dst):
        dst.free()

    def free(self):
        self.src.free()


class AmgRefresh(AmgChange):
    """spmvHipAmgRefresh of each kind of hierarchy, and of a plain one whose smoother is Chebyshev (rho_l and the tables
    are made again).  The source's new values differ entry by entry, so every level's products, sums and transposes have
    something to bring over."""
    KW = {"plain": dict(), "smoothed": dict(smoothed=True), "strength": dict(smoothed=True, theta=0.08, thetaScale=0.5)}

    def __init__(self, kind, cheb, *a):
        super().__init__("refresh", *a)
        self.kind, self.cheb = kind, cheb
        self.name = f"spmvHipAmgRefresh[{kind}" + (", Chebyshev" if cheb else "") + "]"
        self.path = {"plain": "the diagonal's flag, the products' numeric phases, the unit flags",
                     "smoothed": "besides: the damping's vectors, the diagonal handle, the two products and the sum of P, the transpose of R",
                     "strength": "besides: the filtered matrices' refresh with lumping, everything of the smoothed kind on F_l"}[kind] + \
            (", the spectral radii's vectors and the tables rewritten in place" if cheb else "")

    def make(self):
        self.A = M, N, IRP, JA, AS = fr.stencil7(16, 12, 1, (1.0, 0.05, 1.0)) if self.kind == "strength" else _grid()
        self.src = self.api.spMatCpyCSR(self.api.HostCSR(M, N, IRP, JA, AS))
        self.r = np.random.default_rng(4118).standard_normal(M)
        self.AS2 = np.ascontiguousarray(AS * np.random.default_rng(4120).uniform(1.0, 1.5, AS.size))
        self.src.update_values(self.AS2)
        return [(self.src, _x(22, N))]

    def fresh(self):
        self.src.update_values(self.A[4])
        h = self.src.amg(**self.KW[self.kind], **AMG_OPTS)
        if self.cheb:
            h.set_smoother("chebyshev")
        self.src.update_values(self.AS2)
        return h

    def reference(self, dst):
        new = self.A[:4] + (self.AS2,)
        if self.kind == "strength":                                  # the kept sets and the aggregates are the build's
            old, o = fr.strength_setup_ref(self.A, **AMG_OPTS)
            assert len(old) >= 3 and any(lv["F"][3].size < lv["A"][3].size for lv in old[:-1]), "the input is there for a filter that drops entries"
            want = sa.cycle_ref(fr.strength_refresh_ref(old, o, new), o, self.r)
        elif self.kind == "smoothed":
            levels, o = sa.setup_ref(new, **AMG_OPTS)
            want = sa.cycle_ref(levels, o, self.r)
        elif self.cheb:
            levels, o = cb.setup_ref(new, "plain", **AMG_OPTS)
            want = cb.cycle_ref(levels, o, self.r, cb.smoother(o))
        else:
            levels, o = ar.setup_ref(new, **AMG_OPTS)
            want = ar.cycle_ref(levels, o, self.r)
        assert_same_bits(dst.apply(self.r), want, self.name)


def _refresh_of(maker):
    return lambda *a: Refresh(maker(*a), *a)


def _bind(kind, *first):
    return lambda *a: kind(*first, *a)


TABLE = [
    ("spMatCpyCSR", CpyCSR),
    ("spMatCpyELL-row-major", _bind(CpyELL, False)), ("spMatCpyELL-column-major", _bind(CpyELL, True)),
    ("spmvHipCsrToEll-row-major", _bind(CsrToEll, False)), ("spmvHipCsrToEll-column-major", _bind(CsrToEll, True)),
    ("spmvHipAdoptCSR-4", _bind(Adopt, 4)), ("spmvHipAdoptCSR-8", _bind(Adopt, 8)),
    ("spmvHipBuildTiles-arrival", _bind(Tiles, 0)), ("spmvHipBuildTiles-deterministic", _bind(Tiles, 1)),
    ("spmvHipBuildStripes-arrival", _bind(Stripes, 0)), ("spmvHipBuildStripes-owner", _bind(Stripes, 1)),
    ("hipSpMVRowsSELL-build", Sell),
    ("first-hipSpMVRowsCSR", _bind(FirstCall, ROWS)), ("first-hipSpMVWarpPerRowCSR", _bind(FirstCall, WARP)),
    ("spmvHipUpdateValues", UpdateValues),
    ("spmvHipCsrTranspose", Transpose), ("spmvHipTransposeRefresh", _refresh_of(Transpose)),
    ("spmvHipColourCSR", Colour),
    ("spmvHipCsrPermute", Permute), ("spmvHipPermuteRefresh", _refresh_of(Permute)),
    ("spmvHipSpGEMM", Spgemm), ("spmvHipSpGEMMRefresh", _refresh_of(Spgemm)),
    ("spmvHipCsrAdd", Add), ("spmvHipCsrAddRefresh", _refresh_of(Add)),
    ("spmvHipCsrFilter-band", _bind(Filter, "band")), ("spmvHipCsrFilter-abs", _bind(Filter, "abs")),
    ("spmvHipCsrFilter-strength-lump", _bind(Filter, "strength")),
    ("spmvHipCsrFilterRefresh-lump", _refresh_of(_bind(Filter, "strength"))),
    ("first-hipSpTRSVCSR-lower", _bind(Trsv, True)), ("first-hipSpTRSVCSR-upper", _bind(Trsv, False)),
    ("hipSpILU0CSR", Ilu0),
    ("first-hipSpTRSMCSR-lower", Trsm),
    ("spmvHipDot", Dot), ("spmvHipMultiDot", MultiDot), ("spmvHipBlockDot", BlockDot),
    ("hipSpCGCSR", _bind(Krylov, "cg", False)), ("hipSpCGCSR-ilu0", _bind(Krylov, "cg", True)),
    ("hipSpBiCGStabCSR", _bind(Krylov, "bicgstab", False)), ("hipSpBiCGStabCSR-ilu0", _bind(Krylov, "bicgstab", True)),
    ("hipSpGMRESCSR", _bind(Krylov, "gmres", False)), ("hipSpGMRESCSR-ilu0", _bind(Krylov, "gmres", True)),
    ("hipSpCGBlockCSR", _bind(KrylovBlock, "cg")), ("hipSpBiCGStabBlockCSR", _bind(KrylovBlock, "bicgstab")),
    ("spmvHipAggregateCSR", Aggregate),
    ("spmvHipAmgSetup", _bind(AmgSetup, "plain")), ("spmvHipAmgSetupSmoothed", _bind(AmgSetup, "smoothed")),
    ("spmvHipAmgSetupStrength", _bind(AmgSetup, "strength")),
    ("spmvHipAmgRefresh", _bind(AmgRefresh, "plain", False)), ("spmvHipAmgRefresh-smoothed", _bind(AmgRefresh, "smoothed", False)),
    ("spmvHipAmgRefresh-strength", _bind(AmgRefresh, "strength", False)), ("spmvHipAmgRefresh-chebyshev", _bind(AmgRefresh, "plain", True)),
    ("spmvHipAmgSetSmoother-chebyshev", _bind(AmgChange, "chebyshev")),
    ("spmvHipAmgSetGaussSeidel", _bind(AmgChange, "gs")),
    ("spmvHipAmgSetBlockWidth", _bind(AmgChange, "width")), ("spmvHipAmgSetBlockWidth-change", _bind(AmgChange, "rewidth")),
]


# ------------------------------------------------------------------------------------------------------------ the driver
def _sticky_free(api, scratch):
    """invariant 6: the next, unrelated call is judged on its own"""
    assert api.lib.spmvHipVecFill(scratch.ptr, scratch.n, 0) == 0
    assert api.lib.spmvHipVecFill(scratch.ptr, scratch.n, FILL) == 0, "a refused allocation left the runtime's sticky error behind"
    assert np.all(scratch.down().view(np.uint64) == FILL)


@pytest.mark.parametrize("make_op", [t[1] for t in TABLE], ids=[t[0] for t in TABLE])
def test_every_allocation_refused_in_turn(api, oracle, capfd, make_op):
    t0 = time.perf_counter()
    _cold(api)
    base, bad0 = _level(api), int(api.alloc_stats().badFrees)
    op = make_op(api, oracle, capfd)
    sources = op.make()
    scratch = api.DeviceVector(64)
    states = [_source_state(api, d, x) for d, x in sources]

    made = []
    try:
        # the twin: never refused.  N, the reference, the bits every retry must give
        twin = op.fresh()
        made.append(twin)
        _cold(api)
        api.alloc_refuse(-1)
        assert op.call(twin) == 0, op.name + ": the unarmed call"
        N = int(api.alloc_stats().calls)
        assert N >= 1, op.name + " allocates nothing: it does not belong in the table"
        op.reference(twin)
        want = op.result(twin)

        armed = 0
        for n in range(N + 1):                                           # n == N: one past the last, which must refuse nothing
            for onward in (0, 1):
                dst = op.fresh()
                made.append(dst)
                _cold(api)
                before = _level(api)
                capfd.readouterr()
                op.refusing = n
                api.alloc_refuse(n, onward)
                rc = op.call(dst)
                st = api.alloc_stats()
                api.alloc_refuse(-1)
                err = capfd.readouterr().err
                armed += 1
                what = f"{op.name}: allocation {n} of {N}" + (" and every later one" if onward else "") + " refused"
                if n == N:
                    assert st.refused == 0 and rc == 0, what + ": the call's allocation count is not the twin's"
                    assert int(st.calls) == N or op.fallback, what + ": the call's allocation count is not the twin's"
                    assert op.result(dst) == want, what
                    op.drop(made.pop())
                    continue
                # 1 refusal
                if op.fallback and st.refused == 0:                 # a selection times its candidates: this time it built fewer
                    assert rc == 0 and op.result(dst) == want, what + ": nothing was refused, and the call did not answer"
                    op.drop(made.pop())
                    continue
                assert st.refused >= 1, what + ": nothing was refused"
                if op.fallback and rc == 0:
                    assert op.result(dst) == want, what + ": the fallback's result"
                else:
                    assert not (op.fallback and onward and n == 0), what + ": with nothing to allocate the fallback must answer"
                    assert rc == 1, what + f": returned {rc}"
                    assert "libspmvhip" in err, what + ": no line on stderr"
                # 2 ledger
                assert int(st.badFrees) == bad0, what + ": a pointer was released twice, or one that was never allocated"
                if op.nothing_left and rc:
                    now = _level(api)
                    assert (now[0] - before[0], now[1] - before[1]) in op.may_stay(dst), what + f": the library holds {now} where it held {before}"
                # 3 outputs untouched (no launch)
                if rc:
                    op.untouched(dst)
                # 4 sources intact
                for (d, x), state in zip(sources, states):
                    assert _source_state(api, d, x) == state, what + ": a source changed"
                # 5 the handle is still lawful
                if rc:
                    op.still_lawful(dst)
                # 6 no sticky error
                _sticky_free(api, scratch)
                # 7 retry
                if rc:
                    assert op.call(dst) == 0, what + ": the same call made again"
                    assert op.result(dst) == want, what + ": the retry's bits are not the twin's"
                op.drop(made.pop())
    finally:                                                         # a failed assertion ends the case; what it made goes back all the same
        api.alloc_refuse(-1)
        for d in made:
            op.drop(d)
        op.free()
        scratch.free()
    _cold(api)
    assert int(api.alloc_stats().badFrees) == bad0
    assert _level(api) == base, f"{op.name}: the case leaves {_level(api)} where it found {base}"
    seconds = time.perf_counter() - t0
    MEASURED.append((op.name, N, armed, seconds, op.path))
    print(f"alloc-refusals | {op.name} | N = {N} | {armed} armed calls | {seconds:.2f} s | {op.path}{op.note()}")


def test_a_value_update_after_the_factors_are_in_place_makes_ilu0_factorise_again(api, capfd):
    """hipSpILU0CSR whose LAST allocation fails leaves the complete factors and remembers it, so that the same call made
    again only finishes the handle.  Whatever rewrites AS in between must make it forget: after spmvHipUpdateValues, and
    after a refresh of a derived handle (here a transpose), the next call is an ordinary factorisation of the new values --
    not a success with unfactored values."""
    M, N, IRP, JA, AS = A = _square(4113, 500)
    factors = np.array(ilu0_ref.ilu0_loop(M, IRP, JA, AS))
    IRPt, JAt, ASt, _ = stable_transpose(N, IRP, JA, AS)
    At = (M, M, IRPt, JAt, ASt)
    factors_t = np.array(ilu0_ref.ilu0_loop(M, IRPt, JAt, ASt))

    def fail_at_the_last_step(d):
        twin = api.spMatCpyCSR(api.HostCSR(*(At if d is dt else A)))
        _cold(api)
        api.alloc_refuse(-1)
        assert api.lib.hipSpILU0CSR(C.byref(twin.handle)) == 0
        last = int(api.alloc_stats().calls) - 1
        twin.free()
        _cold(api)
        capfd.readouterr()
        with api.alloc_refused(last):
            assert api.lib.hipSpILU0CSR(C.byref(d.handle)) == 1
        assert "the factors are in place" in capfd.readouterr().err

    src = api.spMatCpyCSR(api.HostCSR(*A))
    d = api.spMatCpyCSR(api.HostCSR(*A))
    dt = src.transpose()
    try:
        fail_at_the_last_step(d)
        assert_same_bits(_csr_arrays(api, d)[2], factors, "the factors are in place")
        d.update_values(np.ascontiguousarray(AS))                    # the original values again: the next call must factorise them
        assert api.lib.hipSpILU0CSR(C.byref(d.handle)) == 0
        assert_same_bits(_csr_arrays(api, d)[2], factors, "after a value update in between: factorised again")

        fail_at_the_last_step(dt)
        assert_same_bits(_csr_arrays(api, dt)[2], factors_t, "the transpose's factors are in place")
        dt.refresh_from(src)                                         # the source's values again, through the map
        assert_same_bits(_csr_arrays(api, dt)[2], ASt, "the refresh brought the source's values back")
        assert api.lib.hipSpILU0CSR(C.byref(dt.handle)) == 0
        assert_same_bits(_csr_arrays(api, dt)[2], factors_t, "after a refresh in between: factorised again")
    finally:
        api.alloc_refuse(-1)
        for h in (d, dt, src):
            h.free()


def test_the_ledger_is_back_where_the_module_started(api):
    """everything freed: the ledger holds what it held before the module's first call, and no release was ever a bad one"""
    _cold(api)
    api.spmvHipFinalize()
    st = api.alloc_stats()
    for name, N, armed, seconds, _ in MEASURED:
        print(f"alloc-refusals | {name} | N = {N} | {armed} armed calls | {seconds:.2f} s")
    assert [int(st.live), int(st.liveBytes), int(st.badFrees)] == MODULE_START
    api.spmvHipInit(0)
