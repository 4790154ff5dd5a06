"""What the approximate-inverse entry points refuse -- each refusal with a "libspmvhip" line, EXIT_FAILURE and a destination
that is still zero (a setup) or unchanged (a refresh) -- and what they leave when a device allocation fails: for
spmvHipFsaiSetup, spmvHipFsaiRefresh and spmvHipFsaiApply every allocation is refused in turn and from then on, under the seven
checks of tests/test_gpu_alloc_refusals.py, whose driver runs the entries defined here."""
import ctypes as C

import numpy as np
import pytest

import fsai_ref as fr
import serial_order_inputs as si
import test_gpu_alloc_refusals as ar
from bits import assert_same_bits
from test_gpu_alloc_refusals import _defaults, api  # noqa: F401  (the driver's fixtures: a disarmed, initialised library)
from test_fsai_abi import dense_rows, random_spd

pytestmark = pytest.mark.gpu
P = C.byref


def _up(api, A):
    return api.spMatCpyCSR(api.HostCSR(*A))


def _is_zero(s):
    return C.string_at(C.addressof(s), C.sizeof(s)) == bytes(C.sizeof(s))


def _bytes(s):
    return C.string_at(C.addressof(s), C.sizeof(s))


def _unsorted(A):
    """the same matrix with the entries of one row of at least two swapped"""
    M, N, IRP, JA, AS = A
    JA, AS = JA.copy(), AS.copy()
    r = int(np.flatnonzero(np.diff(IRP.astype(np.int64)) >= 2)[3])
    b = int(IRP[r])
    JA[[b, b + 1]], AS[[b, b + 1]] = JA[[b + 1, b]], AS[[b + 1, b]]
    return (M, N, IRP, JA, AS), r


# -------------------------------------------------------------------------------------------------------------- refusals
def test_what_the_setup_refuses(api, capfd):
    lib = api.lib
    A = random_spd(np.random.default_rng(3901), 120, 4)
    da, small = _up(api, A), _up(api, random_spd(np.random.default_rng(3902), 80, 4))
    wide = _up(api, (120, 130) + tuple(A[2:]))
    ell = api.csr_to_ell_device(da, False)
    bad, row = _unsorted(A)
    dbad = _up(api, bad)
    long_row = _up(api, dense_rows(None, 120, np.where(np.arange(120) == 90, 64, 3)))
    a = P(da.handle)
    dead = api.spmat()
    cases = [
        ("dA is NULL", lambda g, i: lib.spmvHipFsaiSetup(None, None, None, P(g), P(i)), "dA is NULL"),
        ("dG is NULL", lambda g, i: lib.spmvHipFsaiSetup(a, None, None, None, None), "dG is NULL"),
        ("a dA that is not live", lambda g, i: lib.spmvHipFsaiSetup(P(dead), None, None, P(g), P(i)), "not a device handle"),
        ("a dS that is not live", lambda g, i: lib.spmvHipFsaiSetup(a, P(dead), None, P(g), P(i)), "not a device handle"),
        ("an ELL dA", lambda g, i: lib.spmvHipFsaiSetup(P(ell.handle), None, None, P(g), P(i)), "ELL"),
        ("an ELL dS", lambda g, i: lib.spmvHipFsaiSetup(a, P(ell.handle), None, P(g), P(i)), "ELL"),
        ("a dA that is not square", lambda g, i: lib.spmvHipFsaiSetup(P(wide.handle), None, None, P(g), P(i)), "not square"),
        ("a dS that is not square", lambda g, i: lib.spmvHipFsaiSetup(a, P(wide.handle), None, P(g), P(i)), "not square"),
        ("a dS of another size", lambda g, i: lib.spmvHipFsaiSetup(a, P(small.handle), None, P(g), P(i)), "dS has 80 rows, dA 120"),
        ("an unsorted dA", lambda g, i: lib.spmvHipFsaiSetup(P(dbad.handle), None, None, P(g), P(i)), f"row {row} of dA"),
        ("an unsorted dS", lambda g, i: lib.spmvHipFsaiSetup(a, P(dbad.handle), None, P(g), P(i)), f"row {row} of dS"),
        ("a pattern row of 65", lambda g, i: lib.spmvHipFsaiSetup(a, P(long_row.handle), None, P(g), P(i)), "row 90 of the pattern"),
        ("lanesPerRow 5", lambda g, i: lib.spmvHipFsaiSetup(a, None, P(api.spmvFsaiOpts(5)), P(g), P(i)), "lanesPerRow 5"),
    ]
    try:
        level = ar._level(api)
        for what, call, line in cases:
            g, info = api.spmat(), ar._patterned(api.spmvFsaiInfo)
            capfd.readouterr()
            rc = call(g, info)
            err = capfd.readouterr().err
            assert rc == 1 and "libspmvhip" in err and line in err, (what, rc, err)
            assert _is_zero(g) and ar._is_patterned(info) and ar._level(api) == level, what
        capfd.readouterr()
        assert lib.spmvHipFsaiSetup(a, None, None, a, None) == 1 and "source handle itself" in capfd.readouterr().err
        assert da.handle.dev, "dG == dA is refused before anything is written"
        # the pattern row of exactly 64 next to it is taken
        ok = _up(api, dense_rows(None, 120, np.where(np.arange(120) == 90, 63, 3)))
        g = da.fsai(pattern=ok)
        assert g.info().maxRow == 64
        g.free()
        ok.free()
    finally:
        for d in (long_row, dbad, ell, wide, small, da):
            d.free()


def test_what_refresh_apply_and_the_views_refuse(api, capfd):
    lib = api.lib
    A = random_spd(np.random.default_rng(3903), 120, 4)
    da, twin = _up(api, A), _up(api, A)
    g = da.fsai()
    t = da.transpose()
    v, w = api.DeviceVector(121), api.DeviceVector(120)
    try:
        before, arrays, level = _bytes(g.handle), [a.tobytes() for a in ar._csr_arrays(api, g)], ar._level(api)
        h, info, view = P(g.handle), ar._patterned(api.spmvFsaiInfo), api.spmat()
        shifted = C.c_void_p(v.ptr.value + 8)
        cases = [
            ("refresh: dG is NULL", lambda: lib.spmvHipFsaiRefresh(None, P(da.handle), P(info)), "dG is NULL"),
            ("refresh: dA is NULL", lambda: lib.spmvHipFsaiRefresh(h, None, P(info)), "dA is NULL"),
            ("refresh: another source", lambda: lib.spmvHipFsaiRefresh(h, P(twin.handle), P(info)), "dA is not the handle dG was set up from"),
            ("refresh: the factor as its own source", lambda: lib.spmvHipFsaiRefresh(h, h, P(info)), "dA is not the handle dG was set up from"),
            ("refresh: no factor", lambda: lib.spmvHipFsaiRefresh(P(t.handle), P(da.handle), P(info)), "dG was not made by spmvHipFsaiSetup"),
            ("apply: no factor", lambda: lib.spmvHipFsaiApply(P(da.handle), w.ptr, w.ptr), "dG was not made by spmvHipFsaiSetup"),
            ("apply: dR is NULL", lambda: lib.spmvHipFsaiApply(h, None, w.ptr), "dR is NULL"),
            ("apply: dZ is NULL", lambda: lib.spmvHipFsaiApply(h, w.ptr, None), "dZ is NULL"),
            ("apply: an overlap", lambda: lib.spmvHipFsaiApply(h, v.ptr, shifted), "overlap"),
            ("transpose: no factor", lambda: lib.spmvHipFsaiTranspose(P(t.handle), P(view)), "dG was not made by spmvHipFsaiSetup"),
            ("transpose: dGT is NULL", lambda: lib.spmvHipFsaiTranspose(h, None), "dGT is NULL"),
            ("info: no factor", lambda: lib.spmvHipFsaiInfo(P(da.handle), P(info)), "dG was not made by spmvHipFsaiSetup"),
            ("info: info is NULL", lambda: lib.spmvHipFsaiInfo(h, None), "info is NULL"),
        ]
        for what, call, line in cases:
            capfd.readouterr()
            rc = call()
            err = capfd.readouterr().err
            assert rc == 1 and "libspmvhip" in err and line in err, (what, rc, err)
            assert ar._is_patterned(info) and _is_zero(view) and _bytes(g.handle) == before and ar._level(api) == level, what
        assert [a.tobytes() for a in ar._csr_arrays(api, g)] == arrays, "a refused call left the factor as it was"
        assert g.info().setups == 1
    finally:
        for d in (v, w, t, g, twin, da):
            d.free()


# ------------------------------------------------------------------------------------- every allocation refused in turn
def _inputs():
    """a 300-row symmetric matrix and a wider pattern with rows of up to 20"""
    A = random_spd(np.random.default_rng(3910), 300, 4, spread=25)
    return A, dense_rows(None, 300, np.random.default_rng(3911).integers(0, 20, 300))


def _apply_bytes(api, handle, r, M):
    dr, dz = api.DeviceVector(M).up(r), api.DeviceVector(M)
    try:
        dz.poison()
        assert api.lib.spmvHipFsaiApply(P(handle), dr.ptr, dz.ptr) == 0
        return dz.down().tobytes()
    finally:
        dr.free()
        dz.free()


def _view_bytes(api, handle):
    view = api.spmat()
    assert api.lib.spmvHipFsaiTranspose(P(handle), P(view)) == 0
    return ar._blob(api.AmgHierarchy._down(view)[2:])


class Setup(ar.Derived):
    """spmvHipFsaiSetup from sources whose pattern check is already on record: a refusal leaves dG and info alone, the
    sources as they were and nothing behind; the retried handle owns a complete G^T and applies"""
    name = "spmvHipFsaiSetup"
    path = "the counts and their scan, the three arrays, the row report, the transpose with its sort, both sets of row blocks, the workspace"

    def __init__(self, *a):
        super().__init__(*a)
        self.info_kind = self.api.spmvFsaiInfo

    def inputs(self):
        return list(_inputs())

    def make(self):
        out = super().make()
        warm = self.api.DeviceMatrix()
        assert self.call((warm, None)) == 0                              # (the once-per-handle pattern check of both sources)
        warm.free()
        return out

    def call(self, dst):
        return self.lib.spmvHipFsaiSetup(P(self.src[0].handle), P(self.src[1].handle), None, P(dst[0].handle), self.info_ref(dst))

    def expected(self):
        return fr.fsai_vec(*self.mats)[0]

    def result(self, dst):
        M = self.mats[0][0]
        return super().result(dst) + _view_bytes(self.api, dst[0].handle) + (_apply_bytes(self.api, dst[0].handle, ar._x(21, M), M),)

    def reference(self, dst):
        super().reference(dst)
        G = self.expected()
        got = self.result(dst)
        assert got[5:8] == ar._blob([np.asarray(a, t) for a, t in zip(fr.transposed(G)[2:], (np.uint32, np.uint32, np.float64))]), "G^T"
        assert got[8] == fr.Applied(G)(ar._x(21, G[0])).tobytes(), "the apply"


class ColdSetup(Setup):
    """... from sources uploaded for the call: the pattern checks' own allocations are swept too"""
    name = "spmvHipFsaiSetup (first use of its sources)"

    def make(self):
        self.mats = self.inputs()
        self.src = []
        return []

    def fresh(self):
        self.free()
        self.src = [_up(self.api, A) for A in self.mats]
        return super().fresh()


class Refresh(ar.Op):
    """spmvHipFsaiRefresh after the source took new values: a refusal leaves the handle live with its pattern and addresses
    and info alone; the same call made again completes G and G^T"""
    name, path, nothing_left = "spmvHipFsaiRefresh", "the row report, the unit flags of G and of G^T", False

    def make(self):
        self.A = _inputs()[0]
        rng = np.random.default_rng(3912)
        rows, cols = si.row_of_entry(self.A[2]), self.A[3].astype(np.int64)
        _, pair = np.unique(np.minimum(rows, cols) * self.A[0] + np.maximum(rows, cols), return_inverse=True)
        scale = (1.0 + 0.25 * rng.random(int(pair.max()) + 1))[pair]     # one factor per symmetric pair: symmetric, still dominant
        self.new = np.ascontiguousarray(self.A[4] * scale)
        self.da = _up(self.api, self.A)
        self.da.fsai().free()                                            # (the pattern check, once)
        self.da.update_values(self.new)
        return [(self.da, ar._x(22, self.A[0]))]

    def fresh(self):
        self.da.update_values(self.A[4])
        g = self.da.fsai()
        self.da.update_values(self.new)
        return g, ar._patterned(self.api.spmvFsaiInfo), ar._handle_bytes(g)

    def call(self, dst):
        return self.lib.spmvHipFsaiRefresh(P(dst[0].handle), P(self.da.handle), P(dst[1]))

    def untouched(self, dst):
        assert ar._handle_bytes(dst[0]) == dst[2], "a refused refresh changed the handle's pattern or addresses"
        assert ar._is_patterned(dst[1]), "info was written"

    def still_lawful(self, dst):
        ar._product(self.api, ar.ROWS, dst[0], ar._x(23, self.A[0]), self.A[0])

    def result(self, dst):
        M = self.A[0]
        return ar._blob(ar._csr_arrays(self.api, dst[0])) + _view_bytes(self.api, dst[0].handle) + (_apply_bytes(self.api, dst[0].handle, ar._x(21, M), M),)

    def reference(self, dst):
        G = fr.fsai_vec(self.A[:4] + (self.new,))[0]
        got = self.result(dst)
        assert got[:3] == ar._blob([np.asarray(a, t) for a, t in zip(G[2:], (np.uint64, np.uint64, np.float64))]), "G of the new values"
        assert got[3:6] == ar._blob([np.asarray(a, t) for a, t in zip(fr.transposed(G)[2:], (np.uint32, np.uint32, np.float64))]), "G^T"
        assert got[6] == fr.Applied(G)(ar._x(21, G[0])).tobytes(), "the apply"
        assert dst[0].info().setups == 2

    def drop(self, dst):
        dst[0].free()

    def free(self):
        self.da.free()


class Apply(ar.Op):
    """the first spmvHipFsaiApply of a factor large enough for the serial-order selections of G and of G^T to build formats:
    like the first call of a launcher it skips a format it cannot build and answers with the kernel that needs no memory"""
    name, path = "the first spmvHipFsaiApply", "the candidates' formats of two selections, each of which may be skipped"
    fallback, nothing_left = True, False

    def make(self):
        self.A = random_spd(np.random.default_rng(3913), 30000, 18)
        M = self.A[0]
        G = fr.fsai_vec(self.A)[0]
        assert G[3].size >= si.AUTO_MIN_NNZ
        self.r = ar._x(24, M)
        T = fr.transposed(G)
        self.want = self.oracle.csr_serial(T[2], T[3], T[4], self.oracle.csr_serial(G[2], G[3], G[4], self.r))
        self.da = _up(self.api, self.A)
        self.da.fsai().free()
        self.dr, self.dz = self.api.DeviceVector(M).up(self.r), self.api.DeviceVector(M)
        return [(self.da, ar._x(25, M))]

    def fresh(self):
        self.dz.poison()
        return self.da.fsai()

    def call(self, dst):
        return self.lib.spmvHipFsaiApply(P(dst.handle), self.dr.ptr, self.dz.ptr)

    def untouched(self, dst):
        pass

    def result(self, dst):
        assert_same_bits(self.dz.down(), self.want, self.name)
        return ()

    def reference(self, dst):
        self.result(dst)

    def still_lawful(self, dst):
        self.dz.poison()

    def drop(self, dst):
        dst.free()

    def free(self):
        for d in (self.dr, self.dz, self.da):
            d.free()


@pytest.mark.parametrize("make_op", [Setup, ColdSetup, Refresh, Apply], ids=["setup", "setup-cold-sources", "refresh", "apply"])
def test_every_allocation_refused_in_turn(api, oracle, capfd, make_op):
    ar.test_every_allocation_refused_in_turn(api, oracle, capfd, make_op)
