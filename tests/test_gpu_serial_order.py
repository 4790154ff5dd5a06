"""The serial-order contract, bit for bit, on every kernel that may serve it.

hipSpMVRowsCSR (variant 2) promises the bits of sgemvSerial and keeps the promise by TIMING its candidates -- the
LDS-stream kernel, the deterministic two-phase form, the stripes "owner wavefronts" and "ordered tickets" forms -- and
keeping the fastest.  Which one wins differs from process to process, so each must keep the promise on its own.  Every
candidate runs here on inputs where another order, a -0.0 seed or an unstable sort shows (tests/serial_order_inputs.py;
tests/test_serial_order_inputs.py shows on the host that they do), and is compared with the oracle as uint64 patterns.

Rows whose columns do not ascend: the selection must notice one descending pair wherever it sits and keep the LDS-stream
kernel, and the explicit deterministic builds add such rows in the order include/spmvHip.h states (stripes: stable by
column; two-phase: stable by 16 Ki-column slice)."""
import ctypes as C

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits

pytestmark = pytest.mark.gpu

ROWS = "hipSpMVRowsCSR"


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _default_variant(api):
    api.set_variant(ROWS, 2)
    yield
    api.set_variant(ROWS, 2)


class Handle:
    """an uploaded handle, or an adopted one with 8-byte row pointers (the caller's device arrays)"""

    def __init__(self, api, M, N, IRP, JA, AS, adopt64=False):
        self.bufs = []
        if adopt64:
            irp, ja = IRP.astype(np.uint64), JA.astype(np.uint32)
            self.bufs = [api.DeviceBuffer(irp.nbytes).up(irp), api.DeviceBuffer(ja.nbytes).up(ja),
                         api.DeviceBuffer(AS.nbytes).up(np.ascontiguousarray(AS))]
            self.dm = api.DeviceMatrix()
            assert api.lib.spmvHipAdoptCSR(C.byref(self.dm.handle), M, N, JA.size, self.bufs[0].ptr, 8, self.bufs[1].ptr,
                                           self.bufs[2].ptr, irp.ctypes.data_as(C.c_void_p)) == 0
        else:
            self.dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))

    def free(self):
        self.dm.free()
        for b in self.bufs:
            b.free()


class Runner:
    def __init__(self, api, x, M):
        self.api, self.M = api, M
        self.dx, self.dy = api.DeviceVector(x.size).up(x), api.DeviceVector(M)

    def __call__(self, launcher, dm):
        self.dy.poison()
        self.api.spmv(launcher, dm, self.dx, self.dy)
        return self.dy.down()

    def free(self):
        self.dx.free()
        self.dy.free()


def _choice(api, dm):
    return (api.lib.spmvHipAutoChoiceRows(C.byref(dm.handle), None) or b"-").decode()


def _check_twice(run, launcher, dm, y_ref, what, row_info):
    y1 = run(launcher, dm)
    assert_same_bits(y1, y_ref, what, row_info)
    assert_same_bits(run(launcher, dm), y1, what + ", second call", row_info)


@pytest.mark.parametrize("kind", ["uploaded", "adopted-irp64", "unit"])
@pytest.mark.parametrize("name", ["mixed", "narrow17", "widespan"])
def test_every_candidate_gives_the_serial_bits(api, oracle, name, kind):
    """variant 2 as chosen, variant 1, the deterministic two-phase form (automatic bins, 20 000 rows, 4999 rows -- no
    multiple of 4), the two deterministic stripes forms (automatic bins, 20 000 rows, 700 rows on 3 workgroups, the
    32-bit-column encoding forced): each the oracle's bits, twice"""
    inp = si.make(name)
    if kind == "unit":
        inp = si.unit(inp)
    M, N, IRP, JA, AS, x = inp.M, inp.N, inp.IRP, inp.JA, inp.AS, inp.x
    y_ref = oracle.csr_serial(IRP, JA, AS, x)
    lens = inp.lens()
    kinds = {int(r): k for k, rows in inp.special.items() for r in rows}

    def row_info(r):
        return f"length {lens[r]}, {kinds.get(r, 'ordinary')} row, first column {int(JA[IRP[r]]) if lens[r] else '-'}"

    h = Handle(api, M, N, IRP, JA, AS, adopt64=kind == "adopted-irp64")
    run = Runner(api, x, M)
    tag = f"{name}/{kind}"
    try:
        if kind == "unit":
            v = C.c_double()
            assert api.lib.spmvHipUnitValue(C.byref(h.dm.handle), C.byref(v)) == 1 and v.value == -2.5
        y = run(ROWS, h.dm)                                   # first call: the selection, then the chosen kernel's y
        choice = _choice(api, h.dm)
        assert_same_bits(y, y_ref, f"{tag}: hipSpMVRowsCSR variant 2 (chose {choice})", row_info)
        assert_same_bits(run(ROWS, h.dm), y, f"{tag}: hipSpMVRowsCSR variant 2 (chose {choice}), second call", row_info)
        api.set_variant(ROWS, 1)
        _check_twice(run, ROWS, h.dm, y_ref, f"{tag}: hipSpMVRowsCSR variant 1", row_info)
        api.set_variant(ROWS, 2)
        for rows in (0, 20000, 4999):
            api.build_tiles(h.dm, rowsPerBin=rows, deterministic=True)
            assert api.tiles_info(h.dm).deterministic == 1
            _check_twice(run, "hipSpMVTilesCSR", h.dm, y_ref, f"{tag}: tiles deterministic, rowsPerBin {rows}", row_info)
        for form in (1, 2):
            for rows, grid, wide in ((0, 0, -1), (20000, 0, -1), (700, 3, -1), (0, 0, 1)):
                api.build_stripes(h.dm, rowsPerBin=rows, grid=grid, wide=wide, deterministic=form)
                info = api.stripes_info(h.dm)
                assert info.deterministic == form
                if wide == 1 or name == "widespan":           # forced, or chosen by itself: a step spans >= 2^17 columns
                    assert info.wide == 1, (tag, form, rows)
                _check_twice(run, "hipSpMVStripesCSR", h.dm, y_ref,
                             f"{tag}: stripes deterministic {form}, rowsPerBin {rows}, grid {grid}, wide {info.wide}", row_info)
        # after all the explicit builds the selection's pick still serves hipSpMVRowsCSR
        assert_same_bits(run(ROWS, h.dm), y_ref, f"{tag}: hipSpMVRowsCSR variant 2 (chose {choice}) after the builds", row_info)
    finally:
        run.free()
        h.free()


@pytest.mark.parametrize("where,adopt64", [("last-row", False), ("63/64", False), ("127/128", False), ("63/64", True)])
def test_one_descending_pair_keeps_the_lds_stream_kernel(api, oracle, where, adopt64):
    """sorted everywhere but ONE descending pair (placed where a 64-lane stride could step over it): the selection must
    see it, keep the LDS-stream kernel and build no format -- the format kernels would add that row in column order"""
    M, N, IRP, JA, AS, x, row = si.descending_pair(where)
    y_ref = oracle.csr_serial(IRP, JA, AS, x)
    h = Handle(api, M, N, IRP, JA, AS, adopt64=adopt64)
    run = Runner(api, x, M)
    try:
        assert_same_bits(run(ROWS, h.dm), y_ref, f"descending pair at {where} of row {row}")
        assert _choice(api, h.dm) == ROWS
        assert api.lib.spmvHipTilesBytes(C.byref(h.dm.handle)) == 0
        assert api.lib.spmvHipStripesBytes(C.byref(h.dm.handle)) == 0
    finally:
        run.free()
        h.free()


def _blocks(api, M, N, IRP, JA, AS, x, build, launcher, n_blocks):
    cuts = [M * k // n_blocks for k in range(n_blocks + 1)]
    parts = []
    for k, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
        b0, b1 = int(IRP[r0]), int(IRP[r1])
        blk = api.spMatCpyCSR(api.HostCSR(r1 - r0, N, IRP[r0:r1 + 1] - IRP[r0], JA[b0:b1], AS[b0:b1]))
        run = Runner(api, x, r1 - r0)
        try:
            build(blk, k)
            parts.append(run(launcher, blk))
        finally:
            run.free()
            blk.free()
    return np.concatenate(parts)


def test_explicit_deterministic_forms_on_shuffled_rows(api, oracle):
    """rows in random order, repeated columns, five slices: an explicit deterministic build does not check the order, and
    adds a row stably by column (stripes, both forms) or stably by 16 Ki-column slice (two-phase) -- on 1 and 3 row
    blocks alike"""
    M, N, IRP, JA, AS, x = si.shuffled()
    y_stripes = oracle.csr_serial(*si.permuted(IRP, JA, AS, si.stripes_order(IRP, JA)), x)
    y_tiles = oracle.csr_serial(*si.permuted(IRP, JA, AS, si.tiles_order(IRP, JA)), x)
    lens = np.diff(IRP.astype(np.int64))

    def row_info(r):
        return f"length {lens[r]}"

    for n_blocks in (1, 3):
        for form in (1, 2):
            y = _blocks(api, M, N, IRP, JA, AS, x, lambda d, k: api.build_stripes(d, deterministic=form), "hipSpMVStripesCSR", n_blocks)
            assert_same_bits(y, y_stripes, f"stripes deterministic {form}, {n_blocks} row block(s)", row_info)
        y = _blocks(api, M, N, IRP, JA, AS, x, lambda d, k: api.build_tiles(d, deterministic=True), "hipSpMVTilesCSR", n_blocks)
        assert_same_bits(y, y_tiles, f"tiles deterministic, {n_blocks} row block(s)", row_info)
    # the selection itself never offers them these rows
    h = Handle(api, M, N, IRP, JA, AS)
    run = Runner(api, x, M)
    try:
        assert_same_bits(run(ROWS, h.dm), oracle.csr_serial(IRP, JA, AS, x), "hipSpMVRowsCSR on shuffled rows")
        assert _choice(api, h.dm) == ROWS
    finally:
        run.free()
        h.free()
