"""Phase 1 of the two-phase SpMV as a RESIDENT kernel: one workgroup per CU walks a contiguous, slice-major run of work items
and refills its x slice in LDS only when the slice changes (tiles.hip, pb_expand_kernel).

Phase 1 writes a product per entry and nothing else, so a wrong run table, a stale slice in LDS, a missed head or tail or a
wrong hand-over between items shows as a wrong y.  Every case runs through the deterministic form -- required to be the bits
of the serial oracle -- and through the arrival-order form under the tight bound of tests/test_gpu_parity.py, twice on the
same handle with different x (a slice prefetched for one launch must not survive into the next), and once more after
spmvHipUpdateValues (the value map against the slice-major order the work list walks).

The shapes are the ones at which the walk takes another path: empty slices, slices of 1 / 63 / 64 / 65 / an odd number of
entries (scalar head and tail, no whole pair), a partial last slice, one work item in all, fewer work items than CUs, more
than one per CU, and slice lengths that are exact multiples of the work item size, so that runs end on slice boundaries and
begin inside slices."""
import numpy as np
import pytest

from bits import assert_same_bits
from conftest import tight_error
from serial_order_inputs import SLICE, order_values

pytestmark = pytest.mark.gpu

TIGHT = 1e-13                    # tests/test_gpu_parity.py
CHUNK = 4096                     # smallest work item size the build accepts in whole slices of pieces


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


def _matrix(seed, M, N, per_slice, value=None):
    """CSR with per_slice[s] entries in column slice s: random rows, random columns of the slice (repeats allowed), rows
    sorted by column; values of mixed sign and magnitude, or all `value`."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for s, n in enumerate(per_slice):
        lo, hi = s * SLICE, min((s + 1) * SLICE, N)
        assert n == 0 or hi > lo
        rows.append(rng.integers(0, M, n))
        cols.append(rng.integers(lo, hi, n) if n else np.empty(0, dtype=np.int64))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    AS = np.full(rows.size, float(value)) if value is not None else order_values(rng, rows.size)
    return M, N, IRP, cols.astype(np.uint64), AS


def _run(api, dmat, x, rows):
    dx = api.DeviceVector(x.size).up(x)
    dy = api.DeviceVector(rows)
    dy.poison()
    api.spmv("hipSpMVTilesCSR", dmat, dx, dy)
    y = dy.down()
    dx.free()
    dy.free()
    return y


def _check(api, oracle, mat, chunk, nt_stores=(-1,), new_value=None):
    M, N, IRP, JA, AS = mat
    rng = np.random.default_rng(JA.size)
    xs = [order_values(rng, N), order_values(rng, N)]
    AS2 = np.full(AS.size, float(new_value)) if new_value is not None else order_values(rng, AS.size)
    refs = [oracle.csr_serial(IRP, JA, AS, x) for x in xs]
    ref2 = oracle.csr_serial(IRP, JA, AS2, xs[0])
    for det in (True, False):
        for nt in nt_stores:
            dmat = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
            api.build_tiles(dmat, chunk=chunk, ntStore=nt, deterministic=det)
            info = api.tiles_info(dmat)
            assert info.deterministic == int(det) and info.nSlices == (N + SLICE - 1) // SLICE
            assert (info.chunk == chunk if chunk else info.chunk > 0) and (nt < 0 or info.ntStore == nt)
            runs = [(xs[0], AS, refs[0]), (xs[1], AS, refs[1]), (xs[0], AS2, ref2)]
            for k, (x, vals, y_ref) in enumerate(runs):
                if k == 2:
                    dmat.update_values(AS2)
                y = _run(api, dmat, x, M)
                what = f"deterministic={det} ntStore={nt} run {k}"
                if det:
                    assert_same_bits(y, y_ref, what)
                else:
                    err = tight_error(IRP, JA, vals, x, y_ref, y)
                    print(f"{what}: tight error {err:.3e}")
                    assert not np.isnan(y).any() and err <= TIGHT, what
            dmat.free()


N_PARTIAL = 3 * SLICE + 5        # four slices, the last of 5 columns

EDGE_CASES = {
    # entries per slice; the long slices are several pieces of CHUNK
    "odd_empty_1_63": (9001, 0, 1, 63),
    "64_odd_65_few": (64, 12289, 65, 7),
    "1_empty_empty_odd": (1, 0, 0, 4097),
}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_short_and_empty_slices(api, oracle, name):
    """slices of 0 / 1 / 63 / 64 / 65 / an odd number of entries beside slices of several pieces, partial last slice; the
    first case with both kinds of product stores"""
    mat = _matrix(11, 700, N_PARTIAL, EDGE_CASES[name])
    _check(api, oracle, mat, CHUNK, nt_stores=(0, 1) if name == "odd_empty_1_63" else (-1,))


def test_one_slice_one_work_item(api, oracle):
    _check(api, oracle, _matrix(12, 300, 1000, (3001,)), 0)


def test_fewer_work_items_than_compute_units(api, oracle):
    """about 10 work items: most workgroups of a device have nothing to do"""
    _check(api, oracle, _matrix(13, 2000, 2 * SLICE, (25001, 15000)), CHUNK)


def test_more_work_items_than_compute_units(api, oracle):
    """about 300 work items in slices of unequal length: runs of more than one item, cut inside items"""
    _check(api, oracle, _matrix(14, 50_000, 5 * SLICE + 100, (400_001, 150_000, 0, 350_003, 299_000, 1001)), CHUNK)


def test_slice_lengths_that_are_multiples_of_the_work_item(api, oracle):
    """every slice is a whole number of work items, so balanced runs end exactly on slice boundaries and begin inside
    slices: 11 items (one run each on a device with more CUs), and 512 items in 8 equal slices (whole items per run on
    a device whose CU count divides 512)"""
    _check(api, oracle, _matrix(15, 3000, 4 * SLICE, (3 * CHUNK, 2 * CHUNK, 5 * CHUNK, CHUNK)), CHUNK)
    _check(api, oracle, _matrix(16, 60_000, 8 * SLICE, (64 * CHUNK,) * 8), CHUNK)


@pytest.mark.parametrize("name", ["64_odd_65_few", "items"])
def test_all_values_equal(api, oracle, name):
    """the instantiations that do not read the value stream, refreshed with another single value"""
    if name == "items":
        mat = _matrix(17, 2000, 2 * SLICE, (25001, 15000), value=-0.75)
    else:
        mat = _matrix(17, 700, N_PARTIAL, EDGE_CASES[name], value=-0.75)
    _check(api, oracle, mat, CHUNK, nt_stores=(0, 1), new_value=3.0)
