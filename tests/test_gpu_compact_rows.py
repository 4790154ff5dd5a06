"""spmvHipCompactRows: the step after an all-gather of equally padded row blocks.  Block p of dYPad (maxRows doubles)
holds rows bounds[p] .. bounds[p+1]; they are copied back to back into dY.  Uneven blocks, empty ones included; the
padding is never read into y; a block longer than maxRows is refused with y left as it was."""
import ctypes as C

import numpy as np
import pytest

from bits import assert_same_bits

pytestmark = pytest.mark.gpu

POISON = np.array([0x7FF8DEADDEADDEAD], dtype=np.uint64).view(np.float64)[0]
GUARD = 64


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


def _padded(rng, bounds, max_rows):
    """(dYPad on the host: every block's rows, then poison in its padding; the compacted rows expected)"""
    n_parts = bounds.size - 1
    pad = np.full(n_parts * max_rows, POISON)
    want = rng.uniform(-1, 1, int(bounds[-1])) * 2.0 ** rng.integers(-30, 31, int(bounds[-1]))
    for p in range(n_parts):
        r0, r1 = int(bounds[p]), int(bounds[p + 1])
        pad[p * max_rows:p * max_rows + r1 - r0] = want[r0:r1]
    return pad, want


@pytest.mark.parametrize("bounds", [[0, 300, 300, 750, 751, 1000], [0, 0, 0, 5], [0, 7], [0, 1, 2, 3, 3, 3, 900]])
@pytest.mark.parametrize("slack", [0, 3])
def test_blocks_are_copied_back_to_back(api, bounds, slack):
    bounds = np.array(bounds, dtype=np.uint64)
    M = int(bounds[-1])
    max_rows = int(np.diff(bounds.astype(np.int64)).max()) + slack
    pad, want = _padded(np.random.default_rng(M + slack), bounds, max_rows)
    d_pad = api.DeviceBuffer(pad.nbytes).up(pad)
    dy = api.DeviceVector(M + GUARD)
    dy.poison()
    try:
        assert api.lib.spmvHipCompactRows(dy.ptr, d_pad.ptr, bounds.ctypes.data_as(C.c_void_p), bounds.size - 1,
                                          max_rows) == 0
        assert api.lib.spmvHipDeviceSynchronize() == 0
        y = dy.down()
        assert_same_bits(y[:M], want, f"bounds {bounds.tolist()}, maxRows {max_rows}")
        assert (y[M:].view(np.uint64) == np.uint64(0x7FF8DEADDEADDEAD)).all(), "written past the last row"
    finally:
        d_pad.free()
        dy.free()


def test_a_block_longer_than_the_pad_is_refused(api, capfd):
    """the long block is the third: nothing of the first two may have been copied either"""
    bounds = np.array([0, 300, 300, 750, 751, 1000], dtype=np.uint64)
    max_rows = 449
    pad, _ = _padded(np.random.default_rng(5), bounds[:3], max_rows)
    pad = np.concatenate([pad, np.ones(3 * max_rows)])
    d_pad = api.DeviceBuffer(pad.nbytes).up(pad)
    dy = api.DeviceVector(1000 + GUARD)
    before = np.arange(1000 + GUARD, dtype=np.float64)
    dy.up(before)
    try:
        assert api.lib.spmvHipCompactRows(dy.ptr, d_pad.ptr, bounds.ctypes.data_as(C.c_void_p), 5, max_rows) != 0
        assert "block 2 has 450 rows > pad 449" in capfd.readouterr().err
        assert api.lib.spmvHipDeviceSynchronize() == 0
        assert_same_bits(dy.down(), before, "y after a refused compaction")
    finally:
        d_pad.free()
        dy.free()
