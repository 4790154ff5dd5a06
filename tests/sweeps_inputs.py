"""The matrices of the sweep-solve tests (tests/test_sweeps_abi.py on the host, tests/test_gpu_tri_sweeps*.py on the device),
small on purpose: every shape at which the sweep kernels take another path.  A workgroup owns consecutive rows whose entries
are one span of at most SPAN = 2 048 entries and at most MAX_ROWS = 512 rows; a longer row is a block of its own.

make(name) -> (M, IRP, JA, AS, b): whole square matrices (both triangles stored) with order-sensitive values, unsorted rows
and repeated (i, j) pairs unless the name says otherwise; b order-sensitive."""
import numpy as np

import serial_order_inputs as si
from test_trsv_abi import random_square
from trsv_ref import diag_pos, levels

SPAN, MAX_ROWS = 2048, 512
NAMES = ("m1", "r63", "r64", "r65", "span_edge", "short_rows", "long_rows", "diag_only", "pattern", "bad_diagonals", "bad_b")


def sweep_counts(M, IRP, JA, lower):
    """S in {0, 1, 2, 3, levels - 1, levels + 1} of that triangle (sorted, distinct) and the levels"""
    L = int(levels(M, IRP, JA, lower).max()) + 1 if M else 0
    return sorted({0, 1, 2, 3, max(L - 1, 0), L + 1}), L


def _long_rows(rng):
    """2 300 rows of a few entries, and one row of more than SPAN strict entries in each triangle (repeats, unsorted): row
    2 250 reads 2 100 times below itself, row 10 reads 2 100 times above itself"""
    M = 2300
    IRP, JA, AS = random_square(rng, M, 4)
    rows, cols, vals = si.row_of_entry(IRP), JA.astype(np.int64), AS
    lo, up = rng.integers(0, 2250, 2100), rng.integers(11, M, 2100)
    rows = np.concatenate([rows, np.full(2100, 2250), np.full(2100, 10)])
    cols = np.concatenate([cols, lo, up])
    vals = np.concatenate([vals, si.order_values(rng, 4200, 2) / 4000])
    o = rng.permutation(rows.size)
    return M, si.assemble(M, rows[o], cols[o], vals[o])


def make(name):
    rng = np.random.default_rng(4000 + NAMES.index(name))
    if name == "m1":
        M, (IRP, JA, AS) = 1, (np.array([0, 1], np.uint64), np.array([0], np.uint64), np.array([-1.75]))
    elif name in ("r63", "r64", "r65"):
        M = int(name[1:])
        IRP, JA, AS = random_square(rng, M, 6)
    elif name == "span_edge":
        # ~5 000 entries in rows of 0 .. 13: three spans, each closed in front of the row that would cross entry 2 048 of it
        M = 700
        IRP, JA, AS = random_square(rng, M, 12)
        assert int(IRP[-1]) > 2 * SPAN and SPAN % int(np.diff(IRP).max()) != 0
    elif name == "short_rows":
        # more than MAX_ROWS rows inside one span's entries: the row limit closes the blocks, and a lane owns two rows
        M = 1300
        IRP, JA, AS = random_square(rng, M, 1)
        assert int(IRP[MAX_ROWS]) < SPAN
    elif name == "long_rows":
        M, (IRP, JA, AS) = _long_rows(rng)
        lens = np.diff(IRP.astype(np.int64))
        assert lens[2250] > SPAN and lens[10] > SPAN
    elif name == "diag_only":
        M = 130
        i = np.arange(M)
        IRP, JA, AS = si.assemble(M, i, i, rng.choice([-1.0, 1.0], M) * (1.0 + rng.random(M)))
    elif name == "pattern":
        # every stored value the same double: a unit-value handle (the kernels take the value from a register)
        M = 300
        IRP, JA, AS = random_square(rng, M, 4)
        AS = np.full(AS.size, 0.5)
    elif name == "bad_diagonals":
        M = 200
        IRP, JA, AS = random_square(rng, M, 5)
        dpos, bad = diag_pos(M, IRP, JA)
        assert bad == -1
        AS = AS.copy()
        AS[dpos[[3, 50, 120]]] = [0.0, np.nan, np.inf]
    elif name == "bad_b":
        M = 200
        IRP, JA, AS = random_square(rng, M, 5)
    else:
        raise KeyError(name)
    b = si.order_values(rng, M)
    if name == "bad_b":
        b[[7, 90, 150]] = [np.nan, np.inf, -np.inf]
    return M, IRP, JA, AS, b
