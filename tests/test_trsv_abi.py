"""The triangular-solve entry points (spmvHipTriAnalyse, hipSpTRSVCSR, spmvHipTriInfo) are declared, exported and bound
in Python with the C layout of spmvTriInfo, and the test side's references (tests/trsv_ref.py) agree bit for bit on
inputs where another summation order gives other bits.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits, differing_rows
from c_header import HEADER, code as _code
from conftest import ROOT
from trsv_ref import diag_pos, levels, trsv_levels, trsv_loop

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
DECLS = {
    "spmvHipTriAnalyse": r"spmat\s*\*\s*\w+\s*,\s*int\s+\w+",
    "hipSpTRSVCSR": r"spmat\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+",
    "spmvHipTriInfo": r"spmat\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*spmvTriInfo\s*\*\s*\w+",
}
FIELDS = ("levels", "maxLevelRows", "launches", "fusedLevels", "longRows", "firstBadDiag", "analyses", "analysisMs", "bytes")


def test_header_declares_the_three():
    code = _code(HEADER)
    for name, params in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for const, value in (("SPMV_TRI_LOWER", 0), ("SPMV_TRI_UPPER", 1), ("SPMV_DIAG_STORED", 0), ("SPMV_DIAG_UNIT", 1)):
        assert re.search(r"#define\s+" + const + r"\s+" + str(value) + r"\b", code), const


def test_library_exports_the_three():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_three():
    from spmv_openmp_cuda_amd import api
    for name, n in (("spmvHipTriAnalyse", 2), ("hipSpTRSVCSR", 5), ("spmvHipTriInfo", 3)):
        assert name in api._sigs
        assert len(getattr(api.lib, name).argtypes) == n, name
    for m in ("solve_triangular", "triangular_analyse", "triangular_info"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert [f[0] for f in api.spmvTriInfo._fields_] == list(FIELDS)


# ------------------------------------------------------------------------------------------------- the references
def random_square(rng, M, per_row, diag="one", shuffle=True, repeats=True, e=2):
    """a square CSR: per_row random columns per row (repeated pairs when `repeats`), the diagonal once ("one"), twice in
    some rows ("twice"), or not at all ("none"); rows unsorted when `shuffle`.  Values order-sensitive; the diagonal
    dominates so that long chains stay finite."""
    lens = rng.integers(0, per_row + 1, M)
    rows = np.repeat(np.arange(M), lens)
    cols = rng.integers(0, M, rows.size)
    if repeats and rows.size:
        dup = rng.random(rows.size) < 0.15
        cols[dup] = np.maximum(rows[dup] - 1, 0)
    keep = cols != rows
    rows, cols = rows[keep], cols[keep]
    vals = si.order_values(rng, rows.size, e) / (per_row + 1)
    if diag != "none":
        d = np.arange(M)
        dv = rng.choice([-1.0, 1.0], M) * (1.5 + rng.random(M)) * 10.0 ** rng.integers(0, 2, M)
        rows, cols, vals = np.concatenate([rows, d]), np.concatenate([cols, d]), np.concatenate([vals, dv])
        if diag == "twice":
            t = d[rng.random(M) < 0.05]
            rows, cols, vals = np.concatenate([rows, t]), np.concatenate([cols, t]), np.concatenate([vals, np.ones(t.size)])
    o = rng.permutation(rows.size) if shuffle else np.lexsort((cols, rows))
    return si.assemble(M, rows[o], cols[o], vals[o])


def _same(x, ref, what):
    """finite rows by bits, infinities by sign, NaN as NaN"""
    x, ref = np.asarray(x), np.asarray(ref)
    fin = np.isfinite(ref)
    assert_same_bits(x[fin], ref[fin], what)
    inf = np.isinf(ref)
    assert np.array_equal(x[inf], ref[inf]), what
    assert np.isnan(x[np.isnan(ref)]).all(), what


@pytest.mark.parametrize("M,per_row,shuffle,seed", [(1, 0, False, 1), (5, 3, True, 2), (60, 6, False, 3), (300, 9, True, 4),
                                                     (400, 30, True, 5)])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("unit", [False, True])
def test_numpy_reference_is_the_loop(M, per_row, shuffle, seed, lower, unit):
    """whole matrices (both triangles stored) solved as lower and as upper, unsorted rows and repeated pairs, unit
    diagonals stored"""
    rng = np.random.default_rng(seed)
    IRP, JA, AS = random_square(rng, M, per_row, shuffle=shuffle)
    b = si.order_values(rng, M)
    _same(trsv_levels(M, IRP, JA, AS, b, lower, unit), trsv_loop(M, IRP, JA, AS, b, lower, unit), "numpy vs loop")


@pytest.mark.parametrize("lower", [True, False])
def test_numpy_reference_unit_without_diagonal_and_zero_diagonals(lower):
    rng = np.random.default_rng(17)
    M = 200
    IRP, JA, AS = random_square(rng, M, 5, diag="none")
    b = si.order_values(rng, M)
    _same(trsv_levels(M, IRP, JA, AS, b, lower, True), trsv_loop(M, IRP, JA, AS, b, lower, True), "no diagonal, unit")
    IRP, JA, AS = random_square(rng, M, 5)
    dpos, bad = diag_pos(M, IRP, JA)
    assert bad == -1
    AS = AS.copy()
    AS[dpos[[3, 50, 120]]] = 0.0                          # +-Inf and NaN that propagate
    ref = trsv_loop(M, IRP, JA, AS, b, lower, False)
    assert not np.isfinite(ref).all()
    _same(trsv_levels(M, IRP, JA, AS, b, lower, False), ref, "zero diagonals")


def test_diagonal_rule():
    rng = np.random.default_rng(18)
    IRP, JA, AS = random_square(rng, 100, 4, diag="twice")
    _, bad = diag_pos(100, IRP, JA)
    assert bad >= 0
    IRP, JA, AS = random_square(rng, 100, 4, diag="none")
    assert diag_pos(100, IRP, JA)[1] == 0


def test_levels_of_a_stencil_and_a_chain():
    nx, ny, nz = 6, 5, 4
    IRP, JA, _ = laplacian7(nx, ny, nz)
    M = nx * ny * nz
    assert levels(M, IRP, JA, True).max() + 1 == nx + ny + nz - 2
    assert levels(M, IRP, JA, False).max() + 1 == nx + ny + nz - 2
    IRP, JA = np.array([0, 1, 3, 5], np.uint64), np.array([0, 0, 1, 1, 2], np.uint64)
    assert list(levels(3, IRP, JA, True)) == [0, 1, 2]


def laplacian7(nx, ny, nz):
    """the 7-point Laplacian on an nx x ny x nz grid (x fastest), diagonal included, columns sorted"""
    M = nx * ny * nz
    i = np.arange(M)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    rows, cols = [i], [i]
    for ok, off in ((z > 0, -nx * ny), (y > 0, -nx), (x > 0, -1), (x < nx - 1, 1), (y < ny - 1, nx), (z < nz - 1, nx * ny)):
        rows.append(i[ok])
        cols.append(i[ok] + off)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    o = np.lexsort((cols, rows))
    vals = np.where(rows[o] == cols[o], 6.0, -1.0)
    return si.assemble(M, rows[o], cols[o], vals)


def test_inputs_are_order_sensitive():
    """adding each row's products in reverse stored order gives other bits on these inputs: the GPU tests can tell the
    stored order from another"""
    rng = np.random.default_rng(19)
    M = 2000
    IRP, JA, AS = random_square(rng, M, 12)
    b = si.order_values(rng, M)
    x = trsv_levels(M, IRP, JA, AS, b, True, False)
    perm = si.reversed_rows(IRP)
    x_rev = trsv_levels(M, IRP, JA[perm], AS[perm], b, True, False)
    assert differing_rows(x, x_rev).size > M // 10
    with pytest.raises(AssertionError):
        assert_same_bits(x_rev, x)
    IRP2, JA2, AS2 = random_square(rng, M, 12, e=4)       # and with values as spread as serial_order_inputs.order_values
    b2 = si.order_values(rng, M)
    p2 = si.reversed_rows(IRP2)
    assert differing_rows(trsv_levels(M, IRP2, JA2, AS2, b2), trsv_levels(M, IRP2, JA2[p2], AS2[p2], b2)).size > M // 4
