"""The ILU(0) entry points (hipSpILU0CSR, spmvHipIlu0Info) are declared, exported and bound in Python with the C layout of
spmvIluInfo, and the test side's two references (tests/ilu0_ref.py) agree bit for bit -- on inputs where another update
order gives other bits.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits, differing_rows
from c_header import HEADER, code as _code
from conftest import ROOT
from ilu0_ref import check_pattern, ilu0_crout, ilu0_kij, ilu0_levels, ilu0_loop
from test_trsv_abi import laplacian7, random_square

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
DECLS = {
    "hipSpILU0CSR": r"spmat\s*\*\s*\w+",
    "spmvHipIlu0Info": r"spmat\s*\*\s*\w+\s*,\s*spmvIluInfo\s*\*\s*\w+",
}
FIELDS = ("zeroPivot", "firstBadRow", "levels", "launches", "longRows", "factorisations", "ms")


def test_header_declares_the_two_and_the_struct():
    code = _code(HEADER)
    for name, params in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spmvIluInfo\s*;", code, re.S)
    assert body, "spmvIluInfo"
    assert re.findall(r"(\w+)\s*;", body.group(1)) == list(FIELDS)


def test_library_exports_the_two():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_two():
    from spmv_openmp_cuda_amd import api
    for name, n in (("hipSpILU0CSR", 1), ("spmvHipIlu0Info", 2)):
        assert name in api._sigs
        assert len(getattr(api.lib, name).argtypes) == n, name
    for m in ("ilu0", "ilu0_info"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert [f[0] for f in api.spmvIluInfo._fields_] == list(FIELDS)


# ------------------------------------------------------------------------------------------------- the references
def random_ilu(rng, M, per_row, e=2):
    """a square CSR with strictly ascending columns and one dominant diagonal per row; order-sensitive values"""
    IRP, JA, AS = random_square(rng, M, per_row, shuffle=False, repeats=False, e=e)
    rows = si.row_of_entry(IRP)
    keep = np.ones(JA.size, bool)
    keep[1:] = ~((rows[1:] == rows[:-1]) & (JA[1:] == JA[:-1]))          # drop repeated columns
    return si.assemble(M, rows[keep], JA[keep].astype(np.int64), AS[keep])


def chain(rng, M):
    """a tridiagonal matrix: M lower levels of one row"""
    i = np.arange(M)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[1:] - 1, i, i[:-1] + 1])
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    vals = np.where(rows == cols, 3.0 + rng.random(rows.size), si.order_values(rng, rows.size, 1) / 3)
    return si.assemble(M, rows, cols, vals)


def stencil(rng, nx, ny, nz):
    IRP, JA, AS = laplacian7(nx, ny, nz)
    AS = np.where(AS == 6.0, 6.0 + rng.random(AS.size), si.order_values(rng, AS.size, 1) / 7)
    return IRP, JA, AS


def _same(a, ref, what):
    """finite values by bits, infinities by sign, NaN as NaN"""
    a, ref = np.asarray(a), np.asarray(ref)
    fin = np.isfinite(ref)
    assert_same_bits(a[fin], ref[fin], what)
    inf = np.isinf(ref)
    assert np.array_equal(a[inf], ref[inf]), what
    assert np.isnan(a[np.isnan(ref)]).all(), what


@pytest.mark.parametrize("M,per_row,seed", [(1, 0, 1), (5, 3, 2), (60, 6, 3), (300, 9, 4), (400, 30, 5)])
def test_numpy_reference_is_the_loop_random(M, per_row, seed):
    rng = np.random.default_rng(seed)
    IRP, JA, AS = random_ilu(rng, M, per_row)
    _same(ilu0_levels(M, IRP, JA, AS), ilu0_loop(M, IRP, JA, AS), "random")


def test_numpy_reference_is_the_loop_stencil_and_chain():
    rng = np.random.default_rng(6)
    IRP, JA, AS = stencil(rng, 7, 6, 5)
    M = 7 * 6 * 5
    _same(ilu0_levels(M, IRP, JA, AS), ilu0_loop(M, IRP, JA, AS), "stencil")
    IRP, JA, AS = chain(rng, 500)
    _same(ilu0_levels(500, IRP, JA, AS), ilu0_loop(500, IRP, JA, AS), "chain")


def test_numpy_reference_zero_pivots():
    """a zero diagonal: later rows get +-Inf / NaN as the loop gives them, in both references"""
    rng = np.random.default_rng(7)
    M = 200
    IRP, JA, AS = random_ilu(rng, M, 6)
    dpos, _, _ = check_pattern(M, IRP, JA)
    AS = AS.copy()
    AS[dpos[[3, 60]]] = 0.0
    ref = ilu0_loop(M, IRP, JA, AS)
    assert not np.isfinite(ref).all()
    _same(ilu0_levels(M, IRP, JA, AS), ref, "zero pivots")


def test_pattern_rules():
    IRP, JA = np.array([0, 1, 3, 5]), np.array([0, 0, 1, 2, 1])
    assert check_pattern(3, IRP, JA)[1:] == (2, -1)              # row 2 unsorted
    IRP, JA = np.array([0, 1, 3, 6]), np.array([0, 0, 1, 1, 1, 2])
    assert check_pattern(3, IRP, JA)[1:] == (2, -1)              # row 2 repeats column 1
    IRP, JA = np.array([0, 1, 2, 4]), np.array([0, 0, 1, 2])
    assert check_pattern(3, IRP, JA)[1:] == (-1, 1)              # row 1 has no diagonal


def test_ilu_is_a_factorisation():
    """L U equals A on A's pattern (exactly up to rounding): the references compute ILU(0)"""
    rng = np.random.default_rng(8)
    nx, ny, nz = 5, 4, 3
    M = nx * ny * nz
    IRP, JA, AS = stencil(rng, nx, ny, nz)
    F = ilu0_loop(M, IRP, JA, AS)
    rows = si.row_of_entry(IRP)
    A, L, U = np.zeros((M, M)), np.eye(M), np.zeros((M, M))
    A[rows, JA] = AS
    low = JA < rows
    L[rows[low], JA[low]] = F[low]
    U[rows[~low], JA[~low]] = F[~low]
    assert np.allclose((L @ U)[rows, JA], AS, rtol=0, atol=1e-12)


def test_inputs_are_order_sensitive():
    """summing each entry's updates first and subtracting once (the Crout / dot-product form) gives other bits on these
    inputs, so the GPU tests can tell the loop's update order from another.  The right-looking KIJ order applies each
    entry's updates in the same ascending-k order, so it gives the loop's bits."""
    rng = np.random.default_rng(9)
    M = 150
    IRP, JA, AS = random_ilu(rng, M, 40, e=4)
    ref = ilu0_loop(M, IRP, JA, AS)
    crout = ilu0_crout(M, IRP, JA, AS)
    assert np.allclose(crout, ref, rtol=1e-9, atol=1e-12)
    assert differing_rows(crout, ref).size > JA.size // 10
    with pytest.raises(AssertionError):
        assert_same_bits(crout, ref)
    assert_same_bits(ilu0_kij(M, IRP, JA, AS), ref, "KIJ")
    rng = np.random.default_rng(10)
    IRP, JA, AS = stencil(rng, 12, 11, 10)
    M = 12 * 11 * 10
    assert differing_rows(ilu0_crout(M, IRP, JA, AS), ilu0_levels(M, IRP, JA, AS)).size > JA.size // 10
