"""The transpose entry points (spmvHipCsrTranspose, spmvHipTransposeRefresh) are declared, exported and bound in Python,
and the test side's stable transpose (tests/transpose_ref.py) is the scatter loop's order -- an order the GPU tests can
tell from an unstable one.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits, differing_rows
from c_header import HEADER, code as _code
from conftest import ROOT
from transpose_ref import scatter_serial, stable_transpose

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
NAMES = ("spmvHipCsrTranspose", "spmvHipTransposeRefresh")


def test_header_declares_both():
    code = _code(HEADER)
    for name in NAMES:
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*spmat\s*\*\s*\w+\s*,\s*spmat\s*\*\s*\w+\s*\)\s*;", code, re.M), name


def test_library_exports_both():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert name in syms, name


def test_python_binds_both():
    from spmv_openmp_cuda_amd import api
    for name in NAMES:
        assert name in api._sigs
        assert len(getattr(api.lib, name).argtypes) == 2
    assert callable(api.DeviceMatrix.transpose) and callable(api.DeviceMatrix.refresh_from)


def _small(rng, M, N, nnz, shuffle):
    """entries in random rows and columns with repeats; rows unsorted when `shuffle`; row 0, the last row and the last
    column empty"""
    rows = rng.integers(1, max(M - 1, 2), nnz) if M > 2 else rng.integers(0, max(M, 1), nnz)
    cols = rng.integers(0, max(N - 1, 1), nnz)
    cols[rng.random(nnz) < 0.2] = 3 % max(N - 1, 1)                       # many entries of one column
    if not shuffle:
        o = np.lexsort((cols, rows))
        rows, cols = rows[o], cols[o]
    return si.assemble(M, rows, cols, si.order_values(rng, nnz))


@pytest.mark.parametrize("M,N,nnz,shuffle", [(7, 5, 20, False), (7, 5, 20, True), (40, 90, 600, True), (90, 40, 600, True),
                                             (1, 6, 9, True), (6, 1, 9, True), (5, 4, 0, False), (0, 4, 0, False),
                                             (4, 0, 0, False)])
def test_helper_is_the_scatter_loop(oracle, M, N, nnz, shuffle):
    rng = np.random.default_rng(M * 1000 + N + nnz + shuffle)
    IRP, JA, AS = _small(rng, M, N, nnz, shuffle) if N and M else (np.zeros(M + 1, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    x = si.order_values(rng, M)
    IRPt, JAt, ASt, order = stable_transpose(N, IRP, JA, AS)
    assert IRPt.size == N + 1 and int(IRPt[-1]) == JA.size
    assert np.all(np.diff(JAt.astype(np.int64))[np.diff(si.row_of_entry(IRPt)) == 0] >= 0)     # rows non-decreasing
    assert_same_bits(oracle.csr_serial(IRPt, JAt, ASt, x), scatter_serial(M, N, IRP, JA, AS, x), "stable transpose")


def test_unstable_order_gives_other_bits(oracle):
    """Equal columns taken in another order than the CSR position order (ties reversed: what an unstable sort may do)
    change the bits of the transposed product on the GPU tests' kind of input."""
    inp = si.make("mixed")
    IRPt, JAt, ASt, order = stable_transpose(inp.N, inp.IRP, inp.JA, inp.AS)
    x = si.order_values(np.random.default_rng(3), inp.M)
    y = oracle.csr_serial(IRPt, JAt, ASt, x)
    JA = inp.JA.astype(np.int64)
    rev = np.lexsort((-np.arange(JA.size), JA))                          # by column, ties in reverse position order
    rows = si.row_of_entry(inp.IRP)
    y_rev = oracle.csr_serial(IRPt, rows[rev].astype(np.uint64), inp.AS[rev], x)
    assert differing_rows(y, y_rev).size > inp.N // 4
    with pytest.raises(AssertionError):
        assert_same_bits(y_rev, y)
