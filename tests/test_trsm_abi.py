"""The block triangular solve (hipSpTRSMCSR; DeviceMatrix.solve_triangular_block) is declared, exported and bound in
Python, and the test side's reference for it (tests/trsm_ref.py) gives, column by column, the bits of the serial loop of
tests/trsv_ref.py.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import serial_order_inputs as si
from c_header import HEADER, code as _code
from conftest import ROOT
from test_trsv_abi import _same, random_square
from trsm_ref import trsm_levels
from trsv_ref import diag_pos, trsv_loop

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
NAME = "hipSpTRSMCSR"
PARAMS = (r"spmat\s*\*\s*dA\s*,\s*int\s+uplo\s*,\s*int\s+diag\s*,\s*unsigned\s+k\s*,\s*const\s+double\s*\*\s*dB\s*,\s*size_t\s+ldb\s*,"
          r"\s*int\s+bLayout\s*,\s*double\s*\*\s*dX\s*,\s*size_t\s+ldx\s*,\s*int\s+xLayout")


def test_header_declares_it():
    assert re.search(r"^\s*int\s+" + NAME + r"\s*\(\s*" + PARAMS + r"\s*\)\s*;", _code(HEADER), re.M)


def test_library_exports_it():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert NAME in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_python_binds_it():
    from spmv_openmp_cuda_amd import api
    assert NAME in api._sigs
    assert len(getattr(api.lib, NAME).argtypes) == 10


def test_python_has_the_method():
    from spmv_openmp_cuda_amd import api
    assert callable(getattr(api.DeviceMatrix, "solve_triangular_block"))


# ------------------------------------------------------------------------------------------------- the reference
def block_of_columns(rng, M, k):
    """(M, k): every column a distinct order-sensitive vector"""
    return np.stack([si.order_values(rng, M) for _ in range(k)], axis=1) if k else np.zeros((M, 0))


def _columns_are_the_loop(M, IRP, JA, AS, B, lower, unit, what):
    X = trsm_levels(M, IRP, JA, AS, B, lower, unit)
    assert X.shape == B.shape
    for c in range(B.shape[1]):
        _same(X[:, c], trsv_loop(M, IRP, JA, AS, B[:, c], lower, unit), f"{what}, column {c}")
    return X


@pytest.mark.parametrize("M,per_row,shuffle,seed", [(5, 3, True, 2), (60, 6, False, 3), (300, 9, True, 4)])
@pytest.mark.parametrize("k", [1, 3, 17])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("unit", [False, True])
def test_block_reference_is_the_loop_per_column(M, per_row, shuffle, seed, k, lower, unit):
    rng = np.random.default_rng(2600 + seed)
    IRP, JA, AS = random_square(rng, M, per_row, shuffle=shuffle)
    _columns_are_the_loop(M, IRP, JA, AS, block_of_columns(rng, M, k), lower, unit, f"M {M}, k {k}")


@pytest.mark.parametrize("M,per_row,shuffle,rows", [(5, 3, True, (0, 2, 4)), (60, 6, False, (3, 20, 41)), (300, 9, True, (3, 50, 120))])
@pytest.mark.parametrize("k", [1, 3, 17])
@pytest.mark.parametrize("lower", [True, False])
def test_block_reference_zero_diagonals(M, per_row, shuffle, rows, k, lower):
    """zero stored diagonals at three rows: +-Inf and NaN that propagate, per column, as in the loop"""
    rng = np.random.default_rng(2610 + M)
    IRP, JA, AS = random_square(rng, M, per_row, shuffle=shuffle)
    dpos, bad = diag_pos(M, IRP, JA)
    assert bad == -1
    AS = AS.copy()
    AS[dpos[list(rows)]] = 0.0
    X = _columns_are_the_loop(M, IRP, JA, AS, block_of_columns(rng, M, k), lower, False, f"zero diagonals, M {M}, k {k}")
    assert not np.isfinite(X).all()


@pytest.mark.parametrize("M,per_row,shuffle", [(5, 3, True), (60, 6, False), (300, 9, True)])
@pytest.mark.parametrize("k", [1, 3, 17])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("unit", [False, True])
def test_block_reference_nan_column_stays_in_its_column(M, per_row, shuffle, k, lower, unit):
    """one column of B all NaN: that column is the loop's, every other column has the bits it has without the NaN column"""
    rng = np.random.default_rng(2620 + M)
    IRP, JA, AS = random_square(rng, M, per_row, shuffle=shuffle)
    B = block_of_columns(rng, M, k)
    clean = trsm_levels(M, IRP, JA, AS, B, lower, unit)
    nan_col = k // 2
    B2 = B.copy()
    B2[:, nan_col] = np.nan
    X = _columns_are_the_loop(M, IRP, JA, AS, B2, lower, unit, f"NaN column, M {M}, k {k}")
    assert np.isnan(X[:, nan_col]).all()
    others = [c for c in range(k) if c != nan_col]
    _same(X[:, others], clean[:, others], "the other columns")
