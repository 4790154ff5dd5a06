"""spmvHipSpGEMM and spmvHipSpGEMMRefresh are declared, exported and bound in Python with the C layout of spmvSpgemmOpts /
spmvSpgemmInfo, and the test side's reference (tests/spgemm_ref.py) is the loop of include/spmvHip.h: the vectorised form
equals the plain loop as bits on every small case, integer-valued inputs give the dense product exactly with the
structural pattern, rows ascend strictly, and reversing A's stored order changes a bit -- so the inputs can see a wrong
order.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import serial_order_inputs as si
import spgemm_ref as sr
from c_header import HEADER, code as _code
from conftest import ROOT

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H = r"spmat\s*\*\s*\w+"
DECLS = {
    "spmvHipSpGEMM": (H + r"\s*,\s*" + H + r"\s*,\s*const\s+spmvSpgemmOpts\s*\*\s*\w+\s*,\s*" + H + r"\s*,\s*spmvSpgemmInfo\s*\*\s*\w+", 5),
    "spmvHipSpGEMMRefresh": (H + r"\s*,\s*" + H + r"\s*,\s*" + H + r"\s*,\s*spmvSpgemmInfo\s*\*\s*\w+", 4),
}
OPTS = ("waveMaxProducts", "groupMaxProducts", "sortBudgetBytes")
INFO = ("products", "nnzC", "maxRowProducts", "maxRowNnz", "rowsWave", "rowsGroup", "rowsSorted", "sortBatches", "tempBytes",
        "symbolicMs", "numericMs", "ms")
CASES = sr.small_cases()
CASES["nan"] = sr.nan_case()


def test_header_declares_both_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in (("spmvSpgemmOpts", OPTS), ("spmvSpgemmInfo", INFO)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body, struct
        names = [n for decl in body.group(1).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == list(fields), (struct, names)


def test_library_exports_both():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_both():
    from spmv_openmp_cuda_amd import api
    for name, (_, nargs) in DECLS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == nargs, name
    for m in ("multiply", "multiply_refresh", "spgemm_info"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert [f[0] for f in api.spmvSpgemmOpts._fields_] == list(OPTS)
    assert [f[0] for f in api.spmvSpgemmInfo._fields_] == list(INFO)


@pytest.mark.parametrize("name", list(CASES))
def test_vectorised_reference_is_the_loop(name):
    A, B = CASES[name]
    R = sr.spgemm_ref(A, B)
    sr.same_bits(R, sr.spgemm_loop(A, B), name)
    assert np.array_equal(R[4].view(np.uint64)[~np.isnan(R[4])], sr.spgemm_loop(A, B)[4].view(np.uint64)[~np.isnan(R[4])])
    irp, ja = R[2].astype(np.int64), R[3].astype(np.int64)
    inner = np.diff(si.row_of_entry(R[2])) == 0
    assert np.all(np.diff(ja)[inner] > 0), f"{name}: rows of C must ascend strictly"
    assert int(irp[-1]) == ja.size and np.all(np.diff(irp) >= 0)
    assert int(sr.row_products(A, B).sum()) == sr.products(A, B)[2].size


def test_special_values_are_among_the_cases():
    C_ = sr.spgemm_ref(*CASES["special"])[4]
    assert np.isinf(C_).any() and not np.isnan(C_).any()
    Cz = sr.spgemm_ref(*CASES["cancel"])
    assert Cz[4].size and np.all(Cz[4].view(np.uint64) == 0), "sums that cancel are stored, as +0.0"
    assert np.all(sr.spgemm_ref(*CASES["negzero"])[4].view(np.uint64)[:1] == 0), "(-0.0) + (-0.0) after +0.0 is +0.0"
    assert np.isnan(sr.spgemm_ref(*CASES["nan"])[4]).any()
    A, B = CASES["mixed37x53x29"]
    ja = B[3][int(B[2][5]):int(B[2][6])]
    assert ja[10] == ja[40] == 3 and np.count_nonzero(ja == 3) == 2
    ja = B[3][int(B[2][9]):int(B[2][10])]
    assert ja[2] == ja[67] == 7 and np.count_nonzero(ja == 7) == 2
    assert {5, 9} <= set(A[3].tolist())


def test_integer_inputs_equal_the_dense_product_and_the_structural_pattern():
    rng = np.random.default_rng(2210)
    pairs = [CASES["integer"], (sr.random_csr(rng, 30, 40, rng.integers(0, 9, 30), sr.integer_values),
                                sr.random_csr(rng, 40, 25, rng.integers(0, 9, 40), sr.integer_values))]
    for A, B in pairs:
        R = sr.spgemm_ref(A, B)
        assert np.array_equal(sr.dense(R), sr.dense(A) @ sr.dense(B))
        assert np.array_equal(sr.pattern_of(R), sr.structural(A, B))
        assert np.count_nonzero(R[4] == 0.0), "some stored sum is 0.0: the pattern is structural, not numerical"


def test_reversing_a_rows_changes_bits():
    """the order-sensitive values of serial_order_inputs: another (p, q) order shows in the bits"""
    rng = np.random.default_rng(2211)
    A = sr.random_csr(rng, 40, 12, 10)
    B = sr.random_csr(rng, 12, 9, 6)
    R, Rrev = sr.spgemm_ref(A, B), sr.spgemm_ref(sr.reverse_rows(A), B)
    assert np.array_equal(R[2], Rrev[2]) and np.array_equal(R[3], Rrev[3])
    changed = np.count_nonzero(R[4].view(np.uint64) != Rrev[4].view(np.uint64))
    assert changed > R[4].size // 10, changed
    Rb = sr.spgemm_ref(A, sr.reverse_rows(B))                       # ... and B's stored order, through the repeats
    assert np.count_nonzero(R[4].view(np.uint64) != Rb[4].view(np.uint64)) > 0


def test_transpose_helper_is_the_stable_one():
    A, _ = CASES["mixed37x53x29"]
    T = sr.transpose(A)
    assert np.array_equal(sr.dense(T), sr.dense(A).T) or np.allclose(sr.dense(T), sr.dense(A).T)
    assert np.all(np.diff(T[3].astype(np.int64))[np.diff(si.row_of_entry(T[2])) == 0] >= 0)
