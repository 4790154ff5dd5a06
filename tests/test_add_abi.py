"""spmvHipCsrAdd and spmvHipCsrAddRefresh are declared, exported and bound in Python, and the test side's reference
(tests/add_ref.py) is the loop of include/spmvHip.h: the vectorised form equals the plain loop as bits on every small case,
integer-valued inputs give the dense alpha A + beta B exactly with the union pattern, rows ascend strictly, A + (-1) A
stores +0.0 at every place of A, and reversing the stored order of a row with a repeated column changes a bit -- so the
inputs can see a wrong order.  The smoothed prolongator composed from the references equals the dense one.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import add_ref as ar
import serial_order_inputs as si
from c_header import HEADER, code as _code
from conftest import ROOT

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H = r"spmat\s*\*\s*\w+"
D = r"double\s+\w+"
SEP = r"\s*,\s*"
DECLS = {
    "spmvHipCsrAdd": (SEP.join([D, H, D, H, r"const\s+spmvAddOpts\s*\*\s*\w+", H, r"spmvAddInfo\s*\*\s*\w+"]), 7),
    "spmvHipCsrAddRefresh": (SEP.join([H, D, H, D, H, r"spmvAddInfo\s*\*\s*\w+"]), 6),
}
OPTS = ("laneMaxTerms", "waveMaxTerms", "sortBudgetBytes", "allSorted")
INFO = ("terms", "nnzC", "maxRowTerms", "maxRowNnz", "rowsLane", "rowsWave", "rowsSorted", "sortBatches", "tempBytes",
        "symbolicMs", "numericMs", "ms")
CASES = ar.small_cases()
CASES["nan"] = ar.nan_case()


def test_header_declares_both_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in (("spmvAddOpts", OPTS), ("spmvAddInfo", INFO)):
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
    for m in ("add", "add_refresh", "add_info"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert [f[0] for f in api.spmvAddOpts._fields_] == list(OPTS)
    assert [f[0] for f in api.spmvAddInfo._fields_] == list(INFO)


def _inner_ascends(R):
    inner = np.diff(si.row_of_entry(R[2])) == 0
    return np.all(np.diff(R[3].astype(np.int64))[inner] > 0)


@pytest.mark.parametrize("name", list(CASES))
def test_vectorised_reference_is_the_loop(name):
    alpha, A, beta, B = CASES[name]
    R = ar.add_ref(alpha, A, beta, B)
    ar.same_bits(R, ar.add_loop(alpha, A, beta, B), name)
    assert _inner_ascends(R), f"{name}: rows of C must ascend strictly"
    irp = R[2].astype(np.int64)
    assert int(irp[-1]) == R[3].size and np.all(np.diff(irp) >= 0)
    union = (ar.dense(A[:4] + (np.ones(A[3].size),)) + ar.dense(B[:4] + (np.ones(B[3].size),))) > 0
    assert R[3].size == np.count_nonzero(union), f"{name}: the union pattern, nothing dropped"
    assert int(ar.row_terms(A, B).sum()) == A[3].size + B[3].size


def test_special_values_are_among_the_cases():
    _, A, _, B = CASES["special"]
    R = ar.add_ref(*CASES["special"])
    assert np.isinf(R[4]).any() and np.isnan(R[4]).any(), "+-Inf, and -Inf + Inf"
    assert B[4].view(np.uint64)[0] == 1 << 63 and int(B[3][0]) == 0 and 0 not in A[3][:4].tolist()
    assert (int(R[3][0]), int(R[4].view(np.uint64)[0])) == (0, 0), "a -0.0 alone in its column gives +0.0"
    Z = ar.add_ref(*CASES["special alpha=0"])
    assert Z[3].size == R[3].size and np.isnan(Z[4]).any(), "alpha = 0 keeps A's pattern, and 0 * Inf is a NaN at its place"
    N = ar.add_ref(*CASES["negzero"])
    assert not N[4].view(np.uint64)[:2].any(), "(0.0 + -0.0) + -0.0 is +0.0"
    assert np.isnan(ar.add_ref(*CASES["nan"])[4]).any()
    _, A, _, B = CASES["mixed37x53"]
    assert np.count_nonzero(A[3][int(A[2][3]):int(A[2][4])] == 7) >= 3 and np.count_nonzero(B[3][int(B[2][3]):int(B[2][4])] == 7) >= 2
    assert not ar.row_plain(A).all() and not ar.row_plain(B).all()
    P, Q = ar.plain_rows(np.random.default_rng(0))
    assert ar.row_plain(P).all() and ar.row_plain(Q).all() and ar.row_terms(P, Q).max() <= 24


def test_integer_inputs_equal_the_dense_sum_and_the_union_pattern():
    rng = np.random.default_rng(2510)
    quads = [CASES["integer"], (-4.0, ar.random_csr(rng, 30, 40, rng.integers(0, 9, 30), ar.integer_values), 5.0,
                                ar.random_csr(rng, 30, 40, rng.integers(0, 9, 30), ar.integer_values))]
    for alpha, A, beta, B in quads:
        R = ar.add_ref(alpha, A, beta, B)
        assert np.array_equal(ar.dense(R), alpha * ar.dense(A) + beta * ar.dense(B))
        pattern = np.zeros((R[0], R[1]), dtype=bool)
        pattern[si.row_of_entry(R[2]), R[3].astype(np.int64)] = True
        union = np.zeros_like(pattern)
        for X in (A, B):
            union[si.row_of_entry(X[2]), X[3].astype(np.int64)] = True
        assert np.array_equal(pattern, union)
        assert np.count_nonzero(R[4] == 0.0), "some stored sum is 0.0: the pattern is structural, not numerical"


def test_reversing_a_row_with_a_repeated_column_changes_bits():
    """every row of A holds one column six times with the order-sensitive values of serial_order_inputs: another stored
    order shows in the bits"""
    rng = np.random.default_rng(2511)
    A = ar.csr(40, 12, np.repeat(np.arange(40), 6), np.repeat(rng.integers(0, 12, 40), 6), si.order_values(rng, 240))
    B = ar.random_csr(rng, 40, 12, 5)
    R, Rrev = ar.add_ref(1.0, A, 1.0, B), ar.add_ref(1.0, ar.reverse_rows(A), 1.0, B)
    assert np.array_equal(R[2], Rrev[2]) and np.array_equal(R[3], Rrev[3])
    changed = np.count_nonzero(R[4].view(np.uint64) != Rrev[4].view(np.uint64))
    assert changed > 4, changed
    Rb = ar.add_ref(1.0, A, 1.0, ar.reverse_rows(B))               # ... and B's stored order, through its repeats
    assert np.count_nonzero(R[4].view(np.uint64) != Rb[4].view(np.uint64)) > 0
    Rs = ar.add_ref(1.0, B, 1.0, A)                                # ... and which operand comes first
    assert np.array_equal(R[3], Rs[3]) and np.count_nonzero(R[4].view(np.uint64) != Rs[4].view(np.uint64)) > 0


def test_a_minus_a_stores_plus_zero_at_every_place_of_a():
    alpha, A, beta, B = CASES["cancel"]
    R = ar.add_ref(alpha, A, beta, B)
    places = np.unique(si.row_of_entry(A[2]) * A[1] + A[3].astype(np.int64))
    assert np.array_equal(si.row_of_entry(R[2]) * R[1] + R[3].astype(np.int64), places)
    T = ar.sorted_csr(np.random.default_rng(2512), 30, 50, 9)      # no repeats: every place is a - a exactly
    Z = ar.add_ref(1.0, T, -1.0, T)
    assert Z[3].size == T[3].size and not Z[4].view(np.uint64).any(), "sums that cancel are stored, as +0.0"


def test_smoothed_prolongator_of_the_references_is_the_dense_one():
    A = ar.laplacian7(6, 5, 4)
    T = ar.aggregation(6, 5, 4)
    omega = 2.0 / 3.0
    P = ar.smoothed_prolongator(A, T, omega)
    dA, dT = ar.dense(A), ar.dense(T)
    assert np.allclose(ar.dense(P), dT - omega * (np.diag(1.0 / np.diag(dA)) @ dA @ dT))
    assert _inner_ascends(P) and (P[0], P[1]) == (T[0], T[1])


def test_class_rule_of_the_reference():
    A, B = ar.plain_rows(np.random.default_rng(1))
    t = ar.row_terms(A, B)
    assert ar.classes(A, B) == (np.count_nonzero(t), 0, 0)
    assert ar.classes(A, B, laneMax=4, waveMax=10) == (np.count_nonzero((t > 0) & (t <= 4)), np.count_nonzero((t > 4) & (t <= 10)),
                                                       np.count_nonzero(t > 10))
    assert ar.classes(A, B, allSorted=True) == (0, 0, np.count_nonzero(t))
    assert ar.classes(ar.reverse_rows(A), B)[2] == np.count_nonzero(np.diff(A[2].astype(np.int64)) > 1)
