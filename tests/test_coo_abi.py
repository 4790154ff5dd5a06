"""spmvHipCooAssemble / spmvHipCooAssembleRefresh / spmvHipCsrToCoo are declared, exported and bound in Python with the C
layout, and the test side's reference (tests/coo_ref.py) is the loop of include/spmvHip.h: it tells the orders of a run
apart -- so a device test that passes is evidence of the order, not only of the set --, it agrees with
serial_order_inputs.assemble where nothing repeats, skipped places are never read, and a refresh over the build's runs equals
a fresh assembly.  No GPU needed."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import coo_ref as cr
import serial_order_inputs as si
import spgemm_ref as sr
from c_header import HEADER, code as _code, run_c
from conftest import ROOT

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H = r"spmat\s*\*\s*\w+"
UL = r"ulong\s+\w+"
U32 = r"const\s+uint32_t\s*\*\s*\w+"
F64 = r"const\s+double\s*\*\s*\w+"
SEP = r"\s*,\s*"
DECLS = {
    "spmvHipCooAssemble": (SEP.join([UL, UL, UL, U32, U32, F64, r"const\s+spmvCooOpts\s*\*\s*\w+", H, r"spmvCooInfo\s*\*\s*\w+"]), 9),
    "spmvHipCooAssembleRefresh": (SEP.join([H, UL, F64, r"spmvCooInfo\s*\*\s*\w+"]), 4),
    "spmvHipCsrToCoo": (SEP.join([H, r"uint32_t\s*\*\s*\w+", r"uint32_t\s*\*\s*\w+", r"double\s*\*\s*\w+"]), 4),
}
STRUCTS = {"spmvCooOpts": ("duplicates", "keepMap"),
           "spmvCooInfo": ("nEntries", "skipped", "nnzC", "duplicates", "maxRun", "maxRowNnz", "tempBytes", "ms")}


def test_header_declares_the_entry_points_the_constants_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body, struct
        names = [n for decl in body.group(1).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == list(fields), (struct, names)
    for name, value in (("SPMV_COO_SKIP", "0xFFFFFFFFu"), ("SPMV_COO_SUM", "0"), ("SPMV_COO_LAST", "1")):
        assert re.search(r"^\s*#define\s+" + name + r"\s+" + value + r"\b", code, re.M), name


def test_library_exports_them():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_them_with_the_c_layout(tmp_path):
    from spmv_openmp_cuda_amd import api
    for name, (_, nargs) in DECLS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == nargs, name
    assert callable(api.assemble_coo)
    for m in ("assemble_refresh", "assemble_info", "to_coo"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert (api.SPMV_COO_SKIP, api.SPMV_COO_SUM, api.SPMV_COO_LAST) == (cr.SKIP, cr.SUM, cr.LAST)
    assert api.COO_DUPLICATES == cr.MODES
    body = ""
    for struct, fields in STRUCTS.items():
        assert [f[0] for f in getattr(api, struct)._fields_] == list(fields)
        body += f'    printf("{struct} %zu", sizeof({struct}));\n'
        body += "".join(f'    printf(" %zu", offsetof({struct}, {f}));\n' for f in fields) + '    printf("\\n");\n'
    body += '    printf("skip %lu\\n", (unsigned long)SPMV_COO_SKIP);\n'
    lines = run_c(tmp_path, body, "coo_layout").splitlines()
    layout = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in lines}
    for struct, fields in STRUCTS.items():
        py = getattr(api, struct)
        assert layout[struct] == [C.sizeof(py)] + [getattr(py, f).offset for f in fields], struct
    assert layout["skip"] == [cr.SKIP]


# ------------------------------------------------------------------------------------------------------ the reference
ORDER_RUN = [1e16, 1.0, -1e16, 1.0]


def _one_run(vals, mode="sum"):
    n = len(vals)
    C, info, _ = cr.assemble_ref(1, 1, np.zeros(n, np.int64), np.zeros(n, np.int64), np.array(vals), mode)
    assert info["nnzC"] == 1 and info["maxRun"] == n and info["duplicates"] == n - 1
    return np.float64(C[4][0])


def test_the_reference_tells_the_orders_of_a_run_apart():
    """[1e16, 1, -1e16, 1] in input order is ((1e16 + 1) - 1e16) + 1 = 1; other orders give 0 or 2"""
    sums = {p: _one_run([ORDER_RUN[k] for k in p]) for p in itertools.permutations(range(4))}
    assert sums[(0, 1, 2, 3)] == 1.0
    assert sums[(0, 2, 1, 3)] == 2.0 and sums[(0, 1, 3, 2)] == 0.0
    assert len({float(v) for v in sums.values()}) >= 3
    bits = {np.float64(v).view(np.uint64) for v in sums.values()}
    assert len(bits) >= 3, "the permutations give different bits"
    assert _one_run(ORDER_RUN, "last") == 1.0 and _one_run(ORDER_RUN[:3], "last") == -1e16


def test_order_values_show_the_order_of_long_runs():
    """the values the GPU tests draw: reversing a run of 3 or more changes the bits in most draws"""
    rng = np.random.default_rng(3600)
    differ = 0
    for n in (3, 5, 63, 64, 65, 1025):
        for _ in range(8):
            v = si.order_values(rng, n)
            differ += _one_run(v).view(np.uint64) != _one_run(v[::-1]).view(np.uint64)
    print("reversed runs that differ:", differ, "of 48")
    assert differ >= 24


def test_the_reference_agrees_with_assemble_where_nothing_repeats():
    rng = np.random.default_rng(3601)
    for M, N in ((1, 1), (40, 90), (90, 40), (257, 300)):
        A = sr.distinct_csr(rng, M, N, rng.integers(0, min(N, 9) + 1, M), lambda r, n: si.order_values(r, n))
        rows = si.row_of_entry(A[2])
        o = si.stable_rows_by(A[2], A[3].astype(np.int64))                # the entries in (row, col) order
        IRP, JA, AS = si.assemble(M, rows[o], A[3][o].astype(np.int64), A[4][o])
        shuffle = rng.permutation(rows.size)
        for mode in ("sum", "last"):
            C, info, _ = cr.assemble_ref(M, N, rows[shuffle], A[3][shuffle], A[4][shuffle], mode)
            cr.same_bits(C, (M, N, IRP, JA, AS), f"{M}x{N} {mode}")
            assert info["duplicates"] == 0 and info["maxRun"] == (1 if rows.size else 0) and info["skipped"] == 0
            assert np.all(np.diff(JA.astype(np.int64))[np.diff(rows[o]) == 0] > 0), "rows ascend strictly"


def test_skips_singles_and_special_values():
    nan = np.uint64(0x7FF8000000000123).view(np.float64)
    rows = np.array([2, -1, 0, 2, 0, 1, 2, 2], dtype=np.int64)
    cols = np.array([1, 0, 3, -1, 3, 0, 1, 0], dtype=np.int64)
    vals = np.array([np.inf, nan, -0.0, nan, 0.0, nan, -np.inf, -0.0])
    C, info, runs = cr.assemble_ref(3, 4, rows, cols, vals)
    assert info == dict(nEntries=8, skipped=2, nnzC=4, duplicates=2, maxRun=2, maxRowNnz=2)
    assert C[2].tolist() == [0, 1, 2, 4] and C[3].tolist() == [3, 0, 0, 1]
    want = np.array([0.0, nan, -0.0, np.nan])
    cr.same_bits(C, C[:4] + (want,), "special", nan_sums=cr.nan_sums_of(C, runs))
    assert cr.nan_sums_of(C, runs).tolist() == [3], "Inf + -Inf"
    assert C[4][1].view(np.uint64) == np.uint64(0x7FF8000000000123), "a single NaN keeps its payload"
    assert np.signbit(C[4][2]) and not np.signbit(C[4][0]), "-0.0 alone stays; -0.0 + 0.0 is +0.0"
    L, _, _ = cr.assemble_ref(3, 4, rows, cols, vals, "last")
    assert L[4][0].view(np.uint64) == np.float64(0.0).view(np.uint64) and L[4][3] == -np.inf
    U, _, _ = cr.assemble_ref(3, 4, rows.astype(np.uint32), cols.astype(np.uint32), vals)      # 2^32 - 1 is the marker itself
    cr.same_bits(U, C, "uint32 markers", nan_sums=np.array([3]))
    with pytest.raises(IndexError, match="^5$"):
        cr.assemble_ref(3, 4, np.array([0, -1, 2, 2, 1, 3, 9]), np.array([0, 7, 3, -1, 2, 0, 0]), np.zeros(7))
    with pytest.raises(IndexError, match="^2$"):
        cr.assemble_ref(3, 4, np.array([0, 1, 2, 3]), np.array([0, 1, 4, 0]), np.zeros(4))


def test_refresh_over_the_builds_runs_is_a_fresh_assembly_and_to_coo_round_trips():
    rng = np.random.default_rng(3602)
    n = 4000
    rows, cols = rng.integers(-1, 50, n), rng.integers(-1, 60, n)
    vals, new = si.order_values(rng, n), si.order_values(rng, n)
    for mode in ("sum", "last"):
        C, info, runs = cr.assemble_ref(50, 60, rows, cols, vals, mode)
        assert info["skipped"] > 0 and info["duplicates"] > 0 and info["maxRun"] >= 3
        fresh, _, _ = cr.assemble_ref(50, 60, rows, cols, new, mode)
        cr.same_bits(cr.refresh_ref(C, runs, new, mode), fresh, f"refresh {mode}")
        poisoned = np.where((rows == -1) | (cols == -1), np.nan, new)
        cr.same_bits(cr.refresh_ref(C, runs, poisoned, mode), fresh, f"a skipped place is not read ({mode})")
        back, binfo, _ = cr.assemble_ref(50, 60, *cr.to_coo_ref(C), mode)
        cr.same_bits(back, C, f"assemble o to_coo ({mode})")
        assert binfo["duplicates"] == 0 and binfo["nnzC"] == info["nnzC"]
