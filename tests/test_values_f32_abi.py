"""The single-precision value storage (spmvHipValuesF32, ...Info, the four f32 products, spmvHipFsaiSetStorage / ...Storage) is
declared, exported and bound in Python with the C layout of spmvF32Info; the reference rounding (tests/values_f32_ref.py)
agrees with its plain-Python restatement on the boundary set; and the inputs of the GPU tests tell the two storages apart.
No GPU needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fsai_ref as fr
import serial_order_inputs as si
import values_f32_ref as vr
from bits import assert_same_bits, differing_rows
from c_header import HEADER, code as _code, prototypes, run_c, structs
from conftest import ROOT
from krylov_ref import cg_ref
from spgemm_ref import laplacian7
from test_fsai_abi import random_spd, stencil

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
PROTOS = {"spmvHipValuesF32": 2, "spmvHipValuesF32Info": 2, "hipSpMVRowsCSRf32": 4, "hipSpMVWarpPerRowCSRf32": 4,
          "spmvHipEnqueueRowsF32": 4, "hipSpMMRowsCSRf32": 8, "spmvHipFsaiSetStorage": 2, "spmvHipFsaiStorage": 2,
          "spmvHipAmgSetStorage": 3, "spmvHipAmgStorage": 2}
AMG_FIELDS = ["storage", "levels", "f32Bytes"]
INFO_FIELDS = ["built", "unit", "bytes", "refreshes", "inexact", "overflowed", "flushed", "firstOverflow"]


def test_header_declares_the_entry_points_and_the_struct():
    protos = prototypes()
    for name, n in PROTOS.items():
        assert protos.get(name) == n, name
    assert structs()["spmvF32Info"] == INFO_FIELDS
    assert re.search(r"typedef\s+struct\s*\{\s*int\s+storage\s*;\s*unsigned\s+levels\s*;\s*ulong\s+f32Bytes\s*;\s*\}\s*spmvAmgStorageInfo\s*;", _code(HEADER))
    code = _code(HEADER)
    assert re.search(r"^\s*#\s*define\s+SPMV_STORAGE_F64\s+0\b", code, re.M) and re.search(r"^\s*#\s*define\s+SPMV_STORAGE_F32\s+1\b", code, re.M)
    # the twins have their twins' parameter lists
    assert protos["hipSpMVRowsCSRf32"] == protos["hipSpMVRowsCSR"] and protos["hipSpMVWarpPerRowCSRf32"] == protos["hipSpMVWarpPerRowCSR"]
    assert protos["hipSpMMRowsCSRf32"] == protos["hipSpMMRowsCSR"]


def test_library_exports_them():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in PROTOS:
        assert name in syms, name


def test_python_binds_them_with_the_c_layout(tmp_path):
    import ctypes as C

    from spmv_openmp_cuda_amd import api
    for name, n in PROTOS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == n, name
    for name in ("hipSpMVRowsCSRf32", "hipSpMVWarpPerRowCSRf32"):
        assert api.SPMV_LAUNCHERS[name] is not None and api.SPMV_LAUNCHERS[name].argtypes == api.SPMV_LAUNCHERS["hipSpMVRowsCSR"].argtypes
    for m in ("values_f32", "values_f32_info"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert callable(api.Fsai.set_storage) and isinstance(api.Fsai.storage, property)
    assert (api.SPMV_STORAGE_F64, api.SPMV_STORAGE_F32) == (0, 1) and api.STORAGES == {"f64": 0, "f32": 1}
    assert [f[0] for f in api.spmvF32Info._fields_] == INFO_FIELDS
    body = 'printf("%zu", sizeof(spmvF32Info));\n' + "".join(f'printf(" %zu", offsetof(spmvF32Info, {f}));\n' for f in INFO_FIELDS)
    got = [int(v) for v in run_c(tmp_path, body).split()]
    assert got == [C.sizeof(api.spmvF32Info)] + [getattr(api.spmvF32Info, f).offset for f in INFO_FIELDS]
    assert [f[0] for f in api.spmvAmgStorageInfo._fields_] == AMG_FIELDS
    body = 'printf("%zu", sizeof(spmvAmgStorageInfo));\n' + "".join(f'printf(" %zu", offsetof(spmvAmgStorageInfo, {f}));\n' for f in AMG_FIELDS)
    got = [int(v) for v in run_c(tmp_path, body, "amg").split()]
    assert got == [C.sizeof(api.spmvAmgStorageInfo)] + [getattr(api.spmvAmgStorageInfo, f).offset for f in AMG_FIELDS]
    for m in ("set_storage", "storage_info"):
        assert callable(getattr(api.AmgHierarchy, m)), m


# ------------------------------------------------------------------------------------------------------ the rounding
def test_the_reference_rounding_on_the_boundary_set():
    vals = vr.boundary_values()
    got = vr.round32(vals)
    n = len(vr.BOUNDARY_EXPECT)
    want = np.array(vr.BOUNDARY_EXPECT + [-v for v in vr.BOUNDARY_EXPECT])
    plain = np.array([vr.round32_plain(float(v)) for v in vals])
    for i, v in enumerate(vals):
        if math.isnan(want[i]):
            assert math.isnan(got[i]) and math.isnan(plain[i]), v
        else:                                                        # by bits: the sign of a zero is part of the contract
            assert_same_bits(got[i:i + 1], want[i:i + 1], f"numpy on {v!r}")
            assert_same_bits(plain[i:i + 1], want[i:i + 1], f"plain Python on {v!r}")
    assert np.signbit(got[n + vr.BOUNDARY_EXPECT.index(0.0)]), "-0.0 stays -0.0"
    assert np.signbit(vr.round32(np.array([-2.0 ** -150]))[0]), "a negative value flushed to zero keeps its sign"


def test_the_two_roundings_agree_on_ordinary_and_subnormal_values():
    rng = np.random.default_rng(4150)
    vals = np.concatenate([si.order_values(rng, 500, 12), rng.uniform(-1, 1, 300) * 2.0 ** rng.integers(-155, -120, 300),
                           rng.uniform(-1, 1, 100) * 2.0 ** rng.integers(120, 130, 100)])
    vr.same(np.array([vr.round32_plain(float(v)) for v in vals]), vr.round32(vals), "plain Python against numpy")


def test_the_counts_of_the_boundary_case():
    """of the 24 values: exact are +-0, +-1, +-2^-149, +-FLT_MAX, +-Inf; NaN is not counted; the other 2 x 6 are inexact, of
    which +-OVERFLOW overflow and +-2^-150 flush"""
    assert vr.counts(vr.boundary_values()) == (12, 2, 2, 9)
    assert vr.counts(np.array([1.0, 0.5, -3.0])) == (0, 0, 0, -1)


# ------------------------------------------------------------------------------------------- what the inputs tell apart
@pytest.mark.parametrize("name", vr.ORDINARY + ("boundary",))
def test_the_product_inputs_tell_the_storages_apart(oracle, name):
    M, N, IRP, JA, AS, x = vr.case(name)
    y64, y32 = oracle.csr_serial(IRP, JA, AS, x), oracle.csr_serial(IRP, JA, vr.round32(AS), x)
    both = np.isfinite(y64) & np.isfinite(y32)
    assert differing_rows(y32[both], y64[both]).size > 0, "the two storages give other bits somewhere"
    if name == "boundary":
        assert np.isnan(y32).sum() > np.isnan(y64).sum(), "a value flushed to zero times Inf is a NaN only from single precision"
        return
    perm = si.reversed_rows(IRP)                                      # ... and the inputs are order-sensitive
    assert differing_rows(oracle.csr_serial(IRP, JA[perm], vr.round32(AS)[perm], x), y32).size > 0


def test_the_unit_inputs(oracle):
    M, N, IRP, JA, AS, x = vr.unit_case(0.1)
    assert vr.round32(np.array([0.1]))[0] != 0.1 and vr.round32(np.array([1.0]))[0] == 1.0
    assert differing_rows(oracle.csr_serial(IRP, JA, vr.round32(AS), x), oracle.csr_serial(IRP, JA, AS, x)).size > 0


def _fsai_cases():
    L = laplacian7(10, 9, 8)
    return {"laplacian-10x9x8": ((L[0], L[1], L[2], L[3], L[4]), 27),
            "stencil-9x8x7": (stencil(np.random.default_rng(3820), 9, 8, 7), 10),
            "random-spd-300": (random_spd(np.random.default_rng(3803), 300, 4), 10)}


@pytest.mark.parametrize("name", ["laplacian-10x9x8", "stencil-9x8x7", "random-spd-300"])
def test_cg_with_the_rounded_factor_other_bits_the_same_count(name):
    """the counts are pinned: computed on the CPU from the references alone"""
    A, iters = _fsai_cases()[name]
    G, _ = fr.fsai_vec(A)
    Gt = vr.rounded(G)
    assert np.all(Gt[4] != G[4]), "every value of the factor is inexact in single precision"
    b = np.random.default_rng(3821).standard_normal(A[0])
    w64 = cg_ref(fr.PrecondCsr(A, G), b, np.zeros(A[0]), 1e-10, 500)
    w32 = cg_ref(fr.PrecondCsr(A, Gt), b, np.zeros(A[0]), 1e-10, 500)
    assert (w64[1], w64[2]) == (0, iters) and (w32[1], w32[2]) == (0, iters)
    assert differing_rows(w32[0], w64[0]).size > 0


@pytest.mark.parametrize("config", list(vr.AMG_CONFIGS))
def test_the_cycle_on_rounded_levels_differs_by_bits(config):
    """amg_ref's cycle (through amg_cheb_ref.cycle_ref, which is it with a smoother) on levels whose A_l, R and P are rounded
    and whose dinv and tables are the doubles': other bits than the f64 cycle, the same operator to single precision"""
    import amg_cheb_ref as cr
    levels, rounded, o, sm = vr.amg_reference(config)
    assert len(levels) >= 3
    for lv, rv in zip(levels, rounded):
        assert rv["dinv"] is lv["dinv"] and rv["A"] is lv["A"]
        assert np.all(rv["csr"].AS != lv["csr"].AS), "every value of A_l is inexact in single precision"
    r = si.order_values(np.random.default_rng(4510), levels[0]["A"][0], 1)
    z64, z32 = cr.cycle_ref(levels, o, r, sm), cr.cycle_ref(rounded, o, r, sm)
    assert differing_rows(z32, z64).size > z64.size // 2
    assert np.allclose(z32, z64, rtol=0, atol=1e-5 * np.abs(z64).max())
