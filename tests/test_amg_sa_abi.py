"""The smoothed-aggregation entry points are declared, exported and bound in Python with the C layout of their struct, and
the test side's reference (tests/amg_sa_ref.py) has the properties the header states: w_0 = 2/3 as bits on the 7-point
Laplacian, P and the coarse operator equal to the dense T - w D^-1 A T and P^T A P up to rounding order, a fixed omegaP is
used on every level, the smoothed cycle takes fewer CG iterations than the plain hierarchy's, and the plain hierarchy's
gather planted in place of P e changes the bits.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import amg_ref as ar
import amg_sa_ref as sa
import spgemm_ref as sr
from c_header import HEADER, code as _code
from conftest import ROOT
from krylov_ref import CONVERGED, Csr, cg_ref

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H = r"spmat\s*\*\s*\w+"
DECLS = {
    "spmvHipAmgSetupSmoothed": (H + r"\s*,\s*const\s+spmvAmgOpts\s*\*\s*\w+\s*,\s*const\s+spmvAmgSmoothOpts\s*\*\s*\w+\s*,\s*" + H +
                                r"\s*,\s*spmvAmgInfo\s*\*\s*\w+", 5),
    "spmvHipAmgProlongator": (H + r"\s*,\s*unsigned\s+\w+\s*,\s*" + H + r"\s*,\s*" + H + r"\s*,\s*double\s*\*\s*\w+", 5),
}
STRUCTS = {"spmvAmgSmoothOpts": ("omegaP",)}
KRYLOV_OPTS, KRYLOV_TOL = dict(coarseRows=8), 1e-8
# (shape) -> CG iterations of the reference loop: no preconditioner, the plain hierarchy, the smoothed one, omegaP = 0.5
COUNTS = {(12, 10, 8): (48, 18, 13, 14), (24, 20, 16): (89, 27, 16, 19)}


def test_header_declares_the_entry_points_and_the_struct():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body, struct
        names = [n for decl in body.group(1).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == list(fields), (struct, names)


def test_library_exports_them():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_them():
    import inspect
    from spmv_openmp_cuda_amd import api
    for name, (_, nargs) in DECLS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == nargs, name
    assert callable(api.AmgHierarchy.prolongator)
    params = inspect.signature(api.DeviceMatrix.amg).parameters
    assert params["smoothed"].default is False and params["omegaP"].default is None
    for struct, fields in STRUCTS.items():
        assert [f[0] for f in getattr(api, struct)._fields_] == list(fields)


def test_default_damping_on_the_laplacian_is_two_thirds_as_bits():
    A = sr.laplacian7(5, 4, 3)
    rho, g = sa.rho_of(A, ar.dinv_of(A))
    assert rho == 2.0, "an interior row: (1/6) * 12"
    w = sa.damping(rho)
    assert np.float64(w).view(np.uint64) == np.float64(2.0 / 3.0).view(np.uint64)
    levels, _ = sa.setup_ref(A, coarseRows=4, maxLevels=2)
    assert np.float64(levels[0]["w"]).view(np.uint64) == np.float64(2.0 / 3.0).view(np.uint64)


def test_row_sums_are_taken_in_stored_order():
    """three values whose sum depends on the order: (1 + 2^-53) + 2^-53 = 1, (2^-53 + 2^-53) + 1 = 1 + 2^-52"""
    t = 2.0 ** -53
    for vals, want in (([1.0, -t, t], 1.0), ([t, -t, 1.0], 1.0 + 2.0 ** -52)):
        A = (1, 3, np.array([0, 3], np.uint64), np.array([0, 1, 2], np.uint64), np.array(vals))
        rho, g = sa.rho_of(A, np.array([-1.0]))
        assert rho == g[0] == want


@pytest.mark.parametrize("omegaP", [0.0, 0.5])
def test_prolongator_and_coarse_operator_against_the_dense_forms(omegaP):
    A = sa.with_one_diagonal(*ar.small_graphs()["laplacian12x10x8"], seed=3)
    levels, _ = sa.setup_ref(A, omegaP, coarseRows=8)
    assert len(levels) >= 3
    for l, lv in enumerate(levels[:-1]):
        if omegaP:
            assert lv["w"] == 0.5, "a fixed omegaP is used on every level"
        else:
            assert lv["w"] == (4.0 / 3.0) / lv["rho"]
        Ad, T = sr.dense(lv["A"]), sr.dense(lv["T"])
        P = T - lv["w"] * (np.diag(lv["dinv"]) @ Ad @ T)
        assert np.allclose(sr.dense(lv["P"]), P, rtol=1e-13, atol=1e-13), l
        assert np.allclose(sr.dense(lv["R"]), P.T, rtol=1e-13, atol=1e-13), l
        assert np.allclose(sr.dense(levels[l + 1]["A"]), P.T @ Ad @ P, rtol=1e-12, atol=1e-12), l
        assert np.all(np.diff(lv["P"][3].astype(np.int64))[np.diff(sr.si.row_of_entry(lv["P"][2])) == 0] > 0), "P's rows ascend strictly"


def krylov_problem(shape):
    A = sr.laplacian7(*shape)
    return A, np.random.default_rng(24).standard_normal(A[0])


@pytest.mark.parametrize("shape", list(COUNTS))
def test_reference_cg_takes_fewer_iterations_with_the_smoothed_cycle(shape):
    """the condition the GPU test relies on; the counts are those of DESIGN.md section 28"""
    A, b = krylov_problem(shape)
    x0 = np.zeros(A[0])
    none = cg_ref(Csr(A[0], A[2], A[3], A[4]), b, x0, KRYLOV_TOL, 500)
    plain = cg_ref(ar.AmgCsr(A, **KRYLOV_OPTS), b, x0, KRYLOV_TOL, 500)
    smooth = cg_ref(sa.SaCsr(A, **KRYLOV_OPTS), b, x0, KRYLOV_TOL, 500)
    half = cg_ref(sa.SaCsr(A, 0.5, **KRYLOV_OPTS), b, x0, KRYLOV_TOL, 500)
    got = (none[2], plain[2], smooth[2], half[2])
    print("CG iterations (none, plain hierarchy, smoothed, omegaP = 0.5):", got)
    assert none[1] == plain[1] == smooth[1] == half[1] == CONVERGED
    assert got == COUNTS[shape]
    assert smooth[2] < plain[2] < none[2] and half[2] < plain[2]


def test_levels_and_complexity_of_the_smoothed_hierarchy():
    for shape, rows, plain, smooth in (((12, 10, 8), [960, 102, 5], 1.17, 1.35), ((24, 20, 16), [7680, 735, 17, 1], 1.18, 1.39)):
        A = sr.laplacian7(*shape)
        levels, _ = sa.setup_ref(A, **KRYLOV_OPTS)
        assert [lv["A"][0] for lv in levels] == rows
        assert round(sa.complexity(levels), 2) == smooth and round(sa.complexity(ar.setup_ref(A, **KRYLOV_OPTS)[0]), 2) == plain
        assert max(int(np.diff(lv["P"][2].astype(np.int64)).max()) for lv in levels[:-1]) <= 8, "every P fits the fused correction"


def test_the_planted_gather_changes_the_bits():
    A = sr.laplacian7(12, 10, 8)
    levels, o = sa.setup_ref(A, **KRYLOV_OPTS)
    r = np.random.default_rng(25).standard_normal(A[0])
    good, planted = sa.cycle_ref(levels, o, r), sa.cycle_ref(levels, o, r, gather=True)
    assert np.all(np.isfinite(good)) and not np.array_equal(good.view(np.uint64), planted.view(np.uint64))


def test_one_level_is_the_plain_cycle():
    A = sr.laplacian7(4, 3, 2)
    r = np.random.default_rng(26).standard_normal(A[0])
    ls, os_ = sa.setup_ref(A, maxLevels=1)
    lp, op = ar.setup_ref(A, maxLevels=1)
    assert len(ls) == 1 and np.array_equal(sa.cycle_ref(ls, os_, r).view(np.uint64), ar.cycle_ref(lp, op, r).view(np.uint64))


def test_with_one_diagonal_keeps_the_mess_and_meets_the_stored_rule():
    M, IRP, JA = ar.messy(40)
    A = sa.with_one_diagonal(M, IRP, JA, seed=1)
    rows = sr.si.row_of_entry(A[2])
    assert np.array_equal(np.bincount(rows[A[3].astype(np.int64) == rows], minlength=M), np.ones(M, dtype=np.int64))
    assert np.any(np.diff(A[2].astype(np.int64)) == 1), "an isolated vertex keeps its diagonal alone"
    inner = rows[1:] == rows[:-1]
    assert np.any(inner & (np.diff(A[3].astype(np.int64)) < 0)) and np.any(inner & (np.diff(A[3].astype(np.int64)) == 0))
