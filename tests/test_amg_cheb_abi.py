"""The Chebyshev-smoother entry points are declared, exported and bound in Python with the C layout of their structs, and the
test side's reference (tests/amg_cheb_ref.py) has the properties the header states: the interval and b_0 on the 7-point
Laplacian as bits, degree 1 equal to damped Jacobi with omega = b_0 (from nothing and from z), three planted faults -- a
fused multiply-add in the step, a post-smoother that continues the recurrence, rho from the strength-filtered matrix -- each
changing the bits, and the CG counts of DESIGN.md section 30.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import amg_cheb_ref as cr
import amg_ref as ar
import amg_sa_ref as sa
import filter_ref as fr
import spgemm_ref as sr
from c_header import HEADER, code as _code
from conftest import ROOT
from krylov_ref import CONVERGED, cg_ref

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H = r"spmat\s*\*\s*\w+"
DECLS = {
    "spmvHipAmgSetSmoother": (H + r"\s*,\s*" + H + r"\s*,\s*const\s+spmvAmgSmootherOpts\s*\*\s*\w+", 3),
    "spmvHipAmgSmoother": (H + r"\s*,\s*unsigned\s+\w+\s*,\s*spmvAmgSmootherInfo\s*\*\s*\w+", 3),
}
STRUCTS = {"spmvAmgSmootherOpts": ("kind", "nu1", "nu2", "nuCoarse", "eigRatio", "lambdaScale"),
           "spmvAmgSmootherInfo": ("kind", "nu1", "nu2", "nuCoarse", "rho", "lambdaMax", "lambdaMin", "nCoef", "dCoef")}
DEFINES = {"SPMV_AMG_SMOOTHER_JACOBI": 0, "SPMV_AMG_SMOOTHER_CHEBYSHEV": 1, "SPMV_AMG_MAX_DEGREE": 64}
KRYLOV_OPTS, KRYLOV_TOL = dict(coarseRows=8), 1e-8
SHAPES = ((12, 10, 8), (24, 20, 16))
HIERARCHIES = ("plain", "smoothed")
DEGREES = (2, 3)
RATIOS = (4.0, 10.0, 30.0)
# (shape, hierarchy, nu1 = nu2) -> CG iterations of the reference loop: Jacobi, then Chebyshev at eigRatio 4, 10, 30
COUNTS = {
    ((12, 10, 8), "plain", 2): (13, 11, 11, 13),    ((12, 10, 8), "plain", 3): (11, 9, 8, 9),
    ((12, 10, 8), "smoothed", 2): (9, 7, 8, 13),    ((12, 10, 8), "smoothed", 3): (8, 7, 6, 9),
    ((24, 20, 16), "plain", 2): (20, 17, 16, 17),   ((24, 20, 16), "plain", 3): (17, 15, 13, 12),
    ((24, 20, 16), "smoothed", 2): (12, 10, 9, 14), ((24, 20, 16), "smoothed", 3): (10, 8, 8, 9),
}


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_header_declares_the_entry_points_the_kinds_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for name, value in DEFINES.items():
        assert re.search(r"^\s*#define\s+" + name + r"\s+" + str(value) + r"\s*$", code, re.M), name
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
    for struct, fields in STRUCTS.items():
        assert [f[0] for f in getattr(api, struct)._fields_] == list(fields)
    for name, value in DEFINES.items():
        assert getattr(api, name) == value == getattr(cr, name.replace("SPMV_AMG_SMOOTHER_", "").replace("SPMV_AMG_", ""))
    params = inspect.signature(api.AmgHierarchy.set_smoother).parameters
    assert list(params) == ["self", "kind", "nu1", "nu2", "nuCoarse", "eig_ratio", "lambda_scale"]
    assert params["kind"].default == "chebyshev" and all(params[k].default is None for k in list(params)[2:])
    assert callable(api.AmgHierarchy.smoother)
    amg = inspect.signature(api.DeviceMatrix.amg).parameters
    assert list(amg) == ["self", "seed", "coarseRows", "maxLevels", "omega", "nu1", "nu2", "nuCoarse", "smoothed", "omegaP", "theta", "thetaScale"]


# ------------------------------------------------------------------------------------------------------- coefficients
def test_the_interval_and_b0_on_the_laplacian_as_bits():
    A = sr.laplacian7(5, 4, 3)
    rho = cr.level_rho(dict(A=A, dinv=ar.dinv_of(A)))
    assert _bits(rho) == _bits(2.0), "an interior row: (1/6) * 12"
    lmax, lmin, ab = cr.coefficients(rho, 4.0, 1.0, 3)
    assert _bits(lmax) == _bits(2.0) and _bits(lmin) == _bits(0.5)
    theta, delta = (lmax + lmin) / np.float64(2.0), (lmax - lmin) / np.float64(2.0)
    assert _bits(theta) == _bits(1.25) and _bits(delta) == _bits(0.75)
    assert _bits(ab[0, 0]) == _bits(0.0) and _bits(ab[0, 1]) == _bits(1.0 / 1.25)
    # the recurrence by hand, every operation on its own
    sigma = np.float64(1.25) / np.float64(0.75)
    s0 = np.float64(1.0) / sigma
    s1 = np.float64(1.0) / (np.float64(2.0) * sigma - s0)
    s2 = np.float64(1.0) / (np.float64(2.0) * sigma - s1)
    want = [(0.0, 0.8), (s1 * s0, (np.float64(2.0) * s1) / np.float64(0.75)), (s2 * s1, (np.float64(2.0) * s2) / np.float64(0.75))]
    assert np.array_equal(_bits(ab), _bits(np.array(want)))
    assert cr.coefficients(rho, 4.0, 1.0, 0)[2].shape == (0, 2)
    assert np.array_equal(_bits(cr.coefficients(rho, 4.0, 1.0, 2)[2]), _bits(ab[:2])), "a shorter table is a prefix"
    assert _bits(cr.coefficients(rho, 10.0, 1.5, 1)[0]) == _bits(3.0), "lambdaScale scales lambda_max"


def test_the_table_of_a_level_runs_to_its_largest_degree():
    A = sr.laplacian7(12, 10, 8)
    levels, o = ar.setup_ref(A, **KRYLOV_OPTS)
    sm = cr.smoother(o, nu1=2, nu2=3, nuCoarse=5)
    tabs = cr.tables(levels, sm)
    assert len(levels) >= 3 and [t["ab"].shape[0] for t in tabs] == [3] * (len(levels) - 1) + [5]
    assert all(0.0 < t["lmin"] < t["lmax"] == t["rho"] for t in tabs)
    assert cr.smoother(o)["nu1"] == o["nu1"] and cr.smoother(o)["nuCoarse"] == o["nuCoarse"] == 8, "None keeps the hierarchy's"


def test_degree_one_is_jacobi_with_omega_b0():
    """one level, so that one omega serves; then two levels with no coarse sweeps: the correction adds +0.0 and the
    post-smoother's first step from z is one Jacobi sweep"""
    A = sa.with_one_diagonal(*ar.small_graphs()["laplacian12x10x8"], seed=4)
    r = np.random.default_rng(60).standard_normal(A[0])
    for eig in (4.0, 10.0):
        levels, o = ar.setup_ref(A, maxLevels=1)
        tabs = cr.tables(levels, cr.smoother(o, nuCoarse=1, eigRatio=eig))
        b0 = tabs[0]["ab"][0, 1]
        got = cr.cycle_ref(levels, o, r, cr.smoother(o, nuCoarse=1, eigRatio=eig))
        want = ar.cycle_ref(levels, dict(o, omega=b0, nuCoarse=1), r)
        assert np.array_equal(_bits(got), _bits(want))
        levels, o = ar.setup_ref(A, coarseRows=8, maxLevels=2)
        assert len(levels) == 2
        sm = cr.smoother(o, nu1=1, nu2=1, nuCoarse=0, eigRatio=eig)
        b0 = cr.tables(levels, sm)[0]["ab"][0, 1]
        got = cr.cycle_ref(levels, o, r, sm)
        want = ar.cycle_ref(levels, dict(o, omega=b0, nu1=1, nu2=1, nuCoarse=0), r)
        assert np.array_equal(_bits(got), _bits(want))
        # and the step from z alone
        z0 = np.random.default_rng(61).standard_normal(A[0])
        lv = levels[0]
        z1, d1 = cr.cheb(lv["csr"], lv["dinv"], r, z0, np.array([[0.0, b0]]), range(1), False)
        assert np.array_equal(_bits(z1), _bits(z0 + b0 * (lv["dinv"] * (r - lv["csr"].spmv(z0)))))


def test_the_jacobi_kind_is_the_cycle_of_the_setups():
    A = sr.laplacian7(12, 10, 8)
    r = np.random.default_rng(62).standard_normal(A[0])
    for hierarchy, ref in (("plain", ar.cycle_ref), ("smoothed", sa.cycle_ref)):
        levels, o = cr.setup_ref(A, hierarchy, nu1=2, nu2=1, nuCoarse=3, **KRYLOV_OPTS)
        got = cr.cycle_ref(levels, o, r, cr.smoother(o, kind=cr.JACOBI))
        assert np.array_equal(_bits(got), _bits(ref(levels, o, r)))
        got = cr.cycle_ref(levels, o, r, cr.smoother(o, kind=cr.JACOBI, nu1=1, nu2=3, nuCoarse=0))
        assert np.array_equal(_bits(got), _bits(ref(levels, dict(o, nu1=1, nu2=3, nuCoarse=0), r)))


# ------------------------------------------------------------------------------------------------------ planted faults
def test_the_fused_multiply_add_is_one_rounding():
    a, d, p = np.float64(1.0 + 2.0 ** -30), np.array([1.0 + 2.0 ** -30]), np.array([-1.0])
    assert cr._fma(a, d, p)[0] == 2.0 ** -29 + 2.0 ** -60 and (a * d + p)[0] == 2.0 ** -29


@pytest.mark.parametrize("hierarchy", HIERARCHIES)
def test_a_planted_fma_and_a_continued_recurrence_change_the_bits(hierarchy):
    A = sr.laplacian7(12, 10, 8)
    levels, o = cr.setup_ref(A, hierarchy, **KRYLOV_OPTS)
    r = np.random.default_rng(63).standard_normal(A[0])
    good = cr.cycle_ref(levels, o, r, cr.smoother(o, nu1=3, nu2=2))
    assert np.all(np.isfinite(good))
    for fault in ("fma", "carry_on"):
        planted = cr.cycle_ref(levels, o, r, cr.smoother(o, nu1=3, nu2=2, **{fault: True}))
        assert np.all(np.isfinite(planted)) and not np.array_equal(_bits(good), _bits(planted)), fault
        assert np.allclose(good, planted, rtol=0.5, atol=0.5), "another smoother, not another problem"


def test_rho_from_the_filtered_matrix_changes_the_bits():
    A = fr.stencil7(12, 10, 8, (1.0, 0.01, 0.01))
    levels, o = cr.setup_ref(A, "strength", **KRYLOV_OPTS)
    assert len(levels) >= 3 and all("F" in lv for lv in levels[:-1])
    sm, planted = cr.smoother(o, nu1=2, nu2=2), cr.smoother(o, nu1=2, nu2=2, rho_from_F=True)
    ta, tf = cr.tables(levels, sm), cr.tables(levels, planted)
    assert _bits(ta[0]["rho"]) != _bits(tf[0]["rho"]), "F_0 lumps what it drops: its row sums are not A_0's"
    assert _bits(ta[-1]["rho"]) == _bits(tf[-1]["rho"]), "the last level has no filtered matrix"
    r = np.random.default_rng(64).standard_normal(A[0])
    good, bad = cr.cycle_ref(levels, o, r, sm), cr.cycle_ref(levels, o, r, planted)
    assert np.all(np.isfinite(good)) and not np.array_equal(_bits(good), _bits(bad))


# --------------------------------------------------------------------------------------------------------- the counts
def krylov_problem(shape):
    A = sr.laplacian7(*shape)
    return A, np.random.default_rng(24).standard_normal(A[0])


@pytest.mark.parametrize("hierarchy", HIERARCHIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_cg_counts_jacobi_against_chebyshev(shape, hierarchy):
    """the table of DESIGN.md section 30; at eigRatio = 10 on 24 x 20 x 16 Chebyshev takes strictly fewer iterations than
    Jacobi at the same degree, on both hierarchies"""
    A, b = krylov_problem(shape)
    levels, o = cr.setup_ref(A, hierarchy, **KRYLOV_OPTS)
    x0 = np.zeros(A[0])
    for nu in DEGREES:
        got = []
        for sm in [dict(kind=cr.JACOBI)] + [dict(eigRatio=e) for e in RATIOS]:
            res = cg_ref(cr.ChebCsr(A, levels=levels, o=o, sm=dict(sm, nu1=nu, nu2=nu)), b, x0, KRYLOV_TOL, 500)
            assert res[1] == CONVERGED
            got.append(res[2])
        print(f"CG iterations on {shape}, {hierarchy}, nu1 = nu2 = {nu} (Jacobi, Chebyshev at eigRatio 4, 10, 30):", tuple(got))
        assert tuple(got) == COUNTS[(shape, hierarchy, nu)]
        if shape == (24, 20, 16):
            assert got[2] < got[0], "eigRatio = 10"
