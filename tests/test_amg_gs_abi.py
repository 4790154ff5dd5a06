"""The Gauss-Seidel-smoother entry points are declared, exported and bound in Python with the C layout of their structs, and
the test side's reference (tests/amg_gs_ref.py) has the properties the header states: on a diagonal matrix a sweep is the
Jacobi first sweep, on the red-black Laplacian a forward sweep is a hand-written two-colour loop as bits, four planted faults
-- a fused multiply-add in the row update, a forward post-sweep in the symmetric cycle, colours from the strength-filtered
matrix, a Jacobi within the sweep -- each changing the bits, the symmetric cycle is a symmetric operator and the one-way cycle
is not, and the CG counts of DESIGN.md section 32.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import amg_gs_ref as gr
import amg_ref as ar
import c_header
import filter_ref as fr
import spgemm_ref as sr
from c_header import HEADER, code as _code
from conftest import ROOT
from krylov_ref import CONVERGED, cg_ref

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H = r"spmat\s*\*\s*\w+"
DECLS = {
    "spmvHipAmgSetGaussSeidel": (H + r"\s*,\s*" + H + r"\s*,\s*const\s+spmvAmgGsOpts\s*\*\s*\w+", 3),
    "spmvHipAmgGaussSeidel": (H + r"\s*,\s*unsigned\s+\w+\s*,\s*spmvAmgGsInfo\s*\*\s*\w+", 3),
}
STRUCTS = {"spmvAmgGsOpts": ("order", "seed", "omega", "oneWay", "levels", "nu1", "nu2", "nuCoarse"),
           "spmvAmgGsInfo": ("active", "colours", "maxColourRows", "longRows", "small", "omega", "order", "seed", "oneWay", "dPerm",
                             "dColourPtr")}
KRYLOV_OPTS, KRYLOV_TOL = dict(coarseRows=8), 1e-8
SHAPES = ((12, 10, 8), (24, 20, 16))
HIERARCHIES = ("plain", "smoothed")
SWEEPS = (1, 2)
# (shape, hierarchy, nu1 = nu2) -> CG iterations of the reference loop: (damped Jacobi, symmetric Gauss-Seidel), natural
# order, omega = 1
COUNTS = {
    ((12, 10, 8), "plain", 1): (18, 14),    ((12, 10, 8), "plain", 2): (13, 10),
    ((12, 10, 8), "smoothed", 1): (13, 10), ((12, 10, 8), "smoothed", 2): (9, 7),
    ((24, 20, 16), "plain", 1): (27, 21),   ((24, 20, 16), "plain", 2): (20, 15),
    ((24, 20, 16), "smoothed", 1): (16, 12), ((24, 20, 16), "smoothed", 2): (12, 8),
}
# max|B - B^T| / max|B| of the cycle's matrix B on the 5 x 4 x 3 Laplacian (plain hierarchy, coarseRows = 8, nu1 = nu2 = 1):
# the reference gives 6.6e-17 for the symmetric cycle -- rounding, below one unit of 2^-53 -- and 4.8e-02 for the one-way
# cycle (printed by the test below): a margin of 7e14.  The test asks for that margin less two decades,
# and for each figure within two decades of the reference's own.
MARGIN, SYMMETRIC_BELOW, ONE_WAY_ABOVE = 1e12, 6.6e-15, 4.8e-4


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_header_declares_the_entry_points_the_kind_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    assert re.search(r"^\s*#define\s+SPMV_AMG_SMOOTHER_GAUSS_SEIDEL\s+2\s*$", code, re.M)
    for struct, fields in STRUCTS.items():
        assert c_header.structs()[struct] == list(fields), struct


def test_library_exports_them():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_them_with_the_c_layout(tmp_path):
    import inspect
    from spmv_openmp_cuda_amd import api
    for name, (_, nargs) in DECLS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == nargs, name
    assert api.SPMV_AMG_SMOOTHER_GAUSS_SEIDEL == 2 == gr.GAUSS_SEIDEL
    body = ""
    for name, fields in STRUCTS.items():
        body += f'    printf("{name} %zu", sizeof({name}));\n'
        body += "".join(f'    printf(" %zu", offsetof({name}, {f}));\n' for f in fields) + '    printf("\\n");\n'
    layout = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in c_header.run_c(tmp_path, body, "gs_layout").splitlines()}
    for struct, fields in STRUCTS.items():
        py = getattr(api, struct)
        assert [f[0] for f in py._fields_] == list(fields)
        assert layout[struct] == [C.sizeof(py)] + [getattr(py, f).offset for f in fields], struct
    params = inspect.signature(api.AmgHierarchy.set_gauss_seidel).parameters
    assert list(params) == ["self", "omega", "order", "seed", "one_way", "levels", "nu1", "nu2", "nuCoarse"]
    assert (params["order"].default, params["seed"].default, params["one_way"].default) == ("natural", 0, False)
    assert all(params[k].default is None for k in ("omega", "levels", "nu1", "nu2", "nuCoarse"))
    assert callable(api.AmgHierarchy.gauss_seidel)
    amg = inspect.signature(api.DeviceMatrix.amg).parameters
    assert list(amg) == ["self", "seed", "coarseRows", "maxLevels", "omega", "nu1", "nu2", "nuCoarse", "smoothed", "omegaP", "theta", "thetaScale"]


# ----------------------------------------------------------------------------------------------------------- the sweep
def test_on_a_diagonal_matrix_a_sweep_is_the_jacobi_first_sweep():
    M = 37
    rng = np.random.default_rng(70)
    A = (M, M, np.arange(M + 1, dtype=np.uint64), np.arange(M, dtype=np.uint64), 0.5 + rng.random(M))
    r = rng.standard_normal(M)
    for omega in (1.0, 2.0 / 3.0):
        levels, o = ar.setup_ref(A, maxLevels=1, omega=omega, nuCoarse=1)
        sm = gr.smoother(o, omega=omega)
        cols = gr.colourings(levels, sm)
        assert len(cols[0]["classes"]) == 1, "no edge: one colour"
        got = gr.cycle_ref(levels, o, r, sm)
        assert np.array_equal(_bits(got), _bits(ar.cycle_ref(levels, o, r))), "z = 0 + omega * (dinv * (r - 0))"


def test_a_forward_sweep_on_the_red_black_laplacian_is_the_two_colour_loop():
    nx, ny, nz = 5, 4, 3
    A = sr.laplacian7(nx, ny, nz)
    M, _, IRP, JA, AS = A
    levels, o = ar.setup_ref(A, maxLevels=1, nuCoarse=1)
    sm = gr.smoother(o)
    col = gr.colourings(levels, sm)[0]
    ids = np.arange(M)
    parity = (ids % nz + ids // nz % ny + ids // (ny * nz)) % 2     # (the last axis runs fastest)
    assert np.array_equal(col["colour"], parity.astype(np.uint32)), "natural order: red-black"
    assert np.array_equal(col["ptr"], [0, int((parity == 0).sum()), M])
    r = np.random.default_rng(71).standard_normal(M)
    dinv = levels[0]["dinv"]
    z = np.zeros(M)
    for c in (0, 1):                                           # by hand, a row at a time
        for i in ids[parity == c]:
            t = np.float64(0.0)
            for p in range(int(IRP[i]), int(IRP[i + 1])):
                t = t + AS[p] * z[int(JA[p])]
            z[i] = z[i] + np.float64(1.0) * (dinv[i] * (r[i] - t))
    assert np.array_equal(_bits(gr.cycle_ref(levels, o, r, sm)), _bits(z))
    two = gr.cycle_ref(levels, o, r, gr.smoother(o, nuCoarse=2))
    back = gr.gs(col, dinv, r, z, 1, False, lambda k: True, 1.0)
    assert np.array_equal(_bits(two), _bits(back)), "the last level's second sweep runs backward"
    one_way = gr.cycle_ref(levels, o, r, gr.smoother(o, nuCoarse=2, oneWay=True))
    assert np.array_equal(_bits(one_way), _bits(gr.gs(col, dinv, r, z, 1, False, lambda k: False, 1.0)))
    assert not np.array_equal(_bits(two), _bits(one_way))


def test_the_jacobi_levels_of_a_gauss_seidel_hierarchy_are_the_cycle_of_the_setup():
    A = sr.laplacian7(12, 10, 8)
    r = np.random.default_rng(72).standard_normal(A[0])
    levels, o = gr.setup_ref(A, "plain", nu1=2, nu2=1, nuCoarse=3, **KRYLOV_OPTS)
    assert len(levels) >= 3
    full = gr.cycle_ref(levels, o, r, gr.smoother(o))
    assert np.array_equal(_bits(full), _bits(gr.cycle_ref(levels, o, r, gr.smoother(o, levels=len(levels) + 5))))
    top = gr.cycle_ref(levels, o, r, gr.smoother(o, levels=1))
    assert not np.array_equal(_bits(full), _bits(top)) and not np.array_equal(_bits(top), _bits(ar.cycle_ref(levels, o, r)))
    assert [c is None for c in gr.colourings(levels, gr.smoother(o, levels=1))] == [False] + [True] * (len(levels) - 1)


# ------------------------------------------------------------------------------------------------------ planted faults
def test_the_fused_multiply_add_is_one_rounding():
    a, x, z = np.float64(1.0 + 2.0 ** -30), np.array([1.0 + 2.0 ** -30]), np.array([-1.0])
    assert gr._fma(a, x, z)[0] == 2.0 ** -29 + 2.0 ** -60 and (z + a * x)[0] == 2.0 ** -29


@pytest.mark.parametrize("hierarchy", HIERARCHIES)
def test_every_planted_fault_changes_the_bits(hierarchy):
    A = sr.laplacian7(12, 10, 8)
    levels, o = gr.setup_ref(A, hierarchy, **KRYLOV_OPTS)
    r = np.random.default_rng(73).standard_normal(A[0])
    kw = dict(omega=0.9, nu1=2, nu2=2)                          # (omega = 1 makes the update's product exact: an FMA would not show)
    good = gr.cycle_ref(levels, o, r, gr.smoother(o, **kw))
    assert np.all(np.isfinite(good))
    for fault in ("fma", "post_forward", "jacobi_within"):
        planted = gr.cycle_ref(levels, o, r, gr.smoother(o, **kw, **{fault: True}))
        assert np.all(np.isfinite(planted)) and not np.array_equal(_bits(good), _bits(planted)), fault
        assert np.allclose(good, planted, rtol=0.5, atol=0.5), "another smoother, not another problem"


def test_colours_from_the_filtered_matrix_change_the_bits():
    A = fr.stencil7(12, 10, 8, (1.0, 0.01, 0.01))
    levels, o = gr.setup_ref(A, "strength", **KRYLOV_OPTS)
    assert len(levels) >= 3 and all("F" in lv for lv in levels[:-1])
    sm, planted = gr.smoother(o), gr.smoother(o, colours_from_F=True)
    ca, cf = gr.colourings(levels, sm), gr.colourings(levels, planted)
    assert any(not np.array_equal(a["colour"], f["colour"]) for a, f in zip(ca, cf)), "F_l drops edges: other colours"
    assert not all(cl_is_proper(lv, f["colour"]) for lv, f in zip(levels, cf)), "which are no colouring of A_l"
    assert all(cl_is_proper(lv, a["colour"]) for lv, a in zip(levels, ca))
    r = np.random.default_rng(74).standard_normal(A[0])
    good, bad = gr.cycle_ref(levels, o, r, sm), gr.cycle_ref(levels, o, r, planted)
    assert np.all(np.isfinite(good)) and not np.array_equal(_bits(good), _bits(bad))


def cl_is_proper(lv, colour):
    A = lv["A"]
    return gr.cl.is_proper(A[0], A[2], A[3], colour)


# ------------------------------------------------------------------------------------------------------------ symmetry
def _cycle_matrix(levels, o, sm):
    M = levels[0]["A"][0]
    cols = gr.colourings(levels, sm)
    return np.stack([gr.cycle_ref(levels, o, e, sm, cols=cols) for e in np.eye(M)], axis=1)


def test_the_symmetric_cycle_is_symmetric_and_the_one_way_cycle_is_not():
    A = sr.laplacian7(5, 4, 3)
    levels, o = gr.setup_ref(A, "plain", **KRYLOV_OPTS)
    assert len(levels) >= 2
    asym = {}
    for name, kw in (("symmetric", dict()), ("one-way", dict(oneWay=True)), ("forward post-sweep", dict(post_forward=True))):
        B = _cycle_matrix(levels, o, gr.smoother(o, nu1=1, nu2=1, **kw))
        asym[name] = float(np.max(np.abs(B - B.T)) / np.max(np.abs(B)))
        print(f"max|B - B^T| / max|B| of the {name} cycle on 5 x 4 x 3: {asym[name]:.3e}")
    assert asym["symmetric"] * MARGIN < asym["one-way"], "the margin the reference shows, two decades to spare"
    assert asym["symmetric"] < SYMMETRIC_BELOW and asym["one-way"] > ONE_WAY_ABOVE
    assert asym["forward post-sweep"] > ONE_WAY_ABOVE, "the planted fault loses the symmetry"


# --------------------------------------------------------------------------------------------------------- the counts
def krylov_problem(shape):
    A = sr.laplacian7(*shape)
    return A, np.random.default_rng(24).standard_normal(A[0])


@pytest.mark.parametrize("hierarchy", HIERARCHIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_cg_counts_jacobi_against_gauss_seidel(shape, hierarchy):
    """the table of DESIGN.md section 32; on 24 x 20 x 16 the symmetric smoother takes strictly fewer iterations than Jacobi
    at 1 and 2 sweeps, on both hierarchies"""
    A, b = krylov_problem(shape)
    levels, o = gr.setup_ref(A, hierarchy, **KRYLOV_OPTS)
    x0 = np.zeros(A[0])
    for nu in SWEEPS:
        got = []
        for sm in (dict(kind=gr.JACOBI), dict()):
            res = cg_ref(gr.GsCsr(A, levels=levels, o=o, sm=dict(sm, nu1=nu, nu2=nu)), b, x0, KRYLOV_TOL, 500)
            assert res[1] == CONVERGED
            got.append(res[2])
        print(f"CG iterations on {shape}, {hierarchy}, nu1 = nu2 = {nu} (Jacobi, Gauss-Seidel):", tuple(got))
        assert tuple(got) == COUNTS[(shape, hierarchy, nu)]
        if shape == (24, 20, 16):
            assert got[1] < got[0]
