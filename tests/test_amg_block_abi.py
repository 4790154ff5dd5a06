"""The block-cycle entry points (spmvHipAmgSetBlockWidth, spmvHipAmgBlock, spmvHipAmgApplyBlock) are declared, exported and
bound in Python with the C layout of their struct, and the test side's reference (tests/amg_block_ref.py) is column by column
the single cycle's: as bits for k = 1, 3, 16, 17 on plain, smoothed and strength hierarchies with both smoothers; the plain
correction done as a product with the unit prolongator instead of the gather changes the bits (a planted fault); and the CG
counts of DESIGN.md sections 28 and 30 come out per column when three scaled copies of b form a block.  No GPU needed."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import amg_block_ref as br
import amg_cheb_ref as cr
import amg_ref as ar
import amg_sa_ref as sa
import c_header
import filter_ref as fr
import spgemm_ref as sr
import test_amg_cheb_abi as cheb_abi
import test_amg_sa_abi as sa_abi
from c_header import HEADER, code as _code
from conftest import ROOT
from krylov_ref import CONVERGED, Csr

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H = r"spmat\s*\*\s*\w+"
DENSE = r"size_t\s+\w+\s*,\s*int\s+\w+"
DECLS = {
    "spmvHipAmgSetBlockWidth": (H + r"\s*,\s*" + H + r"\s*,\s*unsigned\s+\w+", 3),
    "spmvHipAmgBlock": (H + r"\s*,\s*spmvAmgBlockInfo\s*\*\s*\w+", 2),
    "spmvHipAmgApplyBlock": (H + r"\s*,\s*" + H + r"\s*,\s*unsigned\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*" + DENSE +
                             r"\s*,\s*double\s*\*\s*\w+\s*,\s*" + DENSE, 9),
}
STRUCTS = {"spmvAmgBlockInfo": ("width", "bytes")}
LAP = sr.laplacian7(12, 10, 8)
ANISO = fr.stencil7(12, 10, 8, (1.0, 0.01, 0.01))
WIDTHS = (1, 3, 16, 17)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_header_declares_the_entry_points_and_the_struct():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in STRUCTS.items():
        assert c_header.structs()[struct] == list(fields), struct
    assert all(c_header.prototypes()[name] == n for name, (_, n) in DECLS.items())


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
    body = ""
    for name, fields in STRUCTS.items():
        body += f'    printf("{name} %zu", sizeof({name}));\n'
        body += "".join(f'    printf(" %zu", offsetof({name}, {f}));\n' for f in fields) + '    printf("\\n");\n'
    layout = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in c_header.run_c(tmp_path, body, "amg_block_layout").splitlines()}
    for struct, fields in STRUCTS.items():
        py = getattr(api, struct)
        assert [f[0] for f in py._fields_] == list(fields)
        assert layout[struct] == [C.sizeof(py)] + [getattr(py, f).offset for f in fields], struct
    assert list(inspect.signature(api.AmgHierarchy.set_block_width).parameters) == ["self", "width"]
    assert list(inspect.signature(api.AmgHierarchy.block_info).parameters) == ["self"]
    params = inspect.signature(api.AmgHierarchy.apply_block).parameters
    assert list(params) == ["self", "R", "out"] and params["out"].default is None
    amg = inspect.signature(api.DeviceMatrix.amg).parameters
    assert list(amg) == ["self", "seed", "coarseRows", "maxLevels", "omega", "nu1", "nu2", "nuCoarse", "smoothed", "omegaP", "theta", "thetaScale"]
    for method in ("cg_block", "bicgstab_block"):
        assert list(inspect.signature(getattr(api.DeviceMatrix, method)).parameters) == ["self", "B", "X0", "precond", "tol", "maxiter", "history"]


# ------------------------------------------------------------------------------------------------------- the reference
@functools.lru_cache(maxsize=None)
def levels_of(hierarchy):
    return cr.setup_ref(ANISO if hierarchy == "strength" else LAP, hierarchy, coarseRows=8)


@pytest.mark.parametrize("hierarchy", br.HIERARCHIES)
def test_the_block_reference_is_the_column_references(hierarchy):
    levels, o = levels_of(hierarchy)
    assert len(levels) >= 3
    M = levels[0]["A"][0]
    R = br.ordinary_block(M, max(WIDTHS))
    for name in br.SMOOTHERS:
        sm = br.smoother_of(o, name)
        for k in WIDTHS:
            Z = br.block_cycle_ref(levels, o, R[:, :k], sm)
            assert Z.shape == (M, k)
            for c in range(k):
                if sm["kind"] == cr.JACOBI:                    # the cycles of the setups' own references
                    oo = dict(o, nu1=sm["nu1"], nu2=sm["nu2"], nuCoarse=sm["nuCoarse"])
                    want = ar.cycle_ref(levels, oo, R[:, c]) if hierarchy == "plain" else sa.cycle_ref(levels, oo, R[:, c])
                else:
                    want = cr.cycle_ref(levels, o, R[:, c], sm)
                assert np.array_equal(_bits(Z[:, c]), _bits(want)), (name, k, c)
    # the test block: its columns differ on every level, so a column in the place of another changes bits
    br.assert_columns_differ_on_every_level(levels, o, R[:, :5], br.smoother_of(o, "jacobi118"))
    br.assert_columns_differ_on_every_level(levels, o, R[:, :5], br.smoother_of(o, "cheb222"))


def test_the_special_block_holds_what_it_says():
    R = br.special_block(960)
    assert not R[:, 1].any() and not np.signbit(R[:, 1]).any()
    assert np.signbit(R[::3, 3]).all() and not R[::3, 3].any()
    assert np.isnan(R[:, 4]).sum() == 1 and np.isinf(R[:, 6]).sum() == 2 and (R[:, 6] == 1e308).sum() == 1
    T = br.tamed(R)
    assert np.all(np.isfinite(T)) and all(np.array_equal(_bits(T[:, c]), _bits(R[:, c])) for c in range(8) if c not in br.SPECIAL)


def test_a_correction_by_the_unit_prolongator_is_not_the_gather():
    """The planted fault: z = z + P e with the unit P of a plain hierarchy instead of z = z + e[agg].  P e starts every row at
    +0.0, so an e_j = -0.0 arrives as +0.0.  The input was found by search over the candidates below on the CPU reference: on
    the NEGATED Laplacian every dinv_i is negative, so r = 0 gives z = omega * (dinv * (+0.0)) = -0.0 on every level, e = -0.0,
    and the gather keeps z = -0.0 + -0.0 = -0.0 where the product gives -0.0 + +0.0 = +0.0.  On the Laplacian itself no
    candidate shows it (every value is the same under both forms there)."""
    neg = LAP[:4] + (-LAP[4],)
    found = []
    for A, label in ((LAP, "laplacian"), (neg, "negated")):
        levels, o = ar.setup_ref(A, coarseRows=8)
        planted = [dict(lv, Pcsr=Csr(lv["P"][0], lv["P"][2], lv["P"][3], lv["P"][4])) if "P" in lv else lv for lv in levels]
        sm = cr.smoother(o, kind=cr.JACOBI)
        for r, what in ((np.random.default_rng(5).standard_normal(A[0]), "random"), (np.zeros(A[0]), "zeros")):
            good, bad = cr.cycle_ref(levels, o, r, sm), cr.cycle_ref(planted, o, r, sm)
            assert np.array_equal(good, bad), "the same values"
            if not np.array_equal(_bits(good), _bits(bad)):
                found.append((label, what))
                assert np.signbit(good).all() and not np.signbit(bad).any()
    assert found == [("negated", "zeros")]


# --------------------------------------------------------------------------------------------------------- the counts
@pytest.mark.parametrize("hierarchy", cheb_abi.HIERARCHIES)
def test_the_cg_counts_of_the_tables_come_out_per_column(hierarchy):
    """DESIGN.md section 30's table (Jacobi and Chebyshev at eigRatio 10, nu1 = nu2 = 2 and 3) and section 28's (Jacobi at the
    setup's counts): b, 2 b and b / 2 as one block -- scaling by a power of two scales every quantity of the loop exactly"""
    shape = (12, 10, 8)
    A, b = cheb_abi.krylov_problem(shape)
    levels, o = cr.setup_ref(A, hierarchy, **cheb_abi.KRYLOV_OPTS)
    B = np.stack([b, 2.0 * b, 0.5 * b], axis=1)
    X0 = np.zeros_like(B)
    cases = [(dict(kind=cr.JACOBI), sa_abi.COUNTS[shape][1 if hierarchy == "plain" else 2])]
    for nu in cheb_abi.DEGREES:
        want = cheb_abi.COUNTS[(shape, hierarchy, nu)]
        cases += [(dict(kind=cr.JACOBI, nu1=nu, nu2=nu), want[0]), (dict(eigRatio=10.0, nu1=nu, nu2=nu), want[2])]
    for sm, count in cases:
        cols, (status, iterations, _, _) = br.block_solve_ref("cg", cr.ChebCsr(A, levels=levels, o=o, sm=sm), B, X0, cheb_abi.KRYLOV_TOL, 500)
        assert status == CONVERGED and iterations == count
        assert [c.iterations for c in cols] == [count] * 3, (sm, [c.iterations for c in cols])
        assert np.array_equal(_bits(cols[1].x), _bits(2.0 * cols[0].x)) and np.array_equal(_bits(cols[2].x), _bits(0.5 * cols[0].x))
