"""spmvHipCsrFilter / spmvHipCsrFilterRefresh and the strength-filtered multigrid setup are declared, exported and bound in
Python, and the test side's reference (tests/filter_ref.py) is the loop of include/spmvHip.h: the vectorised form equals the
plain loop as bits, every mode equals a dense formulation, BAND(0, 0) of the Laplacian is its diagonal and tril + triu - diag
gives A back, the lumped inputs used on the GPU can tell a reversed order apart and their filters are neither trivial nor
empty, the filtered hierarchy takes fewer CG iterations than the smoothed one on an anisotropic stencil, and a tiny theta
changes nothing.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import add_ref as ad
import amg_ref as ar
import amg_sa_ref as sa
import filter_ref as fr
import serial_order_inputs as si
import spgemm_ref as sr
from c_header import HEADER, code as _code
from conftest import ROOT
from krylov_ref import CONVERGED, Csr, cg_ref

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H = r"spmat\s*\*\s*\w+"
SEP = r"\s*,\s*"
DECLS = {
    "spmvHipCsrFilter": (SEP.join([H, r"const\s+spmvFilterOpts\s*\*\s*\w+", H, r"spmvFilterInfo\s*\*\s*\w+"]), 4),
    "spmvHipCsrFilterRefresh": (SEP.join([H, H, r"spmvFilterInfo\s*\*\s*\w+"]), 3),
    "spmvHipAmgSetupStrength": (SEP.join([H, r"const\s+spmvAmgOpts\s*\*\s*\w+", r"const\s+spmvAmgSmoothOpts\s*\*\s*\w+",
                                          r"const\s+spmvAmgStrengthOpts\s*\*\s*\w+", H, r"spmvAmgInfo\s*\*\s*\w+"]), 6),
    "spmvHipAmgStrength": (SEP.join([H, r"unsigned\s+\w+", H, r"double\s*\*\s*\w+"]), 4),
}
STRUCTS = {"spmvFilterOpts": ("mode", "lo", "hi", "theta", "lump"),
           "spmvFilterInfo": ("nnzA", "nnzC", "maxRowNnz", "lumpedRows", "tempBytes", "ms"),
           "spmvAmgStrengthOpts": ("theta", "thetaScale")}
ANISO, ISO = (1.0, 0.01, 0.01), (1.0, 1.0, 1.0)
KRYLOV_OPTS, KRYLOV_TOL = dict(coarseRows=8), 1e-8
# weights -> CG iterations of the reference loop on the 12 x 10 x 8 stencil: no preconditioner, smoothed, strength-filtered
COUNTS = {ANISO: (68, 37, 15), ISO: (48, 13, 13)}


def test_header_declares_the_entry_points_the_modes_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body, struct
        names = [n for decl in body.group(1).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == list(fields), (struct, names)
    for name, value in (("SPMV_FILTER_BAND", 0), ("SPMV_FILTER_ABS", 1), ("SPMV_FILTER_STRENGTH", 2)):
        assert re.search(r"^\s*#define\s+" + name + r"\s+" + str(value) + r"\b", code, re.M), name


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
    for m in ("filter", "filter_refresh", "filter_info", "tril", "triu", "diagonal_matrix"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert callable(api.AmgHierarchy.strength)
    params = inspect.signature(api.DeviceMatrix.amg).parameters
    assert params["theta"].default is None and params["thetaScale"].default is None
    for struct, fields in STRUCTS.items():
        assert [f[0] for f in getattr(api, struct)._fields_] == list(fields)
    assert (api.SPMV_FILTER_BAND, api.SPMV_FILTER_ABS, api.SPMV_FILTER_STRENGTH) == (fr.BAND, fr.ABS, fr.STRENGTH)


# ------------------------------------------------------------------------------------------------------ the reference
def _every_option(square):
    out = [fr.opts(fr.BAND, -1, 2), fr.opts(fr.BAND, None, 0), fr.opts(fr.BAND, 0, None), fr.opts(fr.BAND, 0, 0), fr.opts(fr.BAND, 3, 1),
           fr.opts(fr.ABS, theta=0.0), fr.opts(fr.ABS, theta=1.25), fr.opts(fr.ABS, theta=1e300)]
    if square:
        out += [fr.opts(fr.ABS, theta=1.25, lump=True), fr.opts(fr.STRENGTH, theta=0.25), fr.opts(fr.STRENGTH, theta=0.25, lump=True),
                fr.opts(fr.STRENGTH, theta=0.35, lump=True), fr.opts(fr.STRENGTH, theta=0.0, lump=True)]
    return out


@pytest.mark.parametrize("name", list(ar.small_graphs()))
def test_vectorised_reference_is_the_loop(name):
    A = fr.lump_inputs(1)[name]
    special = A[:4] + (fr.special_values(np.random.default_rng(2900), A[3].size),)
    for X in (A, special):
        for o in _every_option(True):
            C, kept = fr.filter_ref(X, o)
            L, kept_loop = fr.filter_loop(X, o)
            fr.same_bits(C, L, f"{name} {o}", lumped=o["lump"])
            assert np.array_equal(kept, kept_loop)
            irp = C[2].astype(np.int64)
            assert int(irp[-1]) == C[3].size == kept.size and np.all(np.diff(irp) >= 0) and np.all(np.diff(kept) > 0)
            assert np.array_equal(C[3], X[3][kept])
            if not o["lump"]:
                assert np.array_equal(C[4].view(np.uint64), X[4][kept].view(np.uint64)), "values are copied as bits"


def test_rectangular_reference_is_the_loop():
    rng = np.random.default_rng(2901)
    for M, N in ((40, 90), (90, 40)):
        A = sr.random_csr(rng, M, N, rng.integers(0, 7, M), lambda r, n: fr.special_values(r, n))
        for o in _every_option(False):
            fr.same_bits(fr.filter_ref(A, o)[0], fr.filter_loop(A, o)[0], f"{M}x{N} {o}")


@pytest.mark.parametrize("o", _every_option(True), ids=lambda o: f"mode{o['mode']}-{o['lo']}-{o['hi']}-{o['theta']}-{o['lump']}")
def test_every_mode_against_a_dense_formulation(o):
    """a matrix without repeats: C's pattern is the dense predicate on the stored places, and with lump every row sum stays"""
    A = sa.with_one_diagonal(*ar.small_graphs()["laplacian12x10x8"], seed=2)
    C, kept = fr.filter_ref(A, o)
    assert np.array_equal(sr.pattern_of(C), fr.dense_keep(A, o))
    D, Dc = sr.dense(A), sr.dense(C)
    off = ~np.eye(A[0], dtype=bool)
    assert np.array_equal(Dc[off & sr.pattern_of(C)], D[off & sr.pattern_of(C)])
    if o["lump"]:
        assert np.allclose(Dc.sum(axis=1), D.sum(axis=1), rtol=1e-13, atol=1e-13), "lumping keeps the row sums"
        assert 0 < kept.size
    else:
        assert np.array_equal(Dc, np.where(sr.pattern_of(C), D, 0.0))


def test_a_nan_fails_every_value_predicate_and_lumps_to_a_nan():
    A = sa.with_one_diagonal(*ar.path(9), seed=3)
    AS = A[4].copy()
    rows = si.row_of_entry(A[2])
    off = np.flatnonzero(A[3].astype(np.int64) != rows)
    AS[off[4]] = np.uint64(0x7FF8000000000123).view(np.float64)
    X = A[:4] + (AS,)
    for o in (fr.opts(fr.ABS, theta=0.0), fr.opts(fr.STRENGTH, theta=0.0)):
        C, kept = fr.filter_ref(X, o)
        assert off[4] not in kept and kept.size == A[3].size - 1
    C, kept = fr.filter_ref(X, fr.opts(fr.STRENGTH, theta=0.0, lump=True))
    d = C[4][C[3].astype(np.int64) == si.row_of_entry(C[2])]
    assert np.count_nonzero(np.isnan(d)) == 1 and np.isnan(d[rows[off[4]]])
    B, _ = fr.filter_ref(X, fr.opts(fr.BAND, None, None))
    assert np.array_equal(B[4].view(np.uint64), AS.view(np.uint64)), "a band copies a NaN with its payload"


def test_band_zero_zero_is_the_diagonal_and_the_triangles_give_a_back():
    A = sr.laplacian7(6, 5, 4)
    D, _ = fr.filter_ref(A, fr.opts(fr.BAND, 0, 0))
    assert np.array_equal(D[2], np.arange(A[0] + 1)) and np.array_equal(D[3], np.arange(A[0])) and np.all(D[4] == 6.0)
    L, _ = fr.filter_ref(A, fr.opts(fr.BAND, None, 0))
    U, _ = fr.filter_ref(A, fr.opts(fr.BAND, 0, None))
    back = ad.add_ref(1.0, ad.add_ref(1.0, L, 1.0, U), -1.0, D)
    sr.same_bits(back, A, "tril + triu - diag")
    E, kept = fr.filter_ref(A, fr.opts(fr.BAND, 1, 0))
    assert kept.size == 0 and not E[2].any() and E[2].size == A[0] + 1, "lo > hi: a valid empty C"
    S, _ = fr.filter_ref(A, fr.opts(fr.BAND, -1, -1))
    assert np.array_equal(S[3].astype(np.int64) + 1, si.row_of_entry(S[2]))


LUMP_CASES = [("laplacian12x10x8", 0.25), ("messy", 0.25), ("path70", 0.35)]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name,theta", LUMP_CASES)
def test_the_lumped_inputs_can_tell_a_reversed_order_apart(name, theta, seed):
    """adding a row's dropped values in reverse stored order changes the bits of at least one diagonal"""
    A = fr.lump_inputs(seed)[name]
    o = fr.opts(fr.STRENGTH, theta=theta, lump=True)
    C, _ = fr.filter_ref(A, o)
    R, _ = fr.filter_ref(sr.reverse_rows(A), o)

    def diag(X):
        return X[4][X[3].astype(np.int64) == si.row_of_entry(X[2])].view(np.uint64)
    differ = np.count_nonzero(diag(C) != diag(R))
    print(name, theta, seed, "diagonals that differ under a reversed order:", differ)
    assert differ >= 1
    assert differ >= {"laplacian12x10x8": 700, "messy": 7, "path70": 27}[name]


@pytest.mark.parametrize("seed", [0, 1])
def test_the_filters_are_neither_trivial_nor_empty(seed):
    G = fr.lump_inputs(seed)

    def kept_off(name, theta):
        A = G[name]
        return fr.filter_ref(A, fr.opts(fr.STRENGTH, theta=theta, lump=True))[0][3].size - A[0], A[3].size - A[0]
    for name in ("path70", "messy"):
        kept, every = kept_off(name, 0.25)
        print(name, seed, kept, "of", every)
        assert 0 < kept < every, name
    if seed == 0:
        assert kept_off("path70", 0.25) == (102, 138) and kept_off("messy", 0.25) == (30, 88)
    assert kept_off("star200", 0.25) == (0, 400) and kept_off("star200_upper", 0.25)[0] == 0
    assert kept_off("laplacian12x10x8", 0.08) == (5168, 5168) and kept_off("laplacian12x10x8", 0.25) == (0, 5168)


def test_refresh_reference_keeps_the_pattern_and_follows_the_values():
    A = fr.lump_inputs(0)["messy"]
    o = fr.opts(fr.STRENGTH, theta=0.25, lump=True)
    C, kept = fr.filter_ref(A, o)
    B = A[:4] + (A[4] * 2.0,)
    R = fr.filter_refresh_ref(kept, B, o)
    fresh, kept2 = fr.filter_ref(B, o)
    assert np.array_equal(kept, kept2), "every comparison scales by exactly 4"
    fr.same_bits(R, fresh, "refresh = fresh when the kept set is the same")
    assert np.array_equal(R[4].view(np.uint64), (C[4] * 2.0).view(np.uint64))
    rng = np.random.default_rng(2902)
    P = A[:4] + (A[4] * (1.0 + rng.random(A[4].size)),)
    R2 = fr.filter_refresh_ref(kept, P, o)
    fresh2, kept3 = fr.filter_ref(P, o)
    assert not np.array_equal(kept, kept3), "a fresh filter would keep other entries"
    assert np.array_equal(R2[2], C[2]) and np.array_equal(R2[3], C[3]), "the pattern stays"
    assert np.allclose(sr.dense(R2).sum(axis=1), sr.dense(P).sum(axis=1), rtol=1e-13), "... and the values follow"


# ------------------------------------------------------------------------------------------- the filtered hierarchy
def krylov_problem(weights):
    A = fr.stencil7(12, 10, 8, weights)
    return A, np.random.default_rng(24).standard_normal(A[0])


def test_theta_is_scaled_by_one_rounded_product_per_level():
    A, _ = krylov_problem(ANISO)
    levels, _ = fr.strength_setup_ref(A, 0.3, 0.3, **KRYLOV_OPTS)
    th = [lv["theta"] for lv in levels[:-1]]
    assert len(th) >= 3 and th[0] == 0.3 and th[1] == np.float64(0.3) * np.float64(0.3) and th[2] == th[1] * np.float64(0.3)
    default, _ = fr.strength_setup_ref(A, **KRYLOV_OPTS)
    assert [lv["theta"] for lv in default[:-1]] == [0.08, 0.04, 0.02, 0.01]


def test_reference_cg_counts_filtered_below_smoothed_below_none():
    """the counts of DESIGN.md section 29"""
    got = {}
    for weights in (ANISO, ISO):
        A, b = krylov_problem(weights)
        x0 = np.zeros(A[0])
        none = cg_ref(Csr(A[0], A[2], A[3], A[4]), b, x0, KRYLOV_TOL, 500)
        smooth = cg_ref(sa.SaCsr(A, **KRYLOV_OPTS), b, x0, KRYLOV_TOL, 500)
        strength = cg_ref(fr.StrengthCsr(A, **KRYLOV_OPTS), b, x0, KRYLOV_TOL, 500)
        assert none[1] == smooth[1] == strength[1] == CONVERGED
        got[weights] = (none[2], smooth[2], strength[2])
        print("CG iterations (none, smoothed, strength-filtered), weights", weights, got[weights])
    n, s, f = got[ANISO]
    assert f < s < n
    assert got[ISO][2] <= got[ISO][1] + 1
    assert got == COUNTS


def test_levels_and_complexity_of_the_filtered_hierarchy():
    A, _ = krylov_problem(ANISO)
    levels, _ = fr.strength_setup_ref(A, **KRYLOV_OPTS)
    assert [lv["A"][0] for lv in levels] == [960, 296, 106, 13, 2] and round(sa.complexity(levels), 2) == 1.65
    F = levels[0]["F"]
    rows = si.row_of_entry(F[2])
    assert np.all(np.abs(F[3].astype(np.int64) - rows) % 80 == 0), "level 0 keeps the strong (x) direction alone"
    assert np.allclose(sr.dense(F).sum(axis=1), sr.dense(A).sum(axis=1), atol=1e-13)


@pytest.mark.parametrize("name", [n for n, g in ar.small_graphs().items() if g[0]])
def test_a_tiny_theta_changes_nothing(name):
    """theta = 1e-200: theta * theta is 0.0 and every nonzero entry is kept"""
    A = fr.lump_inputs(2)[name]
    assert np.all(A[4] != 0.0) and np.float64(1e-200) * np.float64(1e-200) == 0.0
    got, _ = fr.strength_setup_ref(A, theta=1e-200, **KRYLOV_OPTS)
    want, _ = sa.setup_ref(A, **KRYLOV_OPTS)
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want)):
        sr.same_bits(g["A"], w["A"], f"A of level {l}")
        assert np.array_equal(g["dinv"].view(np.uint64), w["dinv"].view(np.uint64))
        assert ("agg" in g) == ("agg" in w)
        if "agg" in w:
            sr.same_bits(g["F"], w["A"], f"F of level {l} is A")
            assert np.array_equal(g["agg"], w["agg"]) and np.float64(g["w"]).view(np.uint64) == np.float64(w["w"]).view(np.uint64)
            sr.same_bits(g["P"], w["P"], f"P of level {l}")
            sr.same_bits(g["R"], w["R"], f"R of level {l}")
