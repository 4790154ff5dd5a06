"""The multigrid entry points are declared, exported and bound in Python with the C layout of their structs, and the test
side's reference (tests/amg_ref.py) has the properties the header states: on every small graph the roots are pairwise more
than 2 apart, every vertex is within 2 of a root and in its ring's aggregate, ids are dense and ordered by root row; a
second seed changes the aggregation; integer-valued A gives the dense P^T A P exactly; a one-level cycle with one sweep is
omega * (r / d); and on the Laplacian the GPU test solves, reference CG with the cycle takes fewer iterations than without.
No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import amg_ref as ar
import spgemm_ref as sr
from c_header import HEADER, code as _code
from conftest import ROOT
from krylov_ref import CONVERGED, Csr, cg_ref

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H = r"spmat\s*\*\s*\w+"
DECLS = {
    "spmvHipAggregateCSR": (H + r"\s*,\s*const\s+spmvAggOpts\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*spmvAggInfo\s*\*\s*\w+", 4),
    "spmvHipAmgSetup": (H + r"\s*,\s*const\s+spmvAmgOpts\s*\*\s*\w+\s*,\s*" + H + r"\s*,\s*spmvAmgInfo\s*\*\s*\w+", 4),
    "spmvHipAmgRefresh": (H + r"\s*,\s*" + H, 2),
    "spmvHipAmgApply": (H + r"\s*,\s*" + H + r"\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+", 4),
    "spmvHipAmgInfo": (H + r"\s*,\s*spmvAmgInfo\s*\*\s*\w+", 2),
    "spmvHipAmgLevel": (H + r"\s*,\s*unsigned\s+\w+\s*,\s*" + H + r"\s*,\s*const\s+uint32_t\s*\*\*\s*\w+\s*,\s*const\s+double\s*\*\*\s*\w+", 5),
}
STRUCTS = {
    "spmvAggOpts": ("seed",),
    "spmvAggInfo": ("aggregates", "rounds", "hostChecks", "longRows", "symmetric", "maxAggRows", "minAggRows", "ms"),
    "spmvAmgOpts": ("seed", "coarseRows", "maxLevels", "omega", "nu1", "nu2", "nuCoarse"),
    "spmvAmgInfo": ("levels", "rows", "nnz", "aggregates", "opComplexity", "bytes", "tempBytes", "ms"),
}
GRAPHS = ar.small_graphs()
# the Laplacian of the Krylov tests (here and on the GPU) and its hierarchy
KRYLOV_SHAPE, KRYLOV_OPTS, KRYLOV_TOL = (12, 10, 8), dict(coarseRows=8), 1e-8


def test_header_declares_the_entry_points_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body, struct
        names = [n for decl in body.group(1).split(";") for n in re.findall(r"(\w+)\s*(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
        assert names == list(fields), (struct, names)


def test_library_exports_them():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_them():
    from spmv_openmp_cuda_amd import api
    for name, (_, nargs) in DECLS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == nargs, name
    for m in ("aggregate", "amg"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    for m in ("apply", "refresh_from", "free", "level"):
        assert callable(getattr(api.AmgHierarchy, m)), m
    for struct, fields in STRUCTS.items():
        assert [f[0] for f in getattr(api, struct)._fields_] == list(fields)
    assert (api.SPMV_AMG_MAX_LEVELS, api.SPMV_AMG_NO_SWEEPS) == (16, 0xFFFFFFFF)


@pytest.mark.parametrize("seed", [0, 0x9E3779B9])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_reference_aggregation_has_the_stated_properties(name, seed):
    M, IRP, JA = GRAPHS[name]
    agg, roots, ring = ar.aggregate_ref(M, IRP, JA, seed, detail=True)
    adj = ar.adjacency(M, IRP, JA)
    near = [ar.within2(adj, i) for i in range(M)]
    for r in roots:
        assert not near[r] & set(roots), f"{name}: roots {r} and {near[r] & set(roots)} are within distance 2"
    for i in range(M):
        assert i in roots or near[i] & set(roots), f"{name}: vertex {i} has no root within distance 2"
        if ring[i] == 1:
            (r,) = [k for k in adj[i] if k in roots]
            assert agg[i] == agg[r]
        if ring[i] == 2:
            assert not [k for k in adj[i] if k in roots]
            assert agg[i] in {agg[k] for k in adj[i] if ring[k] == 1}
    assert [int(agg[r]) for r in roots] == list(range(len(roots))), f"{name}: ids dense and ordered by root row"
    assert M == 0 or int(agg.max()) == len(roots) - 1
    for i in range(M):
        if not adj[i]:
            assert i in roots, f"{name}: an isolated vertex is a root of its own"


def test_a_second_seed_changes_the_aggregation():
    M, IRP, JA = GRAPHS["laplacian12x10x8"]
    assert not np.array_equal(ar.aggregate_ref(M, IRP, JA, 0), ar.aggregate_ref(M, IRP, JA, 0x9E3779B9))


def test_the_middle_first_seed_exists():
    seed = ar.middle_first_seed()
    M, IRP, JA = ar.path(5)
    assert ar.aggregate_ref(M, IRP, JA, seed).tolist() == [0, 0, 0, 1, 1]


def test_integer_values_give_the_dense_galerkin_product_exactly():
    A = sr.laplacian7(5, 4, 3, sr.integer_values)
    A = A[:4] + (np.where(A[3].astype(np.int64) == np.repeat(np.arange(A[0]), np.diff(A[2].astype(np.int64))), 7.0, A[4]),)
    levels, _ = ar.setup_ref(A, coarseRows=4, maxLevels=2)
    assert len(levels) == 2
    P = sr.dense(levels[0]["P"])
    assert np.array_equal(sr.dense(levels[1]["A"]), P.T @ sr.dense(A) @ P)


def test_one_level_one_sweep_is_scaled_jacobi():
    A = sr.laplacian7(4, 3, 2)
    levels, o = ar.setup_ref(A, maxLevels=1, nuCoarse=1, omega=0.5)
    assert len(levels) == 1
    r = np.arange(1.0, A[0] + 1.0) * 3.0                       # multiples of 3 below 2^53: r / 6 * 0.5 is exact
    z = ar.cycle_ref(levels, o, r)
    assert np.array_equal(z.view(np.uint64), (0.5 * (r / 6.0)).view(np.uint64))
    o0 = dict(o, nuCoarse=0)
    assert not ar.cycle_ref(levels, o0, r).view(np.uint64).any(), "no sweep: +0.0"


def krylov_problem():
    A = sr.laplacian7(*KRYLOV_SHAPE)
    rng = np.random.default_rng(24)
    return A, rng.standard_normal(A[0])


def test_reference_cg_takes_fewer_iterations_with_the_cycle():
    """the condition the GPU test relies on; the two counts are in DESIGN.md section 24"""
    A, b = krylov_problem()
    x0 = np.zeros(A[0])
    plain = cg_ref(Csr(A[0], A[2], A[3], A[4]), b, x0, KRYLOV_TOL, 500)
    amg = cg_ref(ar.AmgCsr(A, **KRYLOV_OPTS), b, x0, KRYLOV_TOL, 500)
    print("CG iterations: plain", plain[2], "with the cycle", amg[2])
    assert plain[1] == amg[1] == CONVERGED
    assert amg[2] < plain[2], (amg[2], plain[2])
    assert len(ar.AmgCsr(A, **KRYLOV_OPTS).levels) >= 3
