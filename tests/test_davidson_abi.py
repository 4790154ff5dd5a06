"""spmvHipBlockResidual and hipSpDavidsonCSR are declared, exported and bound in Python with the C layout of spmvDavidsonOpts
and spmvDavidsonInfo, and the test side's reference (tests/davidson_ref.py) is the loop of include/spmvHip.h: davidson_ref
equals the loop written in plain Python (math.sqrt, float) on every small case of tests/davidson_exit_inputs.py, every case
of that table takes the exit the table claims for it, the table is complete, five planted faults each change a case, the
reference's eigenpairs are the matrix's on the converged cases and on the 12 x 10 x 8 Laplacian, and on the 21 x 19 x 17
Laplacian the loop with ILU(0) as M^-1 takes fewer products than Lanczos, and without one about as many.  No GPU needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import davidson_exit_inputs as exits
import davidson_ref as dr
import lanczos_ref as lr
from bits import assert_same_bits
from c_header import HEADER, code as _code
from conftest import ROOT
from ilu0_ref import ilu0_levels
from krylov_ref import BREAKDOWN, CONVERGED, MAXITER, NONFINITE, Csr, dot_ref
from test_krylov_abi import _div, _ops, _same, dot_loop
from test_lanczos_abi import _sqrt, combine_loop, jacobi_loop
from test_trsv_abi import laplacian7

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
_D, _CD, _SZ, _U = r"double\s*\*\s*\w+", r"const\s+double\s*\*\s*\w+", r"size_t\s+\w+", r"unsigned\s+\w+"
DECLS = {
    "spmvHipBlockResidual": (r"\s*,\s*".join([_SZ, _U, _U, _CD, _SZ, _CD, _SZ, _CD, _SZ, _CD, _D, _SZ, _D]), 13),
    "hipSpDavidsonCSR": (r"\s*,\s*".join([r"spmat\s*\*\s*\w+", r"spmat\s*\*\s*\w+", _CD, r"const\s+spmvDavidsonOpts\s*\*\s*\w+", _D, _SZ, _D, _D,
                                          r"spmvDavidsonInfo\s*\*\s*\w+"]), 9),
}
OPTS = ("nev", "ncv", "which", "tol", "maxIter", "keep")
INFO = ("status", "found", "iterations", "restarts", "precondApplies", "launches", "hostChecks", "scale", "sweepsMax", "ms", "jacobiMs")
# Measured on the reference over the table's converged cases and the Laplacian cases below: the
# largest |theta[i] - eigenvalue|, the largest |X^T X - I| entry and the largest |res[i] - ||A x_i - theta_i x_i|||
# recomputed from X were 2.7e-14, 2.3e-15 and 3.8e-15 (all three on the Laplacian; the table's cases gave 8.9e-15, 1.8e-15
# and 2.3e-15).  The tests assert ten times those, so a later edit of the loop that loses an order of magnitude shows.
THETA_GAP_MEASURED = 2.7e-14
ORTH_GAP_MEASURED = 2.3e-15
RES_GAP_MEASURED = 3.8e-15
THETA_GAP, ORTH_GAP, RES_GAP = 10 * THETA_GAP_MEASURED, 10 * ORTH_GAP_MEASURED, 10 * RES_GAP_MEASURED


def test_header_declares_the_two_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in (("spmvDavidsonOpts", OPTS), ("spmvDavidsonInfo", INFO)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body and re.findall(r"(\w+)\s*;", body.group(1)) == list(fields), struct
    assert code.index("hipSpLanczosCSR") < code.index("hipSpDavidsonCSR"), "declared after Lanczos"


def test_library_exports_the_two():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_two():
    import inspect

    from spmv_openmp_cuda_amd import api
    for name, (_, n) in DECLS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == n, name
    assert callable(api.block_residual)
    assert [f[0] for f in api.spmvDavidsonOpts._fields_] == list(OPTS)
    assert [f[0] for f in api.spmvDavidsonInfo._fields_] == list(INFO)
    sig = inspect.signature(api.DeviceMatrix.eigsh).parameters
    assert sig["method"].default == "lanczos" and sig["precond"].default is None


# ------------------------------------------------------------------------------------------------- the loop, restated
def residual_loop(V, W, S, theta, fault=None):
    """(R as a list of columns, norm2), one product and one add at a time; V, W lists of columns, S a list of rows"""
    order = range(len(V) - 1, -1, -1) if fault == "descending" else range(len(V))
    R, n2 = [], []
    for c in range(len(S[0])):
        col = []
        for i in range(len(V[0])):
            if fault == "rounding":
                acc = 0.0
                for j in order:
                    acc = acc + (W[j][i] - theta[c] * V[j][i]) * S[j][c]
                col.append(acc)
                continue
            u = q = 0.0
            for j in order:
                u = u + V[j][i] * S[j][c]
            for j in order:
                q = q + W[j][i] * S[j][c]
            col.append(q - theta[c] * u)
        R.append(col)
        n2.append(dot_loop(col, col))
    return R, n2


def davidson_loop(M, IRP, JA, AS, v0, nev, m, which, tol, maxiter, keep, dm=None, fault=None):
    """the loop of include/spmvHip.h on Python floats; dm: the diagonal of M, or None.  `fault` plants one of
    davidson_ref.FAULTS.  Returns (theta, res, X as a list of columns, status, found, iterations, restarts)."""
    spmv, _ = _ops(M, IRP, JA, AS, None)
    v0 = [float(a) for a in v0]
    nn = dot_loop(v0, v0)
    if not math.isfinite(nn):
        return [], [], [], NONFINITE, 0, 0, 0
    if nn == 0:
        return [], [], [], BREAKDOWN, 0, 0, 0
    if maxiter == 0:
        return [], [], [], MAXITER, 0, 0, 0
    nrm = _sqrt(nn)
    v, w = [[_div(a, nrm) for a in v0]], []
    H = [[0.0] * m for _ in range(m)]
    it = restarts = 0
    kk = keep if keep else min(m - 1, nev + (m - nev) // 2)
    while True:
        j = len(w)
        w.append(spmv(v[j]))
        it += 1
        for i in range(j + 1):
            H[i][j] = H[j][i] = dot_loop(v[i], w[j])
        cols = j + 1
        if not all(math.isfinite(H[i][j]) for i in range(cols)):
            return [], [], [], NONFINITE, 0, it, restarts
        jac = jacobi_loop([row[:cols] for row in H[:cols]])
        if jac is None or not all(math.isfinite(a) for a in jac[0]):
            return [], [], [], NONFINITE, 0, it, restarts
        d, S = jac
        order = sorted(range(cols), key=(lambda i: d[i]) if which == lr.SMALLEST else (lambda i: -d[i]))   # (sorted is stable)
        theta = [d[i] for i in order]
        S = [[row[i] for i in order] for row in S]
        scale = max(abs(a) for a in theta)
        c = min(nev, cols)
        R, n2 = residual_loop(v, w, [row[:c] for row in S], theta[:c], fault)
        res = [_sqrt(a) for a in n2]
        if not all(math.isfinite(a) for a in res):
            return [], [], [], NONFINITE, 0, it, restarts
        done = cols >= nev and all(res[i] <= tol * scale for i in range(nev))
        X = combine_loop(v, [row[:c] for row in S])
        if done or it == maxiter:
            return theta[:c], res, X, CONVERGED if done else MAXITER, c, it, restarts
        l = next((i for i in range(c) if res[i] > tol * scale), c - 1)
        if fault == "target 0":
            l = 0
        if cols == m:
            v, w = combine_loop(v, [row[:kk] for row in S]), combine_loop(w, [row[:kk] for row in S])
            if fault == "full H":
                Sk = np.array(S)[:, :kk]
                G = Sk.T @ np.array(H) @ Sk
                H = [[float(G[r][q]) if r < kk and q < kk else 0.0 for q in range(m)] for r in range(m)]
            else:
                H = [[theta[r] if r == q and r < kk else 0.0 for q in range(m)] for r in range(m)]
            restarts += 1
        t = R[l] if dm is None else [_div(a, b) for a, b in zip(R[l], dm)]
        for _ in range(1 if fault == "one pass" else 2):
            h = [dot_loop(vi, t) for vi in v]
            for hi, vi in zip(h, v):
                t = [ti - hi * a for ti, a in zip(t, vi)]
        beta = _sqrt(dot_loop(t, t))
        if not math.isfinite(beta):
            return [], [], [], NONFINITE, 0, it, restarts
        if beta == 0:
            return theta[:c], res, X, BREAKDOWN, c, it, restarts
        v.append([_div(a, beta) for a in t])


def _case_ref(c, trace=None, stats=None, **kw):
    return dr.davidson_ref(Csr(c.M, c.IRP, c.JA, c.AS), c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep, exits.precond_of(c),
                           trace, stats, **kw)


def _case_loop(c, fault=None):
    return davidson_loop(c.M, c.IRP, c.JA, c.AS, c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep,
                         None if c.dm is None else c.dm.tolist(), fault)


def _same_result(ref, loop, what):
    theta, res, X, st, found, it, rs = ref
    thl, resl, Xl, stl, foundl, itl, rsl = loop
    assert (st, found, it, rs) == (stl, foundl, itl, rsl), what
    _same(theta, thl, what + ": theta")
    _same(res, resl, what + ": res")
    for i in range(found):
        _same(X[:, i], Xl[i], what + f": X[:, {i}]")


@pytest.mark.parametrize("name", exits.NAMES)
def test_exit_case_takes_its_label_and_ref_is_the_loop(name):
    c = exits.case(name)
    trace, stats = [], {}
    ref = _case_ref(c, trace, stats)
    theta, res, X, st, found, it, rs = ref
    assert trace == [c.label] and c.label in dr.DAVIDSON_EXITS, (name, trace)
    assert (st, found) == (c.status, c.found) and (c.restarts is None or rs == c.restarts), (name, st, found, rs)
    assert theta.shape == res.shape == (found,) and X.shape == (c.M, found)
    assert stats["applies"] == (stats["expansions"] if c.dm is not None else 0)
    cols = stats["cols"]
    if c.how == "step1":
        assert it == 1 and cols == [1] and found == c.nev == 1 and np.all(res == 0) and not np.any(np.signbit(res))
    if c.how == "pass1":
        assert rs == 0 and it > c.nev and st == CONVERGED
    if c.how == "restarts":
        assert rs >= 2 and st == CONVERGED
    if c.how == "cols=nev":
        assert cols[-1] == c.nev and st == CONVERGED
    if c.how == "short":
        assert it == c.maxiter and cols[-1] < c.nev and found == cols[-1]
    if c.how == "mid":
        assert it == c.maxiter and rs >= 1 and c.nev <= cols[-1] < c.ncv
    if c.how == "restart":
        assert it == c.maxiter and cols[-1] == c.ncv
    if c.how == "exact":
        assert st == BREAKDOWN and found < c.nev and stats["targets"] == [0] and stats["checks"] == 2 * it + 1
    if c.how == "l>0":
        assert st == BREAKDOWN and stats["targets"][-1] > 0
    if c.how == "inf":
        assert not np.all(np.isfinite(c.AS)) and np.all(np.isfinite(c.v0)) and cols == []
    if c.how == "huge":
        assert np.all(np.isfinite(c.AS)) and cols == [1] and stats["expansions"] == 0
    if c.how == "dM":
        assert c.dm is not None and cols == [1] and stats["expansions"] == 1 and stats["checks"] == 3
    if name in exits.SMALL:
        _same_result(ref, _case_loop(c), name)


def test_exit_table_is_complete():
    """every label of the loop but the stated holes; every required way to reach one; a target other than the first pair;
    both ends of the spectrum without a dM; keep at both of its bounds; the smallest legal basis; a dM; the unit-value handle"""
    rows = [exits.case(n) for n in exits.NAMES]
    for label in dr.DAVIDSON_EXITS:
        assert any(r.label == label for r in rows) != (label in exits.HOLES), label
    assert set(exits.HOLES) <= set(dr.DAVIDSON_EXITS)
    for label, how in exits.REQUIRED:
        assert any((r.label, r.how) == (label, how) for r in rows), (label, how)
    conv = [r for r in rows if r.label == "converged" and r.how == "restarts"]
    assert {r.which for r in conv if r.dm is None} == {lr.LARGEST, lr.SMALLEST}
    assert any(r.keep == r.nev for r in conv) and any(r.keep == r.ncv - 1 for r in conv)
    assert any((r.nev, r.ncv) == (1, 2) for r in rows), "ncv = nev + 1"
    assert any(r.dm is not None and r.status == CONVERGED for r in rows)
    assert all(r.which == lr.SMALLEST for r in rows if r.dm is not None), "a dM goes with SMALLEST only"
    assert any(np.all(r.AS == r.AS[0]) and r.M >= 4 * 4096 for r in rows)
    late = {}
    _case_ref(exits.case("converged_la"), stats=late)
    assert max(late["targets"]) > 0, "a later pair is the target once the first has converged"


@pytest.mark.parametrize("fault", dr.FAULTS)
def test_exit_table_tells_planted_faults_apart(fault):
    """the plain loop with the fault against the reference without it: a case's bits or counts change"""
    caught = []
    for name in exits.SMALL:
        c = exits.case(name)
        try:
            _same_result(_case_ref(c), _case_loop(c, fault), name)
        except AssertionError:
            caught.append(name)
    print(fault, "caught by", caught)
    assert caught, fault


@pytest.mark.parametrize("fault", dr.FAULTS)
def test_faults_are_the_reference_s_too(fault):
    """davidson_ref(fault=...) is the plain loop's planted fault: the two restatements agree on the faults as well (the
    full-H fault goes through a matrix product whose order numpy chooses, so there only the counts are compared)"""
    c = exits.case("maxiter_restart_third")
    ref, loop = _case_ref(c, fault=fault), _case_loop(c, fault)
    if fault == "full H":
        assert ref[3:] == loop[3:]
    else:
        _same_result(ref, loop, fault)


# ------------------------------------------------------------------------------------------------- the parts
def test_residual_ref_is_the_loop():
    rng = np.random.default_rng(7300)
    V, W, S, theta = rng.standard_normal((37, 5)), rng.standard_normal((37, 5)), rng.standard_normal((5, 3)), rng.standard_normal(3)
    V[3, 2], W[4, 1], S[0, 0], W[9, 0] = -0.0, np.nan, -0.0, np.inf
    R, n2 = dr.residual_ref(V, W, S, theta)
    Rl, n2l = residual_loop([V[:, j].tolist() for j in range(5)], [W[:, j].tolist() for j in range(5)], S.tolist(), theta.tolist())
    for c in range(3):
        _same(R[:, c], Rl[c], f"column {c}")
    _same(n2, n2l, "norm2")
    bad = np.zeros(37, bool)
    bad[[4, 9]] = True
    assert not np.isfinite(R[bad]).any() and np.isfinite(R[~bad]).all(), "a NaN or an Inf stays in its row"
    assert np.isnan(n2).all(), "and reaches the norms"
    # the u part is block_combine's
    Z, _ = dr.residual_ref(V[:10], np.zeros((10, 5)), S, -np.ones(3))
    assert_same_bits(Z[:4], lr.combine_ref(V[:10], S)[:4], "q = +0.0 and theta = -1 leave u")
    # a finite case against numpy's own products to a few eps
    V, W = rng.standard_normal((50, 6)), rng.standard_normal((50, 6))
    S, theta = rng.standard_normal((6, 4)), rng.standard_normal(4)
    R, n2 = dr.residual_ref(V, W, S, theta)
    assert np.abs(R - (W @ S - (V @ S) * theta)).max() <= 64 * 2.0 ** -52 * 6 * 16
    assert np.abs(n2 - (R * R).sum(axis=0)).max() <= 64 * 2.0 ** -52 * n2.max()
    for c in range(4):
        assert n2[c] == dot_ref(R[:, c], R[:, c])


# ------------------------------------------------------------------------------------------------- properties
def _dense(A):
    D = np.zeros((A.M, A.M))
    D[np.repeat(np.arange(A.M), np.diff(A.IRP)), A.JA] = A.AS
    return D


def _gaps(A, theta, res, X, which):
    D = _dense(A)
    ev = np.linalg.eigvalsh(D)
    want = ev[::-1][:theta.size] if which == lr.LARGEST else ev[:theta.size]
    true = np.linalg.norm(D @ X - X * theta, axis=0)
    return np.abs(theta - want).max(), np.abs(X.T @ X - np.eye(theta.size)).max(), np.abs(true - res).max()


def test_ref_eigenpairs_over_the_converged_cases():
    worst = np.zeros(3)
    for name in exits.NAMES:
        c = exits.case(name)
        if c.status != CONVERGED or name == "2I" or c.how in ("step1", "cols=nev"):
            continue                                             # (those hold an invariant subspace's pairs, not the extreme ones)
        theta, res, X, st, found, it, rs = _case_ref(c)
        g = np.array(_gaps(Csr(c.M, c.IRP, c.JA, c.AS), theta, res, X, c.which))
        print(f"{name}: |theta - ev| {g[0]:.2e}, |X^T X - I| {g[1]:.2e}, |res - true| {g[2]:.2e}")
        worst = np.maximum(worst, g)
    print(f"converged cases of the table: |theta - ev| {worst[0]:.2e}, |X^T X - I| {worst[1]:.2e}, |res - true| {worst[2]:.2e}")
    assert worst[0] <= THETA_GAP and worst[1] <= ORTH_GAP and worst[2] <= RES_GAP


@pytest.mark.parametrize("which", [lr.LARGEST, lr.SMALLEST])
def test_ref_finds_the_extreme_eigenpairs_of_the_laplacian(which):
    IRP, JA, AS = laplacian7(12, 10, 8)
    A = Csr(960, IRP, JA, AS)
    v0 = np.random.default_rng(0).standard_normal(960)
    stats = {}
    theta, res, X, st, found, it, rs = dr.davidson_ref(A, v0, 4, 20, which, 1e-8, 5000, stats=stats)
    assert (st, found) == (CONVERGED, 4)
    g = _gaps(A, theta, res, X, which)
    print(f"which={which}: {it} products, {rs} restarts, {stats['sweeps']} sweeps at most; |theta - ev| {g[0]:.2e}, "
          f"|X^T X - I| {g[1]:.2e}, |res - true| {g[2]:.2e}")
    assert np.all(res <= 1e-8 * stats["scale"])
    assert g[0] <= THETA_GAP and g[1] <= ORTH_GAP and g[2] <= RES_GAP


def test_ilu0_davidson_needs_fewer_products_than_lanczos():
    """the point of the preconditioned solver, as a condition: on the 21 x 19 x 17 Laplacian, SMALLEST, (4, 20), tol 1e-8,
    v0 = default_rng(0), the loop with ILU(0) of A as M takes fewer products than Lanczos on the same input, and without
    an M no more than 1.25 times Lanczos's"""
    grid = (21, 19, 17)
    IRP, JA, AS = laplacian7(*grid)
    M = int(np.prod(grid))
    v0 = np.random.default_rng(0).standard_normal(M)
    lanczos = lr.lanczos_ref(Csr(M, IRP, JA, AS), v0, 4, 20, lr.SMALLEST, 1e-8, 2000)
    assert lanczos[3] == CONVERGED
    plain = dr.davidson_ref(Csr(M, IRP, JA, AS), v0, 4, 20, lr.SMALLEST, 1e-8, 2000)
    F = ilu0_levels(M, IRP, JA, AS)
    pre = Csr(M, IRP, JA, AS, F)
    stats = {}
    ilu = dr.davidson_ref(pre, v0, 4, 20, lr.SMALLEST, 1e-8, 2000, precond=pre.precond, stats=stats)
    print(f"products to 1e-8: Lanczos {lanczos[5]}, Davidson without M {plain[5]}, Davidson with ILU(0) {ilu[5]} "
          f"({stats['applies']} applications, {ilu[6]} restarts)")
    assert plain[3] == ilu[3] == CONVERGED
    assert ilu[5] < lanczos[5]
    assert plain[5] <= 1.25 * lanczos[5]
    assert np.abs(ilu[0] - lanczos[0]).max() <= 1e-7 * stats["scale"]
