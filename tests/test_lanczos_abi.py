"""spmvHipBlockCombine and hipSpLanczosCSR are declared, exported and bound in Python with the C layout of spmvLanczosOpts
and spmvLanczosInfo, and the test side's reference (tests/lanczos_ref.py) is the loop of include/spmvHip.h: lanczos_ref
equals the loop written in plain Python (math.sqrt, float) on every small case of tests/lanczos_exit_inputs.py, every case
of that table takes the exit the table claims for it, the table is complete, two planted faults each change a case, and on
the 12 x 10 x 8 Laplacian the reference's eigenpairs are the matrix's.  No GPU needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import lanczos_exit_inputs as exits
import lanczos_ref as lr
from bits import assert_same_bits
from c_header import HEADER, code as _code
from conftest import ROOT
from krylov_ref import BREAKDOWN, CONVERGED, MAXITER, NONFINITE, Csr
from test_krylov_abi import _div, _ops, _same, dot_loop
from test_trsv_abi import laplacian7

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
_D, _CD, _SZ, _U = r"double\s*\*\s*\w+", r"const\s+double\s*\*\s*\w+", r"size_t\s+\w+", r"unsigned\s+\w+"
DECLS = {
    "spmvHipBlockCombine": (r"\s*,\s*".join([_SZ, _U, _U, _CD, _SZ, _CD, _SZ, _D, _SZ]), 9),
    "hipSpLanczosCSR": (r"\s*,\s*".join([r"spmat\s*\*\s*\w+", _CD, r"const\s+spmvLanczosOpts\s*\*\s*\w+", _D, _SZ, _D, _D,
                                         r"spmvLanczosInfo\s*\*\s*\w+"]), 8),
}
OPTS = ("nev", "ncv", "which", "tol", "maxIter", "keep")
INFO = ("status", "found", "iterations", "cycles", "launches", "hostChecks", "scale", "sweepsMax", "ms", "jacobiMs")
# Measured on the reference over the table's converged cases and the Laplacian cases below:
# the largest |res[i] - ||A x_i - theta_i x_i||| was 8.2e-15 and the largest |X^T X - I| entry 2.3e-15 (both on the
# Laplacian, LARGEST; the table's cases gave 3.9e-15 and 1.6e-15).  The tests assert ten times those, so a later edit of
# the loop that loses an order of magnitude shows.
RES_GAP = 8.2e-14
ORTH_GAP = 2.3e-14


def test_header_declares_the_two_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in (("spmvLanczosOpts", OPTS), ("spmvLanczosInfo", INFO)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body and re.findall(r"(\w+)\s*;", body.group(1)) == list(fields), struct
    for name, value in (("LARGEST", lr.LARGEST), ("SMALLEST", lr.SMALLEST)):
        assert re.search(r"#define\s+SPMV_EIG_" + name + r"\s+" + str(value) + r"\b", code), name


def test_library_exports_the_two():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_two():
    from spmv_openmp_cuda_amd import api
    for name, (_, n) in DECLS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == n, name
    assert callable(api.DeviceMatrix.eigsh) and callable(api.block_combine)
    assert [f[0] for f in api.spmvLanczosOpts._fields_] == list(OPTS)
    assert [f[0] for f in api.spmvLanczosInfo._fields_] == list(INFO)
    assert api.EIG_WHICH == {"LA": lr.LARGEST, "SA": lr.SMALLEST}


# ------------------------------------------------------------------------------------------------- the loop, restated
def _sqrt(a):
    return math.sqrt(a) if a >= 0 else float("nan")


def combine_loop(V, S, descending=False):
    """Y = V S one product and one add at a time; V a list of columns, S a list of rows"""
    order = range(len(V) - 1, -1, -1) if descending else range(len(V))
    out = []
    for c in range(len(S[0])):
        col = []
        for i in range(len(V[0])):
            acc = 0.0
            for j in order:
                acc = acc + V[j][i] * S[j][c]
            col.append(acc)
        out.append(col)
    return out


def jacobi_loop(T):
    n = len(T)
    A = [row[:] for row in T]
    S = [[1.0 if r == c else 0.0 for c in range(n)] for r in range(n)]
    for sweep in range(1, lr.JACOBI_SWEEPS + 1):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p][q]
                if apq == 0:
                    continue
                app, aqq, g = A[p][p], A[q][q], abs(apq)
                if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                    A[p][q] = A[q][p] = 0.0
                    continue
                rotated = True
                th = _div(aqq - app, 2.0 * apq)
                t = _div(1.0, abs(th) + _sqrt(th * th + 1.0))
                if th < 0:
                    t = -t
                c = _div(1.0, _sqrt(t * t + 1.0))
                s = t * c
                tau = _div(s, 1.0 + c)
                h = t * apq
                for r in range(n):
                    if r in (p, q):
                        continue
                    x, y = A[r][p], A[r][q]
                    A[r][p] = A[p][r] = x - s * (y + tau * x)
                    A[r][q] = A[q][r] = y + s * (x - tau * y)
                A[p][p], A[q][q] = app - h, aqq + h
                A[p][q] = A[q][p] = 0.0
                for r in range(n):
                    x, y = S[r][p], S[r][q]
                    S[r][p] = x - s * (y + tau * x)
                    S[r][q] = y + s * (x - tau * y)
        if not rotated:
            return [A[i][i] for i in range(n)], S
    return None


def lanczos_loop(M, IRP, JA, AS, v0, nev, m, which, tol, maxiter, keep, fault=None):
    """the loop of include/spmvHip.h on Python floats.  `fault` plants one of the mistakes the exit table must tell apart:
    "one pass": a single projection pass; "descending": the sums of the rotation taken in descending j.
    Returns (theta, res, X as a list of columns, status, found, iterations, cycles)."""
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
    v = [[_div(a, nrm) for a in v0]]
    T = [[0.0] * m for _ in range(m)]
    k = it = cycles = 0
    kk = keep if keep else min(m - 1, nev + (m - nev) // 2)
    desc = fault == "descending"
    while True:
        cycles += 1
        cols, exact, beta = m, False, None
        del v[k + 1:]
        for j in range(k, m):
            w = spmv(v[j])
            it += 1
            h = [dot_loop(v[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = [wi - h[i] * vi for wi, vi in zip(w, v[i])]
            c = [0.0] * (j + 1)
            if fault != "one pass":
                c = [dot_loop(v[i], w) for i in range(j + 1)]
                for i in range(j + 1):
                    w = [wi - c[i] * vi for wi, vi in zip(w, v[i])]
            alpha = h[j] + c[j]
            T[j][j] = alpha
            beta = _sqrt(dot_loop(w, w))
            if not (math.isfinite(alpha) and math.isfinite(beta)):
                return [], [], [], NONFINITE, 0, it, cycles
            if beta == 0:
                cols, exact = j + 1, True
                break
            v.append([_div(wi, beta) for wi in w])
            if j + 1 < m:
                T[j][j + 1] = T[j + 1][j] = beta
            if it == maxiter:
                cols = j + 1
                break
        jac = jacobi_loop([row[:cols] for row in T[:cols]])
        if jac is None or not all(math.isfinite(a) for a in jac[0]):
            return [], [], [], NONFINITE, 0, it, cycles
        d, S = jac
        order = sorted(range(cols), key=(lambda i: d[i]) if which == lr.SMALLEST else (lambda i: -d[i]))   # (sorted is stable)
        theta = [d[i] for i in order]
        S = [[row[i] for i in order] for row in S]
        res = [0.0 if exact else abs(beta * S[cols - 1][i]) for i in range(cols)]
        scale = max(abs(a) for a in theta)
        found = min(nev, cols)
        done = cols >= nev and all(res[i] <= tol * scale for i in range(nev))
        if done or exact or it == maxiter:
            X = combine_loop(v[:cols], [row[:found] for row in S], desc)
            return theta[:found], res[:found], X, CONVERGED if done else BREAKDOWN if exact else MAXITER, found, it, cycles
        v[:kk] = combine_loop(v[:m], [row[:kk] for row in S], desc)
        v[kk] = v[m]
        T = [[0.0] * m for _ in range(m)]
        for i in range(kk):
            T[i][i] = theta[i]
            T[kk][i] = T[i][kk] = beta * S[m - 1][i]
        k = kk


def _case_ref(c, trace=None, stats=None, **kw):
    return lr.lanczos_ref(Csr(c.M, c.IRP, c.JA, c.AS), c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep, trace, stats, **kw)


def _same_result(ref, loop, what):
    theta, res, X, st, found, it, cyc = ref
    thl, resl, Xl, stl, foundl, itl, cycl = loop
    assert (st, found, it, cyc) == (stl, foundl, itl, cycl), what
    _same(theta, thl, what + ": theta")
    _same(res, resl, what + ": res")
    for i in range(found):
        _same(X[:, i], Xl[i], what + f": X[:, {i}]")


@pytest.mark.parametrize("name", exits.NAMES)
def test_exit_case_takes_its_label_and_ref_is_the_loop(name):
    c = exits.case(name)
    trace, stats = [], {}
    ref = _case_ref(c, trace, stats)
    theta, res, X, st, found, it, cyc = ref
    assert trace == [c.label] and c.label in lr.LANCZOS_EXITS, (name, trace)
    assert (st, found) == (c.status, c.found) and (c.cycles is None or cyc == c.cycles), (name, st, found, cyc)
    assert theta.shape == res.shape == (found,) and X.shape == (c.M, found)
    steps = stats["steps"]
    if c.how == "j0":
        assert steps == [1] and stats["exact"] and found == c.nev and np.all(res == 0) and not np.any(np.signbit(res))
    if c.how == "exact":
        assert stats["exact"] and found < c.nev
    if c.how == "mid":
        assert it == c.maxiter and steps[-1] < c.ncv - (0 if cyc == 1 else lr.default_keep(c.nev, c.ncv))
    if c.how == "end":
        assert it == c.maxiter and sum(steps) == it and steps[-1] == c.ncv - (0 if cyc == 1 else lr.default_keep(c.nev, c.ncv))
    if c.how == "first":
        assert cyc == 1 and st == CONVERGED
    if c.how == "restarts":
        assert cyc >= 3 and st == CONVERGED
    if c.how == "inf":
        assert not np.all(np.isfinite(c.AS)) and np.all(np.isfinite(c.v0))
    if name in exits.SMALL:
        loop = lanczos_loop(c.M, c.IRP, c.JA, c.AS, c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep)
        _same_result(ref, loop, name)


def test_exit_table_is_complete():
    """every label of the loop but the stated holes; every required way to reach one; both ends of the spectrum; keep at
    both of its bounds; the smallest legal basis; the unit-value handle"""
    rows = [exits.case(n) for n in exits.NAMES if n != "2I"] + [exits.case("2I")]
    for label in lr.LANCZOS_EXITS:
        assert any(r.label == label for r in rows) != (label in exits.HOLES), label
    assert set(exits.HOLES) <= set(lr.LANCZOS_EXITS)
    for label, how in exits.REQUIRED:
        assert any((r.label, r.how) == (label, how) for r in rows), (label, how)
    conv = [r for r in rows if r.label == "converged" and r.how == "restarts"]
    assert {r.which for r in conv} == {lr.LARGEST, lr.SMALLEST}
    assert any(r.keep == r.nev for r in conv) and any(r.keep == r.ncv - 1 for r in conv)
    assert any((r.nev, r.ncv) == (1, 2) for r in rows)
    assert any(np.all(r.AS == r.AS[0]) and r.M >= 4 * 4096 for r in rows)


@pytest.mark.parametrize("fault", ["one pass", "descending"])
def test_exit_table_tells_planted_faults_apart(fault):
    caught = []
    for name in exits.SMALL:
        c = exits.case(name)
        ref = _case_ref(c)
        loop = lanczos_loop(c.M, c.IRP, c.JA, c.AS, c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep, fault=fault)
        try:
            _same_result(ref, loop, name)
        except AssertionError:
            caught.append(name)
    print(fault, "caught by", caught)
    assert caught, fault


def test_one_pass_fault_is_the_reference_s_too():
    """lanczos_ref(one_pass=True) is the plain loop's planted fault: the two restatements agree on the fault as well"""
    c = exits.case("maxiter_mid")
    loop = lanczos_loop(c.M, c.IRP, c.JA, c.AS, c.v0, c.nev, c.ncv, c.which, c.tol, c.maxiter, c.keep, fault="one pass")
    _same_result(_case_ref(c, one_pass=True), loop, "one pass")


# ------------------------------------------------------------------------------------------------- the parts
def test_combine_ref_is_the_in_order_sum():
    rng = np.random.default_rng(7000)
    V, S = rng.standard_normal((37, 5)), rng.standard_normal((5, 3))
    V[3, 2], V[4, 1], S[0, 0] = -0.0, np.nan, -0.0
    Y = lr.combine_ref(V, S)
    Yl = combine_loop([V[:, j].tolist() for j in range(5)], S.tolist())
    for c in range(3):
        assert_same_bits(Y[:, c], np.array(Yl[c]), f"column {c}")
    assert np.isnan(Y[4]).all() and np.isfinite(np.delete(Y, 4, axis=0)).all(), "a NaN stays in its row"
    Z = lr.combine_ref(np.full((2, 3), -0.0), np.ones((3, 1)))
    assert not np.signbit(Z).any(), "sums start from +0.0"


@pytest.mark.parametrize("n", [1, 2, 7, 20])
def test_jacobi_ref_diagonalises(n):
    """S^T T S = diag(d) and S^T S = I to a few n eps |T|; d are the eigenvalues of T; the plain loop gives the same bits"""
    rng = np.random.default_rng(7100 + n)
    B = rng.standard_normal((n, n))
    T = B + B.T
    d, S, sweeps = lr.jacobi_ref(T)
    dl, Sl = jacobi_loop(T.tolist())
    assert_same_bits(d, np.array(dl), "d")
    assert_same_bits(S, np.array(Sl), "S")
    tol = 8 * n * 2.0 ** -52 * max(np.abs(T).sum(axis=1).max(), 1.0)
    assert np.abs(S.T @ T @ S - np.diag(d)).max() <= tol and np.abs(S.T @ S - np.eye(n)).max() <= 8 * n * 2.0 ** -52
    assert np.abs(np.sort(d) - np.linalg.eigvalsh(T)).max() <= tol and 1 <= sweeps <= 12


def test_default_keep_is_within_its_bounds():
    for m in range(2, lr.MAX_NCV + 1):
        for nev in range(1, m):
            assert nev <= lr.default_keep(nev, m) <= m - 1
    assert (lr.default_keep(1, 2), lr.default_keep(4, 20), lr.default_keep(8, 64)) == (1, 12, 36)


# ------------------------------------------------------------------------------------------------- properties
@pytest.fixture(scope="module")
def lap():
    nx, ny, nz = 12, 10, 8
    IRP, JA, AS = laplacian7(nx, ny, nz)
    n = nx * ny * nz
    D = np.zeros((n, n))
    D[np.repeat(np.arange(n), np.diff(IRP.astype(np.int64))), JA.astype(np.int64)] = AS
    return Csr(n, IRP, JA, AS), D, np.linalg.eigvalsh(D), np.random.default_rng(0).standard_normal(n)


@pytest.mark.parametrize("which", [lr.LARGEST, lr.SMALLEST])
def test_ref_finds_the_extreme_eigenpairs_of_the_laplacian(lap, which):
    A, D, ev, v0 = lap
    nev, m = 4, 20
    stats = {}
    theta, res, X, st, found, it, cyc = lr.lanczos_ref(A, v0, nev, m, which, 1e-8, 5000, stats=stats)
    assert (st, found) == (CONVERGED, nev)
    scale = stats["scale"]
    true = np.linalg.norm(D @ X - X * theta, axis=0)
    norms = np.linalg.norm(X, axis=0)
    gap = np.abs(true - res).max()
    orth = np.abs(X.T @ X - np.eye(nev)).max()
    print(f"which={which}: {it} matvecs, {cyc} cycles, {stats['sweeps']} sweeps at most; |res - true| {gap:.2e}, |X^T X - I| {orth:.2e}")
    for i in range(nev):                                 # a symmetric matrix has an eigenvalue within ||A x - theta x|| / ||x|| of theta
        assert np.abs(ev - theta[i]).min() <= 2 * true[i] / norms[i], i
    want = ev[::-1][:nev] if which == lr.LARGEST else ev[:nev]
    assert np.abs(theta - want).max() <= 1e-9 * scale
    assert gap <= RES_GAP and orth <= ORTH_GAP


def test_ref_res_and_orthogonality_over_the_converged_cases():
    worst_gap = worst_orth = 0.0
    for name in exits.NAMES:
        c = exits.case(name)
        if c.status != CONVERGED or name == "2I":
            continue
        theta, res, X, st, found, it, cyc = _case_ref(c)
        A = Csr(c.M, c.IRP, c.JA, c.AS)
        true = np.array([np.linalg.norm(A.spmv(X[:, i]) - theta[i] * X[:, i]) for i in range(found)])
        worst_gap = max(worst_gap, np.abs(true - res).max())
        worst_orth = max(worst_orth, np.abs(X.T @ X - np.eye(found)).max())
    print(f"converged cases of the table: |res - true| {worst_gap:.2e}, |X^T X - I| {worst_orth:.2e}")
    assert worst_gap <= RES_GAP and worst_orth <= ORTH_GAP
