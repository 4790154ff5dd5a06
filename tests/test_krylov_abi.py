"""The Krylov entry points (spmvHipDot, hipSpCGCSR, hipSpBiCGStabCSR) are declared, exported and bound in Python with the
C layouts of spmvKrylovOpts and spmvKrylovInfo, and the test side's references (tests/krylov_ref.py) are the loops of
include/spmvHip.h: dot_ref is the documented order (which np.dot and math.fsum are not), cg_ref and bicgstab_ref equal
the loops written in plain Python on tiny systems, and every case of tests/krylov_exit_inputs.py takes the exit of the
loop that the table claims for it (so the table reaches every `return` of both loops).  No GPU needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits
from c_header import HEADER, code as _code
from conftest import ROOT
from ilu0_ref import ilu0_levels, ilu0_loop
import krylov_exit_inputs as exits
from krylov_ref import BICGSTAB_EXITS, BREAKDOWN, CG_EXITS, CONVERGED, MAXITER, NONFINITE, Csr, bicgstab_ref, cg_ref, dot_ref
from test_trsv_abi import laplacian7
from trsv_ref import trsv_loop

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
_SOLVER = r"spmat\s*\*\s*\w+\s*,\s*spmat\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*" \
          r"const\s+spmvKrylovOpts\s*\*\s*\w+\s*,\s*spmvKrylovInfo\s*\*\s*\w+"
DECLS = {
    "spmvHipDot": r"size_t\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+",
    "hipSpCGCSR": _SOLVER,
    "hipSpBiCGStabCSR": _SOLVER,
}
OPTS = ("tol", "maxIter", "history")
INFO = ("status", "iterations", "rr", "bb", "launches", "hostChecks", "ms")


def test_header_declares_the_three_and_the_structs():
    code = _code(HEADER)
    for name, params in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in (("spmvKrylovOpts", OPTS), ("spmvKrylovInfo", INFO)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body, struct
        assert re.findall(r"(\w+)\s*;", body.group(1)) == list(fields), struct
    for name, value in (("CONVERGED", 0), ("MAXITER", 1), ("BREAKDOWN", 2), ("NONFINITE", 3)):
        assert re.search(r"#define\s+SPMV_KRYLOV_" + name + r"\s+" + str(value) + r"\b", code), name


def test_library_exports_the_three():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_three():
    from spmv_openmp_cuda_amd import api
    for name, n in (("spmvHipDot", 4), ("hipSpCGCSR", 6), ("hipSpBiCGStabCSR", 6)):
        assert name in api._sigs
        assert len(getattr(api.lib, name).argtypes) == n, name
    for m in ("cg", "bicgstab"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert callable(api.dot)
    assert [f[0] for f in api.spmvKrylovOpts._fields_] == list(OPTS)
    assert [f[0] for f in api.spmvKrylovInfo._fields_] == list(INFO)
    assert (api.SPMV_KRYLOV_CONVERGED, api.SPMV_KRYLOV_MAXITER, api.SPMV_KRYLOV_BREAKDOWN, api.SPMV_KRYLOV_NONFINITE) == \
        (CONVERGED, MAXITER, BREAKDOWN, NONFINITE)


# ------------------------------------------------------------------------------------------------- the dot product
def dot_loop(u, v):
    """the order of include/spmvHip.h, one product and one add at a time"""
    u, v = [float(a) for a in u], [float(a) for a in v]
    n = len(u)

    def tree(a):
        h = 128
        while h >= 1:
            for t in range(h):
                a[t] = a[t] + a[t + h]
            h //= 2
        return a[0]

    parts = []
    for c in range(-(-n // 4096)):
        lanes = []
        for t in range(256):
            acc = 0.0
            for s in range(8):
                for e in (0, 1):
                    i = 4096 * c + 512 * s + 2 * t + e
                    acc += u[i] * v[i] if i < n else 0.0
            lanes.append(acc)
        parts.append(tree(lanes))
    if not parts:
        return 0.0
    lanes = []
    for t in range(256):
        acc = 0.0
        for i in range(t, len(parts), 256):
            acc += parts[i]
        lanes.append(acc)
    return tree(lanes)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 4095, 4096, 4097, 3 * 4096 + 5])
def test_dot_ref_is_the_documented_order(n):
    rng = np.random.default_rng(2000 + n)
    u, v = si.order_values(rng, n, 8), si.order_values(rng, n, 8)
    assert_same_bits(np.array([dot_ref(u, v)]), np.array([dot_loop(u, v)]), f"n={n}")


def test_dot_ref_many_blocks():
    """more than 256 block partials: the second stage's lanes each add several"""
    rng = np.random.default_rng(2010)
    n = 300 * 4096 + 77
    u, v = si.order_values(rng, n, 8), si.order_values(rng, n, 8)
    d = dot_ref(u, v)
    parts = np.array([dot_ref(u[c * 4096:(c + 1) * 4096], v[c * 4096:(c + 1) * 4096]) for c in range(-(-n // 4096))])
    lanes = [0.0] * 256
    for t in range(256):
        for i in range(t, parts.size, 256):
            lanes[t] += parts[i]
    h = 128
    while h >= 1:
        for t in range(h):
            lanes[t] = lanes[t] + lanes[t + h]
        h //= 2
    assert_same_bits(np.array([d]), np.array([lanes[0]]), "two stages")


def test_dot_order_is_pinned():
    """on cancelling inputs another order gives other bits: np.dot and the exactly rounded sum both differ"""
    rng = np.random.default_rng(2020)
    n = 3 * 4096 + 5
    u, v = si.order_values(rng, n, 12), si.order_values(rng, n, 12)
    d = dot_ref(u, v)
    assert d != np.dot(u, v)
    assert d != math.fsum((u * v).tolist())
    assert d == dot_loop(u, v)


def test_dot_ref_zeros_and_specials():
    """-0.0 products give +0.0 (every partial starts at +0.0); NaN and Inf propagate"""
    assert np.signbit(dot_ref(np.array([-0.0, -0.0]), np.array([1.0, 1.0]))) == False  # noqa: E712
    assert np.isnan(dot_ref(np.array([np.inf, 1.0]), np.array([0.0, 1.0])))
    assert dot_ref(np.array([np.inf, 1.0]), np.array([1.0, 1.0])) == np.inf


# ------------------------------------------------------------------------------------------------- the solvers
def _dense(M, IRP, JA, AS):
    IRP, JA = IRP.astype(np.int64), JA.astype(np.int64)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    return [[(rows[p], JA[p], float(AS[p])) for p in range(IRP[i], IRP[i + 1])] for i in range(M)]


def _ops(M, IRP, JA, AS, F):
    """plain-Python SpMV (stored order) and M^-1 (trsv_loop) for the loops below"""
    rows = _dense(M, IRP, JA, AS)

    def spmv(x):
        y = []
        for row in rows:
            acc = 0.0
            for _, j, a in row:
                acc += a * x[j]
            y.append(acc)
        return y

    def precond(v):
        if F is None:
            return list(v)
        w = trsv_loop(M, IRP, JA, F, v, True, True)
        return [float(a) for a in trsv_loop(M, IRP, JA, F, w, False, False)]
    return spmv, precond


def _div(a, b):
    """a / b as IEEE double gives it (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def cg_loop(M, IRP, JA, AS, F, b, x, tol, maxiter):
    spmv, precond = _ops(M, IRP, JA, AS, F)
    x, b = [float(a) for a in x], [float(a) for a in b]
    q = spmv(x)
    r = [bi - qi for bi, qi in zip(b, q)]
    rr, bb = dot_loop(r, r), dot_loop(b, b)
    thresh = (tol * tol) * bb
    hist = [rr]
    if rr <= thresh:
        return x, CONVERGED, 0, hist
    if not math.isfinite(rr):
        return x, NONFINITE, 0, hist
    if maxiter == 0:
        return x, MAXITER, 0, hist
    z = precond(r)
    rz = dot_loop(r, z) if F is not None else rr
    p = list(z)
    for k in range(1, maxiter + 1):
        q = spmv(p)
        pq = dot_loop(p, q)
        if pq == 0:
            return x, BREAKDOWN, k - 1, hist
        alpha = _div(rz, pq)
        x = [xi + alpha * pi for xi, pi in zip(x, p)]
        r = [ri - alpha * qi for ri, qi in zip(r, q)]
        rr = dot_loop(r, r)
        hist.append(rr)
        if rr <= thresh:
            return x, CONVERGED, k, hist
        if not math.isfinite(rr):
            return x, NONFINITE, k, hist
        if k == maxiter:
            return x, MAXITER, k, hist
        z = precond(r)
        rzn = dot_loop(r, z)
        beta = _div(rzn, rz)
        rz = rzn
        p = [zi + beta * pi for zi, pi in zip(z, p)]


def bicgstab_loop(M, IRP, JA, AS, F, b, x, tol, maxiter, fault=None):
    """`fault` plants one of the mistakes the exit table must tell apart (test_exit_table_tells_planted_faults_apart):
    "half x": a half-step exit returns x without alpha * phat; "omega rho": the omega == 0 and rho == 0 tests swapped"""
    spmv, precond = _ops(M, IRP, JA, AS, F)
    x, b = [float(a) for a in x], [float(a) for a in b]
    q = spmv(x)
    r = [bi - qi for bi, qi in zip(b, q)]
    rr, bb = dot_loop(r, r), dot_loop(b, b)
    thresh = (tol * tol) * bb
    hist = [rr]
    if rr <= thresh:
        return x, CONVERGED, 0, hist
    if not math.isfinite(rr):
        return x, NONFINITE, 0, hist
    if maxiter == 0:
        return x, MAXITER, 0, hist
    rhat = list(r)
    rho, rho_old, alpha, omega = rr, 1.0, 1.0, 1.0
    p = v = beta = None
    for k in range(1, maxiter + 1):
        if k == 1:
            p = list(r)
        else:
            p = [ri + beta * (pi - omega * vi) for ri, pi, vi in zip(r, p, v)]
        phat = precond(p)
        v = spmv(phat)
        rv = dot_loop(rhat, v)
        if rv == 0:
            return x, BREAKDOWN, k - 1, hist
        alpha = _div(rho, rv)
        s = [ri - alpha * vi for ri, vi in zip(r, v)]
        ss = dot_loop(s, s)
        hist.append(ss)
        if ss <= thresh:
            if fault == "half x":
                return x, CONVERGED, k, hist
            return [xi + alpha * hi for xi, hi in zip(x, phat)], CONVERGED, k, hist
        shat = precond(s)
        t = spmv(shat)
        tt, ts = dot_loop(t, t), dot_loop(t, s)
        if tt == 0:
            return [xi + alpha * hi for xi, hi in zip(x, phat)], BREAKDOWN, k, hist
        omega = _div(ts, tt)
        x = [(xi + alpha * hi) + omega * si_ for xi, hi, si_ in zip(x, phat, shat)]
        r = [si_ - omega * ti for si_, ti in zip(s, t)]
        rr = dot_loop(r, r)
        hist[k] = rr
        rhon = dot_loop(rhat, r)
        if rr <= thresh:
            return x, CONVERGED, k, hist
        if not math.isfinite(rr):
            return x, NONFINITE, k, hist
        if (rhon if fault == "omega rho" else omega) == 0:
            return x, BREAKDOWN, k, hist
        if k == maxiter:
            return x, MAXITER, k, hist
        rho_old, rho = rho, rhon
        if (omega if fault == "omega rho" else rho) == 0:
            return x, BREAKDOWN, k, hist
        beta = _div(rho, rho_old) * _div(alpha, omega)


def convdiff7(nx, ny, nz, c=0.7):
    """a nonsymmetric 7-point upwind convection-diffusion stencil (flow along +x, +y, +z): the upwind neighbour -1 - c,
    the others -1, the diagonal 6 + 3c; columns sorted"""
    M = nx * ny * nz
    i = np.arange(M)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    rows, cols, vals = [i], [i], [np.full(M, 6.0 + 3 * c)]
    for ok, off, v in ((z > 0, -nx * ny, -1.0 - c), (y > 0, -nx, -1.0 - c), (x > 0, -1, -1.0 - c),
                       (x < nx - 1, 1, -1.0), (y < ny - 1, nx, -1.0), (z < nz - 1, nx * ny, -1.0)):
        rows.append(i[ok])
        cols.append(i[ok] + off)
        vals.append(np.full(int(ok.sum()), v))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.lexsort((cols, rows))
    return si.assemble(M, rows[o], cols[o], vals[o])


def _check_solver(ref, loop, M, IRP, JA, AS, precond, b, x0, tol, maxiter, what):
    F = ilu0_loop(M, IRP, JA, AS) if precond else None
    x, st, it, hist, rr = ref(Csr(M, IRP, JA, AS, F), b, x0, tol, maxiter)
    xl, stl, itl, histl = loop(M, IRP, JA, AS, F, b, x0, tol, maxiter)
    assert (st, it) == (stl, itl), what
    assert_same_bits(x, np.array(xl), what + ": x")
    assert_same_bits(hist, np.array(histl), what + ": history")
    assert_same_bits(np.array([rr]), np.array([histl[-1]]), what + ": rr")
    return st, it


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("maxiter", [0, 3, 200])
def test_cg_ref_is_the_loop(precond, maxiter):
    IRP, JA, AS = laplacian7(5, 4, 3)
    M = 60
    rng = np.random.default_rng(2030)
    st, it = _check_solver(cg_ref, cg_loop, M, IRP, JA, AS, precond, si.order_values(rng, M), si.order_values(rng, M),
                           1e-10, maxiter, f"cg precond={precond} maxiter={maxiter}")
    assert st == (CONVERGED if maxiter == 200 else MAXITER) and it <= max(maxiter, 1) * 200


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("maxiter", [0, 3, 200])
def test_bicgstab_ref_is_the_loop(precond, maxiter):
    IRP, JA, AS = convdiff7(5, 4, 3)
    M = 60
    rng = np.random.default_rng(2040)
    st, _ = _check_solver(bicgstab_ref, bicgstab_loop, M, IRP, JA, AS, precond, si.order_values(rng, M), np.zeros(M),
                          1e-10, maxiter, f"bicgstab precond={precond} maxiter={maxiter}")
    assert st == (CONVERGED if maxiter == 200 else MAXITER)


def test_refs_edge_cases_are_the_loops():
    """b = 0 (0 iterations), a breakdown (a zero matrix row makes p^T A p = 0), a NaN value"""
    IRP, JA, AS = laplacian7(4, 3, 2)
    M = 24
    b = np.ones(M)
    for ref, loop in ((cg_ref, cg_loop), (bicgstab_ref, bicgstab_loop)):
        assert _check_solver(ref, loop, M, IRP, JA, AS, False, np.zeros(M), np.zeros(M), 1e-8, 50, "b = 0") == (CONVERGED, 0)
        bad = AS.copy()
        bad[3] = np.nan
        assert _check_solver(ref, loop, M, IRP, JA, bad, False, b, np.zeros(M), 1e-8, 50, "NaN")[0] == NONFINITE
    e0 = np.zeros(M)
    e0[0] = 1.0
    z = np.zeros_like(AS)
    assert _check_solver(cg_ref, cg_loop, M, IRP, JA, z, False, e0, np.zeros(M), 1e-8, 50, "A = 0") == (BREAKDOWN, 0)
    assert _check_solver(bicgstab_ref, bicgstab_loop, M, IRP, JA, z, False, e0, np.zeros(M), 1e-8, 50, "A = 0") == (BREAKDOWN, 0)


def test_ilu0_pcg_needs_fewer_iterations():
    n = 16
    IRP, JA, AS = laplacian7(n, n, n)
    M = n ** 3
    b = np.random.default_rng(2050).random(M)
    F = ilu0_levels(M, IRP, JA, AS)
    _, st0, it_plain, _, _ = cg_ref(Csr(M, IRP, JA, AS), b, np.zeros(M), 1e-8, 1000)
    _, st1, it_ilu, _, _ = cg_ref(Csr(M, IRP, JA, AS, F), b, np.zeros(M), 1e-8, 1000)
    assert st0 == st1 == CONVERGED
    assert it_ilu <= 0.75 * it_plain, (it_ilu, it_plain)


# ------------------------------------------------------------------------------------------------- every exit
def _same(a, b, what):
    """NaN where NaN is, and everything else (the infinities too) by its bits"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what + ": NaN in other places"
    assert_same_bits(a[~np.isnan(a)], b[~np.isnan(b)], what)


def _case_ref(c, trace=None):
    with np.errstate(all="ignore"):
        F = ilu0_levels(c.M, c.IRP, c.JA, c.AS) if c.precond else None
    ref = cg_ref if c.solver == "cg" else bicgstab_ref
    return F, ref(Csr(c.M, c.IRP, c.JA, c.AS, F), c.b, c.x0, c.tol, c.maxiter, trace)


@pytest.mark.parametrize("name", exits.NAMES)
def test_exit_case_takes_its_label_and_ref_is_the_loop(name):
    """the labelled reference leaves by the line the table names, early (iteration <= 1) or late as it says, and on the
    small cases the plain-Python loop gives the same bits"""
    c = exits.case(name)
    trace = []
    F, (x, st, it, hist, rr) = _case_ref(c, trace)
    assert trace == [c.label], (name, trace)
    assert (it >= 2) == (c.when == "late"), (name, it)
    assert c.label in (CG_EXITS if c.solver == "cg" else BICGSTAB_EXITS)
    if name.endswith(":large"):
        assert c.JA.size >= exits.AUTO_MIN_NNZ and c.M > 8 * 4096 and c.x0.any()
        return                                                           # (the twin adds nothing to reference = loop)
    loop = cg_loop if c.solver == "cg" else bicgstab_loop
    xl, stl, itl, histl = loop(c.M, c.IRP, c.JA, c.AS, F, c.b, c.x0, c.tol, c.maxiter)
    assert (st, it) == (stl, itl), name
    _same(x, xl, name + ": x")
    _same(hist, histl, name + ": history")
    _same(np.array([rr]), [histl[-1]], name + ": rr")


def test_exit_table_is_complete():
    """every label of both loops, with and without ILU(0); `early` and `late` where both are asked for; a large twin for
    the labels that must have one; no hole but the documented ones"""
    have = {}
    for name in exits.NAMES:
        solver, label, when = name.split(":")[:3]
        have.setdefault((solver.split("+")[0], "+ilu0" in solver, label), set()).add((when, name.endswith(":large")))
    want = set()
    for solver, labels in (("cg", CG_EXITS), ("bicgstab", BICGSTAB_EXITS)):
        for pre in (False, True):
            for label in labels:
                whens = ("early", "late") if label in exits.BOTH_WHENS else (None,)
                for when in whens:
                    got = {w for w, _ in have.get((solver, pre, label), ())}
                    hole = (solver, pre, label, when) in exits.HOLES
                    assert hole != (bool(got) if when is None else when in got), (solver, pre, label, when)
                    want.add((solver, pre, label))
    assert set(have) | {k[:3] for k in exits.HOLES} == want
    assert not any(pre is False for _, pre, _, _ in exits.HOLES), "the un-preconditioned table has no holes"
    for label in exits.LARGE_REQUIRED:
        assert any(large for _, large in have[("bicgstab", False, label)]), label
    assert any(large for _, large in have[("cg", False, "converged")])


@pytest.mark.parametrize("fault", ["half x", "omega rho"])
def test_exit_table_tells_planted_faults_apart(fault):
    """a loop that forgets x + alpha * phat at a half-step exit, or tests rho == 0 where omega == 0 belongs, differs from
    the reference on a case of the table (status, iterations or the bits of x)"""
    caught = []
    for name in exits.NAMES:
        if not name.startswith("bicgstab") or name.endswith(":large"):
            continue
        c = exits.case(name)
        F, (x, st, it, _, _) = _case_ref(c)
        xl, stl, itl, _ = bicgstab_loop(c.M, c.IRP, c.JA, c.AS, F, c.b, c.x0, c.tol, c.maxiter, fault=fault)
        try:
            assert (st, it) == (stl, itl)
            _same(x, xl, name)
        except AssertionError:
            caught.append(name)
    print(fault, "caught by", caught)
    assert caught, fault
    if fault == "half x":
        assert all(":half_converged:" in n or ":tt0:" in n for n in caught)
