"""spmvHipMultiDot and hipSpGMRESCSR are declared, exported and bound in Python with the C layout of spmvGmresOpts, and
the test side's reference (tests/gmres_ref.py) is the loop of include/spmvHip.h: gmres_ref equals the loop written in
plain Python (math.sqrt, float) on every small case of tests/gmres_exit_inputs.py, every case of that table takes the
exit and the cycle end the table claims for it, the table is complete, and two planted faults each change a case.
No GPU needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import gmres_exit_inputs as exits
import serial_order_inputs as si
from bits import assert_same_bits
from c_header import HEADER, code as _code
from conftest import ROOT
from gmres_ref import CYCLE_ENDS, GMRES_EXITS, gmres_ref, multi_dot_ref
from ilu0_ref import ilu0_levels, ilu0_loop
from krylov_ref import BREAKDOWN, CONVERGED, MAXITER, NONFINITE, Csr, dot_ref
from test_krylov_abi import _div, _ops, _same, convdiff7, dot_loop

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
DECLS = {
    "spmvHipMultiDot": r"size_t\s+\w+\s*,\s*unsigned\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*"
                       r"const\s+double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+",
    "hipSpGMRESCSR": r"spmat\s*\*\s*\w+\s*,\s*spmat\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*"
                     r"const\s+spmvGmresOpts\s*\*\s*\w+\s*,\s*spmvKrylovInfo\s*\*\s*\w+",
}
OPTS = ("tol", "maxIter", "restart", "history")


def test_header_declares_the_two_and_the_struct():
    code = _code(HEADER)
    for name, params in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spmvGmresOpts\s*;", code, re.S)
    assert body and re.findall(r"(\w+)\s*;", body.group(1)) == list(OPTS)


def test_library_exports_the_two():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_two():
    from spmv_openmp_cuda_amd import api
    for name in DECLS:
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == 6, name
    assert callable(api.DeviceMatrix.gmres) and callable(api.multi_dot)
    assert [f[0] for f in api.spmvGmresOpts._fields_] == list(OPTS)


def test_multi_dot_ref_is_k_dots():
    rng = np.random.default_rng(6000)
    n, k = 4097, 5
    V, w = si.order_values(rng, n * k, 8).reshape(k, n).T, si.order_values(rng, n, 8)
    h = multi_dot_ref(V, w)
    assert h.shape == (k,)
    assert_same_bits(h, np.array([dot_ref(V[:, i], w) for i in range(k)]), "k dots")
    assert_same_bits(h[:2], np.array([dot_loop(V[:, i], w) for i in range(2)]), "the documented order")


# ------------------------------------------------------------------------------------------------- the loop, restated
def _sqrt(a):
    return math.sqrt(a) if a >= 0 else float("nan")                     # (NaN passes through math.sqrt; a negative raises)


def gmres_loop(M, IRP, JA, AS, F, b, x, tol, maxiter, restart, fault=None):
    """the loop of include/spmvHip.h on Python floats.  `fault` plants one of the mistakes the exit table must tell apart:
    "sn sign": the Givens rotation applied with sn's sign flipped; "est converged": CONVERGED declared on the estimate"""
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
    m, k = restart, 0
    flip = -1.0 if fault == "sn sign" else 1.0
    while True:
        beta = _sqrt(rr)
        v = [[_div(ri, beta) for ri in r]]
        g = [0.0] * (m + 1)
        g[0] = beta
        cs, sn = [0.0] * m, [0.0] * m
        R = [[0.0] * m for _ in range(m)]
        brk, cols, est_hit = False, None, False
        for j in range(m):
            w = spmv(precond(v[j]))
            h = [dot_loop(v[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = [wi - h[i] * vi for wi, vi in zip(w, v[i])]
            c = [dot_loop(v[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = [wi - c[i] * vi for wi, vi in zip(w, v[i])]
            h = [hi + ci for hi, ci in zip(h, c)]
            hn = _sqrt(dot_loop(w, w))
            for i in range(j):
                t = cs[i] * h[i] + (flip * sn[i]) * h[i + 1]
                h[i + 1] = cs[i] * h[i + 1] - (flip * sn[i]) * h[i]
                h[i] = t
            d = _sqrt(h[j] * h[j] + hn * hn)
            if d == 0:
                if j == 0:
                    return x, BREAKDOWN, k, hist
                brk, cols = True, j
                break
            k += 1
            cs[j], sn[j] = _div(h[j], d), _div(hn, d)
            h[j] = d
            for i in range(j + 1):
                R[i][j] = h[i]
            g[j + 1] = -(sn[j] * g[j])
            g[j] = cs[j] * g[j]
            est = g[j + 1] * g[j + 1]
            hist.append(est)
            if est <= thresh or not math.isfinite(est) or hn == 0 or j == m - 1 or k == maxiter:
                brk, cols, est_hit = hn == 0, j + 1, est <= thresh
                break
            v.append([_div(wi, hn) for wi in w])
        y = [0.0] * cols
        for i in range(cols - 1, -1, -1):
            s = g[i]
            for l in range(i + 1, cols):
                s = s - R[i][l] * y[l]
            y[i] = _div(s, R[i][i])
        u = [y[0] * vi for vi in v[0]]
        for i in range(1, cols):
            u = [ui + y[i] * vi for ui, vi in zip(u, v[i])]
        x = [xi + zi for xi, zi in zip(x, precond(u))]
        q = spmv(x)
        r = [bi - qi for bi, qi in zip(b, q)]
        rr = dot_loop(r, r)
        hist[k] = rr
        if rr <= thresh or (fault == "est converged" and est_hit):
            return x, CONVERGED, k, hist
        if not math.isfinite(rr):
            return x, NONFINITE, k, hist
        if brk:
            return x, BREAKDOWN, k, hist
        if k == maxiter:
            return x, MAXITER, k, hist


def _case_ref(c, trace=None, stats=None):
    with np.errstate(all="ignore"):
        F = ilu0_levels(c.M, c.IRP, c.JA, c.AS) if c.precond else None
        return F, gmres_ref(Csr(c.M, c.IRP, c.JA, c.AS, F), c.b, c.x0, c.tol, c.maxiter, c.restart, trace, stats)


@pytest.mark.parametrize("name", exits.NAMES)
def test_exit_case_takes_its_label_and_ref_is_the_loop(name):
    c = exits.case(name)
    trace, stats = [], {}
    F, (x, st, it, hist, rr) = _case_ref(c, trace, stats)
    assert trace == [c.label] and c.label in GMRES_EXITS, (name, trace)
    assert (stats["ends"][-1] if stats["ends"] else "") == c.ends, (name, stats)
    assert all(e == "d0" or set(e.split("+")) <= set(CYCLE_ENDS) for e in stats["ends"])
    assert stats["cycles"] == c.cycles and (it >= 2) == (c.when == "late"), (name, stats, it)
    assert st == {"init_converged": CONVERGED, "init_nonfinite": NONFINITE, "init_maxiter": MAXITER, "d0_cols0": BREAKDOWN,
                  "converged": CONVERGED, "nonfinite": NONFINITE, "breakdown": BREAKDOWN, "maxiter": MAXITER}[c.label]
    assert hist.size == it + 1
    if name.endswith(":large"):
        assert c.JA.size >= exits.AUTO_MIN_NNZ and c.M > 8 * 4096 and c.x0.any()
        return
    if c.M > 600:
        return                                                           # (2 I: the plain loop adds nothing)
    xl, stl, itl, histl = gmres_loop(c.M, c.IRP, c.JA, c.AS, F, c.b, c.x0, c.tol, c.maxiter, c.restart)
    assert (st, it) == (stl, itl), name
    _same(x, xl, name + ": x")
    _same(hist, histl, name + ": history")


def test_exit_table_is_complete():
    """every label, without and with ILU(0); every required way to end the last cycle; early and late where asked; a
    cycle that ended on the estimate and was followed by another; restart = 1 and restart = 64 > n; large twins"""
    rows = [n.split(":") for n in exits.NAMES]
    for pre in (False, True):
        mine = [r for r in rows if (r[0] == "gmres+ilu0") == pre]
        for label in GMRES_EXITS:
            assert any(r[1] == label for r in mine) != ((pre, label, None) in exits.HOLES), (pre, label)
        for label, cond in exits.REQUIRED:
            assert any(r[1] == label and cond in r[2].split("+") for r in mine) != ((pre, label, cond) in exits.HOLES), (pre, label, cond)
        for label in exits.BOTH_WHENS:
            assert {r[3] for r in mine if r[1] == label} == {"early", "late"}, (pre, label)
        assert any(r[1] == "maxiter" and r[2] == "est+maxiter" and r[4] == "c2" for r in mine), "est, true rr above, another cycle"
        assert any(r[6] == "m1" for r in mine) and any(r[6] == "m64" for r in mine)
        assert any(r[-1] == "large" for r in mine)
    assert not exits.HOLES
    for label in ("converged", "breakdown", "maxiter", "d0_cols0"):
        assert any(r[1] == label and r[-1] == "large" for r in rows), label


@pytest.mark.parametrize("fault", ["sn sign", "est converged"])
def test_exit_table_tells_planted_faults_apart(fault):
    caught = []
    for name in exits.NAMES:
        c = exits.case(name)
        if name.endswith(":large") or c.M > 600:
            continue
        F, (x, st, it, _, _) = _case_ref(c)
        xl, stl, itl, _ = gmres_loop(c.M, c.IRP, c.JA, c.AS, F, c.b, c.x0, c.tol, c.maxiter, c.restart, fault=fault)
        try:
            assert (st, it) == (stl, itl)
            _same(x, xl, name)
        except AssertionError:
            caught.append(name)
    print(fault, "caught by", caught)
    assert caught, fault


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("restart", [1, 5, 30])
def test_gmres_ref_solves_convection_diffusion(precond, restart):
    """6^3 upwind convection-diffusion at tol = 1e-10: the loop ends CONVERGED on the true residual, which in long double
    is within 2e-10 of b (1e-10 and the rounding of r = b - A x in double); the history does not grow inside a cycle"""
    IRP, JA, AS = convdiff7(6, 6, 6)
    M = 216
    b = np.random.default_rng(6100).random(M)
    F = ilu0_loop(M, IRP, JA, AS) if precond else None
    stats = {}
    x, st, it, hist, rr = gmres_ref(Csr(M, IRP, JA, AS, F), b, np.zeros(M), 1e-10, 2000, restart, None, stats)
    assert st == CONVERGED and hist.size == it + 1
    rows = si.row_of_entry(IRP)
    res = b.astype(np.longdouble)
    np.subtract.at(res, rows, AS.astype(np.longdouble) * x.astype(np.longdouble)[JA.astype(np.int64)])
    ratio = float(np.sqrt(np.sum(res * res)) / np.sqrt(np.sum(b.astype(np.longdouble) ** 2)))
    print(f"precond={precond} restart={restart}: iterations {it}, cycles {stats['cycles']}, |b - A x| / |b| = {ratio:.3e}")
    assert ratio <= 2e-10
    eps = 2.0 ** -52
    for cyc in range(stats["cycles"]):                                   # cycle `cyc`: hist[cyc*restart] is a true rr (or rr0),
        lo, hi = cyc * restart, min((cyc + 1) * restart, it)             # then estimates; hist[hi] is the next true rr
        est = hist[lo + 1:hi]
        assert np.all(np.diff(est) <= 0), (cyc, est)                     # |sn| <= 1, and rounding is monotone
        if est.size:
            assert est[0] <= hist[lo] * (1 + 4 * eps), (cyc, hist[lo], est[0])   # g[0]^2 = fl(sqrt(rr))^2 <= rr (1 + 2 eps)^2
