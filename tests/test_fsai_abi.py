"""The approximate-inverse entry points (spmvHipFsaiSetup, ...Refresh, ...Apply, ...Transpose, ...Info) are declared, exported
and bound in Python with the C layout of spmvFsaiOpts / spmvFsaiInfo, and the test side's references (tests/fsai_ref.py) agree
bit for bit -- on inputs where another update order gives other bits -- and compute what FSAI is: every row solves its dense
system, and G A G^T has a unit diagonal.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import fsai_ref as fr
import serial_order_inputs as si
from bits import assert_same_bits, differing_rows
from c_header import HEADER, code as _code
from conftest import ROOT
from spgemm_ref import laplacian7

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
H, I, O = r"spmat\s*\*\s*\w+", r"spmvFsaiInfo\s*\*\s*\w+", r"const\s+spmvFsaiOpts\s*\*\s*\w+"
DECLS = {
    "spmvHipFsaiSetup": (rf"{H}\s*,\s*{H}\s*,\s*{O}\s*,\s*{H}\s*,\s*{I}", 5),
    "spmvHipFsaiRefresh": (rf"{H}\s*,\s*{H}\s*,\s*{I}", 3),
    "spmvHipFsaiApply": (rf"{H}\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+", 3),
    "spmvHipFsaiTranspose": (rf"{H}\s*,\s*{H}", 2),
    "spmvHipFsaiInfo": (rf"{H}\s*,\s*{I}", 2),
}
INFO_FIELDS = ("nnz", "maxRow", "badRows", "firstBadRow", "launches", "setups", "ms")
OPTS_FIELDS = ("lanesPerRow",)


def test_header_declares_the_five_and_both_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in (("spmvFsaiInfo", INFO_FIELDS), ("spmvFsaiOpts", OPTS_FIELDS)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body, struct
        assert re.findall(r"(\w+)\s*;", body.group(1)) == list(fields)
    assert re.search(r"^\s*#\s*define\s+SPMV_FSAI_MAX_ROW\s+64\b", code, re.M)


def test_library_exports_the_five():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_five():
    from spmv_openmp_cuda_amd import api
    for name, (_, n) in DECLS.items():
        assert name in api._sigs
        assert len(getattr(api.lib, name).argtypes) == n, name
    assert callable(api.DeviceMatrix.fsai) and issubclass(api.Fsai, api.DeviceMatrix)
    for m in ("apply", "refresh_from", "transposed", "info"):
        assert callable(getattr(api.Fsai, m)), m
    assert [f[0] for f in api.spmvFsaiInfo._fields_] == list(INFO_FIELDS)
    assert [f[0] for f in api.spmvFsaiOpts._fields_] == list(OPTS_FIELDS)
    assert api.SPMV_FSAI_MAX_ROW == fr.MAX_ROW == 64


# ------------------------------------------------------------------------------------------------------------- the inputs
def random_spd(rng, M, per_row, e=2, spread=None):
    """a symmetric matrix with strictly ascending rows: up to per_row random off-diagonal pairs a row with order-sensitive
    values, and a random diagonal 1.5 to 2.5 times the row's absolute off-diagonal sum (diagonally dominant: D^-1/2 A D^-1/2
    has its eigenvalues in [1/3, 5/3], every principal block a condition of at most 5).  spread: the half-width of the band
    the columns come from (None: anywhere)"""
    rows = np.repeat(np.arange(M), rng.integers(0, per_row + 1, M))
    if spread is None:
        cols = rng.integers(0, max(M, 1), rows.size)
    else:
        cols = np.clip(rows + rng.integers(-spread, spread + 1, rows.size), 0, M - 1)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    key = np.unique((lo * M + hi)[lo != hi])
    lo, hi = key // max(M, 1), key % max(M, 1)
    v = si.order_values(rng, lo.size, e)
    off = np.bincount(lo, np.abs(v), M) + np.bincount(hi, np.abs(v), M)
    d = (1.5 + rng.random(M)) * np.where(off > 0, off, 1.0)
    i = np.arange(M)
    r, c, a = np.concatenate([lo, hi, i]), np.concatenate([hi, lo, i]), np.concatenate([v, v, d])
    o = np.lexsort((c, r))
    return (M, M) + si.assemble(M, r[o], c[o], a[o])


def stencil(rng, nx, ny, nz):
    """the 7-point pattern with symmetric order-sensitive off-diagonals and a dominant random diagonal"""
    M, _, IRP, JA, AS = laplacian7(nx, ny, nz)
    rows, cols = si.row_of_entry(IRP), JA.astype(np.int64)
    pair = np.minimum(rows, cols) * M + np.maximum(rows, cols)
    _, inv = np.unique(pair, return_inverse=True)
    v = (si.order_values(rng, int(inv.max()) + 1, 1) / 7)[inv]
    off = np.bincount(rows[rows != cols], np.abs(v[rows != cols]), M)
    AS = np.where(rows == cols, ((1.5 + rng.random(M)) * np.where(off > 0, off, 1.0))[rows], v)
    return M, M, IRP, JA, AS


def tril_of(A, k=0):
    M, N, IRP, JA, AS = A
    rows = si.row_of_entry(IRP)
    keep = JA.astype(np.int64) - rows <= k
    return (M, N) + si.assemble(M, rows[keep], JA[keep].astype(np.int64), AS[keep])


def dense_rows(rng, M, width):
    """a pattern whose row i holds the `width[i]` columns just left of i (clipped at 0) and i"""
    width = np.minimum(np.asarray(width), np.arange(M))
    rows = np.repeat(np.arange(M), width + 1)
    first = np.cumsum(np.r_[0, width[:-1] + 1])
    cols = rows - width[rows] + (np.arange(rows.size) - first[rows])
    return (M, M) + si.assemble(M, rows, cols, np.ones(rows.size))


def _same(a, ref, what):
    """finite values by bits, infinities by sign, NaN as NaN"""
    a, ref = np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert_same_bits(a[fin], ref[fin], what)
    inf = np.isinf(ref)
    assert np.array_equal(a[inf], ref[inf]), what
    assert np.isnan(a[np.isnan(ref)]).all(), what


def same_factor(got, want, what):
    assert got[0] == want[0] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what + ": the pattern of G"
    _same(got[4], want[4], what)


CASES = {
    "one": lambda: (random_spd(np.random.default_rng(1), 1, 0), None),
    "short": lambda: (random_spd(np.random.default_rng(2), 120, 4), None),
    "stencil": lambda: (stencil(np.random.default_rng(3), 6, 5, 4), None),
    "banded-wide-pattern": lambda: (random_spd(np.random.default_rng(4), 150, 5, spread=12),
                                    dense_rows(None, 150, np.random.default_rng(5).integers(0, 40, 150))),
    "full-64": lambda: (random_spd(np.random.default_rng(6), 90, 30, spread=40), dense_rows(None, 90, np.full(90, 63))),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_references_agree_bit_for_bit(name):
    A, S = CASES[name]()
    loop, info = fr.fsai_loop(A, S)
    vec, info_v = fr.fsai_vec(A, S)
    same_factor(vec, loop, name)
    assert info == info_v and info["badRows"] == 0 and info["firstBadRow"] == -1


def test_the_pattern_rule():
    """the columns j < i of the pattern's row, then i, whether or not the pattern stores the diagonal"""
    S = (4, 4) + si.assemble(4, np.array([1, 1, 2, 2, 3, 3, 3]), np.array([0, 3, 1, 3, 0, 2, 3]), np.ones(7))
    IRPg, JAg = fr.pattern(4, S[2], S[3])
    assert IRPg.tolist() == [0, 1, 3, 5, 8] and JAg.tolist() == [0, 0, 1, 1, 2, 0, 2, 3]
    with pytest.raises(ValueError, match="row 64 "):
        fr.fsai_vec(random_spd(np.random.default_rng(7), 70, 2), dense_rows(None, 70, np.arange(70)))


def test_inputs_are_order_sensitive():
    """the Crout form -- an entry's updates summed first and subtracted once -- gives other bits on these inputs, so the GPU
    tests can tell the loop's update order from another"""
    A, S = CASES["full-64"]()
    ref, crout = fr.fsai_loop(A, S)[0], fr.fsai_crout(A, S)[0]
    assert np.allclose(crout[4], ref[4], rtol=1e-9, atol=1e-13)
    assert differing_rows(crout[4], ref[4]).size > ref[4].size // 20
    with pytest.raises(AssertionError):
        assert_same_bits(crout[4], ref[4])
    A, S = CASES["short"]()
    assert differing_rows(fr.fsai_crout(A, S)[0][4], fr.fsai_vec(A, S)[0][4]).size > 0


@pytest.mark.parametrize("name", ["short", "stencil", "banded-wide-pattern", "full-64"])
def test_every_row_solves_its_dense_system(name):
    """row i of G is e_n^T B^-1 / sqrt((B^-1)_nn) for B = A(P, P): numpy.linalg.solve's answer to a relative 1e-10 (blocks of
    at most 64 with a scaled condition of at most 5: n cond 2^-53 is below 4e-14), and diag(G A G^T) = 1 to the same bound"""
    A, S = CASES[name]()
    (M, _, IRPg, JAg, ASg), info = fr.fsai_vec(A, S)
    IRPg, JAg = IRPg.astype(np.int64), JAg.astype(np.int64)
    D = fr.dense(A)
    D = np.tril(D) + np.tril(D, -1).T                                    # what the setup reads: the lower triangle, mirrored
    worst = 0.0
    for i in range(M):
        P = JAg[IRPg[i]:IRPg[i + 1]]
        B = D[np.ix_(P, P)]
        s = 1.0 / np.sqrt(np.diag(B))
        assert np.linalg.cond(B * s[:, None] * s[None, :]) <= 5.0 + 1e-9
        y = np.linalg.solve(B, np.eye(P.size)[:, -1])
        want = y / np.sqrt(y[-1])
        got = ASg[IRPg[i]:IRPg[i + 1]]
        worst = max(worst, np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"{name}: the worst row differs from numpy.linalg.solve by a relative {worst:.2e}")
    assert worst <= 1e-10
    G = fr.dense((M, M, IRPg, JAg, ASg))
    assert np.max(np.abs(np.diag(G @ D @ G.T) - 1.0)) <= 1e-10
    assert info["maxRow"] == int(np.diff(IRPg).max()) and info["nnz"] == JAg.size


def test_a_planted_negative_diagonal_gives_identity_rows():
    """a diagonal made negative in a middle row: that row and every later row whose columns hold it are BAD -- the identity
    row -- and the first of them is named; every other row keeps its bits"""
    A, _ = CASES["short"]()
    M, _, IRP, JA, AS = A
    r = 57
    clean = fr.fsai_vec(A)[0]
    AS = AS.copy()
    AS[int(IRP[r]) + int(np.searchsorted(JA[int(IRP[r]):int(IRP[r + 1])], r))] = -3.0
    for run in (fr.fsai_loop, fr.fsai_vec):
        (_, _, IRPg, JAg, ASg), info = run((M, M, IRP, JA, AS))
        IRPg, JAg = IRPg.astype(np.int64), JAg.astype(np.int64)
        holds = np.array([r in JAg[IRPg[i]:IRPg[i + 1]] for i in range(M)])
        assert info["firstBadRow"] == r and info["badRows"] == int(holds.sum()) >= 1
        for i in range(M):
            g = ASg[IRPg[i]:IRPg[i + 1]]
            if holds[i]:
                assert_same_bits(g, np.r_[np.zeros(g.size - 1), 1.0], f"row {i}")
            else:
                assert_same_bits(g, clean[4][IRPg[i]:IRPg[i + 1]], f"row {i}")


def test_the_upper_triangle_is_never_read():
    A, S = CASES["banded-wide-pattern"]()
    M, _, IRP, JA, AS = A
    poisoned = np.where(JA.astype(np.int64) > si.row_of_entry(IRP), np.nan, AS)
    same_factor(fr.fsai_vec((M, M, IRP, JA, poisoned), S)[0], fr.fsai_vec(A, S)[0], "NaN right of the diagonal")


def test_the_apply_is_two_serial_order_products(oracle):
    A, _ = CASES["stencil"]()
    G = fr.fsai_vec(A)[0]
    T = fr.transposed(G)
    v = si.order_values(np.random.default_rng(8), A[0])
    want = oracle.csr_serial(T[2], T[3], T[4], oracle.csr_serial(G[2], G[3], G[4], v))
    assert_same_bits(fr.Applied(G)(v), want, "G^T (G v)")
