"""The approximate-inverse preconditioner on the device (spmvHipFsaiSetup / Refresh / Apply / Transpose / Info;
DeviceMatrix.fsai, Fsai): every comparison is by bits with the test side's loop (tests/fsai_ref.py) -- finite values by bits,
infinities by sign, NaN as NaN -- at every forced group width and at the built-in choice.  The inputs are order-sensitive
(tests/test_fsai_abi.py shows that on the host).  References are computed once per case and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import fsai_ref as fr
import serial_order_inputs as si
from bits import assert_same_bits
from gmres_ref import gmres_ref
from krylov_ref import Csr, bicgstab_ref, cg_ref
from test_fsai_abi import _same, dense_rows, random_spd, same_factor, stencil

pytestmark = pytest.mark.gpu

LANES = (0, 4, 16, 64)
TOL = 1e-9


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.lib.spmvHipSetSync(1)
    for name in ("hipSpCGCSR", "hipSpBiCGStabCSR", "hipSpCGBlockCSR", "hipSpBiCGStabBlockCSR"):
        api.set_variant(name, 16)


def _up(api, A):
    return api.spMatCpyCSR(api.HostCSR(*A))


def _down(api, ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes) == 0
    return out


def _arrays(api, dm):
    h = dm.handle
    M, NZ = int(h.M), int(h.NZ)
    return (M, int(h.N), _down(api, h.IRP, M + 1, np.uint32).astype(np.uint64), _down(api, h.JA, NZ, np.uint32).astype(np.uint64),
            _down(api, h.AS, NZ, np.float64))


def _addresses(dm):
    h = dm.handle
    return tuple(C.cast(p, C.c_void_p).value for p in (h.IRP, h.JA, h.AS)) + (int(h.M), int(h.N), int(h.NZ))


# ------------------------------------------------------------------------------------------------------------- the cases
def _empty():
    return 0, 0, np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0)


def _poisoned(A):
    M, N, IRP, JA, AS = A
    return M, N, IRP, JA, np.where(JA.astype(np.int64) > si.row_of_entry(IRP), np.nan, AS)


def _negative_diagonal(A, r):
    M, N, IRP, JA, AS = A
    AS = AS.copy()
    AS[int(IRP[r]) + int(np.searchsorted(JA[int(IRP[r]):int(IRP[r + 1])], r))] = -3.0
    return M, N, IRP, JA, AS


# n = G - 1, G, G + 1 for the three group widths, and exactly SPMV_FSAI_MAX_ROW
EDGE_N = (3, 4, 5, 15, 16, 17, 63, 64, 1, 2)

# name -> (A, S): S None for A's own pattern, a matrix for an uploaded pattern, "AA" for tril(A A) made on the device
CASES = {
    "empty": lambda: (_empty(), None),
    "one": lambda: (random_spd(np.random.default_rng(3801), 1, 0), None),
    "stencil-6x5x4": lambda: (stencil(np.random.default_rng(3802), 6, 5, 4), None),
    "random-300": lambda: (random_spd(np.random.default_rng(3803), 300, 4), None),
    "random-3000": lambda: (random_spd(np.random.default_rng(3804), 3000, 4), None),
    "group-edges": lambda: (random_spd(np.random.default_rng(3805), 200, 30, spread=40),
                            dense_rows(None, 200, np.array(EDGE_N)[np.arange(200) % len(EDGE_N)] - 1)),
    "tril-AA": lambda: (random_spd(np.random.default_rng(3806), 250, 3, spread=30), "AA"),
    "poisoned-upper": lambda: (_poisoned(random_spd(np.random.default_rng(3807), 300, 5)), None),
    "negative-diagonal": lambda: (_negative_diagonal(random_spd(np.random.default_rng(3808), 300, 4), 140), None),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


_REF = {}


def _reference(name, A, S):
    if name not in _REF:
        _REF[name] = fr.fsai_vec(A, S)
    return _REF[name]


def _setup(api, name, lanes):
    """(da, g, A, reference) of a case: the device setup at a forced width, and the shared reference"""
    A, S = _case(name)
    da = _up(api, A)
    ds = None
    try:
        if isinstance(S, str):
            prod = da.multiply(da)
            ds = prod.tril()
            prod.free()
            S = _arrays(api, ds)                                         # the pattern the device made, as the reference's pattern
        elif S is not None:
            ds = _up(api, S)
        g = da.fsai(pattern=ds, lanes_per_row=lanes)
    except Exception:
        da.free()
        raise
    finally:
        if ds is not None:
            ds.free()                                                # the pattern need not outlive the setup
    return da, g, A, _reference(name, A, S)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", list(CASES))
def test_the_factor_has_the_bits_of_the_loop(api, name, lanes):
    da, g, A, (G, info) = _setup(api, name, lanes)
    try:
        same_factor(_arrays(api, g), G, f"{name}, lanesPerRow {lanes}")
        got = g.info()
        assert (got.nnz, got.maxRow, got.badRows, got.firstBadRow) == (info["nnz"], info["maxRow"], info["badRows"], info["firstBadRow"])
        assert got.setups == 1 and (got.launches == 0) == (A[0] == 0), "M = 0 asks for no kernel"
        if name == "negative-diagonal":
            assert got.firstBadRow == 140 and got.badRows >= 1
        elif name == "group-edges":
            assert got.maxRow == 64 and got.badRows == 0
        else:
            assert got.badRows == 0 and got.firstBadRow == -1
    finally:
        g.free()
        da.free()


@pytest.mark.parametrize("name", ["empty", "one", "random-300", "group-edges"])
def test_the_owned_transpose_is_the_transpose(api, name):
    da, g, A, (G, _) = _setup(api, name, 0)
    t = g.transpose()
    try:
        view, made, want = g.transposed(), _arrays(api, t), fr.transposed(G)
        for got, what in ((view, "the view"), (made, "spmvHipCsrTranspose of G")):
            assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what
            _same(got[4], want[4], what)
    finally:
        t.free()
        g.free()
        da.free()


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", ["empty", "one", "stencil-6x5x4", "random-3000", "group-edges", "negative-diagonal"])
def test_apply_is_two_serial_order_products(api, oracle, name, lanes):
    import torch
    da, g, A, (G, _) = _setup(api, name, lanes)
    try:
        M = A[0]
        T = fr.transposed(G)
        r = si.order_values(np.random.default_rng(3810), M)
        want = oracle.csr_serial(T[2], T[3], T[4], oracle.csr_serial(G[2], G[3], G[4], r)) if M else np.zeros(0)
        assert_same_bits(g.apply(r), want, f"{name}: host call")
        if M == 0:                                                       # (an empty tensor has no address to hand over)
            return
        rt = torch.from_numpy(r).cuda()
        assert_same_bits(g.apply(rt).cpu().numpy(), want, f"{name}: device call")
        assert g.apply(rt, out=rt) is rt
        assert_same_bits(rt.cpu().numpy(), want, f"{name}: in place")
    finally:
        g.free()
        da.free()


@pytest.mark.parametrize("lanes", LANES)
def test_refresh_keeps_the_addresses_and_gives_a_fresh_setup(api, oracle, lanes):
    A, _ = _case("random-300")
    M, _, IRP, JA, AS = A
    B = random_spd(np.random.default_rng(3803), 300, 4, e=1)             # the case's seed: the pattern of A, other values
    assert np.array_equal(B[2], IRP) and np.array_equal(B[3], JA) and not np.array_equal(B[4], AS)
    da = _up(api, A)
    g = da.fsai(lanes_per_row=lanes)
    try:
        where, view = _addresses(g), g.transposed()
        da.update_values(B[4])
        info = g.refresh_from(da)
        want, winfo = fr.fsai_vec(B)
        assert _addresses(g) == where, "IRP, JA and AS keep their addresses"
        same_factor(_arrays(api, g), want, "after the refresh")
        assert (info.setups, info.badRows, info.firstBadRow, info.nnz) == (2, winfo["badRows"], winfo["firstBadRow"], winfo["nnz"])
        T = fr.transposed(want)
        got = g.transposed()
        assert np.array_equal(got[2], view[2]) and np.array_equal(got[3], view[3])
        _same(got[4], T[4], "G^T after the refresh")
        r = si.order_values(np.random.default_rng(3812), M)
        assert_same_bits(g.apply(r), fr.Applied(want)(r), "apply after the refresh")
        fresh = da.fsai(lanes_per_row=lanes)
        try:
            same_factor(_arrays(api, g), _arrays(api, fresh), "the refreshed factor against a fresh setup")
        finally:
            fresh.free()
    finally:
        g.free()
        da.free()


# -------------------------------------------------------------------------------------------------------------- Krylov
@pytest.fixture(scope="module")
def krylov(api):
    """a stencil, its factor, the numpy matrix whose M^-1 is G^T (G v), a right-hand side"""
    A = stencil(np.random.default_rng(3820), 9, 8, 7)
    G, _ = fr.fsai_vec(A)
    b = np.random.default_rng(3821).standard_normal(A[0])
    da = _up(api, A)
    g = da.fsai()
    yield A, b, fr.PrecondCsr(A, G), da, g
    g.free()
    da.free()


SOLVERS = {"cg": (cg_ref, {}, ()), "bicgstab": (bicgstab_ref, {}, ()), "gmres": (gmres_ref, dict(restart=5), (5,))}


@pytest.mark.parametrize("method", list(SOLVERS))
def test_the_solvers_take_the_factor(api, krylov, method):
    A, b, ref, da, g = krylov
    loop, kw, tail = SOLVERS[method]
    want = loop(ref, b, np.zeros(A[0]), TOL, 200, *tail)
    x, info = getattr(da, method)(b, precond=g, tol=TOL, maxiter=200, history=True, **kw)
    assert (info.status, info.iterations) == (want[1], want[2]), method
    assert_same_bits(x, want[0], f"{method}: x")
    assert_same_bits(info.history, want[3], f"{method}: history")
    if method == "cg":
        plain = cg_ref(Csr(A[0], A[2], A[3], A[4]), b, np.zeros(A[0]), TOL, 200)
        assert want[1] == 0 and want[2] < plain[2], "the factor is a preconditioner"
        # CG's own kernels: 4 before the loop and 6 per enqueued iteration (whole batches of K = 16); every M^-1 (one before
        # the loop, one per iteration) adds the two SpMVs, a dot pass and its finish
        enq = min(200, -(-want[2] // 16) * 16)
        assert info.launches == 4 + 6 * enq + (enq + 1) * (2 + 2)


def test_products_queued_past_the_stop_change_nothing(api, krylov):
    A, b, ref, da, g = krylov
    want = cg_ref(ref, b, np.zeros(A[0]), TOL, 200)
    assert want[2] % 16, "the stop falls inside a batch of K = 16: queued SpMVs run after it"
    for K in (1, 16):
        api.set_variant("hipSpCGCSR", K)
        x, info = da.cg(b, precond=g, tol=TOL, maxiter=200)
        assert info.iterations == want[2]
        assert_same_bits(x, want[0], f"K = {K}")


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_the_block_solvers_give_the_single_solves(api, krylov, method, k):
    A, b, ref, da, g = krylov
    M = A[0]
    rng = np.random.default_rng(3830 + k)
    B = np.ascontiguousarray(np.stack([b] + [rng.standard_normal(M) for _ in range(k - 1)], axis=1))
    X, info = getattr(da, method + "_block")(B, precond=g, tol=TOL, maxiter=200, history=True)
    for c in range(k):
        x, one = getattr(da, method)(np.ascontiguousarray(B[:, c]), precond=g, tol=TOL, maxiter=200, history=True)
        col = info.columns[c]
        assert (col.status, col.iterations) == (one.status, one.iterations), f"{method}, column {c} of {k}"
        assert_same_bits(X[:, c], x, f"{method}, column {c} of {k}: x")
        assert_same_bits(info.history[c], one.history, f"{method}, column {c} of {k}: history")
        assert_same_bits([col.rr, col.bb], [one.rr, one.bb], f"{method}, column {c} of {k}: rr, bb")
    loop = cg_ref if method == "cg" else bicgstab_ref
    assert_same_bits(X[:, 0], loop(ref, b, np.zeros(M), TOL, 200)[0], f"{method}: column 0 against the numpy loop")


def test_a_factor_of_another_matrix_of_the_size_is_taken_and_another_size_refused(api, krylov, capfd):
    A, b, ref, da, g = krylov
    M = A[0]
    other = stencil(np.random.default_rng(3840), 9, 8, 7)               # the same size, other values: a lagged preconditioner
    small = stencil(np.random.default_rng(3841), 4, 3, 2)
    do, ds = _up(api, other), _up(api, small)
    go, gs = do.fsai(), ds.fsai()
    try:
        want = cg_ref(fr.PrecondCsr(A, fr.fsai_vec(other)[0]), b, np.zeros(M), TOL, 200)
        x, info = da.cg(b, precond=go, tol=TOL, maxiter=200)
        assert (info.status, info.iterations) == (want[1], want[2])
        assert_same_bits(x, want[0], "a factor of another matrix")
        B = np.ascontiguousarray(np.stack([b, 2.0 * b], axis=1))
        calls = [lambda: da.cg(b, precond=gs), lambda: da.bicgstab(b, precond=gs), lambda: da.gmres(b, precond=gs),
                 lambda: da.cg_block(B, precond=gs), lambda: da.bicgstab_block(B, precond=gs)]
        for call in calls:
            capfd.readouterr()
            with pytest.raises(api.SpmvHipError):
                call()
            assert "dM has 24 rows" in capfd.readouterr().err
    finally:
        go.free()
        gs.free()
        do.free()
        ds.free()


def test_the_factor_is_an_ordinary_handle(api, oracle):
    """SpMV, the product and to_coo take G: G A G^T by the public product has a unit diagonal"""
    da, g, A, (G, _) = _setup(api, "stencil-6x5x4", 0)
    t = g.transpose()
    ga = g.multiply(da)
    gag = ga.multiply(t)
    try:
        rows, cols, vals = gag.to_coo()
        d = vals[rows == cols]
        assert d.size == A[0] and np.max(np.abs(d - 1.0)) <= 1e-10
        x = si.order_values(np.random.default_rng(3850), A[0])
        dx, dy = api.DeviceVector(x.size).up(x), api.DeviceVector(A[0])
        try:
            dy.poison()
            api.spmv("hipSpMVRowsCSR", g, dx, dy)
            assert_same_bits(dy.down(), oracle.csr_serial(G[2], G[3], G[4], x), "hipSpMVRowsCSR on G")
        finally:
            dx.free()
            dy.free()
    finally:
        for m in (gag, ga, t, g, da):
            m.free()
