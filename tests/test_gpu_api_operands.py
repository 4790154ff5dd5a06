"""How the Python layer marshals operands (spmv_openmp_cuda_amd/api.py): the cells of the table in
profiles/api_operands_checks.md that no other test reaches.  Accepted forms of a device call (contiguous tensors, views at
an odd element offset, `out=`, every dense layout) give the bits of the host call on the same data; refused forms (wrong
length, float32, a CPU tensor, a non-unit stride, a wrong rank, mixed kinds, `out=` on a host call) raise SpmvHipError,
leave a poisoned `out` / `x0` as it was and launch nothing.  Only marshalling is under test: 27 rows, k = 3."""
import types

import numpy as np
import pytest

import spgemm_ref as sr
from bits import assert_same_bits

pytestmark = pytest.mark.gpu

N, K = 27, 3
POISON = -777.25                                            # no result of these operands holds it everywhere
MARK = ((7, 1, 1), (256, 1, 1))                             # the launch shape of spmvHipMultiDot with k = 13
SOLVERS = {"cg": {}, "bicgstab": {}, "gmres": {"restart": 5}}


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def prob(api, torch):
    """the 3 x 3 x 3 Laplacian, its ILU(0) factors and hierarchy, the operands, and every host call's result, once"""
    A = sr.laplacian7(3, 3, 3)
    assert A[0] == N
    rng = np.random.default_rng(4501)
    p = types.SimpleNamespace()
    p.da, p.F = api.spMatCpyCSR(api.HostCSR(*A)), api.spMatCpyCSR(api.HostCSR(*A))
    p.F.ilu0()
    p.h = p.da.amg(coarseRows=4)
    p.b, p.x0, p.X = rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal((N, K))
    p.perm = rng.permutation(N).astype(np.int32)
    p.dperm = torch.from_numpy(p.perm).cuda()
    p.host = {"matmul": p.da.matmul(p.X), "matmul1": p.da.matmul(p.X[:, :1]), "apply": p.h.apply(p.b),
              "multi_dot": api.multi_dot(p.X, p.b), "multi_dot1": api.multi_dot(p.X[:, :1], p.b)}
    for lower in (True, False):
        p.host["trsv", lower] = p.F.solve_triangular(p.b, lower=lower, unit_diagonal=lower)
    for inverse in (False, True):
        p.host["permute", inverse] = api.permute_vector(p.dperm, p.b, inverse=inverse)
    for kind, kw in SOLVERS.items():
        for x0 in (None, p.x0):
            x, info = getattr(p.da, kind)(p.b, x0=x0, precond=p.F, tol=1e-12, maxiter=40, history=True, **kw)
            p.host[kind, x0 is not None] = x, info.status, info.iterations, info.history
    yield p
    for d in (p.h, p.F, p.da):
        d.free()


def _dev(torch, a, odd=False):
    """`a` on the device: a contiguous tensor, or (odd) a view at element offset 1 of a buffer one element longer, so
    that it is 8-byte and not 16-byte aligned"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not odd:
        return torch.from_numpy(a).cuda()
    buf = torch.full((a.size + 1,), POISON, dtype=torch.float64, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8
    return view


def _poison(torch, shape, odd=False):
    return _dev(torch, np.full(shape, POISON), odd)


def _same(got, want, what):
    assert got.is_cuda and got.dtype.is_floating_point, what
    assert_same_bits(got.cpu().numpy(), want, what)


# ------------------------------------------------------------------------------------------------------ accepted forms
def test_matmul_every_layout_and_offset(api, torch, prob):
    da, want = prob.da, prob.host["matmul"]
    forms = {"row-major": _dev(torch, prob.X), "row-major at an odd offset": _dev(torch, prob.X, odd=True),
             ".t() view, column-major": _dev(torch, prob.X.T).t(), ".t() view at an odd offset": _dev(torch, prob.X.T, odd=True).t()}
    for xn, X in forms.items():
        assert tuple(X.shape) == (N, K)
        Y = da.matmul(X)
        assert tuple(Y.shape) == (N, K) and Y.is_contiguous()
        _same(Y, want, xn)
        outs = {"row-major": _poison(torch, (N, K)), "row-major at an odd offset": _poison(torch, (N, K), odd=True),
                "column-major": _poison(torch, (K, N)).t(), "column-major at an odd offset": _poison(torch, (K, N), odd=True).t()}
        for on, out in outs.items():
            assert da.matmul(X, out=out) is out
            _same(out, want, f"X {xn}, out {on}")
    for xn, X in (("(N, 1)", _dev(torch, prob.X[:, :1])), ("(1, N).t()", _dev(torch, prob.X[:, :1].T).t()),
                  ("a column of a row-major X", _dev(torch, prob.X)[:, :1])):
        _same(da.matmul(X), prob.host["matmul1"], "k = 1, " + xn)
        out = _poison(torch, (N, K))[:, 1:2]                 # k = 1 with a leading dimension of 3
        assert da.matmul(X, out=out) is out
        _same(out, prob.host["matmul1"], "k = 1, out a column, " + xn)


@pytest.mark.parametrize("lower", [True, False])
def test_solve_triangular_offsets_and_out(api, torch, prob, lower):
    F, want = prob.F, prob.host["trsv", lower]
    kw = dict(lower=lower, unit_diagonal=lower)
    for odd_b in (False, True):
        b = _dev(torch, prob.b, odd_b)
        x = F.solve_triangular(b, **kw)
        assert x.data_ptr() != b.data_ptr()
        _same(x, want, f"b odd {odd_b}")
        _same(b, prob.b, "b is read only")
        for odd_out in (False, True):
            out = _poison(torch, (N,), odd_out)
            assert F.solve_triangular(b, out=out, **kw) is out
            _same(out, want, f"b odd {odd_b}, out odd {odd_out}")
        assert F.solve_triangular(b, out=b, **kw) is b      # in place, also at the odd offset
        _same(b, want, f"in place, odd {odd_b}")


@pytest.mark.parametrize("kind", list(SOLVERS))
def test_solvers_offsets_and_x0(api, torch, prob, kind):
    solve = getattr(prob.da, kind)
    for with_x0 in (False, True):
        wx, wstatus, wit, whist = prob.host[kind, with_x0]
        for odd in (False, True):
            b = _dev(torch, prob.b, odd)
            x0 = _dev(torch, prob.x0, odd) if with_x0 else None
            x, info = solve(b, x0=x0, precond=prob.F, tol=1e-12, maxiter=40, history=True, **SOLVERS[kind])
            what = f"{kind}, x0 {with_x0}, odd {odd}"
            assert (info.status, info.iterations) == (wstatus, wit), what
            _same(x, wx, what)
            assert_same_bits(info.history, whist, what + ": history")
            _same(b, prob.b, what + ": b is read only")
            if with_x0:
                assert x.data_ptr() != x0.data_ptr()
                _same(x0, prob.x0, what + ": x0 is never written")


def test_apply_offsets_and_out(api, torch, prob):
    want = prob.host["apply"]
    for odd in (False, True):
        r = _dev(torch, prob.b, odd)
        z = prob.h.apply(r)
        assert tuple(z.shape) == (N,)
        _same(z, want, f"r odd {odd}")
        out = _poison(torch, (N,), not odd)
        assert prob.h.apply(r, out=out) is out
        _same(out, want, f"r odd {odd}, out odd {not odd}")


@pytest.mark.parametrize("inverse", [False, True])
def test_permute_vector_offsets_out_and_perm_kinds(api, torch, prob, inverse):
    want = prob.host["permute", inverse]
    assert_same_bits(want, prob.b[prob.perm] if not inverse else prob.b[np.argsort(prob.perm)], "the host call itself")
    pbuf = api.DeviceBuffer(4 * N).up(prob.perm.astype(np.uint32))
    try:
        for perm in (prob.dperm, pbuf):
            for odd in (False, True):
                v = _dev(torch, prob.b, odd)
                _same(api.permute_vector(perm, v, inverse=inverse), want, f"v odd {odd}")
                out = _poison(torch, (N,), not odd)
                assert api.permute_vector(perm, v, inverse=inverse, out=out) is out
                _same(out, want, f"v odd {odd}, out odd {not odd}")
            assert_same_bits(api.permute_vector(perm, prob.b, inverse=inverse), want, "host call, either kind of perm")
    finally:
        pbuf.free()


def test_multi_dot_offsets_and_leading_dimension(api, torch, prob):
    want = prob.host["multi_dot"]
    wide = torch.full((K, N + 5), POISON, dtype=torch.float64, device="cuda")
    wide[:, :N] = _dev(torch, prob.X.T)
    forms = {"columns contiguous": _dev(torch, prob.X.T).t(), "at an odd offset": _dev(torch, prob.X.T, odd=True).t(),
             "ldv = n + 5": wide[:, :N].t()}
    for vn, V in forms.items():
        assert tuple(V.shape) == (N, K) and V.stride(0) == 1
        for odd in (False, True):
            h = api.multi_dot(V, _dev(torch, prob.b, odd))
            assert tuple(h.shape) == (K,)
            _same(h, want, f"V {vn}, w odd {odd}")
    _same(api.multi_dot(_dev(torch, prob.X[:, :1]), _dev(torch, prob.b)), prob.host["multi_dot1"], "k = 1")
    # dot has no host call: its bits are multi_dot's, column by column (include/spmvHip.h)
    for c in range(K):
        d = api.dot(_dev(torch, prob.X[:, c], odd=True), _dev(torch, prob.b))
        assert d.dim() == 0
        _same(d.reshape(1), want[c:c + 1], f"dot of column {c}")


# ------------------------------------------------------------------------------------------------------- refused forms
def _bad_vectors(torch, n):
    """every way a 1-D float64 device operand of length n can be wrong, each filled with POISON"""
    dev = dict(dtype=torch.float64, device="cuda")
    return {"too long": torch.full((n + 1,), POISON, **dev), "too short": torch.full((n - 1,), POISON, **dev),
            "float32": torch.full((n,), POISON, dtype=torch.float32, device="cuda"),
            "a CPU tensor": torch.full((n,), POISON, dtype=torch.float64),
            "stride 2": torch.full((2 * n,), POISON, **dev)[::2], "rank 2": torch.full((n, 1), POISON, **dev),
            "rank 0": torch.full((), POISON, **dev), "numpy on a device call": np.full(n, POISON)}


def _bad_host(n):
    return {"too long": np.zeros(n + 1), "too short": np.zeros(n - 1), "rank 2": np.zeros((n, 1))}


@pytest.fixture
def refused(api, torch):
    """refused(call, *poisoned): the call raises SpmvHipError, launches nothing (the last launch stays the marker's) and
    leaves every poisoned operand as it was"""
    api.multi_dot(torch.zeros((13, N), dtype=torch.float64, device="cuda").t(), torch.zeros(N, dtype=torch.float64, device="cuda"))
    assert api.last_launch() == MARK

    def check(call, *poisoned, what=""):
        with pytest.raises(api.SpmvHipError):
            call()
        assert api.last_launch() == MARK, what + ": a kernel ran"
        for t in poisoned:
            assert bool((torch.as_tensor(t) == POISON).all()), what + ": a refused call wrote to an operand"
    return check


def _vector_call_refusals(torch, refused, call, who):
    """call(v, out): an entry point with one vector operand and `out=`"""
    good, good_out = _dev(torch, np.arange(1.0, N + 1)), _poison(torch, (N,))
    for name, bad in _bad_vectors(torch, N).items():
        if not isinstance(bad, np.ndarray):                             # (a numpy operand alone is a host call)
            refused(lambda: call(bad, None), what=f"{who}: operand {name}")
        refused(lambda: call(bad, good_out), good_out, what=f"{who}: operand {name}, out given")
        refused(lambda: call(good, bad), bad, what=f"{who}: out {name}")
    for name, bad in _bad_host(N).items():
        refused(lambda: call(bad, None), what=f"{who}: host operand {name}")
    refused(lambda: call(np.ones(N), good_out), good_out, what=f"{who}: out= on a host call")
    refused(lambda: call(np.ones(N), np.full(N, POISON)), what=f"{who}: a numpy out= on a host call")


def test_solve_triangular_refusals(api, torch, prob, refused):
    _vector_call_refusals(torch, refused, lambda b, out: prob.F.solve_triangular(b, out=out), "solve_triangular")


def test_apply_refusals(api, torch, prob, refused):
    _vector_call_refusals(torch, refused, lambda r, out: prob.h.apply(r, out=out), "apply")


def test_permute_vector_refusals(api, torch, prob, refused):
    _vector_call_refusals(torch, refused, lambda v, out: api.permute_vector(prob.dperm, v, out=out), "permute_vector")
    v = _dev(torch, prob.b)
    for name, bad in (("int64", prob.dperm.long()), ("a CPU tensor", prob.dperm.cpu()), ("rank 2", prob.dperm.reshape(N, 1)),
                      ("stride 2", torch.zeros(2 * N, dtype=torch.int32, device="cuda")[::2]), ("numpy", prob.perm),
                      ("too short", prob.dperm[:-1])):
        out = _poison(torch, (N,))
        refused(lambda: api.permute_vector(bad, v, out=out), out, what=f"permute_vector: perm {name}")
        refused(lambda: api.permute_vector(bad, prob.b), what=f"permute_vector: perm {name}, host call")


@pytest.mark.parametrize("kind", list(SOLVERS))
def test_solver_refusals(api, torch, prob, refused, kind):
    def solve(b, x0):
        return getattr(prob.da, kind)(b, x0=x0, precond=prob.F, maxiter=5, **SOLVERS[kind])
    good, good_x0 = _dev(torch, prob.b), _poison(torch, (N,))
    for name, bad in _bad_vectors(torch, N).items():
        if not isinstance(bad, np.ndarray):
            refused(lambda: solve(bad, None), what=f"{kind}: b {name}")
        refused(lambda: solve(bad, good_x0), good_x0, what=f"{kind}: b {name}, x0 given")
        refused(lambda: solve(good, bad), bad, what=f"{kind}: x0 {name}")
    for name, bad in _bad_host(N).items():
        refused(lambda: solve(bad, None), what=f"{kind}: host b {name}")
        refused(lambda: solve(prob.b, bad), what=f"{kind}: host x0 {name}")
    refused(lambda: solve(prob.b, good_x0), good_x0, what=f"{kind}: a numpy b with a tensor x0")


def test_dot_refusals(api, torch, refused):
    good = _dev(torch, np.arange(1.0, N + 1))
    for name, bad in _bad_vectors(torch, N).items():
        refused(lambda: api.dot(bad, good), what=f"dot: u {name}")
        refused(lambda: api.dot(good, bad), what=f"dot: v {name}")
    refused(lambda: api.dot(np.ones(N), np.ones(N)), what="dot: there is no host call")


def test_multi_dot_refusals(api, torch, prob, refused):
    V, w = _dev(torch, prob.X.T).t(), _dev(torch, prob.b)
    for name, bad in _bad_vectors(torch, N).items():
        refused(lambda: api.multi_dot(V, bad), what=f"multi_dot: w {name}")
    dev = dict(dtype=torch.float64, device="cuda")
    bad_V = {"rows contiguous": torch.zeros((N, K), **dev), "too long": torch.zeros((K, N + 1), **dev).t(),
             "float32": torch.zeros((K, N), dtype=torch.float32, device="cuda").t(), "a CPU tensor": torch.zeros((K, N), dtype=torch.float64).t(),
             "rank 1": torch.zeros(N, **dev), "rank 3": torch.zeros((1, K, N), **dev).permute(2, 1, 0),
             "ldv < n": torch.zeros(K * N, **dev).as_strided((N, K), (1, N - 1))}
    for name, bad in bad_V.items():
        refused(lambda: api.multi_dot(bad, w), what=f"multi_dot: V {name}")
    refused(lambda: api.multi_dot(prob.X, w), what="multi_dot: a numpy V with a tensor w")
    refused(lambda: api.multi_dot(V, prob.b), what="multi_dot: a tensor V with a numpy w")
    for name, bad in _bad_host(N).items():
        refused(lambda: api.multi_dot(prob.X, bad), what=f"multi_dot: host w {name}")
    refused(lambda: api.multi_dot(prob.b, prob.b), what="multi_dot: host V of rank 1")


def test_matmul_refusals(api, torch, prob, refused):
    da = prob.da
    dev = dict(dtype=torch.float64, device="cuda")
    X, good_out = _dev(torch, prob.X), _poison(torch, (N, K))

    def bad_dense(rows):
        return {"too many rows": torch.full((rows + 1, K), POISON, **dev), "float32": torch.full((rows, K), POISON, dtype=torch.float32, device="cuda"),
                "a CPU tensor": torch.full((rows, K), POISON, dtype=torch.float64),
                "no unit stride": torch.full((2 * rows, 2 * K), POISON, **dev)[::2, ::2], "rank 1": torch.full((rows,), POISON, **dev),
                "rank 3": torch.full((rows, K, 1), POISON, **dev), "no columns": torch.full((rows, 0), POISON, **dev)}
    for name, bad in bad_dense(N).items():
        refused(lambda: da.matmul(bad), what=f"matmul: X {name}")
        refused(lambda: da.matmul(bad, out=good_out), good_out, what=f"matmul: X {name}, out given")
        if name != "no columns":
            refused(lambda: da.matmul(X, out=bad), bad, what=f"matmul: out {name}")
    refused(lambda: da.matmul(X, out=torch.full((N, K + 1), POISON, **dev)), what="matmul: out with another k")
    for name, bad in (("too many rows", np.zeros((N + 1, K))), ("rank 1", np.zeros(N)), ("no columns", np.zeros((N, 0)))):
        refused(lambda: da.matmul(bad), what=f"matmul: host X {name}")
    refused(lambda: da.matmul(prob.X, out=good_out), good_out, what="matmul: out= on a host call")


def test_matmul_refuses_a_numpy_out_on_a_device_call(api, torch, prob, refused):
    """(a case of its own: `out` has to be checked for its kind before any method of a tensor is called on it)"""
    out = np.full((N, K), POISON)
    refused(lambda: prob.da.matmul(_dev(torch, prob.X), out=out), out, what="matmul: a numpy out with a tensor X")
