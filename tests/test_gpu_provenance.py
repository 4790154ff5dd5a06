"""Where a device handle came from, and the one question every call on a derived handle asks: "was dX made by F from these
sources?".  Handles of every origin -- uploaded, adopted, ELL of a CSR handle, transpose, permutation, product, multigrid
hierarchy -- are made from one 29 x 29 matrix, and every call that takes a derived handle (the four refreshes, the cycle and
a solver's dM) is given every one of them: the wrong kind and the right kind of another source are refused with the maker's
name on stderr and nothing written, the right combination is taken.  Nothing here depends on size."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 29
SENTINEL = 0xAB


def _matrix(seed):
    """a symmetric pattern with a full diagonal, symmetric values, diagonally dominant"""
    rng = np.random.default_rng(seed)
    mask = np.triu(rng.random((M, M)) < 0.15, 1)
    vals = np.where(mask, rng.uniform(-1.0, 1.0, (M, M)), 0.0)
    dense = vals + vals.T
    dense[np.arange(M), np.arange(M)] = np.abs(dense).sum(axis=1) + 1.0
    rows, cols = np.nonzero(dense)
    IRP = np.zeros(M + 1, np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return M, M, IRP, cols.astype(np.uint64), dense[rows, cols]


A = _matrix(29)
PERM = np.random.default_rng(30).permutation(M).astype(np.uint32)
ORIGINS = ("uploaded", "adopted", "ell", "transpose", "permutation", "product", "hierarchy")
CSR_ORIGINS = ("uploaded", "adopted", "transpose", "permutation", "product")


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


def _up(api):
    return api.spMatCpyCSR(api.HostCSR(*A))


def _adopt(api):
    _, _, IRP, JA, AS = A
    bufs = [api.DeviceBuffer(4 * (M + 1)).up(IRP.astype(np.uint32)), api.DeviceBuffer(4 * JA.size).up(JA.astype(np.uint32)),
            api.DeviceBuffer(8 * JA.size).up(AS)]
    dm = api.DeviceMatrix()
    dm.keep = bufs
    assert api.lib.spmvHipAdoptCSR(C.byref(dm.handle), M, M, JA.size, bufs[0].ptr, 4, bufs[1].ptr, bufs[2].ptr, None) == 0
    return dm


def _family(api, src):
    """every kind of handle that is made from another one, made from src (and, the product, from src and its transpose)"""
    t = src.transpose()
    return {"ell": api.csr_to_ell_device(src, False), "transpose": t, "permutation": src.permute(PERM), "product": src.multiply(t),
            "hierarchy": src.amg(coarseRows=8)}


@pytest.fixture(scope="module")
def zoo(api):
    """`own`: a handle of every origin, the derived ones made from own["uploaded"]; `other`: the derived kinds again, from
    another upload of the same matrix (the product: of that upload and the FIRST family's transpose)"""
    up, up2 = _up(api), _up(api)
    own = dict(_family(api, up), uploaded=up, adopted=_adopt(api))
    assert own["hierarchy"].info.levels >= 2, "the hierarchy holds products of its own"
    t2 = up2.transpose()
    other = {"uploaded": up2, "transpose": t2, "permutation": up2.permute(PERM), "product": up2.multiply(own["transpose"]),
             "hierarchy": up2.amg(coarseRows=8)}
    vec = {"r": api.DeviceVector(M).up(np.arange(1.0, M + 1)), "z": api.DeviceVector(M)}
    yield own, other, vec
    for d in list(own.values()) + list(other.values()) + list(vec.values()):
        d.free()


def _bytes_of(api, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    if nbytes:
        assert api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), nbytes) == 0
    return out


def _values(api, dm, origin):
    """the stored values of a handle as bytes (a hierarchy handle has none of its own)"""
    h = dm.handle
    if origin == "hierarchy":
        return np.empty(0, np.uint8)
    return _bytes_of(api, h.AS, 8 * (int(h.M) * int(h.pitchAS) if origin == "ell" else int(h.NZ)))


def _sentinel(obj):
    C.memset(C.byref(obj), SENTINEL, C.sizeof(obj))
    return bytes(obj)


# what takes a derived handle: name -> (the origin it wants, its maker, the names of its handle arguments, what takes a
# hierarchy in that slot although it is no matrix)
CHECKERS = {
    "spmvHipTransposeRefresh": ("transpose", "spmvHipCsrTranspose", ("dAT", "dA"), False),
    "spmvHipPermuteRefresh": ("permutation", "spmvHipCsrPermute", ("dB", "dA"), False),
    "spmvHipSpGEMMRefresh": ("product", "spmvHipSpGEMM", ("dC", "dA", "dB"), False),
    "spmvHipAmgRefresh": ("hierarchy", "spmvHipAmgSetup", ("dM", "dA"), True),
    "spmvHipAmgApply": ("hierarchy", "spmvHipAmgSetup", ("dM", "dA"), True),
    "hipSpCGCSR": ("hierarchy", "spmvHipAmgSetup", ("dM", "dA"), True),
}


def _call(api, name, X, sources, vec):
    """one call of `name` with X in its derived slot and `sources` as its source handle(s); returns (rc, untouched): whether
    every output of the call other than X's own values still holds what it held"""
    lib = api.lib
    S = [C.byref(s.handle) for s in sources]
    HX = C.byref(X.handle)
    if name in ("spmvHipTransposeRefresh", "spmvHipPermuteRefresh", "spmvHipAmgRefresh"):
        return getattr(lib, name)(HX, S[0]), True
    if name == "spmvHipSpGEMMRefresh":
        info = api.spmvSpgemmInfo()
        before = _sentinel(info)
        return lib.spmvHipSpGEMMRefresh(HX, S[0], S[1], C.byref(info)), bytes(info) == before
    vec["z"].poison()
    before = vec["z"].down().tobytes()
    if name == "spmvHipAmgApply":
        rc = lib.spmvHipAmgApply(HX, S[0], vec["r"].ptr, vec["z"].ptr)
        return rc, vec["z"].down().tobytes() == before
    assert name == "hipSpCGCSR"
    opts, info = api.spmvKrylovOpts(1e-8, 1, None), api.spmvKrylovInfo()
    ibefore = _sentinel(info)
    rc = lib.hipSpCGCSR(S[0], HX, vec["r"].ptr, vec["z"].ptr, C.byref(opts), C.byref(info))
    return rc, vec["z"].down().tobytes() == before and bytes(info) == ibefore


def _sources(name, family, own):
    return (family["uploaded"], own["transpose"]) if name == "spmvHipSpGEMMRefresh" else (family["uploaded"],)


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("name", list(CHECKERS))
def test_every_origin_in_the_derived_slot(api, zoo, capfd, name, origin):
    own, other, vec = zoo
    wants, maker, args, takes_hierarchy = CHECKERS[name]
    X = own[origin]
    before = _values(api, X, origin)
    capfd.readouterr()
    rc, untouched = _call(api, name, X, _sources(name, own, own), vec)
    err = capfd.readouterr().err
    if origin == wants:
        assert rc == 0, (name, origin, err)
        return
    if name == "hipSpCGCSR" and origin in CSR_ORIGINS:
        # a solver's dM that is a square CSR matrix is taken as ILU(0) factors, whatever made it: no refusal to pin down,
        # but it must not be mistaken for a hierarchy
        assert rc == 0 and "not made by" not in err, (origin, err)
        assert np.array_equal(_values(api, X, origin), before)
        return
    assert rc != 0 and untouched, (name, origin)
    assert np.array_equal(_values(api, X, origin), before), "a refused call leaves the handle's values alone"
    assert f"{name}: " in err, err
    if name == "hipSpCGCSR":
        assert origin == "ell" and "ELL handle" in err, err
    elif origin == "hierarchy" and not takes_hierarchy:
        assert "multigrid hierarchy" in err and "spmvHipAmgSetup" in err, err
    else:
        assert f"{args[0]} was not made by {maker}" in err, err


@pytest.mark.parametrize("name", list(CHECKERS))
def test_the_right_kind_of_another_source(api, zoo, capfd, name):
    own, other, vec = zoo
    wants, maker, args, _ = CHECKERS[name]
    X = other[wants]
    before = _values(api, X, wants)
    capfd.readouterr()
    rc, untouched = _call(api, name, X, _sources(name, own, own), vec)
    err = capfd.readouterr().err
    assert rc != 0 and untouched, name
    assert np.array_equal(_values(api, X, wants), before)
    assert f"{name}: " in err and "not made by" not in err and all(a in err for a in args), err
    # ... and with the sources it was made from it is taken
    rc, _ = _call(api, name, X, _sources(name, other, own), vec)
    assert rc == 0, name


def test_a_product_wants_its_pair_in_its_order(api, zoo, capfd):
    own, other, vec = zoo
    c, a, b = own["product"], own["uploaded"], own["transpose"]
    before = _values(api, c, "product")
    for pair in ((b, a), (a, a), (b, b), (a, other["transpose"])):
        capfd.readouterr()
        rc, untouched = _call(api, "spmvHipSpGEMMRefresh", c, pair, vec)
        err = capfd.readouterr().err
        assert rc != 0 and untouched and "spmvHipSpGEMMRefresh: " in err and "in its order" in err, err
        assert np.array_equal(_values(api, c, "product"), before)
    assert _call(api, "spmvHipSpGEMMRefresh", c, (a, b), vec)[0] == 0


def test_update_values_by_origin(api, zoo, capfd):
    own, _, _ = zoo
    lib = api.lib
    for origin in CSR_ORIGINS:
        h = own[origin].handle
        vals = np.frombuffer(_values(api, own[origin], origin).tobytes(), np.float64).copy()
        assert vals.size == int(h.NZ)
        assert lib.spmvHipUpdateValues(C.byref(h), vals.ctypes.data_as(C.c_void_p), 0) == 0, origin
        assert np.array_equal(np.frombuffer(_values(api, own[origin], origin).tobytes(), np.float64), vals), origin
    capfd.readouterr()
    ell = own["ell"]
    before = _values(api, ell, "ell")
    vals = np.ones(int(ell.handle.M) * int(ell.handle.MAX_ROW_NZ))
    assert lib.spmvHipUpdateValues(C.byref(ell.handle), vals.ctypes.data_as(C.c_void_p), 0) != 0
    err = capfd.readouterr().err
    assert "spmvHipUpdateValues: " in err and "ELL handle" in err and "spmvHipCsrToEll" in err, err
    assert np.array_equal(_values(api, ell, "ell"), before)
    up_ell = api.spMatCpyELL(api.HostCSR(*A).to_ell())              # an uploaded ELL takes new values
    try:
        K = int(up_ell.handle.MAX_ROW_NZ)
        assert lib.spmvHipUpdateValues(C.byref(up_ell.handle), np.ones(M * K).ctypes.data_as(C.c_void_p), 0) == 0
    finally:
        up_ell.free()


def test_a_hierarchy_is_no_matrix(api, zoo, capfd):
    own, _, vec = zoo
    lib = api.lib
    H, HA = C.byref(own["hierarchy"].handle), C.byref(own["uploaded"].handle)
    r, z = vec["r"].ptr, vec["z"].ptr
    out, cfg = api.spmat(), api.CONFIG()
    vals = np.ones(int(own["uploaded"].handle.NZ))
    perm = api.DeviceBuffer(4 * M).up(PERM)
    opts, info = api.spmvKrylovOpts(1e-8, 1, None), api.spmvKrylovInfo()
    calls = {
        "hipSpMVRowsCSR": lambda: lib.hipSpMVRowsCSR(H, r, cfg, z),
        "hipSpMVWarpPerRowCSR": lambda: lib.hipSpMVWarpPerRowCSR(H, r, cfg, z),
        "hipSpMVRowsELL": lambda: lib.hipSpMVRowsELL(H, r, cfg, z),
        "hipSpMMRowsCSR": lambda: lib.hipSpMMRowsCSR(H, 1, r, 1, 0, z, 1, 0),
        "spmvHipBuildTiles": lambda: lib.spmvHipBuildTiles(H),
        "spmvHipBuildStripes": lambda: lib.spmvHipBuildStripes(H),
        "spmvHipBuildSell": lambda: lib.spmvHipBuildSell(H),
        "spmvHipCsrToEll": lambda: lib.spmvHipCsrToEll(H, 0, C.byref(out)),
        "spmvHipCsrTranspose": lambda: lib.spmvHipCsrTranspose(H, C.byref(out)),
        "spmvHipCsrPermute": lambda: lib.spmvHipCsrPermute(H, perm.ptr, C.byref(out)),
        "spmvHipSpGEMM": lambda: lib.spmvHipSpGEMM(H, HA, None, C.byref(out), None) and lib.spmvHipSpGEMM(HA, H, None, C.byref(out), None),
        "spmvHipUpdateValues": lambda: lib.spmvHipUpdateValues(H, vals.ctypes.data_as(C.c_void_p), 0),
        "spmvHipValuesChanged": lambda: lib.spmvHipValuesChanged(H),
        "spmvHipTriAnalyse": lambda: lib.spmvHipTriAnalyse(H, 0),
        "hipSpTRSVCSR": lambda: lib.hipSpTRSVCSR(H, 0, 0, r, z),
        "hipSpILU0CSR": lambda: lib.hipSpILU0CSR(H),
        "spmvHipColourCSR": lambda: lib.spmvHipColourCSR(H, None, None, perm.ptr, None),
        "spmvHipAggregateCSR": lambda: lib.spmvHipAggregateCSR(H, None, perm.ptr, None),
        "spmvHipAmgSetup": lambda: lib.spmvHipAmgSetup(H, None, C.byref(out), None),
        "hipSpCGCSR": lambda: lib.hipSpCGCSR(H, None, r, z, C.byref(opts), C.byref(info)),
    }
    try:
        vec["z"].poison()
        before = vec["z"].down().tobytes()
        for name, call in calls.items():
            capfd.readouterr()
            assert call() != 0, name
            err = capfd.readouterr().err
            assert f"{name}: " in err and "multigrid hierarchy" in err, (name, err)
        assert not out.dev and vec["z"].down().tobytes() == before and np.array_equal(perm.down(np.uint32), PERM)
    finally:
        perm.free()


def test_a_new_handle_is_not_the_freed_source(api, zoo, capfd):
    """ids are never reused: a handle uploaded after the source was freed -- the same matrix, possibly at the freed
    descriptor's address -- is not the source"""
    _, _, vec = zoo
    src = _up(api)
    fam = _family(api, src)
    fam.pop("ell").free()
    t = fam["transpose"]
    src.free()
    again = [_up(api) for _ in range(4)]                             # (several: one of them lands where src was)
    try:
        for new in again:
            for name, (wants, _, args, _) in CHECKERS.items():
                capfd.readouterr()
                rc, untouched = _call(api, name, fam[wants], (new, t) if name == "spmvHipSpGEMMRefresh" else (new,), vec)
                err = capfd.readouterr().err
                assert rc != 0 and untouched, name
                assert f"{name}: " in err and "not made by" not in err and all(a in err for a in args), err
    finally:
        for d in list(fam.values()) + again:
            d.free()
