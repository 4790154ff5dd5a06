"""New values for a device handle of the same pattern (spmvHipUpdateValues / spmvHipValuesChanged /
spmvHipShardUpdateValues): every launcher computes with the new values, the kernel selections and the private formats'
index data stay, the serial-order kernels stay bit-identical to sgemvSerial, refusals leave the handle as it was."""
import ctypes as C

import numpy as np
import pytest

from bits import assert_same_bits
from conftest import random_csr, tight_error
from exact_ref import check_any_order

pytestmark = pytest.mark.gpu

GATE = 7e-4
TIGHT = 1e-13


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _default_variants(api):
    """every test starts (and leaves) with the default kernel variants, synchronous launches on the default stream"""
    yield
    api.set_variant("hipSpMVRowsCSR", 2)
    api.set_variant("hipSpMVWarpPerRowCSR", 2)
    api.lib.spmvHipSetUnitValues(1)
    api.lib.spmvHipSetStream(None)
    api.lib.spmvHipSetSync(1)


def _x(rng, n):
    return np.sin(rng.uniform(0, 2 * np.pi, size=n)) * 3e-5


def _run(api, launcher, dmat, x, rows):
    dx = api.DeviceVector(x.size).up(x)
    dy = api.DeviceVector(rows)
    dy.poison()
    api.spmv(launcher, dmat, dx, dy)
    y = dy.down()
    dx.free()
    dy.free()
    return y


@pytest.fixture(scope="module")
def pattern():
    """~375 k entries (above the selections' 2^18 threshold, so every format is eligible), 4 column slices of the
    two-phase format, ~20 stripes bins; sorted distinct columns"""
    rng = np.random.default_rng(909)
    M = N = 50_000
    IRP, JA, _ = random_csr(rng, M, N, rng.integers(2, 14, size=M))
    assert JA.size >= 1 << 18
    vals = [rng.uniform(-1, 1, size=JA.size) for _ in range(3)]
    return M, N, IRP, JA, vals, _x(rng, N)


# (label, launcher, variant of a reference name or None, format to build before the first launch, exact?)
PATHS = [
    ("rows selected", "hipSpMVRowsCSR", 2, None, True),
    ("warp selected", "hipSpMVWarpPerRowCSR", 2, None, False),
    ("rows variant 1", "hipSpMVRowsCSR", 1, None, True),
    ("warp variant 1", "hipSpMVWarpPerRowCSR", 1, None, False),
    ("tiles", "hipSpMVTilesCSR", None, ("tiles", 0), False),
    ("tiles deterministic", "hipSpMVTilesCSR", None, ("tiles", 1), True),
    ("stripes", "hipSpMVStripesCSR", None, ("stripes", 0), False),
    ("stripes owner wavefronts", "hipSpMVStripesCSR", None, ("stripes", 1), True),
    ("stripes ordered tickets", "hipSpMVStripesCSR", None, ("stripes", 2), True),
    ("sell", "hipSpMVRowsSELL", None, None, True),
]


def _launch(api, path, dm, x, M):
    _, launcher, variant, _, _ = path
    if variant is not None:
        api.set_variant(launcher, variant)
    try:
        return _run(api, launcher, dm, x, M)
    finally:
        if variant is not None:
            api.set_variant(launcher, 2)


def _setup(api, path, dm):
    fmt = path[3]
    if fmt and fmt[0] == "tiles":
        api.build_tiles(dm, deterministic=fmt[1])
    elif fmt:
        api.build_stripes(dm, deterministic=fmt[1])


def _check(oracle, path, IRP, JA, AS, x, y, step):
    y_ref = oracle.csr_serial(IRP, JA, AS, x)
    assert not np.isnan(y).any(), (path[0], step)
    if path[4]:
        assert_same_bits(y, y_ref, (path[0], step, np.max(np.abs(y - y_ref))))
    else:
        check_any_order(IRP, JA, AS, x, y, f"{path[0]}, {step}")
        assert tight_error(IRP, JA, AS, x, y_ref, y) <= TIGHT, (path[0], step)
    return y_ref


def _choices(api, dm):
    return (api.lib.spmvHipAutoChoice(C.byref(dm.handle), None), api.lib.spmvHipAutoChoiceRows(C.byref(dm.handle), None))


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_every_path_computes_with_the_new_values(api, oracle, pattern, path):
    """Values A uploaded, the path's format built and run; values B from the host; the same launch now computes B.  The
    selections name the same kernels before and after, the update is in place, and the value map (4 B per entry and
    form, built at this first update) shows in the format's byte count."""
    M, N, IRP, JA, (A, B, _), x = pattern
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
    try:
        _setup(api, path, dm)
        _check(oracle, path, IRP, JA, A, x, _launch(api, path, dm, x, M), "A")
        picks = _choices(api, dm)
        t0, s0 = api.lib.spmvHipTilesBytes(C.byref(dm.handle)), api.lib.spmvHipStripesBytes(C.byref(dm.handle))
        dm.update_values(B)
        info = dm.update_info()
        assert info.inPlace == 1 and info.rebuilt == 0 and info.unitBefore == 0 and info.unitAfter == 0
        assert _choices(api, dm) == picks
        maps = (api.lib.spmvHipTilesBytes(C.byref(dm.handle)) - t0) + (api.lib.spmvHipStripesBytes(C.byref(dm.handle)) - s0)
        assert info.mapsBuilt == 0 or maps >= 4 * JA.size * info.mapsBuilt, (info.mapsBuilt, maps)
        if path[3]:
            assert info.mapsBuilt == 1
        _check(oracle, path, IRP, JA, B, x, _launch(api, path, dm, x, M), "B")
        assert _choices(api, dm) == picks
        dm.update_values(B)                              # steady state: the map is there
        assert dm.update_info().mapsBuilt == 0
        _check(oracle, path, IRP, JA, B, x, _launch(api, path, dm, x, M), "B again")
    finally:
        dm.free()


def test_both_forms_held_are_refreshed(api, oracle, pattern):
    """A handle holding both forms of the two-phase format: both get the new values (the second form's map is a copy of
    the first's -- they share the slice-major order); the launched form is the one that was NOT the active slot during
    the update."""
    M, N, IRP, JA, (A, B, _), x = pattern
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
    try:
        api.build_tiles(dm, deterministic=False)
        api.build_tiles(dm, deterministic=True)             # the explicit launcher now runs this form
        _run(api, "hipSpMVWarpPerRowCSR", dm, x, M)          # (the reduction-order selection leaves the other form active)
        dm.update_values(B)
        assert dm.update_info().mapsBuilt == 2
        assert_same_bits(_run(api, "hipSpMVTilesCSR", dm, x, M), oracle.csr_serial(IRP, JA, B, x))
    finally:
        dm.free()


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_several_updates_in_a_row(api, oracle, pattern, path):
    """A -> B -> C -> A on one handle, from the device (a torch tensor) this time: each step equals the oracle, and the
    deterministic kernels give the bytes of the first y again at the end (the arrival-order ones add in arrival order and
    are not bitwise reproducible even between two launches of the same values; they are held to the tight bound)."""
    torch = pytest.importorskip("torch")
    M, N, IRP, JA, (A, B, Cv), x = pattern
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
    try:
        _setup(api, path, dm)
        first = _launch(api, path, dm, x, M)
        _check(oracle, path, IRP, JA, A, x, first, "A")
        picks = _choices(api, dm)
        for step, vals in (("B", B), ("C", Cv), ("A", A)):
            t = torch.from_numpy(vals).cuda()
            torch.cuda.synchronize()
            dm.update_values(t)
            assert dm.update_info().inPlace == 1
            y = _launch(api, path, dm, x, M)
            _check(oracle, path, IRP, JA, vals, x, y, step)
        assert _choices(api, dm) == picks
        if path[4] or path[2] == 1:                          # every serial-order kernel, and the LDS segmented reduction
            assert y.tobytes() == first.tobytes(), path[0]
    finally:
        dm.free()


@pytest.mark.parametrize("irp_bytes", [4, 8])
def test_adopted_handle(api, oracle, pattern, irp_bytes):
    """Adopted torch arrays: dAS rewritten in place by the caller is NOT seen until spmvHipValuesChanged, then it is;
    spmvHipUpdateValues writes into the caller's adopted array."""
    torch = pytest.importorskip("torch")
    M, N, IRP, JA, (A, B, Cv), x = pattern
    d_irp = torch.from_numpy(IRP.astype(np.int32 if irp_bytes == 4 else np.int64)).cuda()
    d_ja = torch.from_numpy(JA.astype(np.int32)).cuda()
    d_as = torch.from_numpy(A.copy()).cuda()
    torch.cuda.synchronize()
    dm = api.DeviceMatrix()
    assert api.lib.spmvHipAdoptCSR(C.byref(dm.handle), M, N, JA.size, C.c_void_p(d_irp.data_ptr()), irp_bytes,
                                   C.c_void_p(d_ja.data_ptr()), C.c_void_p(d_as.data_ptr()), None) == 0
    names = (("hipSpMVRowsCSR", True), ("hipSpMVWarpPerRowCSR", False))
    try:
        for vals, step in ((A, "A"), (B, "B")):
            if step == "B":
                d_as.copy_(torch.from_numpy(B))
                torch.cuda.synchronize()
                dm.values_changed()
                assert dm.update_info().inPlace == 1
            for name, exact in names:
                path = (name, name, None, None, exact)
                _check(oracle, path, IRP, JA, vals, x, _run(api, name, dm, x, M), step)
        dm.update_values(Cv)                                 # from the host into the adopted array
        torch.cuda.synchronize()
        assert np.array_equal(d_as.cpu().numpy(), Cv)
        for name, exact in names:
            _check(oracle, (name, name, None, None, exact), IRP, JA, Cv, x, _run(api, name, dm, x, M), "C")
    finally:
        dm.free()


def test_unit_transitions(api, oracle, pattern):
    """all 1.0 -> random -> all 2.0 -> random: every launcher is right at every step (formats built while the values were
    unit included), spmvHipUnitValue follows, the stripes format built without a value array is rebuilt at the first
    unit -> non-unit step (rebuilt = 1), and no unit transition but non-unit -> unit counts as in place."""
    M, N, IRP, JA, (A, B, _), x = pattern
    ones, twos = np.ones(JA.size), np.full(JA.size, 2.0)
    seq = [("ones", ones, 1.0), ("A", A, None), ("twos", twos, 2.0), ("B", B, None)]
    for path in PATHS:
        dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, ones))
        try:
            _setup(api, path, dm)
            prev_unit = True
            for k, (step, vals, unit) in enumerate(seq):
                if k:
                    dm.update_values(vals)
                    info = dm.update_info()
                    assert info.unitBefore == prev_unit and info.unitAfter == (unit is not None), (path[0], step)
                    assert info.inPlace == (not prev_unit), (path[0], step)
                    if k == 1 and path[3] and path[3][0] == "stripes":
                        assert info.rebuilt == 1, path[0]
                v = C.c_double(0)
                assert api.lib.spmvHipUnitValue(C.byref(dm.handle), C.byref(v)) == (1 if unit is not None else 0), (path[0], step)
                if unit is not None:
                    assert v.value == unit
                _check(oracle, path, IRP, JA, vals, x, _launch(api, path, dm, x, M), step)
                prev_unit = unit is not None
        finally:
            dm.free()


def test_unit_detection_off_is_honoured(api, oracle, pattern):
    M, N, IRP, JA, (A, _, _), x = pattern
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
    try:
        api.lib.spmvHipSetUnitValues(0)
        dm.update_values(np.full(JA.size, 3.0))
        assert api.lib.spmvHipUnitValue(C.byref(dm.handle), None) == 0
        assert_same_bits(_run(api, "hipSpMVRowsCSR", dm, x, M), oracle.csr_serial(IRP, JA, np.full(JA.size, 3.0), x))
    finally:
        dm.free()


def test_ell_handles(api, oracle, capfd):
    """Uploaded ELL, row-major and transposed, with and without row lengths: the host ELL values of the upload's layout
    go in, the ELL launchers compute them (the serial ones bit for bit, y_ref + 0.0); unit values are recognised where row
    lengths exist.  A derived handle (spmvHipCsrToEll) is refused with a message and computes what it did before."""
    rng = np.random.default_rng(515)
    M = N = 3000
    IRP, JA, A = random_csr(rng, M, N, rng.integers(0, 40, size=M))
    B = rng.uniform(-1, 1, size=JA.size)
    x = _x(rng, N)
    for rl in (True, False):
        for transposed in (False, True):
            ell = api.HostCSR(M, N, IRP, JA, A).to_ell(with_row_lens=rl)
            dm = api.spMatCpyELL(ell.transpose() if transposed else ell)
            launchers = (("hipSpMVRowsELL", True),) if transposed else \
                (("hipSpMVRowsELLNNTransposed", True), ("hipSpMVWarpsPerRowELLNTrasposed", False))
            try:
                for vals, step in ((B, "B"), (np.ones(JA.size), "ones"), (A, "A")):
                    new = api.HostCSR(M, N, IRP, JA, vals).to_ell(with_row_lens=rl)
                    dm.update_values((new.transpose() if transposed else new).AS)
                    assert api.lib.spmvHipUnitValue(C.byref(dm.handle), None) == (1 if rl and step == "ones" else 0)
                    y_ref = oracle.csr_serial(IRP, JA, vals, x)
                    for name, exact in launchers:
                        y = _run(api, name, dm, x, M)
                        assert not np.isnan(y).any() and np.max(np.abs(y - y_ref)) <= GATE, (name, rl, step)
                        if exact:
                            assert_same_bits(y, y_ref + 0.0, (name, rl, step))
            finally:
                dm.free()
    dcsr = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
    for transposed in (False, True):
        de = api.csr_to_ell_device(dcsr, transposed)
        name = "hipSpMVRowsELL" if transposed else "hipSpMVRowsELLNNTransposed"
        before = _run(api, name, de, x, M)
        capfd.readouterr()
        with pytest.raises(api.SpmvHipError):
            de.update_values(B)
        assert "spmvHipCsrToEll" in capfd.readouterr().err
        assert api.lib.spmvHipValuesChanged(C.byref(de.handle)) != 0
        assert_same_bits(_run(api, name, de, x, M), before)
        de.free()
    dcsr.free()


def test_sharded_handle_on_one_device(api, oracle, pattern, capfd):
    """spmvHipShardCSRGroups(host, 1, 3): the whole matrix's values go in, every row block takes its slice; both modes
    compute the new values (mode 0 bit for bit).  A freed shard handle is refused."""
    M, N, IRP, JA, (A, B, _), x = pattern
    host = api.HostCSR(M, N, IRP, JA, A)
    h = C.c_void_p()
    assert api.lib.spmvHipShardCSRGroups(C.byref(host.struct), 1, 3, C.byref(h)) == 0
    vp = C.c_void_p
    try:
        for vals, step in ((A, "A"), (B, "B")):
            if step == "B":
                Bc = np.ascontiguousarray(B)
                assert api.lib.spmvHipShardUpdateValues(h, Bc.ctypes.data_as(vp)) == 0
            y_ref = oracle.csr_serial(IRP, JA, vals, x)
            for mode in (0, 1):
                y = np.full(M, np.nan)
                assert api.lib.spmvHipSpMVSharded(h, x.ctypes.data_as(vp), mode, y.ctypes.data_as(vp), None, None) == 0
                if mode == 0:
                    assert_same_bits(y, y_ref, step)
                else:
                    assert tight_error(IRP, JA, vals, x, y_ref, y) <= TIGHT, step
    finally:
        api.lib.spmvHipShardFree(h)
    capfd.readouterr()
    assert api.lib.spmvHipShardUpdateValues(h, np.ascontiguousarray(A).ctypes.data_as(vp)) != 0
    assert "not a live shard" in capfd.readouterr().err
    assert api.lib.spmvHipShardUpdateValues(None, np.ascontiguousarray(A).ctypes.data_as(vp)) != 0


def test_captured_graph_replays_with_the_new_values(api, oracle, pattern):
    """A HIP graph of hipSpMVStripesCSR captured BEFORE an in-place update computes the new values when replayed after
    it: the format's arrays are rewritten at their addresses."""
    torch = pytest.importorskip("torch")
    M, N, IRP, JA, (A, B, _), x_host = pattern
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
    stream = torch.cuda.Stream()
    cfg = api.CONFIG()
    try:
        with torch.cuda.stream(stream):
            x = torch.from_numpy(x_host).cuda()
            y = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
            api.lib.spmvHipSetStream(C.c_void_p(stream.cuda_stream))
            api.lib.spmvHipSetSync(0)
            assert api.lib.hipSpMVStripesCSR(C.byref(dm.handle), x.data_ptr(), cfg, y.data_ptr()) == 0     # builds the format
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                assert api.lib.hipSpMVStripesCSR(C.byref(dm.handle), x.data_ptr(), cfg, y.data_ptr()) == 0
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            y_a = oracle.csr_serial(IRP, JA, A, x_host)
            assert tight_error(IRP, JA, A, x_host, y_a, y.cpu().numpy()) <= TIGHT
            dm.update_values(B)                              # on the library stream = the graph's stream
            info = dm.update_info()
            assert info.inPlace == 1 and info.mapsBuilt == 1
            y.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            y_b = oracle.csr_serial(IRP, JA, B, x_host)
            assert tight_error(IRP, JA, B, x_host, y_b, y.cpu().numpy()) <= TIGHT
    finally:
        api.lib.spmvHipSetStream(None)
        api.lib.spmvHipSetSync(1)
        dm.free()


def test_device_memory_comes_back_after_updates(api, oracle):
    """upload -> both selections -> every format in both forms -> three updates (value maps built) -> free: free device
    memory comes back every round (same tolerance as test_device_memory_comes_back; a map left behind is 6 MB here)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(2027)
    M = N = 200_000
    IRP, JA, A = random_csr(rng, M, N, rng.integers(0, 17, size=M))
    vals = [rng.uniform(-1, 1, size=JA.size) for _ in range(3)]
    x = _x(rng, N)
    free = []
    for _ in range(5):
        d = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
        _run(api, "hipSpMVRowsCSR", d, x, M)
        _run(api, "hipSpMVWarpPerRowCSR", d, x, M)
        for det in (False, True):
            api.build_tiles(d, deterministic=det)
        for mode in (0, 1):
            api.build_stripes(d, deterministic=mode)
        api.lib.spmvHipBuildSell(C.byref(d.handle))
        for v in vals:
            d.update_values(v)
        assert d.update_info().inPlace == 1
        assert_same_bits(_run(api, "hipSpMVRowsCSR", d, x, M), oracle.csr_serial(IRP, JA, vals[-1], x))
        d.free()
        api.spmvHipFinalize()
        api.spmvHipInit(0)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert min(free[2:]) >= free[1] - (8 << 20) and free[-1] >= free[1] - (8 << 20), free


def test_refusals_leave_the_handle_as_it_was(api, oracle, pattern, capfd):
    """NULL handle, NULL values, a freed handle, a derived ELL handle: EXIT_FAILURE with a message, and the live handle's
    next y is what it was."""
    M, N, IRP, JA, (A, B, _), x = pattern
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
    Bc = np.ascontiguousarray(B)
    vp = C.c_void_p
    try:
        api.build_stripes(dm, deterministic=1)
        before = _run(api, "hipSpMVStripesCSR", dm, x, M)
        assert_same_bits(before, oracle.csr_serial(IRP, JA, A, x))
        for call in (lambda: api.lib.spmvHipUpdateValues(None, Bc.ctypes.data_as(vp), 0),
                     lambda: api.lib.spmvHipUpdateValues(C.byref(dm.handle), None, 0),
                     lambda: api.lib.spmvHipValuesChanged(None),
                     lambda: api.lib.spmvHipLastUpdateInfo(C.byref(dm.handle), None)):
            capfd.readouterr()
            assert call() != 0
        gone = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
        gone.free()
        capfd.readouterr()
        assert api.lib.spmvHipUpdateValues(C.byref(gone.handle), Bc.ctypes.data_as(vp), 0) != 0
        assert "not a device handle" in capfd.readouterr().err
        e = api.csr_to_ell_device(dm, False)
        capfd.readouterr()
        assert api.lib.spmvHipUpdateValues(C.byref(e.handle), Bc.ctypes.data_as(vp), 0) != 0
        assert "spmvHipCsrToEll" in capfd.readouterr().err
        e.free()
        assert_same_bits(_run(api, "hipSpMVStripesCSR", dm, x, M), before)
        assert_same_bits(_run(api, "hipSpMVRowsCSR", dm, x, M), before)
    finally:
        dm.free()


def test_unsorted_and_repeated_columns(api, oracle):
    """Rows whose column ids are unsorted and repeat (a caller's own CSR): after an update hipSpMVRowsCSR is still
    bit-identical to sgemvSerial (its selection keeps to the j-order kernel there) and the format launchers agree with
    the oracle."""
    rng = np.random.default_rng(77)
    M = N = 50_000
    lens = rng.integers(2, 14, size=M)
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(lens)
    JA = rng.integers(0, N, size=int(IRP[-1])).astype(np.uint64)          # unsorted inside a row
    JA[1::7] = JA[0::7][:JA[1::7].size]                                    # and repeated
    A, B = rng.uniform(-1, 1, size=JA.size), rng.uniform(-1, 1, size=JA.size)
    x = _x(rng, N)
    dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, A))
    try:
        assert_same_bits(_run(api, "hipSpMVRowsCSR", dm, x, M), oracle.csr_serial(IRP, JA, A, x))
        for name in ("hipSpMVTilesCSR", "hipSpMVStripesCSR", "hipSpMVRowsSELL"):
            _run(api, name, dm, x, M)
        dm.update_values(B)
        y_ref = oracle.csr_serial(IRP, JA, B, x)
        assert_same_bits(_run(api, "hipSpMVRowsCSR", dm, x, M), y_ref)
        for name in ("hipSpMVWarpPerRowCSR", "hipSpMVTilesCSR", "hipSpMVStripesCSR", "hipSpMVRowsSELL"):
            assert tight_error(IRP, JA, B, x, y_ref, _run(api, name, dm, x, M)) <= TIGHT, name
    finally:
        dm.free()
