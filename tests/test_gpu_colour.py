"""spmvHipColourCSR on the device: the colours are the bits of tests/colour_ref.py -- a function of the pattern and the
options alone -- for both orders and two seeds, on patterns that are empty, tiny, around a workgroup's size, one-directional,
without a diagonal, unsorted with repeats, past one 64-colour window and on the wavefront path, a chain whose rounds = M at
three values of K, and a grid of several workgroups."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as cr

pytestmark = pytest.mark.gpu

POISON = 0xA5A5A5A5
PAD = 7
NAME = "spmvHipColourCSR"


@pytest.fixture(scope="module")
def api():
    from spmv_openmp_cuda_amd import api as a
    a.spmvHipInit(0)
    yield a
    a.spmvHipFinalize()


@pytest.fixture(autouse=True)
def _defaults(api):
    yield
    api.set_variant(NAME, 16)


def _upload(api, M, IRP, JA):
    return api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, np.ones(JA.size)))


def _colour(api, dm, M, order, seed, want=(True, True)):
    """(colour, perm, info, tails): the outputs live in poisoned buffers PAD words longer than M"""
    bufs = [api.DeviceBuffer(4 * (M + PAD)).up(np.full(M + PAD, POISON, dtype=np.uint32)) if w else None for w in want]
    opts, info = api.spmvColourOpts(order, seed), api.spmvColourInfo()
    try:
        rc = api.lib.spmvHipColourCSR(C.byref(dm.handle), C.byref(opts), bufs[0].ptr if bufs[0] else None,
                                      bufs[1].ptr if bufs[1] else None, C.byref(info))
        got = [b.down(np.uint32) if b else None for b in bufs]
    finally:
        for b in bufs:
            if b:
                b.free()
    for g in got:
        if g is not None:
            assert np.all(g[M:] == POISON), "a word past M was written"
    return rc, got[0][:M] if want[0] else None, got[1][:M] if want[1] else None, info


def _check(api, M, IRP, JA, order, seed, ref=None, what=""):
    colour_ref, rounds_ref = ref if ref is not None else cr.colour_ref(M, IRP, JA, order, seed)
    dm = _upload(api, M, IRP, JA)
    try:
        rc, colour, perm, info = _colour(api, dm, M, order, seed)
        assert rc == 0, what
        assert np.array_equal(colour, colour_ref), what
        assert np.array_equal(perm, cr.perm_of(colour_ref)), what
        counts = np.bincount(colour_ref.astype(np.int64)) if M else np.zeros(1, dtype=np.int64)
        assert info.colours == (int(colour_ref.max()) + 1 if M else 0), what
        assert info.maxColourRows == (int(counts.max()) if M else 0), what
        print(f"{what}: colours {info.colours}, rounds {info.rounds} (reference {rounds_ref}), checks {info.hostChecks}, "
              f"long rows {info.longRows}, symmetric {info.symmetric}, {info.ms:.2f} ms")
        assert info.rounds <= rounds_ref                       # a colour seen in the round that wrote it only saves rounds
        if M:
            assert info.rounds >= 1 and info.hostChecks == -(-info.rounds // 16)
        rc2, colour2, perm2, _ = _colour(api, dm, M, order, seed)
        assert rc2 == 0 and np.array_equal(colour2, colour) and np.array_equal(perm2, perm), what + ": second run"
        for want in ((True, False), (False, True)):            # either output may be NULL
            rc3, c3, p3, i3 = _colour(api, dm, M, order, seed, want)
            assert rc3 == 0 and i3.colours == info.colours
            assert c3 is None or np.array_equal(c3, colour)
            assert p3 is None or np.array_equal(p3, perm)
        return info
    finally:
        dm.free()


SMALL = cr.small_cases()


@pytest.mark.parametrize("name", list(SMALL))
@pytest.mark.parametrize("order,seed", cr.CONFIGS)
def test_small_cases_equal_the_reference(api, name, order, seed):
    M, IRP, JA = SMALL[name]
    info = _check(api, M, IRP, JA, order, seed, what=f"{name} order {order} seed {seed:#x}")
    if name == "laplacian12x10x8":
        assert info.symmetric == 1 and info.longRows == 0
        if order == cr.NATURAL:
            assert info.colours == 2
    if name in ("bidiagonal", "no_diagonal"):
        assert info.symmetric == 0
    if name == "clique_star":
        assert info.colours >= 70 and info.longRows >= 70 and info.symmetric == 0


def test_opts_null_is_natural(api):
    M, IRP, JA = SMALL["laplacian12x10x8"]
    dm = _upload(api, M, IRP, JA)
    try:
        buf = api.DeviceBuffer(4 * M)
        info = api.spmvColourInfo()
        assert api.lib.spmvHipColourCSR(C.byref(dm.handle), None, buf.ptr, None, C.byref(info)) == 0
        assert np.array_equal(buf.down(np.uint32), cr.colour_ref(M, IRP, JA, cr.NATURAL)[0]) and info.colours == 2
        buf.free()
    finally:
        dm.free()


@pytest.fixture(scope="module")
def chain_ref():
    M, IRP, JA = cr.chain(5000)
    return M, IRP, JA, cr.colour_ref(M, IRP, JA, cr.NATURAL)


@pytest.mark.parametrize("K", [1, 16, 64])
def test_chain_rounds_and_host_checks(api, chain_ref, K):
    """NATURAL on a chain: every vertex waits for the one before it, M rounds; K changes the read-backs, not a colour"""
    M, IRP, JA, (colour_ref, rounds_ref) = chain_ref
    assert rounds_ref == M
    api.set_variant(NAME, K)
    dm = _upload(api, M, IRP, JA)
    try:
        rc, colour, perm, info = _colour(api, dm, M, cr.NATURAL, 0)
        assert rc == 0 and np.array_equal(colour, colour_ref) and np.array_equal(perm, cr.perm_of(colour_ref))
        print(f"K={K}: rounds {info.rounds}, checks {info.hostChecks}, {info.ms:.1f} ms")
        assert info.colours == 2 and info.maxColourRows == M // 2
        assert 1 <= info.rounds <= M and info.hostChecks == -(-info.rounds // K)
    finally:
        dm.free()


@pytest.mark.parametrize("order,seed", cr.CONFIGS)
def test_several_workgroups(api, order, seed):
    M, IRP, JA, _ = cr.laplacian7(64, 64, 16)
    info = _check(api, M, IRP, JA, order, seed, what=f"64x64x16 order {order} seed {seed:#x}")
    assert info.symmetric == 1
    if order == cr.NATURAL:
        assert info.colours == 2 and info.maxColourRows == M // 2


def test_python_colour(api):
    M, IRP, JA = SMALL["unsorted_repeats"]
    dm = _upload(api, M, IRP, JA)
    try:
        ref = cr.colour_ref(M, IRP, JA, cr.HASH, 5)[0]
        col = dm.colour(order="hash", seed=5, want_colours=True)
        assert np.array_equal(col.colours.down(np.uint32), ref) and np.array_equal(col.perm.down(np.uint32), cr.perm_of(ref))
        assert col.info.colours == int(ref.max()) + 1
        col.free()
        col = dm.colour()
        assert col.colours is None and np.array_equal(col.perm.down(np.uint32), cr.perm_of(cr.colour_ref(M, IRP, JA, cr.NATURAL)[0]))
        col.free()
        import torch
        col = dm.colour(order="hash", seed=5, want_colours=True, as_torch=True)
        assert col.perm.dtype == torch.int32 and np.array_equal(col.colours.cpu().numpy().view(np.uint32), ref)
        with pytest.raises(api.SpmvHipError):
            dm.colour(order="rcm")
    finally:
        dm.free()


def test_refusals_leave_outputs_untouched(api, capfd):
    M, IRP, JA = SMALL["random257"]
    dm = _upload(api, M, IRP, JA)
    rect = api.spMatCpyCSR(api.HostCSR(3, 4, np.array([0, 1, 2, 3], dtype=np.uint64), np.array([0, 1, 3], dtype=np.uint64), np.ones(3)))
    ell = api.csr_to_ell_device(dm, False)
    bufs = [api.DeviceBuffer(4 * M).up(np.full(M, POISON, dtype=np.uint32)) for _ in range(2)]
    info = api.spmvColourInfo()
    info.colours = 77
    try:
        bad_order = api.spmvColourOpts(2, 0)
        good = api.spmvColourOpts(cr.HASH, 0)
        empty = api.spmat()
        for handle, opts in ((dm.handle, bad_order), (rect.handle, good), (ell.handle, good), (empty, good)):
            assert api.lib.spmvHipColourCSR(C.byref(handle), C.byref(opts), bufs[0].ptr, bufs[1].ptr, C.byref(info)) == 1
        assert api.lib.spmvHipColourCSR(None, C.byref(good), bufs[0].ptr, bufs[1].ptr, C.byref(info)) == 1
        assert info.colours == 77
        for b in bufs:
            assert np.all(b.down(np.uint32) == POISON)
        assert api.lib.spmvHipSetVariant(NAME.encode(), 0) == 1 and api.lib.spmvHipSetVariant(NAME.encode(), 4097) == 1
        assert "unknown order" in capfd.readouterr().err
    finally:
        for b in bufs:
            b.free()
        for d in (ell, rect, dm):
            d.free()
