"""spmvHipColourCSR, spmvHipCsrPermute, spmvHipPermuteRefresh and spmvHipVecPermute are declared, exported and bound in
Python with the C layout of spmvColourOpts / spmvColourInfo, and the test side's reference (tests/colour_ref.py) is the
loop of include/spmvHip.h: the numpy rounds equal the plain-Python loop on every small case, every result is a proper
colouring of A + A^T, the level sets of the permuted matrix number at most the colours, the fmix32 constants are pinned,
and a planted fault (ignoring the incoming edges) is caught.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import colour_ref as cr
from c_header import HEADER, code as _code
from conftest import ROOT
from trsv_ref import levels

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
U32 = r"uint32_t\s*\*\s*\w+"
DECLS = {
    "spmvHipColourCSR": (r"spmat\s*\*\s*\w+\s*,\s*const\s+spmvColourOpts\s*\*\s*\w+\s*,\s*" + U32 + r"\s*,\s*" + U32 +
                         r"\s*,\s*spmvColourInfo\s*\*\s*\w+", 5),
    "spmvHipCsrPermute": (r"spmat\s*\*\s*\w+\s*,\s*const\s+" + U32 + r"\s*,\s*spmat\s*\*\s*\w+", 3),
    "spmvHipPermuteRefresh": (r"spmat\s*\*\s*\w+\s*,\s*spmat\s*\*\s*\w+", 2),
    "spmvHipVecPermute": (r"size_t\s+\w+\s*,\s*const\s+" + U32 + r"\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*int\s+\w+", 5),
}
OPTS = ("order", "seed")
INFO = ("colours", "rounds", "hostChecks", "maxColourRows", "longRows", "symmetric", "ms")
CASES = cr.small_cases()


def test_header_declares_the_four_and_the_structs():
    code = _code(HEADER)
    for name, (params, _) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
    for struct, fields in (("spmvColourOpts", OPTS), ("spmvColourInfo", INFO)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body and re.findall(r"(\w+)\s*;", body.group(1)) == list(fields), struct
    assert re.search(r"#define\s+SPMV_COLOUR_NATURAL\s+0\b", code) and re.search(r"#define\s+SPMV_COLOUR_HASH\s+1\b", code)


def test_library_exports_the_four():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_the_four():
    from spmv_openmp_cuda_amd import api
    for name, (_, nargs) in DECLS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == nargs, name
    for m in ("colour", "permute", "permute_refresh"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    assert callable(api.permute_vector)
    assert [f[0] for f in api.spmvColourOpts._fields_] == list(OPTS)
    assert [f[0] for f in api.spmvColourInfo._fields_] == list(INFO)
    assert (api.SPMV_COLOUR_NATURAL, api.SPMV_COLOUR_HASH) == (cr.NATURAL, cr.HASH)


def test_fmix32_constants():
    assert [cr.fmix32(v) for v in (1, 2, 0xDEADBEEF)] == [0x514E28B7, 0x30F4C306, 0x0DE5C6A9]
    assert cr.fmix32(0) == 0
    v = np.array([1, 2, 0xDEADBEEF, 12345], dtype=np.uint64)
    assert [int(a) for a in cr.fmix32_np(v)] == [cr.fmix32(int(a)) for a in v]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("order,seed", cr.CONFIGS)
def test_ref_is_the_loop_and_proper(name, order, seed):
    M, IRP, JA = CASES[name]
    colour, rounds = cr.colour_ref(M, IRP, JA, order, seed)
    assert np.array_equal(colour, cr.colour_loop(M, IRP, JA, order, seed)), name
    assert cr.is_proper(M, IRP, JA, colour), name
    perm = cr.perm_of(colour)
    assert np.array_equal(np.sort(perm), np.arange(M))
    assert np.all(np.diff(colour[perm].astype(np.int64)) >= 0)
    if M == 0:
        return
    colours = int(colour.max()) + 1
    irp, ja, _, _ = cr.permute_ref(M, IRP, JA, np.zeros(JA.size), perm)
    for lower in (True, False):
        assert int(levels(M, irp, ja, lower).max()) + 1 <= colours, (name, lower)
    assert rounds >= colours


def test_natural_is_red_black_on_the_laplacian():
    M, IRP, JA = CASES["laplacian12x10x8"]
    colour, rounds = cr.colour_ref(M, IRP, JA, cr.NATURAL)
    assert int(colour.max()) + 1 == 2 and rounds == 12 + 10 + 8 - 2
    irp, ja, _, _ = cr.permute_ref(M, IRP, JA, np.zeros(JA.size), cr.perm_of(colour))
    assert int(levels(M, irp, ja, True).max()) + 1 == 2 and int(levels(M, irp, ja, False).max()) + 1 == 2
    assert int(levels(M, IRP, JA, True).max()) + 1 == 28


def test_chain_takes_m_rounds():
    M, IRP, JA = cr.chain(300)
    colour, rounds = cr.colour_ref(M, IRP, JA, cr.NATURAL)
    assert rounds == M and np.array_equal(colour, np.arange(M) % 2)


def test_ignoring_incoming_edges_is_caught():
    """row i stores (i, i-1) only: under HASH some i-1 loses against i, and sees i only through the transposed pattern"""
    M, IRP, JA = CASES["bidiagonal"]
    caught = []
    for order, seed in cr.CONFIGS:
        good = cr.colour_loop(M, IRP, JA, order, seed)
        bad = cr.colour_loop(M, IRP, JA, order, seed, incoming=False)
        assert cr.is_proper(M, IRP, JA, good)
        if not cr.is_proper(M, IRP, JA, bad):
            caught.append((order, seed))
    assert (cr.HASH, 0) in caught, caught


def test_permute_ref_keeps_stored_order_of_repeats():
    M, IRP, JA = CASES["unsorted_repeats"]
    AS = np.arange(JA.size, dtype=np.float64)
    perm = np.random.default_rng(3).permutation(M)
    irp, ja, a, mp = cr.permute_ref(M, IRP, JA, AS, perm)
    assert np.array_equal(a, AS[mp])
    for r in range(M):
        cols, src = ja[irp[r]:irp[r + 1]], mp[irp[r]:irp[r + 1]].astype(np.int64)
        assert np.all(np.diff(cols.astype(np.int64)) >= 0)
        same = np.flatnonzero(np.diff(cols.astype(np.int64)) == 0)
        assert np.all(src[same] < src[same + 1]), r
        assert np.all((src >= int(IRP[perm[r]])) & (src < int(IRP[perm[r] + 1])))
