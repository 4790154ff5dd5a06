"""spmvHipRcmCSR is declared, exported and bound in Python with the C layout of spmvRcmOpts / spmvRcmInfo, and the test
side's reference (tests/rcm_ref.py) is the loop of include/spmvHip.h: the level-synchronous implementation equals the
plain-Python queue loop on every small case and on seeded random graphs, facts computed with that loop are pinned, and
three planted faults each change the permutation of a pinned small graph.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import rcm_ref as rr
from c_header import HEADER, code as _code
from conftest import ROOT

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
NAME = "spmvHipRcmCSR"
PARAMS = r"spmat\s*\*\s*\w+\s*,\s*const\s+spmvRcmOpts\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*spmvRcmInfo\s*\*\s*\w+"
OPTS = ("start", "maxPasses", "forward")
INFO = ("components", "levels", "startBfs", "maxFrontier", "longRows", "symmetric", "bandwidthBefore", "bandwidthAfter", "launches",
        "hostChecks", "ms")
CASES = rr.small_cases()
PASSES = (0, 1, 2, 8)


def test_header_declares_the_call_the_structs_and_the_defines():
    code = _code(HEADER)
    assert re.search(r"^\s*int\s+" + NAME + r"\s*\(\s*" + PARAMS + r"\s*\)\s*;", code, re.M)
    for struct, fields in (("spmvRcmOpts", OPTS), ("spmvRcmInfo", INFO)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code, re.S)
        assert body and re.findall(r"(\w+)\s*;", body.group(1)) == list(fields), struct
    assert re.search(r"#define\s+SPMV_RCM_START_MIN_DEGREE\s+0\b", code) and re.search(r"#define\s+SPMV_RCM_START_PERIPHERAL\s+1\b", code)
    text = open(HEADER).read()
    for line in ("r = the unvisited vertex of smallest (deg, id)", "perm = order reversed as a whole",
                 "if depth(Lv) > depth(L): r = v; L = Lv"):
        assert line in text, "the loop is written out in the header"


def test_library_exports_it():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert NAME in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_python_binds_it_with_the_c_layout():
    import inspect
    from spmv_openmp_cuda_amd import api
    assert NAME in api._sigs and len(getattr(api.lib, NAME).argtypes) == 4
    assert [f[0] for f in api.spmvRcmOpts._fields_] == list(OPTS)
    assert [f[0] for f in api.spmvRcmInfo._fields_] == list(INFO)
    assert (api.SPMV_RCM_START_MIN_DEGREE, api.SPMV_RCM_START_PERIPHERAL) == (rr.MIN_DEGREE, rr.PERIPHERAL)
    sig = inspect.signature(api.DeviceMatrix.rcm).parameters
    assert list(sig)[1:] == ["start", "max_passes", "forward", "as_torch"]
    assert (sig["start"].default, sig["max_passes"].default, sig["forward"].default, sig["as_torch"].default) == ("peripheral", 0, False, False)
    assert callable(api.Ordering.free)


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_references_agree_on_the_small_cases(name):
    M, IRP, JA = CASES[name]
    for start, forward in rr.CONFIGS:
        for passes in ((0, 1) if name == "path3000" else PASSES):
            a, ia = rr.rcm_loop(M, IRP, JA, start, passes, forward)
            b, ib = rr.rcm_levels(M, IRP, JA, start, passes, forward)
            assert np.array_equal(a, b) and ia == ib, (name, start, forward, passes)
            assert np.array_equal(np.sort(a), np.arange(M))
    assert np.array_equal(rr.rcm_loop(M, IRP, JA, forward=True)[0][::-1], rr.rcm_loop(M, IRP, JA)[0])


@pytest.mark.parametrize("seed", range(12))
def test_the_two_references_agree_on_random_graphs(seed):
    rng = np.random.default_rng(7000 + seed)
    M = int(rng.integers(2, 120))
    edges = int(rng.integers(0, 3 * M))
    M, IRP, JA = rr.from_edges(M, rng.integers(0, M, edges), rng.integers(0, M, edges))
    for start, forward in rr.CONFIGS:
        for passes in PASSES:
            a, ia = rr.rcm_loop(M, IRP, JA, start, passes, forward)
            b, ib = rr.rcm_levels(M, IRP, JA, start, passes, forward)
            assert np.array_equal(a, b) and ia == ib, (seed, start, forward, passes)


def test_pinned_facts_of_the_loop():
    M, IRP, JA = CASES["path3000"]
    perm, info = rr.rcm_loop(M, IRP, JA)
    assert rr.bandwidth(M, IRP, JA) > 2000 and rr.bandwidth(M, IRP, JA, perm) == 1
    assert (info["components"], info["levels"], info["maxFrontier"]) == (1, 3000, 1)
    for name, want in (("grid40x30", 30), ("grid12x10x8", 75)):
        M, IRP, JA = CASES[name]
        for passes in PASSES:
            perm, info = rr.rcm_loop(M, IRP, JA, rr.PERIPHERAL, passes)
            assert rr.bandwidth(M, IRP, JA, perm) == want, (name, passes)
            assert info["startBfs"] == 2, "the corner, then the opposite corner, which is no deeper"
    M, IRP, JA = CASES["three_components"]
    assert rr.rcm_loop(M, IRP, JA)[1]["components"] == 9, "6 isolated vertices and the three"


@pytest.mark.parametrize("fault", rr.FAULTS)
def test_a_planted_fault_changes_the_permutation(fault):
    M, IRP, JA = CASES["three_components"]
    good = rr.rcm_levels(M, IRP, JA)[0]
    assert np.array_equal(good, rr.rcm_loop(M, IRP, JA)[0])
    bad = rr.rcm_levels(M, IRP, JA, fault=fault)[0]
    assert np.array_equal(np.sort(bad), np.arange(M)) and not np.array_equal(bad, good), fault
