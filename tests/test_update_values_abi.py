"""The value-update entry points (spmvHipUpdateValues and friends) are declared, exported and bound in Python
(no compute calls: runs without a GPU)."""
import os
import re
import subprocess

from c_header import HEADER, code as _code
from conftest import ROOT

NAMES = ("spmvHipUpdateValues", "spmvHipValuesChanged", "spmvHipLastUpdateInfo", "spmvHipShardUpdateValues")
LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")


def test_header_declares_the_update_functions():
    code = _code(HEADER)
    for n in NAMES:
        assert re.search(r"^\s*int\s+" + n + r"\s*\(", code, re.M), n
    # the info struct, with the fields the contract documents
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spmvUpdateInfo\s*;", code, re.S)
    assert m, "spmvUpdateInfo"
    for field in ("inPlace", "rebuilt", "mapsBuilt", "unitBefore", "unitAfter", "ms", "mapMs"):
        assert re.search(r"\b" + field + r"\b", m.group(1)), field


def test_header_states_the_adopt_snapshot_contract():
    text = open(HEADER).read()
    adopt = text[:text.index("int spmvHipAdoptCSR(")]
    comment = adopt[adopt.rindex("/*"):]
    assert "spmvHipValuesChanged" in comment and "snapshot" in comment.lower()


def test_library_exports_the_update_functions():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [n for n in NAMES if n not in exported]
    assert not missing, f"libspmvhip.so does not export {missing}"


def test_python_binds_the_update_functions():
    from spmv_openmp_cuda_amd import api
    for n in NAMES:
        assert n in api._sigs, n
        assert getattr(api.lib, n).argtypes, n
    for m in ("update_values", "values_changed", "update_info"):
        assert callable(getattr(api.DeviceMatrix, m)), m
    # the ctypes mirror has the C layout: five ints, then two doubles on their 8-byte alignment
    assert api.spmvUpdateInfo.ms.offset == 24 and api.spmvUpdateInfo.mapMs.offset == 32
