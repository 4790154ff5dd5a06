"""The block-of-vectors entry point (hipSpMMRowsCSR) is declared with its layout constants, exported and bound in Python
(no compute calls: runs without a GPU)."""
import os
import re
import subprocess

from c_header import HEADER, code as _code
from conftest import ROOT

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")


def test_header_declares_spmm_and_layouts():
    code = _code(HEADER)
    assert re.search(r"^\s*int\s+hipSpMMRowsCSR\s*\(\s*spmat\s*\*\s*\w+\s*,\s*unsigned\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
                     r"\s*size_t\s+\w+\s*,\s*int\s+\w+\s*,\s*double\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", code, re.M)
    assert re.search(r"^#define\s+SPMV_DENSE_ROW_MAJOR\s+0\b", code, re.M)
    assert re.search(r"^#define\s+SPMV_DENSE_COL_MAJOR\s+1\b", code, re.M)


def test_library_exports_spmm():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert "hipSpMMRowsCSR" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_python_binds_spmm():
    from spmv_openmp_cuda_amd import api
    assert "hipSpMMRowsCSR" in api._sigs
    assert len(api.lib.hipSpMMRowsCSR.argtypes) == 8
    assert (api.SPMV_DENSE_ROW_MAJOR, api.SPMV_DENSE_COL_MAJOR) == (0, 1)
    assert callable(api.DeviceMatrix.matmul)
