"""The allocation chokepoint (devMalloc / devFree over csrc/hip/alloc_ledger.hpp) and its two entry points for tests,
spmvHipAllocRefuse and spmvHipAllocStats: declared, exported, bound in Python with the C layout; no file of the library
calls the runtime's allocator beside the chokepoint; and the ledger itself, compiled for the CPU over malloc / free under
AddressSanitizer + UBSan (tests/harness/alloc_ledger_check.cpp), keeps its counters, refuses the n-th allocation or every
one from the n-th on, re-arms, and counts a second and a foreign release.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

import c_header
from c_header import HEADER, code as _code
from conftest import ROOT

LIB = os.path.join(ROOT, "spmv_openmp_cuda_amd", "lib", "libspmvhip.so")
HIP_DIR = os.path.join(ROOT, "spmv_openmp_cuda_amd", "csrc", "hip")
DECLS = {
    "spmvHipAllocRefuse": (r"long\s+\w+\s*,\s*int\s+\w+", 2),
    "spmvHipAllocStats": (r"spmvAllocStats\s*\*\s*\w+", 1),
}
STRUCTS = {"spmvAllocStats": ("live", "liveBytes", "peakBytes", "calls", "refused", "badFrees")}


def test_header_declares_the_entry_points_and_the_struct_as_for_tests():
    code = _code(HEADER)
    for name, (params, nargs) in DECLS.items():
        assert re.search(r"^\s*int\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code, re.M), name
        assert c_header.prototypes()[name] == nargs
    for struct, fields in STRUCTS.items():
        assert c_header.structs()[struct] == list(fields), struct
    text = open(HEADER).read()
    comment = text[:text.index("} spmvAllocStats;")].rsplit("/*", 1)[1]
    assert "exist for tests" in comment and "environment variable" in comment


def test_library_exports_them():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DECLS:
        assert name in syms, name


def test_python_binds_them_with_the_c_layout(tmp_path):
    import inspect
    from spmv_openmp_cuda_amd import api
    for name, (_, nargs) in DECLS.items():
        assert name in api._sigs and len(getattr(api.lib, name).argtypes) == nargs, name
    assert api.lib.spmvHipAllocRefuse.argtypes[0] is C.c_long
    body = ""
    for name, fields in STRUCTS.items():
        body += f'    printf("{name} %zu", sizeof({name}));\n'
        body += "".join(f'    printf(" %zu", offsetof({name}, {f}));\n' for f in fields) + '    printf("\\n");\n'
    layout = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in c_header.run_c(tmp_path, body, "alloc_layout").splitlines()}
    for struct, fields in STRUCTS.items():
        py = getattr(api, struct)
        assert [f[0] for f in py._fields_] == list(fields)
        assert layout[struct] == [C.sizeof(py)] + [getattr(py, f).offset for f in fields], struct
    assert list(inspect.signature(api.alloc_refuse).parameters) == ["n", "from_then_on"]
    assert inspect.signature(api.alloc_refuse).parameters["n"].default == -1
    assert list(inspect.signature(api.alloc_refused).parameters) == ["n", "from_then_on"]
    assert callable(api.alloc_stats)


def test_the_ledger_counts_before_the_library_is_initialised():
    """neither call needs a device: the counters read, arming resets calls and refused, the context manager always disarms"""
    from spmv_openmp_cuda_amd import api
    st = api.alloc_stats()
    assert st.badFrees == 0 and st.refused == 0
    with pytest.raises(ZeroDivisionError):
        with api.alloc_refused(0, from_then_on=True):
            1 / 0
    after = api.alloc_stats()
    assert (after.calls, after.refused) == (0, 0) and (after.live, after.liveBytes) == (st.live, st.liveBytes)


def test_no_file_of_the_library_allocates_beside_the_chokepoint():
    """`hipMalloc(` and `hipFree(` appear in csrc/hip exactly once each: in the two backend functions of the ledger in abi.hip
    (hipMallocAsync, hipHostMalloc, hipFreeSpmat and the IPC open / close of peer.hip are other words)"""
    found = []
    files = sorted(glob.glob(os.path.join(HIP_DIR, "*.hip")) + glob.glob(os.path.join(HIP_DIR, "*.hpp")))
    assert len(files) > 30
    for path in files:
        text = re.sub(r"//[^\n]*", "", open(path).read())           # code only: a comment may name the runtime's calls
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        for m in re.finditer(r"\b(hipMalloc|hipFree)\s*\(", text):
            found.append((os.path.basename(path), m.group(1)))
    assert sorted(found) == [("abi.hip", "hipFree"), ("abi.hip", "hipMalloc")], found
    abi = open(os.path.join(HIP_DIR, "abi.hip")).read()
    assert re.search(r"hipError_t devMalloc\(void\*\* p, size_t bytes\) \{ return \(hipError_t\)ledger\(\)\.allocate\(p, bytes\); \}", abi)
    assert re.search(r"hipError_t devFree\(void\* p\) \{ return \(hipError_t\)ledger\(\)\.release\(p\); \}", abi)
    ledger = open(os.path.join(HIP_DIR, "alloc_ledger.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", ledger)), "the ledger includes nothing of HIP"
    assert "getenv" not in abi and "getenv" not in ledger, "armed through the ABI and through nothing else"


def test_the_ledger_under_sanitizers_on_the_cpu(tmp_path):
    """tests/harness/alloc_ledger_check.cpp: the ledger over malloc / free, built with AddressSanitizer + UBSan"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode:
        pytest.skip("this g++ has no sanitizer runtimes")
    r = subprocess.run(["make", "-s", "ledger"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests/harness/alloc_ledger_check.elf")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert r.stdout.strip().splitlines()[-1] == "alloc_ledger_check OK"
