"""Triangular solves (hipSpTRSVCSR): schedule, analysis time and solve time per matrix, against
hipSpMVRowsCSR on the same handle and a single-threaded C loop on the CPU.

Per matrix and triangle:
  levels, maxLevelRows, launches, fusedLevels, longRows   spmvHipTriInfo after the analysis
  analysis_ms   spmvHipTriAnalyse, host wall time (it returns with the schedule complete)
  solve_ms      hipSpTRSVCSR, device events around the enqueued solve, median of 10 after a warm-up
  spmv_ms       hipSpMVRowsCSR on the same handle, the same way
  cpu_ms        the serial loop of spmvHip.h in C (gcc -O2, one thread), median of 3
  check_bitwise the solve == the test side's level-vectorised reference (tests/trsv_ref.py), where --check names it
The run threshold T is swept with --T (spmvHipSetVariant("hipSpTRSVCSR", T), set before each analysis).
Kernel split: `rocprofv3 --kernel-trace --stats -- python scripts/trsv_timing.py ...`.

    python scripts/trsv_timing.py [--matrices lap7,stencil,c2,chain,road] [--T 256] [--out profiles/trsv_timing.log]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from spmv_openmp_cuda_amd import api  # noqa: E402
from spmm_timing import Events, stencil, synthetic  # noqa: E402
from trsv_ref import trsv_levels  # noqa: E402
from test_trsv_abi import laplacian7  # noqa: E402

CPU_LOOP = r"""
#include <stdint.h>
#include <time.h>
double trsv(long M, const uint64_t* IRP, const uint32_t* JA, const double* AS, const double* b, double* x, int lower, int unit) {
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long k = 0; k < M; ++k) {
        const long i = lower ? k : M - 1 - k;
        double acc = 0.0, d = 1.0;
        for (uint64_t p = IRP[i]; p < IRP[i + 1]; ++p) {
            const long j = JA[p];
            if (lower ? j < i : j > i) acc += AS[p] * x[j];
            else if (j == i) d = AS[p];
        }
        x[i] = unit ? b[i] - acc : (b[i] - acc) / d;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    return (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
}
"""


def cpu_lib(tmp):
    src, so = os.path.join(tmp, "trsv_loop.c"), os.path.join(tmp, "trsv_loop.so")
    open(src, "w").write(CPU_LOOP)
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    lib.trsv.restype = C.c_double
    lib.trsv.argtypes = [C.c_long] + [C.c_void_p] * 5 + [C.c_int, C.c_int]
    return lib


def upload(M, IRP, JA, AS):
    return api.spMatCpyCSR(api.HostCSR(M, M, IRP.astype(np.uint64), JA.astype(np.uint64), AS))


def road(n):
    """the road stand-in of bench.py (kind 1) at n rows: generated file -> MMtoCSR -> upload"""
    path = os.path.join("/dev/shm" if os.access("/dev/shm", os.W_OK) else ROOT, f"trsv_timing_{os.getpid()}.mtx")
    Mv, NZv, mxv = C.c_ulong(), C.c_ulong(), C.c_ulong()
    try:
        api._check(api.hostlib.spmvSynthWriteMtx(path.encode(), 1, n, 0, 0, 0x57A7, C.byref(Mv), C.byref(NZv), C.byref(mxv)),
                   "spmvSynthWriteMtx")
        csr = api.hostlib.MMtoCSR(path.encode())
    finally:
        if os.path.exists(path):
            os.remove(path)
    m = csr.contents
    M, nnz = int(m.M), int(m.NZ)
    irp = np.ctypeslib.as_array(m.IRP, shape=(M + 1,)).astype(np.uint64)
    ja = np.ctypeslib.as_array(m.JA, shape=(nnz,)).astype(np.uint32)
    as_ = np.ctypeslib.as_array(m.AS, shape=(nnz,)).copy()
    dm = api.DeviceMatrix()
    api._check(api.lib.spMatCpyCSR(csr, C.byref(dm.handle)), "spMatCpyCSR")
    api.hostlib.freeSpmat(csr)
    return f"road-{n}", dm, irp, ja, as_


def chain(n):
    rng = np.random.default_rng(5)
    i = np.arange(n)
    IRP = np.zeros(n + 1, np.uint64)
    IRP[1:] = np.cumsum(np.where(i > 0, 2, 1))
    JA = np.stack([np.maximum(i - 1, 0), i], 1).reshape(-1)
    AS = np.stack([rng.uniform(-1, 1, n), 1 + rng.random(n)], 1).reshape(-1)
    keep = np.ones(2 * n, bool)
    keep[0] = False
    JA, AS = JA[keep], AS[keep]
    return f"chain-{n}", upload(n, IRP, JA, AS), IRP, JA.astype(np.uint32), AS


def lap7():
    IRP, JA, AS = laplacian7(500, 100, 100)
    M = 500 * 100 * 100
    return "laplace7-500x100x100", upload(M, IRP, JA, AS), IRP, JA.astype(np.uint32), AS


def measure(name, dm, IRP, JA, AS, tri, T, ev, cpu, check, out):
    M = int(dm.handle.M)
    lower, unit = tri
    uplo = 0 if lower else 1
    api._check(api.lib.spmvHipSetVariant(b"hipSpTRSVCSR", T), "variant")
    rng = np.random.default_rng(7)
    b = rng.uniform(-1, 1, M)
    db, dx, dy = api.DeviceVector(M).up(b), api.DeviceVector(M), api.DeviceVector(M)
    t0 = time.perf_counter()
    dm.triangular_analyse(lower)
    analysis_ms = (time.perf_counter() - t0) * 1e3
    info = dm.triangular_info(lower)
    api.lib.spmvHipSetSync(0)
    solve = ev.median(lambda: api._check(api.lib.hipSpTRSVCSR(C.byref(dm.handle), uplo, int(unit), db.ptr, dx.ptr), "trsv"))
    spmv = ev.median(lambda: api._check(api.lib.hipSpMVRowsCSR(C.byref(dm.handle), db.ptr, api.CONFIG(), dy.ptr), "spmv"))
    api.lib.spmvHipSetSync(1)
    api._check(api.lib.spmvHipDeviceSynchronize(), "sync")
    x = dx.down()
    rec = {"matrix": name, "triangle": "lower" if lower else "upper", "diag": "unit" if unit else "stored", "T": T,
           "rows": M, "nnz": int(dm.handle.NZ), "levels": info.levels, "maxLevelRows": info.maxLevelRows,
           "launches": info.launches, "fusedLevels": info.fusedLevels, "longRows": info.longRows,
           "analysis_ms": round(analysis_ms, 3), "analysis_lib_ms": round(info.analysisMs, 3), "solve_ms": round(solve, 4),
           "spmv_ms": round(spmv, 4), "schedule_bytes": info.bytes}
    if info.fusedLevels and info.launches == 1:
        rec["us_per_fused_level"] = round(solve * 1e3 / info.fusedLevels, 3)
        rec["analysis_us_per_level"] = round(analysis_ms * 1e3 / info.levels, 3)
    if cpu is not None:
        xc = np.empty(M)
        irp, ja, a = IRP.astype(np.uint64), JA.astype(np.uint32), np.ascontiguousarray(AS, np.float64)
        ts = [cpu.trsv(M, irp.ctypes.data, ja.ctypes.data, a.ctypes.data, b.ctypes.data, xc.ctypes.data, int(lower), int(unit))
              for _ in range(3)]
        rec["cpu_ms"] = round(float(np.median(ts)), 3)
        rec["cpu_equal_bits"] = bool(np.array_equal(xc.view(np.uint64), x.view(np.uint64)))
    if check:
        ref = trsv_levels(M, IRP, JA, AS, b, lower, unit)
        rec["check_bitwise"] = bool(np.array_equal(ref.view(np.uint64), x.view(np.uint64)))
    for v in (db, dx, dy):
        v.free()
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="lap7,stencil,c2,chain,road")
    ap.add_argument("--T", default="256")
    ap.add_argument("--check", default="lap7,stencil")
    ap.add_argument("--road-rows", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trsv_timing.log"))
    args = ap.parse_args()
    api.spmvHipInit(0)
    ev = Events()
    Ts = [int(t) for t in args.T.split(",")]
    with tempfile.TemporaryDirectory() as tmp, open(args.out, "a") as out:
        cpu = cpu_lib(tmp)
        for key in args.matrices.split(","):
            if key == "lap7":
                name, dm, IRP, JA, AS = lap7()
                tris = [(True, False), (False, False)]
            elif key == "stencil":
                name, dm, IRP, JA, AS = stencil()
                tris = [(True, True), (False, True)]
            elif key == "c2":
                name, dm, IRP, JA, AS = synthetic("c2")
                tris = [(True, True)]
            elif key == "chain":
                name, dm, IRP, JA, AS = chain(100_000)
                tris = [(True, False)]
            elif key == "road":
                name, dm, IRP, JA, AS = road(args.road_rows)
                tris = [(True, True)]
            else:
                raise SystemExit(f"unknown matrix {key}")
            for tri in tris:
                for T in Ts:
                    dm_t = dm
                    if T != Ts[0]:                                 # a fresh schedule for every T
                        dm_t = upload(int(dm.handle.M), IRP, JA, AS)
                    measure(name, dm_t, IRP, JA, AS, tri, T, ev, cpu, key in args.check.split(",") and T == Ts[0], out)
                    if dm_t is not dm:
                        dm_t.free()
            dm.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
