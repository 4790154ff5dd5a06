"""ILU(0) factorisation (hipSpILU0CSR): time per matrix and group width, against the serial loop of
spmvHip.h in C on one CPU thread, with a bitwise check of every record.

Per matrix and group width G (spmvHipSetVariant("hipSpILU0CSR", G)):
  levels, launches, longRows   spmvHipIlu0Info
  first_ms      the first call on a fresh handle: pattern check + lower analysis + factorisation + refresh, host wall time
  ms            a call with the schedule built, host wall time (the call is synchronous: it returns with the factors and
                the refreshed handle), median of 10 after a warm-up; the original values are put back before each call
                (spmvHipUpdateValues from a device copy, not timed)
  trsv_lower_ms hipSpTRSVCSR(LOWER, UNIT) on the factored handle (device events, median of 10), for scale
  cpu_ms        the loop in C (gcc -O2 -ffp-contract=off, one thread), median of 3
  cpu_equal_bits  the GPU's factors == the C loop's, every value, bit for bit
Kernel split: `rocprofv3 --kernel-trace --stats -- python scripts/ilu0_timing.py ...`.

    python scripts/ilu0_timing.py [--matrices lap7,stencil,chain,long] [--widths 8,16,64] [--out profiles/ilu0_timing.log]
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
from spmm_timing import Events, stencil  # noqa: E402
from test_trsv_abi import laplacian7  # noqa: E402

CPU_LOOP = r"""
#include <stdint.h>
#include <stdlib.h>
#include <time.h>
/* the loop of spmvHip.h: pos[c] = the position of column c in row i (or -1); dpos = the diagonal positions */
double ilu0(long M, const uint64_t* IRP, const uint32_t* JA, double* AS, const uint64_t* dpos, long N) {
    long* pos = malloc(N * sizeof(long));
    for (long c = 0; c < N; ++c) pos[c] = -1;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long i = 0; i < M; ++i) {
        for (uint64_t q = IRP[i]; q < IRP[i + 1]; ++q) pos[JA[q]] = (long)q;
        for (uint64_t p = IRP[i]; p < dpos[i]; ++p) {
            const long k = JA[p];
            AS[p] = AS[p] / AS[dpos[k]];
            for (uint64_t r = dpos[k] + 1; r < IRP[k + 1]; ++r) {
                const long q = pos[JA[r]];
                if (q >= 0) AS[q] = AS[q] - AS[p] * AS[r];
            }
        }
        for (uint64_t q = IRP[i]; q < IRP[i + 1]; ++q) pos[JA[q]] = -1;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    free(pos);
    return (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
}
"""


def cpu_lib(tmp):
    src, so = os.path.join(tmp, "ilu0_loop.c"), os.path.join(tmp, "ilu0_loop.so")
    open(src, "w").write(CPU_LOOP)
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    lib.ilu0.restype = C.c_double
    lib.ilu0.argtypes = [C.c_long] + [C.c_void_p] * 4 + [C.c_long]
    return lib


def with_diagonal(M, IRP, JA, AS):
    """sorted rows with exactly one diagonal entry each, dominant (sum of the row's |values| + 1): inserted where missing"""
    IRP = IRP.astype(np.int64)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    JA = JA.astype(np.int64)
    off = JA != rows
    rows, JA, AS = rows[off], JA[off], AS[off]
    dom = np.bincount(rows, weights=np.abs(AS), minlength=M) + 1.0
    rows, JA, AS = np.concatenate([rows, np.arange(M)]), np.concatenate([JA, np.arange(M)]), np.concatenate([AS, dom])
    o = np.lexsort((JA, rows))
    irp = np.zeros(M + 1, np.uint64)
    irp[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return irp, JA[o].astype(np.uint32), AS[o]


def lap7():
    IRP, JA, AS = laplacian7(500, 100, 100)
    rng = np.random.default_rng(3)
    AS = np.where(AS == 6.0, 6.0 + rng.random(AS.size), -rng.random(AS.size))     # values that round differently per order
    return "laplace7-500x100x100", 500 * 100 * 100, IRP.astype(np.uint64), JA.astype(np.uint32), AS


def stencil18():
    name, dm, IRP, JA, AS = stencil()
    M = int(dm.handle.M)
    dm.free()
    return name, M, *with_diagonal(M, IRP, JA, AS)


def chain(n):
    rng = np.random.default_rng(5)
    i = np.arange(n)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[1:] - 1, i, i[:-1] + 1])
    vals = np.where(rows == cols, 3.0 + rng.random(rows.size), rng.uniform(-1, 1, rows.size))
    o = np.lexsort((cols, rows))
    IRP = np.zeros(n + 1, np.uint64)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return f"chain-{n}", n, IRP, cols[o].astype(np.uint32), vals[o]


def long_rows():
    """the 7-point Laplacian 100 x 100 x 20 with 64 rows given 1 500 more lower columns each (rows longer than the 256
    entries a wavefront stages in LDS)"""
    IRP, JA, AS = laplacian7(100, 100, 20)
    M = 100 * 100 * 20
    rng = np.random.default_rng(11)
    rows = np.repeat(np.arange(M), np.diff(IRP.astype(np.int64)))
    extra_rows = np.sort(rng.choice(np.arange(M // 2, M), 64, replace=False))
    er = np.repeat(extra_rows, 1500)
    ec = (rng.random(er.size) * er).astype(np.int64)
    key = np.unique(np.concatenate([rows * M + JA.astype(np.int64), er * M + ec]))
    r, c = key // M, key % M
    vals = np.where(r == c, 0.0, -rng.random(r.size) / 8)
    IRP, JA, AS = with_diagonal(M, np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M))]), c, vals)
    return "laplace7-100x100x20+64x1500", M, IRP, JA, AS


def measure(name, M, IRP, JA, AS, G, ev, cpu, ref, out):
    api._check(api.lib.spmvHipSetVariant(b"hipSpILU0CSR", G), "variant")
    dm = api.spMatCpyCSR(api.HostCSR(M, M, IRP.astype(np.uint64), JA.astype(np.uint64), AS))
    orig = api.DeviceVector(AS.size).up(np.ascontiguousarray(AS))
    t0 = time.perf_counter()
    dm.ilu0()
    first_ms = (time.perf_counter() - t0) * 1e3
    ts = []
    for _ in range(11):
        dm.update_values(orig.ptr, on_device=True)
        t0 = time.perf_counter()
        info = dm.ilu0()
        ts.append((time.perf_counter() - t0) * 1e3)
    got = np.empty(AS.size)
    api._check(api.lib.spmvHipVecDown(got.ctypes.data_as(C.c_void_p), C.cast(dm.handle.AS, C.c_void_p), got.size), "down")
    b, x = api.DeviceVector(M).up(np.random.default_rng(7).uniform(-1, 1, M)), api.DeviceVector(M)
    api.lib.spmvHipSetSync(0)
    trsv = ev.median(lambda: api._check(api.lib.hipSpTRSVCSR(C.byref(dm.handle), 0, 1, b.ptr, x.ptr), "trsv"))
    api.lib.spmvHipSetSync(1)
    api._check(api.lib.spmvHipDeviceSynchronize(), "sync")
    tri = dm.triangular_info(True)
    rec = {"matrix": name, "G": G, "rows": M, "nnz": int(AS.size), "levels": info.levels, "launches": info.launches,
           "fusedLevels": tri.fusedLevels, "longRows": info.longRows, "zeroPivot": info.zeroPivot,
           "analyses": tri.analyses, "first_ms": round(first_ms, 3), "ms": round(float(np.median(ts[1:])), 3),
           "trsv_lower_ms": round(trsv, 4)}
    rec.update(ref)
    rec["cpu_equal_bits"] = bool(np.array_equal(got.view(np.uint64), ref.pop("_bits").view(np.uint64)))
    rec.pop("_bits", None)
    for v in (orig, b, x):
        v.free()
    dm.free()
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")
    out.flush()


def cpu_ref(cpu, M, IRP, JA, AS):
    rows = np.repeat(np.arange(M), np.diff(IRP.astype(np.int64)))
    dpos = np.flatnonzero(JA.astype(np.int64) == rows).astype(np.uint64)
    assert dpos.size == M
    irp, ja = IRP.astype(np.uint64), JA.astype(np.uint32)
    ts, a = [], None
    for _ in range(3):
        a = np.ascontiguousarray(AS, np.float64).copy()
        ts.append(cpu.ilu0(M, irp.ctypes.data, ja.ctypes.data, a.ctypes.data, dpos.ctypes.data, M))
    return {"cpu_ms": round(float(np.median(ts)), 3), "_bits": a}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="lap7,stencil,chain,long")
    ap.add_argument("--widths", default="8,16,64")
    ap.add_argument("--chain-rows", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ilu0_timing.log"))
    args = ap.parse_args()
    api.spmvHipInit(0)
    ev = Events()
    makers = {"lap7": lap7, "stencil": stencil18, "chain": lambda: chain(args.chain_rows), "long": long_rows}
    with tempfile.TemporaryDirectory() as tmp, open(args.out, "a") as out:
        cpu = cpu_lib(tmp)
        for key in args.matrices.split(","):
            name, M, IRP, JA, AS = makers[key]()
            ref = cpu_ref(cpu, M, IRP, JA, AS)
            for G in [int(g) for g in args.widths.split(",")]:
                measure(name, M, IRP, JA, AS, G, ev, cpu, dict(ref), out)
    api._check(api.lib.spmvHipSetVariant(b"hipSpILU0CSR", 16), "variant")
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
