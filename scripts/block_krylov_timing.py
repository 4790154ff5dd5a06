"""Block Krylov solves (hipSpCGBlockCSR, hipSpBiCGStabBlockCSR): time per iteration for k = 1 .. 32
right-hand sides on the 500 x 100 x 100 7-point Laplacian (CG, ILU(0)-PCG) and the upwind convection-diffusion stencil of
the same size (BiCGStab, ILU(0)-BiCGStab), row-major B and X, against the yardstick taken in the same run on the same
handles: k times the per-iteration time of hipSpCGCSR / hipSpBiCGStabCSR.

Records (one JSON line each):
  single       ms per iteration of the single solve = (solve(maxIter = n2) - solve(maxIter = n1)) / (n2 - n1) at tol = 0,
               device events around the synchronous call, median of 3 (the method of scripts/krylov_timing.py)
  parts        hipSpMMRowsCSR, hipSpTRSMCSR lower / upper on the ILU(0) handle and spmvHipBlockDot at k = 16, row-major,
               device events, median of 10 (the fused passes one by one: the kernel trace, see below)
  block        the same difference quotient for the block solve at k columns; yardstick_ms = k * the single record;
               speedup = yardstick_ms / ms_per_iter; launches and hostChecks of the longer solve; equal_bits: after a
               maxIter = `check_iters` solve, the first and the last column of X, their status, iterations and rr equal
               the single solve on a contiguous copy of that column, bit for bit (device against device)
  traffic      the unpreconditioned CG iteration less its SpMM pass against 88 B per row and column of vector traffic
Kernel split: `rocprofv3 --kernel-trace --stats -- python scripts/block_krylov_timing.py --quick` in a run of its own.

    python scripts/block_krylov_timing.py [--quick] [--out profiles/block_krylov_timing.log]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from spmv_openmp_cuda_amd import api  # noqa: E402
from spmm_timing import Events  # noqa: E402
from test_krylov_abi import convdiff7  # noqa: E402
from test_trsv_abi import laplacian7  # noqa: E402

ROW = api.SPMV_DENSE_ROW_MAJOR
SINGLE = {"cg": "hipSpCGCSR", "bicgstab": "hipSpBiCGStabCSR"}
BLOCK = {"cg": "hipSpCGBlockCSR", "bicgstab": "hipSpBiCGStabBlockCSR"}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def handle(m):
    return C.byref(m.handle) if m is not None else None


def single_solve(kind, A, P, b, x, maxit):
    opts, info = api.spmvKrylovOpts(0.0, maxit, None), api.spmvKrylovInfo()
    x.zero_()
    api._check(getattr(api.lib, SINGLE[kind])(handle(A), handle(P), b.data_ptr(), x.data_ptr(), C.byref(opts), C.byref(info)), SINGLE[kind])
    return info


def block_solve(kind, A, P, B, X, maxit, cols=None):
    k = B.shape[1]
    opts, info = api.spmvKrylovOpts(0.0, maxit, None), api.spmvKrylovInfo()
    X.zero_()
    api._check(getattr(api.lib, BLOCK[kind])(handle(A), handle(P), k, B.data_ptr(), k, ROW, X.data_ptr(), k, ROW, C.byref(opts), cols,
                                             C.byref(info)), BLOCK[kind])
    return info


def quotient(ev, run, n1, n2):
    """(ms per iteration, info of the longer solve): the difference quotient of two solve lengths, median of 3 each"""
    t = {}
    for n in (n1, n2):
        reps = []
        for _ in range(3):
            box = {}
            reps.append((ev.time(lambda: box.update(info=run(n))), box["info"]))
        t[n] = (float(np.median([r[0] for r in reps])), reps[-1][1])
    return (t[n2][0] - t[n1][0]) / (n2 - n1), t[n2][1]


def bits_equal(a, b):
    return bool(np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64)))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="k = 16 only, fewer iterations, no bit checks (for the profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_krylov_timing.log"))
    a = ap.parse_args()
    api.spmvHipInit(0)
    ev = Events()
    n1, n2 = (5, 15) if a.quick else (50, 250)
    widths = (16,) if a.quick else (1, 2, 4, 8, 16, 32)
    check_iters = 5
    out = open(a.out, "w")
    out.write("# scripts/block_krylov_timing.py on the MI355X; one JSON record per line (fields: the script's docstring)\n")
    nx, ny, nz = 500, 100, 100
    M = nx * ny * nz
    gen = torch.Generator(device="cuda").manual_seed(27)
    Bfull = torch.rand((M, max(widths)), dtype=torch.float64, device="cuda", generator=gen)
    for mname, make, kind in (("laplace7-500x100x100", laplacian7, "cg"), ("convdiff7-500x100x100", convdiff7, "bicgstab")):
        IRP, JA, AS = make(nx, ny, nz)
        A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
        P = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
        P.ilu0()
        del IRP, JA, AS
        b1, x1 = Bfull[:, 0].contiguous(), torch.zeros(M, dtype=torch.float64, device="cuda")
        single_solve(kind, A, None, b1, x1, 2)                           # the selection of the serial-order kernel
        # ---- the parts at k = 16
        B16 = Bfull[:, :16].contiguous()
        Y16 = torch.empty_like(B16)
        api.lib.spmvHipSetSync(0)
        spmm = ev.median(lambda: api.lib.hipSpMMRowsCSR(handle(A), 16, B16.data_ptr(), 16, ROW, Y16.data_ptr(), 16, ROW))
        lower = ev.median(lambda: api.lib.hipSpTRSMCSR(handle(P), api.SPMV_TRI_LOWER, api.SPMV_DIAG_UNIT, 16, B16.data_ptr(), 16, ROW,
                                                       Y16.data_ptr(), 16, ROW))
        upper = ev.median(lambda: api.lib.hipSpTRSMCSR(handle(P), api.SPMV_TRI_UPPER, api.SPMV_DIAG_STORED, 16, Y16.data_ptr(), 16, ROW,
                                                       Y16.data_ptr(), 16, ROW))
        h = torch.empty(16, dtype=torch.float64, device="cuda")
        bdot = ev.median(lambda: api.lib.spmvHipBlockDot(M, 16, B16.data_ptr(), 16, ROW, Y16.data_ptr(), 16, ROW, h.data_ptr()))
        api.lib.spmvHipSetSync(1)
        emit(out, {"record": "parts", "matrix": mname, "k": 16, "spmm_ms": round(spmm, 4), "trsm_lower_ms": round(lower, 4),
                   "trsm_upper_ms": round(upper, 4), "block_dot_ms": round(bdot, 4),
                   "block_dot_TBps": round(2 * 16 * 8 * M / (bdot * 1e9), 3)})
        del B16, Y16
        for pre in (None, P):
            per1, info1 = quotient(ev, lambda n: single_solve(kind, A, pre, b1, x1, n), n1, n2)
            emit(out, {"record": "single", "matrix": mname, "solver": kind, "ilu0": pre is not None, "ms_per_iter": round(per1, 4),
                       "launches": int(info1.launches), "iters": n2})
            for k in widths:
                B = Bfull[:, :k].contiguous()
                X = torch.zeros_like(B)
                per, info = quotient(ev, lambda n: block_solve(kind, A, pre, B, X, n), n1, n2)
                rec = {"record": "block", "matrix": mname, "solver": kind, "ilu0": pre is not None, "k": k, "K": 16,
                       "ms_per_iter": round(per, 4), "yardstick_ms": round(k * per1, 4), "speedup": round(k * per1 / per, 3),
                       "launches": int(info.launches), "hostChecks": int(info.hostChecks), "iters": n2}
                if not a.quick:
                    cols = (api.spmvKrylovColumn * k)()
                    block_solve(kind, A, pre, B, X, check_iters, cols)
                    ok = True
                    for c in sorted({0, k - 1}):
                        bc = B[:, c].contiguous()
                        s = single_solve(kind, A, pre, bc, x1, check_iters)
                        ok = ok and bits_equal(X[:, c].contiguous(), x1) and (cols[c].status, cols[c].iterations) == (s.status, s.iterations) \
                            and np.float64(cols[c].rr).tobytes() == np.float64(s.rr).tobytes()
                    rec["check_iters"], rec["equal_bits"] = check_iters, bool(ok)
                emit(out, rec)
                if kind == "cg" and pre is None and k == 16:
                    vec_ms = per - spmm
                    emit(out, {"record": "traffic", "matrix": mname, "k": k, "vector_passes_ms": round(vec_ms, 4),
                               "bytes_per_row_and_column": 88, "TBps": round(88.0 * k * M / (vec_ms * 1e9), 3)})
                del B, X
        A.free()
        P.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
