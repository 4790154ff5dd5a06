"""Multi-colour ordering (spmvHipColourCSR, spmvHipCsrPermute) on the 500 x 100 x 100 7-point Laplacian
and the upwind convection-diffusion stencil of the same size: what the colouring and the permutation cost, and what the
triangular solves, ILU(0) and the preconditioned Krylov loops gain, natural ordering and each colouring in the same run.

Records (one JSON line each):
  colour       per order: colours, rounds, hostChecks, symmetric, wall ms of the call (second of two calls)
  permute      build of B = P A P^T, wall ms (second of two), next to spmvHipCsrTranspose of the same matrix as the yardstick
  parts        per ordering: serial-order SpMV, hipSpTRSVCSR lower / upper on the ILU(0) handle (device events, median of
               10), levels of both triangles, hipSpILU0CSR ms (info.ms), ms per PCG iteration as lower + upper + SpMV
  solve        tol 1e-8: iterations, status and wall ms of the synchronous call (second of two), plain and ILU(0), natural
               and each colouring (b permuted, so every configuration solves the same system); equal_bits: x of a short solve
               == the numpy loop on the handle's downloaded arrays

    python scripts/colour_timing.py [--quick] [--out profiles/colour_timing.log]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from spmv_openmp_cuda_amd import api  # noqa: E402
from spmm_timing import Events  # noqa: E402
from krylov_ref import Csr, bicgstab_ref, cg_ref  # noqa: E402
from test_krylov_abi import convdiff7  # noqa: E402
from test_trsv_abi import laplacian7  # noqa: E402


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def wall(fn):
    """the second of two calls, host wall ms, and its result"""
    fn_result = fn()
    if hasattr(fn_result, "free"):
        fn_result.free()
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def down(ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    api._check(api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes), "download")
    return out


def arrays(dm):
    h = dm.handle
    return down(h.IRP, h.M + 1, np.uint32), down(h.JA, h.NZ, np.uint32), down(h.AS, h.NZ, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 100 x 50 x 50 grid and no bit checks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_timing.log"))
    a = ap.parse_args()
    api.spmvHipInit(0)
    ev = Events()
    out = open(a.out, "w")
    out.write("# scripts/colour_timing.py on the MI355X; one JSON record per line (fields: the script's docstring)\n")
    nx, ny, nz = (100, 50, 50) if a.quick else (500, 100, 100)
    M = nx * ny * nz
    b = np.random.default_rng(21).random(M)
    for mname, gen, kind in ((f"laplace7-{nx}x{ny}x{nz}", laplacian7, "cg"), (f"convdiff7-{nx}x{ny}x{nz}", convdiff7, "bicgstab")):
        IRP, JA, AS = gen(nx, ny, nz)
        A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
        ms_t, T = wall(A.transpose)
        T.free()
        orderings = [("natural order", None)]
        for order, seed in (("natural", 0), ("hash", 0)):
            ms, col = wall(lambda: A.colour(order=order, seed=seed))
            i = col.info
            emit(out, {"record": "colour", "matrix": mname, "order": order, "colours": int(i.colours), "rounds": int(i.rounds),
                       "hostChecks": int(i.hostChecks), "maxColourRows": int(i.maxColourRows), "symmetric": int(i.symmetric),
                       "ms": round(ms, 3)})
            orderings.append((f"colour:{order}", col))
        for oname, col in orderings:
            if col is None:
                B = A
                P = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
                bp = b
            else:
                ms_p, B = wall(lambda: A.permute(col))
                P = A.permute(col)
                bp = api.permute_vector(col, b)
                emit(out, {"record": "permute", "matrix": mname, "ordering": oname, "permute_ms": round(ms_p, 3),
                           "transpose_ms": round(ms_t, 3)})
            ilu = P.ilu0()
            lv = [int(P.triangular_info(lo).levels) for lo in (True, False)]
            dx, dy = api.DeviceVector(M).up(bp), api.DeviceVector(M)
            api._check(api.lib.spmvHipEnqueueAutoRows(C.byref(B.handle), dx.ptr, dy.ptr, None), "spmv")   # the selection
            spmv = ev.median(lambda: api.lib.spmvHipEnqueueAutoRows(C.byref(B.handle), dx.ptr, dy.ptr, None))
            P.triangular_analyse(False)
            api.lib.spmvHipSetSync(0)
            lower = ev.median(lambda: api.lib.hipSpTRSVCSR(C.byref(P.handle), api.SPMV_TRI_LOWER, api.SPMV_DIAG_UNIT, dx.ptr, dy.ptr))
            upper = ev.median(lambda: api.lib.hipSpTRSVCSR(C.byref(P.handle), api.SPMV_TRI_UPPER, api.SPMV_DIAG_STORED, dy.ptr, dy.ptr))
            api.lib.spmvHipSetSync(1)
            lv = [int(P.triangular_info(lo).levels) for lo in (True, False)]
            emit(out, {"record": "parts", "matrix": mname, "ordering": oname, "spmv_ms": round(spmv, 4), "trsv_lower_ms": round(lower, 4),
                       "trsv_upper_ms": round(upper, 4), "levels": lv, "ilu0_ms": round(ilu.ms, 3), "ilu0_launches": int(ilu.launches),
                       "pcg_iter_ms": round(lower + upper + spmv, 4)})
            dx.free()
            dy.free()
            ref = None
            if not a.quick:
                irp, ja, av = arrays(B)
                ref = (irp, ja, av, arrays(P)[2])
            for pre in (None, P):
                if pre is None and col is not None and oname != "colour:natural":
                    continue                                             # plain solves: natural order and one permuted order
                ms, (x, info) = wall(lambda: getattr(B, kind)(bp, precond=pre, tol=1e-8, maxiter=5000))
                rec = {"record": "solve", "matrix": mname, "ordering": oname, "solver": kind, "ilu0": pre is not None,
                       "iterations": int(info.iterations), "status": int(info.status), "solve_ms": round(ms, 3),
                       "ms_per_iter": round(ms / max(int(info.iterations), 1), 4)}
                if ref is not None:
                    n = 3
                    xs, si_ = getattr(B, kind)(bp, precond=pre, tol=0.0, maxiter=n)
                    csr = Csr(M, ref[0], ref[1], ref[2], ref[3] if pre is not None else None)
                    r = (cg_ref if kind == "cg" else bicgstab_ref)(csr, bp, np.zeros(M), 0.0, n)
                    rec["check_iters"] = n
                    rec["equal_bits"] = bool(np.array_equal(xs.view(np.uint64), r[0].view(np.uint64))) and \
                        (si_.status, si_.iterations) == (r[1], r[2])
                emit(out, rec)
            P.free()
            if col is not None:
                B.free()
                col.free()
        A.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
