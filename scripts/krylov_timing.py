"""Krylov solves (hipSpCGCSR, hipSpBiCGStabCSR): time per iteration on the 500 x 100 x 100 7-point
Laplacian (CG, ILU(0)-PCG), the upwind convection-diffusion stencil of the same size and c2 (BiCGStab), with a bitwise
check against tests/krylov_ref.py for every timed configuration.

Records (one JSON line each):
  parts        serial-order SpMV (spmvHipEnqueueAutoRows), hipSpTRSVCSR lower / upper on the ILU(0) handle and spmvHipDot,
               device events, median of 10
  solve        ms per iteration = (solve(maxIter = n2) - solve(maxIter = n1)) / (n2 - n1) at tol = 0 (every solve runs to
               MAXITER), device events around the synchronous call; launches and hostChecks of the longer solve;
               equal_bits: x of a maxIter = `check` solve == the numpy loop, bit for bit (same K, same handles)
  torch_loop   the same CG iteration driven from Python: the library's SpMV on device tensors, torch.dot, torch vector ops
               and one host sync (.item()) per iteration; ms per iteration over n2 - n1 iterations
  k_sweep      a converging solve (tol 1e-8) per check interval K: host wall time, iterations, hostChecks; x equal across K
Kernel split: `rocprofv3 --kernel-trace --stats -- python scripts/krylov_timing.py --quick` in a run of its own.

    python scripts/krylov_timing.py [--quick] [--out profiles/krylov_timing.log]
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

from spmv_openmp_cuda_amd import api, synth  # noqa: E402
from spmm_timing import Events  # noqa: E402
from ilu0_ref import ilu0_levels  # noqa: E402
from krylov_ref import Csr, bicgstab_ref, cg_ref  # noqa: E402
from test_krylov_abi import convdiff7  # noqa: E402
from test_trsv_abi import laplacian7  # noqa: E402

HBM_TBPS = 8.0        # MI355X peak HBM rate (MI355X_MICROARCH), for the floor of the vector traffic


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def bits_equal(a, b):
    return bool(np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)))


def solve_ms(ev, fn, A, P, db, dx, tol, maxit, K, name):
    api.lib.spmvHipSetVariant(name.encode(), K)
    opts, info = api.spmvKrylovOpts(tol, maxit, None), api.spmvKrylovInfo()
    api.lib.spmvHipVecFill(dx, int(A.handle.M), 0)                    # x0 = 0

    def run():
        api._check(fn(C.byref(A.handle), C.byref(P.handle) if P is not None else None, db, dx, C.byref(opts), C.byref(info)), name)
    ms = ev.time(run)
    return ms, info


def per_iteration(ev, fn, name, A, P, M, b, n1, n2, K):
    db, dx = api.DeviceVector(M).up(b), api.DeviceVector(M)
    try:
        t = {}
        for n in (n1, n2):
            reps = [solve_ms(ev, fn, A, P, db.ptr, dx.ptr, 0.0, n, K, name) for _ in range(3)]
            t[n] = (float(np.median([r[0] for r in reps])), reps[-1][1])
        return (t[n2][0] - t[n1][0]) / (n2 - n1), t[n2][1]
    finally:
        db.free()
        dx.free()


def check_bits(kind, A, P, IRP, JA, AS, F, M, b, iters):
    x, info = getattr(A, kind)(b, precond=P, tol=0.0, maxiter=iters)
    ref = (cg_ref if kind == "cg" else bicgstab_ref)(Csr(M, IRP, JA, AS, F), b, np.zeros(M), 0.0, iters)
    return bits_equal(x, ref[0]) and (info.status, info.iterations) == (ref[1], ref[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations and no bit checks (for the profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "krylov_timing.log"))
    a = ap.parse_args()
    api.spmvHipInit(0)
    ev = Events()
    n1, n2 = (10, 40) if a.quick else (50, 250)
    out = open(a.out, "w")
    out.write("# scripts/krylov_timing.py on the MI355X; one JSON record per line (fields: the script's docstring)\n")
    nx, ny, nz = 500, 100, 100
    M = nx * ny * nz
    b = np.random.default_rng(19).random(M)
    cg, bi = api.lib.hipSpCGCSR, api.lib.hipSpBiCGStabCSR
    for mname, gen in (("laplace7-500x100x100", laplacian7), ("convdiff7-500x100x100", convdiff7)):
        IRP, JA, AS = gen(nx, ny, nz)
        A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
        P = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
        P.ilu0()
        F = None if a.quick else ilu0_levels(M, IRP, JA, AS)
        dx, dy = api.DeviceVector(M).up(b), api.DeviceVector(M)
        api._check(api.lib.spmvHipEnqueueAutoRows(C.byref(A.handle), dx.ptr, dy.ptr, None), "spmv")   # the selection
        spmv = ev.median(lambda: api.lib.spmvHipEnqueueAutoRows(C.byref(A.handle), dx.ptr, dy.ptr, None))
        api.lib.spmvHipSetSync(0)
        lower = ev.median(lambda: api.lib.hipSpTRSVCSR(C.byref(P.handle), api.SPMV_TRI_LOWER, api.SPMV_DIAG_UNIT, dx.ptr, dy.ptr))
        upper = ev.median(lambda: api.lib.hipSpTRSVCSR(C.byref(P.handle), api.SPMV_TRI_UPPER, api.SPMV_DIAG_STORED, dy.ptr, dy.ptr))
        res = api.DeviceBuffer(8)
        dot = ev.median(lambda: api.lib.spmvHipDot(M, dx.ptr, dy.ptr, res.ptr))
        api.lib.spmvHipSetSync(1)
        emit(out, {"record": "parts", "matrix": mname, "rows": M, "nnz": int(JA.size), "spmv_ms": round(spmv, 4),
                   "trsv_lower_ms": round(lower, 4), "trsv_upper_ms": round(upper, 4), "dot_ms": round(dot, 4),
                   "spmv_choice": (api.lib.spmvHipAutoChoiceRows(C.byref(A.handle), None) or b"-").decode()})
        kinds = (("cg", cg, "hipSpCGCSR"),) if mname.startswith("laplace") else (("bicgstab", bi, "hipSpBiCGStabCSR"),)
        for kind, fn, name in kinds:
            for pre in (None, P):
                per, info = per_iteration(ev, fn, name, A, pre, M, b, n1, n2, 16)
                rec = {"record": "solve", "matrix": mname, "solver": kind, "ilu0": pre is not None, "K": 16,
                       "ms_per_iter": round(per, 4), "launches": int(info.launches), "hostChecks": int(info.hostChecks),
                       "iters": n2}
                if pre is None and kind == "cg":
                    floor = spmv + 88.0 * M / (HBM_TBPS * 1e9)
                    rec["floor_ms"] = round(floor, 4)
                if pre is not None:
                    rec["parts_ms"] = round((lower + upper + spmv) * (2 if kind == "bicgstab" else 1), 4)   # M^-1 and A per half step
                if not a.quick:
                    rec["check_iters"] = 5 if pre is not None else 10
                    rec["equal_bits"] = check_bits(kind, A, pre, IRP, JA, AS, F if pre is not None else None, M, b,
                                                   rec["check_iters"])
                emit(out, rec)
        if mname.startswith("laplace") and not a.quick:
            import torch
            bt = torch.from_numpy(b).cuda()

            def torch_cg(iters):
                x = torch.zeros_like(bt)
                r = bt.clone()
                p = r.clone()
                q = torch.empty_like(bt)
                rz = torch.dot(r, r)
                for _ in range(iters):
                    api.lib.spmvHipEnqueueAutoRows(C.byref(A.handle), p.data_ptr(), q.data_ptr(), None)
                    alpha = rz / torch.dot(p, q)
                    x += alpha * p
                    r -= alpha * q
                    rzn = torch.dot(r, r)
                    if rzn.item() <= 0.0:                               # the one host sync per iteration
                        break
                    p = r + (rzn / rz) * p
                    rz = rzn
                return x
            torch_cg(5)
            torch.cuda.synchronize()
            t = {}
            for n in (n1, n2):
                t0 = time.perf_counter()
                torch_cg(n)
                torch.cuda.synchronize()
                t[n] = (time.perf_counter() - t0) * 1e3
            emit(out, {"record": "torch_loop", "matrix": mname, "ms_per_iter": round((t[n2] - t[n1]) / (n2 - n1), 4)})
        dx.free()
        dy.free()
        res.free()
        A.free()
        P.free()
    # c2: BiCGStab without a preconditioner (its rows hold no diagonal entry in general), report only
    w = synth.WORKLOADS["c2"]
    irp = synth.prefix(synth.row_lengths(w))
    dm = synth.device_csr(w, irp, 0, w.N)
    bc = np.random.default_rng(23).random(w.N)
    per, info = per_iteration(ev, bi, "hipSpBiCGStabCSR", dm, None, w.N, bc, n1 // 5, n2 // 5, 16)
    emit(out, {"record": "solve", "matrix": w.name, "solver": "bicgstab", "ilu0": False, "K": 16, "ms_per_iter": round(per, 4),
               "launches": int(info.launches), "hostChecks": int(info.hostChecks), "iters": n2 // 5, "status": int(info.status),
               "iterations": int(info.iterations)})
    dm.free()
    if not a.quick:                                                     # the check interval on converging solves
        n = 100
        IRP, JA, AS = laplacian7(n, n, n)
        Mk = n ** 3
        A = api.spMatCpyCSR(api.HostCSR(Mk, Mk, IRP, JA, AS))
        P = api.spMatCpyCSR(api.HostCSR(Mk, Mk, IRP, JA, AS))
        P.ilu0()
        bk = np.random.default_rng(29).random(Mk)
        for pre in (None, P):
            xs = None
            for K in (1, 4, 16, 64):
                api.lib.spmvHipSetVariant(b"hipSpCGCSR", K)
                A.cg(bk, precond=pre, tol=1e-8, maxiter=5000)
                t0 = time.perf_counter()
                x, info = A.cg(bk, precond=pre, tol=1e-8, maxiter=5000)
                ms = (time.perf_counter() - t0) * 1e3
                same = xs is None or bits_equal(x, xs)
                xs = x if xs is None else xs
                emit(out, {"record": "k_sweep", "matrix": "laplace7-100^3", "ilu0": pre is not None, "K": K, "solve_ms": round(ms, 3),
                           "iterations": int(info.iterations), "hostChecks": int(info.hostChecks),
                           "ms_per_iter": round(ms / max(info.iterations, 1), 4), "x_equal_across_K": same})
        api.lib.spmvHipSetVariant(b"hipSpCGCSR", 16)
        A.free()
        P.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
