"""Restarted GMRES (hipSpGMRESCSR): time per inner iteration on the 500 x 100 x 100 upwind
convection-diffusion stencil at restart = 30, without and with ILU(0), the plain and the fused first update, against a
torch-driven loop of the same algorithm and the byte floor, all in one run; and the rates of spmvHipMultiDot.

Records (one JSON line each):
  solve        ms per inner iteration = (solve(maxIter = n2) - solve(maxIter = n1)) / (n2 - n1) at tol = 0, device events
               around the synchronous call, median of 3; launches and hostChecks of the longer solve; equal_bits: x, status
               and iterations of a maxIter = 10 solve == tests/gmres_ref.py
  torch_loop   the same CGS2 iteration driven from Python: the library's SpMV (and triangular solves) on device tensors,
               V.T @ w, torch.linalg.norm, the Givens rotations on the host (one sync per step); ms per inner iteration
  floor        one serial-order SpMV (measured) plus the vector traffic of the passes at 8 TB/s: per row and step
               32 (j + 1) B for the two projections and the two updates averaged over a cycle, 48 B for w and v[j+1]
  multidot     spmvHipMultiDot at n = 5 M, k = 1, 8, 30, 64: ms, GB/s against (k + 1) 8 n bytes, and k calls of spmvHipDot
Kernel split: `rocprofv3 --kernel-trace --stats -- python scripts/gmres_timing.py --quick` in a run of its own.

    python scripts/gmres_timing.py [--quick] [--out profiles/gmres_timing.log]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from spmv_openmp_cuda_amd import api  # noqa: E402
from spmm_timing import Events  # noqa: E402
from gmres_ref import gmres_ref  # noqa: E402
from ilu0_ref import ilu0_levels  # noqa: E402
from krylov_ref import Csr  # noqa: E402
from krylov_timing import bits_equal, emit  # noqa: E402
from test_krylov_abi import convdiff7  # noqa: E402

HBM_TBPS = 8.0


def solve_ms(ev, A, P, db, dx, maxit, restart, fused):
    api.lib.spmvHipSetVariant(b"hipSpGMRESCSR", fused)
    opts, info = api.spmvGmresOpts(0.0, maxit, restart, None), api.spmvKrylovInfo()
    api.lib.spmvHipVecFill(dx, int(A.handle.M), 0)

    def run():
        api._check(api.lib.hipSpGMRESCSR(C.byref(A.handle), C.byref(P.handle) if P is not None else None, db, dx, C.byref(opts),
                                         C.byref(info)), "hipSpGMRESCSR")
    return ev.time(run), info


def per_iteration(ev, A, P, M, b, n1, n2, restart, fused):
    db, dx = api.DeviceVector(M).up(b), api.DeviceVector(M)
    try:
        t = {}
        for n in (n1, n2):
            reps = [solve_ms(ev, A, P, db.ptr, dx.ptr, n, restart, fused) for _ in range(3)]
            t[n] = (float(np.median([r[0] for r in reps])), reps[-1][1])
        return (t[n2][0] - t[n1][0]) / (n2 - n1), t[n2][1]
    finally:
        db.free()
        dx.free()


def torch_loop(torch, A, P, b, iters, restart):
    """CGS2 GMRES(restart) for `iters` inner steps at tol = 0: ms per step (device events over the whole loop)"""
    n = b.numel()
    x = torch.zeros_like(b)
    V = torch.empty((restart + 1, n), dtype=torch.float64, device=b.device)
    w, z, t = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)

    def spmv(src, dst):
        api._check(api.lib.spmvHipEnqueueAutoRows(C.byref(A.handle), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), None), "spmv")

    def minv(src, dst):
        if P is None:
            return src
        P.solve_triangular(src, lower=True, unit_diagonal=True, out=t)
        P.solve_triangular(t, lower=False, out=dst)
        return dst
    api.lib.spmvHipSetSync(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    k = 0
    while k < iters:
        spmv(x, w)
        r = b - w
        beta = torch.linalg.norm(r).item()
        V[0] = r / beta
        g = [beta] + [0.0] * restart
        cs, sn, R = [0.0] * restart, [0.0] * restart, np.zeros((restart, restart))
        cols = 0
        for j in range(restart):
            spmv(minv(V[j], z), w)
            Vj = V[:j + 1]
            h = Vj @ w
            w -= Vj.T @ h
            c = Vj @ w
            w -= Vj.T @ c
            hn = torch.linalg.norm(w)
            hh = torch.cat([h + c, hn.reshape(1)]).cpu().numpy()     # the step's one sync
            hv, hnv = hh[:-1].copy(), float(hh[-1])
            for i in range(j):
                ti = cs[i] * hv[i] + sn[i] * hv[i + 1]
                hv[i + 1] = cs[i] * hv[i + 1] - sn[i] * hv[i]
                hv[i] = ti
            d = math.hypot(hv[j], hnv)
            cs[j], sn[j] = hv[j] / d, hnv / d
            hv[j] = d
            R[:j + 1, j] = hv
            g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
            k += 1
            cols = j + 1
            if k == iters or j == restart - 1:
                break
            V[j + 1] = w / hnv
        y = np.linalg.solve(np.triu(R[:cols, :cols]), np.array(g[:cols]))
        u = V[:cols].T @ torch.from_numpy(y).to(b.device)
        x += minv(u, z)
    e1.record()
    torch.cuda.synchronize()
    api.lib.spmvHipSetSync(1)
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations, no bit checks, no torch loop (for the profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmres_timing.log"))
    a = ap.parse_args()
    import torch
    api.spmvHipInit(0)
    ev = Events()
    n1, n2 = (10, 40) if a.quick else (50, 250)
    restart = 30
    out = open(a.out, "w")
    out.write("# scripts/gmres_timing.py on the MI355X; one JSON record per line (fields: the script's docstring)\n")
    nx, ny, nz = 500, 100, 100
    M = nx * ny * nz
    b = np.random.default_rng(20).random(M)
    IRP, JA, AS = convdiff7(nx, ny, nz)
    A = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))
    P.ilu0()
    F = None if a.quick else ilu0_levels(M, IRP, JA, AS)
    dxx, dyy = api.DeviceVector(M).up(b), api.DeviceVector(M)
    spmv_ms = ev.median(lambda: api.lib.spmvHipEnqueueAutoRows(C.byref(A.handle), dxx.ptr, dyy.ptr, None))
    # per row and step: projections and updates read v[0..j] four times (32 (j+1) B, j averaged over a cycle: (restart+1)/2
    # columns), w is read or written 5 times and v[j+1] written once (48 B)
    vec_bytes = M * (32.0 * (restart + 1) / 2 + 48.0)
    floor_ms = spmv_ms + vec_bytes / (HBM_TBPS * 1e12) * 1e3
    emit(out, {"record": "floor", "matrix": "convdiff7-500x100x100", "restart": restart, "spmv_ms": spmv_ms,
               "vector_bytes_per_step": vec_bytes, "floor_ms_per_iter": floor_ms})
    bt = torch.from_numpy(b).cuda()
    for pname, Pm, Fm in (("none", None, None), ("ilu0", P, F)):
        tl = None if a.quick else torch_loop(torch, A, Pm, bt, 60, restart)
        for fused in (0, 1):
            per, info = per_iteration(ev, A, Pm, M, b, n1, n2, restart, fused)
            rec = {"record": "solve", "precond": pname, "restart": restart, "fused": fused, "ms_per_iter": per,
                   "launches": int(info.launches), "hostChecks": int(info.hostChecks), "iterations": int(info.iterations),
                   "ratio_to_floor": per / floor_ms if Pm is None else None}
            if not a.quick:
                api.lib.spmvHipSetVariant(b"hipSpGMRESCSR", fused)
                x, inf = A.gmres(b, precond=Pm, tol=0.0, maxiter=10, restart=restart)
                ref = gmres_ref(Csr(M, IRP, JA, AS, Fm), b, np.zeros(M), 0.0, 10, restart)
                rec["equal_bits"] = bits_equal(x, ref[0]) and (inf.status, inf.iterations) == (ref[1], ref[2])
                rec["torch_loop_ms_per_iter"] = tl
                rec["torch_over_library"] = tl / per
            emit(out, rec)
    api.lib.spmvHipSetVariant(b"hipSpGMRESCSR", 0)
    n = 5_000_000
    kmax = 64
    Vt = torch.rand((kmax, n), dtype=torch.float64, device="cuda")
    wt = torch.rand(n, dtype=torch.float64, device="cuda")
    ht = torch.empty(kmax, dtype=torch.float64, device="cuda")
    for k in (1, 8, 30, 64):
        md = ev.median(lambda: api.lib.spmvHipMultiDot(n, k, Vt.data_ptr(), n, wt.data_ptr(), ht.data_ptr()))

        def kdots():
            for i in range(k):
                api.lib.spmvHipDot(n, Vt.data_ptr() + 8 * n * i, wt.data_ptr(), ht.data_ptr() + 8 * i)
        api.lib.spmvHipSetSync(0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            e0.record()
            kdots()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        api.lib.spmvHipSetSync(1)
        kd = float(np.median(ts))
        emit(out, {"record": "multidot", "n": n, "k": k, "ms": md, "GBps": (k + 1) * 8.0 * n / (md * 1e-3) / 1e9,
                   "k_dots_ms": kd, "k_dots_over_multidot": kd / md})
    out.close()
    A.free()
    P.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
