"""The residual block (spmvHipBlockResidual) and generalised Davidson (hipSpDavidsonCSR), DESIGN.md section 42: the residual
kernel at n = 5 M against the library's own streaming figure for a fused vector pass -- the CGS2 update kernel, section 39's
yardstick, timed in the same run -- and the 500 x 100 x 100 seven-point Laplacian, SMALLEST, nev = 4, ncv = 20, tol = 1e-8,
without a dM, with FSAI and with the smoothed Chebyshev hierarchy, each next to hipSpLanczosCSR on the same v0.

The parent starts its children one after the other, one process per configuration, each with a time limit; after a child that
fails nothing more is started on the device.  Records (one JSON line each):
  residual     child `kernel`: spmvHipBlockResidual at (m, k) = (20, 4) and (64, 16): ms (device events around the pass and
               its finish, median of 10 after a warm-up), bytes = 8 n (2 m + k), GB/s
  update       child `stream` (scripts/lanczos_timing.py's) under rocprofv3 --kernel-trace: the first update kernel of Lanczos
               step j streams 8 n (j + 3) bytes; ms and GB/s of the dispatches nearest the two residual byte counts
  eig          child `e2e:<config>`: hipSpLanczosCSR (600 products at most) and hipSpDavidsonCSR (600 at most), the second
               of two calls each: status, products, restarts or cycles, applications, launches, ms, jacobiMs, res / scale
  split        child `e2e:<config>` once more under rocprofv3 --kernel-trace: the Davidson solve's kernel time by group
               (residual kernel and its finish, CGS2 = projections, updates, scalar steps, divisions and the new column of H,
               restart rotations, and SpMV together with the preconditioner: their kernels share names) from the trace
  verdict      residual GB/s over update GB/s at the nearest byte count

    python scripts/davidson_timing.py [--out profiles/davidson_timing.log]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import lanczos_timing as lt  # noqa: E402

N = lt.N
SHAPES = ((20, 4), (64, 16))
CONFIGS = ("none", "fsai", "amg-chebyshev")
CAP = 600


def say(rec):
    print(json.dumps(rec), flush=True)


def child_kernel(api):
    from spmm_timing import Events
    ev = Events()
    rng = np.random.default_rng(40)
    dV, dW, dR = api.DeviceVector(64 * N), api.DeviceVector(64 * N), api.DeviceVector(16 * N)
    dS, dT, dN = api.DeviceVector(64 * 16), api.DeviceVector(16), api.DeviceVector(16)
    for buf in (dV, dW):
        for c in range(64):                                          # (column by column: no 2.5 GB host array)
            col = rng.random(N)
            api._check(api.lib.spmvHipVecUp(C.c_void_p(buf.ptr.value + 8 * N * c), col.ctypes.data, N), "up")
    dS.up(rng.standard_normal(64 * 16))
    dT.up(rng.standard_normal(16))
    for m, k in SHAPES:
        ms = ev.median(lambda: api.lib.spmvHipBlockResidual(N, m, k, dV.ptr, N, dW.ptr, N, dS.ptr, 64, dT.ptr, dR.ptr, N, dN.ptr))
        nbytes = 8.0 * N * (2 * m + k)
        say({"record": "residual", "n": N, "m": m, "k": k, "ms": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6})
    for b in (dV, dW, dR, dS, dT, dN):
        b.free()


def davidson(api, A, dM, dv, dx, M, maxiter):
    opts, info = api.spmvDavidsonOpts(4, 20, 1, 1e-8, maxiter, 0), api.spmvDavidsonInfo()
    theta, res = np.zeros(4), np.zeros(4)
    api._check(api.lib.hipSpDavidsonCSR(C.byref(A.handle), C.byref(dM.handle) if dM is not None else None, dv.ptr, C.byref(opts), dx.ptr, M,
                                        theta.ctypes.data, res.ctypes.data, C.byref(info)), "hipSpDavidsonCSR")
    return info, theta, res


def child_e2e(api, config):
    A, M = lt.laplacian(api)
    dM = None
    if config == "fsai":
        dM = A.fsai()
    elif config == "amg-chebyshev":
        dM = A.amg(smoothed=True)
        dM.set_smoother("chebyshev", nu1=2, nu2=2)
    dv, dx = api.DeviceVector(M).up(np.random.default_rng(0).standard_normal(M)), api.DeviceVector(4 * M)
    if config == "none":                                             # (Lanczos takes no dM: measured once, next to the plain loop)
        lt.lanczos(api, A, dv, dx, M, 4, 20, 1, CAP)
        info, theta, res = lt.lanczos(api, A, dv, dx, M, 4, 20, 1, CAP)
        say({"record": "eig", "solver": "lanczos", "config": config, "status": info.status, "found": info.found, "products": info.iterations,
             "cycles": info.cycles, "launches": info.launches, "ms": info.ms, "jacobiMs": info.jacobiMs, "theta": theta.tolist(),
             "res_over_scale": (res / info.scale).tolist()})
    davidson(api, A, dM, dv, dx, M, 1)                               # (the handles' first products choose their kernels)
    info, theta, res = davidson(api, A, dM, dv, dx, M, CAP)
    say({"record": "eig", "solver": "davidson", "config": config, "status": info.status, "found": info.found, "products": info.iterations,
         "restarts": info.restarts, "applications": info.precondApplies, "launches": info.launches, "hostChecks": info.hostChecks,
         "ms": info.ms, "jacobiMs": info.jacobiMs, "theta": theta.tolist(), "res_over_scale": (res / info.scale).tolist()})
    if dM is not None:
        dM.free()
    A.free()


def group(name):
    if "block_residual_kernel" in name:
        return "residual"
    if "block_combine_kernel" in name:
        return "restart_rotation"
    if any(s in name for s in ("multidot_", "gmres_update_kernel", "davidson_finish_kernel", "krylov_vec_kernel")):
        return "cgs2_and_dots"
    return "spmv_and_preconditioner"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "davidson_timing.log"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        from spmv_openmp_cuda_amd import api
        api.spmvHipInit(0)
        if a.child == "kernel":
            child_kernel(api)
        elif a.child == "stream":
            lt.child_stream(api)
        else:
            child_e2e(api, a.child.split(":", 1)[1])
        api.spmvHipFinalize()
        return 0
    out = open(a.out, "w")
    out.write("# scripts/davidson_timing.py on the MI355X; one JSON record per line (fields: the script's docstring)\n")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    me = os.path.abspath(__file__)
    lt.__file__ = me                                                 # (lanczos_timing.traced starts `__file__ --child <which>`)
    recs, rc = lt.run([sys.executable, me, "--child", "kernel"])
    for r in recs:
        emit(r)
    if rc:
        emit({"record": "verdict", "error": f"the kernel child ended with {rc}: nothing more was run"})
        return 1
    resid = {(r["m"], r["k"]): r for r in recs if r["record"] == "residual"}
    have_trace = bool(shutil.which("rocprofv3"))
    if have_trace:
        disp, _, rc = lt.traced("stream")
        if disp is None:
            emit({"record": "verdict", "error": f"the stream child ended with {rc}: nothing more was run"})
            return 1
        upd = [ms for name, ms in disp if "gmres_update_kernel<0>" in name or "gmres_update_kernelILi0" in name]
        ratio = {}
        if len(upd) == 64:
            for (m, k), r in resid.items():
                j = min(range(64), key=lambda j: abs(8.0 * N * (j + 3) - r["bytes"]))
                gbps = 8.0 * N * (j + 3) / upd[j] / 1e6
                emit({"record": "update", "nearest": [m, k], "step": j, "ms": upd[j], "bytes": 8.0 * N * (j + 3), "GBps": gbps})
                ratio[f"({m}, {k})"] = r["GBps"] / gbps
            emit({"record": "verdict", "residual_over_update": ratio})
        else:
            emit({"record": "update", "error": f"{len(upd)} dispatches of the first update kernel, 64 expected"})
    else:
        emit({"record": "verdict", "error": "rocprofv3 not found: update and split not measured"})
    for config in CONFIGS:
        recs, rc = lt.run([sys.executable, me, "--child", "e2e:" + config])
        for r in recs:
            emit(r)
        if rc:
            emit({"record": "verdict", "error": f"the e2e child of {config} ended with {rc}: nothing more was run"})
            return 1
        if not have_trace:
            continue
        disp, trecs, rc = lt.traced("e2e:" + config)
        if disp is None:
            emit({"record": "verdict", "error": f"the traced e2e child of {config} ended with {rc}: nothing more was run"})
            return 1
        starts = [i for i, (name, _) in enumerate(disp) if "DotOp" in name]      # dot(v0, v0): the first kernel of a solve
        sums = {}
        for name, ms in disp[starts[-1] if starts else 0:]:
            sums[group(name)] = sums.get(group(name), 0.0) + ms
        base = next(r for r in recs if r["record"] == "eig" and r["solver"] == "davidson")
        sums["jacobi"] = base["jacobiMs"]
        emit({"record": "split", "config": config, "untraced_ms": base["ms"], "group_ms": sums,
              "host_rest_ms": base["ms"] - sum(sums.values()),
              "traced": [r for r in trecs if r.get("record") == "eig" and r.get("solver") == "davidson"]})
    out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
