"""Smoothed against plain aggregation multigrid on the device, on the problem and by the method of
scripts/amg_timing.py: the 500 x 100 x 100 7-point Laplacian, a standard-normal b from default_rng(24), CG to tol = 1e-8, the
device synchronised around every timed call.  One child process under one time limit makes every hierarchy from the same
uploaded handle, so the plain hierarchy -- the code this work does not change -- is the yardstick of the same run:

  plain          spmvHipAmgSetup
  smoothed       spmvHipAmgSetupSmoothed as it comes: the correction is P_l's SpMV and an add on every level
  smoothedFused  the same hierarchy with spmvHipSetVariant("spmvHipAmgApply", 64): one fused kernel wherever P_l has no
                 row above 64 entries (every level of this problem)

Per hierarchy one JSON line: setup and refresh ms, levels, rows per level, operator complexity, bytes kept, ms per cycle, CG
iterations, solver ms and launches.  The log opens with the hypothesis and closes with what the numbers say of it.
Nothing here asserts a time.

    python scripts/amg_sa_timing.py [--quick] [--out profiles/amg_sa_timing.log]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LIMIT = 900
HYPOTHESIS = ("the smoothed hierarchy takes fewer CG iterations than the plain one (reference CG on the CPU: 13 against 18 on "
              "12 x 10 x 8, 16 against 27 on 24 x 20 x 16); whether its solver ms are lower is not known: its coarse operators "
              "are denser, and P and R stream values")
KINDS = (("plain", dict(), 0), ("smoothed", dict(smoothed=True), 0), ("smoothedFused", dict(smoothed=True), 64))


def timed(fn, reps=20):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def child(quick):
    import numpy as np
    import torch
    import spgemm_ref as sr
    from spmv_openmp_cuda_amd import api
    api.spmvHipInit(0)
    A = sr.laplacian7(*((60, 40, 40) if quick else (500, 100, 100)))
    b = np.random.default_rng(24).standard_normal(A[0])
    da = api.spMatCpyCSR(api.HostCSR(*A))
    bt = torch.from_numpy(b).cuda()
    z = torch.empty_like(bt)
    print(json.dumps({"hypothesis": HYPOTHESIS, "rows": A[0], "nnz": int(A[3].size)}), flush=True)
    recs = {}
    for name, kw, threshold in KINDS:
        api.set_variant("spmvHipAmgApply", threshold)
        da.amg(**kw).free()                                          # (a first setup makes what a first call makes)
        h = da.amg(**kw)
        i = h.info
        rec = dict(hierarchy=name, setupMs=i.ms, levels=i.levels, rowsPerLevel=list(i.rows[:i.levels]), nnzPerLevel=list(i.nnz[:i.levels]),
                   opComplexity=i.opComplexity, bytes=i.bytes, tempBytes=i.tempBytes)
        if kw:
            import ctypes as C
            rec["omegaP"] = []
            for l in range(i.levels - 1):                            # (the damping alone: no download of P and R)
                w = C.c_double()
                api.lib.spmvHipAmgProlongator(C.byref(h.handle), l, None, None, C.byref(w))
                rec["omegaP"].append(w.value)
        h.refresh_from(da)
        h.refresh_from(da)
        rec["refreshMs"] = h.info.ms
        rec["cycleMs"] = timed(lambda: h.apply(bt, out=z))
        da.cg(bt, precond=h, tol=1e-8, maxiter=1)                    # (the solver's first call, before the clock)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = da.cg(bt, precond=h, tol=1e-8, maxiter=5000)
        torch.cuda.synchronize()
        rec["cg"] = {"iterations": info.iterations, "status": info.status, "ms": (time.perf_counter() - t0) * 1e3, "launches": info.launches}
        h.free()
        recs[name] = rec
        print(json.dumps(rec), flush=True)
    p, s, f = recs["plain"], recs["smoothed"], recs["smoothedFused"]
    print(json.dumps({"verdict": {
        "fewerIterations": s["cg"]["iterations"] < p["cg"]["iterations"],
        "iterations": [p["cg"]["iterations"], s["cg"]["iterations"]],
        "solverMsPlainSmoothed": [p["cg"]["ms"], s["cg"]["ms"]],
        "smoothedSolverIsFaster": s["cg"]["ms"] < p["cg"]["ms"],
        "cycleMsSplitFused": [s["cycleMs"], f["cycleMs"]],
        "solverMsSplitFused": [s["cg"]["ms"], f["cg"]["ms"]],
        "fusedCorrectionPays": f["cycleMs"] < s["cycleMs"]}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amg_sa_timing.log"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.quick)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--quick"] if args.quick else [])
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        text, rc = p.stdout, p.returncode
        if rc:
            text += json.dumps({"error": p.stderr[-400:]}) + "\n"
    except subprocess.TimeoutExpired as e:
        text, rc = (e.stdout or b"").decode() + json.dumps({"error": f"time limit of {LIMIT} s"}) + "\n", 1
    print(text, end="", flush=True)
    with open(args.out, "w") as out:
        out.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
