"""Aggregation multigrid on the device on the 500 x 100 x 100 7-point Laplacian, one JSON line per
step, each step a child process of its own under its own time limit (a step that fails or runs out of time ends the run):

  setup     setup and refresh ms, levels, rows per level, operator complexity, bytes kept
  apply     one cycle in ms against one ILU(0) pair apply (two triangular solves) on the same matrix
  cg        CG to tol = 1e-8 with no dM, with ILU(0), with ILU(0) on the colour-permuted matrix, with the hierarchy:
            iterations and wall ms of each.  The ms are the solver's alone: b is a device tensor, the factorisation, the
            permutation, the setup and a first one-iteration call (kernel selection, triangle analysis) come before the
            clock, and the device is synchronised around the timed call
Nothing here asserts a time.

    python scripts/amg_timing.py [--quick] [--out profiles/amg_timing.log]
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

STEPS = (("setup", 300), ("apply", 300), ("cg", 600))


def problem(api, quick):
    import numpy as np
    import spgemm_ref as sr
    A = sr.laplacian7(*((60, 40, 40) if quick else (500, 100, 100)))
    b = np.random.default_rng(24).standard_normal(A[0])
    return A, b, api.spMatCpyCSR(api.HostCSR(*A))


def timed(fn, reps=5):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def step(name, quick):
    import torch
    from spmv_openmp_cuda_amd import api
    api.spmvHipInit(0)
    A, b, da = problem(api, quick)
    rec = {"step": name, "rows": A[0], "nnz": int(A[3].size)}
    if name == "setup":
        da.amg().free()
        h = da.amg()
        i = h.info
        rec.update(setupMs=i.ms, levels=i.levels, rowsPerLevel=list(i.rows[:i.levels]), nnzPerLevel=list(i.nnz[:i.levels]),
                   opComplexity=i.opComplexity, bytes=i.bytes, tempBytes=i.tempBytes)
        h.refresh_from(da)
        h.refresh_from(da)
        rec["refreshMs"] = h.info.ms
    elif name == "apply":
        h = da.amg()
        r = torch.from_numpy(b).cuda()
        z = torch.empty_like(r)
        rec["cycleMs"] = timed(lambda: h.apply(r, out=z))
        dm = api.spMatCpyCSR(api.HostCSR(*A))
        dm.ilu0()
        w = torch.empty_like(r)
        rec["ilu0PairMs"] = timed(lambda: dm.solve_triangular(dm.solve_triangular(r, lower=True, unit_diagonal=True, out=w), lower=False, out=z))
    else:
        import numpy as np
        def solve(mat, rhs, precond):
            """solver time alone: b on the device, one call of a single iteration first (it makes what a first call makes:
            the SpMV selection, the analysis of dM's triangles), then the timed call between two synchronisations"""
            bt = torch.from_numpy(rhs).cuda()
            mat.cg(bt, precond=precond, tol=1e-8, maxiter=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, info = mat.cg(bt, precond=precond, tol=1e-8, maxiter=5000)
            torch.cuda.synchronize()
            return {"iterations": info.iterations, "status": info.status, "ms": (time.perf_counter() - t0) * 1e3,
                    "launches": info.launches}
        rec["none"] = solve(da, b, None)
        dm = api.spMatCpyCSR(api.HostCSR(*A))
        dm.ilu0()
        rec["ilu0"] = solve(da, b, dm)
        col = da.colour(order="hash")
        perm = col.perm.down(np.uint32)
        pa = da.permute(col)
        pm = da.permute(col)
        pm.ilu0()
        rec["ilu0Coloured"] = dict(solve(pa, b[perm], pm), colours=col.info.colours)
        h = da.amg()
        rec["amg"] = dict(solve(da, b, h), setupMs=h.info.ms)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amg_timing.log"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.quick)
    with open(args.out, "w") as out:
        for name, limit in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + (["--quick"] if args.quick else [])
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                out.write(json.dumps({"step": name, "error": f"time limit of {limit} s"}) + "\n")
                return 1
            line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else json.dumps({"step": name, "error": p.stderr[-400:]})
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            if p.returncode:
                return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
