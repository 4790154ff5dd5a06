"""Multicolour Gauss-Seidel against damped-Jacobi and Chebyshev smoothing of the multigrid cycle on the device (DESIGN.md
section 32), on the problem and by the method of scripts/amg_cheb_timing.py: the 500 x 100 x 100 7-point Laplacian, a
standard-normal b from default_rng(24), CG to tol = 1e-8, the device synchronised around every timed call, a first
one-iteration solve before the clock.  One child process under one time limit.

Per sweep on level 0: a one-level hierarchy of the same handle, whose cycle is nuCoarse sweeps and nothing else; the cost of a
sweep is (cycle at 5 sweeps - cycle at 1 sweep) / 4, for Jacobi (a serial-order SpMV and the sweep pass) and for Gauss-Seidel
under both orders (one launch per colour) with 1, 4, 8 and 16 lanes per row in the same run (1 is the lane-per-row form, 4
what the default picks for a mean row of 7 entries).

Per solve: a plain and a smoothed hierarchy from the same handle, every variant from the same hierarchy, the parent's smoothers
-- code this work does not change -- as the yardsticks of the same run:

  jacobi        nu1 = nu2 = 1                 (the default)
  chebyshev     nu1 = nu2 = 3, eigRatio 10    (the best of DESIGN.md section 30)
  gauss-seidel  nu1 = nu2 = 1, 2;  levels all, 1, 2;  small-level threshold 0 and the default;  NATURAL and HASH
                (the lanes per row by each level's mean row, the default); and with a lane per row: levels all and 1, NATURAL

The variants run ROUNDS times in turn (one after the other, then again), so that a drift of the machine falls on all of them
alike; per variant one JSON line: CG iterations, launches, ms per cycle and solver ms (median and least over the rounds), the
ms of the set call and the colours per level.  The log opens with the hypothesis and closes with what the numbers say of it.
Nothing here asserts a time.

    python scripts/amg_gs_timing.py [--quick] [--out profiles/amg_gs_timing.log]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LIMIT = 900
ROUNDS = 3
HYPOTHESIS = ("(1) Gauss-Seidel takes fewer CG iterations than Jacobi at the same sweep count (reference CG on the CPU, 24 x 20 x 16: "
              "21 against 27 and 15 against 20 on the plain hierarchy, 12 against 16 and 8 against 12 on the smoothed one); (2) a sweep "
              "on level 0 costs about one Jacobi sweep: it streams A_0 once plus r, dinv, z and perm where Jacobi streams A_0 and five "
              "vectors -- but the rows of a colour are every other row, so the two colour launches may each fetch every line of A_0: the "
              "gather through perm is the unknown, and up to twice the matrix traffic would not surprise; (3) the coarse levels take 8 "
              "to 18 colours, so a launch per colour costs launches that the one-workgroup sweep saves.  Whether any Gauss-Seidel "
              "variant beats Jacobi nu = 1 or Chebyshev nu = 3 in solver ms is not known and is the question; CG's solver ms steps with "
              "ceil(iterations / 16)")
HIERARCHIES = (("plain", dict()), ("smoothed", dict(smoothed=True)))
DEFAULT_SMALL = 1024
GS = [("gauss-seidel", nu, levels, small, order, 0) for nu in (1, 2) for levels in (None, 1, 2) for small in (0, DEFAULT_SMALL)
      for order in ("natural", "hash")]
GS1 = [("gauss-seidel", nu, levels, DEFAULT_SMALL, "natural", 1) for nu in (1, 2) for levels in (None, 1)]      # a lane per row
VARIANTS = [("jacobi", 1, None, DEFAULT_SMALL, None, 0), ("chebyshev", 3, None, DEFAULT_SMALL, None, 0)] + GS + GS1


def timed(fn, reps=20):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def name_of(kind, nu, levels, small, order, lanes):
    if kind != "gauss-seidel":
        return f"{kind} nu={nu}" + (" eigRatio=10" if kind == "chebyshev" else "")
    return f"{kind} nu={nu} levels={'all' if levels is None else levels} small={small} {order} lanes={lanes or 'by the mean row'}"


def set_variant(api, h, v):
    kind, nu, levels, small, order, lanes = v
    if kind == "gauss-seidel":
        api.set_variant("spmvHipAmgSetGaussSeidel", small)
        api.set_variant("spmvHipAmgGaussSeidel", lanes)
        h.set_gauss_seidel(order=order, levels=levels, nu1=nu, nu2=nu)
    else:
        h.set_smoother(kind, nu1=nu, nu2=nu, eig_ratio=10.0 if kind == "chebyshev" else None)


def sweep_cost(api, da, bt, z):
    """ms per sweep on level 0 from a one-level hierarchy: (cycle at 5 sweeps - cycle at 1) / 4, three rounds in turn"""
    import torch
    h = da.amg(maxLevels=1)
    kinds = ("jacobi",) + tuple(f"gauss-seidel {order} lanes={g}" for order in ("natural", "hash") for g in (1, 4, 8, 16))
    runs = {k: [] for k in kinds}
    colours = {}
    for _ in range(ROUNDS):
        for k in kinds:
            ms = {}
            for q in (1, 5):
                if k == "jacobi":
                    h.set_smoother("jacobi", nuCoarse=q)
                else:
                    api.set_variant("spmvHipAmgGaussSeidel", int(k.split("=")[1]))
                    h.set_gauss_seidel(order=k.split()[1], nuCoarse=q)
                    colours[k] = h.gauss_seidel(0)["colours"]
                torch.cuda.synchronize()
                ms[q] = timed(lambda: h.apply(bt, out=z))
            runs[k].append((ms[5] - ms[1]) / 4)
    h.free()
    api.set_variant("spmvHipAmgGaussSeidel", 0)
    out = {k: dict(msPerSweep=statistics.median(v), msPerSweepMin=min(v), colours=colours.get(k)) for k, v in runs.items()}
    for k in kinds[1:]:
        out[k]["overJacobi"] = round(out[k]["msPerSweep"] / out["jacobi"]["msPerSweep"], 3)
    return out


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
    print(json.dumps({"hypothesis": HYPOTHESIS, "rows": A[0], "nnz": int(A[3].size), "rounds": ROUNDS}), flush=True)
    sweeps = sweep_cost(api, da, bt, z)
    print(json.dumps({"perSweepOnLevel0": sweeps}), flush=True)
    verdict = {"sweepOverJacobi": {k: v.get("overJacobi") for k, v in sweeps.items() if k != "jacobi"}}
    for hname, kw in HIERARCHIES:
        da.amg(**kw).free()                                          # (a first setup makes what a first call makes)
        h = da.amg(**kw)
        i = h.info
        print(json.dumps(dict(hierarchy=hname, setupMs=i.ms, levels=i.levels, rowsPerLevel=list(i.rows[:i.levels]), opComplexity=i.opComplexity,
                              bytes=i.bytes)), flush=True)
        runs = {v: [] for v in VARIANTS}
        colours = {}
        for _ in range(ROUNDS):
            for v in VARIANTS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                set_variant(api, h, v)
                torch.cuda.synchronize()
                set_ms = (time.perf_counter() - t0) * 1e3
                if v[0] == "gauss-seidel":
                    colours[v] = [h.gauss_seidel(l)["colours"] if h.gauss_seidel(l)["active"] else None for l in range(i.levels)]
                cycle_ms = timed(lambda: h.apply(bt, out=z))
                da.cg(bt, precond=h, tol=1e-8, maxiter=1)            # (the solver's first call, before the clock)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, info = da.cg(bt, precond=h, tol=1e-8, maxiter=5000)
                torch.cuda.synchronize()
                runs[v].append(dict(setMs=set_ms, cycleMs=cycle_ms, ms=(time.perf_counter() - t0) * 1e3, iterations=info.iterations,
                                    status=info.status, launches=info.launches))
        recs = {}
        for v in VARIANTS:
            rs = runs[v]
            assert len({(r["iterations"], r["status"], r["launches"]) for r in rs}) == 1, "the counts do not depend on the round"
            med = lambda k: statistics.median(r[k] for r in rs)
            recs[v] = dict(hierarchy=hname, variant=name_of(*v), iterations=rs[0]["iterations"], status=rs[0]["status"], launches=rs[0]["launches"],
                           cycleMs=med("cycleMs"), cycleMsMin=min(r["cycleMs"] for r in rs), solverMs=med("ms"), solverMsMin=min(r["ms"] for r in rs),
                           setMs=med("setMs"), coloursPerLevel=colours.get(v))
            print(json.dumps(recs[v]), flush=True)
        h.free()
        jac, che = recs[VARIANTS[0]], recs[VARIANTS[1]]
        best = min(GS + GS1, key=lambda v: recs[v]["solverMs"])
        same = lambda nu, small, lanes=0: recs[("gauss-seidel", nu, None, small, "natural", lanes)]
        verdict[hname] = {
            "iterations": {"jacobi nu=1": jac["iterations"], "chebyshev nu=3": che["iterations"],
                           "gauss-seidel nu=1": same(1, DEFAULT_SMALL)["iterations"], "gauss-seidel nu=2": same(2, DEFAULT_SMALL)["iterations"]},
            "cycleMsOverJacobiNu1": {"gauss-seidel nu=1": round(same(1, DEFAULT_SMALL)["cycleMs"] / jac["cycleMs"], 3),
                                     "gauss-seidel nu=1, a launch per colour everywhere": round(same(1, 0)["cycleMs"] / jac["cycleMs"], 3),
                                     "gauss-seidel nu=1, a lane per row": round(same(1, DEFAULT_SMALL, 1)["cycleMs"] / jac["cycleMs"], 3)},
            "solverMs": {"jacobi nu=1": round(jac["solverMs"], 2), "chebyshev nu=3": round(che["solverMs"], 2)},
            "bestGaussSeidel": {"variant": recs[best]["variant"], "solverMs": round(recs[best]["solverMs"], 2), "iterations": recs[best]["iterations"]},
            "bestGaussSeidelBeatsJacobiNu1": recs[best]["solverMs"] < jac["solverMs"],
            "bestGaussSeidelBeatsChebyshevNu3": recs[best]["solverMs"] < che["solverMs"],
        }
    api.set_variant("spmvHipAmgSetGaussSeidel", DEFAULT_SMALL)
    api.set_variant("spmvHipAmgGaussSeidel", 0)
    print(json.dumps({"verdict": verdict}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amg_gs_timing.log"))
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
