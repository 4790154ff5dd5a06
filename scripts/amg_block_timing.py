"""The multigrid cycle for a block of vectors and a hierarchy as dM of the block solvers on the device,
by the method of scripts/amg_cheb_timing.py on the problem of scripts/amg_sa_timing.py: the 500 x 100 x 100 7-point
Laplacian, standard-normal right-hand sides from default_rng(24), CG to tol = 1e-8, device events around synchronised work,
every shape run once before the clock, ROUNDS rounds in turn with medians.  One child process under one time limit, one
smoothed hierarchy with a block workspace of width 32:

  (a) ms per block cycle at k = 1, 2, 4, 8, 16, 32 against k times the single cycle of the same hierarchy in the same run,
      with Jacobi nu = 1 and with Chebyshev nu = 3 at eigRatio 10;
  (b) cg_block with the hierarchy at k = 16 against sixteen cg solves with it, and against cg_block with ILU(0): ms per
      iteration, iterations, total ms.

The log opens with the hypothesis and closes with what the numbers say of it.  Nothing here asserts a time.  (c), the
per-pass table, is a separate run of the quick mode under a kernel trace (profiles/amg_block_kernels_trace.txt).

    python scripts/amg_block_timing.py [--quick] [--parts a] [--out profiles/amg_block_timing.log]
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
WIDTHS = (1, 2, 4, 8, 16, 32)
SMOOTHERS = (("jacobi", 1, None), ("chebyshev", 3, 10.0))
HYPOTHESIS = ("from the measured parts (0.61 ms per SpMM of A at k = 16, block passes at 4.8-5.4 TB/s, a single smoothed Jacobi nu = 1 "
              "cycle at 0.625 ms): level 0 of a 16-column cycle is two SpMMs with A, one each with R and P and about 96 B per row and "
              "column of pass traffic, roughly 1.5 ms at 5 TB/s, so about 4 ms for sixteen columns against 10 ms for sixteen single "
              "cycles.  (1) a 16-column cycle costs less than eight single cycles measured in the same run; (2) a 16-column AMG-PCG "
              "solve costs less than the 16-column ILU(0)-PCG solve")


def event_ms(fn, reps):
    """ms per call: device events around `reps` calls, the device synchronised before and after; one call before the clock"""
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def child(quick, parts):
    import numpy as np
    import torch
    import spgemm_ref as sr
    from spmv_openmp_cuda_amd import api
    api.spmvHipInit(0)
    A = sr.laplacian7(*((60, 40, 40) if quick else (500, 100, 100)))
    M = A[0]
    B = np.random.default_rng(24).standard_normal((M, max(WIDTHS)))
    da = api.spMatCpyCSR(api.HostCSR(*A))
    dilu = api.spMatCpyCSR(api.HostCSR(*A))
    dilu.ilu0()
    Bt = torch.from_numpy(B).cuda()
    print(json.dumps({"hypothesis": HYPOTHESIS, "rows": M, "nnz": int(A[3].size), "rounds": ROUNDS, "where": "device events / host wall clock"}), flush=True)
    da.amg(smoothed=True).free()                                     # (a first setup makes what a first call makes)
    h = da.amg(smoothed=True)
    before = int(h.info.bytes)
    ms, _ = wall_ms(lambda: h.set_block_width(max(WIDTHS)))
    i = h.info
    print(json.dumps(dict(hierarchy="smoothed", levels=i.levels, rowsPerLevel=list(i.rows[:i.levels]), bytesWithout=before, bytes=int(i.bytes),
                          block=h.block_info(), setBlockWidthMs=ms)), flush=True)
    reps = 5 if quick else 20
    # ---- (a) the cycle
    cycles = {}
    for kind, nu, e in SMOOTHERS:
        h.set_smoother(kind, nu1=nu, nu2=nu, eig_ratio=e)
        name = f"{kind} nu={nu}" + (f" eigRatio={e:g}" if e else "")
        r1, z1 = Bt[:, 0].contiguous(), torch.empty(M, dtype=torch.float64, device="cuda")
        blocks = {k: (Bt[:, :k].contiguous(), torch.empty((M, k), dtype=torch.float64, device="cuda")) for k in WIDTHS}
        runs = {k: [] for k in (0,) + WIDTHS}
        for _ in range(ROUNDS):
            runs[0].append(event_ms(lambda: h.apply(r1, out=z1), reps))
            for k in WIDTHS:
                R, Z = blocks[k]
                runs[k].append(event_ms(lambda: h.apply_block(R, out=Z), reps))
        single = statistics.median(runs[0])
        print(json.dumps(dict(part="a", smoother=name, k="single", cycleMs=single, cycleMsMin=min(runs[0]))), flush=True)
        for k in WIDTHS:
            med = statistics.median(runs[k])
            cycles[(name, k)] = (med, single)
            print(json.dumps(dict(part="a", smoother=name, k=k, cycleMs=med, cycleMsMin=min(runs[k]), kSingleCyclesMs=k * single,
                                  inSingleCycles=med / single, perColumnOverSingle=med / (k * single))), flush=True)
        del blocks
    if "b" not in parts:
        h.free()
        return
    # ---- (b) the solves, k = 16
    k = 16
    B16 = Bt[:, :k].contiguous()
    solves = {}
    for kind, nu, e in SMOOTHERS:
        h.set_smoother(kind, nu1=nu, nu2=nu, eig_ratio=e)
        name = f"{kind} nu={nu}" + (f" eigRatio={e:g}" if e else "")
        da.cg_block(B16, precond=h, tol=1e-8, maxiter=1)             # (the solvers' first calls, before the clock)
        da.cg(B16[:, 0].contiguous(), precond=h, tol=1e-8, maxiter=1)
        runs = {"block": [], "sixteen": []}
        for _ in range(ROUNDS):
            ms, (_, info) = wall_ms(lambda: da.cg_block(B16, precond=h, tol=1e-8, maxiter=5000))
            runs["block"].append((ms, info.iterations, info.launches, [c.iterations for c in info.columns]))
            total, its = 0.0, []
            for c in range(k):
                bc = B16[:, c].contiguous()
                ms, (_, one) = wall_ms(lambda: da.cg(bc, precond=h, tol=1e-8, maxiter=5000))
                total += ms
                its.append(one.iterations)
            runs["sixteen"].append((total, its))
        blk = statistics.median(r[0] for r in runs["block"])
        six = statistics.median(r[0] for r in runs["sixteen"])
        assert runs["block"][0][3] == runs["sixteen"][0][1], "a column of the block takes the iterations of its single solve"
        solves[name] = blk
        print(json.dumps(dict(part="b", solve="cg_block with the hierarchy", smoother=name, k=k, iterations=runs["block"][0][1], launches=runs["block"][0][2],
                              columnIterations=runs["block"][0][3], ms=blk, msMin=min(r[0] for r in runs["block"]), msPerIteration=blk / runs["block"][0][1])), flush=True)
        print(json.dumps(dict(part="b", solve="sixteen cg solves with the hierarchy", smoother=name, iterations=runs["sixteen"][0][1], ms=six,
                              msMin=min(r[0] for r in runs["sixteen"]), msPerIteration=six / sum(runs["sixteen"][0][1]), blockOverSixteen=blk / six)), flush=True)
    da.cg_block(B16, precond=dilu, tol=1e-8, maxiter=1)
    runs = []
    for _ in range(ROUNDS):
        ms, (_, info) = wall_ms(lambda: da.cg_block(B16, precond=dilu, tol=1e-8, maxiter=5000))
        runs.append((ms, info.iterations, info.launches, info.status))
    ilu = statistics.median(r[0] for r in runs)
    print(json.dumps(dict(part="b", solve="cg_block with ILU(0)", k=k, iterations=runs[0][1], launches=runs[0][2], status=runs[0][3], ms=ilu,
                          msMin=min(r[0] for r in runs), msPerIteration=ilu / max(runs[0][1], 1))), flush=True)
    jac, cheb = (f"{kind} nu={nu}" + (f" eigRatio={e:g}" if e else "") for kind, nu, e in SMOOTHERS)
    verdict = {
        "sixteenColumnCycleInSingleCycles": {n: round(cycles[(n, 16)][0] / cycles[(n, 16)][1], 2) for n in (jac, cheb)},
        "hypothesis1_lessThanEightSingleCycles": {n: cycles[(n, 16)][0] < 8 * cycles[(n, 16)][1] for n in (jac, cheb)},
        "amgBlockSolveMs": {n: round(v, 1) for n, v in solves.items()}, "ilu0BlockSolveMs": round(ilu, 1),
        "hypothesis2_amgSolveLessThanIlu0Solve": {n: v < ilu for n, v in solves.items()},
    }
    print(json.dumps({"verdict": verdict}), flush=True)
    h.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amg_block_timing.log"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parts", default="ab", help="a: the cycles alone (what a kernel trace of the full size needs)")
    args = ap.parse_args()
    if args.child:
        return child(args.quick, args.parts)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--parts", args.parts] + (["--quick"] if args.quick else [])
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
