"""Per-call host cost of the Python layer (spmv_openmp_cuda_amd/api.py) at a toy size, for an A/B of two trees.

These are OVERHEADS by design: 27-row operands, the library in its default synchronous mode, so a call is the Python
marshalling, one ctypes call, a few tiny kernels and the wait for them.  They say what a user's own loop around dot(),
solve_triangular() or AmgHierarchy.apply() pays per call, and nothing about solver performance.

One repeat (--one, a process of its own), after a warm-up, microseconds per call:
  dot_us          api.dot(u, v)                        device call, --calls times
  trsv_us         DeviceMatrix.solve_triangular(b)     device call, --calls times (ILU(0) factors, lower unit triangle)
  apply_us        AmgHierarchy.apply(r)                device call, --calls times
  trsv_host_us    solve_triangular(numpy b)            host call (upload, solve, download), --host-calls times
The A/B (--parent DIR, a second tree with a built spmv_openmp_cuda_amd/ in it): --repeats repeats of each tree,
alternating parent / new, every repeat a fresh process with a time limit of its own, one after the other; the first repeat
that fails ends the run.  The measure is the parent: for each timing the new median may exceed the parent's median by at
most the parent's own spread over its repeats (slowest minus fastest); the exit status is 1 when one does.

    python scripts/api_call_overhead.py --parent ../parent-tree [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMINGS = ("dot_us", "trsv_us", "apply_us", "trsv_host_us")


def one(root, calls, host_calls):
    sys.path.insert(0, os.path.abspath(root))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    from spgemm_ref import laplacian7
    from spmv_openmp_cuda_amd import api
    api.spmvHipInit(0)
    A = laplacian7(3, 3, 3)
    da, F = api.spMatCpyCSR(api.HostCSR(*A)), api.spMatCpyCSR(api.HostCSR(*A))
    F.ilu0()
    h = da.amg(coarseRows=4)
    hb = np.random.default_rng(1).standard_normal(A[0])
    b = torch.from_numpy(hb).cuda()
    cases = {"dot_us": (lambda: api.dot(b, b), calls),
             "trsv_us": (lambda: F.solve_triangular(b, lower=True, unit_diagonal=True), calls),
             "apply_us": (lambda: h.apply(b), calls),
             "trsv_host_us": (lambda: F.solve_triangular(hb, lower=True, unit_diagonal=True), host_calls)}
    rec = {"api": os.path.relpath(api.__file__, os.path.abspath(root))}
    for name, (call, n) in cases.items():
        for _ in range(max(n // 10, 20)):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        rec[name] = round((time.perf_counter() - t0) / n * 1e6, 3)
    for d in (h, F, da):
        d.free()
    api.spmvHipFinalize()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", metavar="TREE", help="one repeat on the package of this tree")
    ap.add_argument("--parent", metavar="TREE", help="the tree to measure against")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--host-calls", type=int, default=300)
    ap.add_argument("--limit", type=int, default=120, help="seconds one repeat may take")
    ap.add_argument("--out", help="also append every record to this file (default: standard output only)")
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.calls, args.host_calls)
    if not args.parent:
        raise SystemExit("--parent TREE or --one TREE")
    runs = {"parent": [], "new": []}
    with open(args.out or os.devnull, "a") as out:
        for r in range(args.repeats):
            for label, tree in (("parent", args.parent), ("new", ROOT)):
                cmd = [sys.executable, os.path.abspath(__file__), "--one", tree, "--calls", str(args.calls), "--host-calls",
                       str(args.host_calls)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                if p.returncode:
                    raise SystemExit(f"repeat {r} of {label} ended with status {p.returncode}:\n{p.stderr[-2000:]}")
                rec = dict(json.loads(p.stdout.strip().splitlines()[-1]), tree=label, repeat=r)
                runs[label].append(rec)
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
                out.flush()
        slower = []
        for t in TIMINGS:
            par, new = [x[t] for x in runs["parent"]], [x[t] for x in runs["new"]]
            rec = {"timing": t, "parent_median": statistics.median(par), "new_median": statistics.median(new),
                   "parent_spread": round(max(par) - min(par), 3)}
            rec["within_parent_spread"] = rec["new_median"] - rec["parent_median"] <= rec["parent_spread"]
            if not rec["within_parent_spread"]:
                slower.append(t)
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
