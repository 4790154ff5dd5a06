"""Triangular solves by Jacobi sweeps on the device: what one sweep costs against the serial-order
SpMV on the same handle, what a preconditioner application of S sweeps per triangle costs against the exact pair of solves,
and what PCG / BiCGStab with it take against exact ILU(0), the approximate inverse and no preconditioner, in the same run.
One child process under one time limit; the device is synchronised around every timed call.  One JSON line per record.
Nothing here asserts a time.

Matrices, 500 x 100 x 100 (5 M rows), made on the device from triplets (those of scripts/fsai_timing.py): lap7, the
18-neighbour stand-in st19, and aniso, the 7-point stencil with the weights (1, 0.01, 0.01) of section 29.  F holds the
ILU(0) factors of each.
Records:
  sweep     hipSpMVRowsCSR on F (the yardstick: a sweep moves the same matrix bytes plus one more vector), a lower (UNIT) and
            an upper (STORED) solve of 1 and of 5 sweeps, ms per sweep = (t5 - t1) / 4, its ratio to the SpMV, and the share
            of the streamed entries that lie outside the strict triangle (what a split copy of the factors would save)
  apply     the two sweep solves of S = 1 .. 5 back to back (S_L + S_U + 1 launches; inside a solver the pair is fused to
            S_L + S_U) against the exact pair of hipSpTRSVCSR
  iteration ms per CG iteration = (solve(maxIter = n2) - solve(maxIter = n1)) / (n2 - n1) at tol = 0, section 19's method
  solve     iterations and wall ms to tol = 1e-8 (the second of two solves), CG and BiCGStab: plain, FSAI, exact ILU(0),
            sweeps S = 1 .. 5 (and 8 on aniso)
  block     the 16-column block CG on lap7: exact ILU(0) against sweeps

    python scripts/tri_sweeps_timing.py [--quick] [--only lap7,aniso,st19] [--out profiles/tri_sweeps_timing.log]
Kernel split: `rocprofv3 --kernel-trace --stats -- python scripts/tri_sweeps_timing.py --child --trace --only lap7` in a run of
its own (--trace leaves the exact ILU(0) solves out: 250 000 launches each).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fsai_timing import MATRICES, mean_of, out, second_of_two, timed  # noqa: E402

LIMIT = 1100


def per_iteration(A, b, precond, n1, n2):
    A.cg(b, precond=precond, tol=0.0, maxiter=2)
    t1, _ = timed(lambda: A.cg(b, precond=precond, tol=0.0, maxiter=n1))
    t2, (_, info) = timed(lambda: A.cg(b, precond=precond, tol=0.0, maxiter=n2))
    return (t2 - t1) / (n2 - n1), info.launches


def solve(A, b, precond, method, maxiter=3000):
    ms, (_, info) = second_of_two(lambda: getattr(A, method)(b, precond=precond, tol=1e-8, maxiter=maxiter))
    return {"iterations": info.iterations, "status": info.status, "ms": ms, "launches": info.launches}


def child(quick, only, trace=False):
    import torch
    from spmv_openmp_cuda_amd import api
    api.spmvHipInit(0)
    shape = (60, 40, 40) if quick else (500, 100, 100)
    out(shape=shape, note="wall ms of synchronous calls with the device synchronised around them")
    gen = torch.Generator(device="cuda").manual_seed(40)
    for name in only:
        A = MATRICES[name](api, shape)
        M, nnz = int(A.handle.M), int(A.handle.NZ)
        b = torch.randn(M, dtype=torch.float64, device="cuda", generator=gen)
        w, z = torch.empty_like(b), torch.empty_like(b)
        out(record="matrix", matrix=name, rows=M, nnz=nnz)
        F = A.tril(3 * shape[1] * shape[2])                              # (a copy of A: the band holds every entry)
        F.ilu0()
        ms, _ = timed(lambda: F.prepare_triangular_sweeps(16 if name == "lap7" else 1))
        plan = F.triangular_sweeps_info()
        out(record="prepare", matrix=name, ms=ms, bytes=plan.bytes, width=plan.width, sorted=plan.sorted)
        # ---- one sweep against the SpMV on the same handle
        spmv = mean_of(lambda: api._check(api.lib.hipSpMVRowsCSR(C.byref(F.handle), b.data_ptr(), api.CONFIG(), w.data_ptr()), "hipSpMVRowsCSR"))
        rec = dict(record="sweep", matrix=name, spmvRowsMs=spmv, kernel=(api.lib.spmvHipAutoChoiceRows(C.byref(F.handle), None) or b"-").decode(),
                   outsideTriangleShare=1.0 - (nnz - M) / 2.0 / nnz)
        for tri, lower, unit in (("lower", True, True), ("upper", False, False)):
            t1 = mean_of(lambda: F.solve_triangular(b, lower=lower, unit_diagonal=unit, out=z, sweeps=1))
            t5 = mean_of(lambda: F.solve_triangular(b, lower=lower, unit_diagonal=unit, out=z, sweeps=5))
            rec[tri + "S1Ms"], rec[tri + "S5Ms"], rec[tri + "SweepMs"] = t1, t5, (t5 - t1) / 4
            rec[tri + "SweepOverSpmv"] = (t5 - t1) / 4 / spmv
        out(**rec)
        # ---- one application: the two sweep solves against the exact pair
        def pair(S):
            F.solve_triangular(b, lower=True, unit_diagonal=True, out=w, sweeps=S)
            F.solve_triangular(w, lower=False, unit_diagonal=False, out=z, sweeps=S)
        if not trace:
            exact = mean_of(lambda: pair(None), 5)
            tinfo = [F.triangular_info(lo) for lo in (True, False)]
            out(record="apply", matrix=name, kind="exact", ms=exact, levels=[int(t.levels) for t in tinfo], launches=int(tinfo[0].launches + tinfo[1].launches))
        for S in (1, 2, 3, 4, 5):
            out(record="apply", matrix=name, kind=f"sweeps {S}", ms=mean_of(lambda: pair(S)), launches=2 * S + 1)
        # ---- iterations and wall time
        plain_it, _ = per_iteration(A, b, None, 20, 60)
        out(record="iteration", matrix=name, kind="plain", msPerIteration=plain_it)
        if not trace:
            it, _ = per_iteration(A, b, F, 4, 12)
            out(record="iteration", matrix=name, kind="ilu0 exact", msPerIteration=it)
        g = A.fsai()
        kinds = [("plain", None, None), ("fsai", g, None), ("ilu0 exact", F, None)] + [(f"sweeps {S}", F, S) for S in (1, 2, 3, 4, 5) + ((8,) if name == "aniso" else ())]
        if trace:                                                        # (under the kernel trace: no exact solves, 250 000 launches each)
            kinds = [("sweeps 3", F, 3)]
        for kind, pre, S in kinds:
            if pre is F:
                F.set_triangular_apply(S)
            if S is not None:
                it, launches = per_iteration(A, b, F, 20, 60)
                out(record="iteration", matrix=name, kind=kind, msPerIteration=it, launchesOfTheLongerSolve=launches)
            for method in ("cg", "bicgstab"):
                out(record="solve", matrix=name, kind=kind, method=method, **solve(A, b, pre, method))
        g.free()
        if name == "lap7":
            B = torch.randn((M, 16), dtype=torch.float64, device="cuda", generator=gen)
            for kind, S in ((("sweeps 3", 3),) if trace else (("ilu0 exact", None), ("sweeps 2", 2), ("sweeps 3", 3))):
                F.set_triangular_apply(S, block_width=16)
                ms, (_, info) = second_of_two(lambda: A.cg_block(B, precond=F, tol=1e-8, maxiter=3000))
                out(record="block", matrix=name, kind=kind, columns=16, ms=ms, iterations=info.iterations, status=info.status, launches=info.launches)
            del B
        F.free()
        A.free()
    out(record="done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tri_sweeps_timing.log"))
    ap.add_argument("--only", default="lap7,st19,aniso", help="the matrices, of " + ", ".join(MATRICES))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", action="store_true", help="with --child: the sweep records only, for a run under the kernel trace")
    args = ap.parse_args()
    only = [m for m in args.only.split(",") if m]
    if any(m not in MATRICES for m in only):
        ap.error("--only takes " + ", ".join(MATRICES))
    if args.child:
        return child(args.quick, only, args.trace)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--only", ",".join(only)] + (["--quick"] if args.quick else [])
    with open(args.out, "w") as f:                                       # (the records reach the log as they are made)
        try:
            p = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, text=True, timeout=LIMIT)
            rc, error = p.returncode, p.stderr[-1200:]
        except subprocess.TimeoutExpired:
            rc, error = 1, f"time limit of {LIMIT} s"
        if rc:
            f.write(json.dumps({"error": error}) + "\n")
    print(open(args.out).read(), end="", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
