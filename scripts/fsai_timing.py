"""The approximate-inverse preconditioner on the device: what its setup, its refresh and a
preconditioned iteration cost, and what it buys, against plain CG, ILU(0)-PCG and AMG-PCG in the same run.  One child
process under one time limit; the device is synchronised around every timed call.  One JSON line per record; the log opens
with the estimates, which DESIGN.md section 38 sets against the numbers.  Nothing here asserts a time.

Matrices, 500 x 100 x 100 (5 M rows), made on the device from triplets:
  lap7    the 7-point Laplacian (-1 off the diagonal, 6 on it)
  st19    the 18-neighbour stencil of the shape of the structured stand-in of section 9, made symmetric positive definite:
          -1 for the 6 face and the 12 edge neighbours, 18 on the diagonal
  aniso   the 7-point stencil with the weights (1, 0.01, 0.01) of section 29
Records:
  setup     spmvHipFsaiSetup (the second of two: wall ms and the call's own clock), spmvHipFsaiRefresh, the bytes of G, at
            the built-in group width and at every forced one, for the patterns tril(A) and tril(A A); beside them
            hipSpILU0CSR's first call (analysis and factorisation) and its second (the factorisation)
  parts     serial-order SpMV on A, G and G^T, spmvHipFsaiApply and spmvHipDot: wall ms, the mean of 20 after a first call
  iteration ms per iteration = (solve(maxIter = n2) - solve(maxIter = n1)) / (n2 - n1) at tol = 0, section 19's method
  solve     iterations and wall ms to tol = 1e-8 (the second of two solves)
  block     the 16-column block solve on lap7 with the factor of tril(A), and without a preconditioner

    python scripts/fsai_timing.py [--quick] [--only lap7,aniso,st19] [--out profiles/fsai_timing.log]
Kernel split of a setup: `rocprofv3 --kernel-trace --stats -- python scripts/fsai_timing.py --child --only lap7` in a run of its own.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 1100
ESTIMATES = {
    "iteration": "an apply on lap7 is two SpMVs of 4/7 of A's entries each: an FSAI-PCG iteration should land near 0.184 + 2 x 0.07 + a dot, "
                 "about 0.4 ms, 1/30 of ILU(0)-PCG's 13.48 ms (section 19); none of this was measured before this run",
    "wall": "whether halving the iterations beats plain CG's wall time on the isotropic Laplacian is open (roughly a draw by the estimate); "
            "st19 and aniso are where it should pay",
    "setup": "a setup should cost on the order of one ILU(0) factorisation (6 to 19 ms, section 18)"}
FACE = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
EDGE = [(1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)]


def sync():
    import torch
    torch.cuda.synchronize()


def timed(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def second_of_two(fn):
    fn()
    return timed(fn)


def mean_of(fn, n=20):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    sync()
    return (time.perf_counter() - t0) / n * 1e3


def stencil(api, shape, offsets, diagonal):
    """the symmetric stencil matrix on the grid: offsets is [((dx, dy, dz), weight)] for one of each pair of neighbours"""
    import torch
    nx, ny, nz = shape
    M = nx * ny * nz
    ix, iy, iz = torch.meshgrid(torch.arange(nx, device="cuda"), torch.arange(ny, device="cuda"), torch.arange(nz, device="cuda"), indexing="ij")
    idx = ((ix * ny + iy) * nz + iz).reshape(-1)
    rows, cols, vals = [idx, ], [idx, ], [torch.full((M,), float(diagonal), dtype=torch.float64, device="cuda")]
    for (dx, dy, dz), w in offsets:
        ok = ((ix + dx >= 0) & (ix + dx < nx) & (iy + dy >= 0) & (iy + dy < ny) & (iz + dz >= 0) & (iz + dz < nz)).reshape(-1)
        a = idx[ok]
        b = a + (dx * ny + dy) * nz + dz
        rows += [a, b]
        cols += [b, a]
        vals += [torch.full((a.numel(),), float(w), dtype=torch.float64, device="cuda")] * 2
    r, c, v = torch.cat(rows).to(torch.int32), torch.cat(cols).to(torch.int32), torch.cat(vals)
    A = api.assemble_coo(M, M, r, c, v, keep_map=False)
    del r, c, v
    return A


MATRICES = {
    "lap7": lambda api, s: stencil(api, s, [(o, -1.0) for o in FACE], 6.0),
    "st19": lambda api, s: stencil(api, s, [(o, -1.0) for o in FACE + EDGE], 18.0),
    "aniso": lambda api, s: stencil(api, s, [(o, -w) for o, w in zip(FACE, (1.0, 0.01, 0.01))], 2.0 * 1.02),
}


def per_iteration(A, b, precond, n1, n2):
    A.cg(b, precond=precond, tol=0.0, maxiter=2)
    t1, _ = timed(lambda: A.cg(b, precond=precond, tol=0.0, maxiter=n1))
    t2, (_, info) = timed(lambda: A.cg(b, precond=precond, tol=0.0, maxiter=n2))
    return (t2 - t1) / (n2 - n1), info.launches


def solve(A, b, precond, maxiter=5000):
    ms, (_, info) = second_of_two(lambda: A.cg(b, precond=precond, tol=1e-8, maxiter=maxiter))
    return {"iterations": info.iterations, "status": info.status, "ms": ms, "launches": info.launches, "hostChecks": info.hostChecks}


def out(**rec):
    print(json.dumps(rec), flush=True)


def fsai_records(api, name, A, b, pattern_name, pattern, lanes_list, plain_it):
    import torch
    M = int(A.handle.M)
    best = None
    for lanes in lanes_list:
        wall, g = second_of_two(lambda: A.fsai(pattern=pattern, lanes_per_row=lanes))
        info = g.info()
        rec = dict(record="setup", matrix=name, pattern=pattern_name, lanesPerRow=lanes, setupWallMs=wall, setupMs=info.ms, nnzG=info.nnz, maxRow=info.maxRow,
                   badRows=info.badRows, bytesG=12 * info.nnz + 4 * (M + 1), bytesGT=16 * info.nnz + 4 * (M + 1), launches=info.launches)
        g.refresh_from(A)
        rec["refreshWallMs"], r = timed(lambda: g.refresh_from(A))
        rec["refreshMs"] = r.ms
        out(**rec)
        if lanes == 0:
            best = g
        else:
            g.free()
    g = best
    w, z = torch.empty_like(b), torch.empty_like(b)
    t = g.transpose()                                                    # (a handle of its own for the launcher: the owned one is private)

    def rows(dm):                                                        # hipSpMVRowsCSR: the serial-order selection the solvers enqueue
        return lambda: api._check(api.lib.hipSpMVRowsCSR(C.byref(dm.handle), b.data_ptr(), api.CONFIG(), w.data_ptr()), "hipSpMVRowsCSR")
    parts = {"spmvA": mean_of(rows(A)), "spmvG": mean_of(rows(g)), "spmvGT": mean_of(rows(t)),
             "apply": mean_of(lambda: g.apply(b, out=z)), "dot": mean_of(lambda: api.dot(b, w))}
    t.free()
    out(record="parts", matrix=name, pattern=pattern_name, **parts)
    it, launches = per_iteration(A, b, g, 20, 60)
    out(record="iteration", matrix=name, kind=f"fsai {pattern_name}", msPerIteration=it, launchesOfTheLongerSolve=launches,
        sumOfParts=plain_it + parts["spmvG"] + parts["spmvGT"] + parts["dot"], plainIteration=plain_it)
    out(record="solve", matrix=name, kind=f"fsai {pattern_name}", **solve(A, b, g))
    return g


def child(quick, only):
    import torch
    from spmv_openmp_cuda_amd import api
    api.spmvHipInit(0)
    shape = (60, 40, 40) if quick else (500, 100, 100)
    out(estimates=ESTIMATES, shape=shape, note="wall ms of synchronous calls with the device synchronised around them")
    gen = torch.Generator(device="cuda").manual_seed(38)
    for name in only:
        A = MATRICES[name](api, shape)
        M = int(A.handle.M)
        b = torch.randn(M, dtype=torch.float64, device="cuda", generator=gen)
        out(record="matrix", matrix=name, rows=M, nnz=int(A.handle.NZ))
        plain_it, launches = per_iteration(A, b, None, 20, 60)
        out(record="iteration", matrix=name, kind="plain", msPerIteration=plain_it, launchesOfTheLongerSolve=launches)
        out(record="solve", matrix=name, kind="plain", **solve(A, b, None))
        # ILU(0): its first call (analysis and factorisation), a second factorisation of fresh values
        F = A.tril(3 * shape[1] * shape[2])                              # (a copy of A: the band holds every entry)
        first, _ = timed(F.ilu0)
        F.filter_refresh(A)
        second, info = timed(F.ilu0)
        out(record="setup", matrix=name, pattern="ILU(0)", firstCallWallMs=first, factorisationWallMs=second, factorisationMs=info.ms, levels=info.levels,
            launches=info.launches, zeroPivot=info.zeroPivot)
        it, launches = per_iteration(A, b, F, 4, 12)
        out(record="iteration", matrix=name, kind="ilu0", msPerIteration=it, launchesOfTheLongerSolve=launches)
        out(record="solve", matrix=name, kind="ilu0", **solve(A, b, F))
        F.free()
        ms, h = second_of_two(lambda: A.amg())
        out(record="setup", matrix=name, pattern="AMG", setupWallMs=ms, levels=h.info.levels, opComplexity=h.info.opComplexity)
        out(record="solve", matrix=name, kind="amg", **solve(A, b, h))
        h.free()
        g = fsai_records(api, name, A, b, "tril(A)", None, (4, 16, 64, 0), plain_it)
        if name == "lap7":
            B = torch.randn((M, 16), dtype=torch.float64, device="cuda", generator=gen)
            for kind, pre in (("plain", None), ("fsai tril(A)", g)):
                ms, (_, info) = second_of_two(lambda: A.cg_block(B, precond=pre, tol=1e-8, maxiter=5000))
                out(record="block", matrix=name, kind=kind, columns=16, ms=ms, iterations=info.iterations, status=info.status, launches=info.launches)
            del B
        g.free()
        ms, AA = timed(lambda: A.multiply(A))
        S = AA.tril()
        out(record="pattern", matrix=name, pattern="tril(A A)", productWallMs=ms, nnzAA=int(AA.handle.NZ), nnzPattern=int(S.handle.NZ))
        AA.free()
        fsai_records(api, name, A, b, "tril(A A)", S, (16, 64, 0), plain_it).free()
        S.free()
        A.free()
    out(record="done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsai_timing.log"))
    ap.add_argument("--only", default="lap7,aniso,st19", help="the matrices, of " + ", ".join(MATRICES))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    only = [m for m in args.only.split(",") if m]
    if any(m not in MATRICES for m in only):
        ap.error("--only takes " + ", ".join(MATRICES))
    if args.child:
        return child(args.quick, only)
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
