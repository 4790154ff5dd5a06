"""Single-precision value storage: what a product from the f32 form costs against the same kernel form on
the doubles and against the serial-order selection's pick, what the byte model predicted, what the factor stored in single
precision does to an FSAI-PCG and an AMG-PCG iteration and solve, and what the form costs to build and to keep.  One child
process per matrix, each under its own time limit; the device is synchronised around every timed call.  A solve or a setup is
the second of two calls.  A single product takes 0.07 to 0.26 ms, of the order of the host's own launch-and-synchronise cost, so a
product is recorded twice: the second of two calls, as every other figure here (the fields ending in 2), and the mean of 20
launches after a first between two synchronisations, which is what DESIGN.md section 41 tabulates.  One JSON line per record.
Nothing here asserts a time.

Matrices: the three 500 x 100 x 100 stencils of scripts/fsai_timing.py (lap7, aniso, st19).
Records:
  product   on A, on G = FSAI(tril A) and on G^T: the serial-order selection's pick and its ms; the f64 LDS-stream kernel forced
            (variant 1 of hipSpMVRowsCSR) -- the yardstick: the same kernel form on the same handle --; hipSpMVRowsCSRf32; the bytes
            of each by the model (12 or 8 B per entry, 4 per row pointer, 8 per element of x and y) and the ratio it predicts
  spmm      k = 16 on lap7, hipSpMMRowsCSR against hipSpMMRowsCSRf32
  iteration, solve   FSAI-PCG with the factor in F64 and in F32: ms per iteration by section 19's method, iterations and wall ms
            to tol = 1e-8; on lap7 the 16-column block CG too
  amg       AMG-PCG with the default hierarchy and with the smoothed hierarchy under the Chebyshev smoother, in F64 and in F32:
            ms of one cycle, ms per iteration, iterations and wall ms to tol = 1e-8, the bytes the f32 forms add over all levels;
            on lap7 the 16-column block CG with the default hierarchy
  setup     spmvHipValuesF32 (a build; released and built again), and spmvHipValuesChanged with and without the form; the bytes

    python scripts/values_f32_timing.py [--quick] [--only lap7,aniso,st19] [--out profiles/values_f32_timing.log]
Kernel split: `rocprofv3 --kernel-trace --stats -- python scripts/values_f32_timing.py --child --only lap7` in a run of its own.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from fsai_timing import MATRICES, mean_of, out, per_iteration, second_of_two, solve, timed  # noqa: E402

LIMIT = 420                                                              # seconds, for one matrix's child


def model_bytes(M, N, nnz, value_bytes):
    return (4 + value_bytes) * nnz + 4 * (M + 1) + 8 * N + 8 * M


def product_records(api, matrix, what, dm, x, y):
    H, cfg = C.byref(dm.handle), api.CONFIG()
    M, N, nnz = int(dm.handle.M), int(dm.handle.N), int(dm.handle.NZ)

    def call(name):
        return lambda: api._check(getattr(api.lib, name)(H, x.data_ptr(), cfg, y.data_ptr()), name)
    api.set_variant("hipSpMVRowsCSR", 2)
    pick_ms = mean_of(call("hipSpMVRowsCSR"))
    pick = (api.lib.spmvHipAutoChoiceRows(H, None) or b"-").decode()
    api.set_variant("hipSpMVRowsCSR", 1)
    stream_ms = mean_of(call("hipSpMVRowsCSR"))
    api.set_variant("hipSpMVRowsCSR", 2)
    build_ms, _ = timed(dm.values_f32)
    f32_ms = mean_of(call("hipSpMVRowsCSRf32"))
    f32_2, _ = second_of_two(call("hipSpMVRowsCSRf32"))
    pick_2, _ = second_of_two(call("hipSpMVRowsCSR"))
    api.set_variant("hipSpMVRowsCSR", 1)
    stream_2, _ = second_of_two(call("hipSpMVRowsCSR"))
    api.set_variant("hipSpMVRowsCSR", 2)
    b64, b32 = model_bytes(M, N, nnz, 8), model_bytes(M, N, nnz, 4)
    out(record="product", matrix=matrix, handle=what, rows=M, nnz=nnz, pick=pick, pickMs=pick_ms, f64StreamMs=stream_ms, f32Ms=f32_ms,
        f32OverF64Stream=f32_ms / stream_ms, f32OverPick=f32_ms / pick_ms, modelBytesF64=b64, modelBytesF32=b32, modelRatio=b32 / b64,
        f64StreamGBs=b64 / stream_ms * 1e-6, f32GBs=b32 / f32_ms * 1e-6, pickMs2=pick_2, f64StreamMs2=stream_2, f32Ms2=f32_2, buildMs=build_ms, formBytes=int(dm.values_f32_info().bytes))


def amg_records(api, name, A, b, y, gen):
    """AMG-PCG with the hierarchy in F64 and in F32: the default hierarchy, and the smoothed one with the Chebyshev smoother"""
    import torch
    for kind, make in (("default", lambda: A.amg()), ("smoothed chebyshev", lambda: A.amg(smoothed=True))):
        h = make()
        if kind != "default":
            h.set_smoother("chebyshev")
        for storage in ("f64", "f32"):
            ms, _ = second_of_two(lambda: h.set_storage(storage))
            info = h.storage_info()
            cycle = mean_of(lambda: h.apply(b, out=y))
            it, _ = per_iteration(A, b, h, 10, 30)
            out(record="amg", matrix=name, hierarchy=kind, storage=storage, levels=info["levels"], f32Bytes=info["f32_bytes"], setStorageMs=ms,
                cycleMs=cycle, msPerIteration=it, **solve(A, b, h))
        if name == "lap7" and kind == "default":
            B = torch.randn((int(A.handle.M), 16), dtype=torch.float64, device="cuda", generator=gen)
            h.set_block_width(16)
            for storage in ("f64", "f32"):
                h.set_storage(storage)
                ms, (_, info) = second_of_two(lambda: A.cg_block(B, precond=h, tol=1e-8, maxiter=5000))
                out(record="block", matrix=name, kind=f"amg default {storage}", columns=16, ms=ms, iterations=info.iterations, status=info.status)
            del B
        h.set_storage("f64")                                             # (releases the form it built on A)
        h.free()


def child(quick, only):
    import torch
    from spmv_openmp_cuda_amd import api
    api.spmvHipInit(0)
    shape = (60, 40, 40) if quick else (500, 100, 100)
    out(shape=shape, note="wall ms of synchronous calls with the device synchronised around them; nothing here was measured before this run")
    gen = torch.Generator(device="cuda").manual_seed(41)
    for name in only:
        A = MATRICES[name](api, shape)
        M = int(A.handle.M)
        b = torch.randn(M, dtype=torch.float64, device="cuda", generator=gen)
        y = torch.empty_like(b)
        out(record="matrix", matrix=name, rows=M, nnz=int(A.handle.NZ))
        g = A.fsai()
        t = g.transpose()                                                # (a handle of its own for the launchers: the owned one is private)
        # the solves first: the factor's own handles choose their kernels there, as in section 38
        plain_it, _ = per_iteration(A, b, None, 20, 60)
        for storage in ("f64", "f32"):
            g.set_storage(storage)
            it, launches = per_iteration(A, b, g, 20, 60)
            out(record="iteration", matrix=name, kind=f"fsai {storage}", msPerIteration=it, plainIteration=plain_it, launchesOfTheLongerSolve=launches)
            out(record="solve", matrix=name, kind=f"fsai {storage}", **solve(A, b, g))
            out(record="apply", matrix=name, kind=f"fsai {storage}", ms=mean_of(lambda: g.apply(b, out=y)))
        if name == "lap7":
            B = torch.randn((M, 16), dtype=torch.float64, device="cuda", generator=gen)
            Y = torch.empty_like(B)
            for storage in ("f64", "f32"):
                g.set_storage(storage)
                ms, (_, info) = second_of_two(lambda: A.cg_block(B, precond=g, tol=1e-8, maxiter=5000))
                out(record="block", matrix=name, kind=f"fsai {storage}", columns=16, ms=ms, iterations=info.iterations, status=info.status)
            A.values_f32()
            for values in ("f64", "f32"):
                out(record="spmm", matrix=name, columns=16, values=values, ms=mean_of(lambda: A.matmul(B, out=Y, values=values)))
            A.values_f32(False)
            del B, Y
        g.set_storage("f64")
        amg_records(api, name, A, b, y, gen)
        product_records(api, name, "A", A, b, y)
        product_records(api, name, "G", g, b, y)
        product_records(api, name, "GT", t, b, y)
        # keeping the form: a value refresh of A (spmvHipValuesChanged: the unit detection and every built format) with it and without it
        with_form, _ = second_of_two(A.values_changed)
        form_bytes = int(A.values_f32_info().bytes)
        A.values_f32(False)
        without, _ = second_of_two(A.values_changed)
        rebuild, _ = second_of_two(lambda: (A.values_f32(False), A.values_f32()))
        out(record="setup", matrix=name, refreshWithFormMs=with_form, refreshWithoutMs=without, releaseAndBuildMs=rebuild,
            formBytesA=form_bytes, formBytesG=int(g.values_f32_info().bytes), formBytesGT=int(t.values_f32_info().bytes))
        for m in (t, g, A):
            m.free()
    out(record="done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "values_f32_timing.log"))
    ap.add_argument("--only", default="lap7,aniso,st19", help="the matrices, of " + ", ".join(MATRICES))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    only = [m for m in args.only.split(",") if m]
    if any(m not in MATRICES for m in only):
        ap.error("--only takes " + ", ".join(MATRICES))
    if args.child:
        return child(args.quick, only)
    rc = 0
    with open(args.out, "w") as f:                                       # (the records reach the log as they are made)
        for m in only:                                                   # one child per matrix, each under its own limit
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--only", m] + (["--quick"] if args.quick else [])
            try:
                p = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, text=True, timeout=LIMIT)
                one, error = p.returncode, p.stderr[-1200:]
            except subprocess.TimeoutExpired:
                one, error = 1, f"{m}: time limit of {LIMIT} s"
            if one:
                f.write(json.dumps({"error": error}) + "\n")
                f.flush()
                rc = one
                break                                                    # nothing more is started on the GPU after a failure
    print(open(args.out).read(), end="", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
