"""The basis rotation (spmvHipBlockCombine) and thick-restart Lanczos (hipSpLanczosCSR), DESIGN.md section 39: the rotation
at n = 5 M against the library's own streaming figure for a fused vector pass -- the CGS2 update kernel -- and one
end-to-end solve of the 500 x 100 x 100 seven-point Laplacian at both ends of the spectrum with the shares of its time.

The parent starts three children, one after the other, each with a time limit; after a child that fails nothing more is
started on the device.  Records (one JSON line each):
  rotation     child `plain`: spmvHipBlockCombine at (m, k) = (20, 12) and (64, 32), out of place and (20, 12) in place:
               ms (device events, median of 10 after a warm-up), bytes = 8 n (m + k), GB/s
  eigsh        child `plain`: nev = 4, ncv = 20, tol = 1e-8, maxIter = 600, LARGEST and SMALLEST: status, matvecs, cycles,
               launches, ms and jacobiMs of the second of two calls (host wall time inside the library)
  update       child `stream` under rocprofv3 --kernel-trace: one Lanczos cycle of 64 steps on a 5 M-row diagonal matrix;
               the first update kernel of step j streams 8 n (j + 3) bytes (w read and written, j + 1 columns read): ms
               and GB/s of the dispatches whose byte counts are nearest the two rotations', and of all 64 together
  shares       child `e2e` under rocprofv3 --kernel-trace: the LARGEST solve once more; kernel time by group (SpMV,
               reorthogonalisation = projections, updates, scalar steps and scalings, rotation) from the trace, over
               the untraced ms of `eigsh` (the dispatches from the solve's dot(v0, v0) on); Jacobi from jacobiMs; the rest is read-backs, uploads, enqueue and idle
  verdict      rotation GB/s over update GB/s at the nearest byte count

    python scripts/lanczos_timing.py [--out profiles/lanczos_timing.log]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

N = 5_000_000
GRID = (500, 100, 100)
LIMIT = 420
SHAPES = ((20, 12, False), (20, 12, True), (64, 32, False))


def say(rec):
    print(json.dumps(rec), flush=True)


def lanczos(api, A, dv, dx, M, nev, ncv, which, maxiter):
    opts, info = api.spmvLanczosOpts(nev, ncv, which, 1e-8, maxiter, 0), api.spmvLanczosInfo()
    theta, res = np.zeros(nev), np.zeros(nev)
    api._check(api.lib.hipSpLanczosCSR(C.byref(A.handle), dv.ptr, C.byref(opts), dx.ptr, M, theta.ctypes.data, res.ctypes.data,
                                       C.byref(info)), "hipSpLanczosCSR")
    return info, theta, res


def laplacian(api):
    from test_trsv_abi import laplacian7
    IRP, JA, AS = laplacian7(*GRID)
    M = int(np.prod(GRID))
    return api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS)), M


def child_plain(api):
    from spmm_timing import Events
    ev = Events()
    rng = np.random.default_rng(30)
    dV, dY, dS = api.DeviceVector(64 * N), api.DeviceVector(32 * N), api.DeviceVector(64 * 64)
    for c in range(64):                                              # (column by column: no 2.5 GB host array)
        col = rng.random(N)                                          # (named: it must outlive the call that reads it)
        api._check(api.lib.spmvHipVecUp(C.c_void_p(dV.ptr.value + 8 * N * c), col.ctypes.data, N), "up")
    dS.up(rng.standard_normal(64 * 64))
    for m, k, inplace in SHAPES:
        out = dV if inplace else dY
        ms = ev.median(lambda: api.lib.spmvHipBlockCombine(N, m, k, dV.ptr, N, dS.ptr, 64, out.ptr, N))
        nbytes = 8.0 * N * (m + k)
        say({"record": "rotation", "n": N, "m": m, "k": k, "in_place": inplace, "ms": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6})
    for b in (dV, dY, dS):
        b.free()
    A, M = laplacian(api)
    dv, dx = api.DeviceVector(M).up(np.random.default_rng(0).standard_normal(M)), api.DeviceVector(4 * M)
    for which, name in ((0, "LARGEST"), (1, "SMALLEST")):
        lanczos(api, A, dv, dx, M, 4, 20, which, 600)
        info, theta, res = lanczos(api, A, dv, dx, M, 4, 20, which, 600)
        say({"record": "eigsh", "matrix": "laplacian7-500x100x100", "which": name, "nev": 4, "ncv": 20, "tol": 1e-8, "status": info.status,
             "found": info.found, "matvecs": info.iterations, "cycles": info.cycles, "launches": info.launches, "ms": info.ms,
             "jacobiMs": info.jacobiMs, "theta": theta.tolist(), "res_over_scale": (res / info.scale).tolist()})
    A.free()


def child_stream(api):
    rng = np.random.default_rng(31)
    i = np.arange(N, dtype=np.uint64)
    A = api.spMatCpyCSR(api.HostCSR(N, N, np.arange(N + 1, dtype=np.uint64), i, rng.random(N) + 1.0))
    dv, dx = api.DeviceVector(N).up(rng.standard_normal(N)), api.DeviceVector(N)
    info, _, _ = lanczos(api, A, dv, dx, N, 1, 64, 0, 64)
    say({"record": "stream_child", "matvecs": info.iterations, "cycles": info.cycles})
    A.free()


def child_e2e(api):
    A, M = laplacian(api)
    dv, dx = api.DeviceVector(M).up(np.random.default_rng(0).standard_normal(M)), api.DeviceVector(4 * M)
    lanczos(api, A, dv, dx, M, 4, 20, 0, 1)                          # (the handle's first SpMV chooses its kernel)
    info, _, _ = lanczos(api, A, dv, dx, M, 4, 20, 0, 600)
    say({"record": "e2e_child", "matvecs": info.iterations, "cycles": info.cycles, "traced_ms": info.ms})
    A.free()


def run(cmd):
    """(the child's JSON records, its exit code); the child is ended at LIMIT seconds"""
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        text, rc = p.stdout, p.returncode
        if rc:
            print(p.stderr[-2000:], file=sys.stderr)
    except subprocess.TimeoutExpired as e:
        text, rc = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), 124
    recs = []
    for line in text.splitlines():
        try:
            recs.append(json.loads(line))
        except ValueError:
            pass
    return recs, rc


def traced(which):
    """the dispatches of a traced child, in start order: [(kernel name, ms)]"""
    d = tempfile.mkdtemp(prefix="lanczos_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", which]
        recs, rc = run(cmd)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if rc or not files:
            return None, recs, rc
        rows = []
        for row in csv.DictReader(open(files[0])):
            rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"], (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6))
        rows.sort()
        return [(name, ms) for _, name, ms in rows], recs, rc
    finally:
        shutil.rmtree(d, ignore_errors=True)


def group(name):
    if "block_combine_kernel" in name:
        return "rotation"
    if any(s in name for s in ("multidot_", "gmres_update_kernel", "lanczos_finish_kernel", "krylov_vec_kernel")):
        return "reorthogonalisation"
    return "spmv"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lanczos_timing.log"))
    ap.add_argument("--child", choices=("plain", "stream", "e2e"))
    a = ap.parse_args()
    if a.child:
        from spmv_openmp_cuda_amd import api
        api.spmvHipInit(0)
        {"plain": child_plain, "stream": child_stream, "e2e": child_e2e}[a.child](api)
        api.spmvHipFinalize()
        return 0
    out = open(a.out, "w")
    out.write("# scripts/lanczos_timing.py on the MI355X; one JSON record per line (fields: the script's docstring)\n")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    plain, rc = run([sys.executable, os.path.abspath(__file__), "--child", "plain"])
    for r in plain:
        emit(r)
    if rc:
        emit({"record": "verdict", "error": f"the plain child ended with {rc}: nothing more was run"})
        return 1
    if not shutil.which("rocprofv3"):
        emit({"record": "verdict", "error": "rocprofv3 not found: update and shares not measured"})
        return 1
    disp, _, rc = traced("stream")
    if disp is None:
        emit({"record": "verdict", "error": f"the stream child ended with {rc}: nothing more was run"})
        return 1
    upd = [ms for name, ms in disp if "gmres_update_kernel<0>" in name or "gmres_update_kernelILi0" in name]
    stream = {}
    if len(upd) == 64:
        nbytes = [8.0 * N * (j + 3) for j in range(64)]
        for label, j in (("as (20, 12)", 29), ("nearest (64, 32)", 63)):
            stream[label] = nbytes[j] / upd[j] / 1e6
            emit({"record": "update", "step": j, "columns": j + 1, "ms": upd[j], "bytes": nbytes[j], "GBps": stream[label]})
        emit({"record": "update", "step": "all 64", "ms": sum(upd), "bytes": sum(nbytes), "GBps": sum(nbytes) / sum(upd) / 1e6})
    else:
        emit({"record": "update", "error": f"{len(upd)} dispatches of the first update kernel, 64 expected", "kernels": sorted({n for n, _ in disp})[:40]})
    disp, recs, rc = traced("e2e")
    if disp is None:
        emit({"record": "verdict", "error": f"the e2e child ended with {rc}"})
        return 1
    base = next(r for r in plain if r["record"] == "eigsh" and r["which"] == "LARGEST")
    starts = [i for i, (name, _) in enumerate(disp) if "DotOp" in name]     # dot(v0, v0): the first kernel of a solve
    sums = {}
    for name, ms in disp[starts[-1] if starts else 0:]:
        sums[group(name)] = sums.get(group(name), 0.0) + ms
    sums["jacobi"] = base["jacobiMs"]
    shares = {g: v / base["ms"] for g, v in sums.items()}
    shares["host_rest"] = 1.0 - sum(shares.values())
    emit({"record": "shares", "which": "LARGEST", "untraced_ms": base["ms"], "group_ms": sums, "share_of_untraced_ms": shares,
          "traced": [r for r in recs if r.get("record") == "e2e_child"]})
    rot = {(r["m"], r["k"], r["in_place"]): r["GBps"] for r in plain if r["record"] == "rotation"}
    if stream:
        emit({"record": "verdict", "rotation_over_update": {"(20, 12)": rot[(20, 12, False)] / stream["as (20, 12)"],
                                                            "(20, 12) in place": rot[(20, 12, True)] / stream["as (20, 12)"],
                                                            "(64, 32)": rot[(64, 32, False)] / stream["nearest (64, 32)"]}})
    out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
