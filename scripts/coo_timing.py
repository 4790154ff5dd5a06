"""The COO assembly on the device.  Child processes, each under a time limit of its own; the device is
synchronised around every timed call.  One JSON line per record; the log opens with the hypotheses and closes with what the
numbers say of them.  Nothing here asserts a time.

  workloads   stencil   the 500 x 100 x 100 7-point stencil as 34.8 M triplets in CSR order (no duplicates)
              shuffled  the same triplets in a seeded random order
              hex       the 64 element-matrix entries of every cell of a 101^3-node Q1 grid (64 M triplets, about 8 per
                        entry of C in the interior), in element order
  per workload  build ms and refresh ms: the median of 5 after a warm-up (wall, synchronous calls; infoMs is the build's own
              clock), each over its algorithmic bytes -- a build reads 16 B per entry and writes 4 + 12 B per entry of C
              (+ 4 B per row), a refresh reads 8 + 4 B per kept entry and writes 8 B per entry of C -- and the share of the
              build that is the sort: the radix sort's kernels in a kernel trace of three builds, a run of its own, over the
              untraced build
  for comparison only   the host route on every tenth triplet: numpy lexsort + reduceat + spMatCpyCSR; and
              spmvHipUpdateValues of a ready CSR value array on the device

    python scripts/coo_timing.py [--quick] [--out profiles/coo_timing.log]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LIMIT, TRACE_LIMIT = 600, 240
WORKLOADS = ("stencil", "shuffled", "hex")
HYPOTHESES = {
    "build": "the build is bound by its sort: a 64-bit-key radix sort of (key, index) pairs moves 12 B per entry per pass, so "
             "the build should run at a fraction of the streaming rate and the sort should be most of it; nobody has measured it",
    "order": "a radix sort does the same passes whatever the order, but the value pass gathers val[perm[.]]: in CSR order that "
             "gather streams, shuffled it is random 8-byte reads, so shuffled should cost more in the value pass and the refresh",
    "refresh": "a refresh is the value pass alone plus what spmvHipValuesChanged does: far below a build; if it is not, that is "
               "a finding",
    "runs": "a run is added by one lane: with 8 duplicates per entry the value pass is 8 dependent gathers per lane, still "
            "entry-parallel across C"}


def sync():
    import torch
    torch.cuda.synchronize()


def median_of(fn, n=5):
    fn()
    sync()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def workload(name, quick):
    """(M, rows, cols, vals) as device tensors (int32, int32, float64)"""
    import numpy as np
    import torch
    g = torch.Generator(device="cuda").manual_seed(36)
    if name in ("stencil", "shuffled"):
        import spgemm_ref as sr
        A = sr.laplacian7(*((60, 40, 40) if quick else (500, 100, 100)))
        rows = torch.from_numpy(np.repeat(np.arange(A[0], dtype=np.int32), np.diff(A[2].astype(np.int64)))).cuda()
        cols = torch.from_numpy(A[3].astype(np.int32)).cuda()
        if name == "shuffled":
            p = torch.randperm(rows.numel(), device="cuda", generator=g)
            rows, cols = rows[p].contiguous(), cols[p].contiguous()
        M = A[0]
    else:
        n = 31 if quick else 101
        idx = torch.arange(n ** 3, device="cuda", dtype=torch.int32).reshape(n, n, n)
        first = idx[:-1, :-1, :-1].reshape(-1)
        corner = torch.tensor([x * n * n + y * n + z for x in (0, 1) for y in (0, 1) for z in (0, 1)], device="cuda", dtype=torch.int32)
        nodes = first[:, None] + corner[None, :]
        rows = nodes.repeat_interleave(8, dim=1).reshape(-1).contiguous()
        cols = nodes.repeat(1, 8).reshape(-1).contiguous()
        M = n ** 3
    vals = torch.rand(rows.numel(), device="cuda", dtype=torch.float64, generator=g) - 0.5
    return M, rows, cols, vals


def measure(api, name, quick):
    import numpy as np
    import torch
    M, rows, cols, vals = workload(name, quick)
    n = rows.numel()
    sync()

    def build():
        c = api.assemble_coo(M, M, rows, cols, vals)
        i = c.assemble_info()
        rec = dict(nnzC=int(i.nnzC), duplicates=int(i.duplicates), maxRun=int(i.maxRun), maxRowNnz=int(i.maxRowNnz), tempBytes=int(i.tempBytes), infoMs=i.ms)
        c.free()
        return rec
    rec = build()
    bms = median_of(build)
    rec["infoMs"] = statistics.median(build()["infoMs"] for _ in range(5))
    c = api.assemble_coo(M, M, rows, cols, vals)
    new = vals * 1.5
    rms = median_of(lambda: c.assemble_refresh(new))
    rinfo = statistics.median((c.assemble_refresh(new), c.assemble_info().ms)[1] for _ in range(5))
    ready = torch.rand(rec["nnzC"], device="cuda", dtype=torch.float64)
    ums = median_of(lambda: c.update_values(ready))
    c.free()
    build_bytes = 16 * n + 16 * rec["nnzC"] + 4 * (M + 1)
    refresh_bytes = 12 * n + 8 * rec["nnzC"]
    rec.update(workload=name, rows=M, entries=n, buildWallMs=bms[0], buildWallMinMax=bms[1:], refreshWallMs=rms[0], refreshWallMinMax=rms[1:],
               refreshInfoMs=rinfo, updateValuesWallMs=ums[0], buildBytes=build_bytes, buildGBs=build_bytes / rec["infoMs"] / 1e6,
               buildWallGBs=build_bytes / bms[0] / 1e6, refreshBytes=refresh_bytes, refreshGBs=refresh_bytes / rinfo / 1e6,
               refreshWallGBs=refresh_bytes / rms[0] / 1e6)
    # the host route on every tenth triplet: sort and sum with numpy, then upload
    r, cc, v = (t[::10].cpu().numpy() for t in (rows, cols, vals))
    t0 = time.perf_counter()
    o = np.lexsort((cc, r))
    r, cc, v = r[o], cc[o], v[o]
    head = np.r_[True, (r[1:] != r[:-1]) | (cc[1:] != cc[:-1])]
    AS = np.add.reduceat(v, np.flatnonzero(head))
    IRP = np.zeros(M + 1, np.uint64)
    IRP[1:] = np.cumsum(np.bincount(r[head], minlength=M))
    h = api.spMatCpyCSR(api.HostCSR(M, M, IRP, cc[head].astype(np.uint64), AS))
    sync()
    rec["hostRouteTenthMs"] = (time.perf_counter() - t0) * 1e3
    rec["hostRouteTenthEntries"] = int(r.size)
    h.free()
    print(json.dumps(rec), flush=True)
    return rec


def child(quick, only=None, builds=0):
    from spmv_openmp_cuda_amd import api
    api.spmvHipInit(0)
    if builds:                                                       # under the kernel trace: `builds` builds of one workload
        M, rows, cols, vals = workload(only, quick)
        for _ in range(builds):
            api.assemble_coo(M, M, rows, cols, vals).free()
        sync()
        return 0
    print(json.dumps({"hypotheses": HYPOTHESES, "note": "wall ms of synchronous calls, the median of 5 after a warm-up; infoMs is the call's "
                      "own clock; an idle machine is not guaranteed: other work may share the host"}), flush=True)
    for name in WORKLOADS:
        measure(api, name, quick)
    return 0


def run_limited(cmd, limit, echo=True):
    """the command under its time limit: (what it printed, its status); every line is passed on as it comes"""
    with tempfile.TemporaryFile("w+") as err:
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=err, text=True)
        timer = threading.Timer(limit, p.kill)
        timer.start()
        lines = []
        try:
            for line in p.stdout:
                lines.append(line)
                if echo:
                    print(line, end="", flush=True)
            rc = p.wait()
        finally:
            expired = not timer.is_alive()
            timer.cancel()
        err.seek(0)
        if expired:
            lines.append(json.dumps({"error": f"time limit of {limit} s"}) + "\n")
        elif rc:
            lines.append(json.dumps({"error": err.read()[-600:]}) + "\n")
        if echo and (expired or rc):
            print(lines[-1], end="", flush=True)
        return "".join(lines), 124 if expired else rc


def sort_share(name, quick, builds=3):
    """ns per build of the radix sort's kernels and of every kernel of coo.hip, from a kernel trace of `builds` builds"""
    if not shutil.which("rocprofv3"):
        return {"workload": name, "trace": "rocprofv3 not found: not measured"}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--only", name, "--builds", str(builds)] + (["--quick"] if quick else [])
        text, rc = run_limited(cmd, TRACE_LIMIT, echo=False)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if rc or not files:
            return {"workload": name, "trace": "failed", "rc": rc, "tail": text[-300:]}
        sort_ns = own_ns = 0
        for row in csv.DictReader(open(files[0])):
            kernel, ns = row["Name"], int(row["TotalDurationNs"])
            if "rocprim" in kernel and ("sort" in kernel or "onesweep" in kernel or "histogram" in kernel):
                sort_ns += ns
            elif "co_" in kernel and "spmvhip" in kernel:
                own_ns += ns
        return {"workload": name, "trace": "ok", "builds": builds, "sortMsPerBuild": sort_ns / builds / 1e6, "cooKernelsMsPerBuild": own_ns / builds / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coo_timing.log"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--only")
    ap.add_argument("--builds", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args.quick, args.only, args.builds)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--quick"] if args.quick else [])
    text, rc = run_limited(cmd, LIMIT)
    recs = {}
    for line in text.splitlines():
        try:
            r = json.loads(line)
        except ValueError:
            continue
        if "workload" in r:
            recs[r["workload"]] = r
    verdict = {}
    if rc == 0:                                                      # (after a failed step nothing more is started on the device)
        for name in WORKLOADS:
            s = sort_share(name, args.quick)
            print(json.dumps(s), flush=True)
            text += json.dumps(s) + "\n"
            if s.get("trace") != "ok":
                break
            if name in recs:
                verdict[name] = {"buildInfoMs": recs[name]["infoMs"], "refreshInfoMs": recs[name]["refreshInfoMs"],
                                 "sortShareOfBuild": s["sortMsPerBuild"] / recs[name]["infoMs"],
                                 "refreshOverBuild": recs[name]["refreshInfoMs"] / recs[name]["infoMs"],
                                 "refreshOverUpdateValues": recs[name]["refreshWallMs"] / recs[name]["updateValuesWallMs"],
                                 "hostRouteTenthOverBuild": recs[name]["hostRouteTenthMs"] / recs[name]["buildWallMs"]}
        print(json.dumps({"verdict": verdict}), flush=True)
        text += json.dumps({"verdict": verdict}) + "\n"
    with open(args.out, "w") as out:
        out.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
