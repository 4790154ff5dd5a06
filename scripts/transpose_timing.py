"""A^T of a device CSR handle (spmvHipCsrTranspose) and its refresh (spmvHipTransposeRefresh) on the synthetic c2 / c3 /
c3b matrices built on the device and the 3-D stencil stand-in of DESIGN.md section 9.

Per matrix:
  build_ms         spmvHipCsrTranspose, host wall time of the call (it returns with dAT complete), median of 3
  refresh_first_ms spmvHipTransposeRefresh right after dAT's selections (its formats held), host wall time
  refresh_ms       the same, steady state, median of 5 (new device values for A through spmvHipUpdateValues first)
  ax_rows_ms / ax_warp_ms   A x after the first call of each reference name (its selection): hipSpMVRowsCSR (serial
                   order) / hipSpMVWarpPerRowCSR (reduction order), device events, median of 10 after a warm-up
  atx_rows_ms / atx_warp_ms the same on dAT
  roofline_*       B / t / 8 TB/s with B = nnz*12 + N*12 + M*8 for A^T x (M, N of A) and nnz*12 + M*12 + N*8 for A x
  check_bitwise    hipSpMVRowsCSR on dAT == sgemvSerial on the test side's stable transpose, on sampled rows of A^T
and, on c2 only, the host alternative: download IRP / JA / AS, numpy stable transpose, upload with spMatCpyCSR.
Kernel split of the build: `rocprofv3 --kernel-trace --stats -- python scripts/transpose_timing.py`.

    python scripts/transpose_timing.py [--matrices c2,c3,c3b,stencil] [--out profiles/transpose_timing.log]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from spmv_openmp_cuda_amd import api  # noqa: E402
from spmm_timing import Events, stencil, synthetic  # noqa: E402

PEAK = 8e12


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def spmv_ms(ev, dm, launcher, x, y):
    fn, cfg, H = api.SPMV_LAUNCHERS[launcher], api.CONFIG(), C.byref(dm.handle)
    api._check(fn(H, x.data_ptr(), cfg, y.data_ptr()), launcher)          # first call: the selection
    api.lib.spmvHipSetSync(0)
    try:
        return ev.median(lambda: api._check(fn(H, x.data_ptr(), cfg, y.data_ptr()), launcher))
    finally:
        api.lib.spmvHipSetSync(1)


def check(oracle, irp, ja, as_, N, xt, yt, rows):
    """yt[rows] == sgemvSerial(stable transpose, xt)[rows], bit for bit"""
    from transpose_ref import stable_transpose
    IRPt, JAt, ASt, _ = stable_transpose(N, irp, ja, as_)
    ref = oracle.csr_serial(IRPt, JAt, ASt, xt)
    return bool(np.array_equal(ref[rows].view(np.uint64), yt[rows].view(np.uint64)))


def host_alternative(dm, M, N, nnz):
    """download, numpy stable transpose, upload: the caller's option without spmvHipCsrTranspose"""
    from transpose_ref import stable_transpose
    h = dm.handle
    t0 = time.perf_counter()
    irp = np.empty(M + 1, np.uint32 if getattr(dm, "irp_bytes", 4) == 4 else np.uint64)
    ja, as_ = np.empty(nnz, np.uint32), np.empty(nnz, np.float64)
    for arr, p in ((irp, h.IRP), (ja, h.JA), (as_, h.AS)):
        api._check(api.lib.spmvHipMemcpyDown(arr.ctypes.data_as(C.c_void_p), C.cast(p, C.c_void_p), arr.nbytes), "down")
    t1 = time.perf_counter()
    IRPt, JAt, ASt, _ = stable_transpose(N, irp, ja, as_)
    t2 = time.perf_counter()
    t = api.spMatCpyCSR(api.HostCSR(N, M, IRPt, JAt, ASt))
    t3 = time.perf_counter()
    t.free()
    return {"host_download_ms": (t1 - t0) * 1e3, "host_numpy_ms": (t2 - t1) * 1e3, "host_upload_ms": (t3 - t2) * 1e3,
            "host_total_ms": (t3 - t0) * 1e3}


def measure(name, dm, irp, ja, as_, oracle, torch, log, host):
    M, N, nnz = int(dm.handle.M), int(dm.handle.N), int(dm.handle.NZ)
    unit = api.lib.spmvHipUnitValue(C.byref(dm.handle), None) == 1
    ev = Events()
    gen = torch.Generator(device="cuda").manual_seed(0x7A05)
    x = torch.rand(N, generator=gen, dtype=torch.float64, device="cuda") * 2 - 1
    xt = torch.rand(M, generator=gen, dtype=torch.float64, device="cuda") * 2 - 1
    y, yt = torch.empty(M, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
    rec = {"matrix": name, "M": M, "N": N, "nnz": nnz, "unit": unit}
    builds = []
    for _ in range(3):
        ms, t = wall(dm.transpose)
        builds.append(ms)
        t.free()
    rec["build_ms"] = float(np.median(builds))
    rec["build_ms_all"] = builds
    t = dm.transpose()
    rec["ax_rows_ms"] = spmv_ms(ev, dm, "hipSpMVRowsCSR", x, y)
    rec["ax_warp_ms"] = spmv_ms(ev, dm, "hipSpMVWarpPerRowCSR", x, y)
    rec["atx_rows_ms"] = spmv_ms(ev, t, "hipSpMVRowsCSR", xt, yt)
    rec["atx_warp_ms"] = spmv_ms(ev, t, "hipSpMVWarpPerRowCSR", xt, yt)
    rec["picks_a"] = [(api.lib.spmvHipAutoChoiceRows(C.byref(dm.handle), None) or b"-").decode(),
                      (api.lib.spmvHipAutoChoice(C.byref(dm.handle), None) or b"-").decode()]
    rec["picks_at"] = [(api.lib.spmvHipAutoChoiceRows(C.byref(t.handle), None) or b"-").decode(),
                       (api.lib.spmvHipAutoChoice(C.byref(t.handle), None) or b"-").decode()]
    rec["at_bytes"] = {"tiles": int(api.lib.spmvHipTilesBytes(C.byref(t.handle))),
                       "stripes": int(api.lib.spmvHipStripesBytes(C.byref(t.handle)))}
    ms, _ = wall(lambda: t.refresh_from(dm))
    rec["refresh_first_ms"] = ms
    refreshes = []
    new = torch.rand(nnz, generator=gen, dtype=torch.float64, device="cuda") if not unit else None
    for k in range(5):
        if new is not None:
            dm.update_values(new if k % 2 else new * 0.5)
            torch.cuda.synchronize()
        ms, _ = wall(lambda: t.refresh_from(dm))
        refreshes.append(ms)
    rec["refresh_ms"] = float(np.median(refreshes))
    rec["refresh_ms_all"] = refreshes
    info = t.update_info()
    rec["refresh_in_place"] = info.inPlace
    b_at, b_a = nnz * 12 + N * 12 + M * 8, nnz * 12 + M * 12 + N * 8
    rec["roofline_atx_rows"] = b_at / (rec["atx_rows_ms"] * 1e-3) / PEAK
    rec["roofline_atx_warp"] = b_at / (rec["atx_warp_ms"] * 1e-3) / PEAK
    rec["roofline_ax_rows"] = b_a / (rec["ax_rows_ms"] * 1e-3) / PEAK
    rec["atx_over_ax_rows"] = rec["atx_rows_ms"] / rec["ax_rows_ms"]
    # bits of the serial-order product on dAT (the values A holds now)
    as_ = np.empty(nnz, np.float64)
    api._check(api.lib.spmvHipMemcpyDown(as_.ctypes.data_as(C.c_void_p), C.cast(dm.handle.AS, C.c_void_p), as_.nbytes), "down")
    api._check(api.SPMV_LAUNCHERS["hipSpMVRowsCSR"](C.byref(t.handle), xt.data_ptr(), api.CONFIG(), yt.data_ptr()), "rows")
    torch.cuda.synchronize()
    rng = np.random.default_rng(0x7A05)
    lens_t = np.bincount(ja, minlength=N)
    rows = np.unique(np.concatenate([rng.integers(0, N, size=2000), np.argsort(lens_t, kind="stable")[-8:]]))
    # (the host side of the check sorts nnz keys in numpy: done up to c2's size, the tests cover the rest)
    rec["check_bitwise"] = check(oracle, irp, ja, as_, N, xt.cpu().numpy(), yt.cpu().numpy(), rows) if nnz <= 64 << 20 else None
    t.free()
    if host:
        rec.update(host_alternative(dm, M, N, nnz))
    line = json.dumps(rec)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--matrices", default="c2,c3,c3b,stencil")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transpose_timing.log"), help="JSON records are appended here")
    args = ap.parse_args()
    import torch
    from conftest import Oracle
    oracle = Oracle()
    api.spmvHipInit(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as log:
        log.write(f"# transpose_timing {time.strftime('%Y-%m-%d %H:%M:%S')}\n")
        for key in args.matrices.split(","):
            key = key.strip()
            name, dm, irp, ja, as_ = stencil() if key == "stencil" else synthetic(key)
            measure(name, dm, irp, ja, as_, oracle, torch, log, host=key == "c2")
            dm.free()
            torch.cuda.empty_cache()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
