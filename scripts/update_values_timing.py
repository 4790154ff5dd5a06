"""What a new set of values costs on a kept handle (spmvHipUpdateValues) against one SpMV and against what a caller without
it pays (free + upload + first call), on the synthetic c3 / c5 matrices built on the device.

Per matrix, after the first call of each reference name (its kernel selection):
  (a) one SpMV of the kernel each selection picked      device events (the launcher's own), median of 10
  (b) spmvHipUpdateValues from a device array           device events around the call: first call (value maps built) and
                                                        steady state, median of 5
  (c) free + upload + first call of both names          device events + host wall time; "upload" of a device-resident
                                                        matrix = spmvHipAdoptCSR (row blocks, unit detection) -- a host
                                                        upload adds its PCIe copy on top
The new values are the generator's with another value seed.  Check: after (b) and (c) hipSpMVRowsCSR of the updated
handle and of the fresh one are bit-identical (serial order: the same bits whatever kernel runs).

    python scripts/update_values_timing.py [--matrices c3,c5] [--out profiles/update_values_timing.log]
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

from spmv_openmp_cuda_amd import api, synth  # noqa: E402

NAMES = ("hipSpMVRowsCSR", "hipSpMVWarpPerRowCSR")


class Events:
    def __init__(self):
        self.a, self.b = C.c_void_p(), C.c_void_p()
        api._check(api.lib.spmvHipEventCreate(C.byref(self.a)), "event")
        api._check(api.lib.spmvHipEventCreate(C.byref(self.b)), "event")

    def time(self, fn):
        api.lib.spmvHipEventRecord(self.a)
        fn()
        api.lib.spmvHipEventRecord(self.b)
        ms = C.c_float()
        api._check(api.lib.spmvHipEventElapsedMs(self.a, self.b, C.byref(ms)), "elapsed")
        return ms.value


def adopt(w, rows, nnz, d_irp, irp_bytes, d_ja, d_as, irp_host):
    dm = api.DeviceMatrix()
    api._check(api.lib.spmvHipAdoptCSR(C.byref(dm.handle), rows, w.N, nnz, d_irp.ptr, irp_bytes, d_ja.ptr, d_as.ptr,
                                       irp_host.ctypes.data_as(C.c_void_p)), "spmvHipAdoptCSR")
    return dm


def measure(key, log):
    w = synth.WORKLOADS[key]
    lens = synth.row_lengths(w)
    irp = synth.prefix(lens)
    dm = synth.device_csr(w, irp, 0, w.N)
    nnz, irp_bytes = dm.nnz, dm.irp_bytes
    irp_host = irp.astype(np.uint32 if irp_bytes == 4 else np.uint64)
    d_irp, d_ja = dm.buffers["IRP"], dm.buffers["JA"]
    x = synth.make_x(w.N, w.cfg)
    dx = api.DeviceVector(w.N).up(x)
    dy = api.DeviceVector(w.N)
    ev = Events()
    rec = {"matrix": w.name, "nnz": nnz, "rows": w.N}
    for name in NAMES:                                   # first calls: the selections
        t0 = time.perf_counter()
        api.spmv(name, dm, dx, dy)
        rec[f"first_call_ms[{name}]"] = (time.perf_counter() - t0) * 1e3
    rec["pick[hipSpMVWarpPerRowCSR]"] = (api.lib.spmvHipAutoChoice(C.byref(dm.handle), None) or b"-").decode()
    rec["pick[hipSpMVRowsCSR]"] = (api.lib.spmvHipAutoChoiceRows(C.byref(dm.handle), None) or b"-").decode()
    # (a)
    for name in NAMES:
        t = []
        for _ in range(10):
            api.spmv(name, dm, dx, dy)
            t.append(api.lib.spmvHipLastKernelSeconds() * 1e3)
        rec[f"a_spmv_ms[{name}]"] = float(np.median(t))
    rec["bytes_formats"] = {"tiles": api.lib.spmvHipTilesBytes(C.byref(dm.handle)),
                            "stripes": api.lib.spmvHipStripesBytes(C.byref(dm.handle)),
                            "sell": api.lib.spmvHipSellBytes(C.byref(dm.handle))}
    # new values on the device: the generator with another value seed (its columns land in a scratch array)
    d_ja2 = api.DeviceBuffer(4 * nnz)
    d_as2 = api.DeviceBuffer(8 * nnz)
    api._check(api.lib.spmvHipSynthFillCSR(w.N, w.N, 0, d_irp.ptr, irp_bytes, d_ja2.ptr, d_as2.ptr, synth.SEED_STRUCT + w.cfg,
                                           synth.SEED_VAL + w.cfg + 101, w.band), "spmvHipSynthFillCSR")
    d_ja2.free()
    # (b)
    upd = lambda: api._check(api.lib.spmvHipUpdateValues(C.byref(dm.handle), d_as2.ptr, 1), "spmvHipUpdateValues")  # noqa: E731
    rec["b_update_first_ms"] = ev.time(upd)
    info = dm.update_info()
    rec["b_update_first_info"] = {f: getattr(info, f) for f, _ in api.spmvUpdateInfo._fields_}
    rec["b_update_steady_ms"] = float(np.median([ev.time(upd) for _ in range(5)]))
    info = dm.update_info()
    rec["b_update_steady_info"] = {f: getattr(info, f) for f, _ in api.spmvUpdateInfo._fields_}
    rec["bytes_formats_with_maps"] = {"tiles": api.lib.spmvHipTilesBytes(C.byref(dm.handle)),
                                      "stripes": api.lib.spmvHipStripesBytes(C.byref(dm.handle))}
    rec["picks_kept"] = ((api.lib.spmvHipAutoChoice(C.byref(dm.handle), None) or b"-").decode() == rec["pick[hipSpMVWarpPerRowCSR]"] and
                         (api.lib.spmvHipAutoChoiceRows(C.byref(dm.handle), None) or b"-").decode() == rec["pick[hipSpMVRowsCSR]"])
    api.spmv("hipSpMVRowsCSR", dm, dx, dy)
    y_upd = dy.down()
    # (c): free + upload (adopt the device arrays holding the new values) + first call of both names
    fresh = {}

    def redo():
        dm.handle.dev and api.lib.hipFreeSpmat(C.byref(dm.handle))
        fresh["dm"] = adopt(w, w.N, nnz, d_irp, irp_bytes, d_ja, d_as2, irp_host)
        for name in NAMES:
            api.spmv(name, fresh["dm"], dx, dy)
    t0 = time.perf_counter()
    rec["c_free_upload_first_ms"] = ev.time(redo)
    rec["c_free_upload_first_wall_ms"] = (time.perf_counter() - t0) * 1e3
    api.spmv("hipSpMVRowsCSR", fresh["dm"], dx, dy)
    rec["check_bitwise_equal_to_fresh_handle"] = bool(np.array_equal(dy.down(), y_upd)) and not np.isnan(y_upd).any()
    for name in NAMES:
        rec[f"ratio_b_steady_over_a[{name}]"] = rec["b_update_steady_ms"] / rec[f"a_spmv_ms[{name}]"]
    rec["ratio_c_over_b_steady"] = rec["c_free_upload_first_ms"] / rec["b_update_steady_ms"]
    line = json.dumps(rec)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()
    fresh["dm"].free()
    dm.free()
    d_as2.free()
    dx.free()
    dy.free()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--matrices", default="c3,c5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_values_timing.log"))
    args = ap.parse_args()
    api.spmvHipInit(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as log:
        log.write(f"# update_values_timing {time.strftime('%Y-%m-%d %H:%M:%S')}  library "
                  f"{os.path.getmtime(api.LIB_PATH):.0f}\n")
        for key in args.matrices.split(","):
            measure(key.strip(), log)
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
