"""Y = A X for a block of k vectors (hipSpMMRowsCSR) against k single-vector calls, on the synthetic c2 / c3 / c3b matrices
built on the device and the 3-D stencil stand-in of DESIGN.md section 9.

Per matrix, after the first call of each reference name (its kernel selection), for each k with row-major X and Y:
  spmm_ms          hipSpMMRowsCSR, device events around the call (enqueue-only mode), median of 10 after a warm-up
  rows_k_ms        k calls of hipSpMVRowsCSR (the serial-order selection: the same bits), same timing
  warp_k_ms        k calls of hipSpMVWarpPerRowCSR (the reduction-order selection), same timing
  rows_v1_ms       one call of hipSpMVRowsCSR variant 1 (the LDS-stream kernel), the k = 1 yardstick
  ms_per_vector    spmm_ms / k
  roofline         (nnz*12 + M*(4 + 8k) + N*8k) / spmm_ms / 8 TB/s  (nnz*4 instead of nnz*12 for a unit handle)
and column-major X and Y at k = 8 on c3.  Every spmm row is checked against the oracle's bits (sgemvSerial, stored order)
on a seeded sample of rows, every column.

    python scripts/spmm_timing.py [--matrices c2,c3,c3b,stencil] [--ks 1,2,4,8,16,32] [--out profiles/spmm_timing.log]
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

from spmv_openmp_cuda_amd import api, synth  # noqa: E402

PEAK = 8e12
ROW, COL = api.SPMV_DENSE_ROW_MAJOR, api.SPMV_DENSE_COL_MAJOR


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

    def median(self, fn, reps=10):
        self.time(fn)                                    # warm-up
        return float(np.median([self.time(fn) for _ in range(reps)]))


def synthetic(key):
    """(name, handle, IRP, JA, AS on the host) of a synth workload generated on the device"""
    w = synth.WORKLOADS[key]
    irp = synth.prefix(synth.row_lengths(w))
    dm = synth.device_csr(w, irp, 0, w.N)
    return w.name, dm, irp.astype(np.uint64), dm.buffers["JA"].down(np.uint32), dm.buffers["AS"].down(np.float64)


def stencil():
    """the 3-D stencil stand-in (500 x 100 x 100, 18 neighbours) as bench.py makes it: generated file -> MMtoCSR -> upload"""
    path = os.path.join("/dev/shm" if os.access("/dev/shm", os.W_OK) else ROOT, f"spmm_timing_{os.getpid()}.mtx")
    Mv, NZv, mxv = C.c_ulong(), C.c_ulong(), C.c_ulong()
    try:
        api._check(api.hostlib.spmvSynthWriteMtx(path.encode(), 0, 500, 100, 100, 0x57A7, C.byref(Mv), C.byref(NZv),
                                                 C.byref(mxv)), "spmvSynthWriteMtx")
        csr = api.hostlib.MMtoCSR(path.encode())
    finally:
        if os.path.exists(path):
            os.remove(path)
    if not csr:
        raise api.SpmvHipError("MMtoCSR refused the generated stencil")
    m = csr.contents
    M, nnz = int(m.M), int(m.NZ)
    irp = np.ctypeslib.as_array(m.IRP, shape=(M + 1,)).astype(np.uint64)
    ja = np.ctypeslib.as_array(m.JA, shape=(nnz,)).astype(np.uint32)
    as_ = np.ctypeslib.as_array(m.AS, shape=(nnz,)).copy()
    dm = api.DeviceMatrix()
    api._check(api.lib.spMatCpyCSR(csr, C.byref(dm.handle)), "spMatCpyCSR")
    api.hostlib.freeSpmat(csr)
    return "stencil3d-500x100x100", dm, irp, ja, as_


def check(oracle, irp, ja, as_, Xh, Yh, rows):
    """Y[rows, c] == sgemvSerial(X[:, c])[rows] bit for bit, every column (the sampled rows as a CSR of their own)"""
    lens = (irp[rows + 1] - irp[rows]).astype(np.int64)
    sub_irp = np.zeros(rows.size + 1, dtype=np.uint64)
    sub_irp[1:] = np.cumsum(lens)
    idx = np.concatenate([np.arange(int(irp[r]), int(irp[r + 1])) for r in rows]) if lens.sum() else np.zeros(0, np.int64)
    sub_ja, sub_as = ja[idx].astype(np.uint64), as_[idx]
    for c in range(Xh.shape[1]):
        ref = oracle.csr_serial(sub_irp, sub_ja, sub_as, np.ascontiguousarray(Xh[:, c]))
        if not np.array_equal(ref.view(np.uint64), Yh[rows, c].view(np.uint64)):
            return False
    return True


def measure(name, dm, irp, ja, as_, ks, oracle, torch, log, colmajor_k=0):
    M, N, nnz = int(dm.handle.M), int(dm.handle.N), int(dm.handle.NZ)
    unit = api.lib.spmvHipUnitValue(C.byref(dm.handle), None) == 1
    kmax = max(ks + [colmajor_k])
    gen = torch.Generator(device="cuda").manual_seed(0x5B33)
    X = torch.rand((N, kmax), generator=gen, dtype=torch.float64, device="cuda") * 2 - 1
    Xt = X.t().contiguous()                              # column c of X as a contiguous vector Xt[c]
    Y = torch.empty((M, kmax), dtype=torch.float64, device="cuda")
    ys = torch.empty((kmax, M), dtype=torch.float64, device="cuda")
    Xh = X.cpu().numpy()
    rng = np.random.default_rng(0x5B33)
    lens = np.diff(irp.astype(np.int64))
    rows = np.unique(np.concatenate([rng.integers(0, M, size=2000), np.argsort(lens)[-8:]]))
    ev = Events()
    cfg = api.CONFIG()
    H = C.byref(dm.handle)
    for launcher in ("hipSpMVRowsCSR", "hipSpMVWarpPerRowCSR"):                    # first calls: the selections
        api._check(api.SPMV_LAUNCHERS[launcher](H, Xt[0].data_ptr(), cfg, ys[0].data_ptr()), launcher)
    picks = {"hipSpMVRowsCSR": (api.lib.spmvHipAutoChoiceRows(H, None) or b"-").decode(),
             "hipSpMVWarpPerRowCSR": (api.lib.spmvHipAutoChoice(H, None) or b"-").decode()}
    api.lib.spmvHipSetSync(0)
    try:
        api.set_variant("hipSpMVRowsCSR", 1)
        v1 = ev.median(lambda: api.SPMV_LAUNCHERS["hipSpMVRowsCSR"](H, Xt[0].data_ptr(), cfg, ys[0].data_ptr()))
        api.set_variant("hipSpMVRowsCSR", 2)
        cases = [(k, ROW, ROW) for k in ks] + ([(colmajor_k, COL, COL)] if colmajor_k else [])
        for k, xl, yl in cases:
            if xl == ROW:
                Xk, Yk, ldx, ldy = X[:, :k].contiguous(), Y[:, :k].contiguous(), k, k
            else:
                Xk, Yk, ldx, ldy = Xt[:k].contiguous(), torch.empty((k, M), dtype=torch.float64, device="cuda"), N, M

            def spmm():
                api._check(api.lib.hipSpMMRowsCSR(H, k, Xk.data_ptr(), ldx, xl, Yk.data_ptr(), ldy, yl), "hipSpMMRowsCSR")

            def k_calls(launcher):
                fn = api.SPMV_LAUNCHERS[launcher]
                return lambda: [api._check(fn(H, Xt[c].data_ptr(), cfg, ys[c].data_ptr()), launcher) for c in range(k)]
            Yk.fill_(float("nan"))
            t = ev.median(spmm)
            rec = {"matrix": name, "M": M, "N": N, "nnz": nnz, "unit": unit, "k": k,
                   "layout": "row-major" if xl == ROW else "column-major", "spmm_ms": t, "ms_per_vector": t / k}
            rec["rows_k_ms"] = ev.median(k_calls("hipSpMVRowsCSR"))
            rec["warp_k_ms"] = ev.median(k_calls("hipSpMVWarpPerRowCSR"))
            rec["rows_v1_ms"] = v1
            rec["picks"] = picks
            rec["speedup_vs_rows_k"] = rec["rows_k_ms"] / t
            b = nnz * (4 if unit else 12) + M * (4 + 8 * k) + N * 8 * k
            rec["algorithmic_bytes"] = b
            rec["roofline"] = b / (t * 1e-3) / PEAK
            torch.cuda.synchronize()
            Yh = (Yk if xl == ROW else Yk.t()).cpu().numpy()
            rec["check_rows"] = int(rows.size)
            rec["check_bitwise"] = bool(check(oracle, irp, ja, as_, Xh[:, :k], Yh, rows))
            line = json.dumps(rec)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
    finally:
        api.lib.spmvHipSetSync(1)
        api.set_variant("hipSpMVRowsCSR", 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--matrices", default="c2,c3,c3b,stencil")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--colmajor-k", type=int, default=8, help="column-major X and Y at this k on c3 (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_timing.log"), help="JSON records are appended here")
    args = ap.parse_args()
    import torch
    from conftest import Oracle
    oracle = Oracle()
    api.spmvHipInit(0)
    ks = [int(k) for k in args.ks.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as log:
        log.write(f"# spmm_timing {time.strftime('%Y-%m-%d %H:%M:%S')}  library {os.path.getmtime(api.LIB_PATH):.0f}\n")
        for key in args.matrices.split(","):
            key = key.strip()
            name, dm, irp, ja, as_ = stencil() if key == "stencil" else synthetic(key)
            measure(name, dm, irp, ja, as_, ks, oracle, torch, log, args.colmajor_k if key == "c3" else 0)
            dm.free()
            torch.cuda.empty_cache()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
