"""Block triangular solves (hipSpTRSMCSR): one solve of k right-hand sides against k single solves
(hipSpTRSVCSR) on the same handle, measured in the same run.

Per matrix and k:
  trsm_ms       hipSpTRSMCSR, device events around the enqueued solve, median of 10 after a warm-up
  trsv_ms       hipSpTRSVCSR on the same handle, the same way (once per matrix)
  ratio         trsm_ms / (k * trsv_ms): below 1, the block solve beats k single solves
  us_per_launch trsm_ms / spmvTriInfo.launches
  check_bitwise columns 0 and k - 1 of X == hipSpTRSVCSR on those columns of B, bit for bit
k is row-major (ld = k) for both B and X; --colmajor-k names one width that is also run column-major (ld = M).
Kernel split: `rocprofv3 --kernel-trace --stats -- python scripts/trsm_timing.py ...`.

    python scripts/trsm_timing.py [--matrices lap7,stencil,c2] [--ks 1,2,4,8,16,32] [--colmajor-k 16] [--out profiles/trsm_timing.log]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from spmv_openmp_cuda_amd import api  # noqa: E402
from spmm_timing import Events, stencil, synthetic  # noqa: E402
from trsv_timing import lap7  # noqa: E402

ROW, COL = api.SPMV_DENSE_ROW_MAJOR, api.SPMV_DENSE_COL_MAJOR


def same_bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def measure(name, dm, lower, unit, ks, colmajor_k, ev, out):
    M = int(dm.handle.M)
    uplo, diag = (0 if lower else 1), int(unit)
    h = C.byref(dm.handle)
    rng = np.random.default_rng(11)
    dm.triangular_analyse(lower)
    info = dm.triangular_info(lower)
    db, dx = api.DeviceVector(M), api.DeviceVector(M)
    db.up(rng.uniform(-1, 1, M))
    api.lib.spmvHipSetSync(0)
    trsv = ev.median(lambda: api._check(api.lib.hipSpTRSVCSR(h, uplo, diag, db.ptr, dx.ptr), "trsv"))
    api.lib.spmvHipSetSync(1)
    api._check(api.lib.spmvHipDeviceSynchronize(), "sync")
    cases = [(k, ROW) for k in ks] + ([(colmajor_k, COL)] if colmajor_k else [])
    for k, layout in cases:
        Bh = rng.uniform(-1, 1, (M, k))
        flat = np.ascontiguousarray(Bh if layout == ROW else Bh.T)
        ld = k if layout == ROW else M
        bB, bX = api.DeviceBuffer(flat.nbytes).up(flat), api.DeviceBuffer(flat.nbytes)
        api.lib.spmvHipSetSync(0)
        trsm = ev.median(lambda: api._check(api.lib.hipSpTRSMCSR(h, uplo, diag, k, bB.ptr, ld, layout, bX.ptr, ld, layout), "trsm"))
        api.lib.spmvHipSetSync(1)
        api._check(api.lib.spmvHipDeviceSynchronize(), "sync")
        Xh = bX.down(np.float64).reshape((M, k) if layout == ROW else (k, M))
        Xh = Xh if layout == ROW else Xh.T
        ok = True
        for c in sorted({0, k - 1}):
            db.up(np.ascontiguousarray(Bh[:, c]))
            api._check(api.lib.hipSpTRSVCSR(h, uplo, diag, db.ptr, dx.ptr), "trsv")
            ok = ok and same_bits(Xh[:, c], dx.down())
        rec = {"matrix": name, "triangle": "lower" if lower else "upper", "diag": "unit" if unit else "stored", "k": k,
               "layout": "row" if layout == ROW else "col", "rows": M, "nnz": int(dm.handle.NZ), "levels": info.levels,
               "launches": info.launches, "fusedLevels": info.fusedLevels, "longRows": info.longRows, "analyses": dm.triangular_info(lower).analyses,
               "trsm_ms": round(trsm, 4), "trsv_ms": round(trsv, 4), "k_trsv_ms": round(k * trsv, 4), "ratio": round(trsm / (k * trsv), 4),
               "us_per_launch": round(trsm * 1e3 / max(info.launches, 1), 3), "check_bitwise": ok}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
        bB.free()
        bX.free()
    db.free()
    dx.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="lap7,stencil,c2")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--colmajor-k", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trsm_timing.log"))
    args = ap.parse_args()
    api.spmvHipInit(0)
    ev = Events()
    ks = [int(k) for k in args.ks.split(",")]
    with open(args.out, "a") as out:
        for key in args.matrices.split(","):
            if key == "lap7":
                (name, dm, *_), unit = lap7(), False
            elif key == "stencil":
                (name, dm, *_), unit = stencil(), True
            elif key == "c2":
                (name, dm, *_), unit = synthetic("c2"), True
            else:
                raise SystemExit(f"unknown matrix {key}")
            measure(name, dm, True, unit, ks, args.colmajor_k, ev, out)
            dm.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
