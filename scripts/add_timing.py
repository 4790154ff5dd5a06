"""Sparse sums on the device (spmvHipCsrAdd, spmvHipCsrAddRefresh) on the 500 x 100 x 100 7-point
Laplacian: A + A^T with the transpose handle, the shift A - sigma I with an uploaded identity, and the smoothed prolongator
T - omega (D^-1 A T) of the 2 x 2 x 2 aggregation, its product part built by spmvHipSpGEMM.

Records (one JSON line each), per sum:
  default      terms, nnzC, class counts, sort batches, temporaries, symbolic / numeric / total ms of the build (second of
               two), ms of a refresh (second of two), and the GB/s of the numeric phase and of the refresh against the
               algorithmic bytes 12 (nnzA + nnzB + nnzC) + 4 * 3 (M + 1)
  sorted       the same sum with every row forced onto the sorted path (allSorted)
  torch        for information only: torch's sparse add on CSR tensors of the same matrices (compared with allclose, not as
               bits), ms of the second of two calls
Nothing here asserts a time.

    python scripts/add_timing.py [--quick] [--out profiles/add_timing.log]
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

from spmv_openmp_cuda_amd import api  # noqa: E402
import add_ref as ar  # noqa: E402
import spgemm_ref as sr  # noqa: E402

INFO = ("terms", "nnzC", "maxRowTerms", "maxRowNnz", "rowsLane", "rowsWave", "rowsSorted", "sortBatches", "tempBytes",
        "symbolicMs", "numericMs", "ms")


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def down(ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        api._check(api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes), "download")
    return out


def arrays(dm):
    h = dm.handle
    return down(h.IRP, h.M + 1, np.uint32), down(h.JA, h.NZ, np.uint32), down(h.AS, h.NZ, np.float64)


def build(da, db, alpha, beta, **opts):
    """the second of two builds: its info and the handle"""
    da.add(db, alpha, beta, **opts).free()
    dc = da.add(db, alpha, beta, **opts)
    info = dc.add_info()
    return dc, {k: getattr(info, k) for k in INFO}


def gbs(nbytes, ms):
    return nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0


def torch_sum(alpha, host_a, beta, host_b):
    import torch

    def tensor(A):
        return torch.sparse_csr_tensor(torch.from_numpy(A[2].astype(np.int64)), torch.from_numpy(A[3].astype(np.int64)),
                                       torch.from_numpy(A[4]), size=(A[0], A[1])).cuda()
    ta, tb = tensor(host_a) * alpha, tensor(host_b)
    torch.add(ta, tb, alpha=beta)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tc = torch.add(ta, tb, alpha=beta)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, tc


def one(out, name, alpha, host_a, da, beta, host_b, db, with_torch):
    dc, rec = build(da, db, alpha, beta)
    nbytes = 12 * (int(da.handle.NZ) + int(db.handle.NZ) + rec["nnzC"]) + 4 * 3 * (int(da.handle.M) + 1)
    emit(out, {"sum": name, "path": "default", **rec, "algorithmicBytes": nbytes, "numericGBs": gbs(nbytes, rec["numericMs"])})
    for path, d, opts in (("default", dc, {}), ("sorted", None, {"allSorted": True})):
        if d is None:
            d, rec = build(da, db, alpha, beta, **opts)
            emit(out, {"sum": name, "path": path, **rec, "numericGBs": gbs(nbytes, rec["numericMs"])})
            emit(out, {"sum": name, "equal_bits_default_sorted": all(np.array_equal(u.view(np.uint8), v.view(np.uint8))
                                                                     for u, v in zip(arrays(dc), arrays(d)))})
        d.add_refresh(da, db, alpha, beta)
        t0 = time.perf_counter()
        d.add_refresh(da, db, alpha, beta)
        ms = (time.perf_counter() - t0) * 1e3
        num = d.add_info().numericMs
        emit(out, {"sum": name, "path": path, "refreshMs": ms, "refreshNumericMs": num, "refreshNumericGBs": gbs(nbytes, num)})
        if d is not dc:
            d.free()
    if with_torch:
        try:
            ms, tc = torch_sum(alpha, host_a, beta, host_b)
            irp, ja, a = arrays(dc)
            tc = tc.to_sparse_csr() if tc.layout != __import__("torch").sparse_csr else tc
            same_pattern = int(tc._nnz()) == ja.size
            close = bool(same_pattern and np.allclose(tc.values().cpu().numpy(), a, rtol=1e-12, atol=1e-9))
            emit(out, {"sum": name, "path": "torch.add", "ms": ms, "nnz": int(tc._nnz()), "allclose": close})
        except Exception as e:                                      # (for information only: a torch build without a CSR add)
            emit(out, {"sum": name, "path": "torch.add", "error": repr(e)[:200]})
    return dc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="60 x 40 x 40 instead of 500 x 100 x 100")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "add_timing.log"))
    args = ap.parse_args()
    nx, ny, nz = (60, 40, 40) if args.quick else (500, 100, 100)
    omega, sigma = 2.0 / 3.0, 0.25
    api.spmvHipInit(0)
    with open(args.out, "w") as out:
        emit(out, {"grid": [nx, ny, nz], "note": "wall ms of synchronous calls; the second of two"})
        A = sr.laplacian7(nx, ny, nz)
        A = A[:4] + (np.random.default_rng(25).standard_normal(A[3].size),)
        M = A[0]
        da = api.spMatCpyCSR(api.HostCSR(*A))
        dt = da.transpose()
        one(out, "A + A^T", 1.0, A, da, 1.0, sr.transpose(A), dt, not args.no_torch).free()
        dt.free()
        I = ar.identity(M)
        di = api.spMatCpyCSR(api.HostCSR(*I))
        one(out, "A - sigma I", 1.0, A, da, -sigma, I, di, not args.no_torch).free()
        di.free()
        T = sr.aggregation(nx, ny, nz)
        Dinv = I[:4] + (1.0 / np.where(ar.diagonal(A) != 0, ar.diagonal(A), 1.0),)
        dT, dd = api.spMatCpyCSR(api.HostCSR(*T)), api.spMatCpyCSR(api.HostCSR(*Dinv))
        dat = da.multiply(dT)
        ddat = dd.multiply(dat)
        irp, ja, a = arrays(ddat)
        DAT = (M, T[1], irp.astype(np.uint64), ja.astype(np.uint64), a)
        one(out, "T - omega (D^-1 A T)", 1.0, T, dT, -omega, DAT, ddat, not args.no_torch).free()
        for d in (ddat, dat, dd, dT, da):
            d.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
