"""Sparse products on the device (spmvHipSpGEMM, spmvHipSpGEMMRefresh): the 500 x 100 x 100 7-point
Laplacian squared, the Galerkin product P^T (A P) of its 2 x 2 x 2 aggregation, and A A^T of the upwind convection-diffusion
matrix of the same size.

Records (one JSON line each), per product:
  default      products, nnzC, class counts, sort batches, temporaries, symbolic / numeric / total ms of the build (second of
               two), ms of a refresh (second of two)
  sorted       the same product with every row forced onto the sorted path (waveMaxProducts = groupMaxProducts = 1)
  torch        for information only: torch.sparse.mm on CSR tensors of the same matrices (another summation order, so compared
               with allclose, not as bits), ms of the second of two calls
Nothing here asserts a time.

    python scripts/spgemm_timing.py [--quick] [--out profiles/spgemm_timing.log]
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
import spgemm_ref as sr  # noqa: E402
from test_krylov_abi import convdiff7  # noqa: E402

INFO = ("products", "nnzC", "maxRowProducts", "maxRowNnz", "rowsWave", "rowsGroup", "rowsSorted", "sortBatches", "tempBytes",
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


def build(da, db, **opts):
    """the second of two builds: its info and the handle"""
    da.multiply(db, **opts).free()
    dc = da.multiply(db, **opts)
    info = dc.spgemm_info()
    return dc, {k: getattr(info, k) for k in INFO}


def torch_product(host_a, host_b):
    import torch

    def tensor(A):
        return torch.sparse_csr_tensor(torch.from_numpy(A[2].astype(np.int64)), torch.from_numpy(A[3].astype(np.int64)),
                                       torch.from_numpy(A[4]), size=(A[0], A[1])).cuda()
    ta, tb = tensor(host_a), tensor(host_b)
    torch.sparse.mm(ta, tb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tc = torch.sparse.mm(ta, tb)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, tc


def one(out, name, host_a, host_b, da, db, with_torch):
    dc, rec = build(da, db)
    emit(out, {"product": name, "path": "default", **rec})
    dc.multiply_refresh(da, db)
    t0 = time.perf_counter()
    dc.multiply_refresh(da, db)
    emit(out, {"product": name, "path": "default", "refreshMs": (time.perf_counter() - t0) * 1e3,
               "refreshNumericMs": dc.spgemm_info().numericMs})
    ds, rec = build(da, db, waveMaxProducts=1, groupMaxProducts=1)
    emit(out, {"product": name, "path": "sorted", **rec})
    emit(out, {"product": name, "equal_bits_default_sorted": all(np.array_equal(u.view(np.uint8), v.view(np.uint8))
                                                                 for u, v in zip(arrays(dc), arrays(ds)))})
    ds.free()
    if with_torch:
        try:
            ms, tc = torch_product(host_a, host_b)
            irp, ja, a = arrays(dc)
            same_pattern = int(tc._nnz()) == ja.size
            close = bool(same_pattern and np.allclose(tc.values().cpu().numpy(), a, rtol=1e-12, atol=1e-9))
            emit(out, {"product": name, "path": "torch.sparse.mm", "ms": ms, "nnz": int(tc._nnz()), "allclose": close})
        except Exception as e:                                      # (for information only: a torch build without CSR spgemm)
            emit(out, {"product": name, "path": "torch.sparse.mm", "error": repr(e)[:200]})
    return dc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="60 x 40 x 40 instead of 500 x 100 x 100")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm_timing.log"))
    args = ap.parse_args()
    nx, ny, nz = (60, 40, 40) if args.quick else (500, 100, 100)
    api.spmvHipInit(0)
    with open(args.out, "w") as out:
        emit(out, {"grid": [nx, ny, nz], "note": "wall ms of synchronous calls; the second of two"})
        A = sr.laplacian7(nx, ny, nz)
        P = sr.aggregation(nx, ny, nz)
        da, dp = api.spMatCpyCSR(api.HostCSR(*A)), api.spMatCpyCSR(api.HostCSR(*P))
        one(out, "laplacian^2", A, A, da, da, not args.no_torch).free()
        dap = one(out, "A P", A, P, da, dp, False)
        dpt = dp.transpose()
        irp, ja, a = arrays(dap)
        AP = (A[0], P[1], irp.astype(np.uint64), ja.astype(np.uint64), a)
        one(out, "P^T (A P)", sr.transpose(P), AP, dpt, dap, not args.no_torch).free()
        for d in (dap, dpt, dp, da):
            d.free()
        IRP, JA, AS = convdiff7(nx, ny, nz)
        Cd = (nx * ny * nz, nx * ny * nz, IRP, JA, AS)
        dc_ = api.spMatCpyCSR(api.HostCSR(*Cd))
        dct = dc_.transpose()
        one(out, "convdiff A A^T", Cd, sr.transpose(Cd), dc_, dct, not args.no_torch).free()
        dct.free()
        dc_.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
