#!/usr/bin/env python3
"""Shape of the private formats a library builds, for comparing two builds of libspmvhip.so (SPMV_LIB names the other one):
    python3 scripts/format_shapes.py [c3 c2 test40k]
For every matrix the automatic arrival-order and the automatic deterministic form of the two-phase and the stripes format
are built; every field of spmvTilesInfo / spmvStripesInfo except the times is printed, and the formats' byte totals.
test40k is the 40 000 x 40 000 matrix with 8 entries per row of tests/test_gpu_parity.py.  Two libraries that build the
same formats print the same lines."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fields(info):
    return " ".join(f"{f}={getattr(info, f)}" for f, _ in info._fields_ if not f.endswith("Ms"))


def main():
    import numpy as np
    from spmv_openmp_cuda_amd import api, synth
    api.spmvHipInit(0)
    for name in sys.argv[1:] or ["c3", "c2", "test40k"]:
        if name == "test40k":
            from conftest import random_csr
            M = N = 40_000
            IRP, JA, AS = random_csr(np.random.default_rng(32), M, N, np.full(M, 8))
            dm = api.spMatCpyCSR(api.HostCSR(M, N, IRP, JA, AS))
        else:
            w = synth.WORKLOADS[name]
            dm = synth.device_csr(w, synth.prefix(synth.row_lengths(w)), 0, w.N)
        for det in (0, 1):
            api.build_tiles(dm, deterministic=det)
            print(f"{name} tiles det={det}: {fields(api.tiles_info(dm))}")
            api.build_stripes(dm, deterministic=det)
            print(f"{name} stripes det={det}: {fields(api.stripes_info(dm))}")
        print(f"{name} spmvHipTilesBytes={api.lib.spmvHipTilesBytes(C.byref(dm.handle))} "
              f"spmvHipStripesBytes={api.lib.spmvHipStripesBytes(C.byref(dm.handle))}", flush=True)
        dm.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
