"""Reverse Cuthill-McKee on the device (spmvHipRcmCSR): what the call costs and what the ordering buys.

Matrices:
  (a) the 500 x 100 x 100 7-point Laplacian permuted by a seeded random permutation through spmvHipCsrPermute
  (b) the same in natural order
  (c) the road-network stand-in of the benchmark (csrc/host/structured.c kind 1, through the loader)
  (d) the c3 power-law generator at 1/10 scale
  (e) 20 000 disjoint edges (40 000 rows, randomly numbered): many small components.  Not among the default matrices:
      --only e --out profiles/rcm_timing_components.log
--scale s shrinks every matrix (rows x s; the grid's first dimension); the log's header says which scale it holds.

Records (one JSON line each; every timed figure is a median of at least five, taken after a warm-up call):
  rcm      per matrix and T in (1024, 0): bandwidthBefore / bandwidthAfter, levels, components, startBfs, maxFrontier, longRows,
           symmetric, launches, hostChecks, wall ms of the call; cpu_ms: the same loop in C on one CPU thread (gcc -O2,
           compiled here) over the ready-made adjacency -- the device call builds its adjacency inside its time -- and
           equal: the device's words == the C loop's words
  effect   per matrix: hipSpMVRowsCSR and hipSpMVWarpPerRowCSR ms (device events) on the handle and on B = P A P^T, the
           wall ms of spmvHipCsrPermute, and the ILU(0) level counts (lower triangle's level sets) before and after where the
           matrix has a full diagonal

    python scripts/rcm_timing.py [--scale 1.0] [--only a,b,c,d] [--out profiles/rcm_timing.log]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from spmv_openmp_cuda_amd import api, synth  # noqa: E402
from spmm_timing import Events  # noqa: E402

HYPOTHESES = """# hypotheses, written before the numbers:
#   H1 (a): the random numbering has bandwidth ~M; RCM brings it to the order of the grid's cross-section (~1e4 at full
#      scale) and the SpMV on B comes within 1.3x of the natural-order handle (b) measured in the same process.
#   H2 (b): nothing to gain: bandwidthAfter is of the order of bandwidthBefore and the SpMV time does not improve.
#   H3 (c): the road stand-in has thousands of thin levels; at T = 1024 the call takes far fewer launches than levels and
#      is several times faster than at T = 0, where every level is a launch, a read-back and a sort.
#   H4 (d): a graph with uniformly spread edges has no narrow ordering: bandwidthAfter stays of the order of M and the SpMV
#      does not gain.  Reported as such.
#   H6 (e): the one workgroup takes the components one after the other, about ten steps of its state machine each at a few
#      microseconds a step: the call takes tens of microseconds per component and is one to two orders of magnitude slower
#      than the C loop; at T = 0 every component is several round trips to the host and slower again.
#   H5: the call is slower than the one-thread C loop wherever levels x per-level cost dominates ((c), and (a)/(b) with
#      their ~700 levels): a finding to be written down, not tuned away here.
"""

C_SOURCE = r"""
#include <stdint.h>
#include <stdlib.h>
static const uint32_t* g_deg;
static int by_deg_id(const void* a, const void* b) {
    uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
    if (g_deg[x] != g_deg[y]) return g_deg[x] < g_deg[y] ? -1 : 1;
    return x < y ? -1 : x > y;
}
/* the level structure of r among the vertices with visited[] == 0: its depth, and *vmin = the vertex of the last level of
   smallest (deg, id) */
static uint32_t levels_of(uint32_t r, const uint64_t* ptr, const uint32_t* col, const uint32_t* deg, const uint8_t* visited,
                          uint32_t* mark, uint32_t stamp, uint32_t* q, uint32_t* vmin) {
    uint32_t head = 0, tail = 1, depth = 0, lo = 0;
    q[0] = r; mark[r] = stamp;
    while (head < tail) {
        uint32_t end = tail;
        lo = head; ++depth;
        for (; head < end; ++head)
            for (uint64_t p = ptr[q[head]]; p < ptr[q[head] + 1]; ++p) {
                uint32_t j = col[p];
                if (!visited[j] && mark[j] != stamp) { mark[j] = stamp; q[tail++] = j; }
            }
    }
    uint32_t best = q[lo];
    for (uint32_t k = lo; k < tail; ++k)
        if (deg[q[k]] < deg[best] || (deg[q[k]] == deg[best] && q[k] < best)) best = q[k];
    *vmin = best;
    return depth;
}
int rcm_serial(uint32_t M, const uint64_t* ptr, const uint32_t* col, int peripheral, uint32_t maxPasses, int forward, uint32_t* perm) {
    uint32_t *deg = malloc(4u * (M + 1)), *byDeg = malloc(4u * (M + 1)), *mark = calloc(M + 1, 4), *q = malloc(4u * (M + 1));
    uint32_t* order = malloc(4u * (M + 1));
    uint8_t* visited = calloc(M + 1, 1);
    uint32_t maxDeg = 0, stamp = 0, done = 0, cursor = 0;
    for (uint32_t i = 0; i < M; ++i) { deg[i] = (uint32_t)(ptr[i + 1] - ptr[i]); if (deg[i] > maxDeg) maxDeg = deg[i]; }
    uint32_t* cnt = calloc((size_t)maxDeg + 2, 4);
    for (uint32_t i = 0; i < M; ++i) ++cnt[deg[i] + 1];
    for (uint32_t d = 0; d <= maxDeg; ++d) cnt[d + 1] += cnt[d];
    for (uint32_t i = 0; i < M; ++i) byDeg[cnt[deg[i]]++] = i;
    g_deg = deg;
    while (done < M) {
        while (visited[byDeg[cursor]]) ++cursor;
        uint32_t r = byDeg[cursor];
        if (peripheral) {
            uint32_t v, depth = levels_of(r, ptr, col, deg, visited, mark, ++stamp, q, &v), n = 1;
            while (n <= maxPasses) {
                if (v == r) break;
                uint32_t v2, d2 = levels_of(v, ptr, col, deg, visited, mark, ++stamp, q, &v2);
                ++n;
                if (d2 > depth) { r = v; depth = d2; v = v2; } else break;
            }
        }
        uint32_t head = done, tail = done;
        order[tail++] = r; visited[r] = 1;
        while (head < tail) {
            uint32_t u = order[head++], first = tail;
            for (uint64_t p = ptr[u]; p < ptr[u + 1]; ++p) {
                uint32_t j = col[p];
                if (!visited[j]) { visited[j] = 1; order[tail++] = j; }
            }
            if (tail - first > 1) qsort(order + first, tail - first, 4, by_deg_id);
        }
        done = tail;
    }
    for (uint32_t k = 0; k < M; ++k) perm[k] = forward ? order[k] : order[M - 1 - k];
    free(deg); free(byDeg); free(mark); free(q); free(order); free(visited); free(cnt);
    return 0;
}
"""


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def c_loop():
    d = tempfile.mkdtemp(prefix="rcm_timing_")
    src, so = os.path.join(d, "rcm_serial.c"), os.path.join(d, "rcm_serial.so")
    open(src, "w").write(C_SOURCE)
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, src])
    fn = C.CDLL(so).rcm_serial
    fn.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p]
    return fn


def adjacency(M, IRP, JA):
    """the deduplicated pattern of A + A^T without the diagonal, as (ptr u64, col u32)"""
    IRP, JA = np.asarray(IRP, dtype=np.int64), np.asarray(JA, dtype=np.int64)
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(IRP))
    keep = (JA != rows) & (JA < M)
    key = np.unique(np.concatenate([rows[keep] * M + JA[keep], JA[keep] * M + rows[keep]]))
    ptr = np.zeros(M + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(np.bincount(key // M, minlength=M))
    return ptr, (key % M).astype(np.uint32)


def down(ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        api._check(api.lib.spmvHipMemcpyDown(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes), "download")
    return out


def pattern_of(dm):
    h = dm.handle
    irp = down(h.IRP, h.M + 1, np.uint32 if getattr(dm, "irp_bytes", 4) == 4 else np.uint64)
    return int(h.M), irp.astype(np.uint64), down(h.JA, h.NZ, np.uint32)


def laplacian(nx, ny, nz):
    from test_trsv_abi import laplacian7
    IRP, JA, AS = laplacian7(nx, ny, nz)
    return api.spMatCpyCSR(api.HostCSR(nx * ny * nz, nx * ny * nz, IRP, JA, AS))


def road(rows):
    H = api.hostlib
    path = os.path.join(tempfile.mkdtemp(prefix="rcm_timing_"), "road.mtx")
    Mv, NZv, mxv = C.c_ulong(), C.c_ulong(), C.c_ulong()
    if H.spmvSynthWriteMtx(path.encode(), 1, rows, 0, 0, 0x57A7 + 1, C.byref(Mv), C.byref(NZv), C.byref(mxv)):
        raise RuntimeError("spmvSynthWriteMtx failed")
    csr = H.MMtoCSR(path.encode())
    os.remove(path)
    m = csr.contents
    M, nnz = int(m.M), int(m.NZ)
    IRP = np.ctypeslib.as_array(m.IRP, shape=(M + 1,)).astype(np.uint64)
    JA = np.ctypeslib.as_array(m.JA, shape=(nnz,)).astype(np.uint64)
    AS = np.ctypeslib.as_array(m.AS, shape=(nnz,)).copy()
    return api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, AS))


def powerlaw(scale):
    w = synth.scaled(synth.WORKLOADS["c3"], 0.1 * scale)
    return synth.device_csr(w, synth.prefix(synth.row_lengths(w)), 0, w.N)


def disjoint_edges(edges):
    import rcm_ref
    M, IRP, JA = rcm_ref.from_edges(2 * edges, 2 * np.arange(edges), 2 * np.arange(edges) + 1, seed=39)
    return api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA, np.where(np.repeat(np.arange(M), 2) == JA.astype(np.int64), 2.0, -1.0)))


def spmv_ms(ev, dm, launcher):
    M = int(dm.handle.M)
    dx, dy = api.DeviceVector(M).up(synth.make_x(M, 3)), api.DeviceVector(M)
    api.spmv(launcher, dm, dx, dy)                               # (the selection, if the launcher has one, happens here)
    api.lib.spmvHipSetSync(0)
    fn = getattr(api.lib, launcher)
    ms = ev.median(lambda: fn(C.byref(dm.handle), dx.ptr, api.CONFIG(), dy.ptr), reps=7)
    api.lib.spmvHipSetSync(1)
    dx.free()
    dy.free()
    return ms


def ilu_levels(dm):
    """the level sets of the lower triangle, or None where ILU(0) does not take the matrix"""
    M, IRP, JA = pattern_of(dm)
    twin = api.spMatCpyCSR(api.HostCSR(M, M, IRP, JA.astype(np.uint64), down(dm.handle.AS, dm.handle.NZ, np.float64)))
    try:
        twin.triangular_analyse(True)
        return int(twin.triangular_info(True).levels)
    except api.SpmvHipError:
        return None
    finally:
        twin.free()


def measure(out, ev, serial, name, dm, reps):
    M, IRP, JA = pattern_of(dm)
    ptr, col = adjacency(M, IRP, JA)
    perm_c = np.empty(M, dtype=np.uint32)
    cpu = []
    for _ in range(reps):
        t0 = time.perf_counter()
        serial(M, ptr.ctypes.data, col.ctypes.data, 1, 8, 0, perm_c.ctypes.data)
        cpu.append((time.perf_counter() - t0) * 1e3)
    keep = None
    for T in (1024, 0):
        api.set_variant("spmvHipRcmCSR", T)
        ms, o = [], dm.rcm()                                     # (a warm-up call: the first one is not among the timed)
        for _ in range(reps):
            o.free()
            o = dm.rcm()
            ms.append(o.info.ms)
        i = o.info
        emit(out, {"record": "rcm", "matrix": name, "M": M, "nnz": int(dm.handle.NZ), "T": T, "bandwidthBefore": int(i.bandwidthBefore),
                   "bandwidthAfter": int(i.bandwidthAfter), "levels": int(i.levels), "components": int(i.components), "startBfs": int(i.startBfs),
                   "maxFrontier": int(i.maxFrontier), "longRows": int(i.longRows), "symmetric": int(i.symmetric), "launches": int(i.launches),
                   "hostChecks": int(i.hostChecks), "ms": round(float(np.median(ms)), 3), "runs": len(ms),
                   "cpu_ms": round(float(np.median(cpu)), 3), "equal": bool(np.array_equal(o.perm.down(np.uint32), perm_c))})
        if T:
            keep = o
        else:
            o.free()
    api.set_variant("spmvHipRcmCSR", 1024)
    B, permute = dm.permute(keep), []                            # (a warm-up call)
    for _ in range(reps):
        B.free()
        t0 = time.perf_counter()
        B = dm.permute(keep)
        permute.append((time.perf_counter() - t0) * 1e3)
    rec = {"record": "effect", "matrix": name, "permute_ms": round(float(np.median(permute)), 3), "permute_runs": len(permute)}
    for launcher in ("hipSpMVRowsCSR", "hipSpMVWarpPerRowCSR"):
        rec[launcher + "_before_ms"] = round(spmv_ms(ev, dm, launcher), 4)
        rec[launcher + "_after_ms"] = round(spmv_ms(ev, B, launcher), 4)
    rec["ilu0_levels_before"], rec["ilu0_levels_after"] = ilu_levels(dm), ilu_levels(B)
    emit(out, rec)
    B.free()
    keep.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rcm_timing.log"))
    a = ap.parse_args()
    only = set(a.only.split(","))
    api.spmvHipInit(0)
    ev, serial = Events(), c_loop()
    out = open(a.out, "w")
    out.write(f"# scripts/rcm_timing.py --scale {a.scale:g} on the MI355X; one JSON record per line (fields: the script's docstring)\n")
    out.write(HYPOTHESES)
    out.flush()
    nx = max(8, int(500 * a.scale))
    lap = laplacian(nx, 100, 100) if only & {"a", "b"} else None
    makers = (("a", f"(a) laplace7-{nx}x100x100, random numbering",
               lambda: lap.permute(np.random.default_rng(37).permutation(int(lap.handle.M)).astype(np.uint32))),
              ("b", f"(b) laplace7-{nx}x100x100, natural order", lambda: lap),
              ("c", "(c) road stand-in", lambda: road(max(8, int(12_000_000 * a.scale)))),
              ("d", "(d) c3 power law at 1/10 scale", lambda: powerlaw(a.scale)),
              ("e", "(e) disjoint edges", lambda: disjoint_edges(max(8, int(20_000 * a.scale)))))
    for key, name, make in makers:
        if key not in only:
            continue
        try:                                                     # one matrix that fails does not cost the others their figures
            dm = make()
            measure(out, ev, serial, name, dm, a.reps)
            if dm is not lap:
                dm.free()
        except (api.SpmvHipError, RuntimeError, MemoryError) as e:
            emit(out, {"record": "failed", "matrix": name, "error": str(e)[:300]})
            if api.lib.spmvHipDeviceSynchronize() != 0:          # a device error: nothing more runs on it
                sys.exit(3)
    if lap is not None:
        lap.free()
    api.spmvHipFinalize()


if __name__ == "__main__":
    main()
