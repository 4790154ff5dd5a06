// coo.hip -- a CSR handle assembled on the device from COO triplets (spmvHipCooAssemble), its values again from a new value
// list on the kept pattern (spmvHipCooAssembleRefresh), and a handle's entries written out as triplets (spmvHipCsrToCoo).
// DESIGN.md section 36; the contract -- the bits of a serial loop that adds the duplicates of (i, j) in input order -- is in
// spmvHip.h.
//
// Entry-parallel throughout: a lane per triplet, never a lane per row.
//   keys     every entry is checked and keyed: key = row << bitsFor(N) | col, a 64-bit word of bitsFor(M + 1) + bitsFor(N)
//            bits.  A skipped entry (row or column SPMV_COO_SKIP) takes the key of row M, past the last row, so the sort
//            puts it behind every kept entry; an entry out of range takes the same key and atomicMin keeps the SMALLEST
//            such e for the refusal.  No value is read.
//   sort     ONE stable radix sort of (key, e) with e from enqueueIota.  The STABILITY is the contract: equal keys keep
//            their payloads ascending, so the duplicates of (i, j) stand in input order and the value pass may add them
//            as it finds them.
//   heads    over the sorted keys of the kept entries, in tiles of CO_TILE: the lane of entry s computes the head flag
//            key[s] != key[s - 1]; the 64-bit ballot of a wavefront is counted into counts[tile].
//   scan     tileBase = the exclusive scan of the counts (device_prims.hpp); its last word is nnz(C).
//   write    the ballots again, a scan of the tile's 16 words in LDS, and the rank q of every head: JA[q], runStart[q], and
//            the row pointers -- the lane of entry s writes IRP[i] = rank(s) for every row i in (row[s - 1], row[s]], a
//            head or not, so the empty rows before a row are filled by the entry after them, however many; the lane of the
//            last kept entry fills the rows behind it.
//   values   ONE kernel for the build and the refresh: the lane of entry q of C walks perm[runStart[q] .. runStart[q + 1])
//            and adds val[perm[.]] serially (SUM) or takes the last (LAST).  A run is added by one lane because the order
//            is the contract: a call costs at least its longest run (info.maxRun).  There is no second path for long runs.
// No floating-point atomic anywhere; the integer atomics (a minimum, a maximum, a count) give the same result in any order.
// Every kernel bounds its reads by the entry counts the host sized the buffers by.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {

// what an assembled handle keeps (DevMat::coo); perm and runStart only with keepMap
struct CooPlan {
    int duplicates = SPMV_COO_SUM;
    uint64_t nEntries = 0;                                     // of the build's triplet list
    uint32_t* perm = nullptr;                                  // the kept entries in sorted order (4 B per kept entry)
    uint32_t* runStart = nullptr;                              // nnz(C) + 1 words: the run of entry q is perm[runStart[q] .. runStart[q + 1])
    spmvCooInfo info{};
};

namespace {

constexpr uint32_t CO_THREADS = WG_THREADS;
constexpr uint32_t CO_WAVES = CO_THREADS / 64;
constexpr uint32_t CO_TILE = 1024;                             // sorted entries of a tile: CO_TILE / CO_THREADS per lane
constexpr uint32_t CO_STEPS = CO_TILE / CO_THREADS;
constexpr uint32_t CO_WORDS = CO_TILE / 64;                    // ballots of a tile
constexpr uint32_t CO_NONE = 0xFFFFFFFFu;

// ----------------------------------------------------------------------------------------------------------- keys
// stat[0] grows by the skipped entries, stat[1] = min(the entries out of range)
__global__ __launch_bounds__(CO_THREADS) void co_key_kernel(uint64_t n, uint64_t M, uint64_t N, unsigned cbits, const uint32_t* __restrict__ row,
                                                           const uint32_t* __restrict__ col, uint64_t* __restrict__ key, uint32_t* __restrict__ stat) {
    const uint64_t e = linear_block() * CO_THREADS + threadIdx.x;
    bool skip = false;
    if (e < n) {
        const uint32_t r = row[e], c = col[e];
        skip = r == SPMV_COO_SKIP || c == SPMV_COO_SKIP;
        const bool bad = !skip && (r >= M || c >= N);
        if (bad) atomicMin(stat + 1, (uint32_t)e);
        key[e] = skip || bad ? M << cbits : (uint64_t)r << cbits | c;
    }
    const uint64_t bal = __ballot(skip);
    if (threadIdx.x % 64 == 0 && bal) atomicAdd(stat, (uint32_t)__popcll(bal));
}

// ---------------------------------------------------------------------------------------------------------- heads
__device__ __forceinline__ bool co_head(const uint64_t* __restrict__ key, uint64_t s, uint64_t k) { return s == 0 || key[s - 1] != k; }

__global__ __launch_bounds__(CO_THREADS) void co_count_kernel(uint64_t nKept, const uint64_t* __restrict__ key, uint32_t* __restrict__ counts) {
    __shared__ uint32_t sCnt[CO_WAVES];
    const uint64_t tile = linear_block(), s0 = tile * CO_TILE;
    if (s0 >= nKept) return;
    uint32_t heads = 0;
    for (uint32_t t = 0; t < CO_STEPS; ++t) {
        const uint64_t s = s0 + t * CO_THREADS + threadIdx.x;
        heads += (uint32_t)__popcll(__ballot(s < nKept && co_head(key, s, key[s])));
    }
    if (threadIdx.x % 64 == 0) sCnt[threadIdx.x / 64] = heads;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < CO_WAVES; ++w) sum += sCnt[w];
        counts[tile] = sum;
    }
}

// rows (from, to] take the row pointer q; to <= M by the key check
__device__ __forceinline__ void co_fill_rows(uint32_t* __restrict__ irp, uint64_t from, uint64_t to, uint32_t q) {
    for (uint64_t i = from; i < to; ++i) irp[i + 1] = q;
}

// nKept >= 1.  irp[0] is written by the lane of entry 0, irp[M] by the lane of the last entry: every word once.
__global__ __launch_bounds__(CO_THREADS) void co_write_kernel(uint64_t nKept, uint64_t M, unsigned cbits, const uint64_t* __restrict__ key,
                                                             const uint32_t* __restrict__ tileBase, uint32_t nnzC, uint32_t* __restrict__ irp,
                                                             uint32_t* __restrict__ ja, uint32_t* __restrict__ runStart) {
    __shared__ uint64_t sBal[CO_WORDS];
    __shared__ uint32_t sPre[CO_WORDS];
    const uint64_t tile = linear_block(), s0 = tile * CO_TILE;
    if (s0 >= nKept) return;
    const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const uint64_t cmask = (1ull << cbits) - 1;
    uint64_t k[CO_STEPS], prev[CO_STEPS];
#pragma unroll
    for (uint32_t t = 0; t < CO_STEPS; ++t) {
        const uint64_t s = s0 + t * CO_THREADS + threadIdx.x;
        const bool live = s < nKept;
        k[t] = live ? key[s] : 0;
        prev[t] = live && s ? key[s - 1] : 0;
        const uint64_t bal = __ballot(live && (s == 0 || prev[t] != k[t]));
        if (lane == 0) sBal[t * CO_WAVES + wave] = bal;
    }
    __syncthreads();
    if (threadIdx.x < CO_WORDS) {
        uint32_t pre = tileBase[tile];
        for (uint32_t w = 0; w < threadIdx.x; ++w) pre += (uint32_t)__popcll(sBal[w]);
        sPre[threadIdx.x] = pre;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t t = 0; t < CO_STEPS; ++t) {
        const uint64_t s = s0 + t * CO_THREADS + threadIdx.x;
        if (s >= nKept) continue;
        const uint32_t w = t * CO_WAVES + wave;
        const uint64_t bal = sBal[w];
        const uint32_t q = sPre[w] + (uint32_t)__popcll(bal & ((1ull << lane) - 1));     // the heads before s: s's own rank where it is one
        const uint64_t r = k[t] >> cbits;                      // < M: a kept entry
        if ((bal >> lane) & 1) {
            if (q >= nnzC) continue;                           // (never: the counts and their scan are one launch sequence)
            ja[q] = (uint32_t)(k[t] & cmask); runStart[q] = (uint32_t)s;
        }
        if (s == 0) { irp[0] = 0; co_fill_rows(irp, 0, r, 0); }
        else co_fill_rows(irp, prev[t] >> cbits, r, q);        // nothing where the row is the one before's (then s may be no head)
        if (s == nKept - 1) { co_fill_rows(irp, r, M, nnzC); runStart[nnzC] = (uint32_t)nKept; }
    }
}

// --------------------------------------------------------------------------------------------------------- values
// maxRun: the build's (null at a refresh).  A single entry is copied as bits; a sum is plain adds in the run's order.
template <int MODE>
__global__ __launch_bounds__(CO_THREADS) void co_value_kernel(uint32_t nnzC, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ runStart,
                                                             const uint64_t* __restrict__ val, uint64_t* __restrict__ as, uint32_t* __restrict__ maxRun) {
    const uint64_t q = linear_block() * CO_THREADS + threadIdx.x;
    uint32_t len = 0;
    if (q < nnzC) {
        const uint32_t b = runStart[q], e = runStart[q + 1];   // b < e
        len = e - b;
        if (MODE == SPMV_COO_LAST || len == 1) {
            as[q] = val[perm[e - 1]];
        } else {
            double v = __longlong_as_double((long long)val[perm[b]]);
            for (uint32_t t = b + 1; t < e; ++t) v = v + __longlong_as_double((long long)val[perm[t]]);
            as[q] = (uint64_t)__double_as_longlong(v);
        }
    }
    if (!maxRun) return;
    for (int off = 32; off; off >>= 1) len = max(len, (uint32_t)__shfl_xor((int)len, off));
    // the word only grows, so a wavefront that does not exceed what it reads there -- however stale -- has nothing to add:
    // one atomic per wavefront on one address would serialise the whole pass
    if (threadIdx.x % 64 == 0 && len > __hip_atomic_load(maxRun, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxRun, len);
}

int fail(hipStream_t st, const char* what) { return buildFail(st, "coo", what); }

void launchValues(int mode, uint32_t nnzC, const uint32_t* perm, const uint32_t* runStart, const double* val, double* as, uint32_t* maxRun, hipStream_t st) {
    const uint64_t* v = reinterpret_cast<const uint64_t*>(val);
    uint64_t* out = reinterpret_cast<uint64_t*>(as);
    if (mode == SPMV_COO_LAST) hipLaunchKernelGGL((co_value_kernel<SPMV_COO_LAST>), gridFor(nnzC), dim3(CO_THREADS), 0, st, nnzC, perm, runStart, v, out, maxRun);
    else hipLaunchKernelGGL((co_value_kernel<SPMV_COO_SUM>), gridFor(nnzC), dim3(CO_THREADS), 0, st, nnzC, perm, runStart, v, out, maxRun);
}

}  // namespace

void freeCooPlan(CooPlan* p) {
    if (!p) return;
    (void)devFree(p->perm); (void)devFree(p->runStart);
    delete p;
}

const spmvCooInfo* cooInfo(const DevMat* c) { return &c->coo->info; }
void cooSetMaxRow(DevMat* c) { c->coo->info.maxRowNnz = c->maxRowNnz; }
bool cooHasMap(const DevMat* c) { return c->coo->perm != nullptr; }
uint64_t cooEntries(const DevMat* c) { return c->coo->nEntries; }

// c: kind, M and N set by the caller, nothing allocated.  On success c owns IRP (4 B), JA, AS and the plan (with keepMap
// its two maps), and c->NZ is set; on failure -- one line has been written -- the caller frees c with whatever it holds.
// An entry out of range is found before JA / AS exist.  The host-side checks have passed: the arrays are not null where
// nEntries > 0, M and N fit 32-bit ids, nEntries < IRP32_LIMIT.
int cooBuild(uint64_t nEntries, const uint32_t* dRow, const uint32_t* dCol, const double* dVal, const spmvCooOpts* o, DevMat* c, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t M = c->M, N = c->N, n = nEntries;
    CooPlan* pl = c->coo = new CooPlan;
    pl->duplicates = o->duplicates;
    pl->nEntries = n;
    const bool keepMap = o->keepMap != 0;
    const unsigned cbits = bitsFor(N), rbits = bitsFor(M + 1); // (a skipped entry has the key of row M)
    spmvCooInfo out{};
    out.nEntries = n;
    TempTally tm;
    if (devMalloc(&c->IRP, (M + 1) * 4) != hipSuccess) return fail(st, "allocation of the row pointers");
    c->irpBytes = 4;
    TempBuf stat(&tm), keyA(&tm), keyB(&tm), idxA(&tm), idxB(&tm), sortTmp(&tm), counts(&tm), base(&tm), scanTmp(&tm), runTmp(&tm);
    const uint64_t* skey = nullptr;
    const uint32_t* sperm = nullptr;
    uint64_t nKept = 0, nnzC = 0;
    if (n) {
        // 1. keys
        if (stat.alloc(3 * 4) || keyA.alloc(n * 8) || keyB.alloc(n * 8) || idxA.alloc(n * 4) || idxB.alloc(n * 4))
            return fail(st, "temporary allocation (24 B per entry)");
        uint32_t* const dStat = stat.as<uint32_t>();          // [0] skipped entries, [1] the first entry out of range, [2] the longest run
        const uint32_t init[3] = {0, CO_NONE, 0};
        if (hipMemcpyAsync(dStat, init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return fail(st, "memset");
        hipLaunchKernelGGL(co_key_kernel, gridFor(n), dim3(CO_THREADS), 0, st, n, M, N, cbits, dRow, dCol, keyA.as<uint64_t>(), dStat);
        enqueueIota(n, idxA.as<uint32_t>(), st);
        uint32_t h[2] = {0, CO_NONE};
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, dStat, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "key pass");
        if (h[1] != CO_NONE) {
            uint32_t rc[2] = {0, 0};
            if (hipMemcpy(rc, dRow + h[1], 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(rc + 1, dCol + h[1], 4, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(st, "key pass");
            fprintf(stderr, "libspmvhip: coo: entry %u is (%u, %u), outside the %lu x %lu matrix\n", h[1], rc[0], rc[1], (unsigned long)M, (unsigned long)N);
            return EXIT_FAILURE;
        }
        out.skipped = h[0];
        nKept = n - h[0];
        // 2. ONE stable sort: equal (row, col) keys keep their entry indices ascending, which is "in input order"
        rocprim::double_buffer<uint64_t> keys(keyA.as<uint64_t>(), keyB.as<uint64_t>());
        rocprim::double_buffer<uint32_t> idx(idxA.as<uint32_t>(), idxB.as<uint32_t>());
        if (sortPairs(sortTmp, keys, idx, n, 0, rbits + cbits, st) != hipSuccess) return fail(st, "sort");
        skey = keys.current();
        sperm = idx.current();
    }
    // 3. heads, scan
    const uint64_t nTiles = (nKept + CO_TILE - 1) / CO_TILE;
    const dim3 tiles = gridFor(nTiles, 1, CO_THREADS);
    if (nKept) {
        if (counts.alloc((nTiles + 1) * 4) || base.alloc((nTiles + 1) * 4)) return fail(st, "temporary allocation (the tile counts)");
        if (hipMemsetAsync(counts.as<uint32_t>() + nTiles, 0, 4, st) != hipSuccess) return fail(st, "memset");
        hipLaunchKernelGGL(co_count_kernel, tiles, dim3(CO_THREADS), 0, st, nKept, skey, counts.as<uint32_t>());
        if (hipGetLastError() != hipSuccess) return fail(st, "head pass");
        if (exclusiveScan(scanTmp, counts.as<uint32_t>(), base.as<uint32_t>(), 0u, (size_t)nTiles + 1, st) != hipSuccess) return fail(st, "scan");
        uint32_t total = 0;
        if (hipMemcpyAsync(&total, base.as<uint32_t>() + nTiles, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "head pass");
        nnzC = total;
    }
    // 4. write
    c->NZ = nnzC;
    const size_t nz1 = std::max<uint64_t>(nnzC, 1);
    if (devMalloc(&c->JA, nz1 * 4) != hipSuccess || devMalloc(&c->AS, nz1 * 8) != hipSuccess) return fail(st, "allocation of the assembled arrays");
    uint32_t* runStart = nullptr;
    if (keepMap) {
        if (devMalloc(&pl->perm, std::max<uint64_t>(nKept, 1) * 4) != hipSuccess || devMalloc(&pl->runStart, (nnzC + 1) * 4) != hipSuccess)
            return fail(st, "allocation of the maps");
        runStart = pl->runStart;
    } else {
        if (runTmp.alloc((nnzC + 1) * 4)) return fail(st, "temporary allocation (the run starts)");
        runStart = runTmp.as<uint32_t>();
    }
    if (nKept) {
        uint32_t* const dStat = stat.as<uint32_t>();
        hipLaunchKernelGGL(co_write_kernel, tiles, dim3(CO_THREADS), 0, st, nKept, M, cbits, skey, base.as<uint32_t>(), (uint32_t)nnzC,
                           static_cast<uint32_t*>(c->IRP), c->JA, runStart);
        // 5. values: from the sorted payloads where they lie, or -- kept for the refresh -- from their copy
        const uint32_t* perm = sperm;
        if (keepMap) {
            if (hipMemcpyAsync(pl->perm, sperm, nKept * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(st, "copy of the map");
            perm = pl->perm;
        }
        launchValues(pl->duplicates, (uint32_t)nnzC, perm, runStart, dVal, c->AS, dStat + 2, st);
        uint32_t maxRun = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&maxRun, dStat + 2, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "write pass");
        out.maxRun = maxRun;
    } else {
        if (hipMemsetAsync(c->IRP, 0, (M + 1) * 4, st) != hipSuccess || hipMemsetAsync(runStart, 0, 4, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "row pointers");
    }
    out.nnzC = nnzC;
    out.duplicates = nKept - nnzC;
    out.tempBytes = tm.peak;
    out.ms = msSince(t0);
    pl->info = out;
    return EXIT_SUCCESS;
}

// c's values again from dVal (the build's triplet list, same order) over the build's runs in the build's mode: kernels only,
// nothing is allocated.  The handle has a map and dVal is not null where there is an entry.
int cooRefresh(DevMat* c, const double* dVal, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    CooPlan* pl = c->coo;
    if (c->NZ) {
        launchValues(pl->duplicates, (uint32_t)c->NZ, pl->perm, pl->runStart, dVal, c->AS, nullptr, st);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(st, "value pass");
    }
    pl->info.tempBytes = 0;
    pl->info.ms = msSince(t0);
    return EXIT_SUCCESS;
}

// (i, JA[p], AS[p]) for p in stored order into the caller's arrays (dVal may be null): kernels and copies only
int csrToCoo(const DevMat* a, uint32_t* dRow, uint32_t* dCol, double* dVal, hipStream_t st) {
    if (!a->NZ) return EXIT_SUCCESS;
    enqueueRowOf(a->M, a->IRP, a->irpBytes, dRow, st);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(dCol, a->JA, a->NZ * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        (dVal && hipMemcpyAsync(dVal, a->AS, a->NZ * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) || hipStreamSynchronize(st) != hipSuccess)
        return buildFail(st, "coo", "writing the triplets");
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
