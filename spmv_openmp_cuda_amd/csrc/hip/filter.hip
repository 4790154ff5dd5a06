// filter.hip -- the entry filter of a device CSR handle: C = the entries of A that a predicate keeps, as a CSR handle of its
// own (spmvHipCsrFilter), and its values again on the kept pattern (spmvHipCsrFilterRefresh).  DESIGN.md section 29; the
// contract -- a copy as bits, and with `lump` one ordered sum per row -- is in spmvHip.h.
//
// Entry-parallel: a lane per stored entry, never a lane per row, so the cost does not depend on how the row lengths are
// distributed.  A workgroup takes a TILE of FL_TILE consecutive entries.
//   rows     the row of an entry comes from the slice of A's row pointers that covers the tile: two lanes find the rows
//            of the tile's first and last entry (binary searches over IRP), the slice between them is staged in LDS
//            relative to the tile (clamped to [0, FL_TILE]) and every entry takes an upper bound in it -- empty rows fall
//            out of the upper bound.  The slice holds at most FL_SLICE words: a tile that spans more rows (it then spans
//            empty ones: a tile has at most FL_TILE rows with an entry) searches the same window in global memory.
//   diagonal (STRENGTH and `lump`) every entry (i, i) counts into cnt[i] (an integer atomic) and leaves its position; a row
//            pass takes d_i where the count is 1 and flags the first other row with atomicMin.
//   judge    the predicate per entry; the 64-bit ballot of a wavefront is one word of the keep mask (1 bit per entry of A),
//            and the tile's kept count goes to counts[tile].  A column id >= N is flagged before d is read at it.
//   scan     tileBase = the exclusive scan of the counts (device_prims.hpp).
//   write    rank(p) = tileBase[tile] + the popcounts of the tile's mask words before p's + the bits below p in its own:
//            a kept entry p goes to rank(p) -- stored order is kept by construction --, IRP_C[i] = rank(IRP_A[i]).
//   lump     the one ordered sum: v = d_i, then v = v + A.AS[p] over the dropped p of row i in stored order -- a lane per
//            row of at most 64 entries, a wavefront per longer row (coalesced loads; the ballot of the dropped lanes is
//            walked in order, each value broadcast by a shuffle, so every lane holds the same serial sum).
// No floating-point atomic and no scratch anywhere (profiles/filter_kernels.txt).  Every kernel bounds its reads by NZ, M
// and the tile window the host sized the buffers by.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {

// what a filter handle keeps besides its map (DevMat::filt); the last four only with `lump`
struct FilterPlan {
    spmvFilterOpts opts{};
    uint64_t* mask = nullptr;                                  // 1 bit per entry of A: kept (FL_WORDS words per tile)
    uint32_t* diagC = nullptr;                                 // the position in C of row i's diagonal entry
    uint32_t* longList = nullptr;                              // the rows of A above 64 entries
    uint32_t nLong = 0;
    spmvFilterInfo info{};
};

namespace {

constexpr uint32_t FL_THREADS = WG_THREADS;
constexpr uint32_t FL_WAVES = FL_THREADS / 64;
constexpr uint32_t FL_TILE = 1024;                             // entries of a tile: FL_TILE / FL_THREADS per lane
constexpr uint32_t FL_WORDS = FL_TILE / 64;                    // mask words of a tile
constexpr uint32_t FL_SLICE = FL_TILE + 2;                     // row pointers of a tile staged in LDS, at most
constexpr uint32_t FL_LONG = 64;                               // entries of a row above which the lump takes a wavefront
constexpr uint32_t FL_NONE = 0xFFFFFFFFu;

struct FilterArgs { int64_t lo, hi; double theta, tt; };       // tt = theta * theta, rounded once on the host

// ------------------------------------------------------------------------------------------------- the rows of a tile
// the first k in [lo, hi) with irp[k] > p, or hi
template <typename I>
__device__ __forceinline__ uint32_t fl_upper(const I* __restrict__ irp, uint32_t lo, uint32_t hi, uint64_t p) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)irp[mid] > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

struct TileRows { uint32_t rLo, rHi, n; bool lds; };           // the rows of the tile's first and last entry; n words staged

// Called by every lane of the workgroup (two barriers).  Entries [p0, p1), p0 < p1 <= NZ = irp[M].
template <typename I>
__device__ __forceinline__ TileRows fl_tile_rows(uint64_t M, const I* __restrict__ irp, uint64_t p0, uint64_t p1, uint32_t* sIrp, uint32_t* sEnds) {
    if (threadIdx.x < 2) sEnds[threadIdx.x] = fl_upper(irp, 0u, (uint32_t)M + 1, threadIdx.x ? p1 - 1 : p0) - 1;   // (irp[0] = 0 <= p < irp[M])
    __syncthreads();
    TileRows t;
    t.rLo = sEnds[0]; t.rHi = sEnds[1];
    const uint64_t n = (uint64_t)t.rHi - t.rLo + 2;            // irp[rLo .. rHi + 1]
    t.lds = n <= FL_SLICE;
    t.n = t.lds ? (uint32_t)n : 0u;
    for (uint32_t k = threadIdx.x; k < t.n; k += FL_THREADS) {
        const uint64_t v = irp[t.rLo + k];
        sIrp[k] = v <= p0 ? 0u : (uint32_t)min(v - p0, (uint64_t)FL_TILE);
    }
    __syncthreads();
    return t;
}

// the row of entry p = p0 + q of the tile
template <typename I>
__device__ __forceinline__ uint32_t fl_row(const TileRows& t, const I* __restrict__ irp, const uint32_t* sIrp, uint64_t p, uint32_t q) {
    if (!t.lds) return fl_upper(irp, t.rLo, t.rHi + 1, p) - 1; // (irp[rLo] <= p < irp[rHi + 1])
    uint32_t lo = 1, hi = t.n - 1;                             // sIrp[0] = 0 <= q < sIrp[n - 1]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (sIrp[mid] > q) hi = mid; else lo = mid + 1;
    }
    return t.rLo + lo - 1;
}

// ----------------------------------------------------------------------------------------------------- the diagonal
template <typename I>
__global__ __launch_bounds__(FL_THREADS) void fl_diag_kernel(uint64_t M, uint64_t NZ, const I* __restrict__ irp, const uint32_t* __restrict__ ja,
                                                            uint32_t* __restrict__ cnt, uint32_t* __restrict__ dpos) {
    __shared__ uint32_t sIrp[FL_SLICE], sEnds[2];
    const uint64_t p0 = linear_block() * FL_TILE;
    if (p0 >= NZ) return;
    const uint64_t p1 = min(p0 + FL_TILE, NZ);
    const TileRows t = fl_tile_rows(M, irp, p0, p1, sIrp, sEnds);
    for (uint32_t q = threadIdx.x; q < FL_TILE; q += FL_THREADS) {
        const uint64_t p = p0 + q;
        if (p >= p1) break;
        const uint32_t i = fl_row(t, irp, sIrp, p, q);
        if (ja[p] == i) { atomicAdd(cnt + i, 1u); dpos[i] = (uint32_t)p; }
    }
}

// d_i where row i holds exactly one entry (i, i); *bad = the first other row
__global__ __launch_bounds__(FL_THREADS) void fl_dval_kernel(uint64_t M, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ dpos,
                                                            const double* __restrict__ as, double* __restrict__ d, uint32_t* __restrict__ bad) {
    const uint64_t r = linear_block() * FL_THREADS + threadIdx.x;
    if (r >= M) return;
    if (cnt[r] == 1) d[r] = as[dpos[r]];
    else { d[r] = 0.0; atomicMin(bad, (uint32_t)r); }
}

// ------------------------------------------------------------------------------------------------------- the judge
// DIAG: the entry (i, i) is kept whatever the predicate says (STRENGTH, and `lump` in any mode)
template <int MODE, bool DIAG>
__device__ __forceinline__ bool fl_keep(uint32_t i, uint32_t j, double a, const FilterArgs& f, const double* __restrict__ d) {
    if (DIAG && j == i) return true;
    if (MODE == SPMV_FILTER_BAND) {
        const int64_t k = (int64_t)j - (int64_t)i;
        return f.lo <= k && k <= f.hi;
    }
    if (MODE == SPMV_FILTER_ABS) return fabs(a) > f.theta;
    return a * a > f.tt * fabs(d[i] * d[j]);
}

template <typename I, int MODE, bool DIAG>
__global__ __launch_bounds__(FL_THREADS) void fl_judge_kernel(uint64_t M, uint64_t N, uint64_t NZ, const I* __restrict__ irp,
                                                             const uint32_t* __restrict__ ja, const double* __restrict__ as, FilterArgs f,
                                                             const double* __restrict__ d, uint64_t* __restrict__ mask,
                                                             uint32_t* __restrict__ counts, uint32_t* __restrict__ flag) {
    constexpr bool ROWS = MODE != SPMV_FILTER_ABS || DIAG;
    __shared__ uint32_t sIrp[ROWS ? FL_SLICE : 1], sEnds[2], sCnt[FL_WAVES];
    const uint64_t tile = linear_block(), p0 = tile * FL_TILE;
    if (p0 >= NZ) return;
    const uint64_t p1 = min(p0 + FL_TILE, NZ);
    TileRows t{};
    if (ROWS) t = fl_tile_rows(M, irp, p0, p1, sIrp, sEnds);
    const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    uint32_t kept = 0;
    for (uint32_t s = 0; s < FL_TILE / FL_THREADS; ++s) {
        const uint32_t q = s * FL_THREADS + threadIdx.x;
        const uint64_t p = p0 + q;
        bool keep = false;
        if (p < p1) {
            const uint32_t j = ja[p];
            if (j >= N) atomicOr(flag, 1u);
            else {
                const uint32_t i = ROWS ? fl_row(t, irp, sIrp, p, q) : 0u;
                const double a = MODE == SPMV_FILTER_BAND ? 0.0 : as[p];
                keep = fl_keep<MODE, DIAG>(i, j, a, f, d);
            }
        }
        const uint64_t bal = __ballot(keep);
        if (lane == 0) mask[tile * FL_WORDS + s * FL_WAVES + wave] = bal;
        kept += (uint32_t)__popcll(bal);
    }
    if (lane == 0) sCnt[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < FL_WAVES; ++w) sum += sCnt[w];
        counts[tile] = sum;
    }
}

// -------------------------------------------------------------------------------------------------------- the write
// the kept entries before entry p of A (p <= NZ; p = NZ: all of them)
__device__ __forceinline__ uint32_t fl_rank(uint64_t p, const uint64_t* __restrict__ mask, const uint32_t* __restrict__ tileBase) {
    const uint64_t tile = p / FL_TILE;
    const uint32_t q = (uint32_t)(p % FL_TILE), w = q / 64, b = q % 64;
    uint32_t r = tileBase[tile];                               // (nTiles + 1 words: p = NZ on a tile edge reads the total)
    for (uint32_t k = 0; k < w; ++k) r += (uint32_t)__popcll(mask[tile * FL_WORDS + k]);
    if (b) r += (uint32_t)__popcll(mask[tile * FL_WORDS + w] & ((1ull << b) - 1));
    return r;
}

__global__ __launch_bounds__(FL_THREADS) void fl_write_kernel(uint64_t NZ, const uint32_t* __restrict__ ja, const uint64_t* __restrict__ as,
                                                             const uint64_t* __restrict__ mask, const uint32_t* __restrict__ tileBase,
                                                             uint32_t nnzC, uint32_t* __restrict__ jaC, uint64_t* __restrict__ asC,
                                                             uint32_t* __restrict__ map) {
    __shared__ uint64_t sMask[FL_WORDS];
    __shared__ uint32_t sPre[FL_WORDS];
    const uint64_t tile = linear_block(), p0 = tile * FL_TILE;
    if (p0 >= NZ) return;
    if (threadIdx.x < FL_WORDS) sMask[threadIdx.x] = mask[tile * FL_WORDS + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < FL_WORDS) {
        uint32_t pre = tileBase[tile];
        for (uint32_t k = 0; k < threadIdx.x; ++k) pre += (uint32_t)__popcll(sMask[k]);
        sPre[threadIdx.x] = pre;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    for (uint32_t s = 0; s < FL_TILE / FL_THREADS; ++s) {
        const uint32_t w = s * FL_WAVES + wave;
        const uint64_t m = sMask[w], p = p0 + s * FL_THREADS + threadIdx.x;
        if (!((m >> lane) & 1) || p >= NZ) continue;
        const uint32_t at = sPre[w] + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (at >= nnzC) continue;                              // (never: the mask and its scan are one launch sequence)
        jaC[at] = ja[p];
        asC[at] = as[p];
        map[at] = (uint32_t)p;
    }
}

// IRP_C[i] = rank(IRP_A[i]), i in [0, M]
template <typename I>
__global__ __launch_bounds__(FL_THREADS) void fl_irp_kernel(uint64_t M, const I* __restrict__ irp, const uint64_t* __restrict__ mask,
                                                           const uint32_t* __restrict__ tileBase, uint32_t* __restrict__ irpC) {
    const uint64_t r = linear_block() * FL_THREADS + threadIdx.x;
    if (r <= M) irpC[r] = fl_rank(irp[r], mask, tileBase);
}

__global__ __launch_bounds__(FL_THREADS) void fl_diagc_kernel(uint64_t M, const uint32_t* __restrict__ dpos, const uint64_t* __restrict__ mask,
                                                             const uint32_t* __restrict__ tileBase, uint32_t* __restrict__ diagC) {
    const uint64_t r = linear_block() * FL_THREADS + threadIdx.x;
    if (r < M) diagC[r] = fl_rank(dpos[r], mask, tileBase);
}

// --------------------------------------------------------------------------------------------------------- the lump
__device__ __forceinline__ bool fl_kept(const uint64_t* __restrict__ mask, uint64_t p) { return (mask[p / 64] >> (p % 64)) & 1; }

// rows of at most FL_LONG entries, a lane each; at the build (longList set) the longer rows join the list, and *lumped
// grows by the rows with a dropped entry
template <typename I>
__global__ __launch_bounds__(FL_THREADS) void fl_lump_lane_kernel(uint64_t M, const I* __restrict__ irp, const double* __restrict__ as,
                                                                 const uint64_t* __restrict__ mask, const uint32_t* __restrict__ diagC,
                                                                 uint32_t nnzC, double* __restrict__ asC, uint32_t* __restrict__ longList,
                                                                 uint32_t* __restrict__ nLong, uint32_t* __restrict__ lumped) {
    const uint64_t r = linear_block() * FL_THREADS + threadIdx.x;
    bool isLong = false, any = false;
    if (r < M) {
        const uint64_t b = irp[r], e = irp[r + 1];
        isLong = e - b > FL_LONG;
        const uint32_t at = diagC[r];
        if (!isLong && at < nnzC) {
            double v = asC[at];                                // d_i: the write pass (or the refresh's gather) has put it there
            for (uint64_t p = b; p < e; ++p)
                if (!fl_kept(mask, p)) { v = v + as[p]; any = true; }
            if (any) asC[at] = v;
        }
    }
    if (!longList) return;
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t bl = __ballot(isLong), ba = __ballot(any);
    uint32_t base = 0;
    if (lane == 0 && bl) base = atomicAdd(nLong, (uint32_t)__popcll(bl));
    if (lane == 0 && ba) atomicAdd(lumped, (uint32_t)__popcll(ba));
    base = __shfl(base, 0);
    if (isLong) longList[base + __popcll(bl & ((1ull << lane) - 1))] = (uint32_t)r;
}

// the rows of `list`, a wavefront each: 64 entries per step, loaded coalesced; the dropped ones are added in stored order
template <typename I>
__global__ __launch_bounds__(FL_THREADS) void fl_lump_wave_kernel(uint32_t n, const uint32_t* __restrict__ list, const I* __restrict__ irp,
                                                                 const double* __restrict__ as, const uint64_t* __restrict__ mask,
                                                                 const uint32_t* __restrict__ diagC, uint32_t nnzC, double* __restrict__ asC,
                                                                 uint32_t* __restrict__ lumped) {
    const uint64_t k = linear_block() * FL_WAVES + threadIdx.x / 64;
    if (k >= n) return;                                        // uniform in a wavefront
    const uint32_t lane = threadIdx.x % 64, r = list[k], at = diagC[r];
    if (at >= nnzC) return;
    const uint64_t b = irp[r], e = irp[r + 1];
    double v = asC[at];
    bool any = false;
    for (uint64_t base = b; base < e; base += 64) {
        const uint64_t p = base + lane;
        const bool live = p < e;
        const double a = live ? as[p] : 0.0;
        uint64_t drop = __ballot(live && !fl_kept(mask, p));
        any |= drop != 0;
        while (drop) {                                         // uniform: every lane adds the same values in the same order
            const int src = __ffsll((unsigned long long)drop) - 1;
            v = v + __shfl(a, src);
            drop &= drop - 1;
        }
    }
    if (lane == 0 && any) {
        asC[at] = v;
        if (lumped) atomicAdd(lumped, 1u);
    }
}

int fail(hipStream_t st, const char* what) { return buildFail(st, "filter", what); }

template <typename I, int MODE>
void launchJudge(bool diag, dim3 grid, hipStream_t st, uint64_t M, uint64_t N, uint64_t NZ, const I* irp, const DevMat* a, const FilterArgs& f,
                 const double* d, uint64_t* mask, uint32_t* counts, uint32_t* flag) {
    if (diag) hipLaunchKernelGGL((fl_judge_kernel<I, MODE, true>), grid, dim3(FL_THREADS), 0, st, M, N, NZ, irp, a->JA, a->AS, f, d, mask, counts, flag);
    else hipLaunchKernelGGL((fl_judge_kernel<I, MODE, false>), grid, dim3(FL_THREADS), 0, st, M, N, NZ, irp, a->JA, a->AS, f, d, mask, counts, flag);
}

// the ordered sums into c's diagonal entries, over the mask and the lists that c's plan keeps (build: the lists are made here)
int lumpPass(const DevMat* a, DevMat* c, bool build, uint32_t* dCnt, TempTally* tm, hipStream_t st) {
    FilterPlan* pl = c->filt;
    const uint64_t M = a->M;
    const uint32_t nnzC = (uint32_t)c->NZ;
    TempBuf list(tm);
    if (build && list.alloc(std::min<uint64_t>(M, a->NZ / (FL_LONG + 1) + 1) * 4)) return fail(st, "temporary allocation (long rows)");
    uint32_t* const dList = build ? list.as<uint32_t>() : nullptr;     // (a long row has more than FL_LONG of the NZ entries)
    withIrp(a, [&](auto irp) {
        hipLaunchKernelGGL((fl_lump_lane_kernel<IrpT<decltype(irp)>>), gridFor(M), dim3(FL_THREADS), 0, st, M, irp, a->AS, pl->mask, pl->diagC, nnzC,
                           c->AS, dList, dCnt, dCnt ? dCnt + 1 : nullptr);
    });
    if (build) {
        uint32_t h[2] = {0, 0};
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, dCnt, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "lump pass");
        pl->nLong = h[0];
        if (pl->nLong) {
            if (devMalloc(&pl->longList, (size_t)pl->nLong * 4) != hipSuccess ||
                hipMemcpyAsync(pl->longList, list.p, (size_t)pl->nLong * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
                return fail(st, "allocation of the long rows");
        }
    }
    if (pl->nLong)
        withIrp(a, [&](auto irp) {
            hipLaunchKernelGGL((fl_lump_wave_kernel<IrpT<decltype(irp)>>), gridFor(pl->nLong, FL_WAVES), dim3(FL_THREADS), 0, st, pl->nLong, pl->longList,
                               irp, a->AS, pl->mask, pl->diagC, nnzC, c->AS, build ? dCnt + 1 : nullptr);
        });
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(st, "lump pass");
    return EXIT_SUCCESS;
}

}  // namespace

void freeFilterPlan(FilterPlan* p) {
    if (!p) return;
    (void)devFree(p->mask); (void)devFree(p->diagC); (void)devFree(p->longList);
    delete p;
}

const spmvFilterInfo* filterInfo(const DevMat* c) { return &c->filt->info; }
void filterSetMaxRow(DevMat* c) { c->filt->info.maxRowNnz = c->maxRowNnz; }

// c: kind, M and N set by the caller, nothing allocated.  On success c owns IRP (4 B), JA, AS, the map and the plan, and
// c->NZ is set; on failure the caller frees c with whatever it holds.  The STORED rule and a column id >= N are found
// before JA / AS exist.  o has been checked.
int filterBuild(const DevMat* a, const spmvFilterOpts* o, DevMat* c, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t M = a->M, N = a->N, NZ = a->NZ;
    FilterPlan* pl = c->filt = new FilterPlan;
    pl->opts = *o;
    const bool lump = o->lump != 0, diag = lump || o->mode == SPMV_FILTER_STRENGTH;
    const FilterArgs f{o->lo, o->hi, o->theta, o->theta * o->theta};
    spmvFilterInfo out{};
    out.nnzA = NZ;
    TempTally tm;
    const uint64_t nTiles = (NZ + FL_TILE - 1) / FL_TILE;
    const dim3 tiles = gridFor(nTiles, 1, FL_THREADS);
    if (devMalloc(&c->IRP, (M + 1) * 4) != hipSuccess) return fail(st, "allocation of the row pointers");
    c->irpBytes = 4;
    TempBuf cnt(&tm), dpos(&tm), dval(&tm), dcount(&tm), mask(&tm), counts(&tm), base(&tm), scanTmp(&tm);
    if (cnt.alloc(4 * 4)) return fail(st, "temporary allocation");
    uint32_t* const dCnt = cnt.as<uint32_t>();                 // [0] long rows, [1] lumped rows, [2] a column id out of range, [3] a bad row
    const uint32_t init[4] = {0, 0, 0, FL_NONE};
    if (hipMemcpyAsync(dCnt, init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return fail(st, "memset");
    // 1. the diagonal
    if (diag && M) {
        if (dpos.alloc(M * 4) || dcount.alloc(M * 4) || dval.alloc(M * 8)) return fail(st, "temporary allocation (16 B per row)");
        if (hipMemsetAsync(dcount.p, 0, M * 4, st) != hipSuccess || hipMemsetAsync(dpos.p, 0, M * 4, st) != hipSuccess) return fail(st, "memset");
        withIrp(a, [&](auto irp) {
            if (NZ) hipLaunchKernelGGL((fl_diag_kernel<IrpT<decltype(irp)>>), tiles, dim3(FL_THREADS), 0, st, M, NZ, irp, a->JA, dcount.as<uint32_t>(), dpos.as<uint32_t>());
        });
        hipLaunchKernelGGL(fl_dval_kernel, gridFor(M), dim3(FL_THREADS), 0, st, M, dcount.as<uint32_t>(), dpos.as<uint32_t>(), a->AS, dval.as<double>(), dCnt + 3);
        uint32_t bad = FL_NONE;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, dCnt + 3, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "the diagonal");
        if (bad != FL_NONE) {
            fprintf(stderr, "libspmvhip: filter: row %u does not hold exactly one stored diagonal entry\n", bad);
            return EXIT_FAILURE;
        }
        dcount.release();
    }
    // 2. judge, scan
    uint64_t nnzC = 0;
    if (NZ) {
        if (mask.alloc(nTiles * FL_WORDS * 8) || counts.alloc((nTiles + 1) * 4) || base.alloc((nTiles + 1) * 4))
            return fail(st, "temporary allocation (the keep mask)");
        if (hipMemsetAsync(counts.as<uint32_t>() + nTiles, 0, 4, st) != hipSuccess) return fail(st, "memset");
        withIrp(a, [&](auto irp) {
            using I = IrpT<decltype(irp)>;
            uint64_t* const m = mask.as<uint64_t>();
            uint32_t* const k = counts.as<uint32_t>();
            if (o->mode == SPMV_FILTER_BAND) launchJudge<I, SPMV_FILTER_BAND>(false, tiles, st, M, N, NZ, irp, a, f, nullptr, m, k, dCnt + 2);
            else if (o->mode == SPMV_FILTER_ABS) launchJudge<I, SPMV_FILTER_ABS>(lump, tiles, st, M, N, NZ, irp, a, f, nullptr, m, k, dCnt + 2);
            else launchJudge<I, SPMV_FILTER_STRENGTH>(true, tiles, st, M, N, NZ, irp, a, f, dval.as<double>(), m, k, dCnt + 2);
        });
        if (hipGetLastError() != hipSuccess) return fail(st, "judge pass");
        if (exclusiveScan(scanTmp, counts.as<uint32_t>(), base.as<uint32_t>(), 0u, (size_t)nTiles + 1, st) != hipSuccess) return fail(st, "scan");
        uint32_t total = 0, badCol = 0;
        if (hipMemcpyAsync(&total, base.as<uint32_t>() + nTiles, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(&badCol, dCnt + 2, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "judge pass");
        if (badCol) { fprintf(stderr, "libspmvhip: filter: a column id of the source is >= N\n"); return EXIT_FAILURE; }
        nnzC = total;
    }
    // 3. write
    c->NZ = nnzC;
    const size_t nz1 = std::max<uint64_t>(nnzC, 1);
    if (devMalloc(&c->JA, nz1 * 4) != hipSuccess || devMalloc(&c->AS, nz1 * 8) != hipSuccess || devMalloc(&c->tmap, nz1 * 4) != hipSuccess)
        return fail(st, "allocation of the filtered arrays");
    if (NZ) {
        hipLaunchKernelGGL(fl_write_kernel, tiles, dim3(FL_THREADS), 0, st, NZ, a->JA, reinterpret_cast<const uint64_t*>(a->AS), mask.as<uint64_t>(),
                           base.as<uint32_t>(), (uint32_t)nnzC, c->JA, reinterpret_cast<uint64_t*>(c->AS), c->tmap);
        withIrp(a, [&](auto irp) {
            hipLaunchKernelGGL((fl_irp_kernel<IrpT<decltype(irp)>>), gridFor(M + 1), dim3(FL_THREADS), 0, st, M, irp, mask.as<uint64_t>(), base.as<uint32_t>(),
                               static_cast<uint32_t*>(c->IRP));
        });
        if (hipGetLastError() != hipSuccess) return fail(st, "write pass");
    } else if (hipMemsetAsync(c->IRP, 0, (M + 1) * 4, st) != hipSuccess) {
        return fail(st, "row pointers");
    }
    // 4. lump: the mask stays with the handle
    if (lump && M && NZ) {
        if (devMalloc(&pl->diagC, M * 4) != hipSuccess) return fail(st, "allocation of the diagonal positions");
        hipLaunchKernelGGL(fl_diagc_kernel, gridFor(M), dim3(FL_THREADS), 0, st, M, dpos.as<uint32_t>(), mask.as<uint64_t>(), base.as<uint32_t>(), pl->diagC);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(st, "lump pass");
        out.tempBytes = tm.peak;
        pl->mask = mask.as<uint64_t>();                        // from here the plan owns it
        mask.p = nullptr; mask.n = 0;
        if (lumpPass(a, c, true, dCnt, &tm, st)) return EXIT_FAILURE;
        uint32_t lumped = 0;
        if (hipMemcpy(&lumped, dCnt + 1, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(st, "lump pass");
        out.lumpedRows = lumped;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail(st, "write pass");
    out.nnzC = nnzC;
    out.tempBytes = std::max<ulong>(out.tempBytes, tm.peak);
    out.ms = msSince(t0);
    pl->info = out;
    return EXIT_SUCCESS;
}

// after the gather of A's current values through the map: the ordered sums again, over the build's dropped places
int filterRefresh(DevMat* c, const DevMat* a, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    FilterPlan* pl = c->filt;
    TempTally tm;
    if (pl->opts.lump && pl->mask && lumpPass(a, c, false, nullptr, &tm, st)) return EXIT_FAILURE;
    pl->info.tempBytes = tm.peak;
    pl->info.ms = msSince(t0);
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
