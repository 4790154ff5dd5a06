// fsai.hip -- the factorised sparse approximate inverse G of a square device CSR handle, G^T G ~ A^-1 (spmvHipFsaiSetup,
// spmvHipFsaiRefresh; contract in spmvHip.h).  Row i of G stores the columns P = (p_0 < ... < p_{n-1} = i)
// -- the columns j < i of row i of the pattern, then i -- and its values are the last row of the inverse of the dense block
// A(P, P), scaled to a unit diagonal of G A G^T: the loop of spmvHip.h, in IEEE double with no FMA.
//
// Pass 1 (fsai_count_kernel, the shared scan, fsai_fill_kernel): n_i by one binary search per pattern row, the row
// pointers from the 64-bit scan, the columns copied; the first row with n_i > SPMV_FSAI_MAX_ROW by atomicMin.
//
// Pass 2 (fsai_rows_kernel), one row, one group of G lanes (G = 4, 16 or 64) inside ONE wavefront.  The group holds the
// lower triangle of B = A(P, P) packed BY COLUMNS in LDS (n (n + 1) / 2 doubles; column t at t (2n - t + 1) / 2, its
// entries s = t .. n-1 consecutive), and walks the loop's steps in program order:
//   gather   the (s, t) pairs dealt over the lanes; each is a binary search for column p_t in row p_s of A, +0.0 when absent.
//            Only t <= s is asked for: no value right of A's diagonal is ever read.
//   step k   every lane reads the pivot and takes its square root (the same bits on each; lane 0 stores it); the column
//            below it is divided, split over s; then the trailing triangle's entries -- which are the tail of the packed
//            array, so entry e of the step sits at base + e -- are dealt over the lanes, each subtracting the rounded
//            product B[s][k] * B[t][k].  Consecutive lanes take consecutive s of one column: B[s][t] and B[s][k] are
//            consecutive doubles and B[t][k] is one address (a broadcast), so the step has no LDS bank conflict.
//   back     right-looking too: once y[s] is final, lane t adds B[s][t] * y[s] to acc[t].  acc[t] (and then y[t]) lives in
//            the cell of B[n-1][t], which the substitution reads only in its first step (s = n-1) -- that step writes
//            acc[t] = +0.0 + B[n-1][t] * y[n-1] into it.  So every acc[t] gets its terms in descending s.
//   write    g[t] = y[t] / sqrt(y[n-1]), once.  A row whose pivot or whose y[n-1] fails the test gets the identity row and
//            is counted (atomicAdd) and named (atomicMin).
// Each entry of B is written by one lane per step, and between the parts of a step every lane waits for its memory
// operations (one wavefront: the hand-off needs nothing more, as in ilu0.hip).  So the bits are the loop's whatever G is.
// No flags, tickets, spins or cross-workgroup ordering: rows are independent.
//
// Where a row lives: a wavefront has `budget` doubles of LDS (at least the triangle of the longest row, at most that of a
// 64-entry row: 2080 doubles).  Its 64 / G groups are packed into that span greedily, in lane order; what does not fit goes
// to a next round of the same wavefront (a wave-uniform count), so a narrow group meeting long rows still works, in turns.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {
namespace {

constexpr uint32_t FSAI_THREADS = 128;          // two wavefronts: at most 2 x 16 640 B of LDS per workgroup
constexpr uint32_t FSAI_WAVE_MAX = SPMV_FSAI_MAX_ROW * (SPMV_FSAI_MAX_ROW + 1) / 2;     // 2080 doubles: a 64-entry row
constexpr uint32_t FSAI_FILL_LANES = 8;         // lanes that copy one row's columns
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;

// every memory operation of this lane complete, and no compiler motion across: the hand-off between the parts of a step
__device__ __forceinline__ void step_wait() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ uint32_t tri(uint32_t n) { return n * (n + 1) / 2; }
// where column t of the packed triangle of order n starts (its entry (t, t))
__device__ __forceinline__ uint32_t col_start(uint32_t n, uint32_t t) { return t * (2 * n - t + 1) / 2; }

// entry e of the by-columns packed lower triangle of order m is (row a, column b), b <= a < m.  Counted from the end the
// same entry is entry f of a by-rows packed triangle, whose row is the integer root of a triangular number (f <= 2079:
// single precision finds it to within one).
__device__ __forceinline__ void unpack(uint32_t m, uint32_t e, uint32_t& a, uint32_t& b) {
    const uint32_t f = tri(m) - 1 - e;
    uint32_t r = (uint32_t)((sqrtf(8.0f * (float)f + 1.0f) - 1.0f) * 0.5f);
    while (tri(r) > f) --r;
    while (tri(r + 1) <= f) ++r;
    const uint32_t c = f - tri(r);
    b = m - 1 - r;
    a = m - 1 - c;
}

// row `row` of G on lane g of its group: n columns at P[0, n), values to out[0, n), the triangle in B (LDS, tri(n) doubles)
template <uint32_t G, typename I>
__device__ __forceinline__ void fsai_row(uint32_t g, uint32_t row, uint32_t n, double* B, const I* __restrict__ IRPa,
                                         const uint32_t* __restrict__ JAa, const double* __restrict__ ASa,
                                         const uint32_t* __restrict__ P, double* __restrict__ out, uint32_t* words) {
    const uint32_t T = tri(n);
    for (uint32_t e = g; e < T; e += G) {                                // gather: entry e is (s, t), t <= s
        uint32_t s, t;
        unpack(n, e, s, t);
        const uint32_t ps = P[s], pt = P[t];
        const I end = IRPa[ps + 1];
        I lo = IRPa[ps], hi = end;
        while (lo < hi) {                                                // the first of row p_s's columns >= p_t
            const I mid = lo + (hi - lo) / 2;
            if (JAa[mid] < pt) lo = mid + 1; else hi = mid;
        }
        B[e] = lo < end && JAa[lo] == pt ? ASa[lo] : 0.0;
    }
    step_wait();
    bool bad = false;
    uint32_t colk = 0;                                                   // where column k starts
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t m = n - 1 - k;                                    // rows below the pivot
        const double p = B[colk];
        if (!(p > 0.0) || p == INFINITY) { bad = true; break; }          // (the same on every lane of the group)
        const double d = sqrt(p);
        for (uint32_t a = g; a < m; a += G) B[colk + 1 + a] = B[colk + 1 + a] / d;
        if (g == 0) B[colk] = d;
        step_wait();
        const uint32_t base = colk + 1 + m;                              // column k + 1: the trailing triangle, of order m
        for (uint32_t e = g; e < tri(m); e += G) {
            uint32_t a, b;
            unpack(m, e, a, b);                                          // s = k + 1 + a, t = k + 1 + b
            const double prod = B[colk + 1 + a] * B[colk + 1 + b];
            B[base + e] = B[base + e] - prod;
        }
        step_wait();
        colk = base;
    }
    double ylast = 0.0;
    if (!bad) {                                                          // y[t] in the cell of B[n-1][t]: the last of column t
        const double dn = B[T - 1];
        double ys = ylast = (1.0 / dn) / dn;
        if (g == 0) B[T - 1] = ys;
        for (uint32_t s = n - 1; s >= 1; --s) {
            for (uint32_t t = g; t < s; t += G) {
                const uint32_t c = col_start(n, t), cell = c + (n - 1 - t);
                const double acc = s == n - 1 ? 0.0 : B[cell];
                const double prod = B[c + (s - t)] * ys;
                B[cell] = acc + prod;
            }
            step_wait();
            const uint32_t c = col_start(n, s - 1), cell = c + (n - s);
            ys = (0.0 - B[cell]) / B[c];
            if (g == 0) B[cell] = ys;                                    // (after every lane's read: one wavefront, in order)
        }
        step_wait();
        const double d = sqrt(ylast);
        if (!(d > 0.0) || d == INFINITY) bad = true;
        else
            for (uint32_t t = g; t < n; t += G) out[t] = B[col_start(n, t) + (n - 1 - t)] / d;
    }
    if (bad) {
        for (uint32_t t = g; t < n; t += G) out[t] = t == n - 1 ? 1.0 : 0.0;
        if (g == 0) {
            atomicMin(words, row);
            atomicAdd(words + 1, 1u);
        }
    }
}

// G lanes per row, 64 / G rows per wavefront; words[0] the first BAD row, words[1] their count
template <uint32_t G, typename I>
__global__ __launch_bounds__(FSAI_THREADS) void fsai_rows_kernel(uint32_t M, uint32_t budget, const I* __restrict__ IRPa,
                                                                 const uint32_t* __restrict__ JAa, const double* __restrict__ ASa,
                                                                 const uint32_t* __restrict__ IRPg, const uint32_t* __restrict__ JAg,
                                                                 double* __restrict__ ASg, uint32_t* words) {
    extern __shared__ double fsaiLds[];
    const uint32_t lane = threadIdx.x % WAVE, g = lane % G, h = lane / G;
    const uint64_t r = (linear_block() * FSAI_THREADS + threadIdx.x) / G;
    uint32_t o = 0, n = 0;
    if (r < M) {
        o = IRPg[r];
        n = IRPg[r + 1] - o;
        if (tri(n) > budget) n = 0;                                      // (never: the setup refuses a longer row)
    }
    uint32_t cur = 0, round = 0, off = 0, mine = 0;                      // the groups packed into the wave's span, in lane order
#pragma unroll
    for (uint32_t q = 0; q < WAVE / G; ++q) {
        const uint32_t len = tri((uint32_t)__shfl((int)n, (int)(q * G), WAVE));
        if (cur + len > budget) { ++round; cur = 0; }
        if (q == h) { off = cur; mine = round; }
        cur += len;
    }
    double* const B = fsaiLds + (threadIdx.x / WAVE) * budget + off;
    for (uint32_t t = 0; t <= round; ++t) {                              // (wave-uniform)
        if (n && mine == t) fsai_row<G, I>(g, (uint32_t)r, n, B, IRPa, JAa, ASa, JAg + o, ASg + o, words);
        step_wait();
    }
}

// n_i = 1 + the columns j < i that row i of the pattern stores (strictly ascending rows); cnt[M] = 0
template <typename I>
__global__ __launch_bounds__(WG_THREADS) void fsai_count_kernel(uint32_t M, const I* __restrict__ IRPs, const uint32_t* __restrict__ JAs,
                                                                uint32_t* __restrict__ cnt, uint32_t* __restrict__ firstLong) {
    const uint64_t i = linear_block() * WG_THREADS + threadIdx.x;
    if (i > M) return;
    if (i == M) { cnt[M] = 0; return; }
    const I b = IRPs[i];
    I lo = b, hi = IRPs[i + 1];
    while (lo < hi) {
        const I mid = lo + (hi - lo) / 2;
        if (JAs[mid] < (uint32_t)i) lo = mid + 1; else hi = mid;
    }
    const uint64_t n = (uint64_t)(lo - b) + 1;
    cnt[i] = (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull);
    if (n > SPMV_FSAI_MAX_ROW) atomicMin(firstLong, (uint32_t)i);
}

// row i of G: the first n_i - 1 columns of row i of the pattern, then i
template <typename I>
__global__ __launch_bounds__(WG_THREADS) void fsai_fill_kernel(uint32_t M, const I* __restrict__ IRPs, const uint32_t* __restrict__ JAs,
                                                               const uint32_t* __restrict__ IRPg, uint32_t* __restrict__ JAg) {
    const uint64_t i = (linear_block() * WG_THREADS + threadIdx.x) / FSAI_FILL_LANES;
    const uint32_t g = threadIdx.x % FSAI_FILL_LANES;
    if (i >= M) return;
    const uint32_t o = IRPg[i], n = IRPg[i + 1] - o;
    const I b = IRPs[i];
    for (uint32_t j = g; j + 1 < n; j += FSAI_FILL_LANES) JAg[o + j] = JAs[b + j];
    if (g == 0) JAg[o + n - 1] = (uint32_t)i;
}

template <uint32_t G>
void launchRows(const DevMat* a, const DevMat* g, uint32_t budget, uint32_t* words, hipStream_t st) {
    const uint64_t blocks = (g->M * G + FSAI_THREADS - 1) / FSAI_THREADS;
    const size_t lds = (size_t)(FSAI_THREADS / WAVE) * budget * sizeof(double);
    withIrp(a, [&](auto irp) {
        hipLaunchKernelGGL((fsai_rows_kernel<G, IrpT<decltype(irp)>>), grid2d(blocks, FSAI_THREADS), dim3(FSAI_THREADS), lds, st, (uint32_t)g->M,
                           budget, irp, a->JA, a->AS, static_cast<const uint32_t*>(g->IRP), g->JA, g->AS, words);
    });
}

}  // namespace

uint32_t fsaiLanes(uint32_t forced, uint64_t M, uint64_t nnz) {
    if (forced) return forced;
    const uint64_t mean = M ? (nnz + M - 1) / M : 0;                     // (the choice)
    return mean <= 6 ? 4 : mean <= 24 ? 16 : 64;
}

int fsaiValues(const DevMat* a, DevMat* g, uint32_t lanes, uint32_t maxRow, spmvFsaiInfo* info, hipStream_t st) {
    info->badRows = 0;
    info->firstBadRow = -1;
    if (g->M == 0) return EXIT_SUCCESS;
    TempBuf words;
    uint32_t h[2] = {NO_ROW, 0};
    if (words.alloc(8) != hipSuccess) return buildFail(st, "fsai", "allocation of the row report");
    uint32_t* const w = words.as<uint32_t>();
    if (hipMemcpyAsync(w, h, 8, hipMemcpyHostToDevice, st) != hipSuccess) return buildFail(st, "fsai", "the row report");
    const uint32_t G = fsaiLanes(lanes, g->M, g->NZ);
    const uint32_t one = std::max<uint32_t>(maxRow * (maxRow + 1) / 2, 1);
    const uint32_t budget = std::min<uint32_t>(one * (WAVE / G), std::max(one, FSAI_WAVE_MAX));
    if (G == 64)      launchRows<64>(a, g, budget, w, st);
    else if (G == 16) launchRows<16>(a, g, budget, w, st);
    else              launchRows<4>(a, g, budget, w, st);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, w, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return buildFail(st, "fsai", "fsai_rows_kernel");
    info->badRows = h[1];
    info->firstBadRow = h[0] == NO_ROW ? -1 : (long)h[0];
    ++info->launches;
    return EXIT_SUCCESS;
}

// g: kind, M and N set by the caller, nothing allocated.  On success g owns IRP (4 B), JA and AS, and g->NZ is set; on
// failure the caller frees g with whatever it holds.  *longRow >= 0: a pattern row above SPMV_FSAI_MAX_ROW (nothing printed).
int fsaiBuild(const DevMat* a, const DevMat* s, DevMat* g, uint32_t lanes, spmvFsaiInfo* info, long* longRow, hipStream_t st) {
    const uint64_t M = a->M;
    *longRow = -1;
    g->irpBytes = 4;
    if (devMalloc(&g->IRP, (M + 1) * 4) != hipSuccess) return buildFail(st, "fsai", "allocation of the row pointers");
    uint64_t nnz = 0;
    uint32_t h[2] = {NO_ROW, 0};                                         // [0] the first over-long row, [1] the longest row
    if (M) {
        TempBuf cnt, irp64, scanTmp, words;
        if (cnt.alloc((M + 1) * 4) != hipSuccess || irp64.alloc((M + 1) * 8) != hipSuccess || words.alloc(8) != hipSuccess)
            return buildFail(st, "fsai", "temporary allocation (12 B per row)");
        uint32_t* const w = words.as<uint32_t>();
        if (hipMemcpyAsync(w, h, 8, hipMemcpyHostToDevice, st) != hipSuccess) return buildFail(st, "fsai", "the row report");
        withIrp(s, [&](auto irp) {
            hipLaunchKernelGGL((fsai_count_kernel<IrpT<decltype(irp)>>), gridFor(M + 1), dim3(WG_THREADS), 0, st, (uint32_t)M, irp, s->JA,
                               cnt.as<uint32_t>(), w);
        });
        if (hipGetLastError() != hipSuccess) return buildFail(st, "fsai", "fsai_count_kernel");
        if (exclusiveScan(scanTmp, cnt.as<uint32_t>(), irp64.as<uint64_t>(), (uint64_t)0, (size_t)M + 1, st) != hipSuccess)
            return buildFail(st, "fsai", "scan");
        if (hipMemcpyAsync(&nnz, irp64.as<uint64_t>() + M, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(h, w, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return buildFail(st, "fsai", "row pointers");
        if (h[0] != NO_ROW) { *longRow = (long)h[0]; return EXIT_FAILURE; }
        if (nnz >= IRP32_LIMIT) {
            fprintf(stderr, "libspmvhip: fsai: nnz(G) = %lu: the row pointers of the factor are 32-bit (limit %lu)\n", (unsigned long)nnz,
                    (unsigned long)IRP32_LIMIT);
            return EXIT_FAILURE;
        }
        enqueueNarrowIrp(M, irp64.as<uint64_t>(), static_cast<uint32_t*>(g->IRP), w + 1, st);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, w, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return buildFail(st, "fsai", "row pointers");
        info->launches += 3;                                             // count, fill, narrow (the scan's own are rocPRIM's)
    } else if (hipMemsetAsync(g->IRP, 0, 4, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        return buildFail(st, "fsai", "row pointers");
    }
    g->NZ = nnz;
    info->nnz = nnz;
    info->maxRow = h[1];
    if (devMalloc(&g->JA, std::max<uint64_t>(nnz, 1) * 4) != hipSuccess || devMalloc(&g->AS, std::max<uint64_t>(nnz, 1) * 8) != hipSuccess)
        return buildFail(st, "fsai", "allocation of the factor's arrays");
    if (M) {
        withIrp(s, [&](auto irp) {
            hipLaunchKernelGGL((fsai_fill_kernel<IrpT<decltype(irp)>>), gridFor(M * FSAI_FILL_LANES), dim3(WG_THREADS), 0, st, (uint32_t)M, irp, s->JA,
                               static_cast<const uint32_t*>(g->IRP), g->JA);
        });
        if (hipGetLastError() != hipSuccess) return buildFail(st, "fsai", "fsai_fill_kernel");
    }
    return fsaiValues(a, g, lanes, h[1], info, st);
}

}  // namespace spmvhip
