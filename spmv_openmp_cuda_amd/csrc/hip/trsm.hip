// trsm.hip -- X = T^-1 B for a block of k right-hand sides on a device CSR handle (hipSpTRSMCSR).
// Column c of X has the bits of hipSpTRSVCSR on column c of B: rows in order, each row's strict-triangle products rounded
// and added in STORED order from +0.0, then (b - acc), divided by the stored diagonal unless the diagonal is unit.
//
// The schedule is the single solve's (TriSchedule of trsv.hip: perm, levelPtr, steps, split_h, diagPos), used unchanged,
// and so is the launch plan: one launch per wide level, one per run of thin levels -- whatever k is.  The columns are taken
// in panels of at most 16 (the convention of spmm.hip), and the panel is part of the grid: the linear workgroup id of a
// level launch is (block of the level) * panels + panel, the grid of a run launch is the number of panels.
//   * short rows of a level: a group of P adjacent lanes owns a row (P = the width of the widest panel rounded up to a
//     power of two), so a workgroup takes 256 / P rows of perm.  Lane c walks the row in stored order, TRSM_AHEAD entries'
//     gathers X(col, c) in flight and the adds kept in order.  Every lane of a group loads JA[p] / AS[p] from the same
//     address (one request per group in the load unit; no shuffle, no LDS); with row-major X the P gathers of an entry are
//     one contiguous segment, 128 B at P = 16.
//   * long rows (behind split_h[l]): a wavefront per row and panel, 64 / P entry slots x P columns.  A pass loads
//     TRSM_LONG_SUBS x 64 / P entries' products, then every lane adds its column's products in stored order, fetched by
//     shuffles from the slots that hold a strict-triangle entry (the same sum on every slot; slot 0 stores).
//   * runs of thin levels: one workgroup of 1 024 lanes per panel walks the run's levels, 1 024 / P rows at a time, with
//     the drain-and-barrier hand-off of trsv_run_kernel.  Panels never read each other's columns, so they need no order.
// Lanes whose column is past the panel's width load and store nothing.  A caller may hand a stop word (the block Krylov
// loops do): every launch that finds it set when it starts returns at once; hipSpTRSMCSR hands none.  No flags, tickets, spins or atomics: ordering
// across workgroups comes only from kernel boundaries on one stream, inside a run from the workgroup barrier.
#include <hip/hip_runtime.h>

#include "spmvHip.h"
#include "kernels.hpp"

namespace spmvhip {

namespace {

constexpr uint32_t TRSM_THREADS = 256;
constexpr uint32_t TRSM_RUN_THREADS = 1024;     // the workgroup of a run, as trsv_run_kernel's
constexpr uint32_t TRSM_PANEL = 16;             // columns per panel (the convention of section 15)
constexpr uint32_t TRSM_AHEAD = 8;              // gathers in flight per lane on a short row (TRI_AHEAD of trsv.hip)
constexpr uint32_t TRSM_LONG_SUBS = 4;          // sub-chunks of 64 / P entries in flight per pass of a long row

// the strict triangle, as trsv.hip has it: lower j < i, upper i < j < N
__device__ __forceinline__ bool trsm_in_tri(uint64_t j, uint64_t i, int upper, uint64_t N) {
    return upper ? (j > i && j < N) : j < i;
}

// what every kernel of this file is handed; B(i, c) at B[i*sbr + c*sbc], X(i, c) at X[i*ldx + c] (XROW) or X[c*ldx + i]
struct TrsmArgs {
    const uint32_t* perm;
    const uint32_t* JA;
    const double*   AS;
    const uint32_t* diagPos;
    const uint32_t* stop;                           // null, or a word that ends every launch at once when it is not 0
    const double*   B;
    double*         X;
    double   unitValue;
    uint64_t N, sbr, sbc, ldx;
    uint32_t k, panels;
    int      upper, dunit;
};

template <bool XROW>
__device__ __forceinline__ uint64_t x_at(uint64_t i, uint64_t c, uint64_t ldx) { return XROW ? i * ldx + c : c * ldx + i; }

// X(i, c) of row i on one lane: the products in stored order, TRSM_AHEAD gathers in flight, adds in order (an entry outside
// the triangle is skipped, never added as 0.0)
template <typename I, bool UVAL, bool XROW>
__device__ __forceinline__ void trsm_row(uint64_t i, uint64_t c, const I* __restrict__ IRP, const TrsmArgs& a) {
    const uint64_t s = IRP[i], e = IRP[i + 1];
    double acc = 0.0;
    for (uint64_t p = s; p < e; p += TRSM_AHEAD) {
        uint32_t col[TRSM_AHEAD];
        bool in[TRSM_AHEAD];
        double av[TRSM_AHEAD], xv[TRSM_AHEAD];
#pragma unroll
        for (uint32_t u = 0; u < TRSM_AHEAD; ++u) {
            in[u] = p + u < e;
            col[u] = in[u] ? stream_load(a.JA + p + u) : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < TRSM_AHEAD; ++u) {
            in[u] = in[u] && trsm_in_tri(col[u], i, a.upper, a.N);
            av[u] = in[u] ? value_at<UVAL>(a.AS, p + u, a.unitValue) : 0.0;
            xv[u] = in[u] ? a.X[x_at<XROW>(col[u], c, a.ldx)] : 0.0;
        }
#pragma unroll
        for (uint32_t u = 0; u < TRSM_AHEAD; ++u)
            if (in[u]) acc += av[u] * xv[u];
    }
    const double r = a.B[i * a.sbr + c * a.sbc] - acc;
    a.X[x_at<XROW>(i, c, a.ldx)] = a.dunit ? r : r / (UVAL ? a.unitValue : a.AS[a.diagPos[i]]);
}

// one level, every panel: workgroup (blk, panel) with blk < shortBlocks takes 256 / P short rows of
// perm[begin, begin + nShort), a group of P lanes per row; the others a long row per wavefront (perm[begin + nShort, + nLong))
template <typename I, bool UVAL, int P, bool XROW>
__global__ __launch_bounds__(TRSM_THREADS) void trsm_level_kernel(uint32_t begin, uint32_t nShort, uint32_t nLong,
                                                                  uint32_t shortBlocks, uint64_t nBlocks,
                                                                  const I* __restrict__ IRP, const TrsmArgs a) {
    static_assert(P >= 1 && P <= (int)TRSM_PANEL && (P & (P - 1)) == 0, "panel width");
    if (a.stop && *a.stop) return;                                       // a stopped block Krylov loop (krylov_block.hip)
    const uint64_t lin = linear_block();
    if (lin >= nBlocks * a.panels) return;                               // the fold of grid2d
    const uint64_t blk = lin / a.panels;
    const uint32_t c0 = (uint32_t)(lin % a.panels) * TRSM_PANEL;
    const uint32_t w = a.k - c0 < TRSM_PANEL ? a.k - c0 : TRSM_PANEL;    // this panel's width
    const uint32_t cl = threadIdx.x % P;
    const bool live = cl < w;                                            // lanes past the width load and store nothing
    const uint64_t c = c0 + cl;
    if (blk < shortBlocks) {
        const uint64_t t = blk * (TRSM_THREADS / P) + threadIdx.x / P;
        if (t >= nShort || !live) return;
        trsm_row<I, UVAL, XROW>(a.perm[begin + t], c, IRP, a);
        return;
    }
    const uint64_t wv = (blk - shortBlocks) * (TRSM_THREADS / WAVE) + threadIdx.x / WAVE;
    if (wv >= nLong) return;                                             // wave-uniform
    constexpr uint32_t S = WAVE / P;                                     // entry slots of a sub-chunk
    const uint32_t lane = threadIdx.x % WAVE, slot = lane / P;
    const uint64_t i = a.perm[begin + nShort + wv];
    const uint64_t s = IRP[i], e = IRP[i + 1];
    uint64_t slotBits = 0;                                               // lane 0 of every slot
#pragma unroll
    for (uint32_t q = 0; q < S; ++q) slotBits |= 1ull << (q * P);
    double acc = 0.0;
    for (uint64_t p = s; p < e; p += TRSM_LONG_SUBS * S) {
        uint32_t col[TRSM_LONG_SUBS];
        bool in[TRSM_LONG_SUBS];
        double v[TRSM_LONG_SUBS];
#pragma unroll
        for (uint32_t u = 0; u < TRSM_LONG_SUBS; ++u) {
            const uint64_t q = p + u * S + slot;
            in[u] = q < e;
            col[u] = in[u] ? stream_load(a.JA + q) : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < TRSM_LONG_SUBS; ++u) {
            const uint64_t q = p + u * S + slot;
            in[u] = in[u] && trsm_in_tri(col[u], i, a.upper, a.N);
            v[u] = in[u] && live ? value_at<UVAL>(a.AS, q, a.unitValue) * a.X[x_at<XROW>(col[u], c, a.ldx)] : 0.0;
        }
#pragma unroll
        for (uint32_t u = 0; u < TRSM_LONG_SUBS; ++u) {
            uint64_t mask = __ballot(in[u]) & slotBits;                  // uniform: the slots that hold a strict-triangle entry
            while (mask) {
                const int q = __ffsll((unsigned long long)mask) - 1;
                mask &= mask - 1;
                acc += __shfl(v[u], q + (int)cl, WAVE);                  // column cl of slot q / P
            }
        }
    }
    if (slot == 0 && live) {
        const double r = a.B[i * a.sbr + c * a.sbc] - acc;
        a.X[x_at<XROW>(i, c, a.ldx)] = a.dunit ? r : r / (UVAL ? a.unitValue : a.AS[a.diagPos[i]]);
    }
}

// levels [l0, l1), each of at most T short rows, one workgroup per panel: a group of P lanes per row, and between levels
// every wave's stores drained and a barrier (the waves of a workgroup share one CU and its L1), as trsv_run_kernel
template <typename I, bool UVAL, int P, bool XROW>
__global__ __launch_bounds__(TRSM_RUN_THREADS) void trsm_run_kernel(uint32_t l0, uint32_t l1,
                                                                    const uint32_t* __restrict__ levelPtr,
                                                                    const I* __restrict__ IRP, const TrsmArgs a) {
    static_assert(P >= 1 && P <= (int)TRSM_PANEL && (P & (P - 1)) == 0, "panel width");
    if (a.stop && *a.stop) return;                                       // workgroup-uniform, as the next line: in front of every barrier
    const uint64_t panel = linear_block();
    if (panel >= a.panels) return;
    const uint32_t c0 = (uint32_t)panel * TRSM_PANEL;
    const uint32_t w = a.k - c0 < TRSM_PANEL ? a.k - c0 : TRSM_PANEL;
    const uint32_t cl = threadIdx.x % P, g = threadIdx.x / P;
    const bool live = cl < w;
    const uint64_t c = c0 + cl;
    for (uint32_t l = l0; l < l1; ++l) {
        const uint32_t s = levelPtr[l], e = levelPtr[l + 1];
        if (live)
            for (uint32_t t = s + g; t < e; t += TRSM_RUN_THREADS / P) trsm_row<I, UVAL, XROW>(a.perm[t], c, IRP, a);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

template <typename I, bool UVAL, int P, bool XROW>
void launchSteps(const DevMat* d, const TriSchedule* s, const TrsmArgs& a, hipStream_t st, dim3* lastGrid, dim3* lastBlock) {
    const I* IRP = static_cast<const I*>(d->IRP);
    for (const TriSchedule::Step& step : s->steps) {
        if (step.l1 - step.l0 > 1) {
            const dim3 grid = grid2d(a.panels, TRSM_RUN_THREADS);
            hipLaunchKernelGGL((trsm_run_kernel<I, UVAL, P, XROW>), grid, dim3(TRSM_RUN_THREADS), 0, st, step.l0, step.l1,
                               s->levelPtr, IRP, a);
            *lastGrid = grid; *lastBlock = dim3(TRSM_RUN_THREADS);
            continue;
        }
        const uint32_t l = step.l0, begin = s->levelPtr_h[l], split = s->split_h[l], end = s->levelPtr_h[l + 1];
        const uint32_t nShort = split - begin, nLong = end - split;
        constexpr uint32_t rowsPerBlock = TRSM_THREADS / P;
        const uint32_t shortBlocks = (nShort + rowsPerBlock - 1) / rowsPerBlock;
        const uint32_t longBlocks = (nLong + TRSM_THREADS / WAVE - 1) / (TRSM_THREADS / WAVE);
        const uint64_t nBlocks = (uint64_t)shortBlocks + longBlocks;
        const dim3 grid = grid2d(nBlocks * a.panels, TRSM_THREADS);
        hipLaunchKernelGGL((trsm_level_kernel<I, UVAL, P, XROW>), grid, dim3(TRSM_THREADS), 0, st, begin, nShort, nLong,
                           shortBlocks, nBlocks, IRP, a);
        *lastGrid = grid; *lastBlock = dim3(TRSM_THREADS);
    }
}

template <typename I, bool UVAL, int P>
void launchLayout(const DevMat* d, const TriSchedule* s, const TrsmArgs& a, bool xRowMajor, hipStream_t st, dim3* g, dim3* b) {
    if (xRowMajor) launchSteps<I, UVAL, P, true>(d, s, a, st, g, b);
    else           launchSteps<I, UVAL, P, false>(d, s, a, st, g, b);
}

template <typename I, bool UVAL>
void launchWidth(const DevMat* d, const TriSchedule* s, const TrsmArgs& a, bool xRowMajor, hipStream_t st, dim3* g, dim3* b) {
    const uint32_t w = a.k < TRSM_PANEL ? a.k : TRSM_PANEL;              // the widest panel
    if (w == 1)      launchLayout<I, UVAL, 1>(d, s, a, xRowMajor, st, g, b);
    else if (w == 2) launchLayout<I, UVAL, 2>(d, s, a, xRowMajor, st, g, b);
    else if (w <= 4) launchLayout<I, UVAL, 4>(d, s, a, xRowMajor, st, g, b);
    else if (w <= 8) launchLayout<I, UVAL, 8>(d, s, a, xRowMajor, st, g, b);
    else             launchLayout<I, UVAL, 16>(d, s, a, xRowMajor, st, g, b);
}

}  // namespace

int enqueueTrsm(const DevMat* d, int uplo, int diag, uint32_t k, const Dense& B, const Dense& X, hipStream_t st, dim3* grid,
                dim3* block, const uint32_t* stop) {
    const TriSchedule* s = d->tri[uplo];
    TrsmArgs a;
    a.perm = s->perm; a.JA = d->JA; a.AS = d->AS; a.diagPos = s->diagPos; a.stop = stop; a.B = B.p; a.X = X.p;
    a.unitValue = d->unitValue;
    a.N = d->N; a.sbr = B.sr(); a.sbc = B.sc(); a.ldx = X.ld;
    a.k = k; a.panels = k / TRSM_PANEL + (k % TRSM_PANEL != 0);
    a.upper = uplo == SPMV_TRI_UPPER; a.dunit = diag == SPMV_DIAG_UNIT;
    withIrp(d, [&](auto irp) {
        if (d->unit) launchWidth<IrpT<decltype(irp)>, true>(d, s, a, X.rowMajor, st, grid, block);
        else         launchWidth<IrpT<decltype(irp)>, false>(d, s, a, X.rowMajor, st, grid, block);
    });
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

}  // namespace spmvhip
