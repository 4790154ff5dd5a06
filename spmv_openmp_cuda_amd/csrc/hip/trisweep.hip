// trisweep.hip -- triangular solves by Jacobi sweeps on a device CSR handle (hipSpTRSVSweepsCSR, hipSpTRSMSweepsCSR,
// spmvHipTriSweepsPrepare, spmvHipTriSetApply, spmvHipTriSweepsInfo; contract in spmvHip.h, design in DESIGN.md section 40).
// x(0) = b (UNIT) or b / d (STORED); sweep s computes every row of x(s) from x(s-1) alone: the row's strict-triangle products
// rounded and added in STORED order from +0.0, then (b - acc), divided by the stored diagonal unless the diagonal is unit.
// Rows do not depend on each other inside a sweep, so a sweep is ONE launch and needs no level sets.
//
// Plan (TriSweepPlan, kept on the handle): diagPos and the first row without exactly one diagonal entry, whether every row
// ascends strictly with one diagonal, and two M x width iterates.  The row blocks are the handle's own (blkInfo / blkBase of
// the LDS-stream SpMV kernel: consecutive rows whose entries are one span of at most STREAM_NNZ, a longer row a block of its
// own).  Values are read live: nothing here is rebuilt when AS changes.
// Kernels, 256 lanes, one workgroup per row block:
//   trisweep_kernel        one vector.  The span's columns and values and the block's row pointers are loaded together,
//                          coalesced, with the streaming loads; the row lanes paint each entry's row into LDS; x(s-1) is
//                          gathered for in-triangle entries only and the rounded product parked in LDS, an entry outside the
//                          triangle marked; then one lane per row adds the marked-in products in stored order from +0.0 and
//                          stores (b - acc) [/ d].  A row longer than the span: its chunks' products in parallel into LDS,
//                          lane 0 adds them in order across the chunks.
//   trisweep_block_kernel  k columns in panels of at most 16, the panel part of the grid as in trsm.hip (so the launch
//                          count does not depend on k).  The span's columns and values are staged in LDS once per panel; a
//                          group of P lanes owns a row and lane c walks the row's LDS segment in stored order, SW_AHEAD
//                          gathers of X(s-1)(j, c) in flight and the adds kept in order.
//   trisweep_x0_kernel     x(0) = b / d (or a copy) where a sweep cannot read b itself.
// Every kernel returns at once when *stop != 0 (a stopped Krylov loop).
#include <hip/hip_runtime.h>

#include "lib.hpp"

namespace spmvhip {

void freeTriSweeps(TriSweepPlan* p) {
    if (!p) return;
    (void)devFree(p->diagPos); (void)devFree(p->ws);
    delete p;
}

namespace {

constexpr uint32_t SW_THREADS = WG_THREADS;
constexpr uint32_t SW_SPAN = STREAM_NNZ;
constexpr uint32_t SW_UNROLL = SW_SPAN / SW_THREADS;
constexpr uint32_t SW_PANEL = 16;               // columns per panel (the convention of spmm.hip and trsm.hip)
constexpr uint32_t SW_AHEAD = 8;                // gathers in flight per lane of the block kernel
constexpr uint16_t SW_OUT = 0xFFFF;             // mark of an entry outside the strict triangle (a block has at most 512 rows)
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;

// the strict triangle, as trsv.hip has it: lower j < i, upper i < j < N
__device__ __forceinline__ bool sw_in_tri(uint64_t j, uint64_t i, int upper, uint64_t N) {
    return upper ? (j > i && j < N) : j < i;
}

// what every kernel of this file is handed.  Element (i, c): prev[i*psr + c*psc], b[i*bsr + c*bsc], out[i*osr + c*osc],
// scaled[i*ssr + c] (null: not written; else out / d, the x(0) of a STORED solve on out)
struct SweepArgs {
    const uint4*    blkInfo;
    const uint64_t* blkBase;
    const uint32_t* JA;
    const double*   AS;
    const uint32_t* diagPos;
    const uint32_t* stop;
    const double*   prev;
    const double*   b;
    double*         out;
    double*         scaled;
    double   unitValue;
    uint64_t N, psr, psc, bsr, bsc, osr, osc, ssr;
    uint32_t nBlk, nLong, k, panels;
    int      upper, dunit;
};

// the epilogue of row i, column c.  b is read before out is written, by the same lane: b == out is allowed
template <bool UVAL>
__device__ __forceinline__ void sw_store(const SweepArgs& a, uint64_t i, uint64_t c, double acc) {
    const double r = a.b[i * a.bsr + c * a.bsc] - acc;
    const double dv = (!a.dunit || a.scaled) ? (UVAL ? a.unitValue : a.AS[a.diagPos[i]]) : 1.0;
    const double v = a.dunit ? r : r / dv;
    a.out[i * a.osr + c * a.osc] = v;
    if (a.scaled) a.scaled[i * a.ssr + c] = v / dv;
}

// ------------------------------------------------------------------------------------------------ plan
// one lane per row: the position of its diagonal, the first row without exactly one, the first row that does not ascend strictly
template <typename I>
__global__ __launch_bounds__(SW_THREADS) void trisweep_diag_kernel(uint64_t M, const I* __restrict__ IRP,
                                                                   const uint32_t* __restrict__ JA, uint32_t* __restrict__ diagPos,
                                                                   uint32_t* __restrict__ flags) {
    const uint64_t i = linear_block() * SW_THREADS + threadIdx.x;
    if (i >= M) return;
    const uint64_t s = IRP[i], e = IRP[i + 1];
    uint32_t nd = 0, dp = 0, last = 0;
    bool asc = true;
    for (uint64_t p = s; p < e; ++p) {
        const uint32_t j = JA[p];
        if (j == i) { ++nd; dp = (uint32_t)p; }
        if (p > s && j <= last) asc = false;
        last = j;
    }
    diagPos[i] = nd == 1 ? dp : 0u;
    if (nd != 1) atomicMin(&flags[0], (uint32_t)i);
    if (!asc) atomicMin(&flags[1], (uint32_t)i);
}

// ------------------------------------------------------------------------------------------------ kernels
template <bool UVAL>
__global__ __launch_bounds__(SW_THREADS) void trisweep_x0_kernel(uint64_t M, const SweepArgs a) {
    if (a.stop && *a.stop) return;
    const uint64_t idx = linear_block() * SW_THREADS + threadIdx.x;
    if (idx >= M * a.k) return;
    const uint64_t i = idx / a.k, c = idx % a.k;
    const double v = a.b[i * a.bsr + c * a.bsc];
    a.out[i * a.osr + c * a.osc] = a.dunit ? v : v / (UVAL ? a.unitValue : a.AS[a.diagPos[i]]);
}

template <typename I, bool UVAL>
__global__ __launch_bounds__(SW_THREADS) void trisweep_kernel(const I* __restrict__ IRP, const SweepArgs a) {
    __shared__ double   prod[SW_SPAN];
    __shared__ uint16_t mark[SW_SPAN];          // the entry's row in the block, then SW_OUT where it is outside the triangle
    __shared__ uint16_t rowOff[STREAM2_MAX_ROWS + 1];

    if (a.stop && *a.stop) return;               // workgroup-uniform, as the next line: in front of every barrier
    if (linear_block() >= a.nBlk) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t blk = stream2_block(linear_block(), a.nBlk, a.nLong);
    const uint4 info = a.blkInfo[blk];
    const uint32_t r0 = info.x, R = info.y, n = info.z;
    const uint64_t base = a.blkBase[blk];

    if (info.w) {
        // ---- a single row of n > SW_SPAN entries: chunk products in parallel, added in order by lane 0
        const uint64_t end = base + n;
        double acc = 0.0;
        for (uint64_t c = base; c < end; c += SW_SPAN) {
            const uint32_t cn = (uint32_t)(end - c < (uint64_t)SW_SPAN ? end - c : (uint64_t)SW_SPAN);
#pragma unroll
            for (uint32_t u = 0; u < SW_UNROLL; ++u) {
                const uint32_t k = tid + u * SW_THREADS;
                if (k < cn) {
                    const uint32_t j = stream_load(a.JA + c + k);
                    const bool in = sw_in_tri(j, r0, a.upper, a.N);
                    mark[k] = in ? (uint16_t)0 : SW_OUT;
                    if (in) prod[k] = value_at<UVAL>(a.AS, c + k, a.unitValue) * a.prev[j];
                }
            }
            __syncthreads();
            if (tid == 0)
                for (uint32_t j = 0; j < cn; ++j)
                    if (mark[j] != SW_OUT) acc += prod[j];
            __syncthreads();
        }
        if (tid == 0) sw_store<UVAL>(a, r0, 0, acc);
        return;
    }

    // ---- 1. the span and the row pointers in flight together
    uint32_t col[SW_UNROLL];
    double   val[SW_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < SW_UNROLL; ++u) {
        const uint32_t k = tid + u * SW_THREADS;
        const bool in = k < n;
        col[u] = in ? stream_load(a.JA + base + k) : 0u;
        val[u] = in ? value_at<UVAL>(a.AS, base + k, a.unitValue) : 0.0;
    }
    if (tid < R) rowOff[tid] = (uint16_t)((uint64_t)IRP[r0 + tid] - base);
    if (tid + SW_THREADS < R) rowOff[tid + SW_THREADS] = (uint16_t)((uint64_t)IRP[r0 + tid + SW_THREADS] - base);
    if (tid == 0) rowOff[R] = (uint16_t)n;
    __syncthreads();
    // ---- 2. every entry's row
    for (uint32_t rr = tid; rr < R; rr += SW_THREADS) {
        const uint32_t s = rowOff[rr], e = rowOff[rr + 1];
        for (uint32_t j = s; j < e; ++j) mark[j] = (uint16_t)rr;
    }
    __syncthreads();
    // ---- 3. x(s-1) for the entries of the triangle only, the rounded products parked (a lane touches its own slots only)
#pragma unroll
    for (uint32_t u = 0; u < SW_UNROLL; ++u) {
        const uint32_t k = tid + u * SW_THREADS;
        if (k < n) {
            const bool in = sw_in_tri(col[u], (uint64_t)r0 + mark[k], a.upper, a.N);
            if (in) prod[k] = val[u] * a.prev[col[u]];
            else    mark[k] = SW_OUT;
        }
    }
    __syncthreads();
    // ---- 4. one lane per row: the marked-in products in stored order from +0.0, and the epilogue
    for (uint32_t rr = tid; rr < R; rr += SW_THREADS) {
        const uint32_t s = rowOff[rr], e = rowOff[rr + 1];
        double acc = 0.0;
        for (uint32_t j = s; j < e; ++j)
            if (mark[j] != SW_OUT) acc += prod[j];
        sw_store<UVAL>(a, (uint64_t)r0 + rr, 0, acc);
    }
}

// entries [s, e) of row i staged in LDS (cols, vals), column c: products in stored order, SW_AHEAD gathers in flight
template <bool UVAL>
__device__ __forceinline__ void sw_walk(const SweepArgs& a, uint64_t i, uint64_t c, const uint32_t* cols, const double* vals,
                                        uint32_t s, uint32_t e, double& acc) {
    for (uint32_t p = s; p < e; p += SW_AHEAD) {
        bool in[SW_AHEAD];
        double av[SW_AHEAD], xv[SW_AHEAD];
#pragma unroll
        for (uint32_t u = 0; u < SW_AHEAD; ++u) {
            const uint32_t j = p + u < e ? cols[p + u] : 0u;
            in[u] = p + u < e && sw_in_tri(j, i, a.upper, a.N);
            av[u] = in[u] ? (UVAL ? a.unitValue : vals[p + u]) : 0.0;
            xv[u] = in[u] ? a.prev[(uint64_t)j * a.psr + c * a.psc] : 0.0;
        }
#pragma unroll
        for (uint32_t u = 0; u < SW_AHEAD; ++u)
            if (in[u]) acc += av[u] * xv[u];
    }
}

// workgroup (row block, panel): linear id = block * panels + panel
template <typename I, bool UVAL, int P>
__global__ __launch_bounds__(SW_THREADS) void trisweep_block_kernel(const I* __restrict__ IRP, const SweepArgs a) {
    static_assert(P >= 1 && P <= (int)SW_PANEL && (P & (P - 1)) == 0, "panel width");
    __shared__ double   vals[SW_SPAN];
    __shared__ uint32_t cols[SW_SPAN];
    __shared__ uint16_t rowOff[STREAM2_MAX_ROWS + 1];

    if (a.stop && *a.stop) return;               // workgroup-uniform, as the next line: in front of every barrier
    const uint64_t lin = linear_block();
    if (lin >= (uint64_t)a.nBlk * a.panels) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t blk = stream2_block(lin / a.panels, a.nBlk, a.nLong);
    const uint32_t c0 = (uint32_t)(lin % a.panels) * SW_PANEL;
    const uint32_t w = a.k - c0 < SW_PANEL ? a.k - c0 : SW_PANEL;        // this panel's width
    const uint32_t cl = tid % P, g = tid / P;
    const bool live = cl < w;                                            // lanes past the width gather and store nothing
    const uint64_t c = c0 + cl;
    const uint4 info = a.blkInfo[blk];
    const uint32_t r0 = info.x, R = info.y, n = info.z;
    const uint64_t base = a.blkBase[blk];

    if (info.w) {
        // ---- a single row of n > SW_SPAN entries: its chunks staged in turn, the first group's lanes walk them in order
        const uint64_t end = base + n;
        double acc = 0.0;
        for (uint64_t q = base; q < end; q += SW_SPAN) {
            const uint32_t cn = (uint32_t)(end - q < (uint64_t)SW_SPAN ? end - q : (uint64_t)SW_SPAN);
#pragma unroll
            for (uint32_t u = 0; u < SW_UNROLL; ++u) {
                const uint32_t k = tid + u * SW_THREADS;
                if (k < cn) {
                    cols[k] = stream_load(a.JA + q + k);
                    if (!UVAL) vals[k] = stream_load(a.AS + q + k);
                }
            }
            __syncthreads();
            if (g == 0 && live) sw_walk<UVAL>(a, r0, c, cols, vals, 0, cn, acc);
            __syncthreads();
        }
        if (g == 0 && live) sw_store<UVAL>(a, r0, c, acc);
        return;
    }

#pragma unroll
    for (uint32_t u = 0; u < SW_UNROLL; ++u) {
        const uint32_t k = tid + u * SW_THREADS;
        if (k < n) {
            cols[k] = stream_load(a.JA + base + k);
            if (!UVAL) vals[k] = stream_load(a.AS + base + k);
        }
    }
    if (tid < R) rowOff[tid] = (uint16_t)((uint64_t)IRP[r0 + tid] - base);
    if (tid + SW_THREADS < R) rowOff[tid + SW_THREADS] = (uint16_t)((uint64_t)IRP[r0 + tid + SW_THREADS] - base);
    if (tid == 0) rowOff[R] = (uint16_t)n;
    __syncthreads();
    if (!live) return;                                                   // (no barrier below)
    for (uint32_t rr = g; rr < R; rr += SW_THREADS / P) {
        double acc = 0.0;
        sw_walk<UVAL>(a, (uint64_t)r0 + rr, c, cols, vals, rowOff[rr], rowOff[rr + 1], acc);
        sw_store<UVAL>(a, (uint64_t)r0 + rr, c, acc);
    }
}

// ------------------------------------------------------------------------------------------------ launches
struct SweepRun {
    const DevMat* d; uint32_t k; hipStream_t st; const uint32_t* stop;
    dim3 grid{1}, block{1};
    unsigned long launches = 0;
};

template <typename I, bool UVAL>
void launchSweep(SweepRun& r, const I* irp, const SweepArgs& a) {
    const bool single = a.k == 1 && a.psr == 1 && a.bsr == 1 && a.osr == 1;
    r.block = dim3(SW_THREADS);
    if (single) {
        r.grid = grid2d(a.nBlk, SW_THREADS);
        hipLaunchKernelGGL((trisweep_kernel<I, UVAL>), r.grid, r.block, 0, r.st, irp, a);
        return;
    }
    r.grid = grid2d((uint64_t)a.nBlk * a.panels, SW_THREADS);
    const uint32_t w = a.k < SW_PANEL ? a.k : SW_PANEL;                  // the widest panel
    if (w == 1)      hipLaunchKernelGGL((trisweep_block_kernel<I, UVAL, 1>), r.grid, r.block, 0, r.st, irp, a);
    else if (w == 2) hipLaunchKernelGGL((trisweep_block_kernel<I, UVAL, 2>), r.grid, r.block, 0, r.st, irp, a);
    else if (w <= 4) hipLaunchKernelGGL((trisweep_block_kernel<I, UVAL, 4>), r.grid, r.block, 0, r.st, irp, a);
    else if (w <= 8) hipLaunchKernelGGL((trisweep_block_kernel<I, UVAL, 8>), r.grid, r.block, 0, r.st, irp, a);
    else             hipLaunchKernelGGL((trisweep_block_kernel<I, UVAL, 16>), r.grid, r.block, 0, r.st, irp, a);
}

void sweepKernel(SweepRun& r, const SweepArgs& a) {
    withIrp(r.d, [&](auto irp) {
        if (r.d->unit) launchSweep<IrpT<decltype(irp)>, true>(r, irp, a);
        else           launchSweep<IrpT<decltype(irp)>, false>(r, irp, a);
    });
    ++r.launches;
}

void x0Kernel(SweepRun& r, const SweepArgs& a) {
    r.grid = grid2d((r.d->M * a.k + SW_THREADS - 1) / SW_THREADS, SW_THREADS);
    r.block = dim3(SW_THREADS);
    if (r.d->unit) hipLaunchKernelGGL(trisweep_x0_kernel<true>, r.grid, r.block, 0, r.st, (uint64_t)r.d->M, a);
    else           hipLaunchKernelGGL(trisweep_x0_kernel<false>, r.grid, r.block, 0, r.st, (uint64_t)r.d->M, a);
    ++r.launches;
}

// One solve of S sweeps, X = x(S).  x0Slot >= 0: x(0) is already in that iterate of the workspace.  scaledSlot: the last
// sweep also writes X / d into the iterate it does not read, whose number is returned there (S >= 1).
void sweepSolve(SweepRun& r, int uplo, int dunit, uint32_t S, const Dense& B, const Dense& X, int x0Slot, int* scaledSlot) {
    const DevMat* d = r.d;
    const TriSweepPlan* p = d->sweep;
    const uint64_t M = d->M;
    const auto iterate = [&](int slot) { return Dense{p->ws + (uint64_t)slot * M * p->width, r.k, true}; };
    SweepArgs a{};
    a.blkInfo = d->blkInfo; a.blkBase = d->blkBase; a.JA = d->JA; a.AS = d->AS; a.diagPos = p->diagPos; a.stop = r.stop;
    a.unitValue = d->unitValue; a.N = d->N;
    a.nBlk = d->nBlk2; a.nLong = d->nLong2; a.k = r.k; a.panels = r.k / SW_PANEL + (r.k % SW_PANEL != 0);
    a.upper = uplo == SPMV_TRI_UPPER; a.dunit = dunit;
    a.b = B.p; a.bsr = B.sr(); a.bsc = B.sc();
    const auto to = [&](const Dense& dst) { a.out = dst.p; a.osr = dst.sr(); a.osc = dst.sc(); };
    Dense cur{};
    int curSlot = -1;
    if (x0Slot >= 0) { cur = iterate(x0Slot); curSlot = x0Slot; }
    else if (S == 0) {                                                   // the diagonal scaling (UNIT in place: x is b already)
        if (!(dunit && B.p == X.p)) { to(X); x0Kernel(r, a); }
        return;
    }
    else if (dunit && !(S == 1 && B.p == X.p)) cur = B;                  // a unit lower sweep reads b itself as x(0)
    else { to(iterate(0)); x0Kernel(r, a); cur = iterate(0); curSlot = 0; }
    for (uint32_t s = 1; s <= S; ++s) {
        const bool last = s == S;
        const int other = curSlot == 0 ? 1 : 0;
        const Dense dst = last ? X : iterate(other);
        a.prev = cur.p; a.psr = cur.sr(); a.psc = cur.sc();
        to(dst);
        a.scaled = nullptr;
        if (last && scaledSlot) { *scaledSlot = other; a.scaled = iterate(other).p; a.ssr = r.k; }
        sweepKernel(r, a);
        cur = dst; curSlot = other;
    }
}

}  // namespace

unsigned long triSweepsSolveLaunches(uint32_t S, bool dunit, bool inPlace) {
    if (S == 0) return dunit && inPlace ? 0 : 1;
    return dunit && !(S == 1 && inPlace) ? S : S + 1ul;
}
unsigned long triSweepsApplyLaunches(uint32_t lower, uint32_t upper) { return lower && upper ? (unsigned long)lower + upper : (unsigned long)lower + upper + 1; }
bool triSweepsMode(const DevMat* d) { return d && d->sweep && d->sweep->mode == SPMV_TRI_APPLY_SWEEPS; }

int triSweepsPrepare(DevMat* d, uint32_t width, hipStream_t st) {
    if (width == 0) width = 1;
    TriSweepPlan* old = d->sweep;
    if (old && old->width >= width) return EXIT_SUCCESS;
    const uint64_t M = d->M, m1 = M ? M : 1;
    if (M && (!d->blkInfo || !d->blkBase)) { ERR("triangular sweeps: the handle has no row-block table"); return EXIT_FAILURE; }
    if (width > (SIZE_MAX / 16) / m1) { ERR("triangular sweeps: a workspace of 2 x %lu x %u doubles does not fit", (unsigned long)M, width); return EXIT_FAILURE; }
    const size_t wsBytes = 2 * m1 * (size_t)width * sizeof(double);
    double* ws = nullptr;
    if (old) {                                                           // widening: the new iterates, then the old ones go
        if (devMalloc(&ws, wsBytes) != hipSuccess) { (void)hipGetLastError(); ERR("triangular sweeps: workspace allocation failed"); return EXIT_FAILURE; }
        (void)hipStreamSynchronize(st);                                  // (what is enqueued may still use the old ones)
        (void)devFree(old->ws);
        old->ws = ws; old->width = width; ++old->prepares;
        return EXIT_SUCCESS;
    }
    uint32_t* diagPos = nullptr;
    uint32_t* flags = nullptr;
    const auto fail = [&](const char* what) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
        (void)devFree(diagPos); (void)devFree(ws); (void)devFree(flags);
        ERR("triangular sweeps: %s failed", what);
        return EXIT_FAILURE;
    };
    if (devMalloc(&diagPos, m1 * 4) != hipSuccess || devMalloc(&ws, wsBytes) != hipSuccess || devMalloc(&flags, 8) != hipSuccess)
        return fail("allocation");
    uint32_t hFlags[2] = {NO_ROW, NO_ROW};
    if (hipMemsetAsync(flags, 0xFF, 8, st) != hipSuccess) return fail("memset");
    if (M)
        withIrp(d, [&](auto irp) {
            hipLaunchKernelGGL((trisweep_diag_kernel<IrpT<decltype(irp)>>), grid2d((M + SW_THREADS - 1) / SW_THREADS, SW_THREADS),
                               dim3(SW_THREADS), 0, st, M, irp, d->JA, diagPos, flags);
        });
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hFlags, flags, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail("the diagonal pass");
    (void)devFree(flags);
    TriSweepPlan* p = new TriSweepPlan;
    p->diagPos = diagPos; p->ws = ws; p->width = width;
    p->firstBadDiag = hFlags[0] == NO_ROW ? -1 : (long)hFlags[0];
    p->sorted = hFlags[0] == NO_ROW && hFlags[1] == NO_ROW;
    p->prepares = 1;
    d->sweep = p;
    return EXIT_SUCCESS;
}

int enqueueTriSweeps(const DevMat* d, int uplo, int diag, uint32_t S, uint32_t k, const Dense& B, const Dense& X, hipStream_t st,
                     dim3* grid, dim3* block, const uint32_t* stop, unsigned long* launches) {
    SweepRun r{d, k, st, stop};
    sweepSolve(r, uplo, diag == SPMV_DIAG_UNIT, S, B, X, -1, nullptr);
    if (grid) *grid = r.grid;
    if (block) *block = r.block;
    if (launches) *launches += r.launches;
    d->sweep->solveLaunches = r.launches;
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

int enqueueTriSweepsApply(const DevMat* d, uint32_t k, const Dense& in, const Dense& out, hipStream_t st, const uint32_t* stop,
                          unsigned long* launches) {
    const uint32_t SL = d->sweep->sweeps[0], SU = d->sweep->sweeps[1];
    SweepRun r{d, k, st, stop};
    if (SL == 0) sweepSolve(r, SPMV_TRI_UPPER, 0, SU, in, out, -1, nullptr);
    else if (SU == 0) {                                                  // z = y / d, in place
        sweepSolve(r, SPMV_TRI_LOWER, 1, SL, in, out, -1, nullptr);
        sweepSolve(r, SPMV_TRI_UPPER, 0, 0, out, out, -1, nullptr);
    } else {                                                             // the last lower sweep leaves y / d as the upper x(0)
        int slot = 0;
        sweepSolve(r, SPMV_TRI_LOWER, 1, SL, in, out, -1, &slot);
        sweepSolve(r, SPMV_TRI_UPPER, 0, SU, out, out, slot, nullptr);
    }
    if (launches) *launches += r.launches;
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

}  // namespace spmvhip

using namespace spmvhip;

// what the two solves check alike (those of hipSpTRSVCSR / hipSpTRSMCSR, and the sweep cap): the handle, or null
static DevMat* sweepHandle(spmat* dA, int uplo, int diag, unsigned sweeps, const double* dB, const double* dX, const char* who) {
    DevMat* d = squareCsrOf(dA, who, "the handle is an ELL handle (only CSR handles are solved)");
    if (!d) return nullptr;
    if (uplo != SPMV_TRI_LOWER && uplo != SPMV_TRI_UPPER) { ERR("%s: unknown uplo %d", who, uplo); return nullptr; }
    if (!dB || !dX) { ERR("%s: %s is NULL", who, !dB ? "dB" : "dX"); return nullptr; }
    if (diag != SPMV_DIAG_STORED && diag != SPMV_DIAG_UNIT) { ERR("%s: unknown diag %d", who, diag); return nullptr; }
    if (sweeps > SPMV_TRI_SWEEPS_MAX) { ERR("%s: %u sweeps are above %d", who, sweeps, SPMV_TRI_SWEEPS_MAX); return nullptr; }
    return d;
}
// ... once the operands are checked: the value array, the plan (built at the first solve, for `k` columns), the diagonal
static bool sweepReady(DevMat* d, int diag, unsigned k, hipStream_t st, const char* who) {
    if (d->NZ && !d->AS && !d->unit) { ERR("%s: the handle has no value array", who); return false; }
    if (!d->sweep && triSweepsPrepare(d, k, st)) { ERR("%s: preparing the sweeps failed", who); return false; }
    if (k > d->sweep->width) {
        ERR("%s: k = %u columns, the sweep workspace was prepared for %u: spmvHipTriSweepsPrepare(dA, width >= k) widens it", who, k,
            d->sweep->width);
        return false;
    }
    if (diag == SPMV_DIAG_STORED && d->sweep->firstBadDiag >= 0) {
        ERR("%s: row %ld does not hold exactly one stored diagonal entry (SPMV_DIAG_STORED needs one in every row)", who,
            d->sweep->firstBadDiag);
        return false;
    }
    return true;
}

extern "C" {

int spmvHipTriSweepsPrepare(spmat* dA, unsigned blockWidth) {
    const char* who = "spmvHipTriSweepsPrepare";
    DevMat* d = squareCsrOf(dA, who, "the handle is an ELL handle (only CSR handles are solved)");
    if (!d) return EXIT_FAILURE;
    if (triSweepsPrepare(d, blockWidth, S.stream)) { ERR("%s: preparing the sweeps failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

int hipSpTRSVSweepsCSR(spmat* dA, int uplo, int diag, unsigned sweeps, const double* dB, double* dX) {
    const char* who = "hipSpTRSVSweepsCSR";
    const Ctx cx = libraryCtx();
    DevMat* d = sweepHandle(dA, uplo, diag, sweeps, dB, dX, who);
    if (!d) return EXIT_FAILURE;
    if (dB != dX && overlaps(dB, dX, d->M * sizeof(double))) { ERR("%s: dB and dX overlap without being equal", who); return EXIT_FAILURE; }
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    if (!sweepReady(d, diag, 1, cx.stream, who)) return EXIT_FAILURE;
    Launch L(cx, dim3(0), dim3(0));
    dim3 grid(0, 0, 0), block(0, 0, 0);
    const Dense B{const_cast<double*>(dB), d->M, false}, X{dX, d->M, false};
    if (enqueueTriSweeps(d, uplo, diag, sweeps, 1, B, X, cx.stream, &grid, &block, nullptr, nullptr)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    L.shape(grid, block);
    return L.finish(who);
}

int hipSpTRSMSweepsCSR(spmat* dA, int uplo, int diag, unsigned sweeps, unsigned k, const double* dB, size_t ldb, int bLayout,
                       double* dX, size_t ldx, int xLayout) {
    const char* who = "hipSpTRSMSweepsCSR";
    const Ctx cx = libraryCtx();
    DevMat* d = sweepHandle(dA, uplo, diag, sweeps, dB, dX, who);
    if (!d) return EXIT_FAILURE;
    if (k == 0) { ERR("%s: k = 0 columns", who); return EXIT_FAILURE; }
    Dense B, X;
    if (!denseOperand(who, "ldb", d->M, k, dB, ldb, bLayout, &B) || !denseOperand(who, "ldx", d->M, k, dX, ldx, xLayout, &X)) return EXIT_FAILURE;
    if (denseShare(k, d->M, B, d->M, X, true)) {
        ERR("%s: dB and dX overlap without being the same block (same pointer, layout and leading dimension)", who);
        return EXIT_FAILURE;
    }
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    if (!sweepReady(d, diag, k, cx.stream, who)) return EXIT_FAILURE;
    Launch L(cx, dim3(0), dim3(0));
    dim3 grid(0, 0, 0), block(0, 0, 0);
    if (enqueueTriSweeps(d, uplo, diag, sweeps, k, B, X, cx.stream, &grid, &block, nullptr, nullptr)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    L.shape(grid, block);
    return L.finish(who);
}

int spmvHipTriSetApply(spmat* dA, int mode, unsigned lowerSweeps, unsigned upperSweeps, unsigned blockWidth) {
    const char* who = "spmvHipTriSetApply";
    DevMat* d = squareCsrOf(dA, who, "the handle is an ELL handle (only CSR handles are solved)");
    if (!d) return EXIT_FAILURE;
    if (mode != SPMV_TRI_APPLY_EXACT && mode != SPMV_TRI_APPLY_SWEEPS) { ERR("%s: unknown mode %d", who, mode); return EXIT_FAILURE; }
    if (d->origin == Origin::FSAI) {                                     // (a solver applies such a dM as G^T (G v) whatever is set here)
        ERR("%s: the handle is an approximate-inverse factor (spmvHipFsaiSetup): as a dM it is applied as G^T (G v), not by triangular solves", who);
        return EXIT_FAILURE;
    }
    if (mode == SPMV_TRI_APPLY_EXACT) {                                  // the plan, if there is one, stays
        if (d->sweep) d->sweep->mode = SPMV_TRI_APPLY_EXACT;
        return EXIT_SUCCESS;
    }
    if (lowerSweeps > SPMV_TRI_SWEEPS_MAX || upperSweeps > SPMV_TRI_SWEEPS_MAX) {
        ERR("%s: %u lower and %u upper sweeps: above %d", who, lowerSweeps, upperSweeps, SPMV_TRI_SWEEPS_MAX);
        return EXIT_FAILURE;
    }
    if (triSweepsPrepare(d, blockWidth, S.stream)) { ERR("%s: preparing the sweeps failed", who); return EXIT_FAILURE; }
    d->sweep->mode = SPMV_TRI_APPLY_SWEEPS;
    d->sweep->sweeps[0] = lowerSweeps; d->sweep->sweeps[1] = upperSweeps;
    return EXIT_SUCCESS;
}

int spmvHipTriSweepsInfo(spmat* dA, spmvTriSweepsInfo* info) {
    const char* who = "spmvHipTriSweepsInfo";
    DevMat* d = descOf(dA, who);
    if (!d) return EXIT_FAILURE;
    if (!info) { ERR("%s: info is NULL", who); return EXIT_FAILURE; }
    *info = spmvTriSweepsInfo{};
    const TriSweepPlan* p = d->sweep;
    if (!p) return EXIT_SUCCESS;
    info->mode = p->mode;
    info->lowerSweeps = p->sweeps[0]; info->upperSweeps = p->sweeps[1];
    info->width = p->width;
    info->solveLaunches = p->solveLaunches;
    info->applyLaunches = p->mode == SPMV_TRI_APPLY_SWEEPS ? triSweepsApplyLaunches(p->sweeps[0], p->sweeps[1]) : 0;
    info->firstBadDiag = p->firstBadDiag;
    info->sorted = p->sorted;
    info->bytes = 4 * (size_t)(d->M ? d->M : 1) + 16 * (size_t)(d->M ? d->M : 1) * p->width;
    info->prepares = p->prepares;
    info->diagPos = p->diagPos; info->workspace = p->ws;
    return EXIT_SUCCESS;
}

}  // extern "C"
