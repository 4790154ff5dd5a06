// ilu0.hip -- ILU(0) of a square device CSR handle, in place (hipSpILU0CSR; contract in spmvHip.h).
// AS ends with the bits of the serial loop of spmvHip.h: rows in order; in row i, for each stored k = JA[p] < i in ascending
// order, AS[p] /= the final U diagonal of row k, then every later entry q of row i whose column row k also stores right of
// its diagonal (position r) becomes AS[q] - AS[p] * AS[r], each product and each subtraction rounded on its own.
//
// Schedule: the lower triangle's level sets of trsv.hip (d->tri[SPMV_TRI_LOWER]).  Row i reads only rows k = JA[p] < i,
// which lie in earlier levels, so the rows of one level are factored in parallel once every earlier level is final:
// ilu0_level_kernel for a wide level, ilu0_run_kernel for a run of thin levels in ONE workgroup with every wave's stores
// drained and a barrier between levels (the waves share one CU and its L1, as in trsv_run_kernel).  No flags, tickets or
// spins: ordering across workgroups comes only from kernel boundaries on one stream.
//
// One row, one group of G lanes (G = 8, 16 or 64).  The group walks the row's k steps in program order; in a step every
// lane divides AS[p] by row k's diagonal (the same bits on each; lane 0 stores), the lanes take row k's entries right of its
// diagonal, and each finds its column among row i's columns right of p by binary search and subtracts.  Row i's columns
// are strictly ascending, so within a step each target q is written by at most one lane; between steps every lane waits
// for its memory operations (one wavefront: the hand-off needs nothing more).  So the bits are the loop's, and nothing
// rests on atomics or on the order of LDS operations.
//
// Where row i lives: a wavefront stages the rows of its groups (columns and values) in LDS when together they hold at most
// ILU_WAVE_LDS entries, factors them there and writes the values back once; otherwise (a wave-uniform branch) its groups
// work on JA / AS in global memory, the long-row path.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {
namespace {

constexpr uint32_t ILU_THREADS = 256;           // workgroup of a wide level
constexpr uint32_t ILU_RUN_THREADS = 1024;      // the workgroup of a run of thin levels
constexpr uint32_t ILU_WAVE_LDS = 256;          // entries a wavefront stages in LDS for all its rows (3 KiB)
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;

// every memory operation of this lane complete, and no compiler motion across: the hand-off between the steps of a row
__device__ __forceinline__ void step_wait() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }

// row i, on lane g of its group: n entries at cols[0, n) / vals[0, n) (LDS or AS itself), the first nLow left of the
// diagonal.  Rows k < i are final in AS.
template <uint32_t G, typename I>
__device__ __forceinline__ void ilu_row(uint32_t g, uint32_t nLow, uint32_t n, const uint32_t* cols, double* vals,
                                        const I* IRP, const uint32_t* JA, const double* AS, const uint32_t* diagPos) {
    for (uint32_t t = 0; t < nLow; ++t) {
        const uint32_t k = cols[t];
        const uint32_t dk = diagPos[k], ek = (uint32_t)IRP[k + 1];
        const double l = vals[t] / AS[dk];
        for (uint32_t r = dk + 1 + g; r < ek; r += G) {
            const uint32_t c = JA[r];
            uint32_t lo = t + 1, hi = n;                                 // the first of row i's columns >= c, right of p
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (cols[mid] < c) lo = mid + 1; else hi = mid;
            }
            if (lo < n && cols[lo] == c) vals[lo] = vals[lo] - l * AS[r];
        }
        if (g == 0) vals[t] = l;
        step_wait();
    }
}

// one wavefront's rows: the group h = lane / G takes `row` (NO_ROW: none).  Every lane of the wave calls this (shuffles).
template <uint32_t G, typename I>
__device__ __forceinline__ void ilu_wave(uint32_t row, uint32_t* sCols, double* sVals, const I* IRP, const uint32_t* JA,
                                         double* AS, const uint32_t* diagPos, uint32_t* longRows) {
    const uint32_t lane = threadIdx.x % WAVE, g = lane % G, h = lane / G;
    uint32_t s = 0, n = 0, nLow = 0;
    if (row != NO_ROW) {
        s = (uint32_t)IRP[row];
        n = (uint32_t)IRP[row + 1] - s;
        nLow = diagPos[row] - s;
    }
    uint32_t off = 0, total = 0;                                         // the group's offset in the wave's LDS span
#pragma unroll
    for (uint32_t o = 0; o < WAVE / G; ++o) {
        const uint32_t len = __shfl(n, (int)(o * G), WAVE);
        off += o < h ? len : 0u;
        total += len;
    }
    const uint64_t rows = __ballot(row != NO_ROW && g == 0);
    if (total > ILU_WAVE_LDS) {                                          // wave-uniform: the long-row path, in AS
        if (lane == 0) atomicAdd(longRows, (uint32_t)__popcll(rows));
        if (row != NO_ROW) ilu_row<G, I>(g, nLow, n, JA + s, AS + s, IRP, JA, AS, diagPos);
        return;
    }
    uint32_t* c = sCols + (threadIdx.x / WAVE) * ILU_WAVE_LDS + off;
    double* v = sVals + (threadIdx.x / WAVE) * ILU_WAVE_LDS + off;
    for (uint32_t j = g; j < n; j += G) {
        c[j] = JA[s + j];
        v[j] = AS[s + j];
    }
    step_wait();
    ilu_row<G, I>(g, nLow, n, c, v, IRP, JA, AS, diagPos);
    step_wait();
    for (uint32_t j = g; j < n; j += G) AS[s + j] = v[j];
}

// one level: perm[begin, begin + count), G lanes per row
template <uint32_t G, typename I>
__global__ __launch_bounds__(ILU_THREADS) void ilu0_level_kernel(uint32_t begin, uint32_t count, const uint32_t* __restrict__ perm,
                                                                 const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                                                 double* AS, const uint32_t* __restrict__ diagPos,
                                                                 uint32_t* longRows) {
    __shared__ uint32_t sCols[ILU_THREADS / WAVE * ILU_WAVE_LDS];
    __shared__ double sVals[ILU_THREADS / WAVE * ILU_WAVE_LDS];
    const uint64_t t = (linear_block() * ILU_THREADS + threadIdx.x) / G;
    ilu_wave<G, I>(t < count ? perm[begin + t] : NO_ROW, sCols, sVals, IRP, JA, AS, diagPos, longRows);
}

// levels [l0, l1) in one workgroup: ILU_RUN_THREADS / G rows at a time, and between levels every wave's stores drained and
// a barrier (the waves share one CU and its L1: no agent-scope fence is needed for this hand-off)
template <uint32_t G, typename I>
__global__ __launch_bounds__(ILU_RUN_THREADS) void ilu0_run_kernel(uint32_t l0, uint32_t l1, const uint32_t* __restrict__ levelPtr,
                                                                   const uint32_t* __restrict__ perm, const I* __restrict__ IRP,
                                                                   const uint32_t* __restrict__ JA, double* AS,
                                                                   const uint32_t* __restrict__ diagPos, uint32_t* longRows) {
    __shared__ uint32_t sCols[ILU_RUN_THREADS / WAVE * ILU_WAVE_LDS];
    __shared__ double sVals[ILU_RUN_THREADS / WAVE * ILU_WAVE_LDS];
    for (uint32_t l = l0; l < l1; ++l) {
        const uint32_t s = levelPtr[l], e = levelPtr[l + 1];
        for (uint32_t b = s; b < e; b += ILU_RUN_THREADS / G) {         // uniform over the workgroup
            const uint32_t t = b + threadIdx.x / G;
            ilu_wave<G, I>(t < e ? perm[t] : NO_ROW, sCols, sVals, IRP, JA, AS, diagPos, longRows);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

// the smallest row whose factored diagonal is +-0.0
__global__ __launch_bounds__(ILU_THREADS) void ilu0_pivot_kernel(uint64_t M, const uint32_t* __restrict__ diagPos,
                                                                 const double* __restrict__ AS, uint32_t* __restrict__ first) {
    const uint64_t i = linear_block() * ILU_THREADS + threadIdx.x;
    if (i < M && AS[diagPos[i]] == 0.0) atomicMin(first, (uint32_t)i);
}

// one wavefront per row: the first row whose columns are not STRICTLY ascending (a repeated column counts).  The
// serial-order selection's csr_unsorted_kernel (select.hip) asks the non-strict question.
template <typename I>
__global__ __launch_bounds__(256) void csr_not_strict_kernel(uint64_t M, const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                                             uint32_t* __restrict__ first) {
    const uint64_t r = linear_block() * 4 + threadIdx.x / WAVE;
    if (r >= M) return;
    const uint64_t b = IRP[r], e = IRP[r + 1];
    bool bad = false;
    for (uint64_t j = b + threadIdx.x % WAVE; j + 1 < e; j += WAVE) bad |= JA[j] >= JA[j + 1];
    if (bad) atomicMin(first, (uint32_t)r);
}

template <uint32_t G, typename I>
void launchIlu(const DevMat* d, const TriSchedule* s, uint32_t* longRows, hipStream_t st) {
    const I* IRP = static_cast<const I*>(d->IRP);
    for (const TriSchedule::Step& step : s->steps) {
        if (step.l1 - step.l0 > 1) {
            hipLaunchKernelGGL((ilu0_run_kernel<G, I>), dim3(1), dim3(ILU_RUN_THREADS), 0, st, step.l0, step.l1, s->levelPtr,
                               s->perm, IRP, d->JA, d->AS, s->diagPos, longRows);
            continue;
        }
        const uint32_t begin = s->levelPtr_h[step.l0], count = s->levelPtr_h[step.l0 + 1] - begin;
        const uint64_t blocks = ((uint64_t)count * G + ILU_THREADS - 1) / ILU_THREADS;
        hipLaunchKernelGGL((ilu0_level_kernel<G, I>), grid2d(blocks, ILU_THREADS), dim3(ILU_THREADS), 0, st, begin, count, s->perm,
                           IRP, d->JA, d->AS, s->diagPos, longRows);
    }
}

template <typename I>
void launchIluWidth(const DevMat* d, const TriSchedule* s, uint32_t G, uint32_t* longRows, hipStream_t st) {
    if (G == 64)      launchIlu<64, I>(d, s, longRows, st);
    else if (G == 16) launchIlu<16, I>(d, s, longRows, st);
    else              launchIlu<8, I>(d, s, longRows, st);
}

}  // namespace

int iluUnsortedRow(const DevMat* d, hipStream_t st, long* row) {
    uint32_t first = NO_ROW;
    const int rc = deviceFlag(0xFF, st, "csr_not_strict_kernel", &first, [&](uint32_t* dFirst) {
        withIrp(d, [&](auto irp) {
            hipLaunchKernelGGL((csr_not_strict_kernel<IrpT<decltype(irp)>>), grid2d((d->M + 3) / 4, 256), dim3(256), 0, st, d->M, irp, d->JA, dFirst);
        });
    });
    *row = first == NO_ROW ? -1 : (long)first;
    return rc;
}

int iluFactor(DevMat* d, uint32_t G, hipStream_t st) {
    const TriSchedule* s = d->tri[SPMV_TRI_LOWER];
    TempBuf words;
    uint32_t h[2] = {NO_ROW, 0};                    // [0] the zero pivot, [1] rows on the long-row path
    HIP_TRY(words.alloc(8));
    uint32_t* const w = words.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(w, h, 8, hipMemcpyHostToDevice, st));
    withIrp(d, [&](auto irp) { launchIluWidth<IrpT<decltype(irp)>>(d, s, G, w + 1, st); });
    hipLaunchKernelGGL(ilu0_pivot_kernel, grid2d((d->M + ILU_THREADS - 1) / ILU_THREADS, ILU_THREADS), dim3(ILU_THREADS), 0, st,
                       d->M, s->diagPos, d->AS, w);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, w, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    d->ilu.zeroPivot = h[0] == NO_ROW ? -1 : (long)h[0];
    d->ilu.levels = s->info.levels;
    d->ilu.launches = s->steps.size() + 1;
    d->ilu.longRows = h[1];
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
