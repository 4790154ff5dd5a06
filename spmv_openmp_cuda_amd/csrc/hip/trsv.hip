// trsv.hip -- sparse triangular solves T x = b on a device CSR handle (hipSpTRSVCSR, spmvHipTriAnalyse; DESIGN.md
// section 17).  x has the bits of the serial loop of spmvHip.h: rows in order, each row's strict-triangle products rounded
// and added in STORED order from +0.0, then (b[i] - acc), divided by the stored diagonal unless the diagonal is unit.
//
// Analysis (pattern only, once per triangle, kept on the handle): level sets.  Row i's level is 1 + the largest level of
// the rows it reads (0 for none); the rows of one level are independent, so a level is solved in parallel once every
// earlier level is final, and each row is still summed serially, so the bits are the loop's.
//   1. tri_count_kernel: per row its strict-triangle entry count (repeats included), its diagonal entries and the
//      position of the diagonal; per entry a key: the column for a strict-triangle entry, N for any other
//   2. the dependents list = the strict triangle transposed: the stable radix sort of the keys with the row as payload,
//      the bounds and row-expansion kernels of transpose.hip (keys N are clamped off the end)
//   3. Kahn's peeling: level 0 is every row with no dependency; peeling a level decrements its dependents' counts, and the
//      lane that takes a count to zero places that row in the next level.  Steps of (tri_peel_run_kernel,
//      tri_peel_wide_kernel) are enqueued 64 at a time and one word is read back per batch: the run kernel (one workgroup)
//      peels level after level while a level holds at most T rows, the wide kernel (a fixed grid) takes one wider level.
//      Only the order inside the peeling's frontier depends on atomics; the levels do not.
//   4. perm = rows sorted by (level, long-row class, row id), a stable sort; its level table is copied to the host.
// Solve: the levels in order on the library stream -- trsv_level_kernel for a level (one lane per short row, one
// wavefront per long row), trsv_run_kernel for a run of consecutive thin levels in ONE workgroup with a barrier between
// levels.  No flags, tickets or spins: ordering across workgroups comes only from kernel boundaries on one stream.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <vector>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {

void freeTri(TriSchedule* s) {
    if (!s) return;
    (void)devFree(s->perm); (void)devFree(s->diagPos); (void)devFree(s->levelPtr);
    delete s;
}

namespace {

constexpr uint32_t TRI_THREADS = 256;
constexpr uint32_t TRI_RUN_THREADS = 1024;      // the workgroup of a run (solve and analysis)
constexpr uint32_t TRI_LONG = 64;               // a row with more strict-triangle entries takes a wavefront
constexpr uint32_t TRI_AHEAD = 8;               // gathers in flight per lane on a short row
constexpr uint32_t TRI_BATCH = 64;              // analysis steps enqueued per host read-back
constexpr uint32_t TRI_WIDE_BLOCKS = 1024;      // grid of the wide peeling kernel (grid-stride)
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;

// the strict triangle: lower j < i, upper i < j < N (a column id >= N of an adopted handle is never read)
__device__ __forceinline__ bool in_tri(uint64_t j, uint64_t i, int upper, uint64_t N) {
    return upper ? (j > i && j < N) : j < i;
}

// ------------------------------------------------------------------------------------------------ analysis
// one lane per row.  key[p]: the column of a strict-triangle entry, N for any other (the bounds kernel drops those);
// cls[i] = 1 for a long row (the low bit of the sort key of step 4; the peeling adds the level above it)
template <typename I>
__global__ __launch_bounds__(TRI_THREADS) void tri_count_kernel(uint64_t M, uint64_t N, const I* __restrict__ IRP,
                                                                const uint32_t* __restrict__ JA, int upper,
                                                                uint32_t* __restrict__ cnt, uint32_t* __restrict__ key,
                                                                uint32_t* __restrict__ cls, uint32_t* __restrict__ diagPos,
                                                                uint32_t* __restrict__ firstBad) {
    const uint64_t i = linear_block() * TRI_THREADS + threadIdx.x;
    if (i >= M) return;
    const uint64_t b = IRP[i], e = IRP[i + 1];
    uint32_t c = 0, nd = 0, dp = 0;
    for (uint64_t p = b; p < e; ++p) {
        const uint32_t j = JA[p];
        const bool s = in_tri(j, i, upper, N);
        c += s;
        key[p] = s ? j : (uint32_t)N;
        if (j == i) { ++nd; dp = (uint32_t)p; }
    }
    cnt[i] = c;
    cls[i] = c > TRI_LONG;
    diagPos[i] = nd == 1 ? dp : 0u;
    if (nd != 1) atomicMin(firstBad, (uint32_t)i);
}

// level 0: every row without a dependency, appended to order[] (tab[0] = {base 0, count})
__global__ __launch_bounds__(TRI_THREADS) void tri_level0_kernel(uint64_t M, const uint32_t* __restrict__ cnt,
                                                                 uint32_t* __restrict__ order, uint2* __restrict__ tab) {
    const uint64_t i = linear_block() * TRI_THREADS + threadIdx.x;
    if (i < M && cnt[i] == 0) order[atomicAdd(&tab[0].y, 1u)] = (uint32_t)i;
}

// peel one row of level `cur`: decrement its dependents; a count that reaches zero places its row in level cur + 1 at
// order[next + slot], slot from `counter`
template <typename C>
__device__ __forceinline__ void tri_peel_row(uint32_t row, uint32_t cur, const uint32_t* __restrict__ depPtr,
                                             const uint32_t* __restrict__ depRow, uint32_t* cnt, uint32_t* lvl,
                                             uint32_t* order, uint32_t next, C counter) {
    const uint32_t e = depPtr[row + 1];
    for (uint32_t d = depPtr[row]; d < e; ++d) {
        const uint32_t q = depRow[d];
        if (atomicSub(&cnt[q], 1u) == 1u) {
            lvl[q] = ((cur + 1) << 1) | (lvl[q] & 1u);
            order[next + counter()] = q;
        }
    }
}

// state: [0] the level to peel next, [1] 1: the wide kernel behind this one peels level [0], [2] 1: done
// One workgroup: first retire the wide kernel's level, then peel levels of at most T rows one after another (a barrier
// between levels: the waves of a workgroup share one CU and its L1), and stop at an empty level (done) or a wider one.
__global__ __launch_bounds__(TRI_RUN_THREADS) void tri_peel_run_kernel(uint32_t T, const uint32_t* __restrict__ depPtr,
                                                                       const uint32_t* __restrict__ depRow, uint32_t* cnt,
                                                                       uint32_t* lvl, uint32_t* order, uint2* tab,
                                                                       uint32_t* state) {
    __shared__ uint32_t sCur, sBase, sCount, sNext, sGo;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        uint32_t cur = state[0];
        if (state[1]) { ++cur; state[1] = 0; }
        const uint2 t = tab[cur];
        sCur = cur; sBase = t.x; sCount = t.y; sNext = 0;
        sGo = !state[2];
    }
    __syncthreads();
    if (!sGo) return;
    for (;;) {
        const uint32_t cur = sCur, base = sBase, count = sCount;
        if (count == 0 || count > T) {
            if (tid == 0) {
                state[0] = cur;
                if (count == 0) state[2] = 1; else state[1] = 1;
            }
            return;
        }
        const uint32_t next = base + count;
        for (uint32_t r = tid; r < count; r += TRI_RUN_THREADS)
            tri_peel_row(order[base + r], cur, depPtr, depRow, cnt, lvl, order, next, [] { return atomicAdd(&sNext, 1u); });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            tab[cur + 1] = make_uint2(next, sNext);
            sCur = cur + 1; sBase = next; sCount = sNext; sNext = 0;
        }
        __syncthreads();
    }
}

// the level state[0] when the run kernel in front of it stopped at a wide one; a fixed grid, lane-strided over its rows
__global__ __launch_bounds__(TRI_THREADS) void tri_peel_wide_kernel(const uint32_t* __restrict__ depPtr,
                                                                    const uint32_t* __restrict__ depRow, uint32_t* cnt,
                                                                    uint32_t* lvl, uint32_t* order, uint2* tab,
                                                                    const uint32_t* __restrict__ state) {
    if (!state[1] || state[2]) return;
    const uint32_t cur = state[0];
    const uint2 t = tab[cur];
    const uint32_t next = t.x + t.y;
    const uint64_t gid = linear_block() * TRI_THREADS + threadIdx.x;
    if (gid == 0) tab[cur + 1].x = next;
    uint32_t* slot = &tab[cur + 1].y;
    for (uint64_t r = gid; r < t.y; r += (uint64_t)TRI_WIDE_BLOCKS * TRI_THREADS)
        tri_peel_row(order[t.x + r], cur, depPtr, depRow, cnt, lvl, order, next, [slot] { return atomicAdd(slot, 1u); });
}

// split[l] = the first long row of level l in the sorted keys (level << 1 | class); levels without one keep their init
__global__ __launch_bounds__(TRI_THREADS) void tri_split_kernel(uint64_t M, const uint32_t* __restrict__ keys,
                                                                uint32_t* __restrict__ split) {
    const uint64_t p = linear_block() * TRI_THREADS + threadIdx.x;
    if (p >= M) return;
    const uint32_t k = keys[p];
    if ((k & 1u) && (p == 0 || keys[p - 1] != k)) split[k >> 1] = (uint32_t)p;
}

// ------------------------------------------------------------------------------------------------ solve
// row i on one lane: its strict-triangle products in stored order, TRI_AHEAD gathers of x in flight, adds in order
// (an entry outside the triangle is skipped, never added as 0.0: -0.0 + 0.0 is +0.0)
template <typename I, bool UVAL>
__device__ __forceinline__ double tri_row(uint64_t i, const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                          const double* __restrict__ AS, double unitValue, const uint32_t* __restrict__ diagPos,
                                          int upper, int dunit, uint64_t N, const double* b, const double* x) {
    const uint64_t s = IRP[i], e = IRP[i + 1];
    double acc = 0.0;
    for (uint64_t p = s; p < e; p += TRI_AHEAD) {
        uint32_t col[TRI_AHEAD];
        bool in[TRI_AHEAD];
        double av[TRI_AHEAD], xv[TRI_AHEAD];
#pragma unroll
        for (uint32_t u = 0; u < TRI_AHEAD; ++u) {
            in[u] = p + u < e;
            col[u] = in[u] ? stream_load(JA + p + u) : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < TRI_AHEAD; ++u) {
            in[u] = in[u] && in_tri(col[u], i, upper, N);
            av[u] = in[u] ? value_at<UVAL>(AS, p + u, unitValue) : 0.0;
            xv[u] = in[u] ? x[col[u]] : 0.0;
        }
#pragma unroll
        for (uint32_t u = 0; u < TRI_AHEAD; ++u)
            if (in[u]) acc += av[u] * xv[u];
    }
    const double r = b[i] - acc;
    return dunit ? r : r / (UVAL ? unitValue : AS[diagPos[i]]);
}

// one level: workgroups [0, shortBlocks) take a short row per lane (perm[begin, begin + nShort)), the rest a long row per
// wavefront (perm[begin + nShort, + nLong)): 64 lanes compute a chunk's products, then every lane adds them in stored
// order (the same sum on each; lane 0 stores)
template <typename I, bool UVAL>
__global__ __launch_bounds__(TRI_THREADS) void trsv_level_kernel(
    uint32_t begin, uint32_t nShort, uint32_t nLong, uint32_t shortBlocks, const uint32_t* __restrict__ perm,
    const I* __restrict__ IRP, const uint32_t* __restrict__ JA, const double* __restrict__ AS, double unitValue,
    const uint32_t* __restrict__ diagPos, int upper, int dunit, uint64_t N, const double* b, double* x, const uint32_t* stop) {
    if (stop && *stop) return;                                           // a stopped Krylov loop (krylov.hip)
    const uint64_t blk = linear_block();
    if (blk < shortBlocks) {
        const uint64_t t = blk * TRI_THREADS + threadIdx.x;
        if (t >= nShort) return;
        const uint32_t i = perm[begin + t];
        x[i] = tri_row<I, UVAL>(i, IRP, JA, AS, unitValue, diagPos, upper, dunit, N, b, x);
        return;
    }
    const uint64_t w = (blk - shortBlocks) * (TRI_THREADS / WAVE) + threadIdx.x / WAVE;
    if (w >= nLong) return;                                              // wave-uniform
    const uint32_t lane = threadIdx.x % WAVE;
    const uint64_t i = perm[begin + nShort + w];
    const uint64_t s = IRP[i], e = IRP[i + 1];
    double acc = 0.0;
    for (uint64_t p = s; p < e; p += WAVE) {
        const uint64_t q = p + lane;
        const uint32_t j = q < e ? stream_load(JA + q) : 0u;
        const bool in = q < e && in_tri(j, i, upper, N);
        const double v = in ? value_at<UVAL>(AS, q, unitValue) * x[j] : 0.0;
        uint64_t mask = __ballot(in);
        while (mask) {                                                   // uniform: every lane adds the same products
            const int k = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            acc += __shfl(v, k, WAVE);
        }
    }
    if (lane == 0) {
        const double r = b[i] - acc;
        x[i] = dunit ? r : r / (UVAL ? unitValue : AS[diagPos[i]]);
    }
}

// levels [l0, l1), each of at most T short rows, in one workgroup: a lane per row, and between levels every wave's stores
// drained and a barrier (the waves share one CU and its L1: no agent-scope fence is needed for this hand-off)
template <typename I, bool UVAL>
__global__ __launch_bounds__(TRI_RUN_THREADS) void trsv_run_kernel(
    uint32_t l0, uint32_t l1, const uint32_t* __restrict__ levelPtr, const uint32_t* __restrict__ perm,
    const I* __restrict__ IRP, const uint32_t* __restrict__ JA, const double* __restrict__ AS, double unitValue,
    const uint32_t* __restrict__ diagPos, int upper, int dunit, uint64_t N, const double* b, double* x, const uint32_t* stop) {
    if (stop && *stop) return;
    for (uint32_t l = l0; l < l1; ++l) {
        const uint32_t s = levelPtr[l], e = levelPtr[l + 1];
        for (uint32_t t = s + threadIdx.x; t < e; t += TRI_RUN_THREADS) {
            const uint32_t i = perm[t];
            x[i] = tri_row<I, UVAL>(i, IRP, JA, AS, unitValue, diagPos, upper, dunit, N, b, x);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

template <typename I, bool UVAL>
void launchSteps(const DevMat* d, const TriSchedule* s, int upper, int dunit, const double* b, double* x, hipStream_t st,
                 dim3* lastGrid, dim3* lastBlock, const uint32_t* stop) {
    const I* IRP = static_cast<const I*>(d->IRP);
    for (const TriSchedule::Step& step : s->steps) {
        if (step.l1 - step.l0 > 1) {
            hipLaunchKernelGGL((trsv_run_kernel<I, UVAL>), dim3(1), dim3(TRI_RUN_THREADS), 0, st, step.l0, step.l1, s->levelPtr,
                               s->perm, IRP, d->JA, d->AS, d->unitValue, s->diagPos, upper, dunit, (uint64_t)d->N, b, x, stop);
            *lastGrid = dim3(1); *lastBlock = dim3(TRI_RUN_THREADS);
            continue;
        }
        const uint32_t l = step.l0, begin = s->levelPtr_h[l], split = s->split_h[l], end = s->levelPtr_h[l + 1];
        const uint32_t nShort = split - begin, nLong = end - split;
        const uint32_t shortBlocks = (nShort + TRI_THREADS - 1) / TRI_THREADS;
        const uint32_t longBlocks = (nLong + TRI_THREADS / WAVE - 1) / (TRI_THREADS / WAVE);
        const dim3 grid = grid2d((uint64_t)shortBlocks + longBlocks, TRI_THREADS);
        hipLaunchKernelGGL((trsv_level_kernel<I, UVAL>), grid, dim3(TRI_THREADS), 0, st, begin, nShort, nLong, shortBlocks,
                           s->perm, IRP, d->JA, d->AS, d->unitValue, s->diagPos, upper, dunit, (uint64_t)d->N, b, x, stop);
        *lastGrid = grid; *lastBlock = dim3(TRI_THREADS);
    }
}

}  // namespace

int triAnalyse(DevMat* d, int uplo, uint32_t T, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t M = d->M, N = d->N, nnz = d->NZ;
    TriSchedule* s = new TriSchedule;
    TempBuf cnt, key, rowOf, keysOut, depRow, depPtr, lvl, order, tab, state, sortTmp, split, bad;
    auto fail = [&](const char* what) {
        const int rc = buildFail(st, "triangular analysis", what);
        freeTri(s);                                       // (after the synchronisation)
        return rc;
    };
    const size_t m1 = std::max<uint64_t>(M, 1);
    if (devMalloc(&s->perm, m1 * 4) || devMalloc(&s->diagPos, m1 * 4) || cnt.alloc(m1 * 4) || lvl.alloc(m1 * 4) ||
        order.alloc(m1 * 4) || tab.alloc((M + 2) * sizeof(uint2)) || state.alloc(16) || bad.alloc(4) ||
        key.alloc(nnz * 4) || rowOf.alloc(nnz * 4) || keysOut.alloc(nnz * 4) || depRow.alloc(nnz * 4) || depPtr.alloc((N + 1) * 4))
        return fail("allocation");
    const dim3 rowsGrid = grid2d((M + TRI_THREADS - 1) / TRI_THREADS, TRI_THREADS), blk(TRI_THREADS);
    const int upper = uplo == SPMV_TRI_UPPER;
    if (hipMemsetAsync(tab.p, 0, (M + 2) * sizeof(uint2), st) || hipMemsetAsync(state.p, 0, 16, st) ||
        hipMemsetAsync(bad.p, 0xFF, 4, st))
        return fail("memset");
    // 1. counts, keys, diagonal
    withIrp(d, [&](auto irp) {
        hipLaunchKernelGGL((tri_count_kernel<IrpT<decltype(irp)>>), rowsGrid, blk, 0, st, M, N, irp, d->JA,
                           upper, cnt.as<uint32_t>(), key.as<uint32_t>(), lvl.as<uint32_t>(), s->diagPos, bad.as<uint32_t>());
    });
    // 2. dependents: rows of the strict triangle's entries, stably sorted by column
    if (nnz) enqueueRowOf(M, d->IRP, d->irpBytes, rowOf.as<uint32_t>(), st);
    if (enqueueSortedByColumn(nnz, N, bitsFor(N + 1) /* a key may be N */, key.as<uint32_t>(), rowOf.as<uint32_t>(), keysOut.as<uint32_t>(),
                              depRow.as<uint32_t>(), depPtr.as<uint32_t>(), sortTmp, st) != hipSuccess)
        return fail("sort");
    // 3. levels
    hipLaunchKernelGGL(tri_level0_kernel, rowsGrid, blk, 0, st, M, cnt.as<uint32_t>(), order.as<uint32_t>(), tab.as<uint2>());
    uint32_t hState[4] = {0, 0, 0, 0};
    for (uint64_t steps = 0; !hState[2]; steps += TRI_BATCH) {
        if (steps > M + TRI_BATCH) return fail("level peeling (no progress)");
        for (uint32_t k = 0; k < TRI_BATCH; ++k) {
            hipLaunchKernelGGL(tri_peel_run_kernel, dim3(1), dim3(TRI_RUN_THREADS), 0, st, T, depPtr.as<uint32_t>(),
                               depRow.as<uint32_t>(), cnt.as<uint32_t>(), lvl.as<uint32_t>(), order.as<uint32_t>(), tab.as<uint2>(),
                               state.as<uint32_t>());
            hipLaunchKernelGGL(tri_peel_wide_kernel, dim3(TRI_WIDE_BLOCKS), blk, 0, st, depPtr.as<uint32_t>(), depRow.as<uint32_t>(),
                               cnt.as<uint32_t>(), lvl.as<uint32_t>(), order.as<uint32_t>(), tab.as<uint2>(), state.as<uint32_t>());
        }
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hState, state.p, 16, hipMemcpyDeviceToHost, st) ||
            hipStreamSynchronize(st))
            return fail("level peeling");
    }
    const uint32_t L = hState[0];
    std::vector<uint2> hTab(L + 1);
    uint32_t firstBad = 0;
    if (hipMemcpyAsync(hTab.data(), tab.p, (L + 1) * sizeof(uint2), hipMemcpyDeviceToHost, st) ||
        hipMemcpyAsync(&firstBad, bad.p, 4, hipMemcpyDeviceToHost, st) || hipStreamSynchronize(st))
        return fail("level table read-back");
    if (hTab[L].x != M) return fail("level peeling (rows left unplaced)");
    // 4. perm: rows by (level, class, id) -- a stable sort of the keys over the rows in id order
    s->levelPtr_h.resize(L + 1);
    s->split_h.resize(L);
    for (uint32_t l = 0; l <= L; ++l) s->levelPtr_h[l] = hTab[l].x;
    for (uint32_t l = 0; l < L; ++l) s->split_h[l] = hTab[l + 1].x;
    if (M) {
        enqueueIota(M, order.as<uint32_t>(), st);
        TempBuf sortTmp2;                                 // (not sortTmp: replacing a held workspace waits for the stream)
        if (split.alloc(L * 4ull) ||
            sortPairs(sortTmp2, lvl.as<uint32_t>(), cnt.as<uint32_t>(), order.as<uint32_t>(), s->perm, (size_t)M, 0u, bitsFor(2ull * L + 1), st) !=
                hipSuccess)
            return fail("level sort");
        if (hipMemcpyAsync(split.p, s->split_h.data(), L * 4ull, hipMemcpyHostToDevice, st)) return fail("split upload");
        hipLaunchKernelGGL(tri_split_kernel, rowsGrid, blk, 0, st, M, cnt.as<uint32_t>(), split.as<uint32_t>());
        if (hipMemcpyAsync(s->split_h.data(), split.p, L * 4ull, hipMemcpyDeviceToHost, st) || hipStreamSynchronize(st))
            return fail("split read-back");
    }
    if (devMalloc(&s->levelPtr, (L + 1) * 4ull) ||
        hipMemcpyAsync(s->levelPtr, s->levelPtr_h.data(), (L + 1) * 4ull, hipMemcpyHostToDevice, st))
        return fail("level table upload");
    // the launch plan: runs of consecutive levels of at most T rows without a long row, a launch per other level
    spmvTriInfo& in = s->info;
    in.levels = L;
    in.firstBadDiag = firstBad == NO_ROW ? -1 : (long)firstBad;
    for (uint32_t l = 0; l < L;) {
        uint32_t e = l;
        while (e < L && T && s->levelPtr_h[e + 1] - s->levelPtr_h[e] <= T && s->split_h[e] == s->levelPtr_h[e + 1]) ++e;
        if (e - l > 1) {
            s->steps.push_back({l, e});
            in.fusedLevels += e - l;
            l = e;
        } else {
            s->steps.push_back({l, l + 1});
            ++l;
        }
    }
    for (uint32_t l = 0; l < L; ++l) {
        in.maxLevelRows = std::max<ulong>(in.maxLevelRows, s->levelPtr_h[l + 1] - s->levelPtr_h[l]);
        in.longRows += s->levelPtr_h[l + 1] - s->split_h[l];
    }
    in.launches = s->steps.size();
    in.bytes = 8 * m1 + 4ull * (L + 1);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail("kernels");
    const int before = d->tri[uplo] ? d->tri[uplo]->info.analyses : 0;
    freeTri(d->tri[uplo]);
    in.analyses = before + 1;
    in.analysisMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    d->tri[uplo] = s;
    return EXIT_SUCCESS;
}

int enqueueTrsv(const DevMat* d, int uplo, int diag, const double* b, double* x, hipStream_t st, dim3* grid, dim3* block,
                const uint32_t* stop) {
    const TriSchedule* s = d->tri[uplo];
    const int upper = uplo == SPMV_TRI_UPPER, dunit = diag == SPMV_DIAG_UNIT;
    withIrp(d, [&](auto irp) {
        if (d->unit) launchSteps<IrpT<decltype(irp)>, true>(d, s, upper, dunit, b, x, st, grid, block, stop);
        else         launchSteps<IrpT<decltype(irp)>, false>(d, s, upper, dunit, b, x, st, grid, block, stop);
    });
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

void triInfo(const DevMat* d, int uplo, spmvTriInfo* out) {
    *out = d->tri[uplo] ? d->tri[uplo]->info : spmvTriInfo{};
}

}  // namespace spmvhip
