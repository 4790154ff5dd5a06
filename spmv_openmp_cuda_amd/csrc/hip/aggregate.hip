// aggregate.hip -- the aggregation of a square CSR handle on the device (spmvHipAggregateCSR, and every level of the
// multigrid setups of amg.hip).  DESIGN.md section 24; the contract is in spmvHip.h.
// Aggregation.  The roots are the lexicographically first distance-2 maximal independent set under the HASH order of the
// colouring.  Rounds of two launches over the rows still undecided:
//   select   an undecided row that no vertex within distance 2, retired ones excepted, beats becomes a ROOT.  A state word
//            read inside the launch is UNDECIDED or, for a row that became a root in this very launch, ROOT: both count,
//            and a root of this round within distance 2 beats the row anyway, so the race changes nothing.
//   retire   an undecided row with a ROOT within distance 2 retires; the others are counted into the round's word.  Roots
//            do not change in this launch, and a row writes its own word only.
// The middle vertex of a distance-2 path is never looked at: undecided or retired, the path counts.  No row list is
// compacted between rounds (a decided row returns at its first load); K rounds are enqueued, then their K counts are read.
// Then the roots are numbered by a scan, ring 1 takes its root's id, ring 2 the id of its best ring-1 neighbour.
// Rows with more than 64 adjacency entries take a wavefront each (the lanes share the first hop), the others a lane.
#include <hip/hip_runtime.h>
#include <chrono>
#include <vector>

#include "device_prims.hpp"

namespace spmvhip {

namespace {

constexpr uint32_t AG_THREADS = WG_THREADS;
constexpr uint32_t AG_WAVES = AG_THREADS / 64;
constexpr uint32_t AG_LONG = 64;                               // adjacency entries above which a row takes a wavefront
constexpr uint32_t UNDECIDED = 0xFFFFFFFFu, RETIRED = 0, ROOT = 1, RING1 = 2;

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {      // the murmur3 32-bit finaliser
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
// (key, id) as one word: j beats i iff pri(j) > pri(i)
__device__ __forceinline__ uint64_t pri(uint32_t i, uint32_t seed) { return (uint64_t)fmix32(i ^ seed) << 32 | i; }
__device__ __forceinline__ uint32_t stateOf(const uint32_t* state, uint32_t i) { return __atomic_load_n(state + i, __ATOMIC_RELAXED); }

// the pattern of A + A^T as two CSR sides: the stored rows and the incoming ones (null when the pattern is symmetric)
template <typename I> struct Adj {
    uint64_t M;
    const I* IRP; const uint32_t* JA;
    const uint32_t* tptr; const uint32_t* tcol;
    // f(j) for every adjacency entry j != i, j < M of row i (repeats included) taken `width` apart from `lane`, until f
    // returns true; returns whether it did
    template <typename F> __device__ __forceinline__ bool any(uint32_t i, uint32_t lane, uint32_t width, F&& f) const {
        for (int side = 0; side < 2; ++side) {
            if (side && !tptr) break;
            const uint32_t* col = side ? tcol : JA;
            const uint64_t b = side ? tptr[i] : (uint64_t)IRP[i], e = side ? tptr[i + 1] : (uint64_t)IRP[i + 1];
            for (uint64_t p = b + lane; p < e; p += width) {
                const uint32_t j = col[p];
                if (j != i && j < M && f(j)) return true;
            }
        }
        return false;
    }
};

// every row gets UNDECIDED and joins the short or the long list (one atomic per wavefront and list: the ORDER of a list
// depends on the run, no output does)
template <typename I>
__global__ __launch_bounds__(AG_THREADS) void ag_classify_kernel(Adj<I> g, uint32_t* __restrict__ state, uint32_t* __restrict__ shortList,
                                                                 uint32_t* __restrict__ longList, uint32_t* __restrict__ cnt) {
    const uint64_t r = linear_block() * AG_THREADS + threadIdx.x;
    const bool live = r < g.M;
    uint64_t deg = 0;
    if (live) {
        state[r] = UNDECIDED;
        deg = (uint64_t)g.IRP[r + 1] - (uint64_t)g.IRP[r] + (g.tptr ? g.tptr[r + 1] - g.tptr[r] : 0u);
    }
    const bool isLong = live && deg > AG_LONG, isShort = live && !isLong;
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t below = (1ull << lane) - 1;
    const uint64_t bs = __ballot(isShort), bl = __ballot(isLong);
    uint32_t baseS = 0, baseL = 0;
    if (lane == 0) {
        if (bs) baseS = atomicAdd(&cnt[0], (uint32_t)__popcll(bs));
        if (bl) baseL = atomicAdd(&cnt[1], (uint32_t)__popcll(bl));
    }
    baseS = __shfl(baseS, 0);
    baseL = __shfl(baseL, 0);
    if (isShort) shortList[baseS + __popcll(bs & below)] = (uint32_t)r;
    if (isLong) longList[baseL + __popcll(bl & below)] = (uint32_t)r;
}

// the row of list place k for this lane: a lane per row, or a wavefront per row (uniform in the wavefront)
template <bool WAVE_ROW>
__device__ __forceinline__ bool ag_row(uint32_t n, const uint32_t* __restrict__ list, uint32_t& i, uint32_t& lane) {
    const uint64_t k = WAVE_ROW ? linear_block() * AG_WAVES + threadIdx.x / 64 : linear_block() * AG_THREADS + threadIdx.x;
    lane = WAVE_ROW ? threadIdx.x % 64 : 0;
    if (k >= n) return false;
    i = list[k];
    return true;
}

template <typename I, bool WAVE_ROW>
__global__ __launch_bounds__(AG_THREADS) void ag_select_kernel(Adj<I> g, uint32_t seed, uint32_t n, const uint32_t* __restrict__ list,
                                                               uint32_t* state) {
    uint32_t i = 0, lane = 0;
    const bool live = ag_row<WAVE_ROW>(n, list, i, lane) && stateOf(state, i) == UNDECIDED;
    bool blocked = false;
    if (live) {
        const uint64_t pi = pri(i, seed);
        auto beats = [&](uint32_t j) { return j != i && stateOf(state, j) != RETIRED && pri(j, seed) > pi; };
        blocked = g.any(i, lane, WAVE_ROW ? 64 : 1, [&](uint32_t k) { return beats(k) || g.any(k, 0, 1, beats); });
    }
    if (WAVE_ROW) blocked = __ballot(blocked) != 0;
    if (live && !blocked && lane == 0) __atomic_store_n(state + i, ROOT, __ATOMIC_RELAXED);
}

template <typename I, bool WAVE_ROW>
__global__ __launch_bounds__(AG_THREADS) void ag_retire_kernel(Adj<I> g, uint32_t n, const uint32_t* __restrict__ list, uint32_t* state,
                                                               uint32_t* __restrict__ left) {
    uint32_t i = 0, lane = 0;
    const bool live = ag_row<WAVE_ROW>(n, list, i, lane) && stateOf(state, i) == UNDECIDED;
    bool near = false;
    if (live) {
        auto isRoot = [&](uint32_t j) { return stateOf(state, j) == ROOT; };
        near = g.any(i, lane, WAVE_ROW ? 64 : 1, [&](uint32_t k) { return isRoot(k) || g.any(k, 0, 1, isRoot); });
    }
    if (WAVE_ROW) near = __ballot(near) != 0;
    if (live && near && lane == 0) __atomic_store_n(state + i, RETIRED, __ATOMIC_RELAXED);
    const uint64_t waits = __ballot(live && !near && lane == 0);
    if (waits && threadIdx.x % 64 == 0) atomicAdd(left, (uint32_t)__popcll(waits));
}

__global__ __launch_bounds__(AG_THREADS) void ag_flag_kernel(uint64_t M, const uint32_t* __restrict__ state, uint32_t* __restrict__ flag) {
    const uint64_t r = linear_block() * AG_THREADS + threadIdx.x;
    if (r <= M) flag[r] = r < M && state[r] == ROOT;
}

// roots take their number, ring 1 the number of its root (and the state RING1: a row writes its own word only, and only
// ROOT is looked for)
template <typename I, bool WAVE_ROW>
__global__ __launch_bounds__(AG_THREADS) void ag_ring1_kernel(Adj<I> g, uint32_t n, const uint32_t* __restrict__ list, uint32_t* state,
                                                              const uint32_t* __restrict__ number, uint32_t* __restrict__ agg) {
    uint32_t i = 0, lane = 0;
    if (!ag_row<WAVE_ROW>(n, list, i, lane)) return;
    if (stateOf(state, i) == ROOT) { if (lane == 0) agg[i] = number[i]; return; }
    uint32_t root = UNDECIDED;
    g.any(i, lane, WAVE_ROW ? 64 : 1, [&](uint32_t k) { if (stateOf(state, k) == ROOT) root = k; return root != UNDECIDED; });
    if (WAVE_ROW)
        for (int off = 32; off; off >>= 1) root = min(root, (uint32_t)__shfl_xor(root, off));   // (one root at most: min picks it)
    if (root == UNDECIDED || lane) return;
    agg[i] = number[root];
    __atomic_store_n(state + i, RING1, __ATOMIC_RELAXED);
}

template <typename I, bool WAVE_ROW>
__global__ __launch_bounds__(AG_THREADS) void ag_ring2_kernel(Adj<I> g, uint32_t seed, uint32_t n, const uint32_t* __restrict__ list,
                                                              const uint32_t* __restrict__ state, uint32_t* agg) {
    uint32_t i = 0, lane = 0;
    if (!ag_row<WAVE_ROW>(n, list, i, lane) || state[i] != RETIRED) return;
    uint64_t best = 0;
    bool found = false;
    g.any(i, lane, WAVE_ROW ? 64 : 1, [&](uint32_t k) {
        if (state[k] == RING1) {
            const uint64_t pk = pri(k, seed);
            if (!found || pk > best) best = pk;
            found = true;
        }
        return false;
    });
    if (WAVE_ROW)
        for (int off = 32; off; off >>= 1) {
            const uint64_t ob = __shfl_xor(best, off);
            const bool of = __shfl_xor((int)found, off) != 0;
            if (of && (!found || ob > best)) best = ob;
            found = found || of;
        }
    if (found && lane == 0) agg[i] = __atomic_load_n(agg + (uint32_t)best, __ATOMIC_RELAXED);   // (a ring-1 word: final before this launch)
}

// (bad: an id that is no aggregate -- never, by maximality; it must not index the sizes)
__global__ __launch_bounds__(AG_THREADS) void ag_hist_kernel(uint64_t M, uint32_t nAgg, const uint32_t* __restrict__ agg, uint32_t* __restrict__ size,
                                                             uint32_t* __restrict__ bad) {
    const uint64_t r = linear_block() * AG_THREADS + threadIdx.x;
    if (r >= M) return;
    const uint32_t a = agg[r];
    if (a < nAgg) atomicAdd(size + a, 1u);
    else atomicOr(bad, 1u);
}
__global__ __launch_bounds__(AG_THREADS) void ag_minmax_kernel(uint64_t n, const uint32_t* __restrict__ size, uint32_t* __restrict__ mm) {
    const uint64_t r = linear_block() * AG_THREADS + threadIdx.x;
    if (r < n) { atomicMin(mm, size[r]); atomicMax(mm + 1, size[r]); }
}

}  // namespace

int aggregateCsr(const DevMat* a, uint32_t seed, uint32_t K, uint32_t* dAgg, spmvAggInfo* info, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t M = a->M;
    spmvAggInfo out{};
    out.symmetric = 1;
    auto fail = [&](const char* what) { return buildFail(st, "aggregate", what); };
    if (M == 0) { if (info) *info = out; return EXIT_SUCCESS; }
    IncomingPattern in;
    if (buildIncoming(a, in, st, "aggregate")) return EXIT_FAILURE;
    out.symmetric = in.symmetric;
    TempBuf state, lists, cnt, number, scanTmp, size;
    if (state.alloc(M * 4) || lists.alloc(M * 8) || cnt.alloc((K + 2) * 4) || number.alloc((M + 1) * 8)) return fail("temporary allocation (20 B per row)");
    uint32_t* const dState = state.as<uint32_t>();
    uint32_t* const list[2] = {lists.as<uint32_t>(), lists.as<uint32_t>() + M};
    uint32_t* const dCnt = cnt.as<uint32_t>();                 // [0], [1] the list lengths; [2 .. K + 1] undecided rows after a round
    uint32_t* const dFlag = number.as<uint32_t>();             // root flags, M + 1 words, then their scan, M + 1 words
    uint32_t* const dNumber = dFlag + M + 1;
    std::vector<uint32_t> h(K + 2, 0);
    if (hipMemsetAsync(dCnt, 0, (K + 2) * 4, st) != hipSuccess) return fail("state");
    int rc = EXIT_SUCCESS;
    withIrp(a, [&](auto irp) {
        using I = IrpT<decltype(irp)>;
        const Adj<I> g{M, irp, a->JA, in.ptr, in.col};
        hipLaunchKernelGGL((ag_classify_kernel<I>), gridFor(M), dim3(AG_THREADS), 0, st, g, dState, list[0], list[1], dCnt);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h.data(), dCnt, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { rc = fail("classification"); return; }
        const uint32_t nS = h[0], nL = h[1];
        out.longRows = nL;
        const dim3 gS = gridFor(nS), gL = gridFor(nL, AG_WAVES), blk(AG_THREADS);
        // the rounds
        for (bool done = false; !done;) {
            if (hipMemsetAsync(dCnt + 2, 0, K * 4, st) != hipSuccess) { rc = fail("state"); return; }
            for (uint32_t t = 0; t < K; ++t) {
                if (nS) hipLaunchKernelGGL((ag_select_kernel<I, false>), gS, blk, 0, st, g, seed, nS, list[0], dState);
                if (nL) hipLaunchKernelGGL((ag_select_kernel<I, true>), gL, blk, 0, st, g, seed, nL, list[1], dState);
                if (nS) hipLaunchKernelGGL((ag_retire_kernel<I, false>), gS, blk, 0, st, g, nS, list[0], dState, dCnt + 2 + t);
                if (nL) hipLaunchKernelGGL((ag_retire_kernel<I, true>), gL, blk, 0, st, g, nL, list[1], dState, dCnt + 2 + t);
            }
            if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h.data() + 2, dCnt + 2, K * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) { rc = fail("rounds"); return; }
            ++out.hostChecks;
            uint32_t used = K;
            for (uint32_t t = 0; t < K; ++t)
                if (h[2 + t] == 0) { used = t + 1; done = true; break; }
            out.rounds += used;
        }
        // numbering and the rings
        hipLaunchKernelGGL(ag_flag_kernel, gridFor(M + 1), blk, 0, st, M, dState, dFlag);
        if (exclusiveScan(scanTmp, dFlag, dNumber, 0u, (size_t)M + 1, st) != hipSuccess) { rc = fail("scan"); return; }
        if (nS) hipLaunchKernelGGL((ag_ring1_kernel<I, false>), gS, blk, 0, st, g, nS, list[0], dState, dNumber, dAgg);
        if (nL) hipLaunchKernelGGL((ag_ring1_kernel<I, true>), gL, blk, 0, st, g, nL, list[1], dState, dNumber, dAgg);
        if (nS) hipLaunchKernelGGL((ag_ring2_kernel<I, false>), gS, blk, 0, st, g, seed, nS, list[0], dState, dAgg);
        if (nL) hipLaunchKernelGGL((ag_ring2_kernel<I, true>), gL, blk, 0, st, g, seed, nL, list[1], dState, dAgg);
        uint32_t nAgg = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&nAgg, dNumber + M, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { rc = fail("rings"); return; }
        out.aggregates = nAgg;
    });
    if (rc) return rc;
    // the largest and the smallest aggregate
    uint32_t mm[3] = {UNDECIDED, 0, 0};                        // smallest, largest, "an id out of range"
    if (size.alloc((out.aggregates + 3) * 4)) return fail("temporary allocation (aggregate sizes)");
    uint32_t* const dSize = size.as<uint32_t>();
    if (hipMemsetAsync(dSize, 0, out.aggregates * 4, st) != hipSuccess ||
        hipMemcpyAsync(dSize + out.aggregates, mm, 12, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail("aggregate sizes");
    hipLaunchKernelGGL(ag_hist_kernel, gridFor(M), dim3(AG_THREADS), 0, st, M, (uint32_t)out.aggregates, dAgg, dSize, dSize + out.aggregates + 2);
    hipLaunchKernelGGL(ag_minmax_kernel, gridFor(out.aggregates), dim3(AG_THREADS), 0, st, out.aggregates, dSize, dSize + out.aggregates);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(mm, dSize + out.aggregates, 12, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail("aggregate sizes");
    if (mm[2]) { fprintf(stderr, "libspmvhip: aggregate: a vertex was left without an aggregate\n"); return EXIT_FAILURE; }
    out.minAggRows = mm[0]; out.maxAggRows = mm[1];
    out.ms = msSince(t0);
    if (info) *info = out;
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
