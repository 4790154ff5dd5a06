// add.hip -- C = alpha A + beta B of two device CSR handles as a CSR handle of its own (spmvHipCsrAdd) and the recomputation
// of its values on the kept pattern (spmvHipCsrAddRefresh).  DESIGN.md section 25; the contract -- the bits of a serial loop
// -- is in spmvHip.h.
//
// An accumulator acc[i, j] starts at +0.0 and takes A's terms alpha * A.AS[p] of row i in stored order, then B's terms
// beta * B.AS[q]: each term a rounded product, then a plain add.  No floating-point atomic is used anywhere.
//   1. first pass: t[i] = len A(i) + len B(i), the PLAIN flag (both stored rows ascend strictly) and the check for column
//      ids >= N: a lane per row of at most 64 terms, a wavefront per longer row.  A row's class comes from t[i], the flag
//      and the options alone, is decided once and kept in three row lists (compaction, one atomic per wavefront and list:
//      the ORDER of a list depends on the run, no output does).
//   2. lane class (plain, t <= laneMaxTerms): a lane per row merges the two ascending rows with two pointers.
//   3. wave class (plain, t <= waveMaxTerms): a wavefront per row, 4 rows per workgroup, ranks instead of a merge -- the
//      "not in A" flags of B's row are prefix-counted into LDS (hB); entry p of A goes to p + hB[lower_bound_B(j)], a B-only
//      entry q to hB[q] + lower_bound_A(j).  A plain row has at most two terms per column, A's first: (0.0 + alpha a) + beta b.
//   4. sorted class (everything else: repeats, descents, longer rows, allSorted): the terms are expanded to
//      (row in batch << 32 | j, rounded term) in stored order, A's row then B's, and go through the sorted path that the
//      sparse product defines (device_prims.hpp): one stable radix sort per batch, runs added serially from +0.0.
// Every kernel of a row-list launch covers the count the host read; no kernel spins or waits on a flag.  A numeric kernel
// of the plain classes never writes outside the row of C it was given, and a refresh refuses sources whose entry counts
// are not the build's (the contract asks for unchanged patterns).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {

// what a sum handle keeps (DevMat::sum): the rows by class -- lane, wave, sorted
struct AddPlan {
    uint32_t* list = nullptr;                                  // nLane + nWave + nSorted rows (4 B per row at most)
    uint32_t nLane = 0, nWave = 0, nSorted = 0;
    uint64_t batchTerms = 0;                                   // terms of one batch of the sorted path
    uint64_t nzA = 0, nzB = 0;                                 // the sources' entries at the build: a refresh refuses others
    spmvAddInfo info{};
};

namespace {

constexpr uint32_t AD_THREADS = WG_THREADS;
constexpr uint32_t AD_LONG = 64;                               // terms of a row above which the first pass takes a wavefront
constexpr uint32_t AD_LANE_DEFAULT = 32, AD_LANE_LIMIT = 64;
constexpr uint32_t AD_WAVE_DEFAULT = 2048, AD_WAVE_LIMIT = 2048;   // hB: (LIMIT + 1) words per wavefront, 32 784 B per workgroup
constexpr uint32_t AD_NONE = 0xFFFFFFFFu;                      // no column: the dimension limit keeps it free
constexpr uint64_t AD_BUDGET = 256ull << 20, AD_BUDGET_MAX = 4ull << 30;
constexpr uint64_t AD_TERM_BYTES = 32;                         // keys in / out and values in / out of the sort

// ---------------------------------------------------------------------------------------------------- 1. first pass
// meta[r] = t << 1 | plain.  One stored row: its entries ascend strictly, and none is >= N (flag)
__device__ __forceinline__ bool ad_row_plain(const uint32_t* __restrict__ ja, uint64_t b, uint64_t e, uint64_t N, uint32_t* __restrict__ flag) {
    bool plain = true, bad = false;
    uint32_t prev = 0;
    for (uint64_t p = b; p < e; ++p) {
        const uint32_t j = ja[p];
        bad |= j >= N;
        plain &= p == b || j > prev;
        prev = j;
    }
    if (bad) atomicOr(flag, 1u);
    return plain;
}

// rows of at most 64 terms, a lane each; longer rows join longList (one atomic per wavefront)
template <typename IA, typename IB>
__global__ __launch_bounds__(AD_THREADS) void ad_first_kernel(uint64_t M, uint64_t N, const IA* __restrict__ irpA, const uint32_t* __restrict__ jaA,
                                                              const IB* __restrict__ irpB, const uint32_t* __restrict__ jaB,
                                                              uint64_t* __restrict__ meta, uint32_t* __restrict__ longList,
                                                              uint32_t* __restrict__ nLong, uint32_t* __restrict__ flag) {
    const uint64_t r = linear_block() * AD_THREADS + threadIdx.x;
    bool isLong = false;
    if (r < M) {
        const uint64_t ba = irpA[r], ea = irpA[r + 1], bb = irpB[r], eb = irpB[r + 1];
        const uint64_t t = (ea - ba) + (eb - bb);
        isLong = t > AD_LONG;
        if (!isLong) {
            const bool pa = ad_row_plain(jaA, ba, ea, N, flag), pb = ad_row_plain(jaB, bb, eb, N, flag);
            meta[r] = t << 1 | (uint64_t)(pa && pb);
        }
    }
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t bl = __ballot(isLong);
    uint32_t base = 0;
    if (lane == 0 && bl) base = atomicAdd(nLong, (uint32_t)__popcll(bl));
    base = __shfl(base, 0);
    if (isLong) longList[base + __popcll(bl & ((1ull << lane) - 1))] = (uint32_t)r;
}

// one stored row by a wavefront: true in every lane when it ascends strictly
__device__ __forceinline__ bool ad_row_plain_wave(const uint32_t* __restrict__ ja, uint64_t b, uint64_t e, uint64_t N, uint32_t lane,
                                                  uint32_t* __restrict__ flag) {
    bool ok = true, bad = false;
    for (uint64_t p = b + lane; p < e; p += 64) {
        const uint32_t j = ja[p];
        bad |= j >= N;
        ok &= p == b || ja[p - 1] < j;
    }
    if (bad) atomicOr(flag, 1u);
    return __ballot(!ok) == 0;
}

// the rows of `list`, a wavefront each
template <typename IA, typename IB>
__global__ __launch_bounds__(AD_THREADS) void ad_first_list_kernel(uint32_t n, const uint32_t* __restrict__ list, uint64_t N,
                                                                   const IA* __restrict__ irpA, const uint32_t* __restrict__ jaA,
                                                                   const IB* __restrict__ irpB, const uint32_t* __restrict__ jaB,
                                                                   uint64_t* __restrict__ meta, uint32_t* __restrict__ flag) {
    const uint64_t k = linear_block() * (AD_THREADS / 64) + threadIdx.x / 64;
    if (k >= n) return;
    const uint32_t lane = threadIdx.x % 64, r = list[k];
    const uint64_t ba = irpA[r], ea = irpA[r + 1], bb = irpB[r], eb = irpB[r + 1];
    const bool pa = ad_row_plain_wave(jaA, ba, ea, N, lane, flag), pb = ad_row_plain_wave(jaB, bb, eb, N, lane, flag);
    if (lane == 0) meta[r] = ((ea - ba) + (eb - bb)) << 1 | (uint64_t)(pa && pb);
}

// class of every row with a term: 0 lane, 1 wave, 2 sorted.  tot[0] += terms, tot[1] = max terms of a row
__global__ __launch_bounds__(AD_THREADS) void ad_classify_kernel(uint64_t M, const uint64_t* __restrict__ meta, uint64_t laneMax, uint64_t waveMax,
                                                                 int allSorted, uint32_t* __restrict__ lists, uint32_t* __restrict__ cnt,
                                                                 unsigned long long* __restrict__ tot) {
    const uint64_t r = linear_block() * AD_THREADS + threadIdx.x;
    const uint64_t m = r < M ? meta[r] : 0;
    const uint64_t t = m >> 1;
    const bool plain = (m & 1) && !allSorted;
    const int cls = t == 0 ? -1 : plain && t <= laneMax ? 0 : plain && t <= waveMax ? 1 : 2;
    const uint32_t lane = threadIdx.x % 64;
    for (int c = 0; c < 3; ++c) {
        const uint64_t bal = __ballot(cls == c);
        uint32_t base = 0;
        if (lane == 0 && bal) base = atomicAdd(&cnt[c], (uint32_t)__popcll(bal));
        base = __shfl(base, 0);
        if (cls == c) lists[(uint64_t)c * M + base + __popcll(bal & ((1ull << lane) - 1))] = (uint32_t)r;
    }
    uint64_t s = t, mx = t;
    for (int off = 32; off; off >>= 1) {
        s += __shfl_xor(s, off);
        const uint64_t o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    if (lane == 0 && s) { atomicAdd(&tot[0], (unsigned long long)s); atomicMax(&tot[1], (unsigned long long)mx); }
}

// ---------------------------------------------------------------------------------------------------- 2. lane class
// One lane per row of `rows`: the merge of two strictly ascending rows.  SYMBOLIC: counts[row] = the distinct columns.
// NUMERIC: the row of C at irpC[row] -- (0.0 + alpha a), then + beta b where the columns meet.
template <typename IA, typename IB, bool NUMERIC>
__global__ __launch_bounds__(AD_THREADS) void ad_lane_kernel(uint32_t nRows, const uint32_t* __restrict__ rows, double alpha,
                                                             const IA* __restrict__ irpA, const uint32_t* __restrict__ jaA,
                                                             const double* __restrict__ asA, double beta, const IB* __restrict__ irpB,
                                                             const uint32_t* __restrict__ jaB, const double* __restrict__ asB,
                                                             uint32_t* __restrict__ counts, const uint32_t* __restrict__ irpC,
                                                             uint32_t* __restrict__ jaC, double* __restrict__ asC) {
    const uint64_t k = linear_block() * AD_THREADS + threadIdx.x;
    if (k >= nRows) return;
    const uint32_t row = rows[k];
    uint64_t pa = irpA[row], pb = irpB[row];
    const uint64_t ea = irpA[row + 1], eb = irpB[row + 1];
    const uint32_t cBase = NUMERIC ? irpC[row] : 0, room = NUMERIC ? irpC[row + 1] - cBase : AD_NONE;
    uint32_t n = 0;
    uint32_t ja = pa < ea ? jaA[pa] : AD_NONE, jb = pb < eb ? jaB[pb] : AD_NONE;
    while ((pa < ea || pb < eb) && n < room) {
        const uint32_t j = ja < jb ? ja : jb;
        const bool inA = ja == j && pa < ea, inB = jb == j && pb < eb;
        if (NUMERIC) {
            double acc = 0.0;
            if (inA) acc = acc + alpha * asA[pa];              // rounded product, then the add: the library is built with contraction off
            if (inB) acc = acc + beta * asB[pb];
            jaC[cBase + n] = j;
            asC[cBase + n] = acc;
        }
        ++n;
        if (inA) { ++pa; ja = pa < ea ? jaA[pa] : AD_NONE; }
        if (inB) { ++pb; jb = pb < eb ? jaB[pb] : AD_NONE; }
    }
    if (!NUMERIC) counts[row] = n;
}

// ---------------------------------------------------------------------------------------------------- 3. wave class
// the first index in [0, len) of the ascending ja[base ..] whose column is >= j, or len
__device__ __forceinline__ uint32_t ad_lower_bound(const uint32_t* __restrict__ ja, uint64_t base, uint32_t len, uint32_t j) {
    uint32_t lo = 0, hi = len;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ja[base + mid] < j) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One wavefront per row of `rows`, AD_THREADS / 64 rows per workgroup, no workgroup barrier.
template <typename IA, typename IB, bool NUMERIC>
__global__ __launch_bounds__(AD_THREADS) void ad_wave_kernel(uint32_t nRows, const uint32_t* __restrict__ rows, double alpha,
                                                             const IA* __restrict__ irpA, const uint32_t* __restrict__ jaA,
                                                             const double* __restrict__ asA, double beta, const IB* __restrict__ irpB,
                                                             const uint32_t* __restrict__ jaB, const double* __restrict__ asB,
                                                             uint32_t* __restrict__ counts, const uint32_t* __restrict__ irpC,
                                                             uint32_t* __restrict__ jaC, double* __restrict__ asC) {
    constexpr int TEAMS = AD_THREADS / 64;
    __shared__ uint32_t hBS[NUMERIC ? TEAMS : 1][NUMERIC ? AD_WAVE_LIMIT + 1 : 1];
    const uint32_t team = threadIdx.x / 64, lane = threadIdx.x % 64;
    const uint64_t k = linear_block() * TEAMS + team;
    if (k >= nRows) return;                                    // uniform in a wavefront
    const uint32_t row = rows[k];
    const uint64_t bA = irpA[row], bB = irpB[row];
    const uint64_t lA = (uint64_t)irpA[row + 1] - bA, lB = (uint64_t)irpB[row + 1] - bB;
    if (lA + lB > AD_WAVE_LIMIT) return;                       // (sources whose pattern changed under a refresh: hB holds no more)
    const uint32_t lenA = (uint32_t)lA, lenB = (uint32_t)lB;
    volatile uint32_t* const hB = hBS[NUMERIC ? team : 0];
    // hB[q] = the entries of B's row before q that A's row does not hold
    uint32_t onlyB = 0;
    for (uint32_t base = 0; base < lenB; base += 64) {
        const uint32_t q = base + lane;
        bool only = false;
        if (q < lenB) {
            const uint32_t j = jaB[bB + q], at = ad_lower_bound(jaA, bA, lenA, j);
            only = at == lenA || jaA[bA + at] != j;
        }
        const uint64_t bal = __ballot(only);
        if (NUMERIC && q < lenB) hB[q] = onlyB + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
        onlyB += (uint32_t)__popcll(bal);
    }
    if (!NUMERIC) {
        if (lane == 0) counts[row] = lenA + onlyB;
        return;
    }
    if (lane == 0) hB[lenB] = onlyB;
    team_sync<64>();
    const uint32_t cBase = irpC[row], room = irpC[row + 1] - cBase;
    for (uint32_t p = lane; p < lenA; p += 64) {
        const uint32_t j = jaA[bA + p], at = ad_lower_bound(jaB, bB, lenB, j);
        double acc = 0.0;
        acc = acc + alpha * asA[bA + p];
        if (at < lenB && jaB[bB + at] == j) acc = acc + beta * asB[bB + at];
        const uint32_t pos = p + hB[at];
        if (pos < room) { jaC[cBase + pos] = j; asC[cBase + pos] = acc; }
    }
    for (uint32_t q = lane; q < lenB; q += 64) {
        const uint32_t j = jaB[bB + q], at = ad_lower_bound(jaA, bA, lenA, j);
        if (at < lenA && jaA[bA + at] == j) continue;
        double acc = 0.0;
        acc = acc + beta * asB[bB + q];
        const uint32_t pos = hB[q] + at;
        if (pos < room) { jaC[cBase + pos] = j; asC[cBase + pos] = acc; }
    }
}

// ---------------------------------------------------------------------------------------------------- 4. sorted class
// terms[k] = the terms of row list[k]
template <typename IA, typename IB>
__global__ __launch_bounds__(AD_THREADS) void ad_terms_kernel(uint32_t n, const uint32_t* __restrict__ list, const IA* __restrict__ irpA,
                                                              const IB* __restrict__ irpB, uint64_t* __restrict__ terms) {
    const uint64_t k = linear_block() * AD_THREADS + threadIdx.x;
    if (k >= n) return;
    const uint32_t r = list[k];
    terms[k] = ((uint64_t)irpA[r + 1] - (uint64_t)irpA[r]) + ((uint64_t)irpB[r + 1] - (uint64_t)irpB[r]);
}

// rows list[b], b < nRows, a wavefront each: term f of the row -- A's row as stored, then B's -- goes to off[b] - off[0] + f.
// The room of a row is what the host sized the batch by (off[b + 1] - off[b]).
template <typename IA, typename IB, bool NUMERIC>
__global__ __launch_bounds__(AD_THREADS) void ad_expand_kernel(uint32_t nRows, const uint32_t* __restrict__ list, const uint64_t* __restrict__ off,
                                                               double alpha, const IA* __restrict__ irpA, const uint32_t* __restrict__ jaA,
                                                               const double* __restrict__ asA, double beta, const IB* __restrict__ irpB,
                                                               const uint32_t* __restrict__ jaB, const double* __restrict__ asB,
                                                               uint64_t* __restrict__ key, double* __restrict__ val) {
    const uint64_t b = linear_block() * (AD_THREADS / 64) + threadIdx.x / 64;
    if (b >= nRows) return;
    const uint32_t lane = threadIdx.x % 64, row = list[b];
    const uint64_t out = off[b] - off[0], room = off[b + 1] - off[b];
    const uint64_t bA = irpA[row], bB = irpB[row];
    const uint64_t lenA = (uint64_t)irpA[row + 1] - bA, lenB = (uint64_t)irpB[row + 1] - bB;
    if (lenA + lenB != room) return;                           // (the row pointers changed between the count and this launch)
    for (uint64_t f = lane; f < lenA; f += 64) {
        key[out + f] = b << 32 | jaA[bA + f];
        if (NUMERIC) val[out + f] = alpha * asA[bA + f];
    }
    for (uint64_t f = lane; f < lenB; f += 64) {
        key[out + lenA + f] = b << 32 | jaB[bB + f];
        if (NUMERIC) val[out + lenA + f] = beta * asB[bB + f];
    }
}

// ---------------------------------------------------------------------------------------------------- host side
struct Run {
    const DevMat *a, *b;
    double alpha, beta;
    AddPlan* plan;
    hipStream_t st;
    TempTally tm;                                              // every temporary of the call counts into it: tempBytes = its peak
    SortedPath sp{"add", "terms", &tm};                        // the terms before each sorted row, and the batches of the list
};

int fail(hipStream_t st, const char* what) { return buildFail(st, "add", what); }

// the two plain classes over their lists
template <bool NUMERIC>
int plainPass(Run& r, uint32_t* counts, DevMat* c) {
    const AddPlan* pl = r.plan;
    const uint32_t* irpC = c ? static_cast<const uint32_t*>(c->IRP) : nullptr;
    uint32_t* jaC = c ? c->JA : nullptr;
    double* asC = c ? c->AS : nullptr;
    withBoth(r.a, r.b, [&](auto ia, auto ib) {
        using IA = IrpT<decltype(ia)>;
        using IB = IrpT<decltype(ib)>;
        if (pl->nLane)
            hipLaunchKernelGGL((ad_lane_kernel<IA, IB, NUMERIC>), gridFor(pl->nLane), dim3(AD_THREADS), 0, r.st, pl->nLane, pl->list, r.alpha, ia,
                               r.a->JA, r.a->AS, r.beta, ib, r.b->JA, r.b->AS, counts, irpC, jaC, asC);
        if (pl->nWave)
            hipLaunchKernelGGL((ad_wave_kernel<IA, IB, NUMERIC>), gridFor(pl->nWave, AD_THREADS / 64), dim3(AD_THREADS), 0, r.st, pl->nWave,
                               pl->list + pl->nLane, r.alpha, ia, r.a->JA, r.a->AS, r.beta, ib, r.b->JA, r.b->AS, counts, irpC, jaC, asC);
        return 0;
    });
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : fail(r.st, "plain class kernels");
}

// the terms before every row of the sorted list, and its batches
int sortedPrepare(Run& r) {
    const AddPlan* pl = r.plan;
    const uint32_t n = pl->nSorted;
    if (!n) return EXIT_SUCCESS;
    const uint32_t* list = pl->list + pl->nLane + pl->nWave;
    TempBuf terms(&r.tm);
    if (terms.alloc(((size_t)n + 1) * 8)) return fail(r.st, "temporary allocation (sorted rows)");
    if (hipMemsetAsync(terms.p, 0, ((size_t)n + 1) * 8, r.st) != hipSuccess) return fail(r.st, "memset");
    withBoth(r.a, r.b, [&](auto ia, auto ib) {
        hipLaunchKernelGGL((ad_terms_kernel<IrpT<decltype(ia)>, IrpT<decltype(ib)>>), gridFor(n), dim3(AD_THREADS), 0, r.st, n, list, ia, ib,
                           terms.as<uint64_t>());
        return 0;
    });
    return sortedBatches(r.sp, terms.as<uint64_t>(), n, pl->batchTerms, r.st);
}

// this file's half of the sorted path: the expansion
template <bool NUMERIC>
int sortedClass(Run& r, uint32_t* counts, DevMat* c) {
    const AddPlan* pl = r.plan;
    if (!pl->nSorted) return EXIT_SUCCESS;
    const uint32_t* list = pl->list + pl->nLane + pl->nWave;
    return sortedPass(r.sp, NUMERIC, list, [&](uint32_t k0, uint32_t nRows, const uint64_t* off, uint64_t* key, double* val) {
        withBoth(r.a, r.b, [&](auto ia, auto ib) {
            hipLaunchKernelGGL((ad_expand_kernel<IrpT<decltype(ia)>, IrpT<decltype(ib)>, NUMERIC>), gridFor(nRows, AD_THREADS / 64), dim3(AD_THREADS),
                               0, r.st, nRows, list + k0, off, r.alpha, ia, r.a->JA, r.a->AS, r.beta, ib, r.b->JA, r.b->AS, key, val);
            return 0;
        });
    }, counts, c, r.st);
}

int numericPhase(Run& r, DevMat* c) {
    if (plainPass<true>(r, nullptr, c) || sortedClass<true>(r, nullptr, c)) return EXIT_FAILURE;
    if (hipStreamSynchronize(r.st) != hipSuccess) return fail(r.st, "numeric phase");
    return EXIT_SUCCESS;
}

}  // namespace

void freeAddPlan(AddPlan* p) {
    if (!p) return;
    (void)devFree(p->list);
    delete p;
}

// c: kind, M and N set by the caller, nothing allocated.  On success c owns IRP (4 B), JA, AS and the plan, and c->NZ is
// set; on failure the caller frees c with whatever it holds.  nnz(C) >= IRP32_LIMIT and a column id >= N are found before
// JA / AS exist.
int addBuild(double alpha, const DevMat* a, double beta, const DevMat* b, const spmvAddOpts* opts, DevMat* c, spmvAddInfo* info,
             hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t M = a->M, N = a->N;
    AddPlan* pl = c->sum = new AddPlan;
    const uint64_t laneMax = clampOpt(opts ? opts->laneMaxTerms : 0, AD_LANE_DEFAULT, AD_LANE_LIMIT);
    const uint64_t waveMax = clampOpt(opts ? opts->waveMaxTerms : 0, AD_WAVE_DEFAULT, AD_WAVE_LIMIT);
    pl->batchTerms = std::max<uint64_t>(clampOpt(opts ? opts->sortBudgetBytes : 0, AD_BUDGET, AD_BUDGET_MAX) / AD_TERM_BYTES, 1);
    pl->nzA = a->NZ; pl->nzB = b->NZ;
    spmvAddInfo out{};
    Run r{a, b, alpha, beta, pl, st};
    if (devMalloc(&c->IRP, (M + 1) * 4) != hipSuccess) return fail(st, "allocation of the row pointers");
    c->irpBytes = 4;
    uint64_t nnzC = 0;
    if (M && (a->NZ || b->NZ)) {
        // 1. the first pass, the classes, the lists
        TempBuf meta(&r.tm), lists(&r.tm), longList(&r.tm), cnt(&r.tm), tot(&r.tm);
        const bool longRows = a->maxRowNnz + b->maxRowNnz > AD_LONG;
        if (meta.alloc(M * 8) || lists.alloc(M * 12) || cnt.alloc(5 * 4) || tot.alloc(16) || (longRows && longList.alloc(M * 4)))
            return fail(st, "temporary allocation (20 B per row)");
        uint32_t* const dCnt = cnt.as<uint32_t>();           // [0..2] rows of a class, [3] long rows, [4] a column id out of range
        if (hipMemsetAsync(dCnt, 0, 5 * 4, st) != hipSuccess || hipMemsetAsync(tot.p, 0, 16, st) != hipSuccess) return fail(st, "memset");
        uint32_t h[5] = {0, 0, 0, 0, 0};
        withBoth(a, b, [&](auto ia, auto ib) {
            hipLaunchKernelGGL((ad_first_kernel<IrpT<decltype(ia)>, IrpT<decltype(ib)>>), gridFor(M), dim3(AD_THREADS), 0, st, M, N, ia, a->JA, ib, b->JA,
                               meta.as<uint64_t>(), longList.as<uint32_t>(), dCnt + 3, dCnt + 4);
            return 0;
        });
        if (longRows) {
            if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, dCnt, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return fail(st, "first pass");
            if (h[3])
                withBoth(a, b, [&](auto ia, auto ib) {
                    hipLaunchKernelGGL((ad_first_list_kernel<IrpT<decltype(ia)>, IrpT<decltype(ib)>>), gridFor(h[3], AD_THREADS / 64), dim3(AD_THREADS),
                                       0, st, h[3], longList.as<uint32_t>(), N, ia, a->JA, ib, b->JA, meta.as<uint64_t>(), dCnt + 4);
                    return 0;
                });
        }
        hipLaunchKernelGGL(ad_classify_kernel, gridFor(M), dim3(AD_THREADS), 0, st, M, meta.as<uint64_t>(), laneMax, waveMax,
                           opts && opts->allSorted ? 1 : 0, lists.as<uint32_t>(), dCnt, tot.as<unsigned long long>());
        unsigned long long hTot[2] = {0, 0};
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, dCnt, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(hTot, tot.p, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "classification");
        if (h[4]) { fprintf(stderr, "libspmvhip: add: a column id of a source is >= N\n"); return EXIT_FAILURE; }
        pl->nLane = h[0]; pl->nWave = h[1]; pl->nSorted = h[2];
        out.terms = hTot[0]; out.maxRowTerms = hTot[1];
        const size_t nList = (size_t)h[0] + h[1] + h[2];
        if (devMalloc(&pl->list, std::max<size_t>(nList, 1) * 4) != hipSuccess) return fail(st, "allocation of the class lists");
        for (int cl = 0, at = 0; cl < 3; at += h[cl], ++cl)
            if (h[cl] && hipMemcpyAsync(pl->list + at, lists.as<uint32_t>() + (size_t)cl * M, (size_t)h[cl] * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
                return fail(st, "class lists");
        if (hipStreamSynchronize(st) != hipSuccess) return fail(st, "class lists");
        meta.release(); lists.release(); longList.release();
        // 2. symbolic: the counts, their scan, the row pointers
        TempBuf counts(&r.tm), irp64(&r.tm), scanTmp(&r.tm);
        if (counts.alloc((M + 1) * 4) || irp64.alloc((M + 1) * 8)) return fail(st, "temporary allocation (12 B per row)");
        if (hipMemsetAsync(counts.p, 0, (M + 1) * 4, st) != hipSuccess || hipMemsetAsync(dCnt, 0, 4, st) != hipSuccess) return fail(st, "memset");
        if (sortedPrepare(r) || plainPass<false>(r, counts.as<uint32_t>(), nullptr) || sortedClass<false>(r, counts.as<uint32_t>(), nullptr))
            return EXIT_FAILURE;
        if (exclusiveScan(scanTmp, counts.as<uint32_t>(), irp64.as<uint64_t>(), (uint64_t)0, (size_t)M + 1, st) != hipSuccess) return fail(st, "scan");
        if (hipMemcpyAsync(&nnzC, irp64.as<uint64_t>() + M, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "row pointers");
        if (nnzC >= IRP32_LIMIT) {
            fprintf(stderr, "libspmvhip: add: nnz(C) = %lu: the row pointers of the sum are 32-bit (limit %lu)\n", (unsigned long)nnzC,
                    (unsigned long)IRP32_LIMIT);
            return EXIT_FAILURE;
        }
        uint32_t maxLen = 0;
        enqueueNarrowIrp(M, irp64.as<uint64_t>(), static_cast<uint32_t*>(c->IRP), dCnt, st);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&maxLen, dCnt, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "row pointers");
        out.maxRowNnz = maxLen;
    } else if (hipMemsetAsync(c->IRP, 0, (M + 1) * 4, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        return fail(st, "row pointers");
    }
    out.symbolicMs = msSince(t0);
    // 3. numeric
    const auto t1 = std::chrono::steady_clock::now();
    c->NZ = nnzC;
    if (devMalloc(&c->JA, std::max<uint64_t>(nnzC, 1) * 4) != hipSuccess || devMalloc(&c->AS, std::max<uint64_t>(nnzC, 1) * 8) != hipSuccess)
        return fail(st, "allocation of the sum's arrays");
    if (numericPhase(r, c)) return EXIT_FAILURE;
    out.numericMs = msSince(t1);
    out.nnzC = nnzC;
    out.rowsLane = pl->nLane; out.rowsWave = pl->nWave; out.rowsSorted = pl->nSorted;
    out.sortBatches = r.sp.batches();
    out.tempBytes = r.tm.peak;
    out.ms = msSince(t0);
    pl->info = out;
    if (info) *info = out;
    return EXIT_SUCCESS;
}

// the numeric phase again, on the kept lists, into c's arrays
int addRefresh(DevMat* c, double alpha, const DevMat* a, double beta, const DevMat* b, spmvAddInfo* info, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    AddPlan* pl = c->sum;
    if (a->NZ != pl->nzA || b->NZ != pl->nzB) { fprintf(stderr, "libspmvhip: add: a source has other entries than at the build\n"); return EXIT_FAILURE; }
    Run r{a, b, alpha, beta, pl, st};
    if (sortedPrepare(r) || numericPhase(r, c)) return EXIT_FAILURE;
    spmvAddInfo out = pl->info;
    out.symbolicMs = 0;
    out.numericMs = out.ms = msSince(t0);
    out.sortBatches = r.sp.batches();
    out.tempBytes = r.tm.peak;
    pl->info = out;
    if (info) *info = out;
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
