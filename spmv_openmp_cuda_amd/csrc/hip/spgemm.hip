// spgemm.hip -- C = A B of two device CSR handles as a CSR handle of its own (spmvHipSpGEMM) and the recomputation of its
// values on the kept pattern (spmvHipSpGEMMRefresh).  DESIGN.md section 22; the contract -- the bits of a serial loop -- is
// in spmvHip.h.
//
// The order is the difficulty: an accumulator acc[i, j] takes its terms in (p, q) order, p over A's row i and q over B's row
// JA[p], both as stored.  No floating-point atomic is used anywhere; every sum is a chain of plain adds in that order.
//   1. upper bound  ub[i] = sum over p of len(B row JA[p]): a lane per row of at most 64 entries, a wavefront per longer
//      row.  A row's class comes from min(ub[i], B.N) alone, is decided once and kept in three row lists (compaction, one
//      atomic per wavefront and list: the ORDER of a list depends on the run, no output does).
//   2. hash classes in LDS (open addressing, linear probing, multiplicative hash, empty key 0xFFFFFFFF): a wavefront per
//      row (4 rows per workgroup, 1024 slots each) or a workgroup per row (8192 slots).  Symbolic: integer CAS inserts,
//      the inserts that found the slot empty are counted.  Numeric: the row's products flattened in (p, q) order are taken
//      T at a time, lane t owning product base + t; the adds of a batch run in ORDERED ROUNDS -- every pending lane does
//      atomicMin(owner[slot], t), the lane that owns the slot does a plain val[slot] += product and resets the owner --
//      so a slot takes a batch's terms in ascending flattened index, and batches follow one another.  Then the table is
//      compacted and sorted by column (rank by counting for short rows, bitonic over the table otherwise).
//   3. sorted path (rows above the group class, and whatever the options send there): batches of rows whose products fit
//      the budget are expanded to (row in batch << 32 | j, product) in (p, q) order and sorted by ONE stable
//      radix sort; a wavefront per row counts the run heads (symbolic) or lets one lane per head add its run
//      serially from +0.0 (numeric).  The symbolic phase keeps nothing but the counts; the numeric phase expands again.
// Every kernel of a row-list launch covers the count the host read; no kernel spins or waits on a flag.
// The batching, the sort and the run kernel of the sorted path, and the narrowing of the row pointers, are what the sparse
// sum (add.hip) needs too: they are declared in device_prims.hpp and defined here, once; the expansion is each caller's own.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <vector>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {

// what a product handle keeps (DevMat::prod): the rows by class -- wave, group, sorted
struct SpgemmPlan {
    uint32_t* list = nullptr;                                  // nWave + nGroup + nSorted rows (4 B per row at most)
    uint32_t nWave = 0, nGroup = 0, nSorted = 0;
    uint64_t batchProducts = 0;                                // products of one batch of the sorted path
    spmvSpgemmInfo info{};
};

namespace {

constexpr uint32_t SG_THREADS = WG_THREADS;                    // (what gridFor deals to by default)
constexpr uint32_t SG_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t SG_LONG = 64;                               // entries of A's row above which the bound takes a wavefront
constexpr uint32_t SG_WAVE_SLOTS = 1024, SG_WAVE_MAX = 512;    // min(ub, B.N) <= MAX: the table can never fill
constexpr uint32_t SG_GROUP_SLOTS = 8192, SG_GROUP_MAX = 6144;
constexpr uint32_t SG_WAVE_RANK = 128, SG_GROUP_RANK = 512;    // rows of at most this many entries are ranked by counting
constexpr uint64_t SG_BUDGET = 256ull << 20, SG_BUDGET_MAX = 4ull << 30;
constexpr uint64_t SG_PRODUCT_BYTES = 32;                      // keys in / out and values in / out of the sort

// ---------------------------------------------------------------------------------------------------- 1. upper bound
template <typename IB>
__device__ __forceinline__ uint64_t sg_b_len(uint32_t k, uint64_t BM, const IB* __restrict__ irpB, uint32_t* __restrict__ flag) {
    if (k >= BM) { atomicOr(flag, 1u); return 0; }            // a column of A with no row of B: the call is refused
    return (uint64_t)irpB[k + 1] - (uint64_t)irpB[k];
}

// rows of at most 64 entries, a lane each; longer rows join longList (one atomic per wavefront)
template <typename IA, typename IB>
__global__ __launch_bounds__(SG_THREADS) void sg_ub_short_kernel(uint64_t M, const IA* __restrict__ irpA, const uint32_t* __restrict__ jaA,
                                                                 const IB* __restrict__ irpB, uint64_t BM, uint64_t* __restrict__ ub,
                                                                 uint32_t* __restrict__ longList, uint32_t* __restrict__ nLong,
                                                                 uint32_t* __restrict__ flag) {
    const uint64_t r = linear_block() * SG_THREADS + threadIdx.x;
    const bool live = r < M;
    bool isLong = false;
    if (live) {
        const uint64_t b = irpA[r], e = irpA[r + 1];
        isLong = e - b > SG_LONG;
        if (!isLong) {
            uint64_t s = 0;
            for (uint64_t p = b; p < e; ++p) s += sg_b_len(jaA[p], BM, irpB, flag);
            ub[r] = s;
        }
    }
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t bl = __ballot(isLong);
    uint32_t base = 0;
    if (lane == 0 && bl) base = atomicAdd(nLong, (uint32_t)__popcll(bl));
    base = __shfl(base, 0);
    if (isLong) longList[base + __popcll(bl & ((1ull << lane) - 1))] = (uint32_t)r;
}

// the rows of `list`, a wavefront each (integer sums: any order)
template <typename IA, typename IB>
__global__ __launch_bounds__(SG_THREADS) void sg_ub_list_kernel(uint32_t n, const uint32_t* __restrict__ list, const IA* __restrict__ irpA,
                                                                const uint32_t* __restrict__ jaA, const IB* __restrict__ irpB, uint64_t BM,
                                                                uint64_t* __restrict__ ub, bool byRow, uint32_t* __restrict__ flag) {
    const uint64_t k = linear_block() * (SG_THREADS / 64) + threadIdx.x / 64;
    if (k >= n) return;
    const uint32_t lane = threadIdx.x % 64, r = list[k];
    uint64_t s = 0;
    for (uint64_t p = (uint64_t)irpA[r] + lane, e = irpA[r + 1]; p < e; p += 64) s += sg_b_len(jaA[p], BM, irpB, flag);
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) ub[byRow ? r : k] = s;                      // indexed by the row, or by the place in the list
}

// class of every row with a product: 0 wave, 1 group, 2 sorted.  tot[0] += products, tot[1] = max products of a row
__global__ __launch_bounds__(SG_THREADS) void sg_classify_kernel(uint64_t M, const uint64_t* __restrict__ ub, uint64_t BN, uint64_t waveMax,
                                                                 uint64_t groupMax, uint32_t* __restrict__ lists, uint32_t* __restrict__ cnt,
                                                                 unsigned long long* __restrict__ tot) {
    const uint64_t r = linear_block() * SG_THREADS + threadIdx.x;
    const uint64_t u = r < M ? ub[r] : 0;
    const uint64_t m = u < BN ? u : BN;
    const int cls = u == 0 ? -1 : m <= waveMax ? 0 : m <= groupMax ? 1 : 2;
    const uint32_t lane = threadIdx.x % 64;
    for (int c = 0; c < 3; ++c) {
        const uint64_t bal = __ballot(cls == c);
        uint32_t base = 0;
        if (lane == 0 && bal) base = atomicAdd(&cnt[c], (uint32_t)__popcll(bal));
        base = __shfl(base, 0);
        if (cls == c) lists[(uint64_t)c * M + base + __popcll(bal & ((1ull << lane) - 1))] = (uint32_t)r;
    }
    uint64_t s = u, mx = u;
    for (int off = 32; off; off >>= 1) {
        s += __shfl_xor(s, off);
        const uint64_t o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    if (lane == 0 && s) { atomicAdd(&tot[0], (unsigned long long)s); atomicMax(&tot[1], (unsigned long long)mx); }
}

// IRP of C from the 64-bit scan of the counts, and the longest row
__global__ __launch_bounds__(SG_THREADS) void sg_narrow_kernel(uint64_t M, const uint64_t* __restrict__ irp64, uint32_t* __restrict__ irp,
                                                               uint32_t* __restrict__ maxLen) {
    const uint64_t r = linear_block() * SG_THREADS + threadIdx.x;
    if (r > M) return;
    irp[r] = (uint32_t)irp64[r];
    if (r < M) atomicMax(maxLen, (uint32_t)(irp64[r + 1] - irp64[r]));
}

// ------------------------------------------------------------------------------------------ the products of a row, in order
// A team is the T lanes that share a row: a wavefront or the workgroup (team_sync of device_prims.hpp).
template <int T> __device__ __forceinline__ bool team_any(bool v) {
    if constexpr (T == 64) {
        const bool r = __ballot(v) != 0;
        team_sync<64>();
        return r;
    } else {
        return __syncthreads_or(v) != 0;
    }
}

// per team: the prefix sums of the B-row lengths of up to T entries of A's row, their first positions in B and A's values
template <int T> struct Stage {
    uint64_t pfx[T + 1];
    uint64_t bst[T];
    double   av[T];
};

// stages the entries [p0, min(p0 + T, pe)) of A's row; returns their number of products.  Ends synchronised.
template <int T, bool VALUES, typename IB>
__device__ __forceinline__ uint64_t sg_stage(Stage<T>& st, uint32_t t, uint64_t p0, uint64_t pe, const uint32_t* __restrict__ jaA,
                                             const double* __restrict__ asA, const IB* __restrict__ irpB, uint64_t BM) {
    team_sync<T>();                                            // the previous chunk's readers are done
    const uint64_t p = p0 + t;
    uint64_t len = 0, bs = 0;
    double v = 0.0;
    if (p < pe) {
        const uint32_t k = jaA[p];
        if (k < BM) { bs = irpB[k]; len = (uint64_t)irpB[k + 1] - bs; }
        if (VALUES) v = asA[p];
    }
    st.bst[t] = bs;
    st.av[t] = v;
    st.pfx[t + 1] = len;
    if (t == 0) st.pfx[0] = 0;
    team_sync<T>();
    for (uint32_t d = 1; d < (uint32_t)T; d <<= 1) {
        const uint64_t add = t >= d ? st.pfx[t + 1 - d] : 0;
        team_sync<T>();
        st.pfx[t + 1] += add;
        team_sync<T>();
    }
    return st.pfx[T];
}

// the entry of the chunk that product f of it belongs to: the largest e with pfx[e] <= f (f < pfx[T])
template <int T> __device__ __forceinline__ uint32_t sg_find(const Stage<T>& st, uint64_t f) {
    uint32_t lo = 0, hi = T;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (st.pfx[mid] <= f) lo = mid; else hi = mid;
    }
    return lo;
}

template <uint32_t SLOTS> __device__ __forceinline__ uint32_t sg_hash(uint32_t j) {
    return (j * 0x9E3779B1u) >> (32 - __builtin_ctz(SLOTS));
}

// ---------------------------------------------------------------------------------------------------- 2. hash classes
// One team per row of `rows`.  SYMBOLIC: counts[row] = the distinct columns.  NUMERIC: the row of C at irpC[row].
template <typename IA, typename IB, int T, uint32_t SLOTS, uint32_t RANK, bool NUMERIC>
__global__ __launch_bounds__(SG_THREADS) void sg_hash_kernel(uint32_t nRows, const uint32_t* __restrict__ rows, const IA* __restrict__ irpA,
                                                             const uint32_t* __restrict__ jaA, const double* __restrict__ asA,
                                                             const IB* __restrict__ irpB, const uint32_t* __restrict__ jaB,
                                                             const double* __restrict__ asB, uint64_t BM, uint32_t* __restrict__ counts,
                                                             const uint32_t* __restrict__ irpC, uint32_t* __restrict__ jaC,
                                                             double* __restrict__ asC) {
    constexpr int TEAMS = SG_THREADS / T;
    constexpr uint32_t MASK = SLOTS - 1;
    __shared__ uint32_t keysS[TEAMS][SLOTS];
    __shared__ double   valsS[NUMERIC ? TEAMS : 1][NUMERIC ? SLOTS : 1];
    __shared__ uint32_t ownerS[NUMERIC ? TEAMS : 1][NUMERIC ? SLOTS : 1];
    __shared__ Stage<T> stageS[TEAMS];
    __shared__ uint32_t cntS[TEAMS];
    const uint32_t team = threadIdx.x / T, t = threadIdx.x % T;
    const uint64_t k = linear_block() * TEAMS + team;
    if (k >= nRows) return;                                    // uniform in a team; a wavefront team uses no workgroup barrier
    const uint32_t row = rows[k];
    uint32_t* const keys = keysS[team];
    volatile double* const vals = valsS[NUMERIC ? team : 0];
    volatile uint32_t* const owner = ownerS[NUMERIC ? team : 0];
    Stage<T>& st = stageS[team];
    for (uint32_t s = t; s < SLOTS; s += T) {
        keys[s] = SG_EMPTY;
        if (NUMERIC) { vals[s] = 0.0; owner[s] = SG_EMPTY; }
    }
    if (t == 0) cntS[team] = 0;
    uint32_t fresh = 0;
    const uint64_t pe = irpA[row + 1];
    for (uint64_t p0 = irpA[row]; p0 < pe; p0 += T) {
        const uint64_t total = sg_stage<T, NUMERIC>(st, t, p0, pe, jaA, asA, irpB, BM);
        for (uint64_t base = 0; base < total; base += T) {
            const uint64_t f = base + t;
            bool pending = f < total;
            uint32_t slot = 0;
            double prod = 0.0;
            if (pending) {
                const uint32_t e = sg_find<T>(st, f);
                const uint64_t q = st.bst[e] + (f - st.pfx[e]);
                const uint32_t j = jaB[q];
                if (NUMERIC) prod = st.av[e] * asB[q];         // rounded here: the library is built with contraction off
                slot = sg_hash<SLOTS>(j);
                uint32_t tries = 0;                            // (a table never fills: the class limit is below its slots)
                for (; tries < SLOTS; ++tries) {
                    const uint32_t was = atomicCAS(&keys[slot], SG_EMPTY, j);
                    if (was == SG_EMPTY) { ++fresh; break; }
                    if (was == j) break;
                    slot = (slot + 1) & MASK;
                }
                if (tries == SLOTS) pending = false;           // sources whose pattern changed under a refresh: no endless probe
            }
            if (NUMERIC) {
                // ordered rounds: of the lanes that want a slot, the smallest t adds; the others try again
                do {
                    if (pending) atomicMin(const_cast<uint32_t*>(&owner[slot]), t);
                    team_sync<T>();
                    if (pending && owner[slot] == t) {
                        vals[slot] = vals[slot] + prod;
                        owner[slot] = SG_EMPTY;
                        pending = false;
                    }
                } while (team_any<T>(pending));
            }
        }
    }
    if (!NUMERIC) {
        if (T == 64) {
            for (int off = 32; off; off >>= 1) fresh += __shfl_xor(fresh, off);
            if (t == 0) counts[row] = fresh;
        } else {
            team_sync<T>();
            if (fresh) atomicAdd(&cntS[team], fresh);
            team_sync<T>();
            if (t == 0) counts[row] = cntS[team];
        }
        return;
    }
    // the row of C: ascending column.  owner[] now lists the occupied slots (in any order: the rank decides the place)
    team_sync<T>();
    const uint32_t cBase = irpC[row], n = irpC[row + 1] - cBase;
    if (n <= RANK) {
        for (uint32_t s = t; s < SLOTS; s += T)
            if (keys[s] != SG_EMPTY) owner[atomicAdd(&cntS[team], 1u)] = s;
        team_sync<T>();
        for (uint32_t e = t; e < n; e += T) {
            const uint32_t s = owner[e], j = keys[s];
            uint32_t rank = 0;
            for (uint32_t o = 0; o < n; ++o) rank += keys[owner[o]] < j;
            jaC[cBase + rank] = j;
            asC[cBase + rank] = vals[s];
        }
        return;
    }
    // bitonic over the whole table: the empty key is the largest, so the row ends up in the first n slots
    for (uint32_t span = 2; span <= SLOTS; span <<= 1)
        for (uint32_t d = span >> 1; d; d >>= 1) {
            for (uint32_t i = t; i < SLOTS; i += T) {
                const uint32_t o = i ^ d;
                if (o <= i) continue;
                const uint32_t ki = keys[i], ko = keys[o];
                if ((ki > ko) == ((i & span) == 0)) {
                    keys[i] = ko; keys[o] = ki;
                    const double vi = vals[i], vo = vals[o];
                    vals[i] = vo; vals[o] = vi;
                }
            }
            team_sync<T>();
        }
    for (uint32_t e = t; e < n; e += T) {
        jaC[cBase + e] = keys[e];
        asC[cBase + e] = vals[e];
    }
}

// ---------------------------------------------------------------------------------------------------- 3. sorted path
// rows list[k0 + b], b < nRows, a workgroup each: product f of the row goes to off[k0 + b] - off[k0] + f
template <typename IA, typename IB, bool NUMERIC>
__global__ __launch_bounds__(SG_THREADS) void sg_expand_kernel(uint32_t nRows, const uint32_t* __restrict__ list, const uint64_t* __restrict__ off,
                                                               const IA* __restrict__ irpA, const uint32_t* __restrict__ jaA,
                                                               const double* __restrict__ asA, const IB* __restrict__ irpB,
                                                               const uint32_t* __restrict__ jaB, const double* __restrict__ asB, uint64_t BM,
                                                               uint64_t* __restrict__ key, double* __restrict__ val) {
    __shared__ Stage<SG_THREADS> st;
    const uint64_t b = linear_block();
    if (b >= nRows) return;
    const uint32_t t = threadIdx.x, row = list[b];
    uint64_t out = off[b] - off[0];
    const uint64_t pe = irpA[row + 1];
    for (uint64_t p0 = irpA[row]; p0 < pe; p0 += SG_THREADS) {
        const uint64_t total = sg_stage<SG_THREADS, NUMERIC>(st, t, p0, pe, jaA, asA, irpB, BM);
        for (uint64_t f = t; f < total; f += SG_THREADS) {
            const uint32_t e = sg_find<SG_THREADS>(st, f);
            const uint64_t q = st.bst[e] + (f - st.pfx[e]);
            key[out + f] = b << 32 | jaB[q];
            if (NUMERIC) val[out + f] = st.av[e] * asB[q];
        }
        out += total;
    }
}

// the sorted products of row list[b] are [off[b] - off[0], off[b + 1] - off[0]): a wavefront per row counts the run heads, or
// lets the lane of each head add its run serially from +0.0 and store it at its rank
template <bool NUMERIC>
__global__ __launch_bounds__(SG_THREADS) void sg_runs_kernel(uint32_t nRows, const uint32_t* __restrict__ list, const uint64_t* __restrict__ off,
                                                             const uint64_t* __restrict__ key, const double* __restrict__ val,
                                                             uint32_t* __restrict__ counts, const uint32_t* __restrict__ irpC,
                                                             uint32_t* __restrict__ jaC, double* __restrict__ asC) {
    const uint64_t b = linear_block() * (SG_THREADS / 64) + threadIdx.x / 64;
    if (b >= nRows) return;
    const uint32_t lane = threadIdx.x % 64, row = list[b];
    const uint64_t lo = off[b] - off[0], hi = off[b + 1] - off[0];
    const uint32_t cBase = NUMERIC ? irpC[row] : 0;
    uint32_t done = 0;
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t f = base + lane;
        const bool in = f < hi;
        const uint64_t kf = in ? key[f] : 0;
        const bool head = in && (f == lo || key[f - 1] != kf);
        const uint64_t heads = __ballot(head);
        if (NUMERIC && head) {
            double acc = 0.0;
            for (uint64_t g = f; g < hi && key[g] == kf; ++g) acc = acc + val[g];
            const uint32_t at = cBase + done + __popcll(heads & ((1ull << lane) - 1));
            jaC[at] = (uint32_t)kf;
            asC[at] = acc;
        }
        done += (uint32_t)__popcll(heads);
    }
    if (!NUMERIC && lane == 0) counts[row] = done;
}

// ---------------------------------------------------------------------------------------------------- host side
struct Run {
    const DevMat *a, *b;
    SpgemmPlan* plan;
    hipStream_t st;
    TempTally tm;                                              // every temporary of the call counts into it: tempBytes = its peak
    SortedPath sp{"spgemm", "products", &tm};                  // the products before each sorted row, and the batches of the list
};

int fail(hipStream_t st, const char* what) { return buildFail(st, "spgemm", what); }

// the two hash classes over their lists
template <bool NUMERIC>
int hashPass(Run& r, uint32_t* counts, DevMat* c) {
    const SpgemmPlan* pl = r.plan;
    const uint32_t* irpC = c ? static_cast<const uint32_t*>(c->IRP) : nullptr;
    uint32_t* jaC = c ? c->JA : nullptr;
    double* asC = c ? c->AS : nullptr;
    withBoth(r.a, r.b, [&](auto ia, auto ib) {
        using IA = IrpT<decltype(ia)>;
        using IB = IrpT<decltype(ib)>;
        if (pl->nWave)
            hipLaunchKernelGGL((sg_hash_kernel<IA, IB, 64, SG_WAVE_SLOTS, SG_WAVE_RANK, NUMERIC>), gridFor(pl->nWave, SG_THREADS / 64),
                               dim3(SG_THREADS), 0, r.st, pl->nWave, pl->list, ia, r.a->JA, r.a->AS, ib, r.b->JA, r.b->AS, r.b->M, counts, irpC,
                               jaC, asC);
        if (pl->nGroup)
            hipLaunchKernelGGL((sg_hash_kernel<IA, IB, (int)SG_THREADS, SG_GROUP_SLOTS, SG_GROUP_RANK, NUMERIC>), gridFor(pl->nGroup, 1),
                               dim3(SG_THREADS), 0, r.st, pl->nGroup, pl->list + pl->nWave, ia, r.a->JA, r.a->AS, ib, r.b->JA, r.b->AS, r.b->M,
                               counts, irpC, jaC, asC);
        return 0;
    });
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : fail(r.st, "hash kernels");
}

// the products before every row of the sorted list, and its batches
int sortedPrepare(Run& r) {
    const SpgemmPlan* pl = r.plan;
    const uint32_t n = pl->nSorted;
    if (!n) return EXIT_SUCCESS;
    const uint32_t* list = pl->list + pl->nWave + pl->nGroup;
    TempBuf ubS(&r.tm), flag(&r.tm);
    if (ubS.alloc(((size_t)n + 1) * 8) || flag.alloc(4)) return fail(r.st, "temporary allocation (sorted rows)");
    if (hipMemsetAsync(ubS.p, 0, ((size_t)n + 1) * 8, r.st) != hipSuccess || hipMemsetAsync(flag.p, 0, 4, r.st) != hipSuccess) return fail(r.st, "memset");
    withBoth(r.a, r.b, [&](auto ia, auto ib) {
        hipLaunchKernelGGL((sg_ub_list_kernel<IrpT<decltype(ia)>, IrpT<decltype(ib)>>), gridFor(n, SG_THREADS / 64), dim3(SG_THREADS), 0, r.st, n,
                           list, ia, r.a->JA, ib, r.b->M, ubS.as<uint64_t>(), false, flag.as<uint32_t>());
        return 0;
    });
    return sortedBatches(r.sp, ubS.as<uint64_t>(), n, pl->batchProducts, r.st);
}

// the caller's half of the sorted path: the products of the rows list[k0 + b], b < nRows, in (p, q) order
template <bool NUMERIC>
int sortedClass(Run& r, uint32_t* counts, DevMat* c) {
    const SpgemmPlan* pl = r.plan;
    if (!pl->nSorted) return EXIT_SUCCESS;
    const uint32_t* list = pl->list + pl->nWave + pl->nGroup;
    return sortedPass(r.sp, NUMERIC, list, [&](uint32_t k0, uint32_t nRows, const uint64_t* off, uint64_t* key, double* val) {
        withBoth(r.a, r.b, [&](auto ia, auto ib) {
            hipLaunchKernelGGL((sg_expand_kernel<IrpT<decltype(ia)>, IrpT<decltype(ib)>, NUMERIC>), gridFor(nRows, 1), dim3(SG_THREADS), 0, r.st,
                               nRows, list + k0, off, ia, r.a->JA, r.a->AS, ib, r.b->JA, r.b->AS, r.b->M, key, val);
            return 0;
        });
    }, counts, c, r.st);
}

int numericPhase(Run& r, DevMat* c) {
    if (hashPass<true>(r, nullptr, c) || sortedClass<true>(r, nullptr, c)) return EXIT_FAILURE;
    if (hipStreamSynchronize(r.st) != hipSuccess) return fail(r.st, "numeric phase");
    return EXIT_SUCCESS;
}

}  // namespace

// ------------------------------------------------------------------------- shared with add.hip (device_prims.hpp)
// s.off[k] = the terms before row k of a sorted list of n rows (terms[n] is 0), read back; the batches: rows while their
// terms fit batchTerms, a row above the budget alone
int sortedBatches(SortedPath& s, const uint64_t* terms, uint32_t n, uint64_t batchTerms, hipStream_t st) {
    TempBuf scanTmp(s.tally);
    if (s.off.alloc(((size_t)n + 1) * 8)) return buildFail(st, s.module, "temporary allocation (sorted rows)");
    if (exclusiveScan(scanTmp, terms, s.off.as<uint64_t>(), (uint64_t)0, (size_t)n + 1, st) != hipSuccess) return buildFail(st, s.module, "scan");
    s.hOff.resize((size_t)n + 1);
    if (hipMemcpyAsync(s.hOff.data(), s.off.p, s.hOff.size() * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return buildFail(st, s.module, "sorted rows");
    s.batch.assign(1, 0u);
    for (uint32_t k = 0; k < n;) {
        uint32_t e = k + 1;
        while (e < n && s.hOff[e + 1] - s.hOff[k] <= batchTerms) ++e;
        s.batch.push_back(e);
        k = e;
    }
    return EXIT_SUCCESS;
}

// every batch: the caller's expansion into (key, val), ONE stable sort, the run kernel (counts, or c's rows)
int sortedPass(SortedPath& s, bool numeric, const uint32_t* list, const SortedExpand& expand, uint32_t* counts, const DevMat* c,
               hipStream_t st) {
    uint64_t most = 0;
    uint32_t mostRows = 1;
    for (size_t i = 0; i + 1 < s.batch.size(); ++i) {
        most = std::max(most, s.hOff[s.batch[i + 1]] - s.hOff[s.batch[i]]);
        mostRows = std::max(mostRows, s.batch[i + 1] - s.batch[i]);
    }
    if (most >= (1ull << 40)) {
        fprintf(stderr, "libspmvhip: %s: a batch of %lu %s is not supported\n", s.module, (unsigned long)most, s.items);
        return EXIT_FAILURE;
    }
    TempBuf keyIn(s.tally), keyOut(s.tally), valIn(s.tally), valOut(s.tally), sortTmp(s.tally);
    if (keyIn.alloc(most * 8) || keyOut.alloc(most * 8) || (numeric && (valIn.alloc(most * 8) || valOut.alloc(most * 8))))
        return buildFail(st, s.module, "temporary allocation (a sorted batch)");
    const unsigned endBit = 32 + bitsFor(mostRows);
    const uint32_t* irpC = c ? static_cast<const uint32_t*>(c->IRP) : nullptr;
    for (size_t i = 0; i + 1 < s.batch.size(); ++i) {
        const uint32_t k0 = s.batch[i], nRows = s.batch[i + 1] - k0;
        const uint64_t nTerms = s.hOff[k0 + nRows] - s.hOff[k0];
        const uint64_t* off = s.off.as<uint64_t>() + k0;
        expand(k0, nRows, off, keyIn.as<uint64_t>(), valIn.as<double>());
        // (sortTmp is shared by the batches: it grows, after a wait for the batch before, only when one needs more)
        const hipError_t e = numeric ? sortPairs(sortTmp, keyIn.as<uint64_t>(), keyOut.as<uint64_t>(), valIn.as<double>(), valOut.as<double>(),
                                                 (size_t)nTerms, 0u, endBit, st)
                                     : sortKeys(sortTmp, keyIn.as<uint64_t>(), keyOut.as<uint64_t>(), (size_t)nTerms, 0u, endBit, st);
        if (e != hipSuccess) return buildFail(st, s.module, "sort");
        if (numeric)
            hipLaunchKernelGGL((sg_runs_kernel<true>), gridFor(nRows, SG_THREADS / 64), dim3(SG_THREADS), 0, st, nRows, list + k0, off,
                               keyOut.as<uint64_t>(), valOut.as<double>(), counts, irpC, c ? c->JA : nullptr, c ? c->AS : nullptr);
        else
            hipLaunchKernelGGL((sg_runs_kernel<false>), gridFor(nRows, SG_THREADS / 64), dim3(SG_THREADS), 0, st, nRows, list + k0, off,
                               keyOut.as<uint64_t>(), valOut.as<double>(), counts, irpC, c ? c->JA : nullptr, c ? c->AS : nullptr);
    }
    if (hipGetLastError() != hipSuccess) return buildFail(st, s.module, "sorted path kernels");
    if (hipStreamSynchronize(st) != hipSuccess) return buildFail(st, s.module, "sorted path");
    return EXIT_SUCCESS;
}

void enqueueNarrowIrp(uint64_t M, const uint64_t* irp64, uint32_t* irp, uint32_t* maxLen, hipStream_t st) {
    hipLaunchKernelGGL(sg_narrow_kernel, gridFor(M + 1), dim3(SG_THREADS), 0, st, M, irp64, irp, maxLen);
}

void freeSpgemmPlan(SpgemmPlan* p) {
    if (!p) return;
    (void)devFree(p->list);
    delete p;
}

// c: kind, M and N set by the caller, nothing allocated.  On success c owns IRP (4 B), JA, AS and the plan, and c->NZ is
// set; on failure the caller frees c with whatever it holds.  nnz(C) >= IRP32_LIMIT and a column of A >= B.M are found
// before JA / AS exist.
int spgemmBuild(const DevMat* a, const DevMat* b, const spmvSpgemmOpts* opts, DevMat* c, spmvSpgemmInfo* info, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t M = a->M, BN = b->N;
    SpgemmPlan* pl = c->prod = new SpgemmPlan;
    const uint64_t waveMax = clampOpt(opts ? opts->waveMaxProducts : 0, SG_WAVE_MAX, SG_WAVE_MAX);
    const uint64_t groupMax = clampOpt(opts ? opts->groupMaxProducts : 0, SG_GROUP_MAX, SG_GROUP_MAX);
    pl->batchProducts = std::max<uint64_t>(clampOpt(opts ? opts->sortBudgetBytes : 0, SG_BUDGET, SG_BUDGET_MAX) / SG_PRODUCT_BYTES, 1);
    spmvSpgemmInfo out{};
    Run r{a, b, pl, st};
    if (devMalloc(&c->IRP, (M + 1) * 4) != hipSuccess) return fail(st, "allocation of the row pointers");
    c->irpBytes = 4;
    uint64_t nnzC = 0;
    if (M && a->NZ && b->NZ && BN) {
        // 1. the upper bound, the classes, the lists
        TempBuf ub(&r.tm), lists(&r.tm), longList(&r.tm), cnt(&r.tm), tot(&r.tm);
        const bool longRows = a->maxRowNnz > SG_LONG;
        if (ub.alloc(M * 8) || lists.alloc(M * 12) || cnt.alloc(5 * 4) || tot.alloc(16) || (longRows && longList.alloc(M * 4)))
            return fail(st, "temporary allocation (20 B per row)");
        uint32_t* const dCnt = cnt.as<uint32_t>();           // [0..2] rows of a class, [3] long rows of A, [4] column of A out of range
        if (hipMemsetAsync(dCnt, 0, 5 * 4, st) != hipSuccess || hipMemsetAsync(tot.p, 0, 16, st) != hipSuccess) return fail(st, "memset");
        uint32_t h[5] = {0, 0, 0, 0, 0};
        withBoth(a, b, [&](auto ia, auto ib) {
            hipLaunchKernelGGL((sg_ub_short_kernel<IrpT<decltype(ia)>, IrpT<decltype(ib)>>), gridFor(M), dim3(SG_THREADS), 0, st, M, ia, a->JA, ib, b->M,
                               ub.as<uint64_t>(), longList.as<uint32_t>(), dCnt + 3, dCnt + 4);
            return 0;
        });
        if (longRows) {
            if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, dCnt, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return fail(st, "upper bound");
            if (h[3])
                withBoth(a, b, [&](auto ia, auto ib) {
                    hipLaunchKernelGGL((sg_ub_list_kernel<IrpT<decltype(ia)>, IrpT<decltype(ib)>>), gridFor(h[3], SG_THREADS / 64), dim3(SG_THREADS), 0,
                                       st, h[3], longList.as<uint32_t>(), ia, a->JA, ib, b->M, ub.as<uint64_t>(), true, dCnt + 4);
                    return 0;
                });
        }
        hipLaunchKernelGGL(sg_classify_kernel, gridFor(M), dim3(SG_THREADS), 0, st, M, ub.as<uint64_t>(), BN, waveMax, groupMax, lists.as<uint32_t>(),
                           dCnt, tot.as<unsigned long long>());
        unsigned long long hTot[2] = {0, 0};
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, dCnt, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(hTot, tot.p, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "classification");
        if (h[4]) { fprintf(stderr, "libspmvhip: spgemm: a column id of A is >= B.M\n"); return EXIT_FAILURE; }
        pl->nWave = h[0]; pl->nGroup = h[1]; pl->nSorted = h[2];
        out.products = hTot[0]; out.maxRowProducts = hTot[1];
        const size_t nList = (size_t)h[0] + h[1] + h[2];
        if (devMalloc(&pl->list, std::max<size_t>(nList, 1) * 4) != hipSuccess) return fail(st, "allocation of the class lists");
        for (int cl = 0, at = 0; cl < 3; at += h[cl], ++cl)
            if (h[cl] && hipMemcpyAsync(pl->list + at, lists.as<uint32_t>() + (size_t)cl * M, (size_t)h[cl] * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
                return fail(st, "class lists");
        if (hipStreamSynchronize(st) != hipSuccess) return fail(st, "class lists");
        ub.release(); lists.release(); longList.release();
        // 2. symbolic: the counts, their scan, the row pointers
        TempBuf counts(&r.tm), irp64(&r.tm), scanTmp(&r.tm);
        if (counts.alloc((M + 1) * 4) || irp64.alloc((M + 1) * 8)) return fail(st, "temporary allocation (12 B per row)");
        if (hipMemsetAsync(counts.p, 0, (M + 1) * 4, st) != hipSuccess || hipMemsetAsync(dCnt, 0, 4, st) != hipSuccess) return fail(st, "memset");
        if (sortedPrepare(r) || hashPass<false>(r, counts.as<uint32_t>(), nullptr) || sortedClass<false>(r, counts.as<uint32_t>(), nullptr))
            return EXIT_FAILURE;
        if (exclusiveScan(scanTmp, counts.as<uint32_t>(), irp64.as<uint64_t>(), (uint64_t)0, (size_t)M + 1, st) != hipSuccess) return fail(st, "scan");
        if (hipMemcpyAsync(&nnzC, irp64.as<uint64_t>() + M, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(st, "row pointers");
        if (nnzC >= IRP32_LIMIT) {
            fprintf(stderr, "libspmvhip: spgemm: nnz(C) = %lu: the row pointers of the product are 32-bit (limit %lu)\n", (unsigned long)nnzC,
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
        return fail(st, "allocation of the product's arrays");
    if (numericPhase(r, c)) return EXIT_FAILURE;
    out.numericMs = msSince(t1);
    out.nnzC = nnzC;
    out.rowsWave = pl->nWave; out.rowsGroup = pl->nGroup; out.rowsSorted = pl->nSorted;
    out.sortBatches = r.sp.batches();
    out.tempBytes = r.tm.peak;
    out.ms = msSince(t0);
    pl->info = out;
    if (info) *info = out;
    return EXIT_SUCCESS;
}

// the numeric phase again, on the kept lists, into c's arrays
int spgemmRefresh(DevMat* c, const DevMat* a, const DevMat* b, spmvSpgemmInfo* info, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    SpgemmPlan* pl = c->prod;
    Run r{a, b, pl, st};
    if (sortedPrepare(r) || numericPhase(r, c)) return EXIT_FAILURE;
    spmvSpgemmInfo out = pl->info;
    out.symbolicMs = 0;
    out.numericMs = out.ms = msSince(t0);
    out.sortBatches = r.sp.batches();
    out.tempBytes = r.tm.peak;
    pl->info = out;
    if (info) *info = out;
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
