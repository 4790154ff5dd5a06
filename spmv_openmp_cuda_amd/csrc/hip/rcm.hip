// rcm.hip -- the reverse Cuthill-McKee ordering of a square device CSR handle (spmvHipRcmCSR).  DESIGN.md section 37; the
// contract -- the serial queue loop whose output this is, word for word -- is in spmvHip.h.  Integer work only.
//
// The level-synchronous form of the queue.  If level l stands at positions lo..hi-1 of `order`, level l + 1 is the set of
// unvisited vertices adjacent to it, each with parent(w) = the smallest position of a level-l neighbour, laid out in
// ascending (parent, deg, id).  (deg, id) is one number here: rank[v], the place of v among all vertices sorted by (deg, id)
// once -- so the key (parent - lo, rank) fits 62 bits and every level is ONE stable sort.  The same list, walked by a
// cursor, gives the start of the next component, and its minimum over a last level the next candidate of the start search.
//   par[w]    UNSET until w is reached by the ordering: one atomicMin of the parent's position per frontier edge, and the
//             lane that saw UNSET come back claims w for the next level.  A position never undercuts the parent of a vertex
//             of an earlier level, so the word is mark and parent in one.
//   smark[w]  the number of the last start-search BFS that reached w (atomicMax; those runs leave `par` alone).
// Who runs what.  rc_run_kernel, ONE workgroup of 1024 lanes, is the whole loop as a state machine over a small device
// record: it takes the next component, runs the start search and the ordering level after level with barriers between
// them, and expands a level itself when it is thin: at most T vertices whose degrees sum to at most RC_CAP, so the next
// level fits its LDS list whatever it turns out to be -- no level is ever begun and abandoned, and no mark is left that a
// wide level would have to undo.  The next level is sorted in LDS by counting, for every key, the keys below it.  Any
// other level it hands to the host as a request and stops: rc_expand_kernel over the frontier (a lane per vertex; a vertex
// with more than 64 adjacency entries is then walked by its whole wavefront), for the ordering one read-back of the
// count, the keys, one radix sort and the placement; then the run kernel again.  One read-back per run and one per wide
// ordering level; no flag, ticket or spin -- ordering between workgroups is the kernel boundary on one stream.
// Adjacency: A's own arrays when every row ascends strictly and the pattern is structurally symmetric (diagonal and, by
// the check, ids >= M skipped on the fly); otherwise the deduplicated CSR of A + A^T without the diagonal from one radix
// sort of the (i, j) keys of both directions, heads, a scan and the ranks.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstring>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {

namespace {

constexpr uint32_t RC_THREADS = WG_THREADS;
constexpr uint32_t RC_RUN = 1024;                              // lanes of the run kernel = the largest T
constexpr uint32_t RC_CAP = 2048;                              // entries of the run kernel's LDS list
constexpr uint32_t RC_LONG = 64;                               // adjacency entries above which a vertex takes a wavefront
constexpr uint32_t RC_STEPS = 1u << 16;                        // steps of the state machine per launch
constexpr uint32_t UNSET = 0xFFFFFFFFu;

enum : uint32_t { PH_INIT, PH_PICK, PH_SEARCH_BEGIN, PH_SEARCH_LEVEL, PH_SEARCH_WIDE_DONE, PH_SEARCH_END, PH_ORDER_BEGIN, PH_ORDER_LEVEL,
                  PH_ORDER_WIDE_DONE, PH_DONE };
enum : uint32_t { RQ_NONE, RQ_WIDE_SEARCH, RQ_WIDE_ORDER };

struct RcmState {
    uint32_t phase, request;
    uint32_t cursor, nOrdered, lo, hi;                         // next place in byDeg; vertices ordered; the ordering's frontier
    uint32_t root, cand, nPass, depthBest, minBest;            // the start search: r, v, n, depth(L), min rank of L's last level
    uint32_t depth, lastMin, stamp, fN, flip;                  // the BFS under way: levels, min rank of its last one, number, frontier
    uint32_t wideCount, wideMin;                               // what a wide level found
    uint32_t zeros, components, levels, startBfs, maxFrontier, longRows;
    uint32_t bandwidth[2];
};

// words that the run kernel writes and reads again in the same launch go past the L1
__device__ __forceinline__ uint32_t ld_dev(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_dev(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 1 in *flag unless every stored (i, j), j != i, has a stored (j, i): a binary search in row j (rows ascend strictly: the
// caller has checked).  A column id >= M has no row to look in: not symmetric.
template <typename I>
__global__ __launch_bounds__(RC_THREADS) void rc_symmetric_kernel(uint64_t nnz, uint64_t M, const I* __restrict__ IRP,
                                                                  const uint32_t* __restrict__ JA, const uint32_t* __restrict__ rowOf,
                                                                  uint32_t* __restrict__ flag) {
    const uint64_t p = linear_block() * RC_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const uint32_t i = rowOf[p], j = JA[p];
    if (j == i) return;
    bool found = false;
    if (j < M) {
        uint64_t a = IRP[j], b = IRP[j + 1];
        while (a < b && !found) {
            const uint64_t mid = a + (b - a) / 2;
            const uint32_t c = JA[mid];
            found = c == i;
            if (c < i) a = mid + 1; else b = mid;
        }
    }
    if (!found) atomicOr(flag, 1u);
}

// deg of a strictly ascending, symmetric row: its entries but the diagonal
template <typename I>
__global__ __launch_bounds__(RC_THREADS) void rc_own_degree_kernel(uint64_t M, const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                                                   uint32_t* __restrict__ deg) {
    const uint64_t r = linear_block() * RC_THREADS + threadIdx.x;
    if (r >= M) return;
    uint32_t d = 0;
    for (uint64_t p = IRP[r], e = IRP[r + 1]; p < e; ++p) d += JA[p] != r;
    deg[r] = d;
}

// both directions of every stored (i, j), j != i, j < M, as i << 32 | j; anything else as the key of the row M that is none
__global__ __launch_bounds__(RC_THREADS) void rc_edge_keys_kernel(uint64_t nnz, uint64_t M, const uint32_t* __restrict__ rowOf,
                                                                  const uint32_t* __restrict__ JA, uint64_t* __restrict__ key) {
    const uint64_t p = linear_block() * RC_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const uint32_t i = rowOf[p], j = JA[p];
    const bool edge = j != i && j < M;
    key[2 * p] = edge ? (uint64_t)i << 32 | j : M << 32;
    key[2 * p + 1] = edge ? (uint64_t)j << 32 | i : M << 32;
}

// head[q] = 1 where a new (i, j) begins among the sorted keys, and deg[i] counts its heads
__global__ __launch_bounds__(RC_THREADS) void rc_heads_kernel(uint64_t n, uint64_t M, const uint64_t* __restrict__ key, uint32_t* __restrict__ head,
                                                              uint32_t* __restrict__ deg) {
    const uint64_t q = linear_block() * RC_THREADS + threadIdx.x;
    if (q >= n) return;
    const uint64_t k = key[q];
    const bool h = (k >> 32) < M && (q == 0 || key[q - 1] != k);
    head[q] = h;
    if (h) atomicAdd(deg + (k >> 32), 1u);
}

__global__ __launch_bounds__(RC_THREADS) void rc_compact_kernel(uint64_t n, const uint64_t* __restrict__ key, const uint32_t* __restrict__ head,
                                                                const uint64_t* __restrict__ pos, uint32_t* __restrict__ adjCol) {
    const uint64_t q = linear_block() * RC_THREADS + threadIdx.x;
    if (q >= n || !head[q]) return;
    adjCol[pos[q]] = (uint32_t)key[q];
}

// rank[byDeg[k]] = k.  The vertices without a neighbour stand first in byDeg, in id order, and are the first components,
// one each: placed here, counted in zeros.  longRows: the vertices that a wavefront expands.
__global__ __launch_bounds__(RC_THREADS) void rc_rank_kernel(uint64_t M, const uint32_t* __restrict__ byDeg, const uint32_t* __restrict__ deg,
                                                             uint32_t* __restrict__ rank, uint32_t* __restrict__ order, uint32_t* __restrict__ par,
                                                             RcmState* __restrict__ st) {
    const uint64_t k = linear_block() * RC_THREADS + threadIdx.x;
    bool zero = false, isLong = false;
    if (k < M) {
        const uint32_t v = byDeg[k], d = deg[v];
        rank[v] = (uint32_t)k;
        zero = d == 0;
        isLong = d > RC_LONG;
        if (zero) { order[k] = v; par[v] = 0; }
    }
    const uint64_t bz = __ballot(zero), bl = __ballot(isLong);
    if (threadIdx.x % 64 == 0) {
        if (bz) atomicAdd(&st->zeros, (uint32_t)__popcll(bz));
        if (bl) atomicAdd(&st->longRows, (uint32_t)__popcll(bl));
    }
}

// One wavefront, all 64 lanes here, expands up to 64 frontier vertices: lane k has u, which stands at position pos
// (valid: the lane has one).  A lane walks its own vertex in step with the others; a vertex with more than RC_LONG
// adjacency entries is walked by the whole wavefront afterwards.  ORDERING: atomicMin of pos into par[w], the lane that
// saw UNSET claims w.  Otherwise: atomicMax of the run's number into smark[w], the lane that saw an older one claims w,
// and *levMin takes the smallest rank claimed.  A claimed w goes to list[] at a place taken from *cnt, one atomic per
// wavefront step.  Column ids >= M and the diagonal are skipped.
template <typename I, bool ORDERING>
__device__ __forceinline__ void rc_expand_wave(bool valid, uint32_t u, uint32_t pos, uint64_t M, const I* __restrict__ ptr,
                                               const uint32_t* __restrict__ col, uint32_t* mark, uint32_t stamp, const uint32_t* __restrict__ rank,
                                               uint32_t* cnt, uint32_t* list, uint32_t* levMin) {
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t below = (1ull << lane) - 1;
    uint64_t b = 0, e = 0;
    if (valid) { b = ptr[u]; e = ptr[u + 1]; }
    const uint64_t len = e - b;
    const bool isLong = valid && len > RC_LONG;
    uint32_t myMin = UNSET;
    auto visit = [&](bool act, uint32_t w, uint32_t from, uint32_t p) {
        bool claimed = false;
        if (act && w != from && w < M) {
            if (ORDERING) {
                claimed = atomicMin(mark + w, p) == UNSET;
            } else {
                claimed = atomicMax(mark + w, stamp) != stamp;
                if (claimed) myMin = min(myMin, rank[w]);
            }
        }
        const uint64_t bal = __ballot(claimed);
        if (bal) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(cnt, (uint32_t)__popcll(bal));
            base = __shfl(base, 0);
            if (claimed) list[base + __popcll(bal & below)] = w;
        }
    };
    uint32_t steps = valid && !isLong ? (uint32_t)len : 0u;
    for (int off = 32; off; off >>= 1) steps = max(steps, (uint32_t)__shfl_xor(steps, off));
    for (uint32_t k = 0; k < steps; ++k) {
        const bool act = valid && !isLong && k < len;
        visit(act, act ? col[b + k] : 0u, u, pos);
    }
    for (uint64_t m = __ballot(isLong); m; m &= m - 1) {
        const int l = __ffsll((long long)m) - 1;
        const uint32_t ul = __shfl(u, l), pl = __shfl(pos, l);
        const uint64_t bl = (uint64_t)__shfl((uint32_t)(b >> 32), l) << 32 | __shfl((uint32_t)b, l);
        const uint64_t el = (uint64_t)__shfl((uint32_t)(e >> 32), l) << 32 | __shfl((uint32_t)e, l);
        for (uint64_t q = bl; q < el; q += 64) {
            const bool act = q + lane < el;
            visit(act, act ? col[q + lane] : 0u, ul, pl);
        }
    }
    if (!ORDERING) {
        for (int off = 32; off; off >>= 1) myMin = min(myMin, (uint32_t)__shfl_xor(myMin, off));
        if (lane == 0 && myMin != UNSET) atomicMin(levMin, myMin);
    }
}

// a wide level: frontier[0 .. n), the first at position pos0, into list[0 .. st->wideCount)
template <typename I, bool ORDERING>
__global__ __launch_bounds__(RC_THREADS) void rc_expand_kernel(uint32_t n, const uint32_t* __restrict__ frontier, uint32_t pos0, uint64_t M,
                                                               const I* __restrict__ ptr, const uint32_t* __restrict__ col, uint32_t* mark,
                                                               uint32_t stamp, const uint32_t* __restrict__ rank, uint32_t* __restrict__ list,
                                                               RcmState* st) {
    const uint64_t k = linear_block() * RC_THREADS + threadIdx.x;
    const bool valid = k < n;
    rc_expand_wave<I, ORDERING>(valid, valid ? frontier[k] : 0u, pos0 + (uint32_t)k, M, ptr, col, mark, stamp, rank, &st->wideCount, list,
                                &st->wideMin);
}

// the key of a claimed vertex: (parent's place in the frontier, rank), rank in the low rb bits
__global__ __launch_bounds__(RC_THREADS) void rc_keys_kernel(uint32_t c, const uint32_t* __restrict__ list, const uint32_t* __restrict__ par,
                                                             const uint32_t* __restrict__ rank, uint32_t lo, unsigned rb, uint64_t* __restrict__ key) {
    const uint64_t k = linear_block() * RC_THREADS + threadIdx.x;
    if (k >= c) return;
    const uint32_t w = list[k];
    key[k] = (uint64_t)(par[w] - lo) << rb | rank[w];
}

__global__ __launch_bounds__(RC_THREADS) void rc_place_kernel(uint32_t c, const uint64_t* __restrict__ key, unsigned rb,
                                                              const uint32_t* __restrict__ byDeg, uint32_t* __restrict__ out) {
    const uint64_t k = linear_block() * RC_THREADS + threadIdx.x;
    if (k >= c) return;
    out[k] = byDeg[key[k] & ((1ull << rb) - 1)];
}

// The loop of spmvHip.h as a state machine in one workgroup (the head of this file).  It returns with phase == PH_DONE,
// with a request for a wide level, or after RC_STEPS steps, to be launched again.  T = 0: no level is expanded here.
template <typename I>
__global__ __launch_bounds__(RC_RUN) void rc_run_kernel(RcmState* g, uint64_t M, const I* __restrict__ ptr, const uint32_t* __restrict__ col,
                                                        const uint32_t* __restrict__ deg, const uint32_t* __restrict__ rank,
                                                        const uint32_t* __restrict__ byDeg, uint32_t* par, uint32_t* smark, uint32_t* order,
                                                        uint32_t* fA, uint32_t* fB, uint32_t T, int peripheral, uint32_t maxPasses) {
    __shared__ RcmState s;
    __shared__ uint32_t sList[RC_CAP];
    __shared__ uint64_t sKey[RC_CAP];
    __shared__ uint32_t sCnt, sMin, sSum, sFound;
    const uint32_t tid = threadIdx.x;
    const uint32_t small = max(T, 1u);                         // a frontier this small is looked at for "no edge at all"
    if (tid == 0) { s = *g; s.request = RQ_NONE; }
    for (uint32_t step = 0; step < RC_STEPS; ++step) {
        __syncthreads();
        const uint32_t phase = s.phase, request = s.request, cursor = s.cursor, nOrdered = s.nOrdered, lo = s.lo, hi = s.hi, fN = s.fN,
                       stamp = s.stamp;
        uint32_t* const F = s.flip ? fB : fA;                  // the start search's frontier
        __syncthreads();
        if (phase == PH_DONE || request != RQ_NONE) break;
        if (phase == PH_INIT) {
            if (tid == 0) {
                const uint32_t z = s.zeros;
                s.cursor = s.nOrdered = s.components = s.levels = z;
                s.startBfs = peripheral ? z : 0;
                s.maxFrontier = z ? 1 : 0;
                s.phase = PH_PICK;
            }
        } else if (phase == PH_PICK) {
            if (nOrdered >= M) {
                if (tid == 0) s.phase = PH_DONE;
                continue;
            }
            uint32_t found = UNSET;                            // the first place from the cursor on whose vertex is unvisited
            for (uint64_t k0 = cursor; k0 < M && found == UNSET; k0 += RC_RUN) {
                if (tid == 0) sFound = UNSET;
                __syncthreads();
                const uint64_t k = k0 + tid;
                if (k < M && ld_dev(par + byDeg[k]) == UNSET) atomicMin(&sFound, (uint32_t)k);
                __syncthreads();
                found = sFound;
                __syncthreads();
            }
            if (tid == 0) {
                if (found == UNSET) {                          // (never: fewer than M vertices are ordered)
                    s.phase = PH_DONE;
                } else {
                    s.root = s.cand = byDeg[found];
                    s.cursor = found + 1;
                    ++s.components;
                    s.nPass = 0;
                    s.phase = peripheral ? PH_SEARCH_BEGIN : PH_ORDER_BEGIN;
                }
            }
        } else if (phase == PH_SEARCH_BEGIN) {
            if (tid == 0) {
                const uint32_t c = s.cand;
                ++s.stamp;
                atomicMax(smark + c, s.stamp);
                st_dev(F, c);
                s.fN = 1; s.depth = 1; s.lastMin = rank[c];
                ++s.nPass;
                s.phase = PH_SEARCH_LEVEL;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (phase == PH_SEARCH_LEVEL || phase == PH_ORDER_LEVEL) {
            const bool ordering = phase == PH_ORDER_LEVEL;
            const uint32_t n = ordering ? hi - lo : fN;
            const uint32_t* const front = ordering ? order + lo : F;
            uint32_t sum = RC_CAP + 1;
            if (n <= small) {                                  // the degrees of the frontier, each capped, summed
                if (tid == 0) sSum = 0;
                __syncthreads();
                if (tid < n) atomicAdd(&sSum, min(deg[ld_dev(front + tid)], RC_CAP + 1));
                __syncthreads();
                sum = sSum;
            }
            if (sum == 0) {                                    // no edge leaves the frontier: the BFS ends here
                if (tid == 0) {
                    if (ordering) { s.nOrdered = hi; s.phase = PH_PICK; }
                    else s.phase = PH_SEARCH_END;
                }
            } else if (n <= T && sum <= RC_CAP) {              // thin: at most `sum` claims, which the list holds
                if (tid == 0) { sCnt = 0; sMin = UNSET; }
                __syncthreads();
                const bool valid = tid < n;
                const uint32_t u = valid ? ld_dev(front + tid) : 0u;
                if (ordering) rc_expand_wave<I, true>(valid, u, lo + tid, M, ptr, col, par, 0u, rank, &sCnt, sList, &sMin);
                else          rc_expand_wave<I, false>(valid, u, 0u, M, ptr, col, smark, stamp, rank, &sCnt, sList, &sMin);
                __syncthreads();
                const uint32_t c = sCnt;
                if (ordering) {
                    for (uint32_t k = tid; k < c; k += RC_RUN) {
                        const uint32_t w = sList[k];
                        sKey[k] = (uint64_t)(ld_dev(par + w) - lo) << 31 | rank[w];
                    }
                    __syncthreads();
                    for (uint32_t k = tid; k < c; k += RC_RUN) {       // the place of a key = the keys below it (no two are equal)
                        const uint64_t mine = sKey[k];
                        uint32_t r = 0;
                        for (uint32_t t = 0; t < c; ++t) r += sKey[t] < mine;
                        st_dev(order + hi + r, sList[k]);
                    }
                } else {
                    for (uint32_t k = tid; k < c; k += RC_RUN) st_dev(F + k, sList[k]);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (tid == 0) {
                    if (c == 0) {
                        if (ordering) { s.nOrdered = hi; s.phase = PH_PICK; }
                        else s.phase = PH_SEARCH_END;
                    } else if (ordering) {
                        s.lo = hi; s.hi = hi + c;
                        ++s.levels;
                        s.maxFrontier = max(s.maxFrontier, c);
                    } else {
                        s.fN = c; ++s.depth; s.lastMin = sMin;
                    }
                }
            } else if (tid == 0) {                             // wide: the host's
                s.wideCount = 0; s.wideMin = UNSET;
                s.request = ordering ? RQ_WIDE_ORDER : RQ_WIDE_SEARCH;
                s.phase = ordering ? PH_ORDER_WIDE_DONE : PH_SEARCH_WIDE_DONE;
            }
        } else if (phase == PH_SEARCH_WIDE_DONE) {
            if (tid == 0) {
                if (s.wideCount == 0) {
                    s.phase = PH_SEARCH_END;
                } else {
                    s.flip ^= 1u;
                    s.fN = s.wideCount; ++s.depth; s.lastMin = s.wideMin;
                    s.phase = PH_SEARCH_LEVEL;
                }
            }
        } else if (phase == PH_SEARCH_END) {                   // the BFS from cand is complete: the while loop of spmvHip.h
            if (tid == 0) {
                bool deeper = false;
                if (s.nPass == 1) { s.depthBest = s.depth; s.minBest = s.lastMin; deeper = true; }
                else if (s.depth > s.depthBest) { s.root = s.cand; s.depthBest = s.depth; s.minBest = s.lastMin; deeper = true; }
                const uint32_t v = byDeg[s.minBest];
                if (deeper && s.nPass <= maxPasses && v != s.root) {
                    s.cand = v;
                    s.phase = PH_SEARCH_BEGIN;
                } else {
                    s.startBfs += s.nPass;
                    s.phase = PH_ORDER_BEGIN;
                }
            }
        } else if (phase == PH_ORDER_BEGIN) {
            if (tid == 0) {
                const uint32_t r = s.root, p = s.nOrdered;
                atomicExch(par + r, 0u);                       // (no position undercuts it)
                st_dev(order + p, r);
                s.lo = p; s.hi = p + 1;
                ++s.levels;
                s.maxFrontier = max(s.maxFrontier, 1u);
                s.phase = PH_ORDER_LEVEL;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (phase == PH_ORDER_WIDE_DONE) {
            if (tid == 0) {
                const uint32_t c = s.wideCount;
                if (c == 0) {
                    s.nOrdered = hi; s.phase = PH_PICK;
                } else {
                    s.lo = hi; s.hi = hi + c;
                    ++s.levels;
                    s.maxFrontier = max(s.maxFrontier, c);
                    s.phase = PH_ORDER_LEVEL;
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) *g = s;
}

// perm[k] = order[M - 1 - k] (forward: order[k]) into dPerm, when there is one, and its inverse into inv
__global__ __launch_bounds__(RC_THREADS) void rc_finish_kernel(uint64_t M, const uint32_t* __restrict__ order, int forward,
                                                               uint32_t* __restrict__ dPerm, uint32_t* __restrict__ inv) {
    const uint64_t k = linear_block() * RC_THREADS + threadIdx.x;
    if (k >= M) return;
    const uint32_t v = order[forward ? k : M - 1 - k];
    if (dPerm) dPerm[k] = v;
    inv[v] = (uint32_t)k;
}

// *out = max |inv[i] - inv[j]| over the stored (i, j) with j < M (inv null: the ids themselves)
__global__ __launch_bounds__(RC_THREADS) void rc_bandwidth_kernel(uint64_t nnz, uint64_t M, const uint32_t* __restrict__ rowOf,
                                                                  const uint32_t* __restrict__ JA, const uint32_t* __restrict__ inv,
                                                                  uint32_t* __restrict__ out) {
    const uint64_t p = linear_block() * RC_THREADS + threadIdx.x;
    uint32_t d = 0;
    if (p < nnz) {
        const uint32_t i = rowOf[p], j = JA[p];
        if (j < M) {
            const uint32_t a = inv ? inv[i] : i, b = inv ? inv[j] : j;
            d = a > b ? a - b : b - a;
        }
    }
    for (int off = 32; off; off >>= 1) d = max(d, (uint32_t)__shfl_xor(d, off));
    if (threadIdx.x % 64 == 0 && d) atomicMax(out, d);
}

}  // namespace

int rcmCsr(const DevMat* a, int peripheral, uint32_t maxPasses, int forward, uint32_t T, uint32_t* dPerm, spmvRcmInfo* info, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t M = a->M, nnz = a->NZ;
    spmvRcmInfo out{};
    out.symmetric = 1;                                         // (no entry: A's own arrays, such as they are, serve)
    auto fail = [&](const char* what) { return buildFail(st, "rcm", what); };
    if (M == 0) { *info = out; return EXIT_SUCCESS; }
    T = std::min(T, RC_RUN);
    auto launched = [&](unsigned n = 1) { out.launches += n; };

    // 1. the adjacency and the degrees
    TempBuf rowOf, degBuf, adjPtr, adjCol, sortTmp;
    if (rowOf.alloc(nnz * 4) || degBuf.alloc((M + 1) * 4)) return fail("temporary allocation (rows of the entries, degrees)");
    uint32_t* const deg = degBuf.as<uint32_t>();
    if (nnz) { enqueueRowOf(M, a->IRP, a->irpBytes, rowOf.as<uint32_t>(), st); launched(); }
    long unsorted = -1;
    if (iluUnsortedRow(a, st, &unsorted)) return fail("pattern check");
    launched();
    uint32_t asym = unsorted >= 0;
    if (!asym && nnz) {
        if (deviceFlag(0, st, "rc_symmetric_kernel", &asym, [&](uint32_t* dFlag) {
                withIrp(a, [&](auto irp) {
                    hipLaunchKernelGGL((rc_symmetric_kernel<IrpT<decltype(irp)>>), gridFor(nnz), dim3(RC_THREADS), 0, st, nnz, M, irp, a->JA,
                                       rowOf.as<uint32_t>(), dFlag);
                });
            }))
            return fail("symmetry check");
        launched();
    }
    out.symmetric = asym ? 0 : 1;
    if (!asym) {
        withIrp(a, [&](auto irp) {
            hipLaunchKernelGGL((rc_own_degree_kernel<IrpT<decltype(irp)>>), gridFor(M), dim3(RC_THREADS), 0, st, M, irp, a->JA, deg);
        });
        launched();
    } else {
        const uint64_t n2 = 2 * nnz;
        TempBuf keyIn, keyOut, head, pos;
        if (keyIn.alloc(n2 * 8) || keyOut.alloc(n2 * 8) || head.alloc(n2 * 4) || pos.alloc(n2 * 8) || adjPtr.alloc((M + 1) * 8) ||
            adjCol.alloc(n2 * 4))
            return fail("temporary allocation (the pattern of A + A^T)");
        if (hipMemsetAsync(deg, 0, (M + 1) * 4, st) != hipSuccess) return fail("degrees");
        hipLaunchKernelGGL(rc_edge_keys_kernel, gridFor(nnz), dim3(RC_THREADS), 0, st, nnz, M, rowOf.as<uint32_t>(), a->JA, keyIn.as<uint64_t>());
        if (sortKeys(sortTmp, keyIn.as<uint64_t>(), keyOut.as<uint64_t>(), (size_t)n2, 0u, 32 + bitsFor(M + 1), st) != hipSuccess) return fail("sort");
        hipLaunchKernelGGL(rc_heads_kernel, gridFor(n2), dim3(RC_THREADS), 0, st, n2, M, keyOut.as<uint64_t>(), head.as<uint32_t>(), deg);
        if (exclusiveScan(sortTmp, head.as<uint32_t>(), pos.as<uint64_t>(), (uint64_t)0, (size_t)n2, st) != hipSuccess ||
            exclusiveScan(sortTmp, deg, adjPtr.as<uint64_t>(), (uint64_t)0, (size_t)(M + 1), st) != hipSuccess)
            return fail("scan");
        hipLaunchKernelGGL(rc_compact_kernel, gridFor(n2), dim3(RC_THREADS), 0, st, n2, keyOut.as<uint64_t>(), head.as<uint32_t>(), pos.as<uint64_t>(),
                           adjCol.as<uint32_t>());
        launched(6);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail("the pattern of A + A^T");
    }                                                          // (the keys, heads and places go here, the stream idle)
    auto withAdj = [&](auto&& f) {
        if (!asym) withIrp(a, [&](auto irp) { f(irp, static_cast<const uint32_t*>(a->JA)); });
        else f(static_cast<const uint64_t*>(adjPtr.as<uint64_t>()), static_cast<const uint32_t*>(adjCol.as<uint32_t>()));
    };

    // 2. the vertices by (deg, id), their ranks, the vertices without a neighbour; the state
    TempBuf byDegBuf, rankBuf, parBuf, smarkBuf, orderBuf, fBuf, stateBuf;
    if (byDegBuf.alloc(M * 4) || rankBuf.alloc(M * 4) || parBuf.alloc(M * 4) || smarkBuf.alloc(M * 4) || orderBuf.alloc(M * 4) ||
        fBuf.alloc(M * 8) || stateBuf.alloc(sizeof(RcmState)))
        return fail("temporary allocation (28 B per row)");
    uint32_t *const byDeg = byDegBuf.as<uint32_t>(), *const rank = rankBuf.as<uint32_t>(), *const par = parBuf.as<uint32_t>(),
             *const smark = smarkBuf.as<uint32_t>(), *const order = orderBuf.as<uint32_t>(), *const fA = fBuf.as<uint32_t>(), *const fB = fA + M;
    RcmState* const dS = stateBuf.as<RcmState>();
    RcmState h{};
    static_assert(PH_INIT == 0, "a zeroed state is the initial one");
    if (hipMemsetAsync(dS, 0, sizeof h, st) != hipSuccess || hipMemsetAsync(par, 0xFF, M * 4, st) != hipSuccess ||
        hipMemsetAsync(smark, 0, M * 4, st) != hipSuccess)
        return fail("state");
    enqueueIota(M, fA, st);
    if (sortPairs(sortTmp, deg, fB, fA, byDeg, (size_t)M, 0u, bitsFor(M), st) != hipSuccess) return fail("sort");
    hipLaunchKernelGGL(rc_rank_kernel, gridFor(M), dim3(RC_THREADS), 0, st, M, byDeg, deg, rank, order, par, dS);
    launched(3);

    // 3. the loop: the run kernel, and the wide levels it asks for
    TempBuf keyIn, keyOut;
    const unsigned rb = bitsFor(M);
    for (;;) {
        const RcmState was = h;
        withAdj([&](auto ptr, const uint32_t* col) {
            hipLaunchKernelGGL((rc_run_kernel<IrpT<decltype(ptr)>>), dim3(1), dim3(RC_RUN), 0, st, dS, M, ptr, col, deg, rank, byDeg, par, smark, order,
                               fA, fB, T, peripheral, maxPasses);
        });
        launched();
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, dS, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail("run");
        ++out.hostChecks;
        if (h.phase == PH_DONE) break;
        if (h.request == RQ_NONE && !memcmp(&was, &h, sizeof h)) return fail("run (a launch that changed nothing)");   // (never)
        if (h.request == RQ_WIDE_SEARCH) {
            withAdj([&](auto ptr, const uint32_t* col) {
                hipLaunchKernelGGL((rc_expand_kernel<IrpT<decltype(ptr)>, false>), gridFor(h.fN), dim3(RC_THREADS), 0, st, h.fN, h.flip ? fB : fA, 0u, M,
                                   ptr, col, smark, h.stamp, rank, h.flip ? fA : fB, dS);
            });
            launched();
        } else if (h.request == RQ_WIDE_ORDER) {
            const uint32_t n = h.hi - h.lo;
            withAdj([&](auto ptr, const uint32_t* col) {
                hipLaunchKernelGGL((rc_expand_kernel<IrpT<decltype(ptr)>, true>), gridFor(n), dim3(RC_THREADS), 0, st, n, order + h.lo, h.lo, M, ptr, col,
                                   par, 0u, rank, fA, dS);
            });
            launched();
            uint32_t c = 0;
            if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&c, &dS->wideCount, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return fail("level");
            ++out.hostChecks;
            if ((uint64_t)h.hi + c > M) return fail("level (more vertices than the matrix has)");      // (never)
            if (c) {
                if (!keyIn.p && (keyIn.alloc(M * 8) || keyOut.alloc(M * 8))) return fail("temporary allocation (16 B per row)");
                hipLaunchKernelGGL(rc_keys_kernel, gridFor(c), dim3(RC_THREADS), 0, st, c, fA, par, rank, h.lo, rb, keyIn.as<uint64_t>());
                if (sortKeys(sortTmp, keyIn.as<uint64_t>(), keyOut.as<uint64_t>(), (size_t)c, 0u, rb + bitsFor(n), st) != hipSuccess) return fail("sort");
                hipLaunchKernelGGL(rc_place_kernel, gridFor(c), dim3(RC_THREADS), 0, st, c, keyOut.as<uint64_t>(), rb, byDeg, order + h.hi);
                launched(3);
            }
        }
    }
    if (h.nOrdered != M) return fail("ordering (vertices left over)");                                    // (never)

    // 4. the permutation, its inverse (in the room of smark) and the two bandwidths
    uint32_t* const inv = smark;
    hipLaunchKernelGGL(rc_finish_kernel, gridFor(M), dim3(RC_THREADS), 0, st, M, order, forward, dPerm, inv);
    launched();
    if (nnz) {
        hipLaunchKernelGGL(rc_bandwidth_kernel, gridFor(nnz), dim3(RC_THREADS), 0, st, nnz, M, rowOf.as<uint32_t>(), a->JA,
                           static_cast<const uint32_t*>(nullptr), &dS->bandwidth[0]);
        hipLaunchKernelGGL(rc_bandwidth_kernel, gridFor(nnz), dim3(RC_THREADS), 0, st, nnz, M, rowOf.as<uint32_t>(), a->JA,
                           static_cast<const uint32_t*>(inv), &dS->bandwidth[1]);
        launched(2);
    }
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, dS, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail("permutation");
    ++out.hostChecks;
    out.components = h.components;
    out.levels = h.levels;
    out.startBfs = h.startBfs;
    out.maxFrontier = h.maxFrontier;
    out.longRows = h.longRows;
    out.bandwidthBefore = h.bandwidth[0];
    out.bandwidthAfter = h.bandwidth[1];
    out.ms = msSince(t0);
    *info = out;
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
