// amg.hip -- aggregation multigrid on the device: the aggregation of a square CSR handle (spmvHipAggregateCSR), the
// hierarchy of Galerkin products (spmvHipAmgSetup, spmvHipAmgRefresh) and its damped-Jacobi V-cycle (spmvHipAmgApply, and
// the dM of the Krylov solvers).  DESIGN.md section 24; the contracts -- the bits of the loops -- are in spmvHip.h.
//
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
//
// Hierarchy.  Every level's matrix, prolongator, restriction and A P are handles made by the library's own entry points
// (spmvHipCsrTranspose, spmvHipSpGEMM), so their bits are pinned there.  The cycle's vector kernels are ops of the Krylov
// files' fused-pass kernel (krylov.hpp: 16-byte accesses when every pointer allows, the same bits otherwise), each with the
// stop pointer of a Krylov loop.
//
// Smoothed aggregation (spmvHipAmgSetupSmoothed).  The same build with P_l = T_l - w_l D_l^-1 A_l T_l
// chained from the public sum and products: T_l is the unit prolongator above, D_l the diagonal handle of dinv_l, and
// A_l T_l, D_l (A_l T_l) are kept for the refresh.  w_l comes from amg_rho_kernel (row sums of |a_ij|, an integer max on the
// bit pattern).  The cycle's correction is then z = z + P_l e: one fused launch (amg_prolong_kernel, a lane walks two rows of
// P_l) on a level whose P_l has no row above the threshold read at setup, else P_l's serial-order SpMV into d_l and AmgAddOp.
//
// Strength filtering (spmvHipAmgSetupStrength).  The smoothed build with F_l = spmvHipCsrFilter(A_l,
// STRENGTH, theta_l, lump) in two places: the aggregation runs on F_l's pattern, and the prolongator smoother
// (dF_l = 1 / diag F_l, rho_l, w_l, D_l, F_l T_l) on F_l's values.  The Galerkin product stays R_l (A_l P_l) on the full A_l,
// and the cycle is the smoothed one, its Jacobi sweeps on dinv_l of A_l.  The refresh runs spmvHipCsrFilterRefresh first:
// the kept sets are the build's.
//
// Chebyshev smoother (spmvHipAmgSetSmoother).  A hierarchy of any of the three setups may smooth with
// the three-term recurrence on D^-1 A instead of damped Jacobi: per level lambda_max = lambdaScale * rho_l, rho_l from
// amg_rho_kernel on A_l and dinv_l (the last level too, and A_l -- not F_l -- on a strength hierarchy), the pairs (a_k, b_k)
// computed on the host (chebTable) and kept in DEVICE memory, where the two passes (AmgChebFirstOp, AmgChebStepOp) read
// them: a refresh rewrites the table in place and a captured cycle sees the new values.  The recurrence's d is the level's
// d_l.  A step is one serial-order SpMV and one pass, as a Jacobi sweep is: the launch count is the formula of the sweeps.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "device_prims.hpp"
#include "krylov.hpp"

namespace spmvhip {

struct AmgLevel {
    spmat A{}, P{}, R{}, AP{};          // A: levels below 0 only (level 0 is the caller's); P, R, AP: all but the last level
    spmat T{}, D{}, AT{}, DAT{};        // smoothed, all but the last level: the unit prolongator, diag(dinv), A T, D (A T)
    spmat F{};                          // strength, all but the last level: the filtered A, which then stands for A in D, AT
    double theta = 0.0;                 // ... and its threshold
    double* dF = nullptr;               // ... and 1 / its diagonal
    uint64_t M = 0, nnz = 0, nAgg = 0;
    const uint32_t* agg = nullptr;      // the column array of the unit prolongator (P, or T when smoothed)
    double w = 0.0;                     // smoothed: the damping of P
    bool fused = false;                 // smoothed: no row of P is above the threshold, the correction is one pass
    double* dinv = nullptr;
    double *r = nullptr, *z = nullptr;  // below level 0: the restricted residual and the correction
    double *t = nullptr, *d = nullptr;
    // Chebyshev: rho of A_l and dinv_l, the interval, and the nCoef pairs (a_k, b_k) on the device (null when nCoef = 0)
    double rhoS = 0.0, lmax = 0.0, lmin = 0.0;
    uint32_t nCoef = 0;
    double2* coef = nullptr;
};

struct AmgHierarchy {
    uint32_t seed = 0, nu1 = 1, nu2 = 1, nuCoarse = 8;
    double omega = 2.0 / 3.0;
    bool smoothed = false;
    double omegaP = 0.0;                // smoothed: the caller's damping of P, 0: (4/3) / rho_l per level
    uint32_t fuseMax = 0;               // smoothed: the longest row of P that the fused correction takes (0: never fused)
    bool strength = false;              // smoothed on the strength-filtered F_l
    double theta = 0.0, thetaScale = 0.0;   // strength: theta_0, and theta_{l+1} = theta_l * thetaScale
    int smoother = SPMV_AMG_SMOOTHER_JACOBI;    // of the cycle (spmvHipAmgSetSmoother)
    double eigRatio = 10.0, lambdaScale = 1.0;  // Chebyshev: lambda_min = lambda_max / eigRatio, lambda_max = lambdaScale * rho_l
    std::vector<AmgLevel> lv;
    spmvAmgInfo info{};
};

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

// P's row pointers and values; dinv from the one stored diagonal entry of every row (*bad = the first row without exactly one)
__global__ __launch_bounds__(AG_THREADS) void amg_ones_kernel(uint64_t n, double* __restrict__ v) {
    const uint64_t r = linear_block() * AG_THREADS + threadIdx.x;
    if (r < n) v[r] = 1.0;
}
template <typename I>
__global__ __launch_bounds__(AG_THREADS) void amg_dinv_kernel(uint64_t M, const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                                              const double* __restrict__ AS, double* __restrict__ dinv, uint32_t* __restrict__ bad) {
    const uint64_t r = linear_block() * AG_THREADS + threadIdx.x;
    if (r >= M) return;
    uint32_t count = 0;
    double dv = 0.0;
    for (uint64_t p = IRP[r], e = IRP[r + 1]; p < e; ++p)
        if (JA[p] == r) { ++count; dv = AS[p]; }
    if (count != 1) { atomicMin(bad, (uint32_t)r); return; }
    dinv[r] = 1.0 / dv;
}

// g_i = |dinv_i| * (the sum of |a_ip| in stored order); *rhoBits = the largest g_i as bits (non-negative doubles order as
// their bit patterns), *bad = the first row whose g_i is not finite
template <typename I>
__global__ __launch_bounds__(AG_THREADS) void amg_rho_kernel(uint64_t M, const I* __restrict__ IRP, const double* __restrict__ AS,
                                                             const double* __restrict__ dinv, unsigned long long* __restrict__ rhoBits,
                                                             uint32_t* __restrict__ bad) {
    const uint64_t r = linear_block() * AG_THREADS + threadIdx.x;
    unsigned long long bits = 0;
    if (r < M) {
        double s = 0.0;
        for (uint64_t p = IRP[r], e = IRP[r + 1]; p < e; ++p) s = s + fabs(AS[p]);
        const double g = fabs(dinv[r]) * s;
        if (isfinite(g)) bits = (unsigned long long)__double_as_longlong(g);
        else atomicMin(bad, (uint32_t)r);
    }
    for (int off = 32; off; off >>= 1) bits = max(bits, (unsigned long long)__shfl_xor(bits, off));
    if (threadIdx.x % 64 == 0 && bits) atomicMax(rhoBits, bits);
}

// ------------------------------------------------------------------------------------------------ the cycle's passes
struct StopMode {
    const uint32_t* stop;
    __device__ int mode(const KState*) const { return !(stop && *stop); }
};
struct AmgZeroOp : StopMode {                   // z = +0.0
    static constexpr int NDOT = 0;
    double* z;
    struct R {};
    template <bool VEC> __device__ void load(uint64_t, bool, R&) const {}
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R&, double&, double&) const { st2<VEC>(z, i, two, make_double2(0.0, 0.0)); }
};
struct AmgFirstOp : StopMode {                  // z = omega * (dinv * r)
    static constexpr int NDOT = 0;
    const double* r; const double* dinv; double* z; double omega;
    struct R { double2 r, d; };
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const { v.r = ld2<VEC>(r, i, two); v.d = ld2<VEC>(dinv, i, two); }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double&, double&) const {
        st2<VEC>(z, i, two, make_double2(omega * (v.d.x * v.r.x), omega * (v.d.y * v.r.y)));
    }
};
struct AmgSweepOp : StopMode {                  // z = z + omega * (dinv * (r - t))
    static constexpr int NDOT = 0;
    const double* r; const double* t; const double* dinv; double* z; double omega;
    struct R { double2 r, t, d, z; };
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const {
        v.r = ld2<VEC>(r, i, two); v.t = ld2<VEC>(t, i, two); v.d = ld2<VEC>(dinv, i, two); v.z = ld2<VEC>(z, i, two);
    }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double&, double&) const {
        st2<VEC>(z, i, two, make_double2(v.z.x + omega * (v.d.x * (v.r.x - v.t.x)), v.z.y + omega * (v.d.y * (v.r.y - v.t.y))));
    }
};
// The pair (a_k, b_k) of a Chebyshev step is one uniform 16-byte load from the level's table, made in load() with the
// slot's other loads (in step() it would come after the stores of the slot before, and every slot would wait for it alone).
template <bool FROM_Z>
struct AmgChebFirstOp : StopMode {              // k = 0: d = b_0 * (dinv * r), z = d; FROM_Z: d = b_0 * (dinv * (r - t)), z = z + d
    static constexpr int NDOT = 0;
    const double* r; const double* t; const double* dinv; double* d; double* z; const double2* c;
    struct R { double2 r, t, di, z, c; };
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const {
        v.c = *c;
        v.r = ld2<VEC>(r, i, two); v.di = ld2<VEC>(dinv, i, two);
        if (FROM_Z) { v.t = ld2<VEC>(t, i, two); v.z = ld2<VEC>(z, i, two); }
    }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double&, double&) const {
        const double b = v.c.y;
        if (FROM_Z) {
            const double2 dn = make_double2(b * (v.di.x * (v.r.x - v.t.x)), b * (v.di.y * (v.r.y - v.t.y)));
            st2<VEC>(d, i, two, dn);
            st2<VEC>(z, i, two, make_double2(v.z.x + dn.x, v.z.y + dn.y));
        } else {
            const double2 dn = make_double2(b * (v.di.x * v.r.x), b * (v.di.y * v.r.y));
            st2<VEC>(d, i, two, dn);
            st2<VEC>(z, i, two, dn);
        }
    }
};
struct AmgChebStepOp : StopMode {               // k >= 1: d = a_k * d + b_k * (dinv * (r - t)), z = z + d
    static constexpr int NDOT = 0;
    const double* r; const double* t; const double* dinv; double* d; double* z; const double2* c;
    struct R { double2 r, t, di, d, z, c; };
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const {
        v.c = *c;
        v.r = ld2<VEC>(r, i, two); v.t = ld2<VEC>(t, i, two); v.di = ld2<VEC>(dinv, i, two); v.d = ld2<VEC>(d, i, two); v.z = ld2<VEC>(z, i, two);
    }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double&, double&) const {
        const double2 ab = v.c;
        const double2 dn = make_double2(ab.x * v.d.x + ab.y * (v.di.x * (v.r.x - v.t.x)), ab.x * v.d.y + ab.y * (v.di.y * (v.r.y - v.t.y)));
        st2<VEC>(d, i, two, dn);
        st2<VEC>(z, i, two, make_double2(v.z.x + dn.x, v.z.y + dn.y));
    }
};
struct AmgResidOp : StopMode {                  // d = r - t
    static constexpr int NDOT = 0;
    const double* r; const double* t; double* d;
    struct R { double2 r, t; };
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const { v.r = ld2<VEC>(r, i, two); v.t = ld2<VEC>(t, i, two); }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double&, double&) const {
        st2<VEC>(d, i, two, make_double2(v.r.x - v.t.x, v.r.y - v.t.y));
    }
};
struct AmgCorrectOp : StopMode {                // z = z + e[agg]
    static constexpr int NDOT = 0;
    const double* e; const uint32_t* agg; double* z;
    struct R { double2 z, e; };
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const {
        v.z = ld2<VEC>(z, i, two);
        uint2 a;
        if (VEC && two) a = *reinterpret_cast<const uint2*>(agg + i);      // (i is even, agg a whole allocation: 8-byte aligned)
        else a = make_uint2(agg[i], two ? agg[i + 1] : 0u);
        v.e = make_double2(e[a.x], two ? e[a.y] : 0.0);
    }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double&, double&) const {
        st2<VEC>(z, i, two, make_double2(v.z.x + v.e.x, v.z.y + v.e.y));
    }
};
// z = z + P e in one launch (the prolong-and-correct pass of a smoothed level whose P has short rows): a lane takes two
// consecutive rows of P and walks both in stored order, each sum from +0.0 -- two independent chains per lane, every lane
// of the grid its own pair, so the gathers of e overlap across the rows instead of queueing behind one lane's walk.  The
// row bounds come as one 8-byte load (i is even, irp a whole allocation), z as one 16-byte access when VEC.
template <bool VEC>
__global__ __launch_bounds__(AG_THREADS) void amg_prolong_kernel(uint64_t M, const uint32_t* __restrict__ irp, const uint32_t* __restrict__ ja,
                                                                 const double* __restrict__ as, const double* __restrict__ e, double* __restrict__ z,
                                                                 const uint32_t* __restrict__ stop) {
    const uint64_t i = (linear_block() * AG_THREADS + threadIdx.x) * 2;
    if (i >= M || (stop && *stop)) return;
    const bool two = i + 1 < M;
    const uint2 b = *reinterpret_cast<const uint2*>(irp + i);
    const uint32_t n0 = b.y - b.x, n1 = two ? irp[i + 2] - b.y : 0u, n = max(n0, n1);
    double s0 = 0.0, s1 = 0.0;
    for (uint32_t k = 0; k < n; ++k) {
        if (k < n0) s0 = s0 + as[b.x + k] * e[ja[b.x + k]];
        if (k < n1) s1 = s1 + as[b.y + k] * e[ja[b.y + k]];
    }
    const double2 zv = ld2<VEC>(z, i, two);
    st2<VEC>(z, i, two, make_double2(zv.x + s0, zv.y + s1));
}
struct AmgAddOp : StopMode {                    // z = z + d
    static constexpr int NDOT = 0;
    const double* d; double* z;
    struct R { double2 d, z; };
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const { v.d = ld2<VEC>(d, i, two); v.z = ld2<VEC>(z, i, two); }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double&, double&) const {
        st2<VEC>(z, i, two, make_double2(v.z.x + v.d.x, v.z.y + v.d.y));
    }
};

DevMat* matOf(spmat* h) { return static_cast<DevMat*>(h->dev); }

// dinv of one level; *badRow < 0 when every row has exactly one stored diagonal entry
int levelDinv(const DevMat* a, double* dinv, long* badRow, hipStream_t st) {
    uint32_t bad = UNDECIDED;
    *badRow = -1;
    if (!a->M) return EXIT_SUCCESS;
    if (deviceFlag(0xFF, st, "amg_dinv_kernel", &bad, [&](uint32_t* dFlag) {
            withIrp(a, [&](auto irp) {
                hipLaunchKernelGGL((amg_dinv_kernel<IrpT<decltype(irp)>>), gridFor(a->M), dim3(AG_THREADS), 0, st, a->M, irp, a->JA, a->AS, dinv, dFlag);
            });
        }))
        return EXIT_FAILURE;
    if (bad != UNDECIDED) *badRow = (long)bad;
    return EXIT_SUCCESS;
}

// rho of one level (the largest |dinv_i| * sum_p |a_ip|); *badRow >= 0: the first row where that is not finite
int levelRho(const DevMat* a, const double* dinv, double* rho, long* badRow, hipStream_t st) {
    struct { unsigned long long bits; uint32_t bad, pad; } h{0, UNDECIDED, 0};
    TempBuf buf;
    *badRow = -1;
    if (buf.alloc(sizeof h) != hipSuccess || hipMemcpyAsync(buf.p, &h, sizeof h, hipMemcpyHostToDevice, st) != hipSuccess) return EXIT_FAILURE;
    withIrp(a, [&](auto irp) {
        hipLaunchKernelGGL((amg_rho_kernel<IrpT<decltype(irp)>>), gridFor(a->M), dim3(AG_THREADS), 0, st, a->M, irp, a->AS, dinv,
                           buf.as<unsigned long long>(), buf.as<uint32_t>() + 2);
    });
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, buf.p, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return EXIT_FAILURE;
    if (h.bad != UNDECIDED) *badRow = (long)h.bad;
    memcpy(rho, &h.bits, 8);
    return EXIT_SUCCESS;
}

// w of a smoothed level: the caller's damping, or (4/3) / rho; refuses (with its line) a row sum that is not finite and rho = 0
int levelDamping(const AmgHierarchy* H, const DevMat* a, const double* dinv, size_t l, const char* module, double* w, hipStream_t st) {
    double rho = 0.0;
    long bad = -1;
    if (levelRho(a, dinv, &rho, &bad, st)) return buildFail(st, module, "the row sums");
    const bool zero = bad < 0 && !(rho > 0.0);                 // every row sum is 0: row 0 is the first without a rho
    if (bad >= 0 || zero) {
        fprintf(stderr, "libspmvhip: %s: row %ld of level %zu: |dinv| * (the sum of |a_ij|) is %s, the damping of the prolongator needs 0 < rho < Inf\n",
                module, zero ? 0l : bad, l, zero ? "0, as in every row" : "not finite");
        return EXIT_FAILURE;
    }
    *w = H->omegaP != 0.0 ? H->omegaP : (4.0 / 3.0) / rho;
    return EXIT_SUCCESS;
}

// the Chebyshev interval and the n pairs (a_k, b_k) of the header, a_0 = 0.0, in IEEE double with every operation rounded
// in the order written: this file is compiled with -ffp-contract=off (HIPFLAGS of the Makefile, host and device alike), so
// 2.0 * sigma - s is a product and a difference, and the pragma below says so again for this function alone
struct ChebTable { double rho = 0.0, lmax = 0.0, lmin = 0.0; std::vector<double2> ab; };
void chebTable(double rho, double eigRatio, double lambdaScale, uint32_t n, ChebTable* out) {
#pragma clang fp contract(off)
    out->rho = rho;
    const double lmax = lambdaScale * rho, lmin = lmax / eigRatio;
    out->lmax = lmax; out->lmin = lmin;
    out->ab.assign(n, make_double2(0.0, 0.0));
    if (!n) return;
    const double theta = (lmax + lmin) / 2.0, delta = (lmax - lmin) / 2.0, sigma = theta / delta;
    double s = 1.0 / sigma;
    out->ab[0] = make_double2(0.0, 1.0 / theta);
    for (uint32_t k = 1; k < n; ++k) {
        const double twice = 2.0 * sigma;
        const double sk = 1.0 / (twice - s);
        const double a = sk * s;
        const double twoS = 2.0 * sk;
        out->ab[k] = make_double2(a, twoS / delta);
        s = sk;
    }
}

// rho of level l from A_l's stored rows and dinv_l, and its table of n pairs; refuses (with its line) a row sum that is not
// finite and rho = 0.  A level without rows has rho = 0 and a table of zeros (no kernel reads it).
int levelCheb(const DevMat* a, const AmgLevel& L, size_t l, uint32_t n, double eigRatio, double lambdaScale, const char* module, ChebTable* out,
              hipStream_t st) {
    double rho = 0.0;
    long bad = -1;
    if (!a->M) { out->rho = out->lmax = out->lmin = 0.0; out->ab.assign(n, make_double2(0.0, 0.0)); return EXIT_SUCCESS; }
    if (levelRho(a, L.dinv, &rho, &bad, st)) return buildFail(st, module, "the row sums");
    const bool zero = bad < 0 && !(rho > 0.0);
    if (bad >= 0 || zero) {
        fprintf(stderr, "libspmvhip: %s: row %ld of level %zu: |dinv| * (the sum of |a_ij|) is %s, the Chebyshev smoother needs 0 < rho < Inf\n",
                module, zero ? 0l : bad, l, zero ? "0, as in every row" : "not finite");
        return EXIT_FAILURE;
    }
    chebTable(rho, eigRatio, lambdaScale, n, out);
    return EXIT_SUCCESS;
}

// the pairs a level's table holds: up to the larger of nu1 and nu2, up to nuCoarse on the last level
uint32_t chebPairs(const AmgHierarchy* H, size_t l, uint32_t nu1, uint32_t nu2, uint32_t nuCoarse) {
    return l + 1 == H->lv.size() ? nuCoarse : std::max(nu1, nu2);
}
// a table onto the device at `dst` (n pairs), synchronously
int chebUpload(double2* dst, const ChebTable& tb, hipStream_t st) {
    if (tb.ab.empty()) return EXIT_SUCCESS;
    return hipMemcpyAsync(dst, tb.ab.data(), tb.ab.size() * sizeof(double2), hipMemcpyHostToDevice, st) == hipSuccess &&
           hipStreamSynchronize(st) == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

// the serial-order selection of a handle, made now on workspace vectors so that the cycle only enqueues
int warmSpmv(spmat* h, double* x, double* y, hipStream_t st) {
    const DevMat* d = matOf(h);
    if (!d->M || !d->N) return EXIT_SUCCESS;
    if (hipMemsetAsync(x, 0, d->N * sizeof(double), st) != hipSuccess) return EXIT_FAILURE;
    if (spmvHipEnqueueAutoRows(h, x, y, st)) return EXIT_FAILURE;
    return hipStreamSynchronize(st) == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

size_t handleBytes(const spmat* h) {
    const DevMat* d = static_cast<const DevMat*>(h->dev);
    return d ? (size_t)(d->NZ * 12 + (d->M + 1) * 4 + (d->tmap ? d->NZ * 4 : 0)) : 0;
}

}  // namespace

void freeAmg(AmgHierarchy* h) {
    if (!h) return;
    for (AmgLevel& l : h->lv) {
        for (spmat* m : {&l.A, &l.P, &l.R, &l.AP, &l.T, &l.D, &l.AT, &l.DAT, &l.F})
            if (m->dev) (void)hipFreeSpmat(m);
        for (double* p : {l.dinv, l.r, l.z, l.t, l.d, l.dF}) (void)hipFree(p);
        (void)hipFree(l.coef);
    }
    delete h;
}

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

// the strength-filtered stand-in of a level's matrix and 1 / its diagonal: the build (L.theta set first) or the refresh
static int levelFilter(AmgLevel& L, spmat* cur, bool build, const char* module, spmvFilterInfo* fi, hipStream_t st) {
    const spmvFilterOpts fo{SPMV_FILTER_STRENGTH, 0, 0, L.theta, 1};
    if (build ? spmvHipCsrFilter(cur, &fo, &L.F, fi) : spmvHipCsrFilterRefresh(&L.F, cur, fi)) return buildFail(st, module, "a level's strength filter");
    if (build && hipMalloc(&L.dF, std::max<uint64_t>(L.M, 2) * sizeof(double)) != hipSuccess) return buildFail(st, module, "allocation of a level's vectors");
    long bad = -1;
    if (levelDinv(matOf(&L.F), L.dF, &bad, st) || bad >= 0) return buildFail(st, module, "the diagonal of a level's filtered matrix");
    return EXIT_SUCCESS;
}

int amgBuild(spmat* hA, const spmvAmgOpts* o, const double* omegaP, const spmvAmgStrengthOpts* strength, uint32_t fuseMax, uint32_t K, DevMat* m,
             hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    AmgHierarchy* H = m->amg = new AmgHierarchy;
    H->smoothed = omegaP != nullptr;
    H->omegaP = omegaP ? *omegaP : 0.0;
    H->fuseMax = fuseMax;
    H->strength = strength != nullptr;
    H->theta = strength && strength->theta != 0.0 ? strength->theta : 0.08;
    H->thetaScale = strength && strength->thetaScale != 0.0 ? strength->thetaScale : 0.5;
    double theta = H->theta;
    const uint64_t coarseRows = o && o->coarseRows ? o->coarseRows : 512;
    const uint32_t maxLevels = o && o->maxLevels ? o->maxLevels : SPMV_AMG_MAX_LEVELS;
    auto sweeps = [](unsigned v, uint32_t dflt) { return v == 0 ? dflt : v == SPMV_AMG_NO_SWEEPS ? 0u : v; };
    H->seed = o ? o->seed : 0u;
    H->omega = o && o->omega != 0.0 ? o->omega : 2.0 / 3.0;
    H->nu1 = sweeps(o ? o->nu1 : 0, 1); H->nu2 = sweeps(o ? o->nu2 : 0, 1); H->nuCoarse = sweeps(o ? o->nuCoarse : 0, 8);
    spmvAmgInfo& info = H->info;
    auto fail = [&](const char* what) { return buildFail(st, "multigrid setup", what); };
    auto vec = [&](double** p, uint64_t n) { return hipMalloc(p, std::max<uint64_t>(n, 2) * sizeof(double)) != hipSuccess; };
    H->lv.reserve(SPMV_AMG_MAX_LEVELS);                        // (a level is referred to while the next one is appended)
    H->lv.emplace_back();
    for (uint32_t l = 0;; ++l) {
        AmgLevel& L = H->lv[l];
        spmat* cur = l ? &L.A : hA;
        const DevMat* a = matOf(cur);
        L.M = a->M; L.nnz = a->NZ;
        info.rows[l] = L.M; info.nnz[l] = L.nnz;
        info.levels = l + 1;
        if (vec(&L.dinv, L.M) || vec(&L.t, L.M) || vec(&L.d, L.M) || (l && vec(&L.z, L.M))) return fail("allocation of a level's vectors");
        info.bytes += (l ? 5 : 3) * L.M * 8 + (l ? handleBytes(cur) : 0);
        long bad = -1;
        if (levelDinv(a, L.dinv, &bad, st)) return fail("the diagonal");
        if (bad >= 0) {
            fprintf(stderr, "libspmvhip: multigrid setup: row %ld of level %u does not hold exactly one stored diagonal entry\n", bad, l);
            return EXIT_FAILURE;
        }
        if (warmSpmv(cur, L.d, L.t, st)) return fail("the SpMV selection of a level");
        if (L.M <= coarseRows || l + 1 == maxLevels) break;
        // strength: F stands for A in the aggregation and in the smoother of P
        spmat* soc = cur;
        const double* sdinv = L.dinv;
        if (H->strength) {
            spmvFilterInfo fi{};
            L.theta = theta;
            if (levelFilter(L, cur, true, "multigrid setup", &fi, st)) return EXIT_FAILURE;
            info.tempBytes = std::max<ulong>(info.tempBytes, fi.tempBytes);
            soc = &L.F;
            sdinv = L.dF;
        }
        // aggregates -> P (its column array IS agg), R, A P, R (A P)
        uint32_t *irp = nullptr, *agg = nullptr;
        double* ones = nullptr;
        spmvAggInfo ai{};
        bool ok = hipMalloc(&irp, (L.M + 1) * 4) == hipSuccess && hipMalloc(&agg, L.M * 4) == hipSuccess && hipMalloc(&ones, L.M * 8) == hipSuccess &&
                  !aggregateCsr(matOf(soc), H->seed, K, agg, &ai, st);
        const bool alone = ok && ai.aggregates == L.M;         // every vertex its own aggregate: nothing to coarsen
        if (ok && !alone) {
            enqueueIota(L.M + 1, irp, st);
            hipLaunchKernelGGL(amg_ones_kernel, gridFor(L.M), dim3(AG_THREADS), 0, st, L.M, ones);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        }
        if (!ok || alone) {
            (void)hipFree(irp); (void)hipFree(agg); (void)hipFree(ones);
            if (alone && H->strength) {                        // the last level keeps no filtered matrix
                (void)hipFreeSpmat(&L.F);
                (void)hipFree(L.dF);
                L.dF = nullptr;
            }
            if (alone) break;
            return fail("the aggregation");
        }
        L.nAgg = ai.aggregates;
        info.aggregates[l] = L.nAgg;
        spmat* unitP = H->smoothed ? &L.T : &L.P;
        if (ownCsr(unitP, L.M, L.nAgg, L.M, irp, agg, ones)) return fail("the prolongator");
        L.agg = matOf(unitP)->JA;
        spmvSpgemmInfo s1{}, s2{};
        if (H->smoothed) {                                     // P = T - w D (A T), by the public sum and products
            if (levelDamping(H, matOf(soc), sdinv, l, "multigrid setup", &L.w, st)) return EXIT_FAILURE;
            uint32_t *dIrp = nullptr, *dJa = nullptr;
            double* dAs = nullptr;
            ok = hipMalloc(&dIrp, (L.M + 1) * 4) == hipSuccess && hipMalloc(&dJa, L.M * 4) == hipSuccess && hipMalloc(&dAs, L.M * 8) == hipSuccess;
            if (ok) {
                enqueueIota(L.M + 1, dIrp, st);
                enqueueIota(L.M, dJa, st);
                ok = hipMemcpyAsync(dAs, sdinv, L.M * 8, hipMemcpyDeviceToDevice, st) == hipSuccess && hipGetLastError() == hipSuccess &&
                     hipStreamSynchronize(st) == hipSuccess;
            }
            if (!ok) { (void)hipFree(dIrp); (void)hipFree(dJa); (void)hipFree(dAs); return fail("the diagonal handle"); }
            if (ownCsr(&L.D, L.M, L.M, L.M, dIrp, dJa, dAs)) return fail("the diagonal handle");
            spmvAddInfo sa{};
            if (spmvHipSpGEMM(soc, &L.T, nullptr, &L.AT, &s1) || spmvHipSpGEMM(&L.D, &L.AT, nullptr, &L.DAT, &s2) ||
                spmvHipCsrAdd(1.0, &L.T, -L.w, &L.DAT, nullptr, &L.P, &sa))
                return fail("a level's smoothed prolongator");
            L.fused = sa.maxRowNnz <= H->fuseMax && matOf(&L.P)->irpBytes == 4;     // (a sum's row pointers are 4-byte)
            info.tempBytes = std::max<ulong>(info.tempBytes, std::max({s1.tempBytes, s2.tempBytes, sa.tempBytes}));
            info.bytes += handleBytes(&L.T) + handleBytes(&L.D) + handleBytes(&L.AT) + handleBytes(&L.DAT);
            if (H->strength) info.bytes += handleBytes(&L.F) + L.M * 8;
            theta = theta * H->thetaScale;
        }
        if (spmvHipCsrTranspose(&L.P, &L.R) || spmvHipSpGEMM(cur, &L.P, nullptr, &L.AP, &s1)) return fail("a level's products");
        H->lv.emplace_back();
        if (spmvHipSpGEMM(&L.R, &L.AP, nullptr, &H->lv[l + 1].A, &s2)) { H->lv.pop_back(); return fail("a level's products"); }
        info.tempBytes = std::max<ulong>(info.tempBytes, std::max(s1.tempBytes, s2.tempBytes));
        info.bytes += handleBytes(&L.P) + handleBytes(&L.R) + handleBytes(&L.AP);
        if (vec(&H->lv[l + 1].r, L.nAgg)) return fail("allocation of a level's vectors");
        if (warmSpmv(&L.R, L.d, H->lv[l + 1].r, st)) return fail("the SpMV selection of a restriction");
        if (H->smoothed && !L.fused && warmSpmv(&L.P, H->lv[l + 1].r, L.d, st)) return fail("the SpMV selection of a prolongator");
    }
    double sum = 0;
    for (uint32_t l = 0; l < info.levels; ++l) sum += (double)info.nnz[l];
    info.opComplexity = info.nnz[0] ? sum / (double)info.nnz[0] : 1.0;
    info.ms = msSince(t0);
    return EXIT_SUCCESS;
}

int amgRefresh(DevMat* m, spmat* hA, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    AmgHierarchy* H = m->amg;
    auto fail = [&](const char* what) { return buildFail(st, "multigrid refresh", what); };
    for (size_t l = 0; l < H->lv.size(); ++l) {
        AmgLevel& L = H->lv[l];
        spmat* cur = l ? &L.A : hA;
        long bad = -1;
        if (levelDinv(matOf(cur), L.dinv, &bad, st)) return fail("the diagonal");
        if (bad >= 0) { fprintf(stderr, "libspmvhip: multigrid refresh: row %ld of level %zu lost its one diagonal entry\n", bad, l); return EXIT_FAILURE; }
        if (H->smoother == SPMV_AMG_SMOOTHER_CHEBYSHEV) {      // rho_l and the table again, at the table's address
            ChebTable tb;
            if (levelCheb(matOf(cur), L, l, L.nCoef, H->eigRatio, H->lambdaScale, "multigrid refresh", &tb, st)) return EXIT_FAILURE;
            if (chebUpload(L.coef, tb, st)) return fail("a level's Chebyshev table");
            L.rhoS = tb.rho; L.lmax = tb.lmax; L.lmin = tb.lmin;
        }
        if (warmSpmv(cur, L.d, L.t, st)) return fail("the SpMV selection of a level");
        if (l + 1 == H->lv.size()) break;
        if (H->smoothed) {
            spmat* soc = cur;
            const double* sdinv = L.dinv;
            if (H->strength) {
                if (levelFilter(L, cur, false, "multigrid refresh", nullptr, st)) return EXIT_FAILURE;
                soc = &L.F;
                sdinv = L.dF;
            }
            if (levelDamping(H, matOf(soc), sdinv, l, "multigrid refresh", &L.w, st)) return EXIT_FAILURE;
            if (hipMemcpyAsync(matOf(&L.D)->AS, sdinv, L.M * 8, hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
                spmvHipValuesChanged(&L.D))
                return fail("the diagonal handle");
            if (spmvHipSpGEMMRefresh(&L.AT, soc, &L.T, nullptr) || spmvHipSpGEMMRefresh(&L.DAT, &L.D, &L.AT, nullptr) ||
                spmvHipCsrAddRefresh(&L.P, 1.0, &L.T, -L.w, &L.DAT, nullptr) || spmvHipTransposeRefresh(&L.R, &L.P))
                return fail("a level's smoothed prolongator");
        }
        if (spmvHipSpGEMMRefresh(&L.AP, cur, &L.P, nullptr) || spmvHipSpGEMMRefresh(&H->lv[l + 1].A, &L.R, &L.AP, nullptr)) return fail("a level's products");
    }
    H->info.ms = msSince(t0);
    return EXIT_SUCCESS;
}

int enqueueAmgCycle(const DevMat* m, spmat* hA, const double* r0, double* z0, hipStream_t st, const uint32_t* stop, unsigned long* launches) {
    AmgHierarchy* H = m->amg;
    const size_t nl = H->lv.size();
    const double om = H->omega;
    unsigned long n = 0;
    auto pass = [&](uint64_t rows, const auto& op, std::initializer_list<const void*> ptrs) {
        bool al = true;
        for (const void* p : ptrs) al = al && aligned16(p);
        launchVec(rows, nullptr, op, al, nullptr, nullptr, st);
        ++n;
    };
    auto spmv = [&](spmat* h, const double* x, double* y) { ++n; return spmvHipEnqueueAutoRows(h, const_cast<double*>(x), y, st); };
    auto matAt = [&](size_t l) { return l ? &H->lv[l].A : hA; };
    auto sweep = [&](size_t l, const double* r, double* z) {
        AmgLevel& L = H->lv[l];
        if (spmv(matAt(l), z, L.t)) return EXIT_FAILURE;
        pass(L.M, AmgSweepOp{{stop}, r, L.t, L.dinv, z, om}, {r, L.t, L.dinv, z});
        return EXIT_SUCCESS;
    };
    // q Chebyshev steps on level l, the recurrence from k = 0 (d is the level's d_l: free at both smoothing sites)
    const bool cheb = H->smoother == SPMV_AMG_SMOOTHER_CHEBYSHEV;
    auto chebyshev = [&](size_t l, const double* r, double* z, uint32_t q, bool fromNothing) {
        AmgLevel& L = H->lv[l];
        for (uint32_t k = 0; k < q; ++k) {
            if ((k || !fromNothing) && spmv(matAt(l), z, L.t)) return EXIT_FAILURE;
            if (k) pass(L.M, AmgChebStepOp{{stop}, r, L.t, L.dinv, L.d, z, L.coef + k}, {r, L.t, L.dinv, L.d, z});
            else if (fromNothing) pass(L.M, AmgChebFirstOp<false>{{stop}, r, nullptr, L.dinv, L.d, z, L.coef}, {r, L.dinv, L.d, z});
            else pass(L.M, AmgChebFirstOp<true>{{stop}, r, L.t, L.dinv, L.d, z, L.coef}, {r, L.t, L.dinv, L.d, z});
        }
        return EXIT_SUCCESS;
    };
    for (size_t l = 0; l < nl; ++l) {                          // down
        AmgLevel& L = H->lv[l];
        const double* r = l ? L.r : r0;
        double* z = l ? L.z : z0;
        const bool last = l + 1 == nl;
        const uint32_t sweeps = last ? H->nuCoarse : H->nu1;
        if (sweeps == 0) pass(L.M, AmgZeroOp{{stop}, z}, {z});
        else if (cheb) { if (chebyshev(l, r, z, sweeps, true)) return EXIT_FAILURE; }
        else {
            pass(L.M, AmgFirstOp{{stop}, r, L.dinv, z, om}, {r, L.dinv, z});
            for (uint32_t s = 1; s < sweeps; ++s)
                if (sweep(l, r, z)) return EXIT_FAILURE;
        }
        if (last) break;
        if (spmv(matAt(l), z, L.t)) return EXIT_FAILURE;
        pass(L.M, AmgResidOp{{stop}, r, L.t, L.d}, {r, L.t, L.d});
        if (spmv(&L.R, L.d, H->lv[l + 1].r)) return EXIT_FAILURE;
    }
    for (size_t l = nl - 1; l-- > 0;) {                        // up
        AmgLevel& L = H->lv[l];
        const double* r = l ? L.r : r0;
        double* z = l ? L.z : z0;
        const double* e = H->lv[l + 1].z;
        if (!H->smoothed) pass(L.M, AmgCorrectOp{{stop}, e, L.agg, z}, {z});
        else if (L.fused) {
            const DevMat* p = matOf(&L.P);
            const dim3 grid = gridFor((L.M + 1) / 2);
            const uint32_t* irp = static_cast<const uint32_t*>(p->IRP);
            if (aligned16(z)) hipLaunchKernelGGL(amg_prolong_kernel<true>, grid, dim3(AG_THREADS), 0, st, L.M, irp, p->JA, p->AS, e, z, stop);
            else              hipLaunchKernelGGL(amg_prolong_kernel<false>, grid, dim3(AG_THREADS), 0, st, L.M, irp, p->JA, p->AS, e, z, stop);
            ++n;
        } else {                                               // (d is free: the restriction consumed it)
            if (spmv(&L.P, e, L.d)) return EXIT_FAILURE;
            pass(L.M, AmgAddOp{{stop}, L.d, z}, {L.d, z});
        }
        if (cheb) { if (chebyshev(l, r, z, H->nu2, false)) return EXIT_FAILURE; }
        else
            for (uint32_t s = 0; s < H->nu2; ++s)
                if (sweep(l, r, z)) return EXIT_FAILURE;
    }
    if (launches) *launches += n;
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

int amgSetSmoother(DevMat* m, spmat* hA, const spmvAmgSmootherOpts* o, hipStream_t st) {
    AmgHierarchy* H = m->amg;
    const size_t nl = H->lv.size();
    auto sweeps = [](unsigned v, uint32_t kept) { return v == 0 ? kept : v == SPMV_AMG_NO_SWEEPS ? 0u : v; };
    const int kind = o ? o->kind : SPMV_AMG_SMOOTHER_JACOBI;
    const uint32_t nu1 = sweeps(o ? o->nu1 : 0, H->nu1), nu2 = sweeps(o ? o->nu2 : 0, H->nu2), nuCoarse = sweeps(o ? o->nuCoarse : 0, H->nuCoarse);
    const double eigRatio = o && o->eigRatio != 0.0 ? o->eigRatio : 10.0, lambdaScale = o && o->lambdaScale != 0.0 ? o->lambdaScale : 1.0;
    // everything new is made first: a refusal leaves the hierarchy as it was
    std::vector<ChebTable> tb(nl);
    std::vector<double2*> dev(nl, nullptr);
    auto drop = [&]() { for (double2* p : dev) (void)hipFree(p); return EXIT_FAILURE; };
    if (kind == SPMV_AMG_SMOOTHER_CHEBYSHEV)
        for (size_t l = 0; l < nl; ++l) {
            const uint32_t n = chebPairs(H, l, nu1, nu2, nuCoarse);
            if (levelCheb(matOf(l ? &H->lv[l].A : hA), H->lv[l], l, n, eigRatio, lambdaScale, "multigrid smoother", &tb[l], st)) return drop();
            if (n && (hipMalloc(&dev[l], n * sizeof(double2)) != hipSuccess || chebUpload(dev[l], tb[l], st))) {
                buildFail(st, "multigrid smoother", "a level's Chebyshev table");
                return drop();
            }
        }
    if (hipStreamSynchronize(st) != hipSuccess) return drop();     // (no cycle in flight reads a table that goes)
    for (size_t l = 0; l < nl; ++l) {
        AmgLevel& L = H->lv[l];
        H->info.bytes -= L.nCoef * sizeof(double2);
        (void)hipFree(L.coef);
        L.coef = dev[l];
        L.nCoef = (uint32_t)tb[l].ab.size();
        L.rhoS = tb[l].rho; L.lmax = tb[l].lmax; L.lmin = tb[l].lmin;
        H->info.bytes += L.nCoef * sizeof(double2);
    }
    H->smoother = kind; H->eigRatio = eigRatio; H->lambdaScale = lambdaScale;
    H->nu1 = nu1; H->nu2 = nu2; H->nuCoarse = nuCoarse;
    return EXIT_SUCCESS;
}

void amgSmoother(const DevMat* m, unsigned level, spmvAmgSmootherInfo* info) {
    const AmgHierarchy* H = m->amg;
    const AmgLevel& L = H->lv[level];
    *info = spmvAmgSmootherInfo{H->smoother, H->nu1, H->nu2, H->nuCoarse, L.rhoS, L.lmax, L.lmin, L.nCoef, reinterpret_cast<const double*>(L.coef)};
}

const spmvAmgInfo* amgInfo(const DevMat* m) { return &m->amg->info; }

void amgLevel(const DevMat* m, unsigned level, spmat* dAl, const uint32_t** dAgg, const double** dDinv) {
    const AmgLevel& L = m->amg->lv[level];
    if (dAl) {
        if (level) *dAl = L.A; else memset(dAl, 0, sizeof *dAl);
        dAl->M = dAl->N = L.M; dAl->NZ = L.nnz;
        dAl->dev = nullptr;
    }
    if (dAgg) *dAgg = L.agg;
    if (dDinv) *dDinv = L.dinv;
}

void amgProlongator(const DevMat* m, unsigned level, spmat* dPl, spmat* dRl, double* omegaP) {
    const AmgLevel& L = m->amg->lv[level];
    if (dPl) { *dPl = L.P; dPl->dev = nullptr; }
    if (dRl) { *dRl = L.R; dRl->dev = nullptr; }
    if (omegaP) *omegaP = m->amg->smoothed ? L.w : 0.0;
}

bool amgIsStrength(const DevMat* m) { return m->amg->strength; }

void amgStrength(const DevMat* m, unsigned level, spmat* dFl, double* theta) {
    const AmgLevel& L = m->amg->lv[level];
    if (dFl) { *dFl = L.F; dFl->dev = nullptr; }
    if (theta) *theta = L.theta;
}

}  // namespace spmvhip
