// amg.hip -- aggregation multigrid on the device: the hierarchy of Galerkin products (the three spmvHipAmgSetup* calls,
// spmvHipAmgRefresh) and its V-cycle (spmvHipAmgApply, and the dM of the Krylov solvers).  The contracts -- the bits of the
// loops -- are in spmvHip.h; the aggregation is aggregate.hip.
// Hierarchy.  Every level's matrix, prolongator, restriction and A P are handles made by the library's own entry points
// (transpose, product, sum, filter), so their bits are pinned there.  A level is ONE recipe run in two modes, BUILD and
// REFRESH (levelFilter, smoothProlongator, galerkin below); what a hierarchy is made of is its AmgKind.
// Cycle.  Its vector kernels are ops of the Krylov files' fused-pass kernel (krylov.hpp: 16-byte accesses when every pointer
// allows, the same bits otherwise), each with the stop pointer of a Krylov loop.  A smoothing step is an SpMV into t_l and one
// pass, damped Jacobi or Chebyshev alike: the launch count is the formula of the sweeps.  A Gauss-Seidel sweep is kernels of
// this file: one launch per colour of the level, or one workgroup for a whole sweep of a small level.
// The cycle for a block of vectors (spmvHipAmgApplyBlock, and the dM of the block solvers) is the same loop over row-major
// blocks: SpMM passes and ops of the block pass (krylov_block.hpp), on a workspace that spmvHipAmgSetBlockWidth makes.
// DESIGN.md sections 24 (the cycle), 28 (smoothed P, the fused correction), 29 (strength), 30 (Chebyshev), 31 (the recipe, the kinds),
// 32 (Gauss-Seidel), 33 (the block cycle).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <type_traits>
#include <vector>

#include "device_prims.hpp"
#include "krylov.hpp"
#include "krylov_block.hpp"

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
    // the block cycle's workspace (null on a hierarchy without a block width): M x kp row-major blocks, br and bz below level 0
    double *bt = nullptr, *bd = nullptr, *br = nullptr, *bz = nullptr;
    // Chebyshev: rho of A_l and dinv_l, the interval, and the nCoef pairs (a_k, b_k) on the device (null when nCoef = 0)
    double rhoS = 0.0, lmax = 0.0, lmin = 0.0;
    uint32_t nCoef = 0;
    double2* coef = nullptr;
    // Gauss-Seidel (null and 0 on a level that does not sweep by colours): the rows by (colour, id), the C + 1 offsets of the
    // colour classes on the device and on the host (the grids of the colour launches), and what the view reports
    uint32_t* perm = nullptr;
    uint32_t* colourPtr = nullptr;
    std::vector<uint32_t> hColourPtr;
    uint64_t maxColourRows = 0, longRows = 0;
    bool gsSmall = false;               // the whole sweep in one launch of one workgroup
    uint32_t gsLanes = 1;               // lanes per row of the sweep kernels: 1 (and a wavefront above 64 entries), or 4 .. 64
};

struct AmgHierarchy {
    uint32_t seed = 0, nu1 = 1, nu2 = 1, nuCoarse = 8;
    double omega = 2.0 / 3.0;
    AmgPlan plan{};                     // the setup's, defaults filled in
    bool smoothed() const { return plan.kind != AmgKind::PLAIN; }
    bool strength() const { return plan.kind == AmgKind::STRENGTH; }    // smoothed on the strength-filtered F_l
    int smoother = SPMV_AMG_SMOOTHER_JACOBI;    // of the cycle (spmvHipAmgSetSmoother)
    double eigRatio = 10.0, lambdaScale = 1.0;  // Chebyshev: lambda_min = lambda_max / eigRatio, lambda_max = lambdaScale * rho_l
    double gsOmega = 1.0;                       // Gauss-Seidel: the relaxation, the colouring's order and seed, forward everywhere
    int gsOrder = SPMV_COLOUR_NATURAL;
    uint32_t gsSeed = 0;
    bool gsOneWay = false;
    uint32_t blockWidth = 0;                    // the columns a block cycle may take (spmvHipAmgSetBlockWidth; 0: none) ...
    uint64_t blockBytes = 0;                    // ... and the bytes of its workspace, which info.bytes counts
    // SPMV_STORAGE_F64 | SPMV_STORAGE_F32 (spmvHipAmgSetStorage): with F32 every A_l z, R_l d and P_l e of
    // the two cycles is the f32 product of the level's handle, whose single-precision form this hierarchy built: a0Form says
    // that of the caller's level-0 handle too (it was not there before), a0Bytes what that form held when the storage was set
    int storage = SPMV_STORAGE_F64;
    bool a0Form = false;
    uint64_t a0Bytes = 0;
    std::vector<AmgLevel> lv;
    spmvAmgInfo info{};
};

namespace {

constexpr uint32_t AG_THREADS = WG_THREADS;

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
// row bounds come as one 8-byte load (i is even, irp a whole allocation), z as one 16-byte access when VEC.  V: the type P's
// values are stored in (float: P's single-precision form, widened -- exactly -- before the product; section 41).
template <bool VEC, typename V = double>
__global__ __launch_bounds__(AG_THREADS) void amg_prolong_kernel(uint64_t M, const uint32_t* __restrict__ irp, const uint32_t* __restrict__ ja,
                                                                 const V* __restrict__ as, const double* __restrict__ e, double* __restrict__ z,
                                                                 const uint32_t* __restrict__ stop) {
    const uint64_t i = (linear_block() * AG_THREADS + threadIdx.x) * 2;
    if (i >= M || (stop && *stop)) return;
    const bool two = i + 1 < M;
    const uint2 b = *reinterpret_cast<const uint2*>(irp + i);
    const uint32_t n0 = b.y - b.x, n1 = two ? irp[i + 2] - b.y : 0u, n = max(n0, n1);
    double s0 = 0.0, s1 = 0.0;
    for (uint32_t k = 0; k < n; ++k) {
        if (k < n0) s0 = s0 + (double)as[b.x + k] * e[ja[b.x + k]];
        if (k < n1) s1 = s1 + (double)as[b.y + k] * e[ja[b.y + k]];
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

// ------------------------------------------------------------------------------------------------ the block cycle's passes
// The passes above for a block of columns, as ops of the block pass (krylov_block.hpp): a lane holds the column pair
// (c, c + 1) of a row, .x and .y of every double2, and computes each with exactly the arithmetic of the single form, so a
// column never sees its neighbour.  dinv_l[i] and agg_l[i] belong to the row: one 8-byte (4-byte) load at an address that the
// P lanes of the row share.  No per-column state: mode() reads the stop pointer alone.
struct BStopMode {
    const uint32_t* stop;
    struct Sc {};
    __device__ __forceinline__ int mode(int, const KState*, Sc&) const { return !(stop && *stop); }
};
struct BAmgZeroOp : BStopMode {                 // Z = +0.0
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = 4;
    BMat z;
    struct R {};
    __device__ __forceinline__ void load(uint64_t, uint32_t, bool, const Sc&, R&) const {}
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc&, const R&, Acc&) const {
        stp(z, i, c, w0, w1, make_double2(0.0, 0.0));
    }
};
struct BAmgFirstOp : BStopMode {                // Z = omega * (dinv * R)
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = 4;
    BMat r; const double* dinv; BMat z; double omega;
    struct R { double2 r; double di; };
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& v) const { v.r = ldp(r, i, c, two); v.di = dinv[i]; }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc&, const R& v, Acc&) const {
        stp(z, i, c, w0, w1, make_double2(omega * (v.di * v.r.x), omega * (v.di * v.r.y)));
    }
};
struct BAmgSweepOp : BStopMode {                // Z = Z + omega * (dinv * (R - T))
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = 2;
    BMat r, t; const double* dinv; BMat z; double omega;
    struct R { double2 r, t, z; double di; };
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& v) const {
        v.r = ldp(r, i, c, two); v.t = ldp(t, i, c, two); v.di = dinv[i]; v.z = ldp(z, i, c, two);
    }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc&, const R& v, Acc&) const {
        stp(z, i, c, w0, w1, make_double2(v.z.x + omega * (v.di * (v.r.x - v.t.x)), v.z.y + omega * (v.di * (v.r.y - v.t.y))));
    }
};
// (the pair (a_k, b_k) is loaded in load() with the slot's blocks, as in the single forms)
template <bool FROM_Z>
struct BAmgChebFirstOp : BStopMode {            // k = 0: D = b_0 * (dinv * R), Z = D; FROM_Z: D = b_0 * (dinv * (R - T)), Z = Z + D
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = FROM_Z ? 2 : 4;
    BMat r, t; const double* dinv; BMat d, z; const double2* cf;
    struct R { double2 r, t, z, cf; double di; };
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& v) const {
        v.cf = *cf;
        v.r = ldp(r, i, c, two); v.di = dinv[i];
        if (FROM_Z) { v.t = ldp(t, i, c, two); v.z = ldp(z, i, c, two); }
    }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc&, const R& v, Acc&) const {
        const double b = v.cf.y;
        if (FROM_Z) {
            const double2 dn = make_double2(b * (v.di * (v.r.x - v.t.x)), b * (v.di * (v.r.y - v.t.y)));
            stp(d, i, c, w0, w1, dn);
            stp(z, i, c, w0, w1, make_double2(v.z.x + dn.x, v.z.y + dn.y));
        } else {
            const double2 dn = make_double2(b * (v.di * v.r.x), b * (v.di * v.r.y));
            stp(d, i, c, w0, w1, dn);
            stp(z, i, c, w0, w1, dn);
        }
    }
};
struct BAmgChebStepOp : BStopMode {             // k >= 1: D = a_k * D + b_k * (dinv * (R - T)), Z = Z + D
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = 2;
    BMat r, t; const double* dinv; BMat d, z; const double2* cf;
    struct R { double2 r, t, d, z, cf; double di; };
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& v) const {
        v.cf = *cf;
        v.r = ldp(r, i, c, two); v.t = ldp(t, i, c, two); v.di = dinv[i]; v.d = ldp(d, i, c, two); v.z = ldp(z, i, c, two);
    }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc&, const R& v, Acc&) const {
        const double2 ab = v.cf;
        const double2 dn = make_double2(ab.x * v.d.x + ab.y * (v.di * (v.r.x - v.t.x)), ab.x * v.d.y + ab.y * (v.di * (v.r.y - v.t.y)));
        stp(d, i, c, w0, w1, dn);
        stp(z, i, c, w0, w1, make_double2(v.z.x + dn.x, v.z.y + dn.y));
    }
};
struct BAmgResidOp : BStopMode {                // D = R - T
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = 4;
    BMat r, t, d;
    struct R { double2 r, t; };
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& v) const { v.r = ldp(r, i, c, two); v.t = ldp(t, i, c, two); }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc&, const R& v, Acc&) const {
        stp(d, i, c, w0, w1, make_double2(v.r.x - v.t.x, v.r.y - v.t.y));
    }
};
struct BAmgCorrectOp : BStopMode {              // Z(i, :) = Z(i, :) + E(agg[i], :): row agg[i] of E, a contiguous run per lane group
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = 4;
    BMat e; const uint32_t* agg; BMat z;
    struct R { double2 z, e; };
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& v) const { v.z = ldp(z, i, c, two); v.e = ldp(e, agg[i], c, two); }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc&, const R& v, Acc&) const {
        stp(z, i, c, w0, w1, make_double2(v.z.x + v.e.x, v.z.y + v.e.y));
    }
};
struct BAmgAddOp : BStopMode {                  // Z = Z + D
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = 4;
    BMat d, z;
    struct R { double2 d, z; };
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& v) const { v.d = ldp(d, i, c, two); v.z = ldp(z, i, c, two); }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc&, const R& v, Acc&) const {
        stp(z, i, c, w0, w1, make_double2(v.z.x + v.d.x, v.z.y + v.d.y));
    }
};

// ------------------------------------------------------------------------------------------------ Gauss-Seidel sweeps
// z_i = z_i + omega * (dinv_i * (r_i - t)), t the row sum of A z in stored order from the CURRENT z, for the rows of one
// colour: perm[slot] for the slots of the colour's class.  No row of a colour stores a column of that colour but its own
// diagonal, so the rows of a class neither read nor write what another row of the class writes.  A wavefront takes 64
// slots: a row of at most GS_LONG entries is walked by its lane; the longer rows of the wavefront are then taken one by
// one by all 64 lanes, which form 64 products at a time and add them in stored order (every lane the same sum).  The
// caller passes whole wavefronts (valid = false for a slot past the class), since the long rows are found by a ballot.
constexpr uint32_t GS_LONG = 64;
template <typename I>
__device__ __forceinline__ void gs_slot(bool valid, uint32_t slot, const uint32_t* __restrict__ perm, const I* __restrict__ IRP,
                                        const uint32_t* __restrict__ JA, const double* __restrict__ AS, const double* __restrict__ r,
                                        const double* __restrict__ dinv, double* z, double omega) {
    uint32_t i = 0;
    uint64_t b = 0, e = 0;
    if (valid) { i = perm[slot]; b = IRP[i]; e = IRP[i + 1]; }
    const bool isLong = e - b > GS_LONG;
    if (valid && !isLong) {
        double t = 0.0;
        for (uint64_t p = b; p < e; ++p) t = t + AS[p] * z[JA[p]];
        z[i] = z[i] + omega * (dinv[i] * (r[i] - t));
    }
    unsigned long long todo = __ballot(isLong);
    const uint32_t lane = threadIdx.x % 64;
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        const uint64_t lb = __shfl(b, src), le = __shfl(e, src);
        double t = 0.0;
        for (uint64_t p0 = lb; p0 < le; p0 += 64) {
            const uint64_t p = p0 + lane;
            const double prod = p < le ? AS[p] * z[JA[p]] : 0.0;
            const uint32_t n = (uint32_t)min((uint64_t)64, le - p0);
            for (uint32_t k = 0; k < n; ++k) t = t + __shfl(prod, (int)k);
        }
        if (lane == (uint32_t)src) z[i] = z[i] + omega * (dinv[i] * (r[i] - t));
    }
}
// G > 1 lanes per row: the lanes of a group form G products at a time from G consecutive entries of their row -- one
// contiguous piece of JA and of AS per group, where a lane per row touches a line per lane -- and every lane of the group adds
// them in stored order, so the sum is the lane-per-row form's bit for bit.  A row longer than G takes more pieces.  The
// lanes of a group hold the same slot: they run the same trips and read each other only.
template <typename I, int G>
__device__ __forceinline__ void gs_group(bool valid, uint32_t slot, const uint32_t* __restrict__ perm, const I* __restrict__ IRP,
                                         const uint32_t* __restrict__ JA, const double* __restrict__ AS, const double* __restrict__ r,
                                         const double* __restrict__ dinv, double* z, double omega) {
    if (!valid) return;
    const uint32_t sub = threadIdx.x % G, i = perm[slot];
    const uint64_t b = IRP[i], e = IRP[i + 1];
    double t = 0.0;
    for (uint64_t p0 = b; p0 < e; p0 += G) {
        const uint64_t p = p0 + sub;
        const double prod = p < e ? AS[p] * z[JA[p]] : 0.0;
        const uint32_t n = (uint32_t)min((uint64_t)G, e - p0);
        for (uint32_t k = 0; k < n; ++k) t = t + __shfl(prod, (int)k, G);
    }
    if (sub == 0) z[i] = z[i] + omega * (dinv[i] * (r[i] - t));
}
template <typename I, int G>
__device__ __forceinline__ void gs_rows(bool valid, uint32_t slot, const uint32_t* __restrict__ perm, const I* __restrict__ IRP,
                                        const uint32_t* __restrict__ JA, const double* __restrict__ AS, const double* __restrict__ r,
                                        const double* __restrict__ dinv, double* z, double omega) {
    if constexpr (G == 1) gs_slot<I>(valid, slot, perm, IRP, JA, AS, r, dinv, z, omega);
    else gs_group<I, G>(valid, slot, perm, IRP, JA, AS, r, dinv, z, omega);
}
// one colour of a sweep: the slots [cb, ce) of perm, one launch; G lanes per slot
template <typename I, int G>
__global__ __launch_bounds__(AG_THREADS) void amg_gs_colour_kernel(uint32_t cb, uint32_t ce, const uint32_t* __restrict__ perm, const I* __restrict__ IRP,
                                                                   const uint32_t* __restrict__ JA, const double* __restrict__ AS,
                                                                   const double* __restrict__ r, const double* __restrict__ dinv, double* z,
                                                                   double omega, const uint32_t* __restrict__ stop) {
    if (stop && *stop) return;
    const uint64_t slot = cb + linear_block() * (AG_THREADS / G) + threadIdx.x / G;
    gs_rows<I, G>(slot < ce, (uint32_t)slot, perm, IRP, JA, AS, r, dinv, z, omega);
}
// a whole sweep of a small level in one workgroup: the nC colours in order (backward: last first), a workgroup barrier
// between two colours -- the writes of a colour are visible to the workgroup's other wavefronts after it
template <typename I, int G>
__global__ __launch_bounds__(AG_THREADS) void amg_gs_small_kernel(uint32_t nC, int backward, const uint32_t* __restrict__ colourPtr,
                                                                  const uint32_t* __restrict__ perm, const I* __restrict__ IRP,
                                                                  const uint32_t* __restrict__ JA, const double* __restrict__ AS,
                                                                  const double* __restrict__ r, const double* __restrict__ dinv, double* z,
                                                                  double omega, const uint32_t* __restrict__ stop) {
    if (stop && *stop) return;
    const uint32_t mine = threadIdx.x / G, waveFirst = (threadIdx.x - threadIdx.x % 64) / G;     // the slot of the lane and of its wavefront
    for (uint32_t k = 0; k < nC; ++k) {
        const uint32_t c = backward ? nC - 1 - k : k;
        const uint32_t cb = colourPtr[c], ce = colourPtr[c + 1];
        for (uint64_t base = cb; base + waveFirst < ce; base += AG_THREADS / G)             // (whole wavefronts make the trips)
            gs_rows<I, G>(base + mine < ce, (uint32_t)(base + mine), perm, IRP, JA, AS, r, dinv, z, omega);
        __syncthreads();
    }
}
// the lanes per row as a compile-time constant: f(std::integral_constant<int, G>)
template <typename F>
void withLanes(uint32_t g, F&& f) {
    switch (g) {
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        default: return f(std::integral_constant<int, 1>{});
    }
}
// the view's count of long rows, and keys[s] = colour[perm[s]] (ascending: the class offsets are its bounds)
template <typename I>
__global__ __launch_bounds__(AG_THREADS) void amg_gs_classes_kernel(uint64_t M, const I* __restrict__ IRP, const uint32_t* __restrict__ colour,
                                                                    const uint32_t* __restrict__ perm, uint32_t* __restrict__ keys,
                                                                    uint32_t* __restrict__ nLong) {
    const uint64_t s = linear_block() * AG_THREADS + threadIdx.x;
    bool isLong = false;
    if (s < M) {
        keys[s] = colour[perm[s]];
        isLong = IRP[s + 1] - IRP[s] > GS_LONG;
    }
    const unsigned long long m = __ballot(isLong);
    if (threadIdx.x % 64 == 0 && m) atomicAdd(nLong, (uint32_t)__popcll(m));
}

DevMat* matOf(spmat* h) { return static_cast<DevMat*>(h->dev); }
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;                       // what a kernel's "first bad row" word holds when no row was bad

// dinv of one level; *badRow < 0 when every row has exactly one stored diagonal entry
int levelDinv(const DevMat* a, double* dinv, long* badRow, hipStream_t st) {
    uint32_t bad = NO_ROW;
    *badRow = -1;
    if (!a->M) return EXIT_SUCCESS;
    if (deviceFlag(0xFF, st, "amg_dinv_kernel", &bad, [&](uint32_t* dFlag) {
            withIrp(a, [&](auto irp) {
                hipLaunchKernelGGL((amg_dinv_kernel<IrpT<decltype(irp)>>), gridFor(a->M), dim3(AG_THREADS), 0, st, a->M, irp, a->JA, a->AS, dinv, dFlag);
            });
        }))
        return EXIT_FAILURE;
    if (bad != NO_ROW) *badRow = (long)bad;
    return EXIT_SUCCESS;
}

// rho of one level (the largest |dinv_i| * sum_p |a_ip|); *badRow >= 0: the first row where that is not finite
int levelRho(const DevMat* a, const double* dinv, double* rho, long* badRow, hipStream_t st) {
    struct { unsigned long long bits; uint32_t bad, pad; } h{0, NO_ROW, 0};
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
    if (h.bad != NO_ROW) *badRow = (long)h.bad;
    memcpy(rho, &h.bits, 8);
    return EXIT_SUCCESS;
}

// levelRho for `user` ("the Chebyshev smoother"), which needs 0 < rho < Inf: refuses (with its line) a row sum that is not
// finite and rho = 0.  A level without rows has rho = 0 and is not refused.
int checkedRho(const DevMat* a, const double* dinv, size_t l, const char* module, const char* user, double* rho, hipStream_t st) {
    long bad = -1;
    *rho = 0.0;
    if (!a->M) return EXIT_SUCCESS;
    if (levelRho(a, dinv, rho, &bad, st)) return buildFail(st, module, "the row sums");
    const bool zero = bad < 0 && !(*rho > 0.0);                // every row sum is 0: row 0 is the first without a rho
    if (bad >= 0 || zero) {
        fprintf(stderr, "libspmvhip: %s: row %ld of level %zu: |dinv| * (the sum of |a_ij|) is %s, %s needs 0 < rho < Inf\n",
                module, zero ? 0l : bad, l, zero ? "0, as in every row" : "not finite", user);
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}

// w of a smoothed level (it has rows): the caller's damping, or (4/3) / rho
int levelDamping(const AmgHierarchy* H, const DevMat* a, const double* dinv, size_t l, const char* module, double* w, hipStream_t st) {
    double rho = 0.0;
    if (checkedRho(a, dinv, l, module, "the damping of the prolongator", &rho, st)) return EXIT_FAILURE;
    *w = H->plan.omegaP != 0.0 ? H->plan.omegaP : (4.0 / 3.0) / rho;
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

// rho of level l from A_l's stored rows and dinv_l, and its table of n pairs.  A level without rows has a table of zeros
// (no kernel reads it).
int levelCheb(const DevMat* a, const AmgLevel& L, size_t l, uint32_t n, double eigRatio, double lambdaScale, const char* module, ChebTable* out,
              hipStream_t st) {
    double rho = 0.0;
    if (checkedRho(a, L.dinv, l, module, "the Chebyshev smoother", &rho, st)) return EXIT_FAILURE;
    if (a->M) chebTable(rho, eigRatio, lambdaScale, n, out);
    else { out->rho = out->lmax = out->lmin = 0.0; out->ab.assign(n, make_double2(0.0, 0.0)); }
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

// a sweep count of the options: 0 keeps `kept` (the default, or what the hierarchy has), SPMV_AMG_NO_SWEEPS is none
uint32_t sweepsOf(unsigned v, uint32_t kept) { return v == 0 ? kept : v == SPMV_AMG_NO_SWEEPS ? 0u : v; }

// an owned CSR handle of M rows with exactly one entry per row: its column from `cols` (M words, which the handle takes
// over) or, without, the row's own index; its value vals[row] (copied) or, without, 1.0
int oneEntryRows(spmat* dst, uint64_t M, uint64_t N, TempBuf* cols, const double* vals, hipStream_t st) {
    TempBuf irp, ja, as;
    if (irp.alloc((M + 1) * 4) != hipSuccess || (!cols && ja.alloc(M * 4) != hipSuccess) || as.alloc(M * 8) != hipSuccess) return EXIT_FAILURE;
    enqueueIota(M + 1, irp.as<uint32_t>(), st);
    if (!cols) enqueueIota(M, ja.as<uint32_t>(), st);
    if (!vals) hipLaunchKernelGGL(amg_ones_kernel, gridFor(M), dim3(AG_THREADS), 0, st, M, as.as<double>());
    else if (hipMemcpyAsync(as.p, vals, M * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return EXIT_FAILURE;
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return EXIT_FAILURE;
    return ownCsr(dst, M, N, M, irp.detach<uint32_t>(), (cols ? cols : &ja)->detach<uint32_t>(), as.detach<double>());
}

// ------------------------------------------------------------------------------------------------ the recipe of a level
// One description of a level, run when the hierarchy is built and when it is refreshed.  Only these
// wrappers choose between a build and a refresh entry point; a refresh reports nothing, so `info` is the build's alone.
enum class Mode { BUILD, REFRESH };
const char* moduleOf(Mode mode) { return mode == Mode::BUILD ? "multigrid setup" : "multigrid refresh"; }
int product(Mode mode, spmat* out, spmat* a, spmat* b, spmvSpgemmInfo* info) {
    return mode == Mode::BUILD ? spmvHipSpGEMM(a, b, nullptr, out, info) : spmvHipSpGEMMRefresh(out, a, b, nullptr);
}
int sum(Mode mode, spmat* out, double alpha, spmat* a, double beta, spmat* b, spmvAddInfo* info) {
    return mode == Mode::BUILD ? spmvHipCsrAdd(alpha, a, beta, b, nullptr, out, info) : spmvHipCsrAddRefresh(out, alpha, a, beta, b, nullptr);
}
int transposeOf(Mode mode, spmat* out, spmat* in) { return mode == Mode::BUILD ? spmvHipCsrTranspose(in, out) : spmvHipTransposeRefresh(out, in); }

// strength: F_l, the filtered stand-in of the level's matrix, and dF_l = 1 / its diagonal.  A build sets theta_l first and
// allocates dF_l; a refresh keeps the build's kept sets.
int levelFilter(Mode mode, AmgHierarchy* H, size_t l, spmat* cur, spmvFilterInfo* info, hipStream_t st) {
    AmgLevel& L = H->lv[l];
    const char* module = moduleOf(mode);
    const bool build = mode == Mode::BUILD;
    if (build) L.theta = l ? H->lv[l - 1].theta * H->plan.thetaScale : H->plan.theta;
    const spmvFilterOpts fo{SPMV_FILTER_STRENGTH, 0, 0, L.theta, 1};
    if (build ? spmvHipCsrFilter(cur, &fo, &L.F, info) : spmvHipCsrFilterRefresh(&L.F, cur, nullptr)) return buildFail(st, module, "a level's strength filter");
    if (build && devMalloc(&L.dF, std::max<uint64_t>(L.M, 2) * sizeof(double)) != hipSuccess) return buildFail(st, module, "allocation of a level's vectors");
    long bad = -1;
    if (levelDinv(matOf(&L.F), L.dF, &bad, st) || bad >= 0) return buildFail(st, module, "the diagonal of a level's filtered matrix");
    return EXIT_SUCCESS;
}

// D_l = diag(sdinv): made by a build, its values rewritten by a refresh
int diagonalHandle(Mode mode, AmgLevel& L, const double* sdinv, hipStream_t st) {
    if (mode == Mode::BUILD) return oneEntryRows(&L.D, L.M, L.M, nullptr, sdinv, st);
    return hipMemcpyAsync(matOf(&L.D)->AS, sdinv, L.M * 8, hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
           spmvHipValuesChanged(&L.D);
}

struct StepInfo { ulong tempBytes = 0, maxRowP = 0; };         // what a build's steps report to amgBuild

// what stands for A_l in the aggregation and in the smoother of P: F_l (with dF_l for dinv_l) on a strength hierarchy
spmat* strengthOf(AmgHierarchy* H, size_t l, spmat* cur) { return H->strength() ? &H->lv[l].F : cur; }
// smoothed: P_l = T_l - w_l D_l (A_l T_l) from the unit prolongator T_l, by the public products and sum; A_l T_l and
// D_l (A_l T_l) are kept for the refresh.  A build has made F_l before it aggregated; a refresh makes it first of all.
int smoothProlongator(Mode mode, AmgHierarchy* H, size_t l, spmat* cur, StepInfo* si, hipStream_t st) {
    AmgLevel& L = H->lv[l];
    const char* module = moduleOf(mode);
    if (mode == Mode::REFRESH && H->strength() && levelFilter(mode, H, l, cur, nullptr, st)) return EXIT_FAILURE;
    spmat* soc = strengthOf(H, l, cur);
    const double* sdinv = H->strength() ? L.dF : L.dinv;
    if (levelDamping(H, matOf(soc), sdinv, l, module, &L.w, st)) return EXIT_FAILURE;
    if (diagonalHandle(mode, L, sdinv, st)) return buildFail(st, module, "the diagonal handle");
    spmvSpgemmInfo s1{}, s2{}; spmvAddInfo sa{};
    if (product(mode, &L.AT, soc, &L.T, &s1) || product(mode, &L.DAT, &L.D, &L.AT, &s2) || sum(mode, &L.P, 1.0, &L.T, -L.w, &L.DAT, &sa))
        return buildFail(st, module, "a level's smoothed prolongator");
    si->tempBytes = std::max<ulong>(si->tempBytes, std::max({s1.tempBytes, s2.tempBytes, sa.tempBytes}));
    si->maxRowP = sa.maxRowNnz;
    return EXIT_SUCCESS;
}

// R_l = P_l^T, A_l P_l and A_{l+1} = R_l (A_l P_l) into the next level, which exists.  A refresh transposes again only for a
// smoothed kind: the plain prolongator's values are ones, and its transpose does not change.
int galerkin(Mode mode, AmgHierarchy* H, size_t l, spmat* cur, StepInfo* si, hipStream_t st) {
    AmgLevel& L = H->lv[l];
    spmvSpgemmInfo s1{}, s2{};
    const bool newR = mode == Mode::BUILD || H->smoothed();
    if ((newR && transposeOf(mode, &L.R, &L.P)) || product(mode, &L.AP, cur, &L.P, &s1) || product(mode, &H->lv[l + 1].A, &L.R, &L.AP, &s2))
        return buildFail(st, moduleOf(mode), "a level's products");
    si->tempBytes = std::max<ulong>(si->tempBytes, std::max(s1.tempBytes, s2.tempBytes));
    return EXIT_SUCCESS;
}

}  // namespace

void freeAmg(AmgHierarchy* h) {
    if (!h) return;
    for (AmgLevel& l : h->lv) {
        for (spmat* m : {&l.A, &l.P, &l.R, &l.AP, &l.T, &l.D, &l.AT, &l.DAT, &l.F})
            if (m->dev) (void)hipFreeSpmat(m);
        for (double* p : {l.dinv, l.r, l.z, l.t, l.d, l.dF, l.bt, l.bd, l.br, l.bz}) (void)devFree(p);
        (void)devFree(l.coef);
        (void)devFree(l.perm);
        (void)devFree(l.colourPtr);
    }
    delete h;
}

int amgBuild(spmat* hA, const spmvAmgOpts* o, const AmgPlan& plan, DevMat* m, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    AmgHierarchy* H = m->amg = new AmgHierarchy;
    H->plan = plan;
    if (H->plan.theta == 0.0) H->plan.theta = 0.08;
    if (H->plan.thetaScale == 0.0) H->plan.thetaScale = 0.5;
    const uint64_t coarseRows = o && o->coarseRows ? o->coarseRows : 512;
    const uint32_t maxLevels = o && o->maxLevels ? o->maxLevels : SPMV_AMG_MAX_LEVELS;
    H->seed = o ? o->seed : 0u;
    H->omega = o && o->omega != 0.0 ? o->omega : 2.0 / 3.0;
    H->nu1 = sweepsOf(o ? o->nu1 : 0, 1); H->nu2 = sweepsOf(o ? o->nu2 : 0, 1); H->nuCoarse = sweepsOf(o ? o->nuCoarse : 0, 8);
    spmvAmgInfo& info = H->info;
    auto fail = [&](const char* what) { return buildFail(st, "multigrid setup", what); };
    auto vec = [&](double** p, uint64_t n) { return devMalloc(p, std::max<uint64_t>(n, 2) * sizeof(double)) != hipSuccess; };
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
        if (H->strength()) {                                   // F stands for A in the aggregation and in the smoother of P
            spmvFilterInfo fi{};
            if (levelFilter(Mode::BUILD, H, l, cur, &fi, st)) return EXIT_FAILURE;
            info.tempBytes = std::max<ulong>(info.tempBytes, fi.tempBytes);
        }
        // aggregates -> the unit prolongator (its column array IS agg): P, or T of a smoothed P
        TempBuf agg;
        spmvAggInfo ai{};
        if (agg.alloc(L.M * 4) != hipSuccess || aggregateCsr(matOf(strengthOf(H, l, cur)), H->seed, plan.K, agg.as<uint32_t>(), &ai, st)) return fail("the aggregation");
        if (ai.aggregates == L.M) {                            // every vertex its own aggregate: nothing to coarsen
            if (H->strength()) { (void)hipFreeSpmat(&L.F); (void)devFree(L.dF); L.dF = nullptr; }     // the last level keeps no filtered matrix
            break;
        }
        L.nAgg = ai.aggregates;
        info.aggregates[l] = L.nAgg;
        spmat* unitP = H->smoothed() ? &L.T : &L.P;
        if (oneEntryRows(unitP, L.M, L.nAgg, &agg, nullptr, st)) return fail("the prolongator");
        L.agg = matOf(unitP)->JA;
        StepInfo si;
        if (H->smoothed()) {
            if (smoothProlongator(Mode::BUILD, H, l, cur, &si, st)) return EXIT_FAILURE;
            L.fused = si.maxRowP <= H->plan.fuseMax && matOf(&L.P)->irpBytes == 4;     // (a sum's row pointers are 4-byte)
            info.bytes += handleBytes(&L.T) + handleBytes(&L.D) + handleBytes(&L.AT) + handleBytes(&L.DAT);
            if (H->strength()) info.bytes += handleBytes(&L.F) + L.M * 8;
        }
        H->lv.emplace_back();                                  // (A_{l+1} goes into the next level)
        if (galerkin(Mode::BUILD, H, l, cur, &si, st)) { H->lv.pop_back(); return EXIT_FAILURE; }
        info.tempBytes = std::max<ulong>(info.tempBytes, si.tempBytes);
        info.bytes += handleBytes(&L.P) + handleBytes(&L.R) + handleBytes(&L.AP);
        if (vec(&H->lv[l + 1].r, L.nAgg)) return fail("allocation of a level's vectors");
        if (warmSpmv(&L.R, L.d, H->lv[l + 1].r, st)) return fail("the SpMV selection of a restriction");
        if (H->smoothed() && !L.fused && warmSpmv(&L.P, H->lv[l + 1].r, L.d, st)) return fail("the SpMV selection of a prolongator");
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
    StepInfo none;                                             // (a refresh reports nothing)
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
        if (H->smoothed() && smoothProlongator(Mode::REFRESH, H, l, cur, &none, st)) return EXIT_FAILURE;
        if (galerkin(Mode::REFRESH, H, l, cur, &none, st)) return EXIT_FAILURE;
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
    const bool f32 = H->storage == SPMV_STORAGE_F32;          // (the f32 products refuse, with a line, a handle whose form is gone)
    auto spmv = [&](spmat* h, const double* x, double* y) {
        ++n;
        return f32 ? spmvHipEnqueueRowsF32(h, const_cast<double*>(x), y, st) : spmvHipEnqueueAutoRows(h, const_cast<double*>(x), y, st);
    };
    auto matAt = [&](size_t l) { return l ? &H->lv[l].A : hA; };
    // q sweeps of the hierarchy's smoother on level l, from z or from nothing (z = 0, not read): step k takes A z into t unless
    // it is the first from nothing, then makes its one pass.  (Chebyshev's d is the level's d_l: free at both smoothing sites)
    const bool cheb = H->smoother == SPMV_AMG_SMOOTHER_CHEBYSHEV;
    // one Gauss-Seidel sweep of level l (it has rows), the colours forward or backward: one launch on a small level, else one per colour
    auto gsSweep = [&](size_t l, const double* r, double* z, bool backward) {
        const AmgLevel& L = H->lv[l];
        const DevMat* a = matOf(matAt(l));
        const uint32_t nC = (uint32_t)L.hColourPtr.size() - 1;
        withIrp(a, [&](auto irp) {
            withLanes(L.gsLanes, [&](auto lanes) {
                using I = IrpT<decltype(irp)>;
                constexpr int G = decltype(lanes)::value;
                if (L.gsSmall) {
                    hipLaunchKernelGGL((amg_gs_small_kernel<I, G>), dim3(1), dim3(AG_THREADS), 0, st, nC, (int)backward, L.colourPtr, L.perm, irp, a->JA,
                                       a->AS, r, L.dinv, z, H->gsOmega, stop);
                    ++n;
                    return;
                }
                for (uint32_t k = 0; k < nC; ++k, ++n) {
                    const uint32_t c = backward ? nC - 1 - k : k, cb = L.hColourPtr[c], ce = L.hColourPtr[c + 1];
                    hipLaunchKernelGGL((amg_gs_colour_kernel<I, G>), gridFor(ce - cb, AG_THREADS / G), dim3(AG_THREADS), 0, st, cb, ce, L.perm, irp, a->JA,
                                       a->AS, r, L.dinv, z, H->gsOmega, stop);
                }
            });
        });
    };
    auto smooth = [&](size_t l, const double* r, double* z, uint32_t q, bool fromNothing) {
        AmgLevel& L = H->lv[l];
        if (L.perm) {                                          // a Gauss-Seidel level: forward before the correction, backward after
            if (fromNothing) pass(L.M, AmgZeroOp{{stop}, z}, {z});     // it unless one-way; the last level's sweeps alternate
            for (uint32_t k = 0; k < q && L.M; ++k) gsSweep(l, r, z, !H->gsOneWay && (l + 1 == nl ? (k & 1) != 0 : !fromNothing));
            return EXIT_SUCCESS;
        }
        if (q == 0 && fromNothing) pass(L.M, AmgZeroOp{{stop}, z}, {z});
        for (uint32_t k = 0; k < q; ++k) {
            const bool first = k == 0 && fromNothing;
            if (!first && spmv(matAt(l), z, L.t)) return EXIT_FAILURE;
            if (!cheb && first) pass(L.M, AmgFirstOp{{stop}, r, L.dinv, z, om}, {r, L.dinv, z});
            else if (!cheb) pass(L.M, AmgSweepOp{{stop}, r, L.t, L.dinv, z, om}, {r, L.t, L.dinv, z});
            else if (k) pass(L.M, AmgChebStepOp{{stop}, r, L.t, L.dinv, L.d, z, L.coef + k}, {r, L.t, L.dinv, L.d, z});
            else if (first) pass(L.M, AmgChebFirstOp<false>{{stop}, r, nullptr, L.dinv, L.d, z, L.coef}, {r, L.dinv, L.d, z});
            else pass(L.M, AmgChebFirstOp<true>{{stop}, r, L.t, L.dinv, L.d, z, L.coef}, {r, L.t, L.dinv, L.d, z});
        }
        return EXIT_SUCCESS;
    };
    for (size_t l = 0; l < nl; ++l) {                          // down
        AmgLevel& L = H->lv[l];
        const double* r = l ? L.r : r0;
        double* z = l ? L.z : z0;
        const bool last = l + 1 == nl;
        if (smooth(l, r, z, last ? H->nuCoarse : H->nu1, true)) return EXIT_FAILURE;
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
        if (!H->smoothed()) pass(L.M, AmgCorrectOp{{stop}, e, L.agg, z}, {z});
        else if (L.fused && !(f32 && !matOf(&L.P)->AS32)) {   // (F32 and a P without an array -- a unit P, or the form gone: the product below)
            const DevMat* p = matOf(&L.P);
            const dim3 grid = gridFor((L.M + 1) / 2);
            const uint32_t* irp = static_cast<const uint32_t*>(p->IRP);
            if (f32 && aligned16(z)) hipLaunchKernelGGL((amg_prolong_kernel<true, float>), grid, dim3(AG_THREADS), 0, st, L.M, irp, p->JA, p->AS32, e, z, stop);
            else if (f32)            hipLaunchKernelGGL((amg_prolong_kernel<false, float>), grid, dim3(AG_THREADS), 0, st, L.M, irp, p->JA, p->AS32, e, z, stop);
            else if (aligned16(z))   hipLaunchKernelGGL(amg_prolong_kernel<true>, grid, dim3(AG_THREADS), 0, st, L.M, irp, p->JA, p->AS, e, z, stop);
            else                     hipLaunchKernelGGL(amg_prolong_kernel<false>, grid, dim3(AG_THREADS), 0, st, L.M, irp, p->JA, p->AS, e, z, stop);
            ++n;
        } else {                                               // (d is free: the restriction consumed it)
            if (spmv(&L.P, e, L.d)) return EXIT_FAILURE;
            pass(L.M, AmgAddOp{{stop}, L.d, z}, {L.d, z});
        }
        if (smooth(l, r, z, H->nu2, false)) return EXIT_FAILURE;
    }
    if (launches) *launches += n;
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

// The loop of enqueueAmgCycle for k columns at once: every A_l z, R_l d and P_l e one SpMM pass on the
// level's handle, every vector pass one block launch.  R0 and Z0 are the caller's blocks; everything
// below is the hierarchy's block workspace with the row stride kp of THIS k (k <= the width, so it fits).  A smoothed
// correction is always the product into d_l and an add: the launch count is the header's formula with no level fused.
int enqueueAmgCycleBlock(const DevMat* m, const DevMat* a0, uint32_t k, const Dense& R0, const Dense& Z0, hipStream_t st, const uint32_t* stop,
                         unsigned long* launches) {
    AmgHierarchy* H = m->amg;
    const size_t nl = H->lv.size();
    const double om = H->omega;
    const uint32_t kp = k + (k & 1);
    unsigned long n = 0;
    auto ws = [&](double* p) { return bmat(Dense{p, kp, true}, k, true); };
    auto pass = [&](uint64_t rows, const auto& op) {
        launchBlockVec(rows, k, nullptr, op, nullptr, nullptr, st);
        ++n;
    };
    const bool f32 = H->storage == SPMV_STORAGE_F32;
    auto spmm = [&](const DevMat* h, const BMat& x, const BMat& y) {
        ++n;
        if (f32 && !h->f32) {
            fprintf(stderr, "libspmvhip: multigrid block cycle: the hierarchy is stored in single precision, but a level's handle has lost its "
                            "single-precision value form: spmvHipValuesF32 on dA, or spmvHipAmgSetStorage again\n");
            return EXIT_FAILURE;
        }
        return h->M ? enqueueSpmm(h, k, dense(x), dense(y), st, f32) : EXIT_SUCCESS;
    };
    auto matAt = [&](size_t l) { return l ? matOf(&H->lv[l].A) : a0; };
    const bool cheb = H->smoother == SPMV_AMG_SMOOTHER_CHEBYSHEV;
    const BMat none{};
    auto smooth = [&](size_t l, const BMat& r, const BMat& z, uint32_t q, bool fromNothing) {
        AmgLevel& L = H->lv[l];
        const BMat t = ws(L.bt), d = ws(L.bd);
        if (q == 0 && fromNothing) pass(L.M, BAmgZeroOp{{stop}, z});
        for (uint32_t j = 0; j < q; ++j) {
            const bool first = j == 0 && fromNothing;
            if (!first && spmm(matAt(l), z, t)) return EXIT_FAILURE;
            if (!cheb && first) pass(L.M, BAmgFirstOp{{stop}, r, L.dinv, z, om});
            else if (!cheb) pass(L.M, BAmgSweepOp{{stop}, r, t, L.dinv, z, om});
            else if (j) pass(L.M, BAmgChebStepOp{{stop}, r, t, L.dinv, d, z, L.coef + j});
            else if (first) pass(L.M, BAmgChebFirstOp<false>{{stop}, r, none, L.dinv, d, z, L.coef});
            else pass(L.M, BAmgChebFirstOp<true>{{stop}, r, t, L.dinv, d, z, L.coef});
        }
        return EXIT_SUCCESS;
    };
    const BMat r0 = bmat(R0, k, false), z0 = bmat(Z0, k, false);
    for (size_t l = 0; l < nl; ++l) {                          // down
        AmgLevel& L = H->lv[l];
        const BMat r = l ? ws(L.br) : r0, z = l ? ws(L.bz) : z0, t = ws(L.bt), d = ws(L.bd);
        const bool last = l + 1 == nl;
        if (smooth(l, r, z, last ? H->nuCoarse : H->nu1, true)) return EXIT_FAILURE;
        if (last) break;
        if (spmm(matAt(l), z, t)) return EXIT_FAILURE;
        pass(L.M, BAmgResidOp{{stop}, r, t, d});
        if (spmm(matOf(&L.R), d, ws(H->lv[l + 1].br))) return EXIT_FAILURE;
    }
    for (size_t l = nl - 1; l-- > 0;) {                        // up
        AmgLevel& L = H->lv[l];
        const BMat r = l ? ws(L.br) : r0, z = l ? ws(L.bz) : z0, d = ws(L.bd), e = ws(H->lv[l + 1].bz);
        if (!H->smoothed()) pass(L.M, BAmgCorrectOp{{stop}, e, L.agg, z});
        else {                                                 // (d is free: the restriction consumed it)
            if (spmm(matOf(&L.P), e, d)) return EXIT_FAILURE;
            pass(L.M, BAmgAddOp{{stop}, d, z});
        }
        if (smooth(l, r, z, H->nu2, false)) return EXIT_FAILURE;
    }
    if (launches) *launches += n;
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

// the workspace of a block cycle for up to `width` columns (0: none).  Everything new is made before anything old is
// dropped; the stream is synchronised in between, so no cycle in flight uses a block that goes.
int amgSetBlockWidth(DevMat* m, uint32_t width, hipStream_t st) {
    AmgHierarchy* H = m->amg;
    const size_t nl = H->lv.size();
    const uint64_t kp = (uint64_t)width + (width & 1);
    std::vector<double*> nw(4 * nl, nullptr);                  // t, d, r, z of every level
    auto drop = [&]() { for (double* p : nw) (void)devFree(p); return EXIT_FAILURE; };
    uint64_t bytes = 0;
    if (width) {
        if (H->lv[0].M && kp > UINT64_MAX / 8 / H->lv[0].M) {
            fprintf(stderr, "libspmvhip: multigrid block width: %lu rows x %lu columns x 8 bytes do not fit 64 bits\n", (unsigned long)H->lv[0].M,
                    (unsigned long)kp);
            return EXIT_FAILURE;
        }
        for (size_t l = 0; l < nl; ++l) {
            const uint64_t one = H->lv[l].M * kp * 8;
            for (size_t v = 0; v < (l ? 4u : 2u); ++v) {
                if (devMalloc(&nw[4 * l + v], std::max<uint64_t>(one, 16)) != hipSuccess) {
                    (void)hipGetLastError();
                    fprintf(stderr, "libspmvhip: multigrid block width: allocation of level %zu's %lu-byte block failed\n", l, (unsigned long)one);
                    return drop();
                }
                bytes += one;
            }
        }
    }
    if (hipStreamSynchronize(st) != hipSuccess) return drop();
    for (size_t l = 0; l < nl; ++l) {
        AmgLevel& L = H->lv[l];
        for (double* p : {L.bt, L.bd, L.br, L.bz}) (void)devFree(p);
        L.bt = nw[4 * l]; L.bd = nw[4 * l + 1]; L.br = nw[4 * l + 2]; L.bz = nw[4 * l + 3];
    }
    H->info.bytes = H->info.bytes - H->blockBytes + bytes;
    H->blockBytes = bytes;
    H->blockWidth = width;
    return EXIT_SUCCESS;
}

// The hierarchy's products from single-precision storage (contract in spmvHip.h, design in DESIGN.md section 41).  F32: the form
// on the caller's level-0 handle, on every A_l below it and on every R_l and P_l, all or none -- a refused allocation releases
// what this call built.  F64: those forms released (the level-0 form only if this hierarchy built it).  Refused on a hierarchy
// with a Gauss-Seidel level: its sweeps read AS in kernels of their own.  Synchronous.
int amgSetStorage(DevMat* m, spmat* hA, int storage, hipStream_t st) {
    AmgHierarchy* H = m->amg;
    const size_t nl = H->lv.size();
    const char* who = "spmvHipAmgSetStorage";
    DevMat* a0 = matOf(hA);
    std::vector<DevMat*> own;                                  // the hierarchy's own handles that a product of the cycle streams
    for (size_t l = 0; l < nl; ++l) {
        if (l) own.push_back(matOf(&H->lv[l].A));
        if (l + 1 < nl) { own.push_back(matOf(&H->lv[l].R)); own.push_back(matOf(&H->lv[l].P)); }
    }
    if (storage == SPMV_STORAGE_F64) {
        for (DevMat* d : own) valuesF32Drop(d);
        if (H->a0Form) valuesF32Drop(a0);
        H->a0Form = false; H->a0Bytes = 0;
        H->storage = SPMV_STORAGE_F64;
        return EXIT_SUCCESS;
    }
    for (const AmgLevel& L : H->lv)
        if (L.perm) {
            fprintf(stderr, "libspmvhip: %s: the hierarchy has a Gauss-Seidel level, whose sweeps read the double values in kernels of their own: "
                            "spmvHipAmgSetSmoother with JACOBI or CHEBYSHEV first\n", who);
            return EXIT_FAILURE;
        }
    const bool hadA0 = a0->f32;
    std::vector<DevMat*> built;
    bool ok = valuesF32Set(a0, 1, st, who) == EXIT_SUCCESS;
    if (ok && !hadA0) built.push_back(a0);
    for (size_t i = 0; ok && i < own.size(); ++i) {
        const bool had = own[i]->f32;
        ok = valuesF32Set(own[i], 1, st, who) == EXIT_SUCCESS;
        if (ok && !had) built.push_back(own[i]);
    }
    if (!ok) {
        for (DevMat* d : built) valuesF32Drop(d);
        fprintf(stderr, "libspmvhip: %s: building the single-precision forms failed: the hierarchy keeps its storage\n", who);
        return EXIT_FAILURE;
    }
    H->a0Form = H->a0Form || !hadA0;
    H->a0Bytes = a0->f32Info.bytes;
    H->storage = SPMV_STORAGE_F32;
    return EXIT_SUCCESS;
}

void amgStorage(const DevMat* m, spmvAmgStorageInfo* info) {
    const AmgHierarchy* H = m->amg;
    const size_t nl = H->lv.size();
    uint64_t bytes = 0;
    if (H->storage == SPMV_STORAGE_F32) {
        bytes = H->a0Bytes;
        for (size_t l = 0; l < nl; ++l) {
            if (l) bytes += static_cast<const DevMat*>(H->lv[l].A.dev)->f32Info.bytes;
            if (l + 1 < nl) bytes += static_cast<const DevMat*>(H->lv[l].R.dev)->f32Info.bytes + static_cast<const DevMat*>(H->lv[l].P.dev)->f32Info.bytes;
        }
    }
    *info = spmvAmgStorageInfo{H->storage, (unsigned)nl, (ulong)bytes};
}

void amgBlockState(const DevMat* m, uint32_t* width, uint64_t* bytes, bool* gaussSeidel) {
    const AmgHierarchy* H = m->amg;
    *width = H->blockWidth;
    *bytes = H->blockBytes;
    *gaussSeidel = false;
    for (const AmgLevel& L : H->lv) *gaussSeidel = *gaussSeidel || L.perm != nullptr;
}

// a level's Gauss-Seidel lists go, with their bytes (the stream is synchronised: no cycle in flight reads them)
static void dropGsLists(AmgHierarchy* H, AmgLevel& L) {
    if (!L.perm) return;
    H->info.bytes -= L.M * 4 + L.hColourPtr.size() * 4;
    (void)devFree(L.perm);
    (void)devFree(L.colourPtr);
    L.perm = L.colourPtr = nullptr;
    L.hColourPtr.clear();
    L.maxColourRows = L.longRows = 0;
    L.gsSmall = false;
    L.gsLanes = 1;
}

int amgSetSmoother(DevMat* m, spmat* hA, const spmvAmgSmootherOpts* o, hipStream_t st) {
    AmgHierarchy* H = m->amg;
    const size_t nl = H->lv.size();
    const int kind = o ? o->kind : SPMV_AMG_SMOOTHER_JACOBI;
    const uint32_t nu1 = sweepsOf(o ? o->nu1 : 0, H->nu1), nu2 = sweepsOf(o ? o->nu2 : 0, H->nu2), nuCoarse = sweepsOf(o ? o->nuCoarse : 0, H->nuCoarse);
    const double eigRatio = o && o->eigRatio != 0.0 ? o->eigRatio : 10.0, lambdaScale = o && o->lambdaScale != 0.0 ? o->lambdaScale : 1.0;
    // everything new is made first: a refusal leaves the hierarchy as it was
    std::vector<ChebTable> tb(nl);
    std::vector<double2*> dev(nl, nullptr);
    auto drop = [&]() { for (double2* p : dev) (void)devFree(p); return EXIT_FAILURE; };
    if (kind == SPMV_AMG_SMOOTHER_CHEBYSHEV)
        for (size_t l = 0; l < nl; ++l) {
            const uint32_t n = chebPairs(H, l, nu1, nu2, nuCoarse);
            if (levelCheb(matOf(l ? &H->lv[l].A : hA), H->lv[l], l, n, eigRatio, lambdaScale, "multigrid smoother", &tb[l], st)) return drop();
            if (n && (devMalloc(&dev[l], n * sizeof(double2)) != hipSuccess || chebUpload(dev[l], tb[l], st))) {
                buildFail(st, "multigrid smoother", "a level's Chebyshev table");
                return drop();
            }
        }
    if (hipStreamSynchronize(st) != hipSuccess) return drop();     // (no cycle in flight reads a table that goes)
    for (size_t l = 0; l < nl; ++l) {
        AmgLevel& L = H->lv[l];
        dropGsLists(H, L);
        H->info.bytes -= L.nCoef * sizeof(double2);
        (void)devFree(L.coef);
        L.coef = dev[l];
        L.nCoef = (uint32_t)tb[l].ab.size();
        L.rhoS = tb[l].rho; L.lmax = tb[l].lmax; L.lmin = tb[l].lmin;
        H->info.bytes += L.nCoef * sizeof(double2);
    }
    H->smoother = kind; H->eigRatio = eigRatio; H->lambdaScale = lambdaScale;
    H->nu1 = nu1; H->nu2 = nu2; H->nuCoarse = nuCoarse;
    return EXIT_SUCCESS;
}

// the lanes per row of a level's sweeps: what was asked for, or (0) the largest power of two from 4 to 64 that the mean row
// fills (a level of rows of one or two entries keeps a lane per row): on the 7-point Laplacian 4 lanes measured faster than
// 8, DESIGN.md section 32
static uint32_t gsLanesFor(uint32_t asked, uint64_t M, uint64_t nnz) {
    if (asked) return asked;
    const uint64_t mean = M ? (nnz + M - 1) / M : 0;
    if (mean <= 2) return 1;
    uint32_t g = 4;
    while (g * 2 <= mean && g < 64) g *= 2;
    return g;
}

int amgSetGaussSeidel(DevMat* m, spmat* hA, const spmvAmgGsOpts* o, uint32_t smallRows, uint32_t lanes, uint32_t colourK, hipStream_t st) {
    AmgHierarchy* H = m->amg;
    const size_t nl = H->lv.size();
    const int order = o ? o->order : SPMV_COLOUR_NATURAL;
    const uint32_t seed = o ? o->seed : 0u;
    const size_t gsLevels = o && o->levels ? std::min<size_t>(o->levels, nl) : nl;
    auto fail = [&](const char* what) { return buildFail(st, "multigrid smoother", what); };
    if (H->storage == SPMV_STORAGE_F32) {                      // the colour sweeps read AS in kernels of their own (section 41)
        fprintf(stderr, "libspmvhip: spmvHipAmgSetGaussSeidel: the hierarchy is stored in single precision, which the Gauss-Seidel sweeps "
                        "do not read: spmvHipAmgSetStorage(dM, dA, SPMV_STORAGE_F64) first\n");
        return EXIT_FAILURE;
    }
    // everything new is made first: a refusal leaves the hierarchy as it was
    struct Lists { TempBuf perm, ptr; std::vector<uint32_t> h; uint64_t maxRows = 0, longRows = 0; };
    std::vector<Lists> nw(gsLevels);
    for (size_t l = 0; l < gsLevels; ++l) {
        const DevMat* a = matOf(l ? &H->lv[l].A : hA);
        const uint64_t M = a->M;
        spmvColourInfo ci{};
        TempBuf colour, keys, nLong;
        if (nw[l].perm.alloc(M * 4) != hipSuccess || colour.alloc(M * 4) != hipSuccess || keys.alloc(M * 4) != hipSuccess || nLong.alloc(4) != hipSuccess ||
            hipMemsetAsync(nLong.p, 0, 4, st) != hipSuccess)
            return fail("allocation of a level's colour lists");
        if (colourCsr(a, order, seed, colourK, colour.as<uint32_t>(), nw[l].perm.as<uint32_t>(), &ci, st)) return fail("a level's colouring");
        nw[l].h.assign(ci.colours + 1, 0u);
        if (nw[l].ptr.alloc(nw[l].h.size() * 4) != hipSuccess) return fail("allocation of a level's colour lists");
        if (M)
            withIrp(a, [&](auto irp) {
                hipLaunchKernelGGL((amg_gs_classes_kernel<IrpT<decltype(irp)>>), gridFor(M), dim3(AG_THREADS), 0, st, M, irp, colour.as<uint32_t>(),
                                   nw[l].perm.as<uint32_t>(), keys.as<uint32_t>(), nLong.as<uint32_t>());
            });
        enqueueSortedBounds(M, ci.colours, keys.as<uint32_t>(), nw[l].ptr.as<uint32_t>(), st);
        uint32_t hLong = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(nw[l].h.data(), nw[l].ptr.p, nw[l].h.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(&hLong, nLong.p, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail("a level's colour classes");
        nw[l].maxRows = ci.maxColourRows;
        nw[l].longRows = hLong;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail("the stream");     // (no cycle in flight reads a list or a table that goes)
    for (size_t l = 0; l < nl; ++l) {
        AmgLevel& L = H->lv[l];
        dropGsLists(H, L);
        H->info.bytes -= L.nCoef * sizeof(double2);
        (void)devFree(L.coef);
        L.coef = nullptr; L.nCoef = 0;
        L.rhoS = L.lmax = L.lmin = 0.0;
        if (l >= gsLevels) continue;
        L.perm = nw[l].perm.detach<uint32_t>();
        L.colourPtr = nw[l].ptr.detach<uint32_t>();
        L.hColourPtr = std::move(nw[l].h);
        L.maxColourRows = nw[l].maxRows; L.longRows = nw[l].longRows;
        L.gsSmall = L.M && L.M <= smallRows;
        L.gsLanes = gsLanesFor(lanes, L.M, L.nnz);
        H->info.bytes += L.M * 4 + L.hColourPtr.size() * 4;
    }
    H->smoother = SPMV_AMG_SMOOTHER_GAUSS_SEIDEL;
    H->gsOmega = o && o->omega != 0.0 ? o->omega : 1.0;
    H->gsOrder = order; H->gsSeed = seed; H->gsOneWay = o && o->oneWay != 0;
    H->nu1 = sweepsOf(o ? o->nu1 : 0, H->nu1); H->nu2 = sweepsOf(o ? o->nu2 : 0, H->nu2); H->nuCoarse = sweepsOf(o ? o->nuCoarse : 0, H->nuCoarse);
    return EXIT_SUCCESS;
}

void amgGaussSeidel(const DevMat* m, unsigned level, spmvAmgGsInfo* info) {
    const AmgHierarchy* H = m->amg;
    const AmgLevel& L = H->lv[level];
    *info = spmvAmgGsInfo{};
    if (!L.perm) return;
    *info = spmvAmgGsInfo{1, (unsigned)(L.hColourPtr.size() - 1), L.maxColourRows, L.longRows, L.gsSmall, H->gsOmega, H->gsOrder, H->gsSeed, H->gsOneWay,
                          L.perm, L.colourPtr};
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
    if (omegaP) *omegaP = m->amg->smoothed() ? L.w : 0.0;
}

bool amgIsStrength(const DevMat* m) { return m->amg->strength(); }

void amgStrength(const DevMat* m, unsigned level, spmat* dFl, double* theta) {
    const AmgLevel& L = m->amg->lv[level];
    if (dFl) { *dFl = L.F; dFl->dev = nullptr; }
    if (theta) *theta = L.theta;
}

}  // namespace spmvhip
