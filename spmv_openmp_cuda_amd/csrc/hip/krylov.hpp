// krylov.hpp -- what the Krylov files (krylov.hip, krylov_block.hip, gmres.hip, lanczos.hip) share: the blocks and lanes of the
// fixed-order dot, the element-pair loads and stores, the state block of CG / BiCGStab and its scalar steps, the fixed tree,
// the fused-pass kernel and its launcher, the workspace holder, the preconditioner of a solve, and the enqueue order of CG and
// BiCGStab written once for the single and the block width (krylovLoop).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <vector>

#include "kernels.hpp"

namespace spmvhip {
namespace {

constexpr uint32_t KT = 256;                    // lanes of a block (partials) and of the finish workgroup
constexpr uint32_t KB = 4096;                   // indices of a block
constexpr uint32_t KSLICES = KB / (2 * KT);     // 8 slices of 512 indices, two per lane
constexpr uint32_t KCHUNK = 4;                  // slices whose loads a lane issues together

template <bool VEC>
__device__ __forceinline__ double2 ld2(const double* p, uint64_t i, bool two) {
    if (VEC && two) return *reinterpret_cast<const double2*>(p + i);
    return make_double2(p[i], two ? p[i + 1] : 0.0);
}
template <bool VEC>
__device__ __forceinline__ void st2(double* p, uint64_t i, bool two, double2 v) {
    if (VEC && two) { *reinterpret_cast<double2*>(p + i) = v; return; }
    p[i] = v.x;
    if (two) p[i + 1] = v.y;
}
// acc += a.x * b.x, then a.y * b.y when the pair is whole (a missing element adds nothing: acc is never -0.0)
__device__ __forceinline__ void madd(double& acc, double2 a, double2 b, bool two) {
    acc += a.x * b.x;
    if (two) acc += a.y * b.y;
}

// the loop's scalars and its status (written only by the finish kernels, by one lane)
struct KState {
    uint32_t stop;          // 0 while the loop runs
    int32_t  status;        // SPMV_KRYLOV_* once stopped
    uint64_t iterations;
    uint64_t halfK;         // BiCGStab: the iteration whose x = x + alpha*phat is still to be written (0: none)
    uint64_t maxIter;
    double   tol2, rr, bb, thresh, rz, alpha, beta, omega, rho, rhoOld;
};

enum Phase : int { F_DOT, F_CG_INIT, F_CG_RZ, F_CG_ALPHA, F_CG_RR, F_BI_INIT, F_BI_ALPHA, F_BI_SS, F_BI_OMEGA, F_BI_RR };

// the loop's scalar step `ph` of iteration k on one state block, d the dot (or the two dots) that the step consumes; run
// by one lane.  The single solves (krylov.hip) and the block solves (krylov_block.hip, a state block per column) share it,
// so a column of a block takes the exits of the single loop by construction.
__device__ inline void krylovScalarStep(int ph, uint64_t k, double2 d, KState* st, double* hist, int precond) {
    auto stopAt = [&](int status, uint64_t it) { st->status = status; st->iterations = it; st->stop = 1; };
    switch (ph) {
    case F_CG_INIT:
    case F_BI_INIT: {
        const double rr = d.x, bb = d.y, thresh = st->tol2 * bb;
        st->rr = rr; st->bb = bb; st->thresh = thresh;
        st->iterations = 0; st->halfK = 0; st->stop = 0; st->status = SPMV_KRYLOV_MAXITER;
        if (hist) hist[0] = rr;
        if (rr <= thresh) { stopAt(SPMV_KRYLOV_CONVERGED, 0); break; }
        if (!isfinite(rr)) { stopAt(SPMV_KRYLOV_NONFINITE, 0); break; }
        if (st->maxIter == 0) { stopAt(SPMV_KRYLOV_MAXITER, 0); break; }
        if (ph == F_CG_INIT) {
            if (!precond) st->rz = rr;
        } else {
            st->rho = rr; st->rhoOld = 1.0; st->alpha = 1.0; st->omega = 1.0;
            if (rr == 0.0) stopAt(SPMV_KRYLOV_BREAKDOWN, 0);
        }
        break;
    }
    case F_CG_RZ:                                                        // rz = dot(r, z) (k = 0), else beta = rzn / rz
        if (k == 0) st->rz = d.x;
        else { st->beta = d.x / st->rz; st->rz = d.x; }
        break;
    case F_CG_ALPHA:
        if (d.x == 0.0) stopAt(SPMV_KRYLOV_BREAKDOWN, k - 1);
        else st->alpha = st->rz / d.x;
        break;
    case F_CG_RR: {
        const double rr = d.x;
        st->rr = rr;
        if (hist) hist[k] = rr;
        if (rr <= st->thresh) stopAt(SPMV_KRYLOV_CONVERGED, k);
        else if (!isfinite(rr)) stopAt(SPMV_KRYLOV_NONFINITE, k);
        else if (k == st->maxIter) stopAt(SPMV_KRYLOV_MAXITER, k);
        else if (!precond) { st->beta = rr / st->rz; st->rz = rr; }
        break;
    }
    case F_BI_ALPHA:
        if (d.x == 0.0) stopAt(SPMV_KRYLOV_BREAKDOWN, k - 1);
        else st->alpha = st->rho / d.x;
        break;
    case F_BI_SS:
        st->rr = d.x;
        if (hist) hist[k] = d.x;
        if (d.x <= st->thresh) { st->halfK = k; stopAt(SPMV_KRYLOV_CONVERGED, k); }
        break;
    case F_BI_OMEGA:
        if (d.x == 0.0) { st->halfK = k; stopAt(SPMV_KRYLOV_BREAKDOWN, k); }
        else st->omega = d.y / d.x;
        break;
    case F_BI_RR: {
        const double rr = d.x;
        st->rr = rr;
        if (hist) hist[k] = rr;
        if (rr <= st->thresh) stopAt(SPMV_KRYLOV_CONVERGED, k);
        else if (!isfinite(rr)) stopAt(SPMV_KRYLOV_NONFINITE, k);
        else if (st->omega == 0.0) stopAt(SPMV_KRYLOV_BREAKDOWN, k);
        else if (k == st->maxIter) stopAt(SPMV_KRYLOV_MAXITER, k);
        else {
            st->rhoOld = st->rho;
            st->rho = d.y;
            if (d.y == 0.0) stopAt(SPMV_KRYLOV_BREAKDOWN, k);
            else st->beta = (st->rho / st->rhoOld) * (st->alpha / st->omega);
        }
        break;
    }
    default:
        break;
    }
}

// ------------------------------------------------------------------------------------------------ the fused passes
// Each op: NDOT dots whose partials it produces, mode(st) (0: write nothing; the stopped loop), load() the inputs of
// one element pair, step() the update and the products in order.
struct DotOp {                                  // u . v
    static constexpr int NDOT = 1;
    const double* u; const double* v;
    struct R { double2 u, v; };
    __device__ int mode(const KState*) const { return 1; }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& r) const { r.u = ld2<VEC>(u, i, two); r.v = ld2<VEC>(v, i, two); }
    template <bool VEC> __device__ void step(uint64_t, bool two, const R& r, double& a0, double&) const { madd(a0, r.u, r.v, two); }
};

struct InitOp {                                 // r = b - q (rhat = r too when given); r . r and b . b
    static constexpr int NDOT = 2;
    const double* b; const double* q; double* r; double* rhat;
    struct R { double2 b, q; };
    __device__ int mode(const KState*) const { return 1; }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& x) const { x.b = ld2<VEC>(b, i, two); x.q = ld2<VEC>(q, i, two); }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& x, double& a0, double& a1) const {
        const double2 rv = make_double2(x.b.x - x.q.x, x.b.y - x.q.y);
        st2<VEC>(r, i, two, rv);
        if (rhat) st2<VEC>(rhat, i, two, rv);
        madd(a0, rv, rv, two);
        madd(a1, x.b, x.b, two);
    }
};

// the fixed tree over the 256 lanes of a workgroup: a[t] += a[t + h] for t < h, h = 128, 64, ..., 1; valid in lane 0
__device__ __forceinline__ double2 tree256(double2 a, double2* sh) {
    const uint32_t t = threadIdx.x;
    sh[t] = a;
    __syncthreads();
#pragma unroll
    for (uint32_t h = KT / 2; h >= 1; h >>= 1) {
        if (t < h) {
            const double2 o = sh[t + h], m = sh[t];
            sh[t] = make_double2(m.x + o.x, m.y + o.y);
        }
        __syncthreads();
    }
    return sh[0];
}

// one block of KB indices: the op's update on them, and its dots' block partials into part0 / part1
template <class Op, bool VEC>
__global__ __launch_bounds__(KT) void krylov_vec_kernel(uint64_t n, const KState* __restrict__ st, Op op,
                                                        double* __restrict__ part0, double* __restrict__ part1) {
    __shared__ double2 sh[KT];
    const uint64_t blk = linear_block();
    if (blk * KB >= n || !op.mode(st)) return;                           // (a folded grid's tail); uniform: the state
    const uint64_t base = blk * KB + 2 * threadIdx.x;
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (uint32_t c = 0; c < KSLICES; c += KCHUNK) {
        typename Op::R r[KCHUNK];
#pragma unroll
        for (uint32_t u = 0; u < KCHUNK; ++u) {
            const uint64_t i = base + (uint64_t)(c + u) * (2 * KT);
            if (i < n) op.template load<VEC>(i, i + 1 < n, r[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < KCHUNK; ++u) {
            const uint64_t i = base + (uint64_t)(c + u) * (2 * KT);
            if (i < n) op.template step<VEC>(i, i + 1 < n, r[u], a0, a1);
        }
    }
    if (Op::NDOT == 0) return;
    const double2 s = tree256(make_double2(a0, a1), sh);
    if (threadIdx.x == 0) {
        part0[blk] = s.x;
        if (Op::NDOT > 1) part1[blk] = s.y;
    }
}

uint64_t blocksOf(uint64_t n) { return (n + KB - 1) / KB; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <class Op>
void launchVec(uint64_t n, const KState* st, const Op& op, bool vec, double* p0, double* p1, hipStream_t s) {
    const uint64_t nb = blocksOf(n);
    if (!nb) return;
    const dim3 grid = grid2d(nb, KT);
    if (vec) hipLaunchKernelGGL((krylov_vec_kernel<Op, true>), grid, dim3(KT), 0, s, n, st, op, p0, p1);
    else     hipLaunchKernelGGL((krylov_vec_kernel<Op, false>), grid, dim3(KT), 0, s, n, st, op, p0, p1);
}

struct DevBufs {
    std::vector<void*> ptrs;
    ~DevBufs() { for (void* p : ptrs) (void)devFree(p); }
    template <typename T> T* alloc(size_t count) {
        void* p = nullptr;
        if (devMalloc(&p, std::max<size_t>(count * sizeof(T), 16)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        ptrs.push_back(p);
        return static_cast<T*>(p);
    }
};

// M^-1 of one solve, from its checked dM (null: none, and apply is not called): the ILU(0) pair U^-1 (L^-1 in) of an
// analysed matrix handle (or, in SWEEPS mode, its Jacobi sweeps on the two triangles), the cycle of a hierarchy of hA, or G^T (G in) of an approximate-inverse factor through its
// workspace vector.  apply enqueues kernels only on the solve's stream; every one but an SpMV returns at once when
// *flag != 0; *launches grows by the kernels enqueued.
struct Precond {
    const DevMat* m; spmat* hA; hipStream_t s;
    unsigned long triLaunches = 0;              // of the two triangular solves
    Precond(const DevMat* m_, spmat* hA_, hipStream_t s_) : m(m_), hA(hA_), s(s_) {
        spmvTriInfo t{};
        if (m && m->origin != Origin::HIERARCHY && m->origin != Origin::FSAI)
            for (int uplo : {SPMV_TRI_LOWER, SPMV_TRI_UPPER}) { triInfo(m, uplo, &t); triLaunches += t.launches; }
    }
    int apply(const double* in, double* out, const uint32_t* flag, unsigned long* launches) const {
        if (m->origin == Origin::HIERARCHY) return enqueueAmgCycle(m, hA, in, out, s, flag, launches);
        if (m->origin == Origin::FSAI) {                                 // (each handle's first call chooses its kernel, as hA's does)
            FsaiPlan* const p = m->fsai;
            const auto product = p->storage == SPMV_STORAGE_F32 ? spmvHipEnqueueRowsF32 : spmvHipEnqueueAutoRows;    // (stored in single precision: the f32 products)
            if (product(&p->hG, const_cast<double*>(in), p->work, s)) return EXIT_FAILURE;
            if (product(&p->hGT, p->work, out, s)) return EXIT_FAILURE;
            *launches += 2;
            return EXIT_SUCCESS;
        }
        if (triSweepsMode(m))                                            // Jacobi sweeps on the two triangles (trisweep.hip)
            return enqueueTriSweepsApply(m, 1, Dense{const_cast<double*>(in), m->M, false}, Dense{out, m->M, false}, s, flag, launches);
        dim3 g, bl;
        enqueueTrsv(m, SPMV_TRI_LOWER, SPMV_DIAG_UNIT, in, out, s, &g, &bl, flag);
        enqueueTrsv(m, SPMV_TRI_UPPER, SPMV_DIAG_STORED, out, out, s, &g, &bl, flag);
        *launches += triLaunches;
        return EXIT_SUCCESS;
    }
};

// ------------------------------------------------------------------------------------------------ the two loops
// What CG (bicg = 0) and BiCGStab enqueue, in order, K iterations per host check.  The width W is
// the single solve (krylov.hip) or the block of columns (krylov_block.hip) and answers for everything that differs:
//   Vec; Init, Dot, TtTs, CgUpdate, CgP, BiP, S, BiUpdate   a vector, and the fused passes on it (fields in one order)
//   b, x, v[8]                          the caller's vectors and the workspace: r, p, q (, z) / r, rhat, p, v, s, t (, phat, shat)
//   product(in, out), precond(in, out)  out = A in, out = M^-1 in (asked only with a dM); not 0: the solve fails
//   vec(op, {the op's vectors}), finish(phase, iteration, dots)   one fused pass, and the finish of its dots
//   afterInit(&done), afterBatch(&done) whether the host knows the loop to have stopped; not 0: the solve fails
template <class W>
int krylovLoop(W& w, int bicg, int pre, uint64_t maxIter, uint32_t K) {
    using V = typename W::Vec;
    const V b = w.b, x = w.x, r = w.v[0], q = w.v[2];
    bool done = false;
    if (w.product(x, q)) return EXIT_FAILURE;                            // the first call for a handle chooses the kernel
    if (!bicg) {
        const V p = w.v[1], z = pre ? w.v[3] : r;
        auto rz = [&](uint64_t k) {
            if (w.precond(r, z)) return EXIT_FAILURE;
            w.vec(typename W::Dot{{r, z}}, {r, z});
            w.finish(F_CG_RZ, k, 1);
            return EXIT_SUCCESS;
        };
        w.vec(typename W::Init{b, q, r, V{}}, {b, q, r});
        w.finish(F_CG_INIT, 0, 2);
        if (w.afterInit(&done)) return EXIT_FAILURE;
        if (!done) {
            if (pre && rz(0)) return EXIT_FAILURE;
            w.vec(typename W::CgP{z, p, 1}, {z, p});
        }
        for (uint64_t k = 1; !done && k <= maxIter;) {
            const uint64_t end = std::min<uint64_t>(maxIter, k + K - 1);
            for (; k <= end; ++k) {
                if (w.product(p, q)) return EXIT_FAILURE;
                w.vec(typename W::Dot{{p, q}}, {p, q});
                w.finish(F_CG_ALPHA, k, 1);
                w.vec(typename W::CgUpdate{x, p, r, q}, {x, p, r, q});
                w.finish(F_CG_RR, k, 1);
                if (pre && rz(k)) return EXIT_FAILURE;
                w.vec(typename W::CgP{z, p, 0}, {z, p});
            }
            if (w.afterBatch(&done)) return EXIT_FAILURE;
        }
        return EXIT_SUCCESS;
    }
    const V rhat = w.v[1], p = w.v[3], vv = w.v[4], sv = w.v[5], t = q, phat = pre ? w.v[6] : p, shat = pre ? w.v[7] : sv;
    w.vec(typename W::Init{b, q, r, rhat}, {b, q, r, rhat});
    w.finish(F_BI_INIT, 0, 2);
    if (w.afterInit(&done)) return EXIT_FAILURE;
    for (uint64_t k = 1; !done && k <= maxIter;) {
        const uint64_t end = std::min<uint64_t>(maxIter, k + K - 1);
        for (; k <= end; ++k) {
            w.vec(typename W::BiP{r, p, vv, k == 1}, {r, p, vv});
            if (pre && w.precond(p, phat)) return EXIT_FAILURE;
            if (w.product(phat, vv)) return EXIT_FAILURE;
            w.vec(typename W::Dot{{rhat, vv}}, {rhat, vv});
            w.finish(F_BI_ALPHA, k, 1);
            w.vec(typename W::S{r, vv, sv}, {r, vv, sv});
            w.finish(F_BI_SS, k, 1);
            if (pre && w.precond(sv, shat)) return EXIT_FAILURE;
            if (w.product(shat, t)) return EXIT_FAILURE;
            w.vec(typename W::TtTs{t, sv}, {t, sv});
            w.finish(F_BI_OMEGA, k, 2);
            w.vec(typename W::BiUpdate{x, phat, shat, r, sv, t, rhat, k}, {x, phat, shat, r, sv, t, rhat});
            w.finish(F_BI_RR, k, 2);
        }
        if (w.afterBatch(&done)) return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}

}  // namespace
// the library's dot workspace (krylov.hip): at least `doubles` doubles on the current device, grown (device
// synchronisation, allocation) when a call needs more than any earlier one
int dotWorkspace(uint64_t doubles, double** p);
}  // namespace spmvhip
