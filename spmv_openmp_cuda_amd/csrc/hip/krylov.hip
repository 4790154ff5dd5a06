// krylov.hip -- a fixed-order dot product (spmvHipDot) and the two Krylov solvers hipSpCGCSR / hipSpBiCGStabCSR on a
// device CSR handle (contract in spmvHip.h, design in DESIGN.md section 19).  x, the iteration count and every residual
// norm are the bits of the loops written out in spmvHip.h.
//
// The dot: blocks of KB = 4096 indices, 256 lanes a block; lane t adds the products of elements 2t, 2t+1 of each of the
// block's eight 512-element slices in ascending index order from +0.0 (16-byte loads when every pointer allows, scalar
// loads otherwise: the same order), then the lanes' partials meet in the fixed tree a[t] += a[t + h], h = 128, 64, ..., 1.
// A second, single-workgroup kernel adds the block partials by the same rule (lane t: partials t, t + 256, ... in order,
// then the tree).  Ordering across workgroups comes only from that kernel boundary: no flags, tickets or spins.
//
// The solvers: every vector update of the loop is fused with the partials of the dot that follows it (x += alpha p,
// r -= alpha q and the partials of r.r in one pass), and every finish kernel also computes the loop's scalars and its
// status into a small device state block.  Every kernel that writes x, r, p or the state reads that block first and
// returns once the loop has stopped; so does every triangular solve of the preconditioner (a stop pointer).  The host
// enqueues K iterations at a time and reads the block back once per batch: iterations enqueued past the stop write
// nothing, and x is the loop's x however far the host overshoots.  What is enqueued in which order is krylovLoop of
// krylov.hpp, which the block solves share; here is the single width of it: the ops on plain vectors, the finish kernel, the
// launchers, and the read-back of the one state block.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "spmvHip.h"
#include "kernels.hpp"
#include "krylov.hpp"

namespace spmvhip {
namespace {

struct GuardedDot : DotOp {                     // u . v inside a solve
    __device__ int mode(const KState* st) const { return !st->stop; }
};

struct TtTsOp {                                 // t . t and t . s
    static constexpr int NDOT = 2;
    const double* t; const double* s;
    struct R { double2 t, s; };
    __device__ int mode(const KState* st) const { return !st->stop; }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& r) const { r.t = ld2<VEC>(t, i, two); r.s = ld2<VEC>(s, i, two); }
    template <bool VEC> __device__ void step(uint64_t, bool two, const R& r, double& a0, double& a1) const {
        madd(a0, r.t, r.t, two);
        madd(a1, r.t, r.s, two);
    }
};

struct CgUpdateOp {                             // x = x + alpha*p; r = r - alpha*q; r . r
    static constexpr int NDOT = 1;
    double* x; const double* p; double* r; const double* q;
    mutable double alpha = 0.0;
    struct R { double2 x, p, r, q; };
    __device__ int mode(const KState* st) const { if (st->stop) return 0; alpha = st->alpha; return 1; }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const {
        v.x = ld2<VEC>(x, i, two); v.p = ld2<VEC>(p, i, two); v.r = ld2<VEC>(r, i, two); v.q = ld2<VEC>(q, i, two);
    }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double& a0, double&) const {
        const double2 xn = make_double2(v.x.x + alpha * v.p.x, v.x.y + alpha * v.p.y);
        const double2 rn = make_double2(v.r.x - alpha * v.q.x, v.r.y - alpha * v.q.y);
        st2<VEC>(x, i, two, xn);
        st2<VEC>(r, i, two, rn);
        madd(a0, rn, rn, two);
    }
};

struct CgPOp {                                  // p = z (first) or p = z + beta*p
    static constexpr int NDOT = 0;
    const double* z; double* p; int first;
    mutable double beta = 0.0;
    struct R { double2 z, p; };
    __device__ int mode(const KState* st) const { if (st->stop) return 0; beta = st->beta; return 1; }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const {
        v.z = ld2<VEC>(z, i, two);
        if (!first) v.p = ld2<VEC>(p, i, two);
    }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double&, double&) const {
        st2<VEC>(p, i, two, first ? v.z : make_double2(v.z.x + beta * v.p.x, v.z.y + beta * v.p.y));
    }
};

struct BiPOp {                                  // p = r (first) or p = r + beta*(p - omega*v)
    static constexpr int NDOT = 0;
    const double* r; double* p; const double* v; int first;
    mutable double beta = 0.0, omega = 0.0;
    struct R { double2 r, p, v; };
    __device__ int mode(const KState* st) const { if (st->stop) return 0; beta = st->beta; omega = st->omega; return 1; }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& x) const {
        x.r = ld2<VEC>(r, i, two);
        if (!first) { x.p = ld2<VEC>(p, i, two); x.v = ld2<VEC>(v, i, two); }
    }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& x, double&, double&) const {
        if (first) { st2<VEC>(p, i, two, x.r); return; }
        const double d0 = x.p.x - omega * x.v.x, d1 = x.p.y - omega * x.v.y;
        st2<VEC>(p, i, two, make_double2(x.r.x + beta * d0, x.r.y + beta * d1));
    }
};

struct SOp {                                    // s = r - alpha*v; s . s
    static constexpr int NDOT = 1;
    const double* r; const double* v; double* s;
    mutable double alpha = 0.0;
    struct R { double2 r, v; };
    __device__ int mode(const KState* st) const { if (st->stop) return 0; alpha = st->alpha; return 1; }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& x) const { x.r = ld2<VEC>(r, i, two); x.v = ld2<VEC>(v, i, two); }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& x, double& a0, double&) const {
        const double2 sn = make_double2(x.r.x - alpha * x.v.x, x.r.y - alpha * x.v.y);
        st2<VEC>(s, i, two, sn);
        madd(a0, sn, sn, two);
    }
};

// running: x = (x + alpha*phat) + omega*shat; r = s - omega*t; r . r and rhat . r.  Stopped at a half step of THIS
// iteration (halfK == k): x = x + alpha*phat only.
struct BiUpdateOp {
    static constexpr int NDOT = 2;
    double* x; const double* phat; const double* shat; double* r; const double* s; const double* t; const double* rhat;
    uint64_t k;
    mutable double alpha = 0.0, omega = 0.0;
    mutable int full = 0;
    struct R { double2 x, ph, sh, s, t, rh; };
    __device__ int mode(const KState* st) const {
        full = !st->stop;
        if (!full && st->halfK != k) return 0;
        alpha = st->alpha; omega = st->omega;
        return 1;
    }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& v) const {
        v.x = ld2<VEC>(x, i, two); v.ph = ld2<VEC>(phat, i, two);
        if (full) { v.sh = ld2<VEC>(shat, i, two); v.s = ld2<VEC>(s, i, two); v.t = ld2<VEC>(t, i, two); v.rh = ld2<VEC>(rhat, i, two); }
    }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& v, double& a0, double& a1) const {
        const double h0 = v.x.x + alpha * v.ph.x, h1 = v.x.y + alpha * v.ph.y;
        if (!full) { st2<VEC>(x, i, two, make_double2(h0, h1)); return; }
        st2<VEC>(x, i, two, make_double2(h0 + omega * v.sh.x, h1 + omega * v.sh.y));
        const double2 rn = make_double2(v.s.x - omega * v.t.x, v.s.y - omega * v.t.y);
        st2<VEC>(r, i, two, rn);
        madd(a0, rn, rn, two);
        madd(a1, v.rh, rn, two);
    }
};

// the block partials of one or two dots, by the same rule: lane t adds partials t, t + 256, ... in order, then the tree.
// Lane 0 then runs the loop's scalar step `ph` for iteration k.
__global__ __launch_bounds__(KT) void krylov_finish_kernel(uint64_t nb, const double* __restrict__ part0,
                                                           const double* __restrict__ part1, int ph, uint64_t k, KState* st,
                                                           double* hist, double* out, int precond) {
    __shared__ double2 sh[KT];
    if (ph != F_DOT && ph != F_CG_INIT && ph != F_BI_INIT && st->stop) return;
    double a0 = 0.0, a1 = 0.0;
    for (uint64_t j = threadIdx.x; j < nb; j += KT) {
        a0 += part0[j];
        if (part1) a1 += part1[j];
    }
    const double2 d = tree256(make_double2(a0, a1), sh);
    if (threadIdx.x != 0) return;
    if (ph == F_DOT) *out = d.x;
    else krylovScalarStep(ph, k, d, st, hist, precond);
}

void launchFinish(uint64_t n, const double* p0, const double* p1, int ph, uint64_t k, KState* st, double* hist, double* out,
                  int precond, hipStream_t s) {
    hipLaunchKernelGGL(krylov_finish_kernel, dim3(1), dim3(KT), 0, s, blocksOf(n), p0, p1, ph, k, st, hist, out, precond);
}

// the single width of krylovLoop (krylov.hpp): one vector a role, one state block, which the host reads once per batch
struct SingleWidth {
    using Vec = double*;
    using Init = InitOp; using Dot = GuardedDot; using TtTs = TtTsOp; using CgUpdate = CgUpdateOp; using CgP = CgPOp;
    using BiP = BiPOp; using S = SOp; using BiUpdate = BiUpdateOp;
    const uint64_t n; spmat* const hA; const Precond& pc; const int pre; const hipStream_t s;
    spmvKrylovInfo& out;                        // launches and hostChecks are counted here
    Vec b = nullptr, x = nullptr, v[8] = {};
    double* p0 = nullptr; double* p1 = nullptr; // the block partials of a pass's first and second dot
    KState* st = nullptr; double* hist = nullptr;
    KState h{};                                 // the state as the host last read it
    int product(Vec in, Vec outv) { ++out.launches; return spmvHipEnqueueAutoRows(hA, in, outv, s); }
    int precond(Vec in, Vec outv) { return pc.apply(in, outv, &st->stop, &out.launches); }
    template <class Op> void vec(const Op& op, std::initializer_list<const void*> ptrs) {
        bool al = true;
        for (const void* p : ptrs) al = al && aligned16(p);
        launchVec(n, st, op, al, p0, p1, s);
        ++out.launches;
    }
    void finish(int ph, uint64_t k, int ndot) {
        launchFinish(n, p0, ndot > 1 ? p1 : nullptr, ph, k, st, hist, nullptr, pre, s);
        ++out.launches;
    }
    int afterInit(bool* done) { *done = false; return EXIT_SUCCESS; }    // not read: the first batch is enqueued whatever the init found
    int afterBatch(bool* done) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h, st, sizeof h, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++out.hostChecks;
        *done = h.stop != 0;
        return EXIT_SUCCESS;
    }
};

// the public dot's block partials: a library workspace, grown (synchronously) by the first call that needs more
struct DotWorkspace { double* p = nullptr; uint64_t blocks = 0; int dev = -1; } g_dot;   // blocks: doubles held

}  // namespace

void freeDotWorkspace() {
    if (g_dot.p) (void)devFree(g_dot.p);
    g_dot = DotWorkspace{};
}

int dotWorkspace(uint64_t doubles, double** p) {
    doubles = std::max<uint64_t>(doubles, 1);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (doubles > g_dot.blocks || dev != g_dot.dev) {
        HIP_TRY(hipDeviceSynchronize());                                 // the old workspace may still be read
        freeDotWorkspace();
        HIP_TRY(devMalloc(&g_dot.p, doubles * sizeof(double)));
        g_dot.blocks = doubles;
        g_dot.dev = dev;
    }
    *p = g_dot.p;
    return EXIT_SUCCESS;
}

int enqueueDot(uint64_t n, const double* u, const double* v, double* result, hipStream_t st) {
    double* part = nullptr;
    if (dotWorkspace(blocksOf(n), &part)) return EXIT_FAILURE;
    launchVec(n, nullptr, DotOp{u, v}, aligned16(u) && aligned16(v), part, nullptr, st);
    launchFinish(n, part, nullptr, F_DOT, 0, nullptr, nullptr, result, 0, st);
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

int krylovSolve(int bicg, spmat* hA, const DevMat* a, const DevMat* m, const double* b, double* x, const spmvKrylovOpts* o,
                spmvKrylovInfo* info, uint32_t K, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = a->M, nb = std::max<uint64_t>(blocksOf(n), 1);
    const int pre = m != nullptr;
    spmvKrylovInfo out{};
    DevBufs bufs;
    const Precond pc(m, hA, s);
    SingleWidth w{n, hA, pc, pre, s, out};
    const int nvec = bicg ? (pre ? 8 : 6) : (pre ? 4 : 3);
    for (int i = 0; i < nvec; ++i)
        if (!(w.v[i] = bufs.alloc<double>(n))) { fprintf(stderr, "libspmvhip: Krylov solve: workspace allocation failed\n"); return EXIT_FAILURE; }
    w.p0 = bufs.alloc<double>(2 * nb);
    KState* st = w.st = bufs.alloc<KState>(1);
    double* hist = w.hist = o->history ? bufs.alloc<double>(o->maxIter + 1) : nullptr;
    if (!w.p0 || !st || (o->history && !hist)) { fprintf(stderr, "libspmvhip: Krylov solve: workspace allocation failed\n"); return EXIT_FAILURE; }
    w.p1 = w.p0 + nb;
    w.b = const_cast<double*>(b);
    w.x = x;
    KState& h = w.h;
    h.maxIter = o->maxIter;
    h.tol2 = o->tol * o->tol;
    HIP_TRY(hipMemcpyAsync(st, &h, sizeof h, hipMemcpyHostToDevice, s));
    if (krylovLoop(w, bicg, pre, o->maxIter, K)) return EXIT_FAILURE;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h, st, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!h.stop) { fprintf(stderr, "libspmvhip: Krylov solve: the loop did not stop\n"); return EXIT_FAILURE; }
    if (o->history) {
        HIP_TRY(hipMemcpy(o->history, hist, (h.iterations + 1) * sizeof(double), hipMemcpyDeviceToHost));
    }
    out.status = h.status;
    out.iterations = h.iterations;
    out.rr = h.rr;
    out.bb = h.bb;
    out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = out;
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
