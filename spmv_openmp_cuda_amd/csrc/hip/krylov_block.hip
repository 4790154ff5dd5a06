// krylov_block.hip -- k dots in one pass (spmvHipBlockDot) and CG / BiCGStab for a block of k right-hand sides
// (hipSpCGBlockCSR, hipSpBiCGStabBlockCSR; contract in spmvHip.h, design in DESIGN.md section 27).  These are k independent
// solves advanced in lock step: column c of X, its status, its iteration count and its residual norms are the bits of
// hipSpCGCSR / hipSpBiCGStabCSR on column c alone, while the matrix (one hipSpMMRowsCSR pass), the level schedule of the
// preconditioner (two hipSpTRSMCSR passes; two SpMM passes with an approximate-inverse factor) and every launch are shared
// by the columns.
//
// One state block (KState of krylov.hpp) per column, and the scalar steps of the single loops (krylovScalarStep) run on it
// unchanged, one workgroup per column in one finish launch.  Every fused pass reads the state of its two columns and leaves
// a stopped column alone -- its x, r, p and state are frozen however long its neighbours run on -- and a head word that the
// finish kernel sets when the last column stops is what the host reads once per K iterations and what the triangular
// passes take as their stop pointer.  The order of the launches is krylovLoop of krylov.hpp, the single solves' own; here is
// the block width of it (BlockWidth), and B and X arrive as the checked Dense operands of device_mat.hpp.
//
// The fused passes (the kernel and its launcher are krylov_block.hpp, which amg.hip shares; the ops are here).  The working vectors are row-major n x kp blocks, kp = k rounded up to even, so a row's column pair
// (c, c + 1), c even, is one 16-byte access; B and X are read and written where the caller keeps them, in 16-byte accesses
// when their layout allows and in 8-byte ones otherwise (the same bits).  A workgroup of 256 lanes takes one block of 4096
// rows and one panel of at most 16 columns.  P adjacent lanes hold the panel's P column pairs (P = 1, 2, 4 or 8, from the
// widest panel), so the 256 / P lane groups read 256 / P row pairs per load instruction, each row a contiguous run of 16 P
// bytes.  What the dot's contract calls "lane t" (the products of rows 512 s + 2 t and 512 s + 2 t + 1, s ascending) is
// computed by group g = t mod (256 / P) as its j-th partial, j = t / (256 / P); the partials of one group are exactly those
// that the tree a[t] += a[t + h] joins at h = 128 ... 256 / P, which therefore happens in registers, in the tree's order
// and depth first (log2 P + 1 live partials, not P); the levels below go through LDS as in the single dot.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>

#include "spmvHip.h"
#include "kernels.hpp"
#include "krylov.hpp"
#include "krylov_block.hpp"

namespace spmvhip {
namespace {

// what the host reads once per batch and the triangular passes take as their stop pointer
struct BlockHead {
    uint32_t allStop;       // 0 while a column runs
    uint32_t stopped;       // columns that have stopped (one ordinary atomicAdd by the lane that stops a column)
};

__device__ __forceinline__ void madd2(double2& acc, double2 a, double2 b) { acc.x += a.x * b.x; acc.y += a.y * b.y; }
__device__ __forceinline__ double2 axpy2(double2 a, double2 s, double2 v) { return make_double2(a.x + s.x * v.x, a.y + s.y * v.y); }
__device__ __forceinline__ double2 axmy2(double2 a, double2 s, double2 v) { return make_double2(a.x - s.x * v.x, a.y - s.y * v.y); }
__device__ __forceinline__ void put(double2& v, int x, double s) { if (x) v.y = s; else v.x = s; }

// ------------------------------------------------------------------------------------- the block forms of the fused passes
// Each op: NDOT; mode(x, st, sc) for column x (0 / 1) of the lane's pair with that column's state: 0 leaves the column
// alone, otherwise the column's scalars go to the lane's sc; load() one row's inputs for the pair (two: column c + 1 exists); step() the update
// of the columns w0 / w1 and the products, a row at a time in ascending order.  A column that is left alone is still
// computed (its lanes share the pair's loads) but never stored, and its partials are never written.
struct BDotOp {                                 // U(:, c) . V(:, c)
    static constexpr int NDOT = 1;
    static constexpr uint32_t CHUNK = 4;
    BMat u, v;
    struct R { double2 u, v; };
    struct Sc {};
    __device__ __forceinline__ int mode(int, const KState*, Sc&) const { return 1; }
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& r) const { r.u = ldp(u, i, c, two); r.v = ldp(v, i, c, two); }
    __device__ __forceinline__ void step(uint64_t, uint32_t, int, int, const Sc&, const R& r, Acc& a) const { madd2(a.d0, r.u, r.v); }
};
struct BGuardedDot : BDotOp {
    __device__ __forceinline__ int mode(int, const KState* st, Sc&) const { return !st->stop; }
};

struct BInitOp {                                // r = b - q (rhat = r too when given); r . r and b . b
    static constexpr int NDOT = 2;
    static constexpr uint32_t CHUNK = 4;
    BMat b, q, r, rhat;
    struct R { double2 b, q; };
    struct Sc {};
    __device__ __forceinline__ int mode(int, const KState*, Sc&) const { return 1; }
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& x) const { x.b = ldp(b, i, c, two); x.q = ldp(q, i, c, two); }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc&, const R& x, Acc& a) const {
        const double2 rv = make_double2(x.b.x - x.q.x, x.b.y - x.q.y);
        stp(r, i, c, w0, w1, rv);
        if (rhat.p) stp(rhat, i, c, w0, w1, rv);
        madd2(a.d0, rv, rv);
        madd2(a.d1, x.b, x.b);
    }
};

struct BTtTsOp {                                // t . t and t . s
    static constexpr int NDOT = 2;
    static constexpr uint32_t CHUNK = 4;
    BMat t, s;
    struct R { double2 t, s; };
    struct Sc {};
    __device__ __forceinline__ int mode(int, const KState* st, Sc&) const { return !st->stop; }
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& r) const { r.t = ldp(t, i, c, two); r.s = ldp(s, i, c, two); }
    __device__ __forceinline__ void step(uint64_t, uint32_t, int, int, const Sc&, const R& r, Acc& a) const { madd2(a.d0, r.t, r.t); madd2(a.d1, r.t, r.s); }
};

struct BCgUpdateOp {                            // x = x + alpha*p; r = r - alpha*q; r . r
    static constexpr int NDOT = 1;
    static constexpr uint32_t CHUNK = 2;
    BMat x, p, r, q;
    struct R { double2 x, p, r, q; };
    struct Sc { double2 alpha; };
    __device__ __forceinline__ int mode(int c, const KState* st, Sc& sc) const { if (st->stop) return 0; put(sc.alpha, c, st->alpha); return 1; }
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& v) const {
        v.x = ldp(x, i, c, two); v.p = ldp(p, i, c, two); v.r = ldp(r, i, c, two); v.q = ldp(q, i, c, two);
    }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc& sc, const R& v, Acc& a) const {
        const double2 rn = axmy2(v.r, sc.alpha, v.q);
        stp(x, i, c, w0, w1, axpy2(v.x, sc.alpha, v.p));
        stp(r, i, c, w0, w1, rn);
        madd2(a.d0, rn, rn);
    }
};

struct BCgPOp {                                 // p = z (first) or p = z + beta*p
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = 4;
    BMat z, p; int first;
    struct R { double2 z, p; };
    struct Sc { double2 beta; };
    __device__ __forceinline__ int mode(int c, const KState* st, Sc& sc) const { if (st->stop) return 0; put(sc.beta, c, st->beta); return 1; }
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& v) const {
        v.z = ldp(z, i, c, two);
        if (!first) v.p = ldp(p, i, c, two);
    }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc& sc, const R& v, Acc&) const {
        stp(p, i, c, w0, w1, first ? v.z : axpy2(v.z, sc.beta, v.p));
    }
};

struct BBiPOp {                                 // p = r (first) or p = r + beta*(p - omega*v)
    static constexpr int NDOT = 0;
    static constexpr uint32_t CHUNK = 4;
    BMat r, p, v; int first;
    struct R { double2 r, p, v; };
    struct Sc { double2 beta, omega; };
    __device__ __forceinline__ int mode(int c, const KState* st, Sc& sc) const {
        if (st->stop) return 0;
        put(sc.beta, c, st->beta); put(sc.omega, c, st->omega);
        return 1;
    }
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& x) const {
        x.r = ldp(r, i, c, two);
        if (!first) { x.p = ldp(p, i, c, two); x.v = ldp(v, i, c, two); }
    }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc& sc, const R& x, Acc&) const {
        if (first) { stp(p, i, c, w0, w1, x.r); return; }
        stp(p, i, c, w0, w1, axpy2(x.r, sc.beta, axmy2(x.p, sc.omega, x.v)));
    }
};

struct BSOp {                                   // s = r - alpha*v; s . s
    static constexpr int NDOT = 1;
    static constexpr uint32_t CHUNK = 4;
    BMat r, v, s;
    struct R { double2 r, v; };
    struct Sc { double2 alpha; };
    __device__ __forceinline__ int mode(int c, const KState* st, Sc& sc) const { if (st->stop) return 0; put(sc.alpha, c, st->alpha); return 1; }
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc&, R& x) const { x.r = ldp(r, i, c, two); x.v = ldp(v, i, c, two); }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc& sc, const R& x, Acc& a) const {
        const double2 sn = axmy2(x.r, sc.alpha, x.v);
        stp(s, i, c, w0, w1, sn);
        madd2(a.d0, sn, sn);
    }
};

// a running column: x = (x + alpha*phat) + omega*shat; r = s - omega*t; r . r and rhat . r.  A column stopped at a half
// step of THIS iteration (halfK == k): x = x + alpha*phat only.  Both per column: the two of a pair may differ.
struct BBiUpdateOp {
    static constexpr int NDOT = 2;
    static constexpr uint32_t CHUNK = 2;
    BMat x, phat, shat, r, s, t, rhat;
    uint64_t k;
    struct R { double2 x, ph, sh, s, t, rh; };
    struct Sc { double2 alpha, omega; int full0 = 0, full1 = 0; };
    __device__ __forceinline__ int mode(int c, const KState* st, Sc& sc) const {
        const int full = !st->stop;
        if (c) sc.full1 = full; else sc.full0 = full;
        if (!full && st->halfK != k) return 0;
        put(sc.alpha, c, st->alpha); put(sc.omega, c, st->omega);
        return 1;
    }
    __device__ __forceinline__ void load(uint64_t i, uint32_t c, bool two, const Sc& sc, R& v) const {
        v.x = ldp(x, i, c, two); v.ph = ldp(phat, i, c, two);
        if (sc.full0 | sc.full1) { v.sh = ldp(shat, i, c, two); v.s = ldp(s, i, c, two); v.t = ldp(t, i, c, two); v.rh = ldp(rhat, i, c, two); }
    }
    __device__ __forceinline__ void step(uint64_t i, uint32_t c, int w0, int w1, const Sc& sc, const R& v, Acc& a) const {
        const double2 h = axpy2(v.x, sc.alpha, v.ph);
        if (!(sc.full0 | sc.full1)) { stp(x, i, c, w0, w1, h); return; }
        const double2 xf = axpy2(h, sc.omega, v.sh);
        stp(x, i, c, w0, w1, make_double2(sc.full0 ? xf.x : h.x, sc.full1 ? xf.y : h.y));
        const double2 rn = axmy2(v.s, sc.omega, v.t);
        stp(r, i, c, w0 && sc.full0, w1 && sc.full1, rn);
        madd2(a.d0, rn, rn);
        madd2(a.d1, v.rh, rn);
    }
};

// column c = the workgroup: its block partials by the dot's second level (lane t adds partials t, t + 256, ... in order,
// then the tree), then lane 0 runs the column's scalar step `ph` of iteration it -- or stores the dot (F_DOT)
__global__ __launch_bounds__(KT) void block_finish_kernel(uint64_t nb, uint32_t k, uint32_t kp, const double* __restrict__ part0,
                                                          const double* __restrict__ part1, int ph, uint64_t it, KState* st,
                                                          BlockHead* head, double* hist, uint64_t histLd, double* out, int precond) {
    __shared__ double2 sh[KT];
    const uint32_t c = blockIdx.x;
    if (c >= k) return;
    KState* s = st ? st + c : nullptr;
    if (ph != F_DOT && ph != F_CG_INIT && ph != F_BI_INIT && s->stop) return;
    double a0 = 0.0, a1 = 0.0;
    for (uint64_t j = threadIdx.x; j < nb; j += KT) {
        a0 += part0[j * kp + c];
        if (part1) a1 += part1[j * kp + c];
    }
    const double2 d = tree256(make_double2(a0, a1), sh);
    if (threadIdx.x != 0) return;
    if (ph == F_DOT) { out[c] = d.x; return; }
    krylovScalarStep(ph, it, d, s, hist ? hist + c * histLd : nullptr, precond);
    // the column ran (or starts) and has now stopped: it is counted once, and the last one sets the head word, which
    // later launches read -- ordering comes from the kernel boundary
    if (s->stop && atomicAdd(&head->stopped, 1u) + 1 == k) head->allStop = 1;
}

void launchBlockFinish(uint64_t n, uint32_t k, const double* p0, const double* p1, int ph, uint64_t it, KState* st, BlockHead* head,
                       double* hist, uint64_t histLd, double* out, int precond, hipStream_t s) {
    hipLaunchKernelGGL(block_finish_kernel, dim3(k), dim3(KT), 0, s, blocksOf(n), k, k + (k & 1), p0, p1, ph, it, st, head, hist,
                       histLd, out, precond);
}

// the block width of krylovLoop (krylov.hpp): an n x kp block a role, a state block a column, and the head word, which the
// host reads after the init (every column may have stopped there: no further kernel) and once per batch
struct BlockWidth {
    using Vec = BMat;
    using Init = BInitOp; using Dot = BGuardedDot; using TtTs = BTtTsOp; using CgUpdate = BCgUpdateOp; using CgP = BCgPOp;
    using BiP = BBiPOp; using S = BSOp; using BiUpdate = BBiUpdateOp;
    const uint64_t n; const uint32_t k; const DevMat* const a; const DevMat* const m; const int pre; const uint64_t histLd;
    const hipStream_t s;
    spmvKrylovInfo& out;                        // launches and hostChecks are counted here
    const bool cycle = pre && m->origin == Origin::HIERARCHY;            // M^-1 is a block cycle of the hierarchy (its width is >= k)
    const bool fsai = pre && m->origin == Origin::FSAI;                  // ... or G^T (G in) of an approximate-inverse factor, through gw
    unsigned long triLaunches = 0;              // of the two triangular passes otherwise
    Vec b{}, x{}, v[8] = {}, gw{};
    double* p0 = nullptr; double* p1 = nullptr; // the block partials of a pass's first and second dot
    KState* st = nullptr; BlockHead* head = nullptr; double* hist = nullptr;
    BlockHead hh{};                             // the head word as the host last read it
    int product(const Vec& in, const Vec& outv) { ++out.launches; return enqueueSpmm(a, k, dense(in), dense(outv), s); }
    int precond(const Vec& in, const Vec& outv) {                        // z = U^-1 (L^-1 in), or one cycle: every launch behind the head word
        if (cycle) return enqueueAmgCycleBlock(m, a, k, dense(in), dense(outv), s, &head->allStop, &out.launches);
        if (fsai) {                                                      // two SpMM passes, which run whatever the head word says
            const bool f32 = m->fsai->storage == SPMV_STORAGE_F32;        // (stored in single precision: the f32 passes)
            if (f32 && !(m->f32 && m->fsai->gt->f32)) {
                fprintf(stderr, "libspmvhip: block Krylov solve: dM is an approximate-inverse factor stored in single precision, but its "
                                "single-precision value forms are not built: spmvHipFsaiSetStorage(dM, SPMV_STORAGE_F32) again\n");
                return EXIT_FAILURE;
            }
            if (enqueueSpmm(m, k, dense(in), dense(gw), s, f32) || enqueueSpmm(m->fsai->gt, k, dense(gw), dense(outv), s, f32)) return EXIT_FAILURE;
            out.launches += 2;
            return EXIT_SUCCESS;
        }
        if (triSweepsMode(m)) return enqueueTriSweepsApply(m, k, dense(in), dense(outv), s, &head->allStop, &out.launches);
        dim3 g, bl;
        if (enqueueTrsm(m, SPMV_TRI_LOWER, SPMV_DIAG_UNIT, k, dense(in), dense(outv), s, &g, &bl, &head->allStop)) return EXIT_FAILURE;
        if (enqueueTrsm(m, SPMV_TRI_UPPER, SPMV_DIAG_STORED, k, dense(outv), dense(outv), s, &g, &bl, &head->allStop)) return EXIT_FAILURE;
        out.launches += triLaunches;
        return EXIT_SUCCESS;
    }
    template <class Op> void vec(const Op& op, std::initializer_list<Vec>) {       // (a block's own `pair` is its alignment test)
        launchBlockVec(n, k, st, op, p0, p1, s);
        ++out.launches;
    }
    void finish(int ph, uint64_t it, int ndot) {
        launchBlockFinish(n, k, p0, ndot > 1 ? p1 : nullptr, ph, it, st, head, hist, histLd, nullptr, pre, s);
        ++out.launches;
    }
    int afterInit(bool* done) { return afterBatch(done); }
    int afterBatch(bool* done) {                                         // one read-back of the head word
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&hh, head, sizeof hh, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++out.hostChecks;
        *done = hh.allStop != 0;
        return EXIT_SUCCESS;
    }
};

}  // namespace

int enqueueBlockDot(uint64_t n, uint32_t k, const Dense& U, const Dense& V, double* out, hipStream_t st) {
    const uint32_t kp = k + (k & 1);
    double* part = nullptr;
    if (dotWorkspace(blocksOf(n) * kp, &part)) return EXIT_FAILURE;
    launchBlockVec(n, k, nullptr, BDotOp{bmat(U, k, false), bmat(V, k, false)}, part, nullptr, st);
    launchBlockFinish(n, k, part, nullptr, F_DOT, 0, nullptr, nullptr, nullptr, 0, out, 0, st);
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

int krylovBlockSolve(int bicg, const DevMat* a, const DevMat* m, uint32_t k, const Dense& B, const Dense& X, const spmvKrylovOpts* o,
                     spmvKrylovColumn* cols, spmvKrylovInfo* info, uint32_t K, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = a->M, nb = std::max<uint64_t>(blocksOf(n), 1), histLd = o->maxIter + 1;
    const uint32_t kp = k + (k & 1);
    const int pre = m != nullptr;
    const auto fail = [] { fprintf(stderr, "libspmvhip: block Krylov solve: workspace allocation failed\n"); return EXIT_FAILURE; };
    spmvKrylovInfo out{};
    DevBufs bufs;
    BlockWidth w{n, k, a, m, pre, histLd, s, out};
    const int nvec = bicg ? (pre ? 8 : 6) : (pre ? 4 : 3);
    for (int i = 0; i < nvec; ++i) {
        double* p = bufs.alloc<double>(n * kp);
        if (!p) return fail();
        w.v[i] = bmat(Dense{p, kp, true}, k, true);
    }
    if (w.fsai) {                                                        // one more block: G in, between the two passes
        double* p = bufs.alloc<double>(n * kp);
        if (!p) return fail();
        w.gw = bmat(Dense{p, kp, true}, k, true);
    }
    w.p0 = bufs.alloc<double>(2 * nb * kp);
    BlockHead* head = w.head = bufs.alloc<BlockHead>(1);
    KState* st = w.st = bufs.alloc<KState>(k);
    double* hist = w.hist = o->history ? bufs.alloc<double>(k * histLd) : nullptr;
    if (!w.p0 || !head || !st || (o->history && !hist)) return fail();
    w.p1 = w.p0 + nb * kp;
    KState h0{};
    h0.maxIter = o->maxIter;
    h0.tol2 = o->tol * o->tol;
    std::vector<KState> h(k, h0);
    HIP_TRY(hipMemcpyAsync(st, h.data(), k * sizeof(KState), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(head, &w.hh, sizeof w.hh, hipMemcpyHostToDevice, s));
    w.b = bmat(B, k, false);
    w.x = bmat(X, k, false);
    if (pre && !w.cycle && !w.fsai) {
        spmvTriInfo t{};
        for (int uplo : {SPMV_TRI_LOWER, SPMV_TRI_UPPER}) { triInfo(m, uplo, &t); w.triLaunches += t.launches; }
    }
    if (krylovLoop(w, bicg, pre, o->maxIter, K)) return EXIT_FAILURE;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h.data(), st, k * sizeof(KState), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t c = 0; c < k; ++c)
        if (!h[c].stop) { fprintf(stderr, "libspmvhip: block Krylov solve: column %u did not stop\n", c); return EXIT_FAILURE; }
    uint32_t lead = 0;                                                   // the lowest-numbered column of the largest status
    for (uint32_t c = 0; c < k; ++c) {
        if (o->history)
            HIP_TRY(hipMemcpy(o->history + c * histLd, hist + c * histLd, (h[c].iterations + 1) * sizeof(double), hipMemcpyDeviceToHost));
        if (cols) cols[c] = spmvKrylovColumn{h[c].status, h[c].iterations, h[c].rr, h[c].bb};
        if (h[c].status > h[lead].status) lead = c;
        out.iterations = std::max<unsigned long>(out.iterations, h[c].iterations);
    }
    out.status = h[lead].status;
    out.rr = h[lead].rr;
    out.bb = h[lead].bb;
    out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = out;
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
