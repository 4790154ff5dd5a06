// gmres.hip -- h = V^T w in one pass (spmvHipMultiDot) and restarted GMRES(m) with CGS2 orthogonalisation
// (hipSpGMRESCSR) on a device CSR handle (contract in spmvHip.h, design in DESIGN.md section 20).  Every entry of h is the
// bits of spmvHipDot on its column; x, the iteration count and every residual norm are the bits of the loop in spmvHip.h.
//
// The multi-dot, the update kernel and the scale pass are in orth.hpp, which lanczos.hip shares.
//
// The solver: the scalars of the loop (h, c, cs, sn, g, R, y, k, cols, the status) live in a device state block that only
// single-lane finish steps write.  `stop` ends the solve, `skip` ends a cycle early: every kernel of an inner step and
// its triangular solves return at once on skip (stop implies skip), the cycle-end kernels on stop.  The host enqueues a
// whole cycle and reads the head of the block back once per cycle.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>

#include "spmvHip.h"
#include "kernels.hpp"
#include "krylov.hpp"
#include "orth.hpp"

namespace spmvhip {
namespace {

constexpr uint32_t GM_MAXM = 64;                // restart at most

struct GState {
    uint32_t stop;          // 0 while the solve runs
    uint32_t skip;          // 1 once the cycle has ended (and while stopped): inner steps do nothing
    int32_t  status;        // SPMV_KRYLOV_* once stopped
    uint32_t cols;          // columns of the cycle's least-squares problem
    uint32_t brk;           // the cycle ended on hn == 0 or d == 0
    uint32_t restart;
    uint64_t k, maxIter, cycles;
    double   tol2, rr, bb, thresh, beta, hn;
    // ---- not read back
    double   h[GM_MAXM], c[GM_MAXM], cs[GM_MAXM], sn[GM_MAXM], g[GM_MAXM + 1], y[GM_MAXM];
    double   R[GM_MAXM * GM_MAXM];              // column j at R[j*GM_MAXM ..]
};
constexpr size_t GSTATE_HEAD = offsetof(GState, h);

// cycle end: u = y[0] v[0]; u = u + y[i] v[i], i = 1 .. cols-1; then out = u (x == null) or x = x + u
__global__ __launch_bounds__(KT) void gmres_comb_kernel(uint64_t n, const double* __restrict__ V, uint64_t ldv, const GState* __restrict__ st,
                                                        double* __restrict__ out, double* x, int xvec, uint64_t nb) {
    if (st->stop) return;
    const uint64_t blk = linear_block();
    if (blk >= nb) return;
    const uint64_t base = blk * KB + 2 * threadIdx.x;
    const bool full = blk * KB + KB <= n;
    const uint32_t cols = st->cols;
    double2 u[KSLICES];
    for (uint32_t c = 0; c < cols; ++c) {
        const double yc = st->y[c];
        const double* v = V + (uint64_t)c * ldv;
#pragma unroll
        for (uint32_t s = 0; s < KSLICES; ++s) {
            const uint64_t i = base + (uint64_t)s * (2 * KT);
            double2 r = make_double2(0.0, 0.0);
            if (full || i < n) r = ld2<true>(v, i, full || i + 1 < n);
            if (c == 0) u[s] = make_double2(yc * r.x, yc * r.y);
            else        u[s] = make_double2(u[s].x + yc * r.x, u[s].y + yc * r.y);
        }
    }
    if (!x) { storeW<true>(out, base, n, full, u); return; }
#pragma unroll
    for (uint32_t s = 0; s < KSLICES; ++s) {
        const uint64_t i = base + (uint64_t)s * (2 * KT);
        if (!(full || i < n)) continue;
        const bool two = full || i + 1 < n;
        if (xvec) { const double2 xv = ld2<true>(x, i, two);  st2<true>(x, i, two, make_double2(xv.x + u[s].x, xv.y + u[s].y)); }
        else      { const double2 xv = ld2<false>(x, i, two); st2<false>(x, i, two, make_double2(xv.x + u[s].x, xv.y + u[s].y)); }
    }
}

struct GAddOp {                                 // x = x + z, unless *flag
    static constexpr int NDOT = 0;
    double* x; const double* z; const uint32_t* flag;
    struct R { double2 x, z; };
    __device__ int mode(const KState*) const { return !*flag; }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& r) const { r.x = ld2<VEC>(x, i, two); r.z = ld2<VEC>(z, i, two); }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& r, double&, double&) const {
        st2<VEC>(x, i, two, make_double2(r.x.x + r.z.x, r.x.y + r.z.y));
    }
};

struct GResidOp : InitOp {                      // r = b - q; r . r (and b . b), unless *flag
    const uint32_t* flag;
    __device__ int mode(const KState*) const { return !*flag; }
};

enum GPhase : int { G_INIT, G_WW, G_END };

// y = R^-1 g over the cycle's `cols` columns (one lane)
__device__ void backSolve(GState* st, uint32_t cols) {
    for (int i = (int)cols - 1; i >= 0; --i) {
        double s = st->g[i];
        for (uint32_t l = i + 1; l < cols; ++l) s = s - st->R[l * GM_MAXM + i] * st->y[l];
        st->y[i] = s / st->R[i * GM_MAXM + i];
    }
}

// the block partials of one or two dots (krylov_finish_kernel's rule), then lane 0 runs the loop's scalar step:
//   G_INIT  rr, bb, thresh, the three first exits; beta = sqrt(rr)
//   G_WW    inner step j: h += c, hn, the Givens rotations, the estimate and the cycle's end tests; y at the cycle's end
//   G_END   the true rr after x = x + z: the exits, or the next cycle's beta
__global__ __launch_bounds__(KT) void gmres_finish_kernel(uint64_t nb, const double* __restrict__ part0, const double* __restrict__ part1,
                                                          int ph, uint32_t j, GState* st, double* hist) {
    __shared__ double2 sh[KT];
    if (ph == G_WW && (st->stop | st->skip)) return;
    if (ph == G_END && st->stop) return;
    double a0 = 0.0, a1 = 0.0;
    for (uint64_t i = threadIdx.x; i < nb; i += KT) {
        a0 += part0[i];
        if (part1) a1 += part1[i];
    }
    const double2 d = tree256(make_double2(a0, a1), sh);
    if (threadIdx.x != 0) return;
    auto stopAt = [&](int status) { st->status = status; st->stop = 1; st->skip = 1; };
    auto begin = [&](double rr) {                                        // a cycle starts from the residual r, rr = r . r
        const double beta = sqrt(rr);
        st->beta = beta; st->g[0] = beta; st->skip = 0; st->brk = 0; st->cols = 0; ++st->cycles;
    };
    switch (ph) {
    case G_INIT: {
        const double rr = d.x, bb = d.y, thresh = st->tol2 * bb;
        st->rr = rr; st->bb = bb; st->thresh = thresh;
        st->k = 0; st->cycles = 0; st->stop = 0; st->skip = 1; st->status = SPMV_KRYLOV_MAXITER;
        if (hist) hist[0] = rr;
        if (rr <= thresh) stopAt(SPMV_KRYLOV_CONVERGED);
        else if (!isfinite(rr)) stopAt(SPMV_KRYLOV_NONFINITE);
        else if (st->maxIter == 0) stopAt(SPMV_KRYLOV_MAXITER);
        else begin(rr);
        break;
    }
    case G_WW: {
        const uint64_t k = st->k + 1;
        double* h = st->h;
        for (uint32_t i = 0; i <= j; ++i) h[i] = h[i] + st->c[i];
        const double hn = sqrt(d.x);
        st->hn = hn;
        for (uint32_t i = 0; i < j; ++i) {
            const double cs = st->cs[i], sn = st->sn[i], lo = h[i], hi = h[i + 1];
            const double t = cs * lo + sn * hi;
            h[i + 1] = cs * hi - sn * lo;
            h[i] = t;
        }
        const double hj = h[j];
        const double dd = sqrt(hj * hj + hn * hn);
        if (dd == 0.0) {                                                 // the step is dropped: k stays, hist[k] is not written
            st->brk = 1;
            st->cols = j;
            if (j == 0) { stopAt(SPMV_KRYLOV_BREAKDOWN); break; }        // nothing to add to x: the solve ends here
            st->skip = 1;
            backSolve(st, j);
            break;
        }
        const double cs = hj / dd, sn = hn / dd;
        st->cs[j] = cs; st->sn[j] = sn;
        h[j] = dd;
        for (uint32_t i = 0; i <= j; ++i) st->R[j * GM_MAXM + i] = h[i];
        const double gj = st->g[j];
        const double gn = -(sn * gj);
        st->g[j + 1] = gn;
        st->g[j] = cs * gj;
        const double est = gn * gn;
        st->k = k;
        if (hist) hist[k] = est;
        if (est <= st->thresh || !isfinite(est) || hn == 0.0 || j == st->restart - 1 || k == st->maxIter) {
            st->brk = hn == 0.0;
            st->cols = j + 1;
            st->skip = 1;
            backSolve(st, j + 1);
        }
        break;
    }
    case G_END: {
        const double rr = d.x;
        const uint64_t k = st->k;
        st->rr = rr;
        if (hist) hist[k] = rr;
        if (rr <= st->thresh) stopAt(SPMV_KRYLOV_CONVERGED);
        else if (!isfinite(rr)) stopAt(SPMV_KRYLOV_NONFINITE);
        else if (st->brk) stopAt(SPMV_KRYLOV_BREAKDOWN);
        else if (k == st->maxIter) stopAt(SPMV_KRYLOV_MAXITER);
        else begin(rr);
        break;
    }
    default:
        break;
    }
}

}  // namespace

int enqueueMultiDot(uint64_t n, uint32_t k, const double* V, uint64_t ldv, const double* w, double* out, hipStream_t st) {
    const uint64_t nb = blocksOf(n);
    double* part = nullptr;
    if (dotWorkspace((uint64_t)k * nb, &part)) return EXIT_FAILURE;
    const bool vec = aligned16(V) && aligned16(w) && (k == 1 || ldv % 2 == 0);   // every column's pointer
    launchMultiDot(n, k, V, ldv, w, part, out, vec, nullptr, st);
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

size_t gmresWorkspaceBytes(uint64_t n, uint32_t restart, uint64_t maxIter, int precond, int history) {
    const uint64_t ldv = (n + 1) & ~1ull, nb = std::max<uint64_t>(blocksOf(n), 1);
    return (size_t)(((uint64_t)restart + 1 + 3 + (precond ? 1 : 0)) * ldv * 8 + ((uint64_t)restart + 2) * nb * 8 + sizeof(GState) +
                    (history ? (maxIter + 1) * 8 : 0));
}

int gmresSolve(spmat* hA, const DevMat* a, const DevMat* m, const double* b, double* x, const spmvGmresOpts* o, spmvKrylovInfo* info,
               int fused, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = a->M, nb = std::max<uint64_t>(blocksOf(n), 1), ldv = (n + 1) & ~1ull;
    const uint32_t m_ = o->restart;
    const int pre = m != nullptr;
    spmvKrylovInfo out{};
    DevBufs ws;
    auto fail = [] { fprintf(stderr, "libspmvhip: GMRES solve: workspace allocation failed\n"); return EXIT_FAILURE; };
    double* V = ws.alloc<double>(((uint64_t)m_ + 1) * ldv);              // the basis, every column 16-byte aligned
    double* w = ws.alloc<double>(ldv);                                   // w, and u at the cycle's end
    double* z = pre ? ws.alloc<double>(ldv) : nullptr;
    double* r = ws.alloc<double>(ldv);
    double* q = ws.alloc<double>(ldv);
    double* part = ws.alloc<double>(((uint64_t)m_ + 2) * nb);            // m_ columns of partials; two more for r . r, b . b
    GState* st = ws.alloc<GState>(1);
    double* hist = o->history ? ws.alloc<double>(o->maxIter + 1) : nullptr;
    if (!V || !w || (pre && !z) || !r || !q || !part || !st || (o->history && !hist)) return fail();
    double* p0 = part + (uint64_t)m_ * nb;
    double* p1 = p0 + nb;
    GState h{};
    h.maxIter = o->maxIter;
    h.restart = m_;
    h.tol2 = o->tol * o->tol;
    HIP_TRY(hipMemcpyAsync(st, &h, GSTATE_HEAD, hipMemcpyHostToDevice, s));
    const uint32_t* flags = &st->stop;                                   // {stop, skip}
    const Precond pc(m, hA, s);
    auto precond = [&](const double* in, double* outv, const uint32_t* flag) { return pc.apply(in, outv, flag, &out.launches); };
    auto spmv = [&](const double* in, double* outv) {
        ++out.launches;
        return spmvHipEnqueueAutoRows(hA, const_cast<double*>(in), outv, s);
    };
    auto vec = [&](const auto& op, std::initializer_list<const void*> ptrs) {
        bool al = true;
        for (const void* p : ptrs) al = al && aligned16(p);
        launchVec(n, nullptr, op, al, p0, p1, s);
        ++out.launches;
    };
    auto finish = [&](int ph, uint32_t j, int ndot) {
        hipLaunchKernelGGL(gmres_finish_kernel, dim3(1), dim3(KT), 0, s, blocksOf(n), p0, ndot > 1 ? p1 : nullptr, ph, j, st, hist);
        ++out.launches;
    };
    auto project = [&](uint32_t k, double* coef) {                       // coef[0 .. k-1] = V^T w
        launchMultiDot(n, k, V, ldv, w, part, coef, true, flags, s);
        out.launches += 2;
    };
    const dim3 ugrid = grid2d(nb, KT);
    if (spmv(x, q)) return EXIT_FAILURE;                                 // the first call for a handle chooses the kernel
    vec(InitOp{b, q, r, nullptr}, {b, q, r});
    finish(G_INIT, 0, 2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h, st, GSTATE_HEAD, hipMemcpyDeviceToHost, s));   // (the init's exits: not counted as a check)
    HIP_TRY(hipStreamSynchronize(s));
    while (!h.stop) {
        const uint32_t steps = (uint32_t)std::min<uint64_t>(m_, o->maxIter - h.k);
        vec(GScaleOp{r, V, &st->beta, &st->skip, 0.0}, {r, V});          // v[0] = r / beta
        for (uint32_t j = 0; j < steps; ++j) {
            const double* vj = V + (uint64_t)j * ldv;
            if (pre && precond(vj, z, &st->skip)) return EXIT_FAILURE;
            if (spmv(pre ? z : vj, w)) return EXIT_FAILURE;
            project(j + 1, st->h);
            if (fused) {
                hipLaunchKernelGGL(gmres_update_kernel<1>, ugrid, dim3(KT), 0, s, n, j + 1, V, ldv, w, st->h, part, nb, flags);
                hipLaunchKernelGGL(multidot_finish_kernel, dim3((j + 2) / 2), dim3(KT), 0, s, blocksOf(n), j + 1, part, st->c, flags);
                out.launches += 2;
            } else {
                hipLaunchKernelGGL(gmres_update_kernel<0>, ugrid, dim3(KT), 0, s, n, j + 1, V, ldv, w, st->h, part, nb, flags);
                ++out.launches;
                project(j + 1, st->c);
            }
            hipLaunchKernelGGL(gmres_update_kernel<2>, ugrid, dim3(KT), 0, s, n, j + 1, V, ldv, w, st->c, p0, nb, flags);
            ++out.launches;
            finish(G_WW, j, 1);
            if (j + 1 < steps) vec(GScaleOp{w, V + (uint64_t)(j + 1) * ldv, &st->hn, &st->skip, 0.0}, {w, V});   // v[j+1] = w / hn
        }
        // the cycle's end: x = x + M^-1 (V y), the true residual and its exits
        if (pre) {
            hipLaunchKernelGGL(gmres_comb_kernel, ugrid, dim3(KT), 0, s, n, V, ldv, st, w, (double*)nullptr, 0, nb);
            ++out.launches;
            if (precond(w, z, &st->stop)) return EXIT_FAILURE;
            vec(GAddOp{x, z, &st->stop}, {x, z});
        } else {
            hipLaunchKernelGGL(gmres_comb_kernel, ugrid, dim3(KT), 0, s, n, V, ldv, st, w, x, (int)aligned16(x), nb);
            ++out.launches;
        }
        if (spmv(x, q)) return EXIT_FAILURE;
        vec(GResidOp{{b, q, r, nullptr}, &st->stop}, {b, q, r});
        finish(G_END, 0, 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h, st, GSTATE_HEAD, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++out.hostChecks;
        if (!h.stop && h.skip) { fprintf(stderr, "libspmvhip: GMRES solve: a cycle did not end\n"); return EXIT_FAILURE; }
    }
    if (o->history) HIP_TRY(hipMemcpy(o->history, hist, (h.k + 1) * sizeof(double), hipMemcpyDeviceToHost));
    out.status = h.status;
    out.iterations = h.k;
    out.rr = h.rr;
    out.bb = h.bb;
    out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = out;
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
