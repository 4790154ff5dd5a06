// davidson.hip -- the residual block R = W S - (V S) diag(theta) with its column norms (spmvHipBlockResidual) and generalised
// Davidson with single-vector expansion, CGS2 and thick restart (hipSpDavidsonCSR) on a symmetric device CSR handle, with
// any dM of the Krylov solvers as M^-1 (contract in spmvHip.h, design in DESIGN.md section 42).  Every R(i, c) is the
// rounded expression of the header, every norm the bits of spmvHipDot; theta, res, X and the counts are the bits of the
// loop written there.
//
// The residual block: a workgroup takes one block of KB = 4096 rows -- the block of the fixed-order dot --, and a lane its
// eight element pairs of that block, one after the other.  For a pair it streams j: the pair's values of v[j] and w[j]
// (a wave's load is one contiguous run of the column; BR_CHUNK columns of each are issued before the first use) meet the k
// entries S[j][.] at wave-uniform addresses in 2 k running sums, u = V S and q = W S, each in ascending j from +0.0.  Then
// R = q - theta*u is stored and its squares join the lane's partials of the k norms in spmvHipDot's order; the tree and the
// block partials are the dot's, and the second kernel of spmvHipMultiDot adds them.  Not in place: nothing of a row is kept
// beyond its sums, so the register budget is 2 k double2 of sums (8 k VGPRs) and 2 BR_CHUNK double2 of loads, and the
// kernel is instantiated for k <= 4, 8 and 16.  No MFMA, no FMA.
//
// The solver: beta, the new column of H, the k norms and the flags live in a device state block; `stop` ends the solve (a
// beta that is not finite), `skip` the step's remaining kernels (beta == 0, stop).  The host reads the block back twice a
// step: beta with the column of H, then the norms.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "spmvHip.h"
#include "kernels.hpp"
#include "krylov.hpp"
#include "orth.hpp"
#include "jacobi.hpp"

namespace spmvhip {
namespace {

constexpr uint32_t DV_MAXK = 16;                // eigenpairs at most: columns of a residual block
constexpr int      BR_CHUNK = 4;                // columns of V and of W whose loads a lane issues together

// ------------------------------------------------------------------------------------------------ the residual block
__device__ __forceinline__ void pairMadd(double2& a, double2 v, double s) { a.x = a.x + v.x * s; a.y = a.y + v.y * s; }

// the pair of rows i, i + 1: WIDE, both rows in one 16-byte access (the caller knows the pair to be whole and aligned);
// else 8-byte accesses, the second row only when `two`
template <bool WIDE>
__device__ __forceinline__ double2 pairLoad(const double* p, uint64_t i, bool two) {
    if constexpr (WIDE) return *reinterpret_cast<const double2*>(p + i);
    else return make_double2(p[i], two ? p[i + 1] : 0.0);
}
template <bool WIDE>
__device__ __forceinline__ void pairStore(double* p, uint64_t i, bool two, double2 v) {
    if constexpr (WIDE) *reinterpret_cast<double2*>(p + i) = v;
    else { p[i] = v.x; if (two) p[i + 1] = v.y; }
}

// columns j0 .. j0 + NJ - 1 of V and W at the pair i into the sums: NJ loads of each first, then the products, a column's
// KCAP chains next to each other (a sum's order is ascending j whatever NJ is)
template <int KCAP, bool WIDE, int NJ>
__device__ __forceinline__ void residualColumns(const double* __restrict__ V, uint64_t ldv, const double* __restrict__ W, uint64_t ldw,
                                                const double* __restrict__ S, uint64_t lds, uint32_t k, uint32_t j0, uint64_t i, bool two,
                                                double2 (&u)[KCAP], double2 (&q)[KCAP]) {
    double2 v[NJ], w[NJ];
#pragma unroll
    for (int a = 0; a < NJ; ++a) {
        v[a] = pairLoad<WIDE>(V + (uint64_t)(j0 + a) * ldv, i, two);
        w[a] = pairLoad<WIDE>(W + (uint64_t)(j0 + a) * ldw, i, two);
    }
#pragma unroll
    for (int a = 0; a < NJ; ++a)
#pragma unroll
        for (int c = 0; c < KCAP; ++c) {
            const double sv = (uint32_t)c < k ? S[(uint64_t)c * lds + j0 + a] : 0.0;      // (uniform; a column >= k is never stored)
            pairMadd(u[c], v[a], sv);
            pairMadd(q[c], w[a], sv);
        }
}

// one pair of rows: its 2 k sums over the m columns, its k entries of R, and their squares into the lane's partials
template <int KCAP, bool WIDE>
__device__ __forceinline__ void residualPair(uint32_t m, uint32_t k, const double* __restrict__ V, uint64_t ldv, const double* __restrict__ W,
                                             uint64_t ldw, const double* __restrict__ S, uint64_t lds, const double* __restrict__ theta,
                                             double* __restrict__ R, uint64_t ldr, uint64_t i, bool two, double (&nacc)[KCAP]) {
    double2 u[KCAP], q[KCAP];
#pragma unroll
    for (int c = 0; c < KCAP; ++c) { u[c] = make_double2(0.0, 0.0); q[c] = make_double2(0.0, 0.0); }
    uint32_t j = 0;
    for (; j + BR_CHUNK <= m; j += BR_CHUNK) residualColumns<KCAP, WIDE, BR_CHUNK>(V, ldv, W, ldw, S, lds, k, j, i, two, u, q);
    for (; j < m; ++j) residualColumns<KCAP, WIDE, 1>(V, ldv, W, ldw, S, lds, k, j, i, two, u, q);
#pragma unroll
    for (int c = 0; c < KCAP; ++c)
        if ((uint32_t)c < k) {
            const double th = theta[c];
            const double2 r = make_double2(q[c].x - th * u[c].x, q[c].y - th * u[c].y);
            pairStore<WIDE>(R + (uint64_t)c * ldr, i, two, r);
            madd(nacc[c], r, r, two);
        }
}

// R(i, c) = (sum_j W(i, j) S[j][c]) - theta[c] * (sum_j V(i, j) S[j][c]), and the block partials part[c*nb + blk] of
// dot(R(:, c), R(:, c)).  VEC: every column of V, W and R is 16-byte aligned, so a whole pair takes the 16-byte accesses (the
// one half pair of an odd n takes the 8-byte ones).  flags: null, or {stop, skip} of a solve
template <int KCAP, bool VEC>
__global__ __launch_bounds__(KT) void block_residual_kernel(uint64_t n, uint32_t m, uint32_t k, const double* __restrict__ V, uint64_t ldv,
                                                            const double* __restrict__ W, uint64_t ldw, const double* __restrict__ S,
                                                            uint64_t lds, const double* __restrict__ theta, double* __restrict__ R,
                                                            uint64_t ldr, double* __restrict__ part, uint64_t nb,
                                                            const uint32_t* __restrict__ flags) {
    __shared__ double2 sh[2][KT];
    if (flags && (flags[0] | flags[1])) return;
    const uint64_t blk = linear_block();
    if (blk >= nb) return;                                               // (a folded grid's tail)
    const uint64_t base = blk * KB + 2 * threadIdx.x;
    const bool full = blk * KB + KB <= n;
    double nacc[KCAP];
#pragma unroll
    for (int c = 0; c < KCAP; ++c) nacc[c] = 0.0;
#pragma unroll 1
    for (uint32_t s = 0; s < KSLICES; ++s) {
        const uint64_t i = base + (uint64_t)s * (2 * KT);
        if (!(full || i < n)) break;                                     // (the slices ascend: the later ones are past n too)
        const bool two = full || i + 1 < n;
        if (VEC && two) residualPair<KCAP, true>(m, k, V, ldv, W, ldw, S, lds, theta, R, ldr, i, true, nacc);
        else            residualPair<KCAP, false>(m, k, V, ldv, W, ldw, S, lds, theta, R, ldr, i, two, nacc);
    }
#pragma unroll
    for (int c = 0; c < KCAP; c += 2)
        if ((uint32_t)c < k) {                                           // (uniform) two columns a tree pass, the buffers alternating
            const bool pair = (uint32_t)c + 1 < k;
            const double2 d = tree256(make_double2(nacc[c], nacc[c + 1]), sh[(c >> 1) & 1]);      // (KCAP is even; a column >= k holds 0.0)
            if (threadIdx.x == 0) {
                part[(uint64_t)c * nb + blk] = d.x;
                if (pair) part[(uint64_t)(c + 1) * nb + blk] = d.y;
            }
        }
}

template <int KCAP>
void launchResidual(bool vec, dim3 grid, hipStream_t st, uint64_t n, uint32_t m, uint32_t k, const double* V, uint64_t ldv, const double* W,
                    uint64_t ldw, const double* S, uint64_t lds, const double* theta, double* R, uint64_t ldr, double* part, uint64_t nb,
                    const uint32_t* flags) {
    if (vec) hipLaunchKernelGGL((block_residual_kernel<KCAP, true>), grid, dim3(KT), 0, st, n, m, k, V, ldv, W, ldw, S, lds, theta, R, ldr, part, nb, flags);
    else     hipLaunchKernelGGL((block_residual_kernel<KCAP, false>), grid, dim3(KT), 0, st, n, m, k, V, ldv, W, ldw, S, lds, theta, R, ldr, part, nb, flags);
}

// ------------------------------------------------------------------------------------------------ the solver's state
struct DState {
    uint32_t stop;          // 0 while the solve runs
    uint32_t skip;          // 1 once the step's remaining kernels are to do nothing (stop implies skip)
    int32_t  status;        // SPMV_KRYLOV_* once stopped
    uint32_t exact;         // the last expansion found beta == 0
    uint64_t maxIter;
    double   nrm;           // sqrt(dot(v0, v0))
    double   beta;          // sqrt(dot(t, t)) of the last expansion
    double   hcol[LZ_MAXM]; // dot(v[i], w[j]) of the last product
    double   n2[DV_MAXK];   // dot(R(:, c), R(:, c)) of the last residual block
    // ---- not read back
    double   h[LZ_MAXM], c[LZ_MAXM];
};
constexpr size_t DSTATE_HEAD = offsetof(DState, h);

enum DPhase : int { D_INIT, D_BETA };

// the block partials of one dot (krylov_finish_kernel's rule), then lane 0 runs the loop's scalar step:
//   D_INIT  dot(v0, v0): the three first exits, or nrm
//   D_BETA  beta = sqrt(dot(t, t)) and its two tests
__global__ __launch_bounds__(KT) void davidson_finish_kernel(uint64_t nb, const double* __restrict__ part, int ph, DState* st) {
    __shared__ double2 sh[KT];
    if (ph == D_BETA && (st->stop | st->skip)) return;
    double a0 = 0.0;
    for (uint64_t i = threadIdx.x; i < nb; i += KT) a0 += part[i];
    const double2 d = tree256(make_double2(a0, 0.0), sh);
    if (threadIdx.x != 0) return;
    auto stopAt = [&](int status) { st->status = status; st->stop = 1; st->skip = 1; };
    if (ph == D_INIT) {
        st->exact = 0; st->stop = 0; st->skip = 0; st->status = SPMV_KRYLOV_MAXITER;
        if (!isfinite(d.x)) stopAt(SPMV_KRYLOV_NONFINITE);
        else if (d.x == 0.0) stopAt(SPMV_KRYLOV_BREAKDOWN);
        else if (st->maxIter == 0) stopAt(SPMV_KRYLOV_MAXITER);
        else st->nrm = sqrt(d.x);
        return;
    }
    const double beta = sqrt(d.x);
    st->beta = beta;
    if (!isfinite(beta)) stopAt(SPMV_KRYLOV_NONFINITE);
    else if (beta == 0.0) { st->exact = 1; st->skip = 1; }
}

}  // namespace

int enqueueBlockResidual(uint64_t n, uint32_t m, uint32_t k, const double* V, uint64_t ldv, const double* W, uint64_t ldw, const double* S,
                         uint64_t lds, const double* theta, double* R, uint64_t ldr, double* part, double* norm2, const uint32_t* flags,
                         hipStream_t st, dim3* gridOut) {
    const uint64_t nb = blocksOf(n);
    const bool vec = aligned16(V) && aligned16(W) && aligned16(R) && (m == 1 || (ldv % 2 == 0 && ldw % 2 == 0)) && (k == 1 || ldr % 2 == 0);
    const dim3 grid = grid2d(nb, KT);
    if (gridOut) *gridOut = grid;
    if (n == 0) return EXIT_SUCCESS;
    if (k <= 4)      launchResidual<4>(vec, grid, st, n, m, k, V, ldv, W, ldw, S, lds, theta, R, ldr, part, nb, flags);
    else if (k <= 8) launchResidual<8>(vec, grid, st, n, m, k, V, ldv, W, ldw, S, lds, theta, R, ldr, part, nb, flags);
    else             launchResidual<16>(vec, grid, st, n, m, k, V, ldv, W, ldw, S, lds, theta, R, ldr, part, nb, flags);
    hipLaunchKernelGGL(multidot_finish_kernel, dim3((k + 1) / 2), dim3(KT), 0, st, nb, k, part, norm2, flags);
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

int blockResidual(uint64_t n, uint32_t m, uint32_t k, const double* V, uint64_t ldv, const double* W, uint64_t ldw, const double* S,
                  uint64_t lds, const double* theta, double* R, uint64_t ldr, double* norm2, hipStream_t st, dim3* grid) {
    double* part = nullptr;
    if (n && dotWorkspace((uint64_t)k * blocksOf(n), &part)) return EXIT_FAILURE;
    return enqueueBlockResidual(n, m, k, V, ldv, W, ldw, S, lds, theta, R, ldr, part, norm2, nullptr, st, grid);
}

size_t davidsonWorkspaceBytes(uint64_t n, uint32_t ncv, uint32_t nev, int precond) {
    const uint64_t ldv = (n + 1) & ~1ull, nb = std::max<uint64_t>(blocksOf(n), 1);
    return (size_t)((2 * (uint64_t)ncv + nev + (precond ? 1 : 0)) * ldv * 8 + ((uint64_t)ncv + 1) * nb * 8 +
                    ((size_t)LZ_MAXM * LZ_MAXM + DV_MAXK) * 8 + sizeof(DState));
}

int davidsonSolve(spmat* hA, const DevMat* a, const DevMat* dm, const double* v0, const spmvDavidsonOpts* o, double* X, uint64_t ldx,
                  double* theta, double* res, spmvDavidsonInfo* info, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = a->M, nb = std::max<uint64_t>(blocksOf(n), 1), ldv = (n + 1) & ~1ull;
    const uint32_t m = o->ncv, nev = o->nev, kk = o->keep ? o->keep : lanczosDefaultKeep(nev, m);
    const bool pre = dm != nullptr;
    spmvDavidsonInfo out{};
    DevBufs ws;
    double* V = ws.alloc<double>((uint64_t)m * ldv);                     // the basis v[0 .. m-1], every column 16-byte aligned
    double* W = ws.alloc<double>((uint64_t)m * ldv);                     // w[j] = A v[j], rotated with the basis
    double* R = ws.alloc<double>((uint64_t)nev * ldv);                   // the residual block; without a dM its column l is t
    double* tv = pre ? ws.alloc<double>(ldv) : nullptr;                  // t = M^-1 R(:, l): no apply runs in place
    double* part = ws.alloc<double>(((uint64_t)m + 1) * nb);             // m columns of partials; one more for the single dots
    double* dS = ws.alloc<double>((size_t)LZ_MAXM * LZ_MAXM + DV_MAXK);  // theta[0 .. 15], then column c of the block at [16 + c*LZ_MAXM ..]
    DState* st = ws.alloc<DState>(1);
    if (!V || !W || !R || (pre && !tv) || !part || !dS || !st) { fprintf(stderr, "libspmvhip: Davidson: workspace allocation failed\n"); return EXIT_FAILURE; }
    double* p0 = part + (uint64_t)m * nb;
    double* dTh = dS;
    double* dSb = dS + DV_MAXK;
    DState h{};
    h.maxIter = o->maxIter;
    HIP_TRY(hipMemcpyAsync(st, &h, DSTATE_HEAD, hipMemcpyHostToDevice, s));
    const uint32_t* flags = &st->stop;                                   // {stop, skip}
    const dim3 ugrid = grid2d(nb, KT);
    const Precond pc(dm, hA, s);
    auto finish = [&](int ph) {
        hipLaunchKernelGGL(davidson_finish_kernel, dim3(1), dim3(KT), 0, s, blocksOf(n), p0, ph, st);
        ++out.launches;
    };
    auto project = [&](const double* w, uint32_t k, double* coef) {      // coef[0 .. k-1] = V^T w
        launchMultiDot(n, k, V, ldv, w, part, coef, true, flags, s);
        out.launches += 2;
    };
    auto scale = [&](const double* in, double* outv, const double* by) { // outv = in / *by, unless skip
        launchVec(n, nullptr, GScaleOp{in, outv, by, &st->skip, 0.0}, aligned16(in) && aligned16(outv), p0, p0, s);
        ++out.launches;
    };
    std::vector<double> hS((size_t)DV_MAXK + (size_t)LZ_MAXM * LZ_MAXM);
    // theta[0 .. k-1] and the first k ordered columns of S (rows 0 .. cols-1) to the device: one copy
    auto upload = [&](const std::vector<double>& Sm, const uint32_t* order, const double* th, uint32_t cols, uint32_t k) {
        for (uint32_t c = 0; c < k; ++c) {
            if (c < DV_MAXK) hS[c] = th[c];
            for (uint32_t j = 0; j < cols; ++j) hS[DV_MAXK + (size_t)c * LZ_MAXM + j] = Sm[(size_t)j * LZ_MAXM + order[c]];
        }
        HIP_TRY(hipMemcpyAsync(dS, hS.data(), (DV_MAXK + (size_t)k * LZ_MAXM) * sizeof(double), hipMemcpyHostToDevice, s));
        return EXIT_SUCCESS;
    };
    uint64_t it = 0;
    auto done = [&](int status, uint32_t found) {
        out.status = status;
        out.found = found;
        out.iterations = it;
        out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (info) *info = out;
        return EXIT_SUCCESS;
    };
    // v[0] = v0 / sqrt(dot(v0, v0)), and the exits before the first step
    launchVec(n, nullptr, DotOp{v0, v0}, aligned16(v0), p0, p0, s);
    ++out.launches;
    finish(D_INIT);
    scale(v0, V, &st->nrm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h, st, DSTATE_HEAD, hipMemcpyDeviceToHost, s));   // (the init's exits: not counted as a check)
    HIP_TRY(hipStreamSynchronize(s));
    if (h.stop) return done(h.status, 0);
    std::vector<double> H((size_t)LZ_MAXM * LZ_MAXM, 0.0), A(H.size()), Sm(H.size());
    uint32_t order[LZ_MAXM];
    double th[LZ_MAXM], rs[DV_MAXK];
    auto Hat = [&](uint32_t r, uint32_t c) -> double& { return H[(size_t)r * LZ_MAXM + c]; };
    uint32_t cols = 0, c = 0, l = 0;
    bool restarted = false;                                              // this step's expansion came after a restart
    for (bool first = true;; first = false) {
        if (!first) {
            // the expansion: t = M^-1 R(:, l) (or R(:, l) itself), CGS2 against v[0 .. cols-1], beta, v[cols] = t / beta
            double* t = R + (uint64_t)l * ldv;
            if (pre) {
                if (pc.apply(t, tv, &st->skip, &out.launches)) return EXIT_FAILURE;
                ++out.precondApplies;
                t = tv;
            }
            project(t, cols, st->h);
            hipLaunchKernelGGL(gmres_update_kernel<0>, ugrid, dim3(KT), 0, s, n, cols, V, ldv, t, st->h, part, nb, flags);
            ++out.launches;
            project(t, cols, st->c);
            hipLaunchKernelGGL(gmres_update_kernel<2>, ugrid, dim3(KT), 0, s, n, cols, V, ldv, t, st->c, p0, nb, flags);
            ++out.launches;
            finish(D_BETA);
            scale(t, V + (uint64_t)cols * ldv, &st->beta);
        }
        // the product w[j] = A v[j] and the new column of H
        const uint32_t j = cols;
        ++out.launches;
        if (spmvHipEnqueueAutoRows(hA, V + (uint64_t)j * ldv, W + (uint64_t)j * ldv, s)) return EXIT_FAILURE;
        project(W + (uint64_t)j * ldv, j + 1, st->hcol);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h, st, DSTATE_HEAD, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++out.hostChecks;
        if (h.stop) return done(h.status, 0);
        if (h.exact) {                                                   // beta == 0: the pairs of the step before
            if (restarted) {                                             // (the basis was rotated: its first c columns are V S[:, :c])
                HIP_TRY(hipMemcpy2DAsync(X, ldx * sizeof(double), V, ldv * sizeof(double), n * sizeof(double), c, hipMemcpyDeviceToDevice, s));
            } else if (enqueueBlockCombine(n, cols, c, V, ldv, dSb, LZ_MAXM, X, ldx, s, nullptr)) return EXIT_FAILURE;
            ++out.launches;
            HIP_TRY(hipStreamSynchronize(s));
            for (uint32_t i = 0; i < c; ++i) { theta[i] = th[i]; res[i] = rs[i]; }
            return done(SPMV_KRYLOV_BREAKDOWN, c);
        }
        ++it;
        bool finite = true;
        for (uint32_t i = 0; i <= j; ++i) {
            Hat(i, j) = Hat(j, i) = h.hcol[i];
            finite = finite && std::isfinite(h.hcol[i]);
        }
        cols = j + 1;
        if (!finite) return done(SPMV_KRYLOV_NONFINITE, 0);
        A = H;
        const auto j0 = std::chrono::steady_clock::now();
        const int sweeps = jacobi(cols, A.data(), Sm.data());
        out.jacobiMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - j0).count();
        out.sweepsMax = std::max<unsigned>(out.sweepsMax, sweeps ? sweeps : JACOBI_SWEEPS);
        finite = sweeps != 0;
        for (uint32_t i = 0; i < cols; ++i) { order[i] = i; finite = finite && std::isfinite(A[(size_t)i * LZ_MAXM + i]); }
        if (!finite) return done(SPMV_KRYLOV_NONFINITE, 0);
        auto diag = [&](uint32_t i) { return A[(size_t)i * LZ_MAXM + i]; };
        if (o->which == SPMV_EIG_SMALLEST) std::stable_sort(order, order + cols, [&](uint32_t x, uint32_t y) { return diag(x) < diag(y); });
        else                               std::stable_sort(order, order + cols, [&](uint32_t x, uint32_t y) { return diag(x) > diag(y); });
        double sc = 0.0;
        for (uint32_t i = 0; i < cols; ++i) {
            th[i] = diag(order[i]);
            sc = std::max(sc, std::fabs(th[i]));
        }
        out.scale = sc;
        c = std::min(nev, cols);
        // the residual block of the c wanted pairs and its norms
        if (upload(Sm, order, th, cols, c)) return EXIT_FAILURE;
        if (enqueueBlockResidual(n, cols, c, V, ldv, W, ldv, dSb, LZ_MAXM, dTh, R, ldv, part, st->n2, flags, s, nullptr)) return EXIT_FAILURE;
        out.launches += 2;
        HIP_TRY(hipMemcpyAsync(h.n2, st->n2, c * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++out.hostChecks;
        finite = true;
        for (uint32_t i = 0; i < c; ++i) { rs[i] = std::sqrt(h.n2[i]); finite = finite && std::isfinite(rs[i]); }
        if (!finite) return done(SPMV_KRYLOV_NONFINITE, 0);
        bool conv = cols >= nev;
        for (uint32_t i = 0; conv && i < nev; ++i) conv = rs[i] <= o->tol * sc;
        if (conv || it == o->maxIter) {
            if (enqueueBlockCombine(n, cols, c, V, ldv, dSb, LZ_MAXM, X, ldx, s, nullptr)) return EXIT_FAILURE;
            ++out.launches;
            HIP_TRY(hipStreamSynchronize(s));
            for (uint32_t i = 0; i < c; ++i) { theta[i] = th[i]; res[i] = rs[i]; }
            return done(conv ? SPMV_KRYLOV_CONVERGED : SPMV_KRYLOV_MAXITER, c);
        }
        for (l = 0; l < c && rs[l] <= o->tol * sc; ++l) {}               // the first wanted pair that has not converged
        if (l == c) l = c - 1;                                           // (none: cols < nev)
        restarted = cols == m;
        if (restarted) {
            // the restart: the kk wanted Ritz vectors and their products; H = diag(theta)
            if (upload(Sm, order, th, m, kk)) return EXIT_FAILURE;
            if (enqueueBlockCombine(n, m, kk, V, ldv, dSb, LZ_MAXM, V, ldv, s, nullptr)) return EXIT_FAILURE;
            if (enqueueBlockCombine(n, m, kk, W, ldv, dSb, LZ_MAXM, W, ldv, s, nullptr)) return EXIT_FAILURE;
            out.launches += 2;
            std::fill(H.begin(), H.end(), 0.0);
            for (uint32_t i = 0; i < kk; ++i) Hat(i, i) = th[i];
            cols = kk;
            ++out.restarts;
        }
    }
}

}  // namespace spmvhip
