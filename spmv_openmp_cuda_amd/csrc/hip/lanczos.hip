// lanczos.hip -- the basis rotation Y = V S (spmvHipBlockCombine) and thick-restart Lanczos with CGS2 reorthogonalisation
// (hipSpLanczosCSR) on a symmetric device CSR handle (contract in spmvHip.h, design in DESIGN.md section 39).  Every
// Y(i, c) is the in-order rounded sum of the header; theta, res, X and the counts are the bits of the loop written there.
//
// The rotation: a lane owns a row (two adjacent rows in the 16-byte form).  It loads the row's m values, column by column,
// so a wave's load is one contiguous run of V's column; then, output column by output column, it adds the m products in
// ascending j from +0.0 and stores the sum.  The row is complete in registers before the first store, which is what makes
// dY == dV legal.  S is read at wave-uniform addresses.  Register budget: the row is m doubles = 2 m VGPRs a lane (4 m in the
// 16-byte form), so the kernel is instantiated for m <= 8, 16, 32 and 64, and the 16-byte form stops at m <= 32
// (128 VGPRs of row either way: three to four waves a SIMD, enough loads in flight for a stream); the sums of four output
// columns (two in the 16-byte form) are formed together -- BC_COLS = 4 independent add chains --, so k costs no registers
// beyond those.  Columns of the row are walked in chunks of BC_CHUNK with one uniform
// branch a chunk.  No MFMA, no FMA.
//
// The solver: the step's scalars (h, c, alpha, beta, the matvec count, the status) live in a device state block that only
// single-lane finish steps write.  `stop` ends the solve (a value that is not finite), `skip` ends the cycle's remaining
// enqueued steps (beta == 0, maxIter, stop).  The host enqueues a cycle's steps, reads the head of the block back once,
// runs Jacobi on the projected matrix, uploads the wanted block of S and enqueues the rotation.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "spmvHip.h"
#include "kernels.hpp"
#include "krylov.hpp"
#include "orth.hpp"
#include "jacobi.hpp"

namespace spmvhip {
namespace {

constexpr uint32_t BC_T = 256;                  // lanes of a rotation workgroup
constexpr int      BC_CHUNK = 8;                // columns of the row between two uniform branches
constexpr int      BC_COLS = 4;                 // independent add chains of a lane: 4 output columns, 2 in the 16-byte form

// ------------------------------------------------------------------------------------------------ the rotation
template <bool VEC> using RowT = std::conditional_t<VEC, double2, double>;

template <bool VEC>
__device__ __forceinline__ RowT<VEC> rowLoad(const double* p, uint64_t i, bool two) {
    if constexpr (VEC) return ld2<true>(p, i, two);
    else return p[i];
}
template <bool VEC>
__device__ __forceinline__ void rowStore(double* p, uint64_t i, bool two, RowT<VEC> v) {
    if constexpr (VEC) st2<true>(p, i, two, v);
    else p[i] = v;
}
__device__ __forceinline__ void rowMadd(double& a, double v, double s) { a = a + v * s; }
__device__ __forceinline__ void rowMadd(double2& a, double2 v, double s) { a.x = a.x + v.x * s; a.y = a.y + v.y * s; }

// NB output columns of this lane's row at once: NB independent sums, each in ascending j from +0.0 (a column's order does
// not depend on NB), so the dependent add chain of one column is interleaved with its neighbours'
template <int MCAP, bool VEC, int NB>
__device__ __forceinline__ void combineColumns(const RowT<VEC> (&v)[MCAP], uint32_t m, const double* __restrict__ s, uint64_t lds, double* y,
                                               uint64_t ldy, uint64_t i, bool two) {
    RowT<VEC> acc[NB] = {};
#pragma unroll
    for (int jc = 0; jc < MCAP; jc += BC_CHUNK) {
        if (jc + BC_CHUNK <= (int)m) {
#pragma unroll
            for (int u = 0; u < BC_CHUNK; ++u)
#pragma unroll
                for (int b = 0; b < NB; ++b) rowMadd(acc[b], v[jc + u], s[(uint64_t)b * lds + jc + u]);
        } else if (jc < (int)m) {
#pragma unroll
            for (int u = 0; u < BC_CHUNK; ++u)
                if (jc + u < (int)m) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) rowMadd(acc[b], v[jc + u], s[(uint64_t)b * lds + jc + u]);
                }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) rowStore<VEC>(y + (uint64_t)b * ldy, i, two, acc[b]);
}

// Y(i, c) = sum_j V(i, j) * S[j][c], j ascending from +0.0; V and Y may be the same block (no __restrict__ on either)
template <int MCAP, bool VEC>
__global__ __launch_bounds__(BC_T) void block_combine_kernel(uint64_t n, uint32_t m, uint32_t k, const double* V, uint64_t ldv,
                                                             const double* __restrict__ S, uint64_t lds, double* Y, uint64_t ldy) {
    const uint64_t t = linear_block() * BC_T + threadIdx.x;
    const uint64_t i = VEC ? 2 * t : t;
    if (i >= n) return;                                                  // (the last workgroup's tail, a folded grid's)
    const bool two = VEC && i + 1 < n;
    RowT<VEC> v[MCAP];
#pragma unroll
    for (int jc = 0; jc < MCAP; jc += BC_CHUNK) {
        if (jc + BC_CHUNK <= (int)m) {
#pragma unroll
            for (int u = 0; u < BC_CHUNK; ++u) v[jc + u] = rowLoad<VEC>(V + (uint64_t)(jc + u) * ldv, i, two);
        } else if (jc < (int)m) {
#pragma unroll
            for (int u = 0; u < BC_CHUNK; ++u)
                if (jc + u < (int)m) v[jc + u] = rowLoad<VEC>(V + (uint64_t)(jc + u) * ldv, i, two);
        }
    }
    uint32_t c = 0;
    constexpr int NB = VEC ? BC_COLS / 2 : BC_COLS;
    for (; c + NB <= k; c += NB) combineColumns<MCAP, VEC, NB>(v, m, S + (uint64_t)c * lds, lds, Y + (uint64_t)c * ldy, ldy, i, two);
    for (; c < k; ++c) combineColumns<MCAP, VEC, 1>(v, m, S + (uint64_t)c * lds, lds, Y + (uint64_t)c * ldy, ldy, i, two);
}

template <int MCAP>
void launchCombine(bool vec, dim3 grid, hipStream_t st, uint64_t n, uint32_t m, uint32_t k, const double* V, uint64_t ldv, const double* S,
                   uint64_t lds, double* Y, uint64_t ldy) {
    if constexpr (MCAP <= 32) {
        if (vec) { hipLaunchKernelGGL((block_combine_kernel<MCAP, true>), grid, dim3(BC_T), 0, st, n, m, k, V, ldv, S, lds, Y, ldy); return; }
    }
    hipLaunchKernelGGL((block_combine_kernel<MCAP, false>), grid, dim3(BC_T), 0, st, n, m, k, V, ldv, S, lds, Y, ldy);
}

// ------------------------------------------------------------------------------------------------ the solver's state
struct LState {
    uint32_t stop;          // 0 while the solve runs
    uint32_t skip;          // 1 once the cycle's remaining steps are to do nothing (stop implies skip)
    int32_t  status;        // SPMV_KRYLOV_* once stopped
    uint32_t cols;          // Lanczos columns the basis holds: the last finished step's j + 1
    uint32_t exact;         // the last step found beta == 0
    uint32_t pad;
    uint64_t it, maxIter;
    double   nrm;           // sqrt(dot(v0, v0))
    double   alpha[LZ_MAXM], beta[LZ_MAXM];
    // ---- not read back
    double   h[LZ_MAXM], c[LZ_MAXM];
};
constexpr size_t LSTATE_HEAD = offsetof(LState, h);

enum LPhase : int { L_INIT, L_WW };

// the block partials of one dot (krylov_finish_kernel's rule), then lane 0 runs the loop's scalar step:
//   L_INIT  dot(v0, v0): the three first exits, or nrm
//   L_WW    step j: alpha = h[j] + c[j], beta = sqrt(dot(w,w)), the matvec count and the step's tests
__global__ __launch_bounds__(KT) void lanczos_finish_kernel(uint64_t nb, const double* __restrict__ part, int ph, uint32_t j, LState* st) {
    __shared__ double2 sh[KT];
    if (ph == L_WW && (st->stop | st->skip)) return;
    double a0 = 0.0;
    for (uint64_t i = threadIdx.x; i < nb; i += KT) a0 += part[i];
    const double2 d = tree256(make_double2(a0, 0.0), sh);
    if (threadIdx.x != 0) return;
    auto stopAt = [&](int status) { st->status = status; st->stop = 1; st->skip = 1; };
    if (ph == L_INIT) {
        st->it = 0; st->cols = 0; st->exact = 0; st->stop = 0; st->skip = 0; st->status = SPMV_KRYLOV_MAXITER;
        if (!isfinite(d.x)) stopAt(SPMV_KRYLOV_NONFINITE);
        else if (d.x == 0.0) stopAt(SPMV_KRYLOV_BREAKDOWN);
        else if (st->maxIter == 0) stopAt(SPMV_KRYLOV_MAXITER);
        else st->nrm = sqrt(d.x);
        return;
    }
    const double alpha = st->h[j] + st->c[j], beta = sqrt(d.x);
    st->alpha[j] = alpha; st->beta[j] = beta;
    st->cols = j + 1;
    const uint64_t it = ++st->it;
    if (!isfinite(alpha) || !isfinite(beta)) stopAt(SPMV_KRYLOV_NONFINITE);
    else if (beta == 0.0) { st->exact = 1; st->skip = 1; }
    else if (it == st->maxIter) st->skip = 1;
}

}  // namespace

int enqueueBlockCombine(uint64_t n, uint32_t m, uint32_t k, const double* V, uint64_t ldv, const double* S, uint64_t lds, double* Y,
                        uint64_t ldy, hipStream_t st, dim3* gridOut) {
    const bool vec = m <= 32 && aligned16(V) && aligned16(Y) && (m == 1 || ldv % 2 == 0) && (k == 1 || ldy % 2 == 0);
    const uint64_t rows = vec ? 2 * BC_T : BC_T;
    const dim3 grid = grid2d((n + rows - 1) / rows, BC_T);
    if (gridOut) *gridOut = grid;
    if (n == 0) return EXIT_SUCCESS;
    if (m <= 8)       launchCombine<8>(vec, grid, st, n, m, k, V, ldv, S, lds, Y, ldy);
    else if (m <= 16) launchCombine<16>(vec, grid, st, n, m, k, V, ldv, S, lds, Y, ldy);
    else if (m <= 32) launchCombine<32>(vec, grid, st, n, m, k, V, ldv, S, lds, Y, ldy);
    else              launchCombine<64>(vec, grid, st, n, m, k, V, ldv, S, lds, Y, ldy);
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

unsigned lanczosDefaultKeep(unsigned nev, unsigned ncv) { return std::min(ncv - 1, nev + (ncv - nev) / 2); }

size_t lanczosWorkspaceBytes(uint64_t n, uint32_t ncv) {
    const uint64_t ldv = (n + 1) & ~1ull, nb = std::max<uint64_t>(blocksOf(n), 1);
    return (size_t)(((uint64_t)ncv + 2) * ldv * 8 + ((uint64_t)ncv + 1) * nb * 8 + (size_t)LZ_MAXM * LZ_MAXM * 8 + sizeof(LState));
}

int lanczosSolve(spmat* hA, const DevMat* a, const double* v0, const spmvLanczosOpts* o, double* X, uint64_t ldx, double* theta,
                 double* res, spmvLanczosInfo* info, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = a->M, nb = std::max<uint64_t>(blocksOf(n), 1), ldv = (n + 1) & ~1ull;
    const uint32_t m = o->ncv, nev = o->nev, kk = o->keep ? o->keep : lanczosDefaultKeep(nev, m);
    spmvLanczosInfo out{};
    DevBufs ws;
    double* V = ws.alloc<double>(((uint64_t)m + 1) * ldv);               // the basis v[0 .. m], every column 16-byte aligned
    double* w = ws.alloc<double>(ldv);
    double* part = ws.alloc<double>(((uint64_t)m + 1) * nb);             // m columns of partials; one more for the single dots
    double* dS = ws.alloc<double>((size_t)LZ_MAXM * LZ_MAXM);            // column c of the uploaded block at dS[c*LZ_MAXM ..]
    LState* st = ws.alloc<LState>(1);
    if (!V || !w || !part || !dS || !st) { fprintf(stderr, "libspmvhip: Lanczos: workspace allocation failed\n"); return EXIT_FAILURE; }
    double* p0 = part + (uint64_t)m * nb;
    LState h{};
    h.maxIter = o->maxIter;
    HIP_TRY(hipMemcpyAsync(st, &h, LSTATE_HEAD, hipMemcpyHostToDevice, s));
    const uint32_t* flags = &st->stop;                                   // {stop, skip}
    const dim3 ugrid = grid2d(nb, KT);
    auto finish = [&](int ph, uint32_t j) {
        hipLaunchKernelGGL(lanczos_finish_kernel, dim3(1), dim3(KT), 0, s, blocksOf(n), p0, ph, j, st);
        ++out.launches;
    };
    auto project = [&](uint32_t k, double* coef) {                       // coef[0 .. k-1] = V^T w
        launchMultiDot(n, k, V, ldv, w, part, coef, true, flags, s);
        out.launches += 2;
    };
    auto scale = [&](const double* in, double* outv, const double* by) { // outv = in / *by, unless skip
        launchVec(n, nullptr, GScaleOp{in, outv, by, &st->skip, 0.0}, aligned16(in) && aligned16(outv), p0, p0, s);
        ++out.launches;
    };
    std::vector<double> hS((size_t)LZ_MAXM * LZ_MAXM);
    auto rotate = [&](const std::vector<double>& Sm, const uint32_t* order, uint32_t cols, uint32_t k, double* Y, uint64_t ldy) {
        for (uint32_t c = 0; c < k; ++c)                                 // Y(:, c) = V(:, 0 .. cols-1) S(:, order[c])
            for (uint32_t j = 0; j < cols; ++j) hS[(size_t)c * LZ_MAXM + j] = Sm[(size_t)j * LZ_MAXM + order[c]];
        HIP_TRY(hipMemcpyAsync(dS, hS.data(), (size_t)k * LZ_MAXM * sizeof(double), hipMemcpyHostToDevice, s));
        ++out.launches;
        return enqueueBlockCombine(n, cols, k, V, ldv, dS, LZ_MAXM, Y, ldy, s, nullptr);
    };
    auto done = [&](int status, uint32_t found) {
        out.status = status;
        out.found = found;
        out.iterations = h.it;
        out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (info) *info = out;
        return EXIT_SUCCESS;
    };
    // v[0] = v0 / sqrt(dot(v0, v0)), and the exits before the first cycle
    launchVec(n, nullptr, DotOp{v0, v0}, aligned16(v0), p0, p0, s);
    ++out.launches;
    finish(L_INIT, 0);
    scale(v0, V, &st->nrm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h, st, LSTATE_HEAD, hipMemcpyDeviceToHost, s));   // (the init's exits: not counted as a check)
    HIP_TRY(hipStreamSynchronize(s));
    if (h.stop) return done(h.status, 0);
    std::vector<double> T((size_t)LZ_MAXM * LZ_MAXM, 0.0), A(T.size()), Sm(T.size());
    uint32_t order[LZ_MAXM];
    double th[LZ_MAXM], rs[LZ_MAXM];
    auto Tat = [&](uint32_t r, uint32_t c) -> double& { return T[(size_t)r * LZ_MAXM + c]; };
    for (uint32_t k = 0;;) {
        ++out.cycles;
        const uint32_t steps = (uint32_t)std::min<uint64_t>(m - k, o->maxIter - h.it);
        for (uint32_t j = k; j < k + steps; ++j) {
            ++out.launches;
            if (spmvHipEnqueueAutoRows(hA, V + (uint64_t)j * ldv, w, s)) return EXIT_FAILURE;
            project(j + 1, st->h);
            hipLaunchKernelGGL(gmres_update_kernel<0>, ugrid, dim3(KT), 0, s, n, j + 1, V, ldv, w, st->h, part, nb, flags);
            ++out.launches;
            project(j + 1, st->c);
            hipLaunchKernelGGL(gmres_update_kernel<2>, ugrid, dim3(KT), 0, s, n, j + 1, V, ldv, w, st->c, p0, nb, flags);
            ++out.launches;
            finish(L_WW, j);
            scale(w, V + (uint64_t)(j + 1) * ldv, &st->beta[j]);         // v[j+1] = w / beta
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h, st, LSTATE_HEAD, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++out.hostChecks;
        if (h.stop) return done(h.status, 0);
        const uint32_t cols = h.cols;
        const bool exact = h.exact != 0, last = h.it == o->maxIter;
        if (cols <= k || cols > m || (cols < m && !exact && !last)) { fprintf(stderr, "libspmvhip: Lanczos: a cycle did not end\n"); return EXIT_FAILURE; }
        for (uint32_t j = k; j < cols; ++j) {
            Tat(j, j) = h.alpha[j];
            if (j + 1 < cols) Tat(j, j + 1) = Tat(j + 1, j) = h.beta[j];
        }
        const double beta = h.beta[cols - 1];
        A = T;
        const auto j0 = std::chrono::steady_clock::now();
        const int sweeps = jacobi(cols, A.data(), Sm.data());
        out.jacobiMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - j0).count();
        out.sweepsMax = std::max<unsigned>(out.sweepsMax, sweeps ? sweeps : JACOBI_SWEEPS);
        bool finite = sweeps != 0;
        for (uint32_t i = 0; i < cols; ++i) { order[i] = i; finite = finite && std::isfinite(A[(size_t)i * LZ_MAXM + i]); }
        if (!finite) return done(SPMV_KRYLOV_NONFINITE, 0);
        auto diag = [&](uint32_t i) { return A[(size_t)i * LZ_MAXM + i]; };
        if (o->which == SPMV_EIG_SMALLEST) std::stable_sort(order, order + cols, [&](uint32_t x, uint32_t y) { return diag(x) < diag(y); });
        else                               std::stable_sort(order, order + cols, [&](uint32_t x, uint32_t y) { return diag(x) > diag(y); });
        double sc = 0.0;
        for (uint32_t i = 0; i < cols; ++i) {
            th[i] = diag(order[i]);
            rs[i] = exact ? 0.0 : std::fabs(beta * Sm[(size_t)(cols - 1) * LZ_MAXM + order[i]]);
            sc = std::max(sc, std::fabs(th[i]));
        }
        out.scale = sc;
        const uint32_t found = std::min(nev, cols);
        bool conv = cols >= nev;
        for (uint32_t i = 0; conv && i < nev; ++i) conv = rs[i] <= o->tol * sc;
        if (conv || exact || last) {
            if (rotate(Sm, order, cols, found, X, ldx)) return EXIT_FAILURE;
            HIP_TRY(hipStreamSynchronize(s));
            for (uint32_t i = 0; i < found; ++i) { theta[i] = th[i]; res[i] = rs[i]; }
            return done(conv ? SPMV_KRYLOV_CONVERGED : exact ? SPMV_KRYLOV_BREAKDOWN : SPMV_KRYLOV_MAXITER, found);
        }
        // the restart: the kk wanted Ritz vectors, then v[m]; T = diag(theta) with the coupling row beta * S[m-1][.]
        if (rotate(Sm, order, m, kk, V, ldv)) return EXIT_FAILURE;
        HIP_TRY(hipMemcpyAsync(V + (uint64_t)kk * ldv, V + (uint64_t)m * ldv, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        std::fill(T.begin(), T.end(), 0.0);
        for (uint32_t i = 0; i < kk; ++i) {
            Tat(i, i) = th[i];
            Tat(kk, i) = Tat(i, kk) = beta * Sm[(size_t)(m - 1) * LZ_MAXM + order[i]];
        }
        k = kk;
    }
}

}  // namespace spmvhip
