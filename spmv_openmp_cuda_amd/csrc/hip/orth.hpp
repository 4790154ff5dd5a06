// orth.hpp -- the CGS2 orthogonalisation step that gmres.hip and lanczos.hip share: h = V^T w in one pass (the two kernels
// of spmvHipMultiDot), the update w = w - sum coef[i] v[i] with the partials of the next projection or of dot(w,w), and
// out = in / *s.  Every entry of h is the bits of spmvHipDot on its column.
//
// The multi-dot: a workgroup takes one block of KB = 4096 indices and a panel of MD_PANEL columns.  It loads its 16 doubles
// of w per lane once, keeps them in registers and walks the panel's columns, a column's eight slices issued as
// krylov_vec_kernel issues them; two columns meet in one pass of the double2 tree.  Block partials go to part[i*nb + blk];
// a second kernel, one workgroup per pair of columns, adds them by the rule of krylov_finish_kernel.  Ordering between
// the two is the kernel boundary.
//
// `flags` is {stop, skip} of a solve's state block (null for the public multi-dot): every kernel returns at once when
// either is set.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>

#include "kernels.hpp"
#include "krylov.hpp"

namespace spmvhip {
namespace {

constexpr uint32_t MD_PANEL = 16;               // columns a multi-dot workgroup walks with one load of w

// w's 16 doubles of this lane: elements base + 512 s, base + 512 s + 1 (zeros past n)
template <bool VEC>
__device__ __forceinline__ void loadW(const double* __restrict__ w, uint64_t base, uint64_t n, bool full, double2 (&wv)[KSLICES]) {
#pragma unroll
    for (uint32_t s = 0; s < KSLICES; ++s) {
        const uint64_t i = base + (uint64_t)s * (2 * KT);
        wv[s] = make_double2(0.0, 0.0);
        if (full || i < n) wv[s] = ld2<VEC>(w, i, full || i + 1 < n);
    }
}
template <bool VEC>
__device__ __forceinline__ void storeW(double* __restrict__ w, uint64_t base, uint64_t n, bool full, const double2 (&wv)[KSLICES]) {
#pragma unroll
    for (uint32_t s = 0; s < KSLICES; ++s) {
        const uint64_t i = base + (uint64_t)s * (2 * KT);
        if (full || i < n) st2<VEC>(w, i, full || i + 1 < n, wv[s]);
    }
}

// this lane's partial of v . w in spmvHipDot's order: from +0.0, slices ascending, the pair's elements in order
template <bool VEC>
__device__ __forceinline__ double colDot(const double* __restrict__ v, uint64_t base, uint64_t n, bool full, const double2 (&wv)[KSLICES]) {
    double a = 0.0;
#pragma unroll
    for (uint32_t c = 0; c < KSLICES; c += KCHUNK) {
        double2 r[KCHUNK];
#pragma unroll
        for (uint32_t u = 0; u < KCHUNK; ++u) {
            const uint64_t i = base + (uint64_t)(c + u) * (2 * KT);
            if (full || i < n) r[u] = ld2<VEC>(v, i, full || i + 1 < n);
        }
#pragma unroll
        for (uint32_t u = 0; u < KCHUNK; ++u) {
            const uint64_t i = base + (uint64_t)(c + u) * (2 * KT);
            if (full || i < n) madd(a, r[u], wv[c + u], full || i + 1 < n);
        }
    }
    return a;
}

// wv = wv - s * v, element by element (two roundings)
template <bool VEC>
__device__ __forceinline__ void colAxpy(const double* __restrict__ v, double s, uint64_t base, uint64_t n, bool full, double2 (&wv)[KSLICES]) {
#pragma unroll
    for (uint32_t c = 0; c < KSLICES; c += KCHUNK) {
        double2 r[KCHUNK];
#pragma unroll
        for (uint32_t u = 0; u < KCHUNK; ++u) {
            const uint64_t i = base + (uint64_t)(c + u) * (2 * KT);
            r[u] = make_double2(0.0, 0.0);
            if (full || i < n) r[u] = ld2<VEC>(v, i, full || i + 1 < n);
        }
#pragma unroll
        for (uint32_t u = 0; u < KCHUNK; ++u) {
            wv[c + u].x = wv[c + u].x - s * r[u].x;
            wv[c + u].y = wv[c + u].y - s * r[u].y;
        }
    }
}

// columns [c0, c1) of V against the w in registers: block partials part[c*nb + blk], two columns a tree pass; the passes
// alternate between two LDS buffers, so a lane still reading one pass's root does not meet the next pass's first write
template <bool VEC>
__device__ __forceinline__ void panelDots(const double* __restrict__ V, uint64_t ldv, uint32_t c0, uint32_t c1, uint64_t base, uint64_t n,
                                          bool full, const double2 (&wv)[KSLICES], double* __restrict__ part, uint64_t nb, uint64_t blk,
                                          double2 (*sh)[KT]) {
    uint32_t flip = 0;
    for (uint32_t c = c0; c < c1; c += 2, flip ^= 1) {
        const bool pair = c + 1 < c1;
        const double a0 = colDot<VEC>(V + (uint64_t)c * ldv, base, n, full, wv);
        const double a1 = pair ? colDot<VEC>(V + (uint64_t)(c + 1) * ldv, base, n, full, wv) : 0.0;
        const double2 s = tree256(make_double2(a0, a1), sh[flip]);
        if (threadIdx.x == 0) {
            part[(uint64_t)c * nb + blk] = s.x;
            if (pair) part[(uint64_t)(c + 1) * nb + blk] = s.y;
        }
    }
}

// spmvHipMultiDot, first kernel: grid (blocks folded in x, y; panels in z).  flags: null, or {stop, skip} of a solve
template <bool VEC>
__global__ __launch_bounds__(KT) void multidot_part_kernel(uint64_t n, uint32_t k, const double* __restrict__ V, uint64_t ldv,
                                                           const double* __restrict__ w, double* __restrict__ part, uint64_t nb,
                                                           const uint32_t* __restrict__ flags) {
    __shared__ double2 sh[2][KT];
    if (flags && (flags[0] | flags[1])) return;
    const uint64_t blk = linear_block();
    if (blk >= nb) return;                                               // (a folded grid's tail)
    const uint64_t base = blk * KB + 2 * threadIdx.x;
    const bool full = blk * KB + KB <= n;
    double2 wv[KSLICES];
    loadW<VEC>(w, base, n, full, wv);
    const uint32_t c0 = blockIdx.z * MD_PANEL;
    panelDots<VEC>(V, ldv, c0, min(k, c0 + MD_PANEL), base, n, full, wv, part, nb, blk, sh);
}

// second kernel: workgroup p adds the block partials of columns 2p and 2p + 1 (lane t: partials t, t + 256, ... in order,
// then the tree) into out[2p], out[2p + 1]
__global__ __launch_bounds__(KT) void multidot_finish_kernel(uint64_t nb, uint32_t k, const double* __restrict__ part,
                                                             double* __restrict__ out, const uint32_t* __restrict__ flags) {
    __shared__ double2 sh[KT];
    if (flags && (flags[0] | flags[1])) return;
    const uint32_t c = 2 * blockIdx.x;
    const bool pair = c + 1 < k;
    const double* p0 = part + (uint64_t)c * nb;
    const double* p1 = p0 + nb;
    double a0 = 0.0, a1 = 0.0;
    for (uint64_t j = threadIdx.x; j < nb; j += KT) {
        a0 += p0[j];
        if (pair) a1 += p1[j];
    }
    const double2 d = tree256(make_double2(a0, a1), sh);
    if (threadIdx.x != 0) return;
    out[c] = d.x;
    if (pair) out[c + 1] = d.y;
}

// w = w - coef[0] v[0] - coef[1] v[1] - ... (ascending), w read and written once, the columns streamed; then
//   MODE 0: nothing more;  MODE 1: the block partials of V^T w (the next projection);  MODE 2: those of w . w
template <int MODE>
__global__ __launch_bounds__(KT) void gmres_update_kernel(uint64_t n, uint32_t k, const double* __restrict__ V, uint64_t ldv,
                                                          double* __restrict__ w, const double* __restrict__ coef,
                                                          double* __restrict__ part, uint64_t nb, const uint32_t* __restrict__ flags) {
    __shared__ double2 sh[2][KT];
    if (flags[0] | flags[1]) return;
    const uint64_t blk = linear_block();
    if (blk >= nb) return;
    const uint64_t base = blk * KB + 2 * threadIdx.x;
    const bool full = blk * KB + KB <= n;
    double2 wv[KSLICES];
    loadW<true>(w, base, n, full, wv);
    for (uint32_t c = 0; c < k; ++c) colAxpy<true>(V + (uint64_t)c * ldv, coef[c], base, n, full, wv);
    storeW<true>(w, base, n, full, wv);
    if (MODE == 1) panelDots<true>(V, ldv, 0, k, base, n, full, wv, part, nb, blk, sh);
    if (MODE == 2) {
        double a = 0.0;
#pragma unroll
        for (uint32_t s = 0; s < KSLICES; ++s) {
            const uint64_t i = base + (uint64_t)s * (2 * KT);
            if (full || i < n) madd(a, wv[s], wv[s], full || i + 1 < n);
        }
        const double2 d = tree256(make_double2(a, 0.0), sh[0]);
        if (threadIdx.x == 0) part[blk] = d.x;
    }
}

struct GScaleOp {                               // out = in / *s (element by element), unless *flag
    static constexpr int NDOT = 0;
    const double* in; double* out; const double* s; const uint32_t* flag;
    mutable double sv;
    struct R { double2 v; };
    __device__ int mode(const KState*) const { if (*flag) return 0; sv = *s; return 1; }
    template <bool VEC> __device__ void load(uint64_t i, bool two, R& r) const { r.v = ld2<VEC>(in, i, two); }
    template <bool VEC> __device__ void step(uint64_t i, bool two, const R& r, double&, double&) const {
        st2<VEC>(out, i, two, make_double2(r.v.x / sv, two ? r.v.y / sv : 0.0));
    }
};

// the two kernels of h = V^T w into `out` (device), partials in `part` (k * nb doubles)
void launchMultiDot(uint64_t n, uint32_t k, const double* V, uint64_t ldv, const double* w, double* part, double* out, bool vec,
                    const uint32_t* flags, hipStream_t s) {
    const uint64_t nb = blocksOf(n);
    if (nb) {
        const uint32_t ZMAX = 65535;
        for (uint32_t c0 = 0; c0 < k;) {                                 // (one launch unless k > 16 * 65535)
            const uint32_t kc = (uint32_t)std::min<uint64_t>(k - c0, (uint64_t)ZMAX * MD_PANEL);
            dim3 grid = grid2d(nb, KT);
            grid.z = (kc + MD_PANEL - 1) / MD_PANEL;
            const double* Vc = V + (uint64_t)c0 * ldv;
            double* pc = part + (uint64_t)c0 * nb;
            if (vec) hipLaunchKernelGGL(multidot_part_kernel<true>, grid, dim3(KT), 0, s, n, kc, Vc, ldv, w, pc, nb, flags);
            else     hipLaunchKernelGGL(multidot_part_kernel<false>, grid, dim3(KT), 0, s, n, kc, Vc, ldv, w, pc, nb, flags);
            c0 += kc;
        }
    }
    hipLaunchKernelGGL(multidot_finish_kernel, dim3((k + 1) / 2), dim3(KT), 0, s, nb, k, part, out, flags);
}

}  // namespace
}  // namespace spmvhip
