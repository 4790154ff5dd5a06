// krylov_block.hpp -- the fused pass over a block of columns, shared by the block solvers (krylov_block.hip) and the block
// form of the multigrid cycle (amg.hip): the dense block as the kernels take it (made from a Dense of device_mat.hpp, and
// back) and its pair accesses, the partials of a column pair, the kernel of one block of rows and one panel of columns, and
// its launcher.  DESIGN.md sections 27 (the pass), 33 (why a header) and 34 (the operand).
//
// The working vectors are row-major n x kp blocks, kp = k rounded up to even, so a row's column pair (c, c + 1), c even, is
// one 16-byte access; a caller's block is read and written where the caller keeps it, in 16-byte accesses when its layout
// allows and in 8-byte ones otherwise (the same bits).  A workgroup of 256 lanes takes one block of 4096 rows and one panel
// of at most 16 columns.  P adjacent lanes hold the panel's P column pairs (P = 1, 2, 4 or 8, from the widest panel), so
// the 256 / P lane groups read 256 / P row pairs per load instruction, each row a contiguous run of 16 P bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "krylov.hpp"

namespace spmvhip {
namespace {

constexpr uint32_t BK_PANEL = 16;               // columns of a panel (the convention of spmm.hip and trsm.hip)

// a dense block: element (i, c) at p[i*sr + c*sc]; pair: columns (c, c + 1), c even, of a row are one aligned 16-byte access
struct BMat {
    double* p; uint64_t sr, sc; int pair;
};
BMat bmat(const Dense& d, uint32_t k, bool padded) {
    // a caller's block has no element behind column k - 1: with k odd its last pair is not there to be loaded
    const bool pair = d.sc() == 1 && d.sr() % 2 == 0 && aligned16(d.p) && (padded || k % 2 == 0);
    return BMat{d.p, d.sr(), d.sc(), pair};
}
// ... and as the launchers of device_mat.hpp take it (an SpMM, a TRSM, the block cycle on a block of a pass): the same
// strides (one of the two is 1), and a workspace block comes back as the row-major one it was made from
Dense dense(const BMat& m) { return m.sc == 1 ? Dense{m.p, m.sr, true} : Dense{m.p, m.sc, false}; }

__device__ __forceinline__ double2 ldp(const BMat& m, uint64_t i, uint32_t c, bool two) {
    const double* q = m.p + i * m.sr + c * m.sc;
    if (m.pair) return *reinterpret_cast<const double2*>(q);
    return make_double2(q[0], two ? q[m.sc] : 0.0);
}
// columns c (w0) and c + 1 (w1) of row i
__device__ __forceinline__ void stp(const BMat& m, uint64_t i, uint32_t c, int w0, int w1, double2 v) {
    double* q = m.p + i * m.sr + c * m.sc;
    if (m.pair && w0 && w1) { *reinterpret_cast<double2*>(q) = v; return; }
    if (w0) q[0] = v.x;
    if (w1) q[m.sc] = v.y;
}

// the partials of a column pair: d0 / d1 the op's first / second dot, .x column c, .y column c + 1
struct Acc { double2 d0, d1; };
__device__ __forceinline__ Acc accAdd(const Acc& m, const Acc& o) {
    return Acc{make_double2(m.d0.x + o.d0.x, m.d0.y + o.d0.y), make_double2(m.d1.x + o.d1.x, m.d1.y + o.d1.y)};
}

// Each op: NDOT; mode(x, st, sc) for column x (0 / 1) of the lane's pair with that column's state: 0 leaves the column
// alone, otherwise the column's scalars go to the lane's sc; load() one row's inputs for the pair (two: column c + 1 exists); step() the update
// of the columns w0 / w1 and the products, a row at a time in ascending order.  A column that is left alone is still
// computed (its lanes share the pair's loads) but never stored, and its partials are never written.

// "lane t" of the dot's contract for one column pair: rows base + 512 s + 2 t and + 1 for s = 0 .. 7, in that order from +0.0
template <class Op>
__device__ __forceinline__ Acc lane_partial(const Op& op, const typename Op::Sc sc, uint64_t n, uint64_t base, uint32_t t, uint32_t c, bool two, int w0, int w1) {
    Acc a{make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
    if (!(w0 | w1)) return a;
    const uint64_t first = base + 2 * t;
#pragma unroll
    for (uint32_t s = 0; s < KSLICES; s += Op::CHUNK) {
        typename Op::R r[Op::CHUNK][2];
#pragma unroll
        for (uint32_t u = 0; u < Op::CHUNK; ++u) {
            const uint64_t i = first + (uint64_t)(s + u) * (2 * KT);
            if (i < n) op.load(i, c, two, sc, r[u][0]);
            if (i + 1 < n) op.load(i + 1, c, two, sc, r[u][1]);
        }
#pragma unroll
        for (uint32_t u = 0; u < Op::CHUNK; ++u) {
            const uint64_t i = first + (uint64_t)(s + u) * (2 * KT);
            if (i < n) op.step(i, c, w0, w1, sc, r[u][0], a);
            if (i + 1 < n) op.step(i + 1, c, w0, w1, sc, r[u][1], a);
        }
    }
    return a;
}

// the tree's levels h = 128 ... 256 / P on the partials t = g + (256 / P) j of one lane group: a[j] += a[j + S'] for
// S' = P / 2 ... 1, written depth first so that only one partial per level is alive
template <class Op, int P, int S>
__device__ __forceinline__ Acc group_partial(const Op& op, const typename Op::Sc sc, uint64_t n, uint64_t base, uint32_t g, uint32_t j, uint32_t c, bool two,
                                             int w0, int w1) {
    if constexpr (S >= P) {
        return lane_partial(op, sc, n, base, g + (KT / P) * j, c, two, w0, w1);
    } else {
        const Acc m = group_partial<Op, P, 2 * S>(op, sc, n, base, g, j, c, two, w0, w1);
        const Acc o = group_partial<Op, P, 2 * S>(op, sc, n, base, g, j + S, c, two, w0, w1);
        return accAdd(m, o);
    }
}

// one block of KB rows and one panel of columns: the op's update on them, and its dots' block partials into
// part0 / part1[blk * kp + column]
template <class Op, int P>
__global__ __launch_bounds__(KT) void block_vec_kernel(uint64_t n, uint32_t k, uint32_t kp, uint32_t panels,
                                                       const KState* __restrict__ st, const Op op, double* __restrict__ part0,
                                                       double* __restrict__ part1) {
    static_assert(P == 1 || P == 2 || P == 4 || P == 8, "column pairs of a panel");
    __shared__ Acc sh[KT];
    const uint64_t lin = linear_block();
    const uint64_t blk = lin / panels;
    if (blk * KB >= n) return;                                           // (a folded grid's tail)
    const uint32_t tid = threadIdx.x;
    const uint32_t c = (uint32_t)(lin % panels) * BK_PANEL + 2 * (tid % P);
    typename Op::Sc sc{};                                                // the scalars of this lane's two columns
    const int w0 = c < k ? op.mode(0, st + c, sc) : 0;
    const int w1 = c + 1 < k ? op.mode(1, st + c + 1, sc) : 0;
    if (!__syncthreads_or(w0 | w1)) return;                              // every column of this panel has stopped
    Acc a = group_partial<Op, P, 1>(op, sc, n, blk * KB, tid / P, 0, c, c + 1 < k, w0, w1);
    if (Op::NDOT == 0) return;
    sh[tid] = a;
    __syncthreads();
#pragma unroll
    for (uint32_t h = KT / 2; h >= P; h >>= 1) {
        if (tid < h) sh[tid] = accAdd(sh[tid], sh[tid + h]);
        __syncthreads();
    }
    if (tid >= P) return;
    a = sh[tid];
    double* q0 = part0 + blk * kp + c;
    if (w0) q0[0] = a.d0.x;
    if (w1) q0[1] = a.d0.y;
    if (Op::NDOT > 1) {
        double* q1 = part1 + blk * kp + c;
        if (w0) q1[0] = a.d1.x;
        if (w1) q1[1] = a.d1.y;
    }
}

template <class Op>
void launchBlockVec(uint64_t n, uint32_t k, const KState* st, const Op& op, double* p0, double* p1, hipStream_t s) {
    const uint64_t nb = blocksOf(n);
    if (!nb) return;
    const uint32_t kp = k + (k & 1), panels = (k + BK_PANEL - 1) / BK_PANEL;
    const uint32_t w = k < BK_PANEL ? k : BK_PANEL;                      // the widest panel
    const dim3 grid = grid2d(nb * panels, KT);
    if (w <= 2)      hipLaunchKernelGGL((block_vec_kernel<Op, 1>), grid, dim3(KT), 0, s, n, k, kp, panels, st, op, p0, p1);
    else if (w <= 4) hipLaunchKernelGGL((block_vec_kernel<Op, 2>), grid, dim3(KT), 0, s, n, k, kp, panels, st, op, p0, p1);
    else if (w <= 8) hipLaunchKernelGGL((block_vec_kernel<Op, 4>), grid, dim3(KT), 0, s, n, k, kp, panels, st, op, p0, p1);
    else             hipLaunchKernelGGL((block_vec_kernel<Op, 8>), grid, dim3(KT), 0, s, n, k, kp, panels, st, op, p0, p1);
}

}  // namespace
}  // namespace spmvhip
