// spmm.hip -- Y = A X for a block of k vectors (hipSpMMRowsCSR).
//
// Every column of Y has the bits of sgemvSerial on the matching column of X: each row's products are rounded and added in
// the handle's STORED entry order (the library is compiled with -ffp-contract=off), whatever the row's columns are.
//
// The kernel walks the handle's row-block table (blkInfo / blkBase, the blocks of csr_stream2_kernel) once per PANEL of at
// most 16 columns, so the matrix is streamed once per panel instead of once per vector, and one gathered row of X carries
// up to 16 useful doubles (a whole 128-B line at k >= 16 with row-major X) instead of 8 bytes of one.
//   * short-row blocks (<= 2048 entries, <= 512 rows): the block's JA / AS span and its row offsets are staged in LDS with
//     coalesced non-temporal loads, as csr_stream2_kernel does.  Then a group of P lanes (P = the panel width rounded up to
//     a power of two) owns a row: lane c walks the row in stored order, SPMM_AHEAD entries' gathers in flight and the adds
//     kept in order.  Consecutive lanes read consecutive doubles of one X row, so a 64-lane gather covers 64/P entries.
//   * long-row blocks (one row of more than 2048 entries): the workgroup computes a chunk's products in parallel into LDS
//     ([entry][P], 16 KiB), then lane c of the first wavefront adds its column in stored order.
// Layouts are element strides (X(j, c) at X[j*sxr + c*sxc]): row-major is sxr = ld, sxc = 1; column-major sxr = 1,
// sxc = ld, which gathers P separate lines per entry (correct, not tuned).
#include <hip/hip_runtime.h>

#include "spmvHip.h"
#include "kernels.hpp"

namespace spmvhip {

namespace {

constexpr uint32_t SPMM_PANEL = 16;               // columns per panel: the matrix is streamed once per panel
constexpr uint32_t SPMM_AHEAD = 8;                // gathers in flight per lane on a short row
constexpr int      SPMM_LONG_PER = STREAM_NNZ / WG_THREADS;   // products per lane and long-row chunk (8: 16 KiB in all)

// V: the type the value stream is stored in (double, or float for the handle's single-precision form, widened at the load:
// the LDS copy of the span and everything after it are the same for both)
template <typename I, int P, bool UNIT, typename V = double>
__global__ __launch_bounds__(WG_THREADS) void csr_spmm_kernel(
    uint32_t nBlk, uint32_t nLong, const uint4* __restrict__ blkInfo, const uint64_t* __restrict__ blkBase,
    const I* __restrict__ IRP, const uint32_t* __restrict__ JA, const V* __restrict__ AS, double unitValue,
    uint32_t w, const double* __restrict__ X, uint64_t sxr, uint64_t sxc, double* __restrict__ Y, uint64_t syr, uint64_t syc) {
    static_assert(P >= 1 && P <= (int)SPMM_PANEL && (P & (P - 1)) == 0 && WG_THREADS % P == 0, "panel width");
    // short-row blocks: AS span in [0, STREAM_NNZ), the JA span as u32 behind it; long rows: the products of a chunk
    __shared__ double   smem[STREAM_NNZ + STREAM_NNZ / 2];
    __shared__ uint16_t rowOff[STREAM2_MAX_ROWS + 1];

    const uint32_t tid = threadIdx.x;
    if (linear_block() >= nBlk) return;
    const uint64_t blk = stream2_block(linear_block(), nBlk, nLong);
    const uint4 info = blkInfo[blk];
    const uint32_t r0 = info.x, R = info.y, n = info.z;
    const uint64_t base = blkBase[blk];
    const uint32_t c = tid % P;                       // this lane's column of the panel
    const bool live = c < w;                          // lanes past the panel's width read and write nothing
    const double* __restrict__ Xc = X + c * sxc;

    if (info.w) {
        // ---- long row: chunks of E entries; product q = tid + i*256 is entry q / P, column q % P = c
        constexpr uint32_t E = SPMM_LONG_PER * WG_THREADS / P;
        const uint64_t end = base + n;
        double acc = 0;
        for (uint64_t ch = base; ch < end; ch += E) {
            const uint32_t cn = (uint32_t)(end - ch < (uint64_t)E ? end - ch : (uint64_t)E);
            uint32_t col[SPMM_LONG_PER];
            double   av[SPMM_LONG_PER], xv[SPMM_LONG_PER];
#pragma unroll
            for (int i = 0; i < SPMM_LONG_PER; ++i) {
                const uint32_t e = (tid + i * WG_THREADS) / P;
                const bool in = live && e < cn;
                col[i] = in ? stream_load(JA + ch + e) : 0u;
                av[i] = in ? value_at<UNIT>(AS, ch + e, unitValue) : 0.0;
            }
#pragma unroll
            for (int i = 0; i < SPMM_LONG_PER; ++i) {
                const uint32_t e = (tid + i * WG_THREADS) / P;
                xv[i] = live && e < cn ? Xc[col[i] * sxr] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < SPMM_LONG_PER; ++i)
                if (live && (tid + i * WG_THREADS) / P < cn) smem[tid + i * WG_THREADS] = av[i] * xv[i];
            __syncthreads();
            if (tid < w)
                for (uint32_t e = 0; e < cn; ++e) acc += smem[e * P + tid];
            __syncthreads();
        }
        if (tid < w) Y[(uint64_t)r0 * syr + tid * syc] = acc;
        return;
    }

    // ---- short rows: 1. span + row pointers into LDS
    double* sAS = smem;
    uint32_t* sJA = reinterpret_cast<uint32_t*>(smem + STREAM_NNZ);
    {
        uint32_t col[STREAM_UNROLL];
        double   val[STREAM_UNROLL];
#pragma unroll
        for (int u = 0; u < STREAM_UNROLL; ++u) {
            const uint32_t k = tid + u * WG_THREADS;
            col[u] = k < n ? stream_load(JA + base + k) : 0u;
            if (!UNIT) val[u] = k < n ? (double)stream_load(AS + base + k) : 0.0;
        }
        uint32_t rp0 = 0, rp1 = 0;
        if (tid < R) rp0 = (uint32_t)((uint64_t)IRP[r0 + tid] - base);
        if (tid + WG_THREADS < R) rp1 = (uint32_t)((uint64_t)IRP[r0 + tid + WG_THREADS] - base);
#pragma unroll
        for (int u = 0; u < STREAM_UNROLL; ++u) {
            const uint32_t k = tid + u * WG_THREADS;
            if (k < n) {
                sJA[k] = col[u];
                if (!UNIT) sAS[k] = val[u];
            }
        }
        if (tid < R) rowOff[tid] = (uint16_t)rp0;
        if (tid + WG_THREADS < R) rowOff[tid + WG_THREADS] = (uint16_t)rp1;
        if (tid == 0) rowOff[R] = (uint16_t)n;
    }
    __syncthreads();
    if (!live) return;

    // ---- 2. group g of P lanes per row; lane c adds column c of its row in stored order
    for (uint32_t rr = tid / P; rr < R; rr += WG_THREADS / P) {
        const uint32_t s = rowOff[rr], e = rowOff[rr + 1];
        double acc = 0;
        for (uint32_t j = s; j < e; j += SPMM_AHEAD) {
            double xv[SPMM_AHEAD], av[SPMM_AHEAD];
#pragma unroll
            for (uint32_t u = 0; u < SPMM_AHEAD; ++u) {
                const bool in = j + u < e;
                xv[u] = in ? Xc[sJA[j + u] * sxr] : 0.0;
                av[u] = UNIT ? unitValue : (in ? sAS[j + u] : 0.0);
            }
#pragma unroll
            for (uint32_t u = 0; u < SPMM_AHEAD; ++u)
                if (j + u < e) acc += av[u] * xv[u];
        }
        Y[(uint64_t)(r0 + rr) * syr + c * syc] = acc;
    }
}

// AS / unitValue: the handle's double stream and unit value, or those of its single-precision form
template <int P, bool UNIT, typename V>
void launchPanel(const DevMat* d, const V* AS, double unitValue, uint32_t w, const double* X, uint64_t sxr, uint64_t sxc, double* Y,
                 uint64_t syr, uint64_t syc, hipStream_t stream) {
    const dim3 grid = grid2d(d->nBlk2, WG_THREADS), block(WG_THREADS);
    withIrp(d, [&](auto irp) {
        hipLaunchKernelGGL((csr_spmm_kernel<IrpT<decltype(irp)>, P, UNIT, V>), grid, block, 0, stream, d->nBlk2, d->nLong2, d->blkInfo,
                           d->blkBase, irp, d->JA, AS, unitValue, w, X, sxr, sxc, Y, syr, syc);
    });
}

template <bool UNIT, typename V>
void launchPanelP(const DevMat* d, const V* AS, double unitValue, uint32_t w, const double* X, uint64_t sxr, uint64_t sxc, double* Y,
                  uint64_t syr, uint64_t syc, hipStream_t stream) {
    if (w == 1)      launchPanel<1, UNIT>(d, AS, unitValue, w, X, sxr, sxc, Y, syr, syc, stream);
    else if (w == 2) launchPanel<2, UNIT>(d, AS, unitValue, w, X, sxr, sxc, Y, syr, syc, stream);
    else if (w <= 4) launchPanel<4, UNIT>(d, AS, unitValue, w, X, sxr, sxc, Y, syr, syc, stream);
    else if (w <= 8) launchPanel<8, UNIT>(d, AS, unitValue, w, X, sxr, sxc, Y, syr, syc, stream);
    else             launchPanel<16, UNIT>(d, AS, unitValue, w, X, sxr, sxc, Y, syr, syc, stream);
}

}  // namespace

// one launch per panel of at most 16 columns, in column order, on `stream`; the caller has checked the arguments (f32: and
// that the handle's single-precision form is built, which then is what the panels stream)
int enqueueSpmm(const DevMat* d, uint32_t k, const Dense& X, const Dense& Y, hipStream_t stream, bool f32) {
    const uint64_t sxr = X.sr(), sxc = X.sc(), syr = Y.sr(), syc = Y.sc();
    for (uint32_t c0 = 0; c0 < k; c0 += SPMM_PANEL) {
        const uint32_t w = k - c0 < SPMM_PANEL ? k - c0 : SPMM_PANEL;
        const double* Xp = X.p + (uint64_t)c0 * sxc;
        double* Yp = Y.p + (uint64_t)c0 * syc;
        if (d->unit)  launchPanelP<true>(d, d->AS, f32 ? d->unitValue32 : d->unitValue, w, Xp, sxr, sxc, Yp, syr, syc, stream);
        else if (f32) launchPanelP<false>(d, d->AS32, 0.0, w, Xp, sxr, sxc, Yp, syr, syc, stream);
        else          launchPanelP<false>(d, d->AS, d->unitValue, w, Xp, sxr, sxc, Yp, syr, syc, stream);
    }
    HIP_TRY(hipGetLastError());
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
