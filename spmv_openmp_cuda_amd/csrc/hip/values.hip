// values.hip -- the kernels that rewrite a private format's value array in place when the handle gets new values for the
// same pattern (spmvHipUpdateValues).  The formats (tiles.hip, stripes.hip, sell.hip) own their
// layouts and the maps into them; these kernels only move values.
//
// Locality.  Every format stores its entries in an order other than CSR order, so one side of the copy is a permutation.
// Which side, and in what order the work is dealt out, decides whether the permuted side stays in a cache:
//   * two-phase (tiles): the map is INDEXED BY CSR POSITION (where entry j sits in the slice-major `val`), and the kernel
//     walks AS in order -- reads stream.  Inside a tile the entries keep CSR order (the build's sort is stable), so a run of
//     rows writes every tile of its bin front to back: the writes of a stretch of CSR have one open line per slice
//     (c5: 610 slices, 78 KB), and the lines fill in L2 before they leave it.  Walked in storage order instead, every
//     entry of a slice would fetch a line of AS of its own (a row has 0.26 entries per slice on c5), once per slice.
//   * stripes: the map is INDEXED BY STORAGE POSITION (which CSR entry cell q holds, VMAP_NONE for a padding cell) and the
//     kernel walks the cells in order -- writes stream.  The cells of a bin are in COLUMN order, so its reads gather from
//     the bin's CSR range (c3: ~400 k entries, 3.2 MB) at random; written in CSR order the scattered side would be the
//     writes, and partial lines are worse than gathered ones.
//   * in both kernels a workgroup takes a CHUNK of consecutive positions, and the chunks are dealt to the 8 XCDs in
//     contiguous ranges (workgroups are placed round-robin over the XCDs: blocks b, b + 8, ... share one), so at any time
//     an XCD works on ONE stretch of the stream -- about one bin -- and the permuted side of the copy stays in its 4 MiB
//     L2 instead of 32 bins' worth competing for it (the same dealing as sell_spmv_kernel's).
//   * SELL needs no map: its slices hold whole rows, so the build's fill kernel is re-run without the column stream.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "spmvHip.h"
#include "device_mat.hpp"

namespace spmvhip {

namespace {

constexpr uint32_t VAL_THREADS = 256;
constexpr uint32_t VAL_PER_THREAD = 8;                        // positions per lane: a chunk is 2048 consecutive positions
constexpr uint32_t VAL_CHUNK = VAL_THREADS * VAL_PER_THREAD;

// chunk handled by this workgroup: workgroup q runs on XCD q % 8; XCD x takes the chunks [x * n / 8, (x + 1) * n / 8) in
// order (a bijection of [0, nChunks), like sell_spmv_kernel's)
__device__ __forceinline__ uint64_t val_chunk(uint64_t nChunks) {
    const uint64_t q = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const uint64_t a = nChunks / 8, rem = nChunks % 8, xcd = q % 8;
    return xcd * a + (xcd < rem ? xcd : rem) + q / 8;
}

// val[q] = AS[map[q]] (0.0 for a padding cell) for q in [0, n): writes stream, reads gather
__global__ __launch_bounds__(VAL_THREADS) void val_gather_kernel(uint64_t n, const uint32_t* __restrict__ map,
                                                                 const double* __restrict__ AS, double* __restrict__ val) {
    const uint64_t nChunks = (n + VAL_CHUNK - 1) / VAL_CHUNK;
    if ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x >= nChunks) return;
    const uint64_t base = val_chunk(nChunks) * VAL_CHUNK + threadIdx.x;
    uint32_t m[VAL_PER_THREAD];
#pragma unroll
    for (uint32_t u = 0; u < VAL_PER_THREAD; ++u) {
        const uint64_t q = base + (uint64_t)u * VAL_THREADS;
        m[u] = q < n ? __builtin_nontemporal_load(map + q) : VMAP_NONE;
    }
#pragma unroll
    for (uint32_t u = 0; u < VAL_PER_THREAD; ++u) {
        const uint64_t q = base + (uint64_t)u * VAL_THREADS;
        if (q < n) val[q] = m[u] != VMAP_NONE ? AS[m[u]] : 0.0;
    }
}

// val[map[j]] = AS[j] for j in [0, n): reads stream, writes scatter (map is a permutation of [0, n))
__global__ __launch_bounds__(VAL_THREADS) void val_scatter_kernel(uint64_t n, const uint32_t* __restrict__ map,
                                                                  const double* __restrict__ AS, double* __restrict__ val) {
    const uint64_t nChunks = (n + VAL_CHUNK - 1) / VAL_CHUNK;
    if ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x >= nChunks) return;
    const uint64_t base = val_chunk(nChunks) * VAL_CHUNK + threadIdx.x;
    uint32_t m[VAL_PER_THREAD];
    double v[VAL_PER_THREAD];
#pragma unroll
    for (uint32_t u = 0; u < VAL_PER_THREAD; ++u) {
        const uint64_t j = base + (uint64_t)u * VAL_THREADS;
        const uint64_t jc = j < n ? j : n - 1;               // clamped, not branched: the loads stay in one batch
        m[u] = __builtin_nontemporal_load(map + jc);
        v[u] = __builtin_nontemporal_load(AS + jc);
    }
#pragma unroll
    for (uint32_t u = 0; u < VAL_PER_THREAD; ++u)
        if (base + (uint64_t)u * VAL_THREADS < n) val[m[u]] = v[u];
}

// SELL: one wavefront per slice rewrites the slice's values from its rows (sell_fill_kernel without the column stream).
// perm holds the original row, 0xFFFFFFFF for a pad lane and the row with its top bit set for a row of the long-row path;
// both of those have slen = 0 and only store padding zeros.
template <typename I>
__global__ __launch_bounds__(256) void sell_values_kernel(uint32_t nSlices, const uint64_t* __restrict__ sliceOff,
                                                          const uint32_t* __restrict__ perm, const uint32_t* __restrict__ slen,
                                                          const I* __restrict__ IRP, const double* __restrict__ AS,
                                                          double* __restrict__ val) {
    const uint64_t s = ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + threadIdx.x / 64;
    if (s >= nSlices) return;
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t off = sliceOff[s];
    const uint32_t width = (uint32_t)((sliceOff[s + 1] - off) / 64);
    const uint32_t n = slen[s * 64 + lane];
    const uint64_t b = n ? (uint64_t)IRP[perm[s * 64 + lane]] : 0;     // (n > 0: a plain row id)
    for (uint32_t k = 0; k < width; ++k) val[off + (uint64_t)k * 64 + lane] = k < n ? AS[b + k] : 0.0;
}

}  // namespace

int enqueueGatherValues(double* val, const uint32_t* map, uint64_t n, const double* AS, hipStream_t stream) {
    if (!n) return EXIT_SUCCESS;
    hipLaunchKernelGGL(val_gather_kernel, grid2d((n + VAL_CHUNK - 1) / VAL_CHUNK, VAL_THREADS), dim3(VAL_THREADS), 0, stream, n, map, AS, val);
    return hipOk(hipGetLastError(), "val_gather_kernel") ? EXIT_SUCCESS : EXIT_FAILURE;
}

int enqueueScatterValues(double* val, const uint32_t* map, uint64_t n, const double* AS, hipStream_t stream) {
    if (!n) return EXIT_SUCCESS;
    hipLaunchKernelGGL(val_scatter_kernel, grid2d((n + VAL_CHUNK - 1) / VAL_CHUNK, VAL_THREADS), dim3(VAL_THREADS), 0, stream, n, map, AS, val);
    return hipOk(hipGetLastError(), "val_scatter_kernel") ? EXIT_SUCCESS : EXIT_FAILURE;
}

int enqueueSellValues(uint32_t nSlices, const uint64_t* sliceOff, const uint32_t* perm, const uint32_t* slen, const void* IRP,
                      int irpBytes, const double* AS, double* val, hipStream_t stream) {
    if (!nSlices) return EXIT_SUCCESS;
    const dim3 grid = grid2d(((uint64_t)nSlices + 3) / 4, 256);
    withIrp(IRP, irpBytes, [&](auto irp) { hipLaunchKernelGGL((sell_values_kernel<IrpT<decltype(irp)>>), grid, dim3(256), 0, stream, nSlices, sliceOff, perm, slen, irp, AS, val); });
    return hipOk(hipGetLastError(), "sell_values_kernel") ? EXIT_SUCCESS : EXIT_FAILURE;
}

}  // namespace spmvhip
