// transpose.hip -- A^T of a device CSR handle, built on the device as a CSR handle of its own (spmvHipCsrTranspose,
// DESIGN.md section 16), and the map that links its values back to the source (spmvHipTransposeRefresh).
//
// Order.  Row j of A^T holds the entries of column j of A in their CSR position order (ascending source row, and
// within a row the stored order): a STABLE sort of JA with the CSR position as payload gives exactly that, and the
// sorted payload is the map ASt[p] = AS[map[p]].  Then every row of A^T has non-decreasing column ids (source rows), so
// hipSpMVRowsCSR on the transpose gives the bits of the textbook scatter loop
//     y = +0.0;  for i: for p in row i: y[JA[p]] += AS[p] * x[i]
// on every candidate of its selection (DESIGN.md section 16 says why).
//
// Steps, all on the library stream, none with atomics (the arrays are the same on every run):
//   1. iota payload (in the room of ASt, which is written last)
//   2. the stable radix sort of JA over bits [0, ceil(log2 N)): keys into JAt (the room is free until step 5),
//      payload into the map
//   3. tr_bounds_kernel: IRPt from the sorted keys -- empty columns included, and the final NZ
//   4. tr_row_of_kernel: the source row of every CSR position (a 4 B/nnz temporary)
//   5. tr_place_kernel: JAt[p] = rowOf[map[p]], ASt[p] = AS[map[p]], chunks dealt to the XCDs in contiguous ranges
// Why a row-expansion array and not a search in IRP for step 5: a gather instruction costs a CU's L1 ~28 clocks whatever
// its addresses, and a binary search over M rows is ~log2(M) dependent gathers per entry (24 on
// c3); the expansion is one streamed write of 4 B/nnz and ONE more gather per entry, at the index AS is gathered at.
#include <hip/hip_runtime.h>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {

namespace {

constexpr uint32_t TR_THREADS = 256;
constexpr uint32_t TR_PER_THREAD = 8;                          // positions per lane: a chunk is 2048 consecutive positions
constexpr uint32_t TR_CHUNK = TR_THREADS * TR_PER_THREAD;
constexpr uint32_t TR_ROW_LANES = 16;                          // lanes per source row in tr_row_of_kernel

// the two kernels of device_prims.hpp
__global__ __launch_bounds__(TR_THREADS) void iota_kernel(uint64_t n, uint32_t* __restrict__ p) {
    const uint64_t i = linear_block() * TR_THREADS + threadIdx.x;
    if (i < n) p[i] = (uint32_t)i;
}
__global__ __launch_bounds__(TR_THREADS) void fill32_kernel(uint32_t* __restrict__ p, uint64_t n, uint32_t v) {
    const uint64_t i = linear_block() * TR_THREADS + threadIdx.x;
    if (i < n) p[i] = v;
}

// IRPt[c] = the first sorted position whose key is >= c.  Lane p (0 <= p <= nnz) writes the columns in
// (keys[p - 1], keys[p]] -- with keys[-1] = -1 and keys[nnz] = N -- so every c in [0, N] is written exactly once, runs of
// empty columns by the lane after them.  The clamp to N keeps a column id >= N (an adopted JA out of range) from
// writing past the array.
__global__ __launch_bounds__(TR_THREADS) void tr_bounds_kernel(uint64_t nnz, uint64_t N, const uint32_t* __restrict__ keys,
                                                               uint32_t* __restrict__ IRPt) {
    const uint64_t p = linear_block() * TR_THREADS + threadIdx.x;
    if (p > nnz) return;
    const uint64_t lo = p ? (uint64_t)keys[p - 1] + 1 : 0;
    const uint64_t k = p < nnz ? (uint64_t)keys[p] : N, hi = k < N ? k : N;
    for (uint64_t c = lo; c <= hi; ++c) IRPt[c] = (uint32_t)p;
}

// rowOf[j] = the source row of CSR position j: 16 lanes per row, 16 rows per workgroup (the ~20-entry rows of the
// power-law inputs would leave most of a wavefront idle; a long row is walked 16 entries a step)
template <typename I>
__global__ __launch_bounds__(TR_THREADS) void tr_row_of_kernel(uint64_t M, const I* __restrict__ IRP, uint32_t* __restrict__ rowOf) {
    const uint64_t r = linear_block() * (TR_THREADS / TR_ROW_LANES) + threadIdx.x / TR_ROW_LANES;
    if (r >= M) return;
    const uint64_t e = IRP[r + 1];
    for (uint64_t j = (uint64_t)IRP[r] + threadIdx.x % TR_ROW_LANES; j < e; j += TR_ROW_LANES) rowOf[j] = (uint32_t)r;
}

// chunk handled by this workgroup: workgroup q runs on XCD q % 8; XCD x takes the chunks [x * n / 8, (x + 1) * n / 8)
// in order (a bijection of [0, nChunks), as val_gather_kernel deals them), so an XCD gathers from one stretch of rows
__device__ __forceinline__ uint64_t tr_chunk(uint64_t nChunks) {
    const uint64_t q = linear_block();
    const uint64_t a = nChunks / 8, rem = nChunks % 8, xcd = q % 8;
    return xcd * a + (xcd < rem ? xcd : rem) + q / 8;
}

// JAt[p] = rowOf[map[p]], ASt[p] = AS[map[p]]: the map and both outputs stream, the two reads gather at one index
__global__ __launch_bounds__(TR_THREADS) void tr_place_kernel(uint64_t n, const uint32_t* __restrict__ map,
                                                              const uint32_t* __restrict__ rowOf, const double* __restrict__ AS,
                                                              uint32_t* __restrict__ JAt, double* __restrict__ ASt) {
    const uint64_t nChunks = (n + TR_CHUNK - 1) / TR_CHUNK;
    if (linear_block() >= nChunks) return;
    const uint64_t base = tr_chunk(nChunks) * TR_CHUNK + threadIdx.x;
    uint32_t m[TR_PER_THREAD], r[TR_PER_THREAD];
    double v[TR_PER_THREAD];
#pragma unroll
    for (uint32_t u = 0; u < TR_PER_THREAD; ++u) {
        const uint64_t q = base + (uint64_t)u * TR_THREADS;
        m[u] = __builtin_nontemporal_load(map + (q < n ? q : n - 1));      // clamped, not branched: one batch of loads
    }
#pragma unroll
    for (uint32_t u = 0; u < TR_PER_THREAD; ++u) {
        r[u] = rowOf[m[u]];
        v[u] = AS[m[u]];
    }
#pragma unroll
    for (uint32_t u = 0; u < TR_PER_THREAD; ++u) {
        const uint64_t q = base + (uint64_t)u * TR_THREADS;
        if (q < n) { JAt[q] = r[u]; ASt[q] = v[u]; }
    }
}

}  // namespace

void enqueueIota(uint64_t n, uint32_t* p, hipStream_t st) {
    hipLaunchKernelGGL(iota_kernel, gridFor(n, TR_THREADS, TR_THREADS), dim3(TR_THREADS), 0, st, n, p);
}

void enqueueFill32(uint32_t* p, uint64_t n, uint32_t v, hipStream_t st) {
    hipLaunchKernelGGL(fill32_kernel, gridFor(n, TR_THREADS, TR_THREADS), dim3(TR_THREADS), 0, st, p, n, v);
}

void enqueueSortedBounds(uint64_t nnz, uint64_t N, const uint32_t* keys, uint32_t* ptr, hipStream_t st) {
    hipLaunchKernelGGL(tr_bounds_kernel, grid2d((nnz + 1 + TR_THREADS - 1) / TR_THREADS, TR_THREADS), dim3(TR_THREADS), 0, st,
                       nnz, N, keys, ptr);
}

// The pattern sorted by column: the stable sort of (keys, payload) over the low `bits` key bits into (keysOut,
// payloadOut), then ptr[0 .. N] from the sorted keys.  Payload = the row of every position: the transposed pattern (the
// dependents of a triangular analysis, the incoming side of a colouring); = an iota: the transpose's value map.  The
// pointers are not const: rocPRIM's kernels are instantiated on the iterator types, and every caller holds plain ones.
hipError_t enqueueSortedByColumn(uint64_t nnz, uint64_t N, unsigned bits, uint32_t* keys, uint32_t* payload, uint32_t* keysOut,
                                 uint32_t* payloadOut, uint32_t* ptr, TempBuf& ws, hipStream_t st) {
    if (nnz) {
        const hipError_t e = sortPairs(ws, keys, keysOut, payload, payloadOut, (size_t)nnz, 0u, bits, st);
        if (e != hipSuccess) return e;
    }
    enqueueSortedBounds(nnz, N, keysOut, ptr, st);
    return hipSuccess;
}

void enqueueRowOf(uint64_t M, const void* IRP, int irpBytes, uint32_t* rowOf, hipStream_t st) {
    if (!M) return;
    const dim3 rows = grid2d((M + TR_THREADS / TR_ROW_LANES - 1) / (TR_THREADS / TR_ROW_LANES), TR_THREADS);
    withIrp(IRP, irpBytes, [&](auto irp) { hipLaunchKernelGGL((tr_row_of_kernel<IrpT<decltype(irp)>>), rows, dim3(TR_THREADS), 0, st, M, irp, rowOf); });
}

int transposeCsr(const DevMat* a, DevMat* t, hipStream_t st) {
    const uint64_t nnz = a->NZ, M = a->M, N = a->N;
    uint32_t* const IRPt = static_cast<uint32_t*>(t->IRP);
    TempBuf rowOf, sortTmp;
    auto fail = [&](const char* what) { return buildFail(st, "transpose", what); };
    uint32_t* const iota = reinterpret_cast<uint32_t*>(t->AS);
    if (nnz) {
        if (rowOf.alloc(nnz * 4)) return fail("temporary allocation (4 B per entry)");
        enqueueIota(nnz, iota, st);
    }
    if (enqueueSortedByColumn(nnz, N, bitsFor(N), a->JA, iota, t->JA, t->tmap, IRPt, sortTmp, st) != hipSuccess) return fail("sort");
    if (nnz) {
        enqueueRowOf(M, a->IRP, a->irpBytes, rowOf.as<uint32_t>(), st);
        hipLaunchKernelGGL(tr_place_kernel, grid2d((nnz + TR_CHUNK - 1) / TR_CHUNK, TR_THREADS), dim3(TR_THREADS), 0, st,
                           nnz, t->tmap, rowOf.as<uint32_t>(), a->AS, t->JA, t->AS);
    }
    if (hipGetLastError() != hipSuccess) return fail("kernels");
    if (hipStreamSynchronize(st) != hipSuccess) return fail("synchronise");
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
