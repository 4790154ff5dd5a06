// colour.hip -- a multi-colour ordering of a square device CSR handle (spmvHipColourCSR), the symmetric permutation
// B = P A P^T as a CSR handle of its own (spmvHipCsrPermute) and the permutation of a vector (spmvHipVecPermute).
// DESIGN.md section 21; the contracts are in spmvHip.h.
//
// Colouring.  colour[i] = the smallest colour that no neighbour WINNING against i has, neighbours taken in the pattern of
// A + A^T.  "Winning" is a fixed total order of the vertices (the natural order, or a hash of the id), so the colours are a
// function of the pattern and the options alone.  Jones-Plassmann rounds, one launch per round over the rows still
// uncoloured: a row whose winning neighbours are all coloured takes its first-fit colour, any other row waits for a later
// round.  Inside one launch a lane may see a neighbour's colour word as "uncoloured" or as its final value: it then waits,
// or uses a value that never changes again.  Only the NUMBER of rounds depends on that race, never a colour.  No spin, no
// flag, no ticket: a row never waits inside a kernel.
//   1. the incoming side of the adjacency = the pattern transposed: the stable radix sort of JA with the source row as
//      payload, row bounds from the sorted keys (transpose.hip's kernels; keys only, no values).  Skipped when a check of
//      the stored pattern finds it structurally symmetric (tried when no row has more than 64 entries).
//   2. rows with more than 64 adjacency entries (stored + incoming) go to the long list, one wavefront each; the others to
//      the short list, one lane each.
//   3. K rounds are enqueued, then the K + 1 list counts of the batch are read back (one small state, as the Krylov loops
//      do).  Every round compacts: it reads its list and writes the rows that wait into the other one.
//   4. dPerm: a stable radix sort of the colours over an iota = the rows by (colour, id).
//
// Permutation.  One stable sort of the keys (new row << bits | new column) with the source CSR position as payload gives the
// entries of B in their order -- rows ascending, within a row ascending new column, repeated columns in A's stored order --
// and the payload is the source-position map.  Then the row pointers from the sorted keys and a gather of the values.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <vector>

#include "spmvHip.h"
#include "kernels.hpp"
#include "device_prims.hpp"

namespace spmvhip {

namespace {

constexpr uint32_t CL_THREADS = WG_THREADS;                    // (what gridFor deals to by default)
constexpr uint32_t CL_WAVES = CL_THREADS / 64;
constexpr uint32_t UNCOLOURED = 0xFFFFFFFFu;
constexpr uint32_t CL_LONG = 64;                               // adjacency entries above which a row takes a wavefront

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {      // the murmur3 32-bit finaliser
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// does j win against i (j != i)?  NATURAL: the smaller index.  HASH: the larger pair (fmix32(id ^ seed), id).
__device__ __forceinline__ bool wins(uint32_t j, uint32_t i, int order, uint32_t seed) {
    if (order == SPMV_COLOUR_NATURAL) return j < i;
    const uint32_t kj = fmix32(j ^ seed), ki = fmix32(i ^ seed);
    return kj != ki ? kj > ki : j > i;
}

// 1 in *flag unless every stored (i, j), j != i, has a stored (j, i): one lane per entry scans row j (rows of at most 64
// entries: the caller does not try otherwise).  A column id >= M has no row to look in: not symmetric.
template <typename I>
__global__ __launch_bounds__(CL_THREADS) void cl_symmetric_kernel(uint64_t nnz, uint64_t M, const I* __restrict__ IRP,
                                                                  const uint32_t* __restrict__ JA, const uint32_t* __restrict__ rowOf,
                                                                  uint32_t* __restrict__ flag) {
    const uint64_t p = linear_block() * CL_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const uint32_t i = rowOf[p], j = JA[p];
    if (j == i) return;
    bool found = false;
    if (j < M)
        for (uint64_t q = IRP[j], e = IRP[j + 1]; q < e && !found; ++q) found = JA[q] == i;
    if (!found) atomicOr(flag, 1u);
}

// every row gets UNCOLOURED and joins the short or the long list: a wavefront takes its places with one atomic per list,
// so the ORDER of a list depends on the run -- which no colour does
template <typename I>
__global__ __launch_bounds__(CL_THREADS) void cl_classify_kernel(uint64_t M, const I* __restrict__ IRP, const uint32_t* __restrict__ tptr,
                                                                 uint32_t* __restrict__ colour, uint32_t* __restrict__ shortList,
                                                                 uint32_t* __restrict__ longList, uint32_t* __restrict__ cnt) {
    const uint64_t r = linear_block() * CL_THREADS + threadIdx.x;
    const bool live = r < M;
    uint64_t deg = 0;
    if (live) {
        colour[r] = UNCOLOURED;
        deg = (uint64_t)IRP[r + 1] - (uint64_t)IRP[r] + (tptr ? tptr[r + 1] - tptr[r] : 0u);
    }
    const bool isLong = live && deg > CL_LONG, isShort = live && !isLong;
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t below = (1ull << lane) - 1;
    const uint64_t bs = __ballot(isShort), bl = __ballot(isLong);
    uint32_t baseS = 0, baseL = 0;
    if (lane == 0) {
        if (bs) baseS = atomicAdd(&cnt[0], (uint32_t)__popcll(bs));
        if (bl) baseL = atomicAdd(&cnt[1], (uint32_t)__popcll(bl));
    }
    baseS = __shfl(baseS, 0);
    baseL = __shfl(baseL, 0);
    if (isShort) shortList[baseS + __popcll(bs & below)] = (uint32_t)r;
    if (isLong) longList[baseL + __popcll(bl & below)] = (uint32_t)r;
}

// The decision of one row, by `width` lanes (1, or the 64 of a wavefront) that share the adjacency stride `width` apart.
// A colour word is an aligned 32-bit load: UNCOLOURED or the final value.  Pass 0 reads every neighbour's word once and
// decides "ready" (all winning neighbours coloured) together with the mask of the colours 0..63; only a ready row walks
// further windows of 64 colours, and what it reads again there is final, so the same value.  Returns UNCOLOURED when the
// row has to wait.  Column ids >= M (an adopted array out of range) are no vertices and are skipped.
template <typename I, bool WAVE_ROW>
__device__ __forceinline__ uint32_t cl_decide(uint32_t i, uint32_t lane, uint64_t M, const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                              const uint32_t* __restrict__ tptr, const uint32_t* __restrict__ tcol,
                                              const uint32_t* colour, int order, uint32_t seed) {
    constexpr uint32_t width = WAVE_ROW ? 64 : 1;
    const uint64_t b0 = IRP[i], e0 = IRP[i + 1];
    const uint64_t b1 = tptr ? tptr[i] : 0, e1 = tptr ? tptr[i + 1] : 0;
    for (uint32_t base = 0;; base += 64) {
        uint64_t mask = 0;
        bool wait = false;
        for (int side = 0; side < 2; ++side) {
            const uint32_t* adj = side ? tcol : JA;
            for (uint64_t p = (side ? b1 : b0) + lane, e = side ? e1 : e0; p < e; p += width) {
                const uint32_t j = adj[p];
                if (j == i || j >= M || !wins(j, i, order, seed)) continue;
                const uint32_t c = __atomic_load_n(colour + j, __ATOMIC_RELAXED);
                if (c == UNCOLOURED) wait = true;
                else if (c - base < 64u) mask |= 1ull << (c - base);
            }
        }
        if (WAVE_ROW) {
            if (__ballot(wait)) return UNCOLOURED;
            for (int off = 32; off; off >>= 1) {
                const uint32_t lo = __shfl_xor((uint32_t)mask, off), hi = __shfl_xor((uint32_t)(mask >> 32), off);
                mask |= (uint64_t)hi << 32 | lo;
            }
        } else if (wait) {
            return UNCOLOURED;
        }
        if (~mask) return base + (uint32_t)__ffsll((long long)~mask) - 1;
        if (base >= 0xFFFFFF00u) return UNCOLOURED;            // (never: a row has fewer than 2^32 neighbours)
    }
}

// one round over the short list: in[0 .. *nIn) -> the rows that wait go to out[0 .. *nOut).  grid covers the count the
// host last read, which *nIn never exceeds.
template <typename I>
__global__ __launch_bounds__(CL_THREADS) void cl_round_short_kernel(uint64_t M, const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                                                    const uint32_t* __restrict__ tptr, const uint32_t* __restrict__ tcol,
                                                                    uint32_t* colour, int order, uint32_t seed, const uint32_t* __restrict__ in,
                                                                    const uint32_t* __restrict__ nIn, uint32_t* __restrict__ out,
                                                                    uint32_t* __restrict__ nOut, uint32_t* __restrict__ maxColour) {
    const uint64_t k = linear_block() * CL_THREADS + threadIdx.x;
    const bool live = k < *nIn;
    bool waits = false;
    uint32_t i = 0;
    if (live) {
        i = in[k];
        const uint32_t c = cl_decide<I, false>(i, 0, M, IRP, JA, tptr, tcol, colour, order, seed);
        waits = c == UNCOLOURED;
        if (!waits) {
            __atomic_store_n(colour + i, c, __ATOMIC_RELAXED);
            atomicMax(maxColour, c);
        }
    }
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t bw = __ballot(waits);
    uint32_t base = 0;
    if (lane == 0 && bw) base = atomicAdd(nOut, (uint32_t)__popcll(bw));
    base = __shfl(base, 0);
    if (waits) out[base + __popcll(bw & ((1ull << lane) - 1))] = i;
}

// ... over the long list, one wavefront per row
template <typename I>
__global__ __launch_bounds__(CL_THREADS) void cl_round_long_kernel(uint64_t M, const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                                                   const uint32_t* __restrict__ tptr, const uint32_t* __restrict__ tcol,
                                                                   uint32_t* colour, int order, uint32_t seed, const uint32_t* __restrict__ in,
                                                                   const uint32_t* __restrict__ nIn, uint32_t* __restrict__ out,
                                                                   uint32_t* __restrict__ nOut, uint32_t* __restrict__ maxColour) {
    const uint64_t k = linear_block() * CL_WAVES + threadIdx.x / 64;
    if (k >= *nIn) return;                                     // uniform in a wavefront
    const uint32_t lane = threadIdx.x % 64, i = in[k];
    const uint32_t c = cl_decide<I, true>(i, lane, M, IRP, JA, tptr, tcol, colour, order, seed);
    if (lane) return;
    if (c == UNCOLOURED) { out[atomicAdd(nOut, 1u)] = i; return; }
    __atomic_store_n(colour + i, c, __ATOMIC_RELAXED);
    atomicMax(maxColour, c);
}

// inv[perm[r]] = r with inv preset to UNCOLOURED words; *flag |= 1 for a value >= M, |= 2 for a repeated one
__global__ __launch_bounds__(CL_THREADS) void pm_invert_kernel(uint64_t M, const uint32_t* __restrict__ perm, uint32_t* __restrict__ inv,
                                                               uint32_t* __restrict__ flag) {
    const uint64_t r = linear_block() * CL_THREADS + threadIdx.x;
    if (r >= M) return;
    const uint32_t v = perm[r];
    if (v >= M) { atomicOr(flag, 1u); return; }
    if (atomicExch(inv + v, (uint32_t)r) != UNCOLOURED) atomicOr(flag, 2u);
}

// key[p] = inv[row of p] << bits | inv[JA[p]]; a column id >= M has no new id: *flag = 1 and the key stays in range
__global__ __launch_bounds__(CL_THREADS) void pm_keys_kernel(uint64_t nnz, uint64_t M, unsigned bits, const uint32_t* __restrict__ rowOf,
                                                             const uint32_t* __restrict__ JA, const uint32_t* __restrict__ inv,
                                                             uint64_t* __restrict__ key, uint32_t* __restrict__ flag) {
    const uint64_t p = linear_block() * CL_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const uint32_t j = JA[p];
    if (j >= M) atomicOr(flag, 1u);
    key[p] = (uint64_t)inv[rowOf[p]] << bits | (j < M ? inv[j] : 0u);
}

// the sorted keys taken apart: the new row (for the row pointers) and the new column
__global__ __launch_bounds__(CL_THREADS) void pm_split_kernel(uint64_t nnz, unsigned bits, const uint64_t* __restrict__ key,
                                                              uint32_t* __restrict__ row, uint32_t* __restrict__ col) {
    const uint64_t p = linear_block() * CL_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const uint64_t k = key[p];
    row[p] = (uint32_t)(k >> bits);
    col[p] = (uint32_t)(k & ((1ull << bits) - 1));
}

// forward: out[r] = in[perm[r]]; inverse: out[perm[r]] = in[r].  Bits are copied.  A perm value >= n is skipped.
__global__ __launch_bounds__(CL_THREADS) void vec_permute_kernel(uint64_t n, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ in,
                                                                 uint64_t* __restrict__ out, int inverse) {
    const uint64_t r = linear_block() * CL_THREADS + threadIdx.x;
    if (r >= n) return;
    const uint32_t v = perm[r];
    if (v >= n) return;
    if (inverse) out[v] = in[r];
    else         out[r] = in[v];
}

}  // namespace

int enqueueVecPermute(uint64_t n, const uint32_t* perm, const double* in, double* out, int inverse, hipStream_t st) {
    if (!n) return EXIT_SUCCESS;
    hipLaunchKernelGGL(vec_permute_kernel, gridFor(n), dim3(CL_THREADS), 0, st, n, perm, reinterpret_cast<const uint64_t*>(in),
                       reinterpret_cast<uint64_t*>(out), inverse);
    return hipGetLastError() == hipSuccess ? EXIT_SUCCESS : EXIT_FAILURE;
}

// inv (M words, the caller's) = the inverse of perm; *bad = 0 a permutation, bit 0 a value >= M, bit 1 a repeated value
int invertPerm(uint64_t M, const uint32_t* perm, uint32_t* inv, uint32_t* bad, hipStream_t st) {
    *bad = 0;
    if (!M) return EXIT_SUCCESS;
    HIP_TRY(hipMemsetAsync(inv, 0xFF, M * 4, st));
    return deviceFlag(0, st, "pm_invert_kernel", bad, [&](uint32_t* dFlag) {
        hipLaunchKernelGGL(pm_invert_kernel, gridFor(M), dim3(CL_THREADS), 0, st, M, perm, inv, dFlag);
    });
}

int permuteCsr(const DevMat* a, const uint32_t* inv, DevMat* t, hipStream_t st) {
    const uint64_t nnz = a->NZ, M = a->M;
    uint32_t* const IRPt = static_cast<uint32_t*>(t->IRP);
    TempBuf rowOf, keyIn, keyOut, sortTmp;
    auto fail = [&](const char* what) { return buildFail(st, "permute", what); };
    const unsigned bits = bitsFor(M);
    if (nnz) {
        if (rowOf.alloc(nnz * 4) || keyIn.alloc(nnz * 8) || keyOut.alloc(nnz * 8)) return fail("temporary allocation (20 B per entry)");
        uint32_t* const iota = reinterpret_cast<uint32_t*>(t->AS);                  // (the room of the values, written last)
        enqueueIota(nnz, iota, st);
        enqueueRowOf(M, a->IRP, a->irpBytes, rowOf.as<uint32_t>(), st);
        uint32_t outOfRange = 0;
        if (deviceFlag(0, st, "pm_keys_kernel", &outOfRange, [&](uint32_t* dFlag) {
                hipLaunchKernelGGL(pm_keys_kernel, gridFor(nnz), dim3(CL_THREADS), 0, st, nnz, M, bits, rowOf.as<uint32_t>(), a->JA, inv,
                                   keyIn.as<uint64_t>(), dFlag);
            }))
            return fail("keys");
        if (outOfRange) { fprintf(stderr, "libspmvhip: permute: a column id of the source is >= M\n"); return EXIT_FAILURE; }
        if (sortPairs(sortTmp, keyIn.as<uint64_t>(), keyOut.as<uint64_t>(), iota, t->tmap, (size_t)nnz, 0u, 2 * bits, st) != hipSuccess)
            return fail("sort");
        hipLaunchKernelGGL(pm_split_kernel, gridFor(nnz), dim3(CL_THREADS), 0, st, nnz, bits, keyOut.as<uint64_t>(), rowOf.as<uint32_t>(), t->JA);
    }
    enqueueSortedBounds(nnz, M, rowOf.as<uint32_t>(), IRPt, st);
    if (nnz && enqueueGatherValues(t->AS, t->tmap, nnz, a->AS, st)) return fail("value gather");
    if (hipGetLastError() != hipSuccess) return fail("kernels");
    if (hipStreamSynchronize(st) != hipSuccess) return fail("synchronise");
    return EXIT_SUCCESS;
}

int buildIncoming(const DevMat* a, IncomingPattern& in, hipStream_t st, const char* module) {
    const uint64_t nnz = a->NZ, M = a->M;
    auto fail = [&](const char* what) { return buildFail(st, module, what); };
    if (!nnz) return EXIT_SUCCESS;
    if (in.rowOf.alloc(nnz * 4)) return fail("temporary allocation (4 B per entry)");
    enqueueRowOf(M, a->IRP, a->irpBytes, in.rowOf.as<uint32_t>(), st);
    uint32_t asym = 1;
    if (a->maxRowNnz <= CL_LONG &&
        deviceFlag(0, st, "cl_symmetric_kernel", &asym, [&](uint32_t* dFlag) {
            withIrp(a, [&](auto irp) {
                hipLaunchKernelGGL((cl_symmetric_kernel<IrpT<decltype(irp)>>), gridFor(nnz), dim3(CL_THREADS), 0, st, nnz, M, irp, a->JA,
                                   in.rowOf.as<uint32_t>(), dFlag);
            });
        }))
        return fail("symmetry check");
    in.symmetric = asym ? 0 : 1;
    if (!asym) return EXIT_SUCCESS;
    if (in.keys.alloc(nnz * 4) || in.colBuf.alloc(nnz * 4) || in.ptrBuf.alloc((M + 1) * 4)) return fail("temporary allocation (transposed pattern)");
    // (preset: with column ids >= N the sort leaves keys out of order and the bounds kernel words unwritten)
    if (hipMemsetAsync(in.ptrBuf.p, 0, (M + 1) * 4, st) != hipSuccess) return fail("transposed pattern");
    if (enqueueSortedByColumn(nnz, M, bitsFor(a->N), a->JA, in.rowOf.as<uint32_t>(), in.keys.as<uint32_t>(), in.colBuf.as<uint32_t>(),
                              in.ptrBuf.as<uint32_t>(), in.sortTmp, st) != hipSuccess)
        return fail("sort");
    in.ptr = in.ptrBuf.as<uint32_t>();
    in.col = in.colBuf.as<uint32_t>();
    return EXIT_SUCCESS;
}

int colourCsr(const DevMat* a, int order, uint32_t seed, uint32_t K, uint32_t* dColour, uint32_t* dPerm, spmvColourInfo* info,
              hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t M = a->M;
    spmvColourInfo out{};
    out.symmetric = 1;                                         // (no entry: nothing comes in from the transposed side)
    auto fail = [&](const char* what) { return buildFail(st, "colour", what); };
    if (M == 0) { if (info) *info = out; return EXIT_SUCCESS; }
    TempBuf colourBuf, lists, state, iotaBuf, sortedBuf, permBuf;
    // 1. the incoming side
    IncomingPattern in;
    if (buildIncoming(a, in, st, "colour")) return EXIT_FAILURE;
    out.symmetric = in.symmetric;
    const uint32_t *tptr = in.ptr, *tcol = in.col;
    // 2. colours, lists and the state: cnt[0 .. K] short counts, cnt[K+1 .. 2K+1] long counts, then the largest colour
    if (!dColour) {
        if (colourBuf.alloc(M * 4)) return fail("temporary allocation (colours)");
        dColour = colourBuf.as<uint32_t>();
    }
    const uint32_t nState = 2 * (K + 1) + 1;
    if (lists.alloc(M * 4 * 4) || state.alloc(nState * 4)) return fail("temporary allocation (row lists)");
    uint32_t* const list[2][2] = {{lists.as<uint32_t>(), lists.as<uint32_t>() + M}, {lists.as<uint32_t>() + 2 * M, lists.as<uint32_t>() + 3 * M}};
    uint32_t* const cntS = state.as<uint32_t>(), *const cntL = cntS + K + 1, *const maxColour = cntS + 2 * (K + 1);
    std::vector<uint32_t> h(nState, 0);
    if (hipMemsetAsync(cntS, 0, nState * 4, st) != hipSuccess) return fail("state");
    {   // the two list lengths, counted into a pair of words of their own
        TempBuf pair;
        if (pair.alloc(8) || hipMemsetAsync(pair.p, 0, 8, st) != hipSuccess) return fail("state");
        withIrp(a, [&](auto irp) {
            hipLaunchKernelGGL((cl_classify_kernel<IrpT<decltype(irp)>>), gridFor(M), dim3(CL_THREADS), 0, st, M, irp, tptr, dColour, list[0][0],
                               list[1][0], pair.as<uint32_t>());
        });
        uint32_t n2[2] = {0, 0};
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(n2, pair.p, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail("classification");
        h[0] = n2[0]; h[K + 1] = n2[1];
    }
    out.longRows = h[K + 1];
    // 3. the rounds
    uint64_t nShort = h[0], nLong = h[K + 1];
    int side = 0;                                              // which half of the list pairs the next round reads
    while (nShort + nLong) {
        h[0] = (uint32_t)nShort; h[K + 1] = (uint32_t)nLong;
        for (uint32_t t = 1; t <= K; ++t) h[t] = h[K + 1 + t] = 0;
        if (hipMemcpyAsync(cntS, h.data(), 2 * (K + 1) * 4, hipMemcpyHostToDevice, st) != hipSuccess) return fail("state");
        for (uint32_t t = 0; t < K; ++t, side ^= 1) {
            withIrp(a, [&](auto irp) {
                using I = IrpT<decltype(irp)>;
                if (nShort)
                    hipLaunchKernelGGL((cl_round_short_kernel<I>), gridFor(nShort), dim3(CL_THREADS), 0, st, M, irp, a->JA, tptr, tcol, dColour, order,
                                       seed, list[0][side], cntS + t, list[0][side ^ 1], cntS + t + 1, maxColour);
                if (nLong)
                    hipLaunchKernelGGL((cl_round_long_kernel<I>), gridFor(nLong, CL_WAVES), dim3(CL_THREADS), 0, st, M, irp, a->JA, tptr, tcol, dColour,
                                       order, seed, list[1][side], cntL + t, list[1][side ^ 1], cntL + t + 1, maxColour);
            });
        }
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h.data(), cntS, nState * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail("rounds");
        ++out.hostChecks;
        uint32_t used = K;                                     // the rounds of this batch that still had a row to look at
        for (uint32_t t = 1; t <= K; ++t)
            if (h[t] + (uint64_t)h[K + 1 + t] == 0) { used = t; break; }
        out.rounds += used;
        if ((uint64_t)h[K] + h[2 * K + 1] >= nShort + nLong) {  // (never: the row that wins against all that wait is ready)
            fprintf(stderr, "libspmvhip: colour: no row could be coloured in %u rounds\n", K);
            return EXIT_FAILURE;
        }
        nShort = h[K]; nLong = h[2 * K + 1];
    }
    out.colours = (unsigned long)h[2 * (K + 1)] + 1;
    // 4. rows by (colour, id), and the largest colour class
    if (iotaBuf.alloc(M * 4) || sortedBuf.alloc(M * 4)) return fail("temporary allocation (order)");
    if (!dPerm) {
        if (permBuf.alloc(M * 4)) return fail("temporary allocation (order)");
        dPerm = permBuf.as<uint32_t>();
    }
    enqueueIota(M, iotaBuf.as<uint32_t>(), st);
    {
        TempBuf tmp;
        if (sortPairs(tmp, dColour, sortedBuf.as<uint32_t>(), iotaBuf.as<uint32_t>(), dPerm, (size_t)M, 0u, bitsFor(out.colours), st) != hipSuccess)
            return fail("sort");
        TempBuf cptr;
        std::vector<uint32_t> hc(out.colours + 1);
        if (cptr.alloc(hc.size() * 4)) return fail("temporary allocation (colour classes)");
        enqueueSortedBounds(M, out.colours, sortedBuf.as<uint32_t>(), cptr.as<uint32_t>(), st);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hc.data(), cptr.p, hc.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail("colour classes");
        for (size_t c = 0; c + 1 < hc.size(); ++c) out.maxColourRows = std::max<unsigned long>(out.maxColourRows, hc[c + 1] - hc[c]);
    }
    out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = out;
    return EXIT_SUCCESS;
}

}  // namespace spmvhip
