// device_prims.hpp -- what a build step on the device gets its temporaries, sorts and scans from (library-private; the
// format files tiles / stripes / sell and transpose, trsv, ilu0, colour, rcm, spgemm, add include it after kernels.hpp).
//
//   TempBuf                     one scoped device buffer; with a TempTally it keeps the bytes held and their peak
//   sortPairs / sortKeys /      rocPRIM's "two-call" algorithms in one call: the size query, the workspace (grown only
//   exclusiveScan               when the call needs more than it holds), the run.  The argument list is written once.
//   enqueueIota / enqueueFill32 the two trivial kernels, defined ONCE in transpose.hip (a definition here would put a
//                               copy of each into every translation unit that includes this header)
//   bitsFor / gridFor           key bits of a radix sort, the grid of a one-item-per-lane launch
//   team_sync / clampOpt /      what the sparse product and the sparse sum share besides: the synchronisation of the lanes
//   msSince                     of a row, an option with a default and a limit, wall milliseconds
//   buildFail                   how a synchronous build step reports a failure and leaves
//   SortedPath / sortedBatches  the general path of the sparse product and the sparse sum: batches of rows, one stable
//   / sortedPass                sort per batch, a run kernel; enqueueNarrowIrp: their row pointers from a 64-bit scan.
//                               Defined ONCE, in spgemm.hip, with the kernels they launch
// rocPRIM is included here and nowhere else; its kernels are still instantiated by, and compiled into, each caller.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <functional>
#include <vector>

#include "kernels.hpp"

namespace spmvhip {

struct TempTally { size_t cur = 0, peak = 0; };     // bytes held now by the buffers that share it, and the most they held

// freed when it leaves scope: the caller sees to it that no kernel still uses it then (a synchronised stream)
struct TempBuf {
    void* p = nullptr;
    size_t n = 0;                                   // bytes asked for (the allocation itself has a floor of one byte)
    TempTally* tally;
    explicit TempBuf(TempTally* t = nullptr) : tally(t) {}
    TempBuf(const TempBuf&) = delete;
    TempBuf& operator=(const TempBuf&) = delete;
    ~TempBuf() { release(); }
    void release() {
        if (!p) return;
        (void)devFree(p);
        if (tally) tally->cur -= n;
        p = nullptr; n = 0;
    }
    hipError_t alloc(size_t bytes) {                // a buffer that holds memory gives it back first
        release();
        const hipError_t e = devMalloc(&p, std::max<size_t>(bytes, 1));
        if (e != hipSuccess) { p = nullptr; return e; }
        n = bytes;
        if (tally) { tally->cur += n; tally->peak = std::max(tally->peak, tally->cur); }
        return e;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
    // the memory is the caller's from here on (a handle takes it)
    template <typename T> T* detach() { T* q = as<T>(); if (tally) tally->cur -= n; p = nullptr; n = 0; return q; }
};

// call(nullptr, bytes) asks a rocPRIM algorithm for its workspace size, call(ws.p, bytes) runs it on `stream`.  ws grows
// only when it holds less (the size is no monotonic function of the item count); a workspace that already holds memory
// may still be in use by what the stream has queued, so the stream is synchronised before it is replaced.  Returns the
// error of the step that failed; ws.n is the size of the workspace afterwards.
template <typename F>
hipError_t withWorkspace(TempBuf& ws, hipStream_t stream, F&& call) {
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e != hipSuccess) return e;
    if (!ws.p || bytes > ws.n) {
        if (ws.p && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        if ((e = ws.alloc(bytes)) != hipSuccess) return e;
    }
    return call(ws.p, bytes);
}

// The iterator types are the callers' (a rocPRIM kernel is instantiated on them): pass the pointers as they are held.
// Stable sorts of key bits [beginBit, endBit).
template <typename KI, typename KO, typename VI, typename VO>
hipError_t sortPairs(TempBuf& ws, KI keysIn, KO keysOut, VI valsIn, VO valsOut, size_t n, unsigned beginBit, unsigned endBit,
                     hipStream_t stream) {
    return withWorkspace(ws, stream, [&](void* tmp, size_t& bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, keysIn, keysOut, valsIn, valsOut, n, beginBit, endBit, stream);
    });
}
// ... ping-pong between the two halves of each double buffer (no third full-size pair inside the workspace); the sorted
// data is where current() points afterwards
template <typename K, typename V>
hipError_t sortPairs(TempBuf& ws, rocprim::double_buffer<K>& keys, rocprim::double_buffer<V>& vals, size_t n, unsigned beginBit,
                     unsigned endBit, hipStream_t stream) {
    return withWorkspace(ws, stream, [&](void* tmp, size_t& bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, keys, vals, n, beginBit, endBit, stream);
    });
}
template <typename KI, typename KO>
hipError_t sortKeys(TempBuf& ws, KI keysIn, KO keysOut, size_t n, unsigned beginBit, unsigned endBit, hipStream_t stream) {
    return withWorkspace(ws, stream, [&](void* tmp, size_t& bytes) {
        return rocprim::radix_sort_keys(tmp, bytes, keysIn, keysOut, n, beginBit, endBit, stream);
    });
}
// out[i] = init + in[0] + ... + in[i - 1], summed in the output's type
template <typename In, typename T>
hipError_t exclusiveScan(TempBuf& ws, In in, T* out, T init, size_t n, hipStream_t stream) {
    return withWorkspace(ws, stream, [&](void* tmp, size_t& bytes) {
        return rocprim::exclusive_scan(tmp, bytes, in, out, init, n, rocprim::plus<T>(), stream);
    });
}

void enqueueIota(uint64_t n, uint32_t* p, hipStream_t stream);                  // p[i] = i          (transpose.hip)
void enqueueFill32(uint32_t* p, uint64_t n, uint32_t v, hipStream_t stream);    // p[i] = v

// The incoming side of a square handle's adjacency (colour.hip; the colouring and the aggregation share it): the pattern
// transposed -- ptr / col, M + 1 and nnz words -- or nothing (ptr == col == null, symmetric = 1) when the stored pattern
// was found structurally symmetric, which is tried when no row stores more than 64 entries.  The sort is enqueued on
// `stream`; the buffers live as long as the object, which must outlive what reads them.
struct IncomingPattern {
    TempBuf rowOf, keys, colBuf, ptrBuf, sortTmp;
    const uint32_t* ptr = nullptr;
    const uint32_t* col = nullptr;
    int symmetric = 1;                              // (no entry: nothing comes in from the transposed side)
};
struct DevMat;
int buildIncoming(const DevMat* a, IncomingPattern& in, hipStream_t stream, const char* module);

// The sorted path that the sparse product (spgemm.hip) and the sparse sum (add.hip) share; DESIGN.md sections 22 and 25.
// A caller lists rows, counts the terms of each (terms[n] = 0) and calls sortedBatches: off[k] = the terms before row k
// of the list, and the batches [batch[i], batch[i + 1]) of consecutive rows whose terms fit batchTerms (a row above the
// budget is a batch of its own).  sortedPass then runs every batch: expand(k0, nRows, off + k0, key, val) is the caller's
// own -- it enqueues what writes term f of row list[k0 + b] to off[k0 + b] - off[k0] + f as (b << 32 | column, rounded
// term; no val when !numeric) in the order of its contract --, ONE stable radix sort, and a wavefront per row that
// counts the run heads into counts[row] (!numeric) or lets the lane of each head add its run serially from +0.0 into c's
// row at its rank (numeric; c's IRP is 4-byte).  Both synchronous; every temporary counts into `tally`.
struct SortedPath {
    const char* module;                             // for the error lines ("spgemm") ...
    const char* items;                              // ... and what a term is there ("products")
    TempTally* tally;
    TempBuf off;
    std::vector<uint64_t> hOff;
    std::vector<uint32_t> batch;
    SortedPath(const char* m, const char* i, TempTally* t) : module(m), items(i), tally(t), off(t) {}
    size_t batches() const { return batch.empty() ? 0 : batch.size() - 1; }
};
using SortedExpand = std::function<void(uint32_t k0, uint32_t nRows, const uint64_t* off, uint64_t* key, double* val)>;
int sortedBatches(SortedPath& s, const uint64_t* terms, uint32_t n, uint64_t batchTerms, hipStream_t stream);
int sortedPass(SortedPath& s, bool numeric, const uint32_t* list, const SortedExpand& expand, uint32_t* counts, const DevMat* c,
               hipStream_t stream);
// irp[r] = (uint32_t)irp64[r] for r in [0, M], and *maxLen = max(*maxLen, the longest row)
void enqueueNarrowIrp(uint64_t M, const uint64_t* irp64, uint32_t* irp, uint32_t* maxLen, hipStream_t stream);

// The T lanes that share a row in the sparse product and the sparse sum synchronise here: a wavefront (T = 64; its LDS
// operations execute in issue order, so a compiler fence is the whole synchronisation) or the workgroup.
template <int T> __device__ __forceinline__ void team_sync() {
    if constexpr (T == 64) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    } else {
        __syncthreads();
    }
}

// an option of a build: 0 asks for the default, a value above the limit is clamped to it
inline uint64_t clampOpt(uint64_t v, uint64_t dflt, uint64_t limit) { return v == 0 ? dflt : std::min(v, limit); }
inline double msSince(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the bits that hold every key below n (at least 1, at most 32); every key in [0, maxKey] needs bitsFor(maxKey + 1)
inline unsigned bitsFor(uint64_t n) {
    unsigned bits = 1;
    while (bits < 32 && (1ull << bits) < n) ++bits;
    return bits;
}

// the grid of `items` dealt perBlock to a workgroup of `threads` lanes
inline dim3 gridFor(uint64_t items, uint32_t perBlock = WG_THREADS, unsigned threads = WG_THREADS) {
    return grid2d((items + perBlock - 1) / perBlock, threads);
}

// a failed step of a synchronous build: the sticky error cleared, one line, and the stream synchronised -- nothing may
// still use the caller's temporaries when they go
inline int buildFail(hipStream_t stream, const char* module, const char* what) {
    (void)hipGetLastError();
    fprintf(stderr, "libspmvhip: %s: %s failed\n", module, what);
    (void)hipStreamSynchronize(stream);
    return EXIT_FAILURE;
}

}  // namespace spmvhip
