// lib.hpp -- what the files behind the extern "C" boundary of libspmvhip.so (abi.hip, upload.hip, launch.hip, solve.hip,
// select.hip, hostcall.hip; DESIGN.md has the table) share: the library state, the error line, the handle checks (live,
// matrix, CSR, square, made by whom from what), the launch context with its timing bracket, and the few functions one of
// those files calls in another.
#pragma once
#include <algorithm>

#include "spmvHip.h"
#include "kernels.hpp"

#pragma GCC visibility push(hidden)                  // shared between the library's files, not part of its exported surface
namespace spmvhip {

struct State {
    bool        inited = false;
    int         dev = 0;
    hipStream_t stream = nullptr;       // written by spmvHipSetStream only: a call on another stream passes a Ctx down
    bool        sync = true;            // written by spmvHipSetSync only
    int         variantRowsCSR = 2;     // 0 scalar restatement, 1 LDS-stream kernel (sequential row sums), 2 the fastest serial-order
                                        // kernel for the matrix (LDS-stream / deterministic two-phase / deterministic stripes)
    int         variantWarpCSR = 2;     // 0 wavefront-per-row restatement, 1 LDS-stream kernel (LDS segmented reduction), 2 the fastest
                                        // reduction-order kernel for the matrix (LDS-stream / two-phase / stripes), measured at first use
    int         variantEllRowMajor = 1; // hipSpMVRowsELLNNTransposed: 0 a thread walks its row in global memory, 1 LDS-stream kernel, same sums
    uint32_t    triRunRows = 256;       // hipSpTRSVCSR: T, the row threshold of the single-workgroup runs
    uint32_t    iluGroup = 16;          // hipSpILU0CSR: lanes per row
    int         gmresFused = 0;         // hipSpGMRESCSR: fold the first CGS2 update into the second projection
    uint32_t    colourK = 16;           // spmvHipColourCSR: rounds per host check
    uint32_t    aggK = 16;              // spmvHipAggregateCSR: rounds per host check
    uint32_t    rcmT = 1024;            // spmvHipRcmCSR: T, the frontier up to which one workgroup carries on
    uint32_t    amgFuseMax = 0;         // spmvHipAmgSetupSmoothed: the longest row of P_l that the fused correction takes; 0: never
                                        // fused, the form that measured faster
    uint32_t    amgGsSmallRows = 1024;  // spmvHipAmgSetGaussSeidel: a level of at most this many rows sweeps in one workgroup; 0: never
                                        // (a convention)
    uint32_t    amgGsLanes = 0;         // spmvHipAmgSetGaussSeidel: lanes per row of the sweeps: 1, 4, 8, 16, 32, 64; 0: by the level's mean row
    uint32_t    krylovK[2] = {16, 16};  // hipSpCGCSR, hipSpBiCGStabCSR: iterations per host check
    uint32_t    krylovBlockK[2] = {16, 16};   // hipSpCGBlockCSR, hipSpBiCGStabBlockCSR: the same
    int         ldsOrder = -1;          // lds_order_probe_kernel: -1 not run yet, 1 lane-ascending + in issue order, 0 anything else
    bool        ellRowLens = true;
    bool        unitValues = true;      // look for "every stored value is the same double" at upload (spmvHipSetUnitValues)
    double      lastSeconds = 0;
    spmvDim3    lastGrid{0, 0, 0}, lastBlock{0, 0, 0};
    hipEvent_t  ev0 = nullptr, ev1 = nullptr;
};
extern State S;                         // abi.hip

#define ERR(...) do { fprintf(stderr, "\33[31m\33[1m\33[44mlibspmvhip: "); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\33[0m\n"); } while (0)

// Where a launch goes and whether the call waits for it (and is timed with the library's events, which belong to the device
// of spmvHipInit).  The public launchers build it from the library state; a call on another device's stream (shard.hip), the
// host-matrix wrappers (always synchronous) and the timed loops of the selections (always enqueue-only) build their own.
struct Ctx { hipStream_t stream; bool sync; };
inline Ctx libraryCtx() { return {S.stream, S.sync}; }

inline bool ready(const char* who) {
    if (S.inited) return true;
    ERR("%s: spmvHipInit() has not been called", who);
    return false;
}

// any live device handle, a multigrid hierarchy included: hipFreeSpmat, the spmvHipAmg* calls and the solvers' dM
inline DevMat* anyDescOf(spmat* h, const char* who) {
    if (!h || !h->dev || h->dev == SPMAT_TAG_ELL_TRANSPOSED) {
        ERR("%s: not a device handle (upload with spMatCpyCSR/spMatCpyELL first)", who);
        return nullptr;
    }
    DevMat* d = static_cast<DevMat*>(h->dev);
    if (d->magic != 0x53504D56) { ERR("%s: corrupted device handle", who); return nullptr; }
    return d;
}
// ... that is a matrix: what every SpMV, format, build and solve entry point takes
inline DevMat* descOf(spmat* h, const char* who) {
    DevMat* d = anyDescOf(h, who);
    if (d && d->origin == Origin::HIERARCHY) {
        ERR("%s: the handle is a multigrid hierarchy (spmvHipAmgSetup), not a matrix: spmvHipAmgApply, spmvHipAmgRefresh, the dM of a "
            "Krylov solve and hipFreeSpmat take it", who);
        return nullptr;
    }
    return d;
}
// ... for a launcher: the vectors are raw device pointers whose extent the library cannot know, but a NULL one would be
// dereferenced by every lane of the kernel -- a GPU page fault, which on a shared node is everybody's problem
inline DevMat* descOf(spmat* h, const double* x, const double* y, const char* who) {
    DevMat* d = descOf(h, who);
    if (d && (!x || !y)) { ERR("%s: %s is NULL", who, !x ? "x" : "y"); return nullptr; }
    return d;
}
// ... that must be CSR: `what` is this entry point's own wording of the refusal (null: refused without a line)
inline DevMat* csrOnly(DevMat* d, const char* who, const char* what = "handle is not CSR") {
    if (!d || d->kind == Kind::CSR) return d;
    if (what) ERR("%s: %s", who, what);
    return nullptr;
}
inline DevMat* csrOf(spmat* h, const char* who, const char* what = "handle is not CSR") { return csrOnly(descOf(h, who), who, what); }
inline DevMat* csrOf(spmat* h, const double* x, const double* y, const char* who, const char* what = "handle is not CSR") {
    return csrOnly(descOf(h, x, y, who), who, what);
}
// ... square, with rows and positions that fit 32-bit words, and a column array: what the triangular solves, ILU(0), the
// colouring, the permutation, the aggregation and the multigrid setup take (`ell`: the entry point's wording for an ELL handle)
inline DevMat* squareCsrOf(spmat* h, const char* who, const char* ell) {
    if (!ready(who)) return nullptr;
    DevMat* d = csrOf(h, who, ell);
    if (!d) return nullptr;
    if (d->M != d->N) { ERR("%s: M=%lu != N=%lu: the matrix is not square", who, (unsigned long)d->M, (unsigned long)d->N); return nullptr; }
    if (d->NZ >= IRP32_LIMIT || d->M >= (1ull << 31)) {
        ERR("%s: NZ=%lu, M=%lu: positions and rows are 32-bit (limits %lu, 2^31)", who, (unsigned long)d->NZ, (unsigned long)d->M,
            (unsigned long)IRP32_LIMIT);
        return nullptr;
    }
    if (d->NZ && !d->JA) { ERR("%s: the handle has no column array", who); return nullptr; }
    return d;
}

// Provenance.  The makers record it with setOrigin; everything that takes a derived handle asks madeBy: was x (argument
// xName) made as `want`, TRANSPOSE or later, from a (and, a product or a sum, from b, in that order)?  The refusal names the
// maker, or the argument that is not the source.  a == null asks for the origin alone.
inline void setOrigin(DevMat* d, Origin o, const DevMat* a = nullptr, const DevMat* b = nullptr) {
    d->origin = o; d->src[0] = a ? a->id : 0; d->src[1] = b ? b->id : 0;
}
inline bool madeBy(const DevMat* x, Origin want, const DevMat* a, const DevMat* b, const char* who, const char* xName,
                   const char* aName = nullptr, const char* bName = nullptr) {
    static const struct { const char* maker; const char* made; } texts[] = {     // TRANSPOSE .. FSAI
        {"spmvHipCsrTranspose", "transposed"}, {"spmvHipCsrPermute", "permuted"}, {"spmvHipSpGEMM", ""}, {"spmvHipAmgSetup", "set up"},
        {"spmvHipCsrAdd", ""}, {"spmvHipCsrFilter", "filtered"}, {"spmvHipCooAssemble", "assembled"}, {"spmvHipFsaiSetup", "set up"}};
    const auto& text = texts[(int)want - (int)Origin::TRANSPOSE];
    if (x->origin != want) { ERR("%s: %s was not made by %s", who, xName, text.maker); return false; }
    if (!a || (a->id == x->src[0] && (!b || b->id == x->src[1]))) return true;
    if (b && want == Origin::SUM) ERR("%s: (%s, %s) is not the pair, alpha with the first, that %s is the sum of", who, aName, bName, xName);
    else if (b) ERR("%s: (%s, %s) is not the pair, in its order, that %s is the product of", who, aName, bName, xName);
    else ERR("%s: %s is not the handle %s was %s from", who, aName, xName, text.made);
    return false;
}

// two vectors of `bytes` bytes each share memory (the same vector included)
inline bool overlaps(const void* p, const void* q, uint64_t bytes) {
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    return bytes && p0 < q0 + bytes && q0 < p0 + bytes;
}

// Dense blocks at the boundary: the one place that knows the layout constants of spmvHip.h.
// The rows x k operand (p, ld, layout) whose leading dimension is the argument `name`, checked: ld >= k (row-major) or >=
// the rows (column-major).  A refusal leaves *out alone.
inline bool denseOperand(const char* who, const char* name, uint64_t rows, unsigned k, const double* p, size_t ld, int layout, Dense* out) {
    if (layout != SPMV_DENSE_ROW_MAJOR && layout != SPMV_DENSE_COL_MAJOR) { ERR("%s: unknown layout %d", who, layout); return false; }
    const uint64_t need = layout == SPMV_DENSE_ROW_MAJOR ? k : rows;
    if (ld < need) { ERR("%s: leading dimension %s = %zu is below %lu", who, name, ld, (unsigned long)need); return false; }
    *out = Dense{const_cast<double*>(p), ld, layout == SPMV_DENSE_ROW_MAJOR};
    return true;
}
// bytes spanned by a dense rows x k block (0 for an empty block)
inline unsigned __int128 denseSpan(uint64_t rows, unsigned k, const Dense& d) {
    if (rows == 0) return 0;
    const unsigned __int128 last = d.rowMajor ? (unsigned __int128)(rows - 1) * d.ld + (k - 1)
                                              : (unsigned __int128)(k - 1) * d.ld + (rows - 1);
    return (last + 1) * sizeof(double);
}
// two blocks of k columns share memory.  inPlace: the same block (pointer, layout and leading dimension) does not count
inline bool denseShare(unsigned k, uint64_t rowsA, const Dense& a, uint64_t rowsB, const Dense& b, bool inPlace = false) {
    if (inPlace && a.p == b.p && a.rowMajor == b.rowMajor && a.ld == b.ld) return false;
    const unsigned __int128 spanA = denseSpan(rowsA, k, a), spanB = denseSpan(rowsB, k, b);
    const unsigned __int128 a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return spanA && spanB && a0 < b0 + spanB && b0 < a0 + spanA;
}

// timing bracket used by every launcher
struct Launch {
    const Ctx cx;
    Launch(Ctx c, dim3 grid, dim3 block) : cx(c) {
        (void)hipGetLastError();                    // finish() judges THIS launch, not whatever failed before it
        shape(grid, block);
        if (cx.sync) (void)hipEventRecord(S.ev0, cx.stream);
    }
    void shape(dim3 grid, dim3 block) { S.lastGrid = {grid.x, grid.y, grid.z}; S.lastBlock = {block.x, block.y, block.z}; }
    int finish(const char* who) {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { ERR("%s: launch failed: %s", who, hipGetErrorString(e)); return EXIT_FAILURE; }
        if (!cx.sync) return EXIT_SUCCESS;
        (void)hipEventRecord(S.ev1, cx.stream);
        e = hipEventSynchronize(S.ev1);
        if (e != hipSuccess) { ERR("%s: kernel failed: %s", who, hipGetErrorString(e)); return EXIT_FAILURE; }
        float ms = 0;
        (void)hipEventElapsedTime(&ms, S.ev0, S.ev1);
        S.lastSeconds = ms * 1e-3;
        return EXIT_SUCCESS;
    }
};

// a launcher call that has nothing to launch (no rows, or no entries: y = 0): no stale time or shape is left behind
inline int nothingToLaunch(Ctx cx, DevMat* d, double* dY) {
    S.lastSeconds = 0;
    S.lastGrid = {0, 0, 0}; S.lastBlock = {0, 0, 0};
    if (d->M && dY) {
        HIP_TRY(hipMemsetAsync(dY, 0, d->M * sizeof(double), cx.stream));
        if (cx.sync) HIP_TRY(hipStreamSynchronize(cx.stream));
    }
    return EXIT_SUCCESS;
}

// the bodies of the public launchers that the host-matrix wrappers and the selections call with a context of their own
typedef int LaunchFn(Ctx cx, spmat* dMat, double* dX, CONFIG cfg, double* dY);
LaunchFn rowsCSR, warpPerRowCSR, rowsELL, warpsPerRowELL;     // launch.hip: hipSpMVRowsCSR, ...WarpPerRowCSR, ...RowsELL, ...WarpsPerRowELLNTrasposed
int streamCSR(Ctx cx, spmat* dMat, double* dX, double* dY, bool seq);              // launch.hip: the LDS-stream kernel
int tilesForm(Ctx cx, spmat* dMat, double* dX, double* dY, bool det, const char* who);     // ... the two-phase / stripes launchers on
int stripesForm(Ctx cx, spmat* dMat, double* dX, double* dY, int mode, const char* who);   // the given form (built at the first call)
int autoRun(Ctx cx, spmat* dMat, double* dX, double* dY, int serial, const char* who);     // select.hip
void freeDesc(DevMat* d);                                                          // upload.hip: a descriptor and all it holds
void publish(spmat* h, DevMat* d, ulong M, ulong N, ulong NZ, ulong maxRowNz);     // ... into the caller's handle
int vecFill(Ctx cx, double* dVec, size_t n, uint64_t pattern);                     // abi.hip: spmvHipVecFill
int probeLdsOrder(hipStream_t stream);                                             // abi.hip: spmvHipProbeLdsAtomicOrder
void freePushStream();                                                             // launch.hip: the side stream of hipSpMVTilesReducePush

}  // namespace spmvhip
#pragma GCC visibility pop
