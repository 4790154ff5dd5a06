// select.hip -- the two timed selections among the CSR launchers (DESIGN.md sections 4, 7, 8).
#include <hip/hip_runtime.h>
#include <cstring>

#include "lib.hpp"

using namespace spmvhip;

// ---- the fastest CSR launcher for THIS matrix, found by timing --------------------------------------------------
// Which kernel wins depends on where x lives relative to the caches (DESIGN.md sections 4, 7, 8): the LDS-stream
// kernel when the columns of neighbouring rows meet in L1/L2 (narrow bands, small matrices), the stripes kernel
// while x fits the Infinity Cache, the two-phase kernel beyond.  A caller of the reference picks a kernel by name
// (CUDA_CSR_ROWS, CUDA_CSR_ROWS_WARP ...); here the two names stand for two CONTRACTS, and inside each contract the
// kernel is picked by measurement, once per handle, on the caller's own x:
//   selection 0, reduction order free (hipSpMVAutoCSR, hipSpMVWarpPerRowCSR variant 2): LDS-stream kernel with the LDS
//                segmented reduction / two-phase / stripes, sums in arrival order;
//   selection 1, serial order (hipSpMVRowsCSR variant 2): LDS-stream kernel with one thread per row / the deterministic
//                forms of the two-phase and the stripes kernel -- every candidate adds a row's products in ascending j,
//                so all of them give the bits of the serial oracle and the choice is invisible in y.
// Every eligible candidate computes y (one warm-up launch that also builds its format, then AUTO_REPS timed ones -- one
// if a launch takes milliseconds), the fastest
// stays, the formats of the others are released, and the chosen launcher runs once more so that y is its own.  The
// first call is a normal -- slow -- SpMV and synchronises the stream even in enqueue-only mode.
namespace {
// one wavefront per row: does any row hold a column smaller than its predecessor?  (the deterministic format kernels add a
// row's products in ascending COLUMN order, which is the serial oracle's ascending-j order only for such rows)
template <typename I>
__global__ __launch_bounds__(256) void csr_unsorted_kernel(uint64_t M, const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                                           uint32_t* __restrict__ flag) {
    const uint64_t r = linear_block() * 4 + threadIdx.x / 64;
    if (r >= M) return;
    const uint64_t b = IRP[r], e = IRP[r + 1];
    bool bad = false;
    for (uint64_t j = b + threadIdx.x % 64; j + 1 < e; j += 64) bad |= JA[j] > JA[j + 1];
    if (bad) atomicOr(flag, 1u);
}

constexpr int      AUTO_N = 4, AUTO_REPS = 3;
constexpr float    AUTO_LONG_MS = 2.0f;                 // a launch this long is timed once
constexpr uint64_t AUTO_MIN_NNZ = 1ull << 18;        // below this a launch is mostly latency: no private format pays
constexpr uint64_t AUTO_STRIPES_X_BYTES = 256ull << 20;   // the stripes kernel re-reads x once per XCD and round of bins
typedef int CandFn(Ctx cx, spmat* m, double* x, double* y);
int streamReduce(Ctx cx, spmat* m, double* x, double* y)   { return streamCSR(cx, m, x, y, false); }
int streamSerial(Ctx cx, spmat* m, double* x, double* y)   { return streamCSR(cx, m, x, y, true); }
int tilesArrival(Ctx cx, spmat* m, double* x, double* y)   { return tilesForm(cx, m, x, y, false, "hipSpMVTilesCSR"); }
int tilesSerial(Ctx cx, spmat* m, double* x, double* y)    { return tilesForm(cx, m, x, y, true, "hipSpMVTilesCSR (deterministic)"); }
int stripesArrival(Ctx cx, spmat* m, double* x, double* y) { return stripesForm(cx, m, x, y, 0, "hipSpMVStripesCSR"); }
int stripesOwner(Ctx cx, spmat* m, double* x, double* y)   { return stripesForm(cx, m, x, y, 1, "hipSpMVStripesCSR (deterministic: owner wavefronts)"); }
int stripesOrdered(Ctx cx, spmat* m, double* x, double* y) { return stripesForm(cx, m, x, y, 2, "hipSpMVStripesCSR (deterministic: ordered tickets)"); }
struct AutoCand { const char* name; CandFn* fn; };
const AutoCand AUTO_CAND[2][AUTO_N] = {
    {{"hipSpMVWarpPerRowCSR", &streamReduce}, {"hipSpMVTilesCSR", &tilesArrival}, {"hipSpMVStripesCSR", &stripesArrival}, {nullptr, nullptr}},
    {{"hipSpMVRowsCSR", &streamSerial}, {"hipSpMVTilesCSR(deterministic)", &tilesSerial}, {"hipSpMVStripesCSR(owner wavefronts)", &stripesOwner},
     {"hipSpMVStripesCSR(ordered tickets)", &stripesOrdered}}};

int autoSelect(Ctx cx, spmat* dMat, DevMat* d, int serial, double* dX, double* dY) {
    const bool fmtOk = d->NZ >= AUTO_MIN_NNZ && d->NZ < IRP32_LIMIT;
    const bool stripesOk = fmtOk && d->N * 8 <= AUTO_STRIPES_X_BYTES;
    bool eligible[AUTO_N] = {true, fmtOk, stripesOk, stripesOk && serial != 0};
    if (!fmtOk) { d->autoPick[serial] = 0; return EXIT_SUCCESS; }
    if (serial) {
        // the serial-order contract is ascending j; the deterministic format kernels deliver ascending COLUMNS: the same thing
        // only when no row holds a column below its predecessor (the reference's loader guarantees it, parser.c:195-202; a
        // caller's own device CSR may not) -- otherwise the LDS-stream kernel, which walks j, is the only candidate
        uint32_t unsorted = 1;                       // (what a check that fails leaves behind)
        (void)deviceFlag(0, cx.stream, "csr_unsorted_kernel", &unsorted, [&](uint32_t* dFlag) {
            withIrp(d, [&](auto irp) {
                hipLaunchKernelGGL((csr_unsorted_kernel<IrpT<decltype(irp)>>), grid2d((d->M + 3) / 4, 256), dim3(256), 0, cx.stream, d->M, irp, d->JA, dFlag);
            });
        });
        if (unsorted || probeLdsOrder(cx.stream) != 1) { d->autoPick[serial] = 0; return EXIT_SUCCESS; }
    }
    // which formats exist already (the caller's, or the other selection's winner): those are never freed here
    TileFormat*& tiles = d->tiles[serial != 0];
    StripeFormat *&shared = d->stripes[0], *&owner = d->stripes[1];    // one stream per bin (arrival order, ordered tickets) / sub-streams
    const bool hadTiles = tiles != nullptr, hadShared = shared != nullptr, hadOwner = owner != nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); ERR("hipSpMVAutoCSR: event creation failed"); return EXIT_FAILURE; }
    // enqueue-only throughout (the library's own timing events belong to the device of spmvHipInit; this may run on another
    // device's stream, spmvHipEnqueueAuto) and no host round trip inside e0..e1
    const Ctx timed{cx.stream, false};
    int best = -1;
    float bestMs = 0;
    // Lower bound of a format kernel's time: its bytes per entry at the rate this HBM streams (MI355X_MICROARCH.md: 6.3 TB/s).
    // A candidate whose BOUND is no better than what has already been measured cannot win: its format (12 B/nnz of memory,
    // 12 B/nnz of temporaries) is not built.  Order: no format, 12 B/nnz (stripes), 28 B/nnz (two-phase).
    const double vb = d->unit ? 8.0 : 0.0;           // a matrix whose values are all the same streams no values
    const double boundMs[AUTO_N] = {0.0, (double)d->NZ * (28.0 - vb) / 6.3e12 * 1e3, (double)d->NZ * (12.0 - vb) / 6.3e12 * 1e3,
                                    (double)d->NZ * (12.0 - vb) / 6.3e12 * 1e3};
    const int order[AUTO_N] = {0, 2, 3, 1};
    for (int k = 0; k < AUTO_N; ++k) {
        const int c = order[k];
        if (!eligible[c] || !AUTO_CAND[serial][c].fn) continue;
        if (best >= 0 && boundMs[c] >= bestMs) { d->autoMs[serial][c] = 0; continue; }
        const int rcWarm = AUTO_CAND[serial][c].fn(timed, dMat, dX, dY) || hipStreamSynchronize(cx.stream) != hipSuccess;   // warm-up + format build
        if (rcWarm) {                                                     // a candidate that fails is not a candidate ...
            (void)hipGetLastError();                                      // ... and must not leave its error behind for the next one
            continue;
        }
        // one timed launch; AUTO_REPS - 1 more only when a launch is short enough for its timing to be noisy (on c5 the
        // LDS-stream candidate takes 31 ms a launch: measuring it three times more costs as much as building the winner's format)
        float ms = 0, more = 0;
        bool ok = hipEventRecord(e0, cx.stream) == hipSuccess && AUTO_CAND[serial][c].fn(timed, dMat, dX, dY) == EXIT_SUCCESS &&
                  hipEventRecord(e1, cx.stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        int reps = 1;
        if (ok && ms < AUTO_LONG_MS) {
            ok = hipEventRecord(e0, cx.stream) == hipSuccess;
            for (int r = 1; ok && r < AUTO_REPS; ++r) ok = AUTO_CAND[serial][c].fn(timed, dMat, dX, dY) == EXIT_SUCCESS;
            ok = ok && hipEventRecord(e1, cx.stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
                 hipEventElapsedTime(&more, e0, e1) == hipSuccess;
            reps = AUTO_REPS;
        }
        if (!ok) { (void)hipGetLastError(); continue; }
        const float perLaunch = (ms + more) / reps;
        d->autoMs[serial][c] = perLaunch;
        if (best < 0 || perLaunch < bestMs) { best = c; bestMs = perLaunch; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (best < 0) { ERR("hipSpMVAutoCSR: no candidate kernel ran"); return EXIT_FAILURE; }
    // the losers' private copies of the matrix (12 B/nnz each) go; formats that existed before stay.  The shared-stream
    // stripes layout serves candidate 2 of the reduction-order selection and candidate 3 of the serial-order one.
    const bool keepShared = serial ? best == 3 : best == 2, keepOwner = serial && best == 2;
    if (best != 1 && !hadTiles) { freeTiles(tiles); tiles = nullptr; }
    if (!keepShared && !hadShared) { freeStripes(shared); shared = nullptr; }
    if (!keepOwner && !hadOwner) { freeStripes(owner); owner = nullptr; }
    d->autoPick[serial] = best;
    return EXIT_SUCCESS;
}
}  // namespace

namespace spmvhip {
int autoRun(Ctx cx, spmat* dMat, double* dX, double* dY, int serial, const char* who) {
    DevMat* d = csrOf(dMat, dX, dY, who);
    if (!d) return EXIT_FAILURE;
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    if (d->autoPick[serial] < 0 && autoSelect(cx, dMat, d, serial, dX, dY)) return EXIT_FAILURE;
    return AUTO_CAND[serial][d->autoPick[serial]].fn(cx, dMat, dX, dY);   // (also after the selection: y then is the chosen kernel's own)
}

}  // namespace spmvhip

extern "C" {

int hipSpMVAutoCSR(spmat* dMat, double* dX, CONFIG, double* dY) { return autoRun(libraryCtx(), dMat, dX, dY, 0, "hipSpMVAutoCSR"); }

static const char* autoChoice(spmat* dMat, int serial, double* msPerCandidate) {
    DevMat* d = descOf(dMat, "spmvHipAutoChoice");
    if (!d || d->autoPick[serial] < 0) return nullptr;
    if (msPerCandidate) for (int c = 0; c < AUTO_N; ++c) msPerCandidate[c] = d->autoMs[serial][c];
    return AUTO_CAND[serial][d->autoPick[serial]].name;
}
const char* spmvHipAutoChoice(spmat* dMat, double* msPerCandidate) { return autoChoice(dMat, 0, msPerCandidate); }
const char* spmvHipAutoChoiceRows(spmat* dMat, double* msPerCandidate) { return autoChoice(dMat, 1, msPerCandidate); }

// enqueue-only form of a selection's launcher on an explicit stream (shard.hip: one stream per device); the first call
// for a handle measures the candidates on that stream and synchronises it
int spmvHipEnqueueAuto(spmat* dMat, double* dX, double* dY, void* stream) { return autoRun(Ctx{static_cast<hipStream_t>(stream), false}, dMat, dX, dY, 0, "spmvHipEnqueueAuto"); }
int spmvHipEnqueueAutoRows(spmat* dMat, double* dX, double* dY, void* stream) { return autoRun(Ctx{static_cast<hipStream_t>(stream), false}, dMat, dX, dY, 1, "spmvHipEnqueueAutoRows"); }

}  // extern "C"
