// launch.hip -- the launchers of the extern "C" boundary: CSR (restatements, LDS-stream kernel, blocks of vectors), SELL, the
// two-phase and the stripes format with their build entry points and queries, and ELL.  (The solver side is solve.hip.)
// Every launcher takes its stream and its synchronisation from a Ctx (lib.hpp); the public ones build it from the library state.
#include <hip/hip_runtime.h>

#include "lib.hpp"

using namespace spmvhip;

namespace {

unsigned blockThreads(const CONFIG& cfg, unsigned dflt, unsigned maxThreads) {
    unsigned t = cfg.blockSize.x * std::max(1u, cfg.blockSize.y) * std::max(1u, cfg.blockSize.z);
    if (cfg.blockSize.x == 0) return dflt;
    if (t % WAVE != 0 || t > maxThreads) {
        ERR("CONFIG.blockSize %ux%ux%u is not a multiple of the 64-lane wavefront (or exceeds %u): using %u",
            cfg.blockSize.x, cfg.blockSize.y, cfg.blockSize.z, maxThreads, dflt);
        return dflt;
    }
    return t;
}

// the LDS-stream kernel: SEQ = one thread sums its row in ascending j, otherwise the LDS segmented reduction
template <bool SEQ>
void launchStream2(hipStream_t stream, DevMat* d, double* x, double* y) {
    withIrp(d, [&](auto irp) {
        const auto kernel = d->unit ? csr_stream2_kernel<IrpT<decltype(irp)>, SEQ, true> : csr_stream2_kernel<IrpT<decltype(irp)>, SEQ, false>;
        hipLaunchKernelGGL(kernel, grid2d(d->nBlk2, WG_THREADS), dim3(WG_THREADS), 0, stream,
                           d->nBlk2, d->nLong2, d->blkInfo, d->blkBase, irp, d->JA, d->AS, d->unitValue, x, y);
    });
}

// ... from the handle's single-precision form (built: the caller has checked): the V = float instance on AS32, or -- a unit
// handle -- the UNIT instance with the register value rounded to single precision
template <bool SEQ>
void launchStream2F32(hipStream_t stream, DevMat* d, double* x, double* y) {
    withIrp(d, [&](auto irp) {
        using I = IrpT<decltype(irp)>;
        const dim3 grid = grid2d(d->nBlk2, WG_THREADS), block(WG_THREADS);
        if (d->unit)
            hipLaunchKernelGGL((csr_stream2_kernel<I, SEQ, true>), grid, block, 0, stream, d->nBlk2, d->nLong2, d->blkInfo, d->blkBase, irp, d->JA,
                               d->AS, d->unitValue32, x, y);
        else
            hipLaunchKernelGGL((csr_stream2_kernel<I, SEQ, false, float>), grid, block, 0, stream, d->nBlk2, d->nLong2, d->blkInfo, d->blkBase, irp,
                               d->JA, d->AS32, 0.0, x, y);
    });
}

// the checked CSR handle of an f32 launcher: its single-precision form must be built (a launcher never allocates)
DevMat* f32Of(spmat* dMat, const double* dX, const double* dY, const char* who) {
    DevMat* d = csrOf(dMat, dX, dY, who, "handle is not CSR (only CSR handles have a single-precision value form)");
    if (d && !d->f32) {
        ERR("%s: the handle's single-precision value form is not built: call spmvHipValuesF32(dMat, 1) first", who);
        return nullptr;
    }
    return d;
}

int streamCSRf32(Ctx cx, spmat* dMat, double* dX, double* dY, bool seq) {
    const char* who = seq ? "hipSpMVRowsCSRf32" : "hipSpMVWarpPerRowCSRf32";
    DevMat* d = f32Of(dMat, dX, dY, who);
    if (!d) return EXIT_FAILURE;
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    Launch L(cx, grid2d(d->nBlk2, WG_THREADS), dim3(WG_THREADS));
    (seq ? launchStream2F32<true> : launchStream2F32<false>)(cx.stream, d, dX, dY);
    return L.finish(who);
}

// row-major ELL through the LDS-stream kernel (a row must fit a block): seq = one thread sums a row in ascending slots
int launchEllStream(Ctx cx, DevMat* d, bool rl, bool seq, double* x, double* y, const char* who) {
    const uint32_t rowsPerBlk = std::min<uint32_t>((uint32_t)(STREAM_NNZ / d->pitch), WG_THREADS);
    const uint64_t nBlk = (d->M + rowsPerBlk - 1) / rowsPerBlk;
    const dim3 grid = grid2d(nBlk, WG_THREADS), block(WG_THREADS);
    Launch L(cx, grid, block);
#define ELL_STREAM(RLV, SEQV, ...) hipLaunchKernelGGL((ell_stream_kernel<RLV, SEQV, ##__VA_ARGS__>), grid, block, 0, cx.stream, (uint32_t)d->M, (uint32_t)d->K, \
                                                      (uint32_t)d->pitch, rowsPerBlk, nBlk, d->JA, d->AS, d->RL, x, y, d->unitValue)
    if (rl && d->unit) { if (seq) ELL_STREAM(true, true, true); else ELL_STREAM(true, false, true); }
    else if (rl) { if (seq) ELL_STREAM(true, true); else ELL_STREAM(true, false); }
    else    { if (seq) ELL_STREAM(false, true); else ELL_STREAM(false, false); }
#undef ELL_STREAM
    return L.finish(who);
}

template <int G>
void launchEllGroup(hipStream_t stream, DevMat* d, bool rl, dim3 grid, dim3 block, double* x, double* y) {
    const auto kernel = rl ? ell_rowmajor_group<true, G> : ell_rowmajor_group<false, G>;
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, (uint32_t)d->M, (uint32_t)d->K, d->pitch, d->JA, d->AS, d->RL, x, y);
}

// What a form of the two-phase / stripes format is built with when nobody gave options (spmvHipBuild*Opt): the arrival-order
// forms with the builders' own defaults, the deterministic forms (serial-order sums / owner wavefronts) with these
const spmvTilesOpts   TILES_DETERMINISTIC{0, 0, -1, 0, 1};
const spmvStripesOpts STRIPES_OWNER{0, 0, -1, -1, 1};
// that form / the layout of that launch mode, built if it is missing; null: the build failed
TileFormat* ensureTiles(DevMat* d, bool deterministic) {
    if (!d->tiles[deterministic]) (void)buildTiles(d, deterministic ? &TILES_DETERMINISTIC : nullptr);
    return d->tiles[deterministic];
}
StripeFormat* ensureStripes(DevMat* d, int mode) {
    const int layout = stripesLayout(mode);
    if (!d->stripes[layout]) (void)buildStripes(d, layout ? &STRIPES_OWNER : nullptr);
    return d->stripes[layout];
}
bool nonEmptyCsr(const DevMat* d, const char* who) {
    if (d->kind == Kind::CSR && d->M && d->NZ) return true;
    ERR("%s: needs a non-empty CSR handle", who);
    return false;
}

// the push kernel's side stream (hipSpMVTilesReducePush) with its fork / join events: made on first use, on the device of
// that moment, and given back by spmvHipFinalize()
hipStream_t g_pushSide = nullptr; hipEvent_t g_pushFork = nullptr, g_pushJoin = nullptr; bool g_pushPending = false;

}  // namespace

namespace spmvhip {

void freePushStream() {
    if (!g_pushSide) return;
    (void)hipStreamSynchronize(g_pushSide);
    (void)hipStreamDestroy(g_pushSide);
    (void)hipEventDestroy(g_pushFork);
    (void)hipEventDestroy(g_pushJoin);
    g_pushSide = nullptr; g_pushFork = g_pushJoin = nullptr; g_pushPending = false;
}

// ---- CSR launchers --------------------------------------------------------------------------------------------
// variant 1 of hipSpMVRowsCSR (seq) / hipSpMVWarpPerRowCSR; candidate 0 of the two selections
int streamCSR(Ctx cx, spmat* dMat, double* dX, double* dY, bool seq) {
    const char* who = seq ? "hipSpMVRowsCSR" : "hipSpMVWarpPerRowCSR";
    DevMat* d = csrOf(dMat, dX, dY, who);
    if (!d) return EXIT_FAILURE;
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    Launch L(cx, grid2d(d->nBlk2, WG_THREADS), dim3(WG_THREADS));
    (seq ? launchStream2<true> : launchStream2<false>)(cx.stream, d, dX, dY);
    return L.finish(who);
}

int tilesForm(Ctx cx, spmat* dMat, double* dX, double* dY, bool det, const char* who) {
    DevMat* d = csrOf(dMat, dX, dY, who);
    if (!d) return EXIT_FAILURE;
    if (d->M == 0 || d->NZ == 0) return nothingToLaunch(cx, d, dY);         // nothing to slice: y = 0
    const TileFormat* t = ensureTiles(d, det);
    if (!t) return EXIT_FAILURE;
    uint32_t bins = 0, rowsPerBin = 0;
    tilesShape(t, &bins, &rowsPerBin);
    const uint32_t p2t = tilesPhase2Threads(t);
    Launch L(cx, grid2d((uint64_t)((bins + 7) / 8) * 8, p2t), dim3(p2t));   // phase 2's shape (phase 1: one workgroup per slice piece)
    if (enqueueTiles(d, t, dX, dY, cx.stream)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    return L.finish(who);
}
// mode: 0 arrival order, 1 owner wavefronts (its own layout), 2 ordered tickets (the layout of mode 0)
int stripesForm(Ctx cx, spmat* dMat, double* dX, double* dY, int mode, const char* who) {
    DevMat* d = csrOf(dMat, dX, dY, who);
    if (!d) return EXIT_FAILURE;
    if (d->M == 0 || d->NZ == 0) return nothingToLaunch(cx, d, dY);         // nothing to sweep: y = 0
    const StripeFormat* f = ensureStripes(d, mode);
    if (!f) return EXIT_FAILURE;
    Launch L(cx, dim3(1), dim3(1));
    dim3 grid, block;
    if (enqueueStripes(f, dX, dY, cx.stream, mode, &grid, &block)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    L.shape(grid, block);                            // the persistent grid that ran: min(bins, CUs) workgroups of 256 threads
    return L.finish(who);
}

int rowsCSR(Ctx cx, spmat* dMat, double* dX, CONFIG cfg, double* dY) {
    if (S.variantRowsCSR == 2) return autoRun(cx, dMat, dX, dY, 1, "hipSpMVRowsCSR");
    if (S.variantRowsCSR == 1) return streamCSR(cx, dMat, dX, dY, true);
    DevMat* d = csrOf(dMat, dX, dY, "hipSpMVRowsCSR");
    if (!d) return EXIT_FAILURE;
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    const unsigned bt = blockThreads(cfg, BLOCKS_1D, 1024);
    const dim3 grid = grid2d((d->M + bt - 1) / bt, bt), block(bt);
    Launch L(cx, grid, block);
    withIrp(d, [&](auto irp) { hipLaunchKernelGGL((csr_scalar_kernel<IrpT<decltype(irp)>>), grid, block, 0, cx.stream, (uint32_t)d->M, irp, d->JA, d->AS, dX, dY); });
    return L.finish("hipSpMVRowsCSR");
}

int warpPerRowCSR(Ctx cx, spmat* dMat, double* dX, CONFIG cfg, double* dY) {
    if (S.variantWarpCSR == 2) return autoRun(cx, dMat, dX, dY, 0, "hipSpMVWarpPerRowCSR");
    if (S.variantWarpCSR == 1) return streamCSR(cx, dMat, dX, dY, false);
    DevMat* d = csrOf(dMat, dX, dY, "hipSpMVWarpPerRowCSR");
    if (!d) return EXIT_FAILURE;
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    const unsigned bt = blockThreads(cfg, WAVESIZE * BLOCKS_2D_WARP_R, 1024);
    const unsigned rowsPerWg = bt / WAVE;
    const dim3 grid = grid2d((d->M + rowsPerWg - 1) / rowsPerWg, bt), block(bt);
    Launch L(cx, grid, block);
    withIrp(d, [&](auto irp) { hipLaunchKernelGGL((csr_vector_kernel<IrpT<decltype(irp)>>), grid, block, 0, cx.stream, (uint32_t)d->M, irp, d->JA, d->AS, dX, dY); });
    return L.finish("hipSpMVWarpPerRowCSR");
}

// ---- ELL launchers
int rowsELL(Ctx cx, spmat* dMat, double* dX, CONFIG cfg, double* dY) {
    DevMat* d = descOf(dMat, dX, dY, "hipSpMVRowsELL");
    if (!d) return EXIT_FAILURE;
    if (d->kind != Kind::ELL_COLMAJOR) { ERR("hipSpMVRowsELL: expects the transposed (column-major) ELL upload: ellTranspose() + spMatCpyELL()"); return EXIT_FAILURE; }
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    const unsigned bt = blockThreads(cfg, BLOCKS_1D, 1024);
    const dim3 grid = grid2d((d->M + bt - 1) / bt, bt), block(bt);
    Launch L(cx, grid, block);
    const bool rl = S.ellRowLens && d->RL;
    if (rl && d->unit) hipLaunchKernelGGL((ell_colmajor_thread<true, true>), grid, block, 0, cx.stream, (uint32_t)d->M, (uint32_t)d->K, d->pitch, d->JA, d->AS, d->RL, dX, dY, d->unitValue);
    else if (rl) hipLaunchKernelGGL((ell_colmajor_thread<true>), grid, block, 0, cx.stream, (uint32_t)d->M, (uint32_t)d->K, d->pitch, d->JA, d->AS, d->RL, dX, dY, 0.0);
    else         hipLaunchKernelGGL((ell_colmajor_thread<false>), grid, block, 0, cx.stream, (uint32_t)d->M, (uint32_t)d->K, d->pitch, d->JA, d->AS, d->RL, dX, dY, 0.0);
    return L.finish("hipSpMVRowsELL");
}

int warpsPerRowELL(Ctx cx, spmat* dMat, double* dX, CONFIG, double* dY) {
    DevMat* d = descOf(dMat, dX, dY, "hipSpMVWarpsPerRowELLNTrasposed");
    if (!d) return EXIT_FAILURE;
    if (d->kind != Kind::ELL_ROWMAJOR) { ERR("hipSpMVWarpsPerRowELLNTrasposed: expects the row-major ELL upload (no ellTranspose)"); return EXIT_FAILURE; }
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    const bool rl = S.ellRowLens && d->RL;
    if (d->pitch && d->pitch <= (size_t)STREAM_NNZ)   // a row fits a block of the LDS-stream kernel: dense span loads, LDS segmented reduction
        return launchEllStream(cx, d, rl, false, dX, dY, "hipSpMVWarpsPerRowELLNTrasposed");
    // longer rows: G lanes per row -- the smallest power of two covering the slots, 4..64
    int G = 4;
    while (G < WAVE && (uint64_t)G < d->K) G <<= 1;
    const unsigned bt = 256;
    const uint64_t threads = (d->M + ELL_GROUP_ROWS - 1) / ELL_GROUP_ROWS * (uint64_t)G;     // a group of G lanes owns 4 rows
    const dim3 grid = grid2d((threads + bt - 1) / bt, bt), block(bt);
    Launch L(cx, grid, block);
    switch (G) {
        case 4:  launchEllGroup<4>(cx.stream, d, rl, grid, block, dX, dY); break;
        case 8:  launchEllGroup<8>(cx.stream, d, rl, grid, block, dX, dY); break;
        case 16: launchEllGroup<16>(cx.stream, d, rl, grid, block, dX, dY); break;
        case 32: launchEllGroup<32>(cx.stream, d, rl, grid, block, dX, dY); break;
        default: launchEllGroup<64>(cx.stream, d, rl, grid, block, dX, dY); break;
    }
    return L.finish("hipSpMVWarpsPerRowELLNTrasposed");
}
}  // namespace spmvhip

extern "C" {

int hipSpMVRowsCSR(spmat* dMat, double* dX, CONFIG cfg, double* dY) { return rowsCSR(libraryCtx(), dMat, dX, cfg, dY); }
int hipSpMVWarpPerRowCSR(spmat* dMat, double* dX, CONFIG cfg, double* dY) { return warpPerRowCSR(libraryCtx(), dMat, dX, cfg, dY); }
int hipSpMVRowsELL(spmat* dMat, double* dX, CONFIG cfg, double* dY) { return rowsELL(libraryCtx(), dMat, dX, cfg, dY); }
int hipSpMVWarpsPerRowELLNTrasposed(spmat* dMat, double* dX, CONFIG cfg, double* dY) { return warpsPerRowELL(libraryCtx(), dMat, dX, cfg, dY); }

// enqueue-only entry used by shard.hip (explicit stream, no timing bracket, current device = the matrix')
int spmvHipEnqueueCSR(spmat* dMat, int warpPerRow, double* dX, double* dY, void* stream) {
    DevMat* d = csrOf(dMat, dX, dY, "spmvHipEnqueueCSR", nullptr);
    if (!d) return EXIT_FAILURE;
    if (d->M == 0) return EXIT_SUCCESS;
    (warpPerRow ? launchStream2<false> : launchStream2<true>)(static_cast<hipStream_t>(stream), d, dX, dY);
    HIP_TRY(hipGetLastError());
    return EXIT_SUCCESS;
}

// ---- the products from single-precision storage (contract in spmvHip.h, design in DESIGN.md section 41): the LDS-stream kernel only
int hipSpMVRowsCSRf32(spmat* dMat, double* dX, CONFIG, double* dY) { return streamCSRf32(libraryCtx(), dMat, dX, dY, true); }
int hipSpMVWarpPerRowCSRf32(spmat* dMat, double* dX, CONFIG, double* dY) { return streamCSRf32(libraryCtx(), dMat, dX, dY, false); }
int spmvHipEnqueueRowsF32(spmat* dMat, double* dX, double* dY, void* stream) {
    DevMat* d = f32Of(dMat, dX, dY, "spmvHipEnqueueRowsF32");
    if (!d) return EXIT_FAILURE;
    if (d->M == 0) return EXIT_SUCCESS;
    launchStream2F32<true>(static_cast<hipStream_t>(stream), d, dX, dY);
    HIP_TRY(hipGetLastError());
    return EXIT_SUCCESS;
}

// ---- blocks of vectors: Y = A X (contract in spmvHip.h, design in DESIGN.md section 15); f32: from the single-precision form
static int spmmRows(const char* who, bool f32, spmat* dMat, unsigned k, const double* dX, size_t ldx, int xLayout, double* dY, size_t ldy, int yLayout) {
    const Ctx cx = libraryCtx();
    DevMat* d = f32 ? f32Of(dMat, dX, dY, who) : csrOf(dMat, dX, dY, who, "handle is not CSR (ELL handles are not supported)");
    if (!d) return EXIT_FAILURE;
    if (k == 0) { ERR("%s: k = 0 columns", who); return EXIT_FAILURE; }
    Dense X, Y;                                                          // X has N rows, Y has M
    if (!denseOperand(who, "ldx", d->N, k, dX, ldx, xLayout, &X) || !denseOperand(who, "ldy", d->M, k, dY, ldy, yLayout, &Y)) return EXIT_FAILURE;
    if (denseShare(k, d->N, X, d->M, Y)) { ERR("%s: X and Y overlap", who); return EXIT_FAILURE; }
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    Launch L(cx, grid2d(d->nBlk2, WG_THREADS), dim3(WG_THREADS));
    if (k == 1 && X.sr() == 1 && Y.sr() == 1) (f32 ? launchStream2F32<true> : launchStream2<true>)(cx.stream, d, X.p, dY);     // one plain vector: the SpMV kernel
    else if (enqueueSpmm(d, k, X, Y, cx.stream, f32)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    return L.finish(who);
}
int hipSpMMRowsCSR(spmat* dMat, unsigned k, const double* dX, size_t ldx, int xLayout, double* dY, size_t ldy, int yLayout) {
    return spmmRows("hipSpMMRowsCSR", false, dMat, k, dX, ldx, xLayout, dY, ldy, yLayout);
}
int hipSpMMRowsCSRf32(spmat* dMat, unsigned k, const double* dX, size_t ldx, int xLayout, double* dY, size_t ldy, int yLayout) {
    return spmmRows("hipSpMMRowsCSRf32", true, dMat, k, dX, ldx, xLayout, dY, ldy, yLayout);
}

// explicit launchers and queries work on the form last asked for with spmvHipBuild*Opt (default: arrival order)
int hipSpMVTilesCSR(spmat* dMat, double* dX, CONFIG, double* dY) {
    DevMat* d = descOf(dMat, "hipSpMVTilesCSR");
    return d ? tilesForm(libraryCtx(), dMat, dX, dY, d->tilesPref, "hipSpMVTilesCSR") : EXIT_FAILURE;
}
int hipSpMVStripesCSR(spmat* dMat, double* dX, CONFIG, double* dY) {
    DevMat* d = descOf(dMat, "hipSpMVStripesCSR");
    return d ? stripesForm(libraryCtx(), dMat, dX, dY, d->stripesPref, "hipSpMVStripesCSR") : EXIT_FAILURE;
}

int spmvHipBuildTiles(spmat* dMat) {
    DevMat* d = csrOf(dMat, "spmvHipBuildTiles");
    return d && ensureTiles(d, d->tilesPref) ? EXIT_SUCCESS : EXIT_FAILURE;
}
size_t spmvHipTilesBytes(spmat* dMat) { DevMat* d = descOf(dMat, "spmvHipTilesBytes"); return d ? tilesBytes(d) : 0; }

int spmvHipBuildSell(spmat* dMat) {
    DevMat* d = csrOf(dMat, "spmvHipBuildSell");
    return d ? buildSell(d) : EXIT_FAILURE;
}
size_t spmvHipSellBytes(spmat* dMat) { DevMat* d = descOf(dMat, "spmvHipSellBytes"); return d ? sellBytes(d) : 0; }
int hipSpMVRowsSELL(spmat* dMat, double* dX, CONFIG, double* dY) {
    const Ctx cx = libraryCtx();
    DevMat* d = csrOf(dMat, dX, dY, "hipSpMVRowsSELL", "handle is not CSR (the SELL-C-sigma copy is derived from an uploaded CSR)");
    if (!d) return EXIT_FAILURE;
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    if (!d->sell && buildSell(d)) return EXIT_FAILURE;
    Launch L(cx, grid2d((d->M + 255) / 256, 256), dim3(256));
    if (enqueueSell(d, dX, dY, cx.stream)) { ERR("hipSpMVRowsSELL: launch failed"); return EXIT_FAILURE; }
    return L.finish("hipSpMVRowsSELL");
}

int spmvHipBuildStripes(spmat* dMat) {
    DevMat* d = csrOf(dMat, "spmvHipBuildStripes");
    return d && ensureStripes(d, d->stripesPref) ? EXIT_SUCCESS : EXIT_FAILURE;
}
int spmvHipBuildStripesOpt(spmat* dMat, const spmvStripesOpts* opts) {
    DevMat* d = descOf(dMat, "spmvHipBuildStripesOpt");
    if (!d || !opts || !nonEmptyCsr(d, "spmvHipBuildStripesOpt") || buildStripes(d, opts)) return EXIT_FAILURE;
    d->stripesPref = opts->deterministic;            // what hipSpMVStripesCSR and the queries use from now on
    return EXIT_SUCCESS;
}
size_t spmvHipStripesBytes(spmat* dMat) { DevMat* d = descOf(dMat, "spmvHipStripesBytes"); return d ? stripesBytes(d) : 0; }
int spmvHipStripesInfo(spmat* dMat, spmvStripesInfo* info) {
    DevMat* d = descOf(dMat, "spmvHipStripesInfo");
    if (!d || !info) return EXIT_FAILURE;
    stripesInfo(d->stripes[stripesLayout(d->stripesPref)], info);
    if (info->nBins && d->stripesPref == 2) info->deterministic = 2;     // the shared-stream layout, launched in ticket order
    return EXIT_SUCCESS;
}
int spmvHipStripesShape(spmat* dMat, unsigned* nBins, unsigned* rowsPerBin, int* wide, double* buildMs) {
    spmvStripesInfo i;
    if (spmvHipStripesInfo(dMat, &i)) return EXIT_FAILURE;
    if (nBins) *nBins = i.nBins;
    if (rowsPerBin) *rowsPerBin = i.rowsPerBin;
    if (wide) *wide = i.wide;
    if (buildMs) *buildMs = i.buildMs;
    return EXIT_SUCCESS;
}

// the two-phase format the explicit entry points below work on: the preferred form, built if missing (null: refused or failed)
struct TilesOf { DevMat* d; TileFormat* t; };
static TilesOf tilesReady(spmat* dMat, const char* who) {
    DevMat* d = descOf(dMat, who);
    return {d, d && nonEmptyCsr(d, who) ? ensureTiles(d, d->tilesPref) : nullptr};
}

int spmvHipTilesShape(spmat* dMat, unsigned* nBins, unsigned* rowsPerBin) {
    const TileFormat* t = tilesReady(dMat, "spmvHipTilesShape").t;
    if (!t || !nBins || !rowsPerBin) return EXIT_FAILURE;
    uint32_t b = 0, r = 0;
    tilesShape(t, &b, &r);
    *nBins = b; *rowsPerBin = r;
    return EXIT_SUCCESS;
}

int spmvHipBuildTilesOpt(spmat* dMat, const spmvTilesOpts* opts) {
    DevMat* d = descOf(dMat, "spmvHipBuildTilesOpt");
    if (!d || !opts || !nonEmptyCsr(d, "spmvHipBuildTilesOpt") || buildTiles(d, opts)) return EXIT_FAILURE;
    d->tilesPref = opts->deterministic != 0;         // what hipSpMVTilesCSR, Expand / Reduce and the queries use from now on
    return EXIT_SUCCESS;
}

int spmvHipTilesInfo(spmat* dMat, spmvTilesInfo* info) {
    DevMat* d = descOf(dMat, "spmvHipTilesInfo");
    if (!d || !info) return EXIT_FAILURE;
    tilesInfo(d->tiles[d->tilesPref], info);
    return EXIT_SUCCESS;
}

int spmvHipTilesBinRow(spmat* dMat, unsigned bin, ulong* firstRow) {
    const auto [d, t] = tilesReady(dMat, "spmvHipTilesBinRow");
    if (!t || !firstRow) return EXIT_FAILURE;
    *firstRow = tilesBinRow(d, t, bin);
    return EXIT_SUCCESS;
}

int hipSpMVTilesExpand(spmat* dMat, double* dX) {
    const Ctx cx = libraryCtx();
    const auto [d, t] = tilesReady(dMat, "hipSpMVTilesExpand");
    if (!t) return EXIT_FAILURE;
    if (!dX) { ERR("hipSpMVTilesExpand: x is NULL"); return EXIT_FAILURE; }
    Launch L(cx, dim3(1), dim3(1024));
    if (enqueueTilesExpand(d, t, dX, cx.stream)) { ERR("hipSpMVTilesExpand: launch failed"); return EXIT_FAILURE; }
    return L.finish("hipSpMVTilesExpand");
}

int hipSpMVTilesReduce(spmat* dMat, unsigned binBegin, unsigned binEnd, double* dY, int nExtra, double* const* dExtra) {
    const Ctx cx = libraryCtx();
    const auto [d, t] = tilesReady(dMat, "hipSpMVTilesReduce");
    if (!t) return EXIT_FAILURE;
    uint32_t b = 0, r = 0;
    tilesShape(t, &b, &r);
    if (binBegin > binEnd || binEnd > b || nExtra < 0 || nExtra > SPMV_MAX_PEERS || (nExtra && !dExtra) || !dY) {
        ERR("hipSpMVTilesReduce: bins [%u,%u) of %u, %d extra destinations: invalid", binBegin, binEnd, b, nExtra);
        return EXIT_FAILURE;
    }
    Launch L(cx, dim3(binEnd - binBegin ? binEnd - binBegin : 1), dim3(1024));
    if (enqueueTilesReduce(d, t, binBegin, binEnd, dY, nExtra, dExtra, cx.stream)) { ERR("hipSpMVTilesReduce: launch failed"); return EXIT_FAILURE; }
    return L.finish("hipSpMVTilesReduce");
}

int hipSpMVTilesReducePush(spmat* dMat, double* dY, int nExtra, double* const* dExtra) {
    const Ctx cx = libraryCtx();
    const auto [d, t] = tilesReady(dMat, "hipSpMVTilesReducePush");
    if (!t) return EXIT_FAILURE;
    if (nExtra < 1 || nExtra > SPMV_MAX_PEERS || !dExtra || !dY) { ERR("hipSpMVTilesReducePush: %d destinations: invalid", nExtra); return EXIT_FAILURE; }
    if (!g_pushSide) {
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(hipStreamCreateWithPriority(&g_pushSide, hipStreamNonBlocking, hi));      // dispatched ahead of phase 2's later rounds
        HIP_TRY(hipEventCreateWithFlags(&g_pushFork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&g_pushJoin, hipEventDisableTiming));
    }
    uint32_t b = 0, r = 0;
    tilesShape(t, &b, &r);
    Launch L(cx, dim3(b), dim3(1024));
    if (enqueueTilesReducePush(d, t, dY, nExtra, dExtra, cx.stream, g_pushSide, g_pushFork, g_pushJoin)) { ERR("hipSpMVTilesReducePush: launch failed"); return EXIT_FAILURE; }
    g_pushPending = true;
    if (cx.sync && spmvHipTilesPushJoin()) return EXIT_FAILURE;         // synchronous mode: everything delivered on return
    return L.finish("hipSpMVTilesReducePush");
}

int spmvHipTilesPushJoin(void) {
    if (g_pushPending) {
        HIP_TRY(hipStreamWaitEvent(S.stream, g_pushJoin, 0));        // push kernels run in order on one stream: the last event covers all
        g_pushPending = false;
    }
    return EXIT_SUCCESS;
}

int spmvHipTilesPushFailed(spmat* dMat) { DevMat* d = descOf(dMat, "spmvHipTilesPushFailed"); return d ? tilesPushFailed(d->tiles[d->tilesPref]) : 1; }

int hipSpMVRowsELLNNTransposed(spmat* dMat, double* dX, CONFIG cfg, double* dY) {
    const Ctx cx = libraryCtx();
    DevMat* d = descOf(dMat, dX, dY, "hipSpMVRowsELLNNTransposed");
    if (!d) return EXIT_FAILURE;
    if (d->kind != Kind::ELL_ROWMAJOR) { ERR("hipSpMVRowsELLNNTransposed: expects the row-major ELL upload (no ellTranspose)"); return EXIT_FAILURE; }
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    if (S.variantEllRowMajor == 1 && cfg.blockSize.x == 0 && d->pitch && d->pitch <= (size_t)STREAM_NNZ)
        return launchEllStream(cx, d, S.ellRowLens && d->RL, true, dX, dY, "hipSpMVRowsELLNNTransposed");
    const unsigned bt = blockThreads(cfg, BLOCKS_1D, 1024);
    const dim3 grid = grid2d((d->M + bt - 1) / bt, bt), block(bt);
    Launch L(cx, grid, block);
    const bool rl = S.ellRowLens && d->RL;
    if (rl) hipLaunchKernelGGL((ell_rowmajor_thread<true>), grid, block, 0, cx.stream, (uint32_t)d->M, (uint32_t)d->K, d->pitch, d->JA, d->AS, d->RL, dX, dY);
    else    hipLaunchKernelGGL((ell_rowmajor_thread<false>), grid, block, 0, cx.stream, (uint32_t)d->M, (uint32_t)d->K, d->pitch, d->JA, d->AS, d->RL, dX, dY);
    return L.finish("hipSpMVRowsELLNNTransposed");
}

}  // extern "C"
