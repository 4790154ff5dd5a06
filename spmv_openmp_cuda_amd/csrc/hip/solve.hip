// solve.hip -- the solver side of the extern "C" boundary: triangular solves, ILU(0), the multi-colour ordering, the reverse
// Cuthill-McKee ordering and the vector permutation, the dots, aggregation multigrid, the three Krylov solvers, the basis rotation
// and the two eigensolvers (Lanczos, Davidson) with the residual block.  The algorithm
// files (trsv.hip, ilu0.hip, colour.hip, rcm.hip, krylov.hip, gmres.hip, lanczos.hip, davidson.hip, aggregate.hip, amg.hip) build and launch; here are the checks, the library's settings
// handed down as arguments, and the timing bracket.  Contracts in spmvHip.h, designs in DESIGN.md sections 17 to 21 and 24.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>

#include "lib.hpp"
#include "krylov.hpp"

using namespace spmvhip;

// a square CSR handle and a triangle of it
static DevMat* triHandle(spmat* dA, int uplo, const char* who) {
    DevMat* d = squareCsrOf(dA, who, "the handle is an ELL handle (only CSR handles are solved)");
    if (d && uplo != SPMV_TRI_LOWER && uplo != SPMV_TRI_UPPER) { ERR("%s: unknown uplo %d", who, uplo); return nullptr; }
    return d;
}

// dM as a hierarchy of dA (*pa)
static DevMat* hierarchyOf(spmat* dM, spmat* dA, const char* who, DevMat** pa) {
    if (!ready(who)) return nullptr;
    if (!dM || !dA) { ERR("%s: %s is NULL", who, !dM ? "dM" : "dA"); return nullptr; }
    DevMat* m = anyDescOf(dM, who);
    DevMat* a = m ? csrOf(dA, who, "dA is an ELL handle") : nullptr;
    if (!a || !madeBy(m, Origin::HIERARCHY, a, nullptr, who, "dM", "dA")) return nullptr;
    *pa = a;
    return m;
}

// dM as a hierarchy, for a view of its level `level`: one below the last when lastLacks says what the last level has not.
// noInfo: the entry's info, which it cannot do without, is NULL (refused after the handle, before the hierarchy, as ever).
static DevMat* hierarchyLevel(spmat* dM, const char* who, unsigned level, const char* lastLacks, bool noInfo = false) {
    DevMat* m = anyDescOf(dM, who);
    if (!m) return nullptr;
    if (noInfo) { ERR("%s: info is NULL", who); return nullptr; }
    if (!madeBy(m, Origin::HIERARCHY, nullptr, nullptr, who, "dM")) return nullptr;
    const size_t levels = amgInfo(m)->levels;              // (a hierarchy has at least one level)
    if (lastLacks && level >= levels - 1) { ERR("%s: level %u of %zu: the last level has no %s", who, level, levels, lastLacks); return nullptr; }
    if (level >= levels) { ERR("%s: level %u of %zu", who, level, levels); return nullptr; }
    return m;
}

extern "C" {

// ---- triangular solves
int spmvHipTriAnalyse(spmat* dA, int uplo) {
    const char* who = "spmvHipTriAnalyse";
    DevMat* d = triHandle(dA, uplo, who);
    if (!d) return EXIT_FAILURE;
    if (d->tri[uplo] || d->M == 0) return EXIT_SUCCESS;
    if (triAnalyse(d, uplo, S.triRunRows, S.stream)) { ERR("%s: the analysis failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

int hipSpTRSVCSR(spmat* dA, int uplo, int diag, const double* dB, double* dX) {
    const char* who = "hipSpTRSVCSR";
    const Ctx cx = libraryCtx();
    DevMat* d = triHandle(dA, uplo, who);
    if (!d) return EXIT_FAILURE;
    if (!dB || !dX) { ERR("%s: %s is NULL", who, !dB ? "dB" : "dX"); return EXIT_FAILURE; }
    if (diag != SPMV_DIAG_STORED && diag != SPMV_DIAG_UNIT) { ERR("%s: unknown diag %d", who, diag); return EXIT_FAILURE; }
    if (dB != dX && overlaps(dB, dX, d->M * sizeof(double))) { ERR("%s: dB and dX overlap without being equal", who); return EXIT_FAILURE; }
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    if (d->NZ && !d->AS && !d->unit) { ERR("%s: the handle has no value array", who); return EXIT_FAILURE; }
    if (!d->tri[uplo] && triAnalyse(d, uplo, S.triRunRows, cx.stream)) { ERR("%s: the analysis failed", who); return EXIT_FAILURE; }
    spmvTriInfo info;
    triInfo(d, uplo, &info);
    if (diag == SPMV_DIAG_STORED && info.firstBadDiag >= 0) {
        ERR("%s: row %ld does not hold exactly one stored diagonal entry (SPMV_DIAG_STORED needs one in every row)", who,
            info.firstBadDiag);
        return EXIT_FAILURE;
    }
    Launch L(cx, dim3(1), dim3(1));
    dim3 grid(1), block(1);
    if (enqueueTrsv(d, uplo, diag, dB, dX, cx.stream, &grid, &block)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    L.shape(grid, block);
    return L.finish(who);
}

// a block of right-hand sides (contract in spmvHip.h, design in DESIGN.md section 26)
int hipSpTRSMCSR(spmat* dA, int uplo, int diag, unsigned k, const double* dB, size_t ldb, int bLayout, double* dX, size_t ldx,
                 int xLayout) {
    const char* who = "hipSpTRSMCSR";
    const Ctx cx = libraryCtx();
    DevMat* d = triHandle(dA, uplo, who);
    if (!d) return EXIT_FAILURE;
    if (!dB || !dX) { ERR("%s: %s is NULL", who, !dB ? "dB" : "dX"); return EXIT_FAILURE; }
    if (diag != SPMV_DIAG_STORED && diag != SPMV_DIAG_UNIT) { ERR("%s: unknown diag %d", who, diag); return EXIT_FAILURE; }
    if (k == 0) { ERR("%s: k = 0 columns", who); return EXIT_FAILURE; }
    Dense B, X;
    if (!denseOperand(who, "ldb", d->M, k, dB, ldb, bLayout, &B) || !denseOperand(who, "ldx", d->M, k, dX, ldx, xLayout, &X)) return EXIT_FAILURE;
    // in place is the same block: a row reads B only at its own (i, c) and writes X only there; anything else that shares
    // memory is refused
    if (denseShare(k, d->M, B, d->M, X, true)) {
        ERR("%s: dB and dX overlap without being the same block (same pointer, layout and leading dimension)", who);
        return EXIT_FAILURE;
    }
    if (d->M == 0) return nothingToLaunch(cx, d, nullptr);
    if (d->NZ && !d->AS && !d->unit) { ERR("%s: the handle has no value array", who); return EXIT_FAILURE; }
    if (!d->tri[uplo] && triAnalyse(d, uplo, S.triRunRows, cx.stream)) { ERR("%s: the analysis failed", who); return EXIT_FAILURE; }
    spmvTriInfo info;
    triInfo(d, uplo, &info);
    if (diag == SPMV_DIAG_STORED && info.firstBadDiag >= 0) {
        ERR("%s: row %ld does not hold exactly one stored diagonal entry (SPMV_DIAG_STORED needs one in every row)", who,
            info.firstBadDiag);
        return EXIT_FAILURE;
    }
    Launch L(cx, dim3(1), dim3(1));
    dim3 grid(1), block(1);
    const int rc = k == 1 && B.sr() == 1 && X.sr() == 1              // one plain vector: the single solve
                       ? enqueueTrsv(d, uplo, diag, dB, dX, cx.stream, &grid, &block)
                       : enqueueTrsm(d, uplo, diag, k, B, X, cx.stream, &grid, &block);
    if (rc) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    L.shape(grid, block);
    return L.finish(who);
}

int spmvHipTriInfo(spmat* dA, int uplo, spmvTriInfo* info) {
    const char* who = "spmvHipTriInfo";
    DevMat* d = descOf(dA, who);
    if (!d) return EXIT_FAILURE;
    if (!info) { ERR("%s: info is NULL", who); return EXIT_FAILURE; }
    if (uplo != SPMV_TRI_LOWER && uplo != SPMV_TRI_UPPER) { ERR("%s: unknown uplo %d", who, uplo); return EXIT_FAILURE; }
    triInfo(d, uplo, info);
    return EXIT_SUCCESS;
}

// ---- ILU(0)
int hipSpILU0CSR(spmat* dA) {
    const char* who = "hipSpILU0CSR";
    const auto t0 = std::chrono::steady_clock::now();
    DevMat* d = triHandle(dA, SPMV_TRI_LOWER, who);
    if (!d) return EXIT_FAILURE;
    if (d->NZ && !d->AS) { ERR("%s: the handle has no value array", who); return EXIT_FAILURE; }
    if (d->M) {
        if (!d->iluChecked) {
            long row = -1;
            if (iluUnsortedRow(d, S.stream, &row)) { ERR("%s: the pattern check failed", who); return EXIT_FAILURE; }
            d->iluUnsortedRow = row;
            d->iluChecked = true;
        }
        if (!d->tri[SPMV_TRI_LOWER] && triAnalyse(d, SPMV_TRI_LOWER, S.triRunRows, S.stream)) {
            ERR("%s: the analysis failed", who);
            return EXIT_FAILURE;
        }
        const long unsorted = d->iluUnsortedRow, badDiag = d->tri[SPMV_TRI_LOWER]->info.firstBadDiag;
        if (unsorted >= 0 || badDiag >= 0) {
            const bool first = unsorted >= 0 && (badDiag < 0 || unsorted <= badDiag);
            d->ilu.firstBadRow = first ? unsorted : badDiag;
            if (first) ERR("%s: row %ld: its columns are not strictly ascending (unsorted, or a repeated column)", who, unsorted);
            else       ERR("%s: row %ld does not hold exactly one stored diagonal entry", who, badDiag);
            return EXIT_FAILURE;
        }
        d->ilu.firstBadRow = -1;
        if (!d->iluPending && iluFactor(d, S.iluGroup, S.stream)) { ERR("%s: the factorisation failed", who); return EXIT_FAILURE; }
        if (updateValues(dA, nullptr, true, true, S.stream, who)) {
            d->iluPending = true;                        // (after updateValues, which clears it as every value update does)
            ERR("%s: the factors are in place, but bringing the handle's unit flag and formats up to them failed: call again", who);
            return EXIT_FAILURE;
        }
    } else {
        d->ilu.zeroPivot = d->ilu.firstBadRow = -1;
        d->ilu.levels = d->ilu.launches = d->ilu.longRows = 0;
    }
    ++d->ilu.factorisations;
    d->ilu.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return EXIT_SUCCESS;
}

int spmvHipIlu0Info(spmat* dA, spmvIluInfo* info) {
    const char* who = "spmvHipIlu0Info";
    DevMat* d = descOf(dA, who);
    if (!d) return EXIT_FAILURE;
    if (!info) { ERR("%s: info is NULL", who); return EXIT_FAILURE; }
    *info = d->ilu;
    return EXIT_SUCCESS;
}

// ---- multi-colour ordering and vector permutation
int spmvHipColourCSR(spmat* dA, const spmvColourOpts* opts, uint32_t* dColour, uint32_t* dPerm, spmvColourInfo* info) {
    const char* who = "spmvHipColourCSR";
    DevMat* d = squareCsrOf(dA, who, "the handle is an ELL handle (only CSR handles are coloured)");
    if (!d) return EXIT_FAILURE;
    const int order = opts ? opts->order : SPMV_COLOUR_NATURAL;
    if (order != SPMV_COLOUR_NATURAL && order != SPMV_COLOUR_HASH) { ERR("%s: unknown order %d", who, order); return EXIT_FAILURE; }
    if (colourCsr(d, order, opts ? opts->seed : 0u, S.colourK, dColour, dPerm, info, S.stream)) { ERR("%s: the colouring failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

// ---- reverse Cuthill-McKee ordering
int spmvHipRcmCSR(spmat* dA, const spmvRcmOpts* opts, uint32_t* dPerm, spmvRcmInfo* info) {
    const char* who = "spmvHipRcmCSR";
    DevMat* d = squareCsrOf(dA, who, "the handle is an ELL handle (only CSR handles are ordered)");
    if (!d) return EXIT_FAILURE;
    const int start = opts ? opts->start : SPMV_RCM_START_PERIPHERAL;
    if (start != SPMV_RCM_START_MIN_DEGREE && start != SPMV_RCM_START_PERIPHERAL) { ERR("%s: unknown start %d", who, start); return EXIT_FAILURE; }
    const unsigned maxPasses = opts && opts->maxPasses ? opts->maxPasses : 8u;
    spmvRcmInfo out{};
    if (rcmCsr(d, start == SPMV_RCM_START_PERIPHERAL, maxPasses, opts && opts->forward, S.rcmT, dPerm, &out, S.stream)) {
        ERR("%s: the ordering failed", who);
        return EXIT_FAILURE;
    }
    if (info) *info = out;
    return EXIT_SUCCESS;
}

int spmvHipVecPermute(size_t n, const uint32_t* dPerm, const double* dIn, double* dOut, int inverse) {
    const char* who = "spmvHipVecPermute";
    const Ctx cx = libraryCtx();
    if (!ready(who)) return EXIT_FAILURE;
    if (n && (!dPerm || !dIn || !dOut)) { ERR("%s: %s is NULL", who, !dPerm ? "dPerm" : !dIn ? "dIn" : "dOut"); return EXIT_FAILURE; }
    if (n >= (1ull << 32)) { ERR("%s: n=%zu does not fit the 32-bit ids of a permutation", who, n); return EXIT_FAILURE; }
    if (overlaps(dIn, dOut, n * sizeof(double))) { ERR("%s: dIn and dOut are the same vector or overlap", who); return EXIT_FAILURE; }
    Launch L(cx, grid2d((n + 255) / 256, 256), dim3(256));
    if (enqueueVecPermute(n, dPerm, dIn, dOut, inverse != 0, cx.stream)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    return L.finish(who);
}

// ---- the dots
int spmvHipDot(size_t n, const double* dU, const double* dV, double* dResult) {
    const char* who = "spmvHipDot";
    const Ctx cx = libraryCtx();
    if (!ready(who)) return EXIT_FAILURE;
    if (!dResult || (n && (!dU || !dV))) { ERR("%s: %s is NULL", who, !dResult ? "dResult" : !dU ? "dU" : "dV"); return EXIT_FAILURE; }
    Launch L(cx, dim3(1), dim3(256));
    if (enqueueDot(n, dU, dV, dResult, cx.stream)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    return L.finish(who);
}

int spmvHipMultiDot(size_t n, unsigned k, const double* dV, size_t ldv, const double* dW, double* dH) {
    const char* who = "spmvHipMultiDot";
    const Ctx cx = libraryCtx();
    if (!ready(who)) return EXIT_FAILURE;
    if (!dH || (n && (!dV || !dW))) { ERR("%s: %s is NULL", who, !dH ? "dH" : !dV ? "dV" : "dW"); return EXIT_FAILURE; }
    if (k == 0) { ERR("%s: k = 0 columns", who); return EXIT_FAILURE; }
    if (ldv < n) { ERR("%s: ldv=%zu < n=%zu", who, ldv, n); return EXIT_FAILURE; }
    Launch L(cx, dim3((k + 1) / 2), dim3(256));
    if (enqueueMultiDot(n, k, dV, ldv, dW, dH, cx.stream)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    return L.finish(who);
}

// ---- aggregation multigrid
int spmvHipAggregateCSR(spmat* dA, const spmvAggOpts* opts, uint32_t* dAgg, spmvAggInfo* info) {
    const char* who = "spmvHipAggregateCSR";
    DevMat* d = squareCsrOf(dA, who, "the handle is an ELL handle (only CSR handles are aggregated)");
    if (!d) return EXIT_FAILURE;
    if (d->M && !dAgg) { ERR("%s: dAgg is NULL", who); return EXIT_FAILURE; }
    spmvAggInfo out{};
    if (aggregateCsr(d, opts ? opts->seed : 0u, S.aggK, dAgg, &out, S.stream)) { ERR("%s: the aggregation failed", who); return EXIT_FAILURE; }
    if (info) *info = out;
    return EXIT_SUCCESS;
}

// the three setups: the plan holds the kind and the caller's numbers of that kind (what a kind does not use is 0, which
// passes every check here); the library's settings are filled in here
static int amgSetup(const char* who, spmat* dA, const spmvAmgOpts* opts, AmgPlan plan, spmat* dM, spmvAmgInfo* info) {
    if (!ready(who)) return EXIT_FAILURE;
    if (!dA || !dM) { ERR("%s: %s is NULL", who, !dA ? "dA" : "dM"); return EXIT_FAILURE; }
    if (dM == dA) { ERR("%s: dM is the source handle itself", who); return EXIT_FAILURE; }
    DevMat* a = squareCsrOf(dA, who, "the handle is an ELL handle (only CSR handles are aggregated)");
    if (!a) return EXIT_FAILURE;
    if (a->NZ && (!a->JA || !a->AS)) { ERR("%s: the source has no column or value array", who); return EXIT_FAILURE; }
    if (opts && opts->maxLevels > SPMV_AMG_MAX_LEVELS) { ERR("%s: maxLevels %u is above %d", who, opts->maxLevels, SPMV_AMG_MAX_LEVELS); return EXIT_FAILURE; }
    if (opts && !(opts->omega >= 0.0 && std::isfinite(opts->omega))) { ERR("%s: omega %g is negative or not finite", who, opts->omega); return EXIT_FAILURE; }
    if (!(plan.omegaP >= 0.0 && std::isfinite(plan.omegaP))) { ERR("%s: omegaP %g is negative or not finite", who, plan.omegaP); return EXIT_FAILURE; }
    if (!(plan.theta >= 0.0 && std::isfinite(plan.theta))) { ERR("%s: theta %g is negative or not finite", who, plan.theta); return EXIT_FAILURE; }
    if (!(plan.thetaScale >= 0.0 && plan.thetaScale <= 1.0)) {
        ERR("%s: thetaScale %g is negative, above 1 or not finite", who, plan.thetaScale);
        return EXIT_FAILURE;
    }
    plan.fuseMax = S.amgFuseMax;
    plan.K = S.aggK;
    DevMat* m = new DevMat;
    m->M = m->N = a->M;
    setOrigin(m, Origin::HIERARCHY, a);
    if (amgBuild(dA, opts, plan, m, S.stream)) { ERR("%s: building the hierarchy failed", who); freeDesc(m); return EXIT_FAILURE; }
    publish(dM, m, m->M, m->N, 0, 0);
    if (info) *info = *amgInfo(m);
    return EXIT_SUCCESS;
}

int spmvHipAmgSetup(spmat* dA, const spmvAmgOpts* opts, spmat* dM, spmvAmgInfo* info) {
    return amgSetup("spmvHipAmgSetup", dA, opts, AmgPlan{}, dM, info);
}
int spmvHipAmgSetupSmoothed(spmat* dA, const spmvAmgOpts* opts, const spmvAmgSmoothOpts* smooth, spmat* dM, spmvAmgInfo* info) {
    return amgSetup("spmvHipAmgSetupSmoothed", dA, opts, AmgPlan{AmgKind::SMOOTHED, smooth ? smooth->omegaP : 0.0}, dM, info);
}
int spmvHipAmgSetupStrength(spmat* dA, const spmvAmgOpts* opts, const spmvAmgSmoothOpts* smooth, const spmvAmgStrengthOpts* strength, spmat* dM,
                            spmvAmgInfo* info) {
    AmgPlan plan{AmgKind::STRENGTH, smooth ? smooth->omegaP : 0.0};
    if (strength) { plan.theta = strength->theta; plan.thetaScale = strength->thetaScale; }
    return amgSetup("spmvHipAmgSetupStrength", dA, opts, plan, dM, info);
}

int spmvHipAmgRefresh(spmat* dM, spmat* dA) {
    const char* who = "spmvHipAmgRefresh";
    DevMat* a = nullptr;
    DevMat* m = hierarchyOf(dM, dA, who, &a);
    if (!m) return EXIT_FAILURE;
    if (amgRefresh(m, dA, S.stream)) { ERR("%s: recomputing the hierarchy failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

int spmvHipAmgApply(spmat* dM, spmat* dA, const double* dR, double* dZ) {
    const char* who = "spmvHipAmgApply";
    const Ctx cx = libraryCtx();
    DevMat* a = nullptr;
    DevMat* m = hierarchyOf(dM, dA, who, &a);
    if (!m) return EXIT_FAILURE;
    if (!dR || !dZ) { ERR("%s: %s is NULL", who, !dR ? "dR" : "dZ"); return EXIT_FAILURE; }
    if (a->M != m->M) { ERR("%s: dA has %lu rows, dM %lu", who, (unsigned long)a->M, (unsigned long)m->M); return EXIT_FAILURE; }
    if (overlaps(dR, dZ, m->M * sizeof(double))) { ERR("%s: dR and dZ are the same vector or overlap", who); return EXIT_FAILURE; }
    if (m->M == 0) return nothingToLaunch(cx, m, nullptr);
    Launch L(cx, grid2d((m->M + KB - 1) / KB, KT), dim3(KT));
    if (enqueueAmgCycle(m, dA, dR, dZ, cx.stream, nullptr, nullptr)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    return L.finish(who);
}

// ---- the block cycle (contract in spmvHip.h, design in DESIGN.md section 33)
// the hierarchy m cannot run a block cycle of k columns: the line says why
static bool blockCycleRefused(const DevMat* m, unsigned k, const char* who) {
    uint32_t width = 0;
    uint64_t bytes = 0;
    bool gs = false;
    amgBlockState(m, &width, &bytes, &gs);
    if (width < k) {
        ERR("%s: dM is a multigrid hierarchy with a block workspace of width %u, k = %u columns: spmvHipAmgSetBlockWidth(dM, dA, width >= k) gives "
            "it one (without, its cycle takes one vector at a time)", who, width, k);
        return true;
    }
    if (gs) {
        ERR("%s: dM is a multigrid hierarchy with a Gauss-Seidel level: the block cycle has no colour sweeps (spmvHipAmgSetSmoother with JACOBI "
            "or CHEBYSHEV first; the width is kept)", who);
        return true;
    }
    return false;
}

int spmvHipAmgSetBlockWidth(spmat* dM, spmat* dA, unsigned width) {
    const char* who = "spmvHipAmgSetBlockWidth";
    DevMat* a = nullptr;
    DevMat* m = hierarchyOf(dM, dA, who, &a);
    if (!m) return EXIT_FAILURE;
    if (amgSetBlockWidth(m, width, S.stream)) { ERR("%s: the block workspace was not set", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

int spmvHipAmgBlock(spmat* dM, spmvAmgBlockInfo* info) {
    DevMat* m = hierarchyLevel(dM, "spmvHipAmgBlock", 0, nullptr, !info);
    if (!m) return EXIT_FAILURE;
    uint32_t width = 0;
    uint64_t bytes = 0;
    bool gs = false;
    amgBlockState(m, &width, &bytes, &gs);
    *info = spmvAmgBlockInfo{width, (ulong)bytes};
    return EXIT_SUCCESS;
}

int spmvHipAmgApplyBlock(spmat* dM, spmat* dA, unsigned k, const double* dR, size_t ldr, int rLayout, double* dZ, size_t ldz, int zLayout) {
    const char* who = "spmvHipAmgApplyBlock";
    const Ctx cx = libraryCtx();
    DevMat* a = nullptr;
    DevMat* m = hierarchyOf(dM, dA, who, &a);
    if (!m) return EXIT_FAILURE;
    if (!dR || !dZ) { ERR("%s: %s is NULL", who, !dR ? "dR" : "dZ"); return EXIT_FAILURE; }
    if (a->M != m->M) { ERR("%s: dA has %lu rows, dM %lu", who, (unsigned long)a->M, (unsigned long)m->M); return EXIT_FAILURE; }
    if (k == 0) { ERR("%s: k = 0 columns", who); return EXIT_FAILURE; }
    Dense R, Z;
    if (!denseOperand(who, "ldr", m->M, k, dR, ldr, rLayout, &R) || !denseOperand(who, "ldz", m->M, k, dZ, ldz, zLayout, &Z)) return EXIT_FAILURE;
    if (denseShare(k, m->M, R, m->M, Z)) { ERR("%s: dR and dZ overlap", who); return EXIT_FAILURE; }
    if (blockCycleRefused(m, k, who)) return EXIT_FAILURE;
    if (m->M == 0) return nothingToLaunch(cx, m, nullptr);
    Launch L(cx, grid2d((m->M + KB - 1) / KB * ((k + 15) / 16), KT), dim3(KT));
    if (enqueueAmgCycleBlock(m, a, k, R, Z, cx.stream, nullptr, nullptr)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    return L.finish(who);
}

// ---- the hierarchy stored in single precision (contract in spmvHip.h, design in DESIGN.md section 41)
int spmvHipAmgSetStorage(spmat* dM, spmat* dA, int storage) {
    const char* who = "spmvHipAmgSetStorage";
    DevMat* a = nullptr;
    DevMat* m = hierarchyOf(dM, dA, who, &a);
    if (!m) return EXIT_FAILURE;
    if (storage != SPMV_STORAGE_F64 && storage != SPMV_STORAGE_F32) {
        ERR("%s: storage %d is neither SPMV_STORAGE_F64 nor SPMV_STORAGE_F32", who, storage);
        return EXIT_FAILURE;
    }
    if (amgSetStorage(m, dA, storage, S.stream)) { ERR("%s: the storage was not set", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

int spmvHipAmgStorage(spmat* dM, spmvAmgStorageInfo* info) {
    DevMat* m = hierarchyLevel(dM, "spmvHipAmgStorage", 0, nullptr, !info);
    if (!m) return EXIT_FAILURE;
    amgStorage(m, info);
    return EXIT_SUCCESS;
}

int spmvHipAmgInfo(spmat* dM, spmvAmgInfo* info) {
    DevMat* m = hierarchyLevel(dM, "spmvHipAmgInfo", 0, nullptr, !info);
    if (!m) return EXIT_FAILURE;
    *info = *amgInfo(m);
    return EXIT_SUCCESS;
}

int spmvHipAmgLevel(spmat* dM, unsigned level, spmat* dAl, const uint32_t** dAgg, const double** dDinv) {
    DevMat* m = hierarchyLevel(dM, "spmvHipAmgLevel", level, nullptr);
    if (!m) return EXIT_FAILURE;
    amgLevel(m, level, dAl, dAgg, dDinv);
    return EXIT_SUCCESS;
}

int spmvHipAmgProlongator(spmat* dM, unsigned level, spmat* dPl, spmat* dRl, double* omegaP) {
    DevMat* m = hierarchyLevel(dM, "spmvHipAmgProlongator", level, "prolongator");
    if (!m) return EXIT_FAILURE;
    amgProlongator(m, level, dPl, dRl, omegaP);
    return EXIT_SUCCESS;
}

int spmvHipAmgStrength(spmat* dM, unsigned level, spmat* dFl, double* theta) {
    const char* who = "spmvHipAmgStrength";
    DevMat* m = hierarchyLevel(dM, who, level, "filtered matrix");
    if (!m) return EXIT_FAILURE;
    if (!amgIsStrength(m)) { ERR("%s: dM was not made by spmvHipAmgSetupStrength", who); return EXIT_FAILURE; }
    amgStrength(m, level, dFl, theta);
    return EXIT_SUCCESS;
}

int spmvHipAmgSetSmoother(spmat* dM, spmat* dA, const spmvAmgSmootherOpts* opts) {
    const char* who = "spmvHipAmgSetSmoother";
    DevMat* a = nullptr;
    DevMat* m = hierarchyOf(dM, dA, who, &a);
    if (!m) return EXIT_FAILURE;
    if (opts) {
        if (opts->kind != SPMV_AMG_SMOOTHER_JACOBI && opts->kind != SPMV_AMG_SMOOTHER_CHEBYSHEV) { ERR("%s: kind %d is no smoother", who, opts->kind); return EXIT_FAILURE; }
        if (opts->eigRatio != 0.0 && !(opts->eigRatio > 1.0 && std::isfinite(opts->eigRatio))) {
            ERR("%s: eigRatio %g is not finite or not above 1", who, opts->eigRatio);
            return EXIT_FAILURE;
        }
        if (!(opts->lambdaScale >= 0.0 && std::isfinite(opts->lambdaScale))) { ERR("%s: lambdaScale %g is negative or not finite", who, opts->lambdaScale); return EXIT_FAILURE; }
        for (unsigned nu : {opts->nu1, opts->nu2, opts->nuCoarse})
            if (nu > SPMV_AMG_MAX_DEGREE && nu != SPMV_AMG_NO_SWEEPS) { ERR("%s: %u sweeps are above %d", who, nu, SPMV_AMG_MAX_DEGREE); return EXIT_FAILURE; }
    }
    if (amgSetSmoother(m, dA, opts, S.stream)) { ERR("%s: the smoother was not set", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

int spmvHipAmgSmoother(spmat* dM, unsigned level, spmvAmgSmootherInfo* info) {
    DevMat* m = hierarchyLevel(dM, "spmvHipAmgSmoother", level, nullptr, !info);
    if (!m) return EXIT_FAILURE;
    amgSmoother(m, level, info);
    return EXIT_SUCCESS;
}

int spmvHipAmgSetGaussSeidel(spmat* dM, spmat* dA, const spmvAmgGsOpts* opts) {
    const char* who = "spmvHipAmgSetGaussSeidel";
    DevMat* a = nullptr;
    DevMat* m = hierarchyOf(dM, dA, who, &a);
    if (!m) return EXIT_FAILURE;
    if (opts) {
        if (opts->order != SPMV_COLOUR_NATURAL && opts->order != SPMV_COLOUR_HASH) { ERR("%s: unknown order %d", who, opts->order); return EXIT_FAILURE; }
        if (!(opts->omega >= 0.0 && std::isfinite(opts->omega))) { ERR("%s: omega %g is negative or not finite", who, opts->omega); return EXIT_FAILURE; }
        for (unsigned nu : {opts->nu1, opts->nu2, opts->nuCoarse})
            if (nu > SPMV_AMG_MAX_DEGREE && nu != SPMV_AMG_NO_SWEEPS) { ERR("%s: %u sweeps are above %d", who, nu, SPMV_AMG_MAX_DEGREE); return EXIT_FAILURE; }
    }
    if (amgSetGaussSeidel(m, dA, opts, S.amgGsSmallRows, S.amgGsLanes, S.colourK, S.stream)) { ERR("%s: the smoother was not set", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

int spmvHipAmgGaussSeidel(spmat* dM, unsigned level, spmvAmgGsInfo* info) {
    DevMat* m = hierarchyLevel(dM, "spmvHipAmgGaussSeidel", level, nullptr, !info);
    if (!m) return EXIT_FAILURE;
    amgGaussSeidel(m, level, info);
    return EXIT_SUCCESS;
}

// ---- Krylov solves
// dM as the preconditioner of a solve on the checked dA (a): NULL (none), a multigrid hierarchy of dA, an approximate-inverse
// factor of dA's size, or a square CSR handle whose two triangles are applied (analysed here unless it runs by sweeps).
// What hipSpCGCSR, hipSpBiCGStabCSR, hipSpGMRESCSR, their block forms and hipSpDavidsonCSR check alike; false: refused.
static bool precondOf(const char* who, spmat* dM, DevMat* a, DevMat** pm) {
    DevMat* m = dM ? anyDescOf(dM, who) : nullptr;
    if (dM && !m) return false;
    if (m && m->origin == Origin::HIERARCHY) {               // a multigrid hierarchy: M^-1 v is its cycle
        if (!madeBy(m, Origin::HIERARCHY, a, nullptr, who, "dM", "dA")) return false;
    } else if (m && m->origin == Origin::FSAI) {             // an approximate-inverse factor: M^-1 v = G^T (G v), of any source of dA's size
        if (m->M != a->M) { ERR("%s: dM has %lu rows, dA %lu", who, (unsigned long)m->M, (unsigned long)a->M); return false; }
    } else if (dM) {
        if (!(m = triHandle(dM, SPMV_TRI_LOWER, who))) return false;
        if (m->M != a->M) { ERR("%s: dM has %lu rows, dA %lu", who, (unsigned long)m->M, (unsigned long)a->M); return false; }
        if (m->NZ && !m->AS && !m->unit) { ERR("%s: dM has no value array", who); return false; }
        const bool sweeps = triSweepsMode(m);                // applied by Jacobi sweeps (spmvHipTriSetApply): no level sets
        for (int uplo : {SPMV_TRI_LOWER, SPMV_TRI_UPPER})
            if (!sweeps && m->M && !m->tri[uplo] && triAnalyse(m, uplo, S.triRunRows, S.stream)) { ERR("%s: the analysis of dM failed", who); return false; }
        const long badDiag = !m->M ? -1 : sweeps ? m->sweep->firstBadDiag : m->tri[SPMV_TRI_UPPER]->info.firstBadDiag;
        if (badDiag >= 0) {
            ERR("%s: row %ld of dM does not hold exactly one stored diagonal entry (M^-1 divides by it)", who, badDiag);
            return false;
        }
    }
    *pm = m;
    return true;
}

// what the three solvers check alike: 0 go on (a, m set), 1 refused, 2 done (M = 0)
static int krylovArgs(const char* who, spmat* dA, spmat* dM, const double* dB, double* dX, const void* optsPtr, double tol, ulong maxIter,
                      double* history, spmvKrylovInfo* info, DevMat** pa, DevMat** pm) {
    if (!ready(who)) return EXIT_FAILURE;
    if (!dB || !dX || !optsPtr) { ERR("%s: %s is NULL", who, !dB ? "dB" : !dX ? "dX" : "opts"); return EXIT_FAILURE; }
    DevMat* a = csrOf(dA, who, "dA is an ELL handle (only CSR handles are solved)");
    if (!a) return EXIT_FAILURE;
    if (a->M != a->N) { ERR("%s: M=%lu != N=%lu: dA is not square", who, (unsigned long)a->M, (unsigned long)a->N); return EXIT_FAILURE; }
    if (a->NZ && !a->AS && !a->unit) { ERR("%s: dA has no value array", who); return EXIT_FAILURE; }
    if (overlaps(dB, dX, a->M * sizeof(double))) { ERR("%s: dB and dX overlap", who); return EXIT_FAILURE; }
    if (!(tol >= 0.0)) { ERR("%s: tol %g is negative or NaN", who, tol); return EXIT_FAILURE; }
    if (history && maxIter >= (SIZE_MAX / sizeof(double)) - 1) {
        ERR("%s: a history of maxIter + 1 = %lu + 1 doubles does not fit", who, (unsigned long)maxIter);
        return EXIT_FAILURE;
    }
    DevMat* m = nullptr;
    if (!precondOf(who, dM, a, &m)) return EXIT_FAILURE;
    *pa = a;
    *pm = m;
    if (a->M == 0) {
        if (history) history[0] = 0.0;
        if (info) *info = spmvKrylovInfo{SPMV_KRYLOV_CONVERGED, 0, 0.0, 0.0, 0, 0, 0.0};
        return 2;
    }
    return 0;
}

static int krylov(int bicg, spmat* dA, spmat* dM, const double* dB, double* dX, const spmvKrylovOpts* opts, spmvKrylovInfo* info) {
    const char* who = bicg ? "hipSpBiCGStabCSR" : "hipSpCGCSR";
    DevMat* a = nullptr;
    DevMat* m = nullptr;
    const int rc = krylovArgs(who, dA, dM, dB, dX, opts, opts ? opts->tol : 0.0, opts ? opts->maxIter : 0, opts ? opts->history : nullptr, info, &a, &m);
    if (rc) return rc == 2 ? EXIT_SUCCESS : EXIT_FAILURE;
    if (krylovSolve(bicg, dA, a, m, dB, dX, opts, info, S.krylovK[bicg], S.stream)) { ERR("%s: the solve failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}
int hipSpCGCSR(spmat* dA, spmat* dM, const double* dB, double* dX, const spmvKrylovOpts* opts, spmvKrylovInfo* info) { return krylov(0, dA, dM, dB, dX, opts, info); }
int hipSpBiCGStabCSR(spmat* dA, spmat* dM, const double* dB, double* dX, const spmvKrylovOpts* opts, spmvKrylovInfo* info) { return krylov(1, dA, dM, dB, dX, opts, info); }

// ---- blocks of right-hand sides (contract in spmvHip.h, design in DESIGN.md section 27)
int spmvHipBlockDot(size_t n, unsigned k, const double* dU, size_t ldu, int uLayout, const double* dV, size_t ldv, int vLayout,
                    double* dH) {
    const char* who = "spmvHipBlockDot";
    const Ctx cx = libraryCtx();
    if (!ready(who)) return EXIT_FAILURE;
    if (!dH || (n && (!dU || !dV))) { ERR("%s: %s is NULL", who, !dH ? "dH" : !dU ? "dU" : "dV"); return EXIT_FAILURE; }
    if (k == 0) { ERR("%s: k = 0 columns", who); return EXIT_FAILURE; }
    Dense U, V;
    if (!denseOperand(who, "ldu", n, k, dU, ldu, uLayout, &U) || !denseOperand(who, "ldv", n, k, dV, ldv, vLayout, &V)) return EXIT_FAILURE;
    Launch L(cx, dim3(k), dim3(KT));
    if (enqueueBlockDot(n, k, U, V, dH, cx.stream)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    return L.finish(who);
}

static int krylovBlock(int bicg, spmat* dA, spmat* dM, unsigned k, const double* dB, size_t ldb, int bLayout, double* dX, size_t ldx,
                       int xLayout, const spmvKrylovOpts* opts, spmvKrylovColumn* cols, spmvKrylovInfo* info) {
    const char* who = bicg ? "hipSpBiCGStabBlockCSR" : "hipSpCGBlockCSR";
    if (!ready(who)) return EXIT_FAILURE;
    if (k == 0) { ERR("%s: k = 0 columns", who); return EXIT_FAILURE; }
    if (dM && dM->dev && dM->dev != SPMAT_TAG_ELL_TRANSPOSED) {
        const DevMat* h = anyDescOf(dM, who);
        // a hierarchy is taken when it has the workspace of a block cycle of k columns (spmvHipAmgSetBlockWidth)
        if (h && h->origin == Origin::HIERARCHY && blockCycleRefused(h, k, who)) return EXIT_FAILURE;
        // a handle applied by sweeps is taken when its workspace holds k columns (spmvHipTriSetApply, spmvHipTriSweepsPrepare)
        if (h && triSweepsMode(h) && h->sweep->width < k) {
            ERR("%s: dM is applied by sweeps with a workspace of width %u, k = %u columns: spmvHipTriSweepsPrepare(dM, width >= k) widens it", who,
                h->sweep->width, k);
            return EXIT_FAILURE;
        }
    }
    DevMat* a = nullptr;
    DevMat* m = nullptr;
    // (history and info stay with this function: they are per column)
    const int rc = krylovArgs(who, dA, dM, dB, dX, opts, opts ? opts->tol : 0.0, opts ? opts->maxIter : 0, nullptr, nullptr, &a, &m);
    if (rc == EXIT_FAILURE) return EXIT_FAILURE;
    Dense B, X;
    if (!denseOperand(who, "ldb", a->M, k, dB, ldb, bLayout, &B) || !denseOperand(who, "ldx", a->M, k, dX, ldx, xLayout, &X)) return EXIT_FAILURE;
    if (denseShare(k, a->M, B, a->M, X)) { ERR("%s: dB and dX overlap", who); return EXIT_FAILURE; }
    if (opts->history && opts->maxIter >= (SIZE_MAX / sizeof(double)) / k - 1) {
        ERR("%s: a history of k * (maxIter + 1) = %u * (%lu + 1) doubles does not fit", who, k, (unsigned long)opts->maxIter);
        return EXIT_FAILURE;
    }
    if (rc == 2) {                                                       // M = 0: every column CONVERGED, 0; no kernel
        for (unsigned c = 0; c < k; ++c) {
            if (opts->history) opts->history[(size_t)c * (opts->maxIter + 1)] = 0.0;
            if (cols) cols[c] = spmvKrylovColumn{SPMV_KRYLOV_CONVERGED, 0, 0.0, 0.0};
        }
        if (info) *info = spmvKrylovInfo{SPMV_KRYLOV_CONVERGED, 0, 0.0, 0.0, 0, 0, 0.0};
        return EXIT_SUCCESS;
    }
    if (k == 1 && B.sr() == 1 && X.sr() == 1) {                          // one plain vector: the single solve
        spmvKrylovInfo one{};
        if (krylovSolve(bicg, dA, a, m, dB, dX, opts, &one, S.krylovBlockK[bicg], S.stream)) { ERR("%s: the solve failed", who); return EXIT_FAILURE; }
        if (cols) cols[0] = spmvKrylovColumn{one.status, one.iterations, one.rr, one.bb};
        if (info) *info = one;
        return EXIT_SUCCESS;
    }
    if (krylovBlockSolve(bicg, a, m, k, B, X, opts, cols, info, S.krylovBlockK[bicg], S.stream)) { ERR("%s: the solve failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}
int hipSpCGBlockCSR(spmat* dA, spmat* dM, unsigned k, const double* dB, size_t ldb, int bLayout, double* dX, size_t ldx, int xLayout,
                    const spmvKrylovOpts* opts, spmvKrylovColumn* cols, spmvKrylovInfo* info) {
    return krylovBlock(0, dA, dM, k, dB, ldb, bLayout, dX, ldx, xLayout, opts, cols, info);
}
int hipSpBiCGStabBlockCSR(spmat* dA, spmat* dM, unsigned k, const double* dB, size_t ldb, int bLayout, double* dX, size_t ldx,
                          int xLayout, const spmvKrylovOpts* opts, spmvKrylovColumn* cols, spmvKrylovInfo* info) {
    return krylovBlock(1, dA, dM, k, dB, ldb, bLayout, dX, ldx, xLayout, opts, cols, info);
}

int hipSpGMRESCSR(spmat* dA, spmat* dM, const double* dB, double* dX, const spmvGmresOpts* opts, spmvKrylovInfo* info) {
    const char* who = "hipSpGMRESCSR";
    if (opts && (opts->restart == 0 || opts->restart > 64)) {
        if (ready(who)) ERR("%s: restart %u is not in 1 .. 64", who, opts->restart);
        return EXIT_FAILURE;
    }
    DevMat* a = nullptr;
    DevMat* m = nullptr;
    const int rc = krylovArgs(who, dA, dM, dB, dX, opts, opts ? opts->tol : 0.0, opts ? opts->maxIter : 0, opts ? opts->history : nullptr, info, &a, &m);
    if (rc) return rc == 2 ? EXIT_SUCCESS : EXIT_FAILURE;
    if (gmresSolve(dA, a, m, dB, dX, opts, info, S.gmresFused, S.stream)) { ERR("%s: the solve failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

// ---- the basis rotation and the extreme eigenpairs (contract in spmvHip.h, design in DESIGN.md section 39)
// bytes spanned by a column-major rows x cols block of leading dimension ld (0 for an empty block)
static uint64_t colMajorSpan(uint64_t rows, unsigned cols, uint64_t ld) { return rows && cols ? ((cols - 1) * ld + rows) * sizeof(double) : 0; }
static bool spansShare(const void* p, uint64_t pBytes, const void* q, uint64_t qBytes) {
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    return pBytes && qBytes && p0 < q0 + qBytes && q0 < p0 + pBytes;
}

int spmvHipBlockCombine(size_t n, unsigned m, unsigned k, const double* dV, size_t ldv, const double* dS, size_t lds, double* dY,
                        size_t ldy) {
    const char* who = "spmvHipBlockCombine";
    const Ctx cx = libraryCtx();
    if (!ready(who)) return EXIT_FAILURE;
    if (n && (!dV || !dS || !dY)) { ERR("%s: %s is NULL", who, !dV ? "dV" : !dS ? "dS" : "dY"); return EXIT_FAILURE; }
    if (m == 0 || m > 64 || k == 0 || k > 64) { ERR("%s: m=%u, k=%u: both must be in 1 .. 64", who, m, k); return EXIT_FAILURE; }
    if (ldv < n || ldy < n || lds < m) { ERR("%s: ldv=%zu, ldy=%zu (n=%zu) or lds=%zu (m=%u) is too small", who, ldv, ldy, n, lds, m); return EXIT_FAILURE; }
    const uint64_t vBytes = colMajorSpan(n, m, ldv), yBytes = colMajorSpan(n, k, ldy);
    if (n && dY == dV) {
        if (k > m || ldy != ldv) { ERR("%s: in place (dY == dV) needs k <= m and ldy == ldv", who); return EXIT_FAILURE; }
    } else if (spansShare(dV, vBytes, dY, yBytes)) {
        ERR("%s: dV and dY overlap without being the same block", who);
        return EXIT_FAILURE;
    }
    if (spansShare(dS, colMajorSpan(m, k, lds), dY, yBytes)) { ERR("%s: dS and dY overlap", who); return EXIT_FAILURE; }
    Launch L(cx, dim3(1), dim3(256));
    dim3 grid(1);
    if (enqueueBlockCombine(n, m, k, dV, ldv, dS, lds, dY, ldy, cx.stream, &grid)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    L.shape(grid, dim3(256));
    return L.finish(who);
}

int hipSpLanczosCSR(spmat* dA, const double* dV0, const spmvLanczosOpts* opts, double* dX, size_t ldx, double* theta, double* res,
                    spmvLanczosInfo* info) {
    const char* who = "hipSpLanczosCSR";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dV0 || !opts || !dX || !theta || !res) {
        ERR("%s: %s is NULL", who, !dV0 ? "dV0" : !opts ? "opts" : !dX ? "dX" : !theta ? "theta" : "res");
        return EXIT_FAILURE;
    }
    DevMat* a = csrOf(dA, who, "dA is an ELL handle (only CSR handles are solved)");
    if (!a) return EXIT_FAILURE;
    if (a->M != a->N) { ERR("%s: M=%lu != N=%lu: dA is not square", who, (unsigned long)a->M, (unsigned long)a->N); return EXIT_FAILURE; }
    if (a->NZ && !a->AS && !a->unit) { ERR("%s: dA has no value array", who); return EXIT_FAILURE; }
    if (opts->nev == 0 || opts->nev >= opts->ncv || opts->ncv > 64 || opts->ncv > a->M) {
        ERR("%s: nev=%u, ncv=%u, M=%lu: 1 <= nev < ncv <= min(64, M) is required", who, opts->nev, opts->ncv, (unsigned long)a->M);
        return EXIT_FAILURE;
    }
    if (opts->which != SPMV_EIG_LARGEST && opts->which != SPMV_EIG_SMALLEST) { ERR("%s: unknown which %d", who, opts->which); return EXIT_FAILURE; }
    if (!(opts->tol >= 0.0)) { ERR("%s: tol %g is negative or NaN", who, opts->tol); return EXIT_FAILURE; }
    if (opts->keep && (opts->keep < opts->nev || opts->keep > opts->ncv - 1)) {
        ERR("%s: keep=%u is not 0 and not in nev .. ncv-1 = %u .. %u", who, opts->keep, opts->nev, opts->ncv - 1);
        return EXIT_FAILURE;
    }
    if (ldx < a->M) { ERR("%s: ldx=%zu < M=%lu", who, ldx, (unsigned long)a->M); return EXIT_FAILURE; }
    if (spansShare(dV0, a->M * sizeof(double), dX, colMajorSpan(a->M, opts->nev, ldx))) { ERR("%s: dV0 and dX overlap", who); return EXIT_FAILURE; }
    if (lanczosSolve(dA, a, dV0, opts, dX, ldx, theta, res, info, S.stream)) { ERR("%s: the solve failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

// ---- the residual block and the preconditioned eigensolver (contract in spmvHip.h, design in DESIGN.md section 42)
int spmvHipBlockResidual(size_t n, unsigned m, unsigned k, const double* dV, size_t ldv, const double* dW, size_t ldw, const double* dS,
                         size_t lds, const double* dTheta, double* dR, size_t ldr, double* dNorm2) {
    const char* who = "spmvHipBlockResidual";
    const Ctx cx = libraryCtx();
    if (!ready(who)) return EXIT_FAILURE;
    if (n && (!dV || !dW || !dS || !dTheta || !dR || !dNorm2)) {
        ERR("%s: %s is NULL", who, !dV ? "dV" : !dW ? "dW" : !dS ? "dS" : !dTheta ? "dTheta" : !dR ? "dR" : "dNorm2");
        return EXIT_FAILURE;
    }
    if (m == 0 || m > 64 || k == 0 || k > 16) { ERR("%s: m=%u, k=%u: m must be in 1 .. 64 and k in 1 .. 16", who, m, k); return EXIT_FAILURE; }
    if (ldv < n || ldw < n || ldr < n || lds < m) {
        ERR("%s: ldv=%zu, ldw=%zu, ldr=%zu (n=%zu) or lds=%zu (m=%u) is too small", who, ldv, ldw, ldr, n, lds, m);
        return EXIT_FAILURE;
    }
    const uint64_t rBytes = colMajorSpan(n, k, ldr), nBytes = (uint64_t)k * sizeof(double);
    const struct { const void* p; uint64_t bytes; const char* name; } in[] = {
        {dV, colMajorSpan(n, m, ldv), "dV"}, {dW, colMajorSpan(n, m, ldw), "dW"}, {dS, colMajorSpan(m, k, lds), "dS"}, {dTheta, nBytes, "dTheta"}};
    for (const auto& x : in)
        if (spansShare(x.p, x.bytes, dR, rBytes) || (n && spansShare(x.p, x.bytes, dNorm2, nBytes))) {
            ERR("%s: %s overlaps dR or dNorm2", who, x.name);
            return EXIT_FAILURE;
        }
    if (spansShare(dR, rBytes, dNorm2, nBytes)) { ERR("%s: dR and dNorm2 overlap", who); return EXIT_FAILURE; }
    Launch L(cx, dim3(1), dim3(256));
    dim3 grid(1);
    if (blockResidual(n, m, k, dV, ldv, dW, ldw, dS, lds, dTheta, dR, ldr, dNorm2, cx.stream, &grid)) { ERR("%s: launch failed", who); return EXIT_FAILURE; }
    L.shape(grid, dim3(256));
    return L.finish(who);
}

int hipSpDavidsonCSR(spmat* dA, spmat* dM, const double* dV0, const spmvDavidsonOpts* opts, double* dX, size_t ldx, double* theta,
                     double* res, spmvDavidsonInfo* info) {
    const char* who = "hipSpDavidsonCSR";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dV0 || !opts || !dX || !theta || !res) {
        ERR("%s: %s is NULL", who, !dV0 ? "dV0" : !opts ? "opts" : !dX ? "dX" : !theta ? "theta" : "res");
        return EXIT_FAILURE;
    }
    DevMat* a = csrOf(dA, who, "dA is an ELL handle (only CSR handles are solved)");
    if (!a) return EXIT_FAILURE;
    if (a->M != a->N) { ERR("%s: M=%lu != N=%lu: dA is not square", who, (unsigned long)a->M, (unsigned long)a->N); return EXIT_FAILURE; }
    if (a->NZ && !a->AS && !a->unit) { ERR("%s: dA has no value array", who); return EXIT_FAILURE; }
    if (opts->nev == 0 || opts->nev > 16 || opts->nev >= opts->ncv || opts->ncv > 64 || opts->ncv > a->M) {
        ERR("%s: nev=%u, ncv=%u, M=%lu: 1 <= nev <= 16 and nev < ncv <= min(64, M) are required", who, opts->nev, opts->ncv, (unsigned long)a->M);
        return EXIT_FAILURE;
    }
    if (opts->which != SPMV_EIG_LARGEST && opts->which != SPMV_EIG_SMALLEST) { ERR("%s: unknown which %d", who, opts->which); return EXIT_FAILURE; }
    if (!(opts->tol >= 0.0)) { ERR("%s: tol %g is negative or NaN", who, opts->tol); return EXIT_FAILURE; }
    if (opts->keep && (opts->keep < opts->nev || opts->keep > opts->ncv - 1)) {
        ERR("%s: keep=%u is not 0 and not in nev .. ncv-1 = %u .. %u", who, opts->keep, opts->nev, opts->ncv - 1);
        return EXIT_FAILURE;
    }
    if (ldx < a->M) { ERR("%s: ldx=%zu < M=%lu", who, ldx, (unsigned long)a->M); return EXIT_FAILURE; }
    if (spansShare(dV0, a->M * sizeof(double), dX, colMajorSpan(a->M, opts->nev, ldx))) { ERR("%s: dV0 and dX overlap", who); return EXIT_FAILURE; }
    if (dM && opts->which == SPMV_EIG_LARGEST) {
        ERR("%s: a dM with SPMV_EIG_LARGEST: a positive definite M^-1 damps the directions of the large eigenvalues, and the search for "
            "the upper end then takes many times the products it takes without a dM (DESIGN.md section 42); drop dM or ask for "
            "SPMV_EIG_SMALLEST", who);
        return EXIT_FAILURE;
    }
    DevMat* m = nullptr;
    if (!precondOf(who, dM, a, &m)) return EXIT_FAILURE;
    if (davidsonSolve(dA, a, m, dV0, opts, dX, ldx, theta, res, info, S.stream)) { ERR("%s: the solve failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

}  // extern "C"
