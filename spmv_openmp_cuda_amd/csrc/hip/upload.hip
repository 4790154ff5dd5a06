// upload.hip -- device handles: upload, adoption of device arrays, and the handles made from other handles (CSR -> ELL,
// transpose, permutation, product, sum, filter) with their refreshes, the handle assembled from COO triplets with its own;
// free; and what looks at the values of a handle (unit-value detection, the value refresh).
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstring>
#include <limits>
#include <vector>

#include "lib.hpp"

using namespace spmvhip;

namespace {

// Block table of csr_stream2_kernel: rows packed while nnz <= STREAM_NNZ and rows <= STREAM2_MAX_ROWS;
// a longer row is a block of its own, flagged, and all such blocks come first (longest first) so that
// their serial tails overlap the rest of the grid.
template <typename I>
int buildRowBlocks2(DevMat* d, const I* IRP, uint64_t M) {
    std::vector<uint4> info, longs;
    std::vector<uint64_t> base, longBase;
    info.reserve(M / 64 + 2); base.reserve(M / 64 + 2);
    d->maxRowNnz = 0;
    for (uint64_t i = 0; i < M; ++i) d->maxRowNnz = std::max<uint64_t>(d->maxRowNnz, (uint64_t)IRP[i + 1] - (uint64_t)IRP[i]);
    uint64_t r = 0;
    while (r < M) {
        const uint64_t start = IRP[r];
        uint64_t e = r;
        while (e < M && (uint64_t)IRP[e + 1] - start <= (uint64_t)STREAM_NNZ && e - r < STREAM2_MAX_ROWS) ++e;
        if (e == r) {
            const uint64_t len = (uint64_t)IRP[r + 1] - start;
            if (len >= (1ull << 32)) { ERR("a single row with %lu entries is not supported", (unsigned long)len); return EXIT_FAILURE; }
            longs.push_back(make_uint4((uint32_t)r, 1u, (uint32_t)len, 1u));
            longBase.push_back(start);
            e = r + 1;
        } else {
            info.push_back(make_uint4((uint32_t)r, (uint32_t)(e - r), (uint32_t)((uint64_t)IRP[e] - start), 0u));
            base.push_back(start);
        }
        r = e;
    }
    std::vector<size_t> order(longs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return longs[a].z > longs[b].z; });
    std::vector<uint4> allInfo; std::vector<uint64_t> allBase;
    allInfo.reserve(longs.size() + info.size()); allBase.reserve(longs.size() + info.size());
    for (size_t i : order) { allInfo.push_back(longs[i]); allBase.push_back(longBase[i]); }
    allInfo.insert(allInfo.end(), info.begin(), info.end());
    allBase.insert(allBase.end(), base.begin(), base.end());
    d->nBlk2 = (uint32_t)allInfo.size();
    d->nLong2 = (uint32_t)longs.size();
    HIP_TRY(devMalloc(&d->blkInfo, std::max<size_t>(allInfo.size(), 1) * sizeof(uint4)));
    HIP_TRY(devMalloc(&d->blkBase, std::max<size_t>(allBase.size(), 1) * sizeof(uint64_t)));
    HIP_TRY(hipMemcpy(d->blkInfo, allInfo.data(), allInfo.size() * sizeof(uint4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->blkBase, allBase.data(), allBase.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    return EXIT_SUCCESS;
}

}  // namespace

namespace spmvhip {
void freeDesc(DevMat* d) {
    if (!d) return;
    if (d->owns) {
        (void)devFree(d->IRP); (void)devFree(d->JA); (void)devFree(d->AS); (void)devFree(d->RL);
    }
    (void)devFree(d->blkInfo); (void)devFree(d->blkBase); (void)devFree(d->tmap); (void)devFree(d->AS32);
    freeTri(d->tri[0]); freeTri(d->tri[1]);
    freeTriSweeps(d->sweep);
    freeSpgemmPlan(d->prod);
    freeAddPlan(d->sum);
    freeFilterPlan(d->filt);
    freeCooPlan(d->coo);
    freeAmg(d->amg);
    if (d->fsai) {                                      // an approximate-inverse factor: its transpose and its workspace
        freeDesc(d->fsai->gt);
        (void)devFree(d->fsai->work);
        delete d->fsai;
    }
    freeTiles(d->tiles[0]); freeTiles(d->tiles[1]);
    freeSell(d->sell);
    freeStripes(d->stripes[0]); freeStripes(d->stripes[1]);
    d->magic = 0;
    delete d;
}

void publish(spmat* h, DevMat* d, ulong M, ulong N, ulong NZ, ulong maxRowNz) {
    memset(h, 0, sizeof *h);
    h->M = M; h->N = N; h->NZ = NZ; h->MAX_ROW_NZ = maxRowNz;
    h->JA = reinterpret_cast<ulong*>(d->JA);
    h->AS = d->AS;
    h->IRP = reinterpret_cast<ulong*>(d->IRP);
    h->RL = reinterpret_cast<ulong*>(d->RL);
    h->pitchJA = h->pitchAS = d->pitch;
    h->dev = d;
}
}  // namespace spmvhip

namespace {

template <typename T>
int narrowUpload(T** dDst, const ulong* hSrc, size_t n, ulong limit, const char* what) {
    std::vector<T> tmp(n);
    for (size_t i = 0; i < n; ++i) {
        if (hSrc[i] > limit) { ERR("%s[%zu] = %lu does not fit the device index width", what, i, hSrc[i]); return EXIT_FAILURE; }
        tmp[i] = (T)hSrc[i];
    }
    HIP_TRY(devMalloc(dDst, std::max<size_t>(n, 1) * sizeof(T)));
    HIP_TRY(hipMemcpy(*dDst, tmp.data(), n * sizeof(T), hipMemcpyHostToDevice));
    return EXIT_SUCCESS;
}

// device-side CSR -> ELL (row-major [rows][pitch] or column-major [slots][pitch]); one wavefront per row
template <typename I>
__global__ __launch_bounds__(256) void csr_to_ell_kernel(uint32_t M, uint32_t K, size_t pitch, int colMajor,
                                                         const I* __restrict__ IRP, const uint32_t* __restrict__ JA,
                                                         const double* __restrict__ AS, uint32_t* __restrict__ EJ,
                                                         double* __restrict__ EA, uint32_t* __restrict__ RL) {
    const uint64_t row = linear_block() * 4 + threadIdx.x / 64;
    if (row >= M) return;
    const uint32_t lane = threadIdx.x % 64;
    const I b = IRP[row];
    const uint32_t len = (uint32_t)(IRP[row + 1] - b);
    if (lane == 0) RL[row] = len;
    for (uint32_t c = lane; c < K; c += 64) {
        const size_t at = colMajor ? (size_t)c * pitch + row : (size_t)row * pitch + c;
        EJ[at] = c < len ? JA[b + c] : 0u;          // padding {0, 0.0} like the loader's calloc
        EA[at] = c < len ? AS[b + c] : 0.0;
    }
}

// 1 in *flag unless every value has the bit pattern `first` (bit patterns: -0.0 and 0.0, or two NaNs, are different values here)
__global__ __launch_bounds__(256) void values_differ_kernel(const uint64_t* __restrict__ AS, uint64_t n, uint64_t first, uint32_t* __restrict__ flag) {
    bool differ = false;
    for (uint64_t j = linear_block() * 256 + threadIdx.x; j < n; j += (uint64_t)gridDim.x * gridDim.y * 256) differ |= AS[j] != first;
    if (differ) atomicOr(flag, 1u);
}

// ELL: every REAL cell (slot < RL[row]) has the bit pattern `first`; padding cells are not looked at
__global__ __launch_bounds__(256) void ell_values_differ_kernel(uint64_t rows, size_t pitch, int colMajor, const uint64_t* __restrict__ AS,
                                                                const uint32_t* __restrict__ RL, uint64_t first, uint32_t* __restrict__ flag) {
    const uint64_t r = linear_block() * 256 + threadIdx.x;
    if (r >= rows) return;
    bool differ = false;
    for (uint32_t i = 0, n = RL[r]; i < n; ++i) differ |= AS[colMajor ? r + (uint64_t)i * pitch : r * pitch + i] != first;
    if (differ) atomicOr(flag, 1u);
}

// sets d->unit / d->unitValue (one pass over the values at upload and after a value update; off with spmvHipSetUnitValues(0)):
// does every stored value have the bit pattern `first` of one of them?  CSR: all of AS against AS[0]; ELL with row
// lengths: every real cell against slot 0 of the first non-empty row
int detectUnit(DevMat* d, hipStream_t st = nullptr) {
    const bool csr = d->kind == Kind::CSR, colMajor = d->kind == Kind::ELL_COLMAJOR;
    d->unit = false;
    if (!S.unitValues || !d->AS || (csr ? d->NZ == 0 : !d->RL || d->M == 0 || d->ellFirstRow == ~0ull)) return EXIT_SUCCESS;
    uint64_t first = 0;
    uint32_t differ = 1;
    HIP_TRY(hipMemcpyAsync(&first, d->AS + (csr ? 0 : colMajor ? d->ellFirstRow : d->ellFirstRow * d->pitch), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t* AS = reinterpret_cast<const uint64_t*>(d->AS);
    const int rc = deviceFlag(0, st, csr ? "values_differ_kernel" : "ell_values_differ_kernel", &differ, [&](uint32_t* dFlag) {
        if (csr) hipLaunchKernelGGL(values_differ_kernel, grid2d(std::min<uint64_t>((d->NZ + 255) / 256, 256 * 64), 256), dim3(256), 0, st, AS, d->NZ, first, dFlag);
        else hipLaunchKernelGGL(ell_values_differ_kernel, grid2d((d->M + 255) / 256, 256), dim3(256), 0, st, d->M, d->pitch, colMajor ? 1 : 0, AS, d->RL, first, dFlag);
    });
    if (rc == EXIT_SUCCESS && !differ) { d->unit = true; memcpy(&d->unitValue, &first, 8); }
    return rc;
}
// row pointers must start at 0, never decrease and end at NZ: the kernels trust them for every AS/JA access
template <typename I>
bool rowPointersOk(const I* IRP, uint64_t M, uint64_t NZ, const char* who) {
    if ((uint64_t)IRP[0] != 0 || (uint64_t)IRP[M] != NZ) {
        ERR("%s: inconsistent row pointers (IRP[0]=%lu IRP[M]=%lu NZ=%lu)", who, (unsigned long)IRP[0], (unsigned long)IRP[M], (unsigned long)NZ);
        return false;
    }
    for (uint64_t r = 0; r < M; ++r)
        if (IRP[r] > IRP[r + 1]) { ERR("%s: row pointers decrease at row %lu (%lu > %lu)", who, (unsigned long)r, (unsigned long)IRP[r], (unsigned long)IRP[r + 1]); return false; }
    return true;
}

// Upload an (nRows x nCols) row-major host array pair with a padded pitch.
int uploadPitched(DevMat* d, const ulong* hJA, const double* hAS, size_t nRows, size_t nCols,
                         size_t pitch, ulong colLimit) {
    const size_t total = std::max<size_t>(nRows * pitch, 1);
    std::vector<uint32_t> ja(total, 0u);
    std::vector<double>   as(total, 0.0);
    for (size_t r = 0; r < nRows; ++r)
        for (size_t c = 0; c < nCols; ++c) {
            const ulong col = hJA[r * nCols + c];
            if (col > colLimit) { ERR("spMatCpyELL: column id %lu out of range", col); return EXIT_FAILURE; }
            ja[r * pitch + c] = (uint32_t)col;
            as[r * pitch + c] = hAS[r * nCols + c];
        }
    HIP_TRY(devMalloc(&d->JA, total * sizeof(uint32_t)));
    HIP_TRY(devMalloc(&d->AS, total * sizeof(double)));
    HIP_TRY(hipMemcpy(d->JA, ja.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->AS, as.data(), total * sizeof(double), hipMemcpyHostToDevice));
    d->pitch = pitch;
    return EXIT_SUCCESS;
}

int ellUpload(spmat* m, spmat* dst, bool transposed) {
    if (!ready("spMatCpyELL") || !m || !dst) return EXIT_FAILURE;
    if (!m->JA || !m->AS) { ERR("spMatCpyELL: host matrix has no ELL arrays"); return EXIT_FAILURE; }
    // reference field convention: a transposed matrix keeps slots in M and rows in MAX_ROW_NZ / N
    const ulong rows  = transposed ? m->MAX_ROW_NZ : m->M;
    const ulong slots = transposed ? m->M : m->MAX_ROW_NZ;
    // a transposed struct has lost the column count to the reference's field swap; this repo's ellTranspose (and
    // api.HostELL.transpose) keep it in the unused host field pitchJA -- 0 = unknown, column ids then cannot be checked
    const ulong cols  = transposed ? (ulong)m->pitchJA : m->N;
    if (rows >= (1ull << 32) - 1 || slots >= (1ull << 32) - 1) { ERR("spMatCpyELL: dimensions exceed 32-bit ids"); return EXIT_FAILURE; }
    DevMat* d = new DevMat;
    d->kind = transposed ? Kind::ELL_COLMAJOR : Kind::ELL_ROWMAJOR;
    d->M = rows; d->N = cols; d->NZ = m->NZ; d->K = slots;
    int rc;
    const ulong colLimit = transposed ? (cols ? cols - 1 : 0xFFFFFFFFul) : (m->N ? m->N - 1 : 0);
    if (transposed) rc = uploadPitched(d, m->JA, m->AS, slots, rows, (rows + 63) / 64 * 64, colLimit);
    else            rc = uploadPitched(d, m->JA, m->AS, rows, slots, (slots + 1) / 2 * 2, colLimit);   // (rows stay 16-B aligned; a wider pitch is only padding to stream)
    if (!rc && m->RL) rc = narrowUpload<uint32_t>(&d->RL, m->RL, rows, slots, "RL");
    if (!rc && m->RL) {                                // the first non-empty row: slot 0 of it is what the unit detection compares with
        ulong r = 0;
        while (r < rows && m->RL[r] == 0) ++r;
        if (r < rows) d->ellFirstRow = r;
        rc = detectUnit(d);
    }
    if (rc) { freeDesc(d); return EXIT_FAILURE; }
    publish(dst, d, m->M, m->N, m->NZ, m->MAX_ROW_NZ);
    return EXIT_SUCCESS;
}

}  // namespace

namespace spmvhip {
// spmvHipUpdateValues / spmvHipValuesChanged (reread: the handle's own AS was rewritten) / spmvHipShardUpdateValues (its
// per-device stream): the contract is in spmvHip.h, the design in DESIGN.md section 14
int updateValues(spmat* h, const double* AS, bool onDevice, bool reread, hipStream_t st, const char* who) {
    if (!ready(who)) return EXIT_FAILURE;
    DevMat* d = descOf(h, who);
    if (!d) return EXIT_FAILURE;
    if (!reread && !AS) { ERR("%s: AS is NULL", who); return EXIT_FAILURE; }
    if (d->origin == Origin::ELL_OF_CSR) {
        ERR("%s: this ELL handle was made on the device from a CSR handle (spmvHipCsrToEll) and keeps no link to it: "
            "update the CSR handle and convert again", who);
        return EXIT_FAILURE;
    }
    const auto t0 = std::chrono::steady_clock::now();
    d->iluPending = false;                              // whatever the values were, they are being replaced or reread
    spmvUpdateInfo info{};
    bool f32Failed = false;
    info.unitBefore = d->unit;
    const double valueBefore = d->unitValue;
    const hipMemcpyKind kind = onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (d->kind == Kind::CSR) {
        if (!reread && d->NZ) HIP_TRY(hipMemcpyAsync(d->AS, AS, d->NZ * sizeof(double), kind, st));
        if (detectUnit(d, st)) { valuesF32Drop(d); return EXIT_FAILURE; }      // (a form that cannot follow the values is given back)
        // the single-precision form first: whatever becomes of the formats below, it holds the new roundings or is gone.  Its
        // failure (the array of a unit -> non-unit update refused) fails the call at its end, with the f64 side complete.
        f32Failed = d->f32 && valuesF32Follow(d, st, who) != EXIT_SUCCESS;
        // every built format, both forms.  When the values were unit before and are unit now no kernel reads a value array
        // (SELL has no unit kernel): only the value in the registers changes.  A stripes format built for a unit matrix has
        // no value array: it is rebuilt, with its recorded options, when the values stop being unit.
        const bool arrays = !(info.unitBefore && d->unit);
        for (TileFormat* t : d->tiles)
            if (t && arrays && tilesRefreshValues(d, t, st, &info.mapMs, &info.mapsBuilt)) return EXIT_FAILURE;
        std::vector<spmvStripesOpts> rebuild;
        for (StripeFormat* f : d->stripes) {
            if (!f) continue;
            if (!stripesHasValues(f) && !d->unit) { rebuild.push_back(stripesOptions(f)); continue; }
            if (stripesHasValues(f) && arrays && stripesRefreshValues(d, f, st, &info.mapMs, &info.mapsBuilt)) return EXIT_FAILURE;
            stripesSetUnit(f, d->unit, d->unitValue);
        }
        if (sellRefreshValues(d, st)) return EXIT_FAILURE;
        if (!rebuild.empty()) {
            HIP_TRY(hipStreamSynchronize(st));           // the builds run on the null stream from AS
            for (const spmvStripesOpts& o : rebuild)
                if (buildStripes(d, &o)) { ERR("%s: rebuilding the stripes format failed", who); return EXIT_FAILURE; }
            info.rebuilt = 1;
        }
        if (info.unitBefore && !d->unit) {               // the selections measured the byte counts of the unit kernels
            d->autoPick[0] = d->autoPick[1] = -1;
            memset(d->autoMs, 0, sizeof d->autoMs);
        }
    } else {
        const bool colMajor = d->kind == Kind::ELL_COLMAJOR;
        const size_t nRows = colMajor ? d->K : d->M, nCols = colMajor ? d->M : d->K;      // the host layout of the upload
        if (!reread && nRows && nCols)
            HIP_TRY(hipMemcpy2DAsync(d->AS, d->pitch * sizeof(double), AS, nCols * sizeof(double), nCols * sizeof(double), nRows, kind, st));
        if (detectUnit(d, st)) return EXIT_FAILURE;
    }
    HIP_TRY(hipStreamSynchronize(st));
    info.unitAfter = d->unit;
    const bool sameUnit = info.unitBefore && d->unit && memcmp(&valueBefore, &d->unitValue, 8) == 0;
    info.inPlace = !info.rebuilt && (!info.unitBefore || sameUnit);
    info.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    d->lastUpdate = info;
    return f32Failed ? EXIT_FAILURE : EXIT_SUCCESS;
}

// The tail of every CSR handle whose arrays (4-byte row pointers) were made on the device: the row pointers come back to
// the host for the row blocks, then the unit detection; the descriptor is published into dst, or -- when that fails, or
// what came before it did (built = false) -- freed with all it holds.
static int finishCsr(spmat* dst, DevMat* d, bool built = true) {
    std::vector<uint32_t> hIRP(d->M + 1);
    const bool ok = built && hipOk(hipMemcpy(hIRP.data(), d->IRP, hIRP.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy IRP") &&
                    !buildRowBlocks2(d, hIRP.data(), d->M) && !detectUnit(d, S.stream);
    if (!ok) { freeDesc(d); return EXIT_FAILURE; }
    publish(dst, d, d->M, d->N, d->NZ, 0);
    return EXIT_SUCCESS;
}

// a CSR handle over three device arrays the library itself has made (4-byte row pointers): the handle owns them from the
// call on -- on failure they are freed with the descriptor
int ownCsr(spmat* dst, uint64_t M, uint64_t N, uint64_t NZ, uint32_t* dIRP, uint32_t* dJA, double* dAS) {
    DevMat* d = new DevMat;
    d->M = M; d->N = N; d->NZ = NZ;
    d->IRP = dIRP; d->JA = dJA; d->AS = dAS;
    return finishCsr(dst, d);
}
}  // namespace spmvhip

// a CSR descriptor with a map, made as `o` from a, for M rows and a's entries: what transposeCsr / permuteCsr fill
static DevMat* newMappedCsr(Origin o, const DevMat* a, uint64_t M, uint64_t N, bool* ok) {
    DevMat* t = new DevMat;
    t->M = M; t->N = N; t->NZ = a->NZ;
    setOrigin(t, o, a);
    const size_t nz1 = std::max<size_t>(a->NZ, 1);
    *ok = hipOk(devMalloc(&t->IRP, (M + 1) * 4), "hipMalloc IRP") && hipOk(devMalloc(&t->JA, nz1 * 4), "hipMalloc JA") &&
          hipOk(devMalloc(&t->AS, nz1 * 8), "hipMalloc AS") && hipOk(devMalloc(&t->tmap, nz1 * 4), "hipMalloc map");
    return t;
}

// dX (made as `o` from dA) takes dA's current values through its map, then refreshes its formats: the three refreshes.
// `after` (the filter's ordered sums) runs between the gather and the formats.
static int mappedRefresh(const char* who, Origin o, spmat* dX, const char* xName, spmat* dA,
                         int (*after)(DevMat* x, const DevMat* a, hipStream_t st) = nullptr) {
    if (!ready(who)) return EXIT_FAILURE;
    DevMat* t = descOf(dX, who);
    if (!t) return EXIT_FAILURE;
    DevMat* a = descOf(dA, who);
    if (!a || !madeBy(t, o, a, nullptr, who, xName, "dA")) return EXIT_FAILURE;
    t->iluPending = false;                              // AS is rewritten from here on, whatever becomes of the call
    if (enqueueGatherValues(t->AS, t->tmap, t->NZ, a->AS, S.stream)) return EXIT_FAILURE;
    if (after && after(t, a, S.stream)) { ERR("%s: recomputing the values failed", who); return EXIT_FAILURE; }
    return updateValues(dX, nullptr, true, true, S.stream, who);
}

extern "C" {

int spMatCpyCSR(spmat* m, spmat* dst) {
    if (!ready("spMatCpyCSR") || !m || !dst) return EXIT_FAILURE;
    if (!m->IRP || (m->NZ && (!m->JA || !m->AS))) { ERR("spMatCpyCSR: host matrix has no CSR arrays"); return EXIT_FAILURE; }
    if (m->M >= (1ull << 32) - 1 || m->N > (1ull << 32)) { ERR("spMatCpyCSR: %lu x %lu exceeds the 32-bit row/column ids of the device format", m->M, m->N); return EXIT_FAILURE; }
    if (!rowPointersOk(m->IRP, m->M, m->NZ, "spMatCpyCSR")) return EXIT_FAILURE;
    DevMat* d = new DevMat;
    d->kind = Kind::CSR;
    d->M = m->M; d->N = m->N; d->NZ = m->NZ;
    d->irpBytes = m->NZ < IRP32_LIMIT ? 4 : 8;
    int rc = withIrp(d, [&](auto irp) {
        using I = IrpT<decltype(irp)>;
        return narrowUpload<I>(reinterpret_cast<I**>(&d->IRP), m->IRP, m->M + 1, std::numeric_limits<I>::max(), "IRP");
    });
    if (!rc) rc = narrowUpload<uint32_t>(&d->JA, m->JA, m->NZ, m->N ? m->N - 1 : 0, "JA");
    if (!rc) {
        if (!hipOk(devMalloc(&d->AS, std::max<size_t>(m->NZ, 1) * sizeof(double)), "hipMalloc AS") ||
            !hipOk(hipMemcpy(d->AS, m->AS, m->NZ * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy AS")) rc = EXIT_FAILURE;
    }
    if (!rc && m->RL) rc = narrowUpload<uint32_t>(&d->RL, m->RL, m->M, 0xFFFFFFFFul, "RL");
    if (!rc) rc = buildRowBlocks2(d, m->IRP, m->M);
    if (!rc) rc = detectUnit(d);
    if (rc) { freeDesc(d); return EXIT_FAILURE; }
    publish(dst, d, m->M, m->N, m->NZ, 0);
    return EXIT_SUCCESS;
}

int spmvHipAdoptCSR(spmat* dst, ulong M, ulong N, ulong NZ, const void* dIRP, int irpBytes,
                    const uint32_t* dJA, const double* dAS, const void* hIRP) {
    if (!ready("spmvHipAdoptCSR") || !dst || !dIRP) return EXIT_FAILURE;
    if (irpBytes != 4 && irpBytes != 8) { ERR("spmvHipAdoptCSR: irpBytes must be 4 or 8"); return EXIT_FAILURE; }
    if (irpBytes < 8 && NZ >= IRP32_LIMIT) { ERR("spmvHipAdoptCSR: NZ=%lu needs 64-bit row pointers", NZ); return EXIT_FAILURE; }
    if (M >= (1ull << 32) - 1 || N > (1ull << 32)) { ERR("spmvHipAdoptCSR: dimensions exceed 32-bit ids"); return EXIT_FAILURE; }
    std::vector<unsigned char> tmp;
    if (!hIRP) {
        tmp.resize((M + 1) * (size_t)irpBytes);
        HIP_TRY(hipMemcpy(tmp.data(), dIRP, tmp.size(), hipMemcpyDeviceToHost));
        hIRP = tmp.data();
    }
    if (!withIrp(hIRP, irpBytes, [&](auto irp) { return rowPointersOk(irp, M, NZ, "spmvHipAdoptCSR"); })) return EXIT_FAILURE;
    DevMat* d = new DevMat;
    d->kind = Kind::CSR; d->owns = false;
    d->M = M; d->N = N; d->NZ = NZ; d->irpBytes = irpBytes;
    d->IRP = const_cast<void*>(dIRP); d->JA = const_cast<uint32_t*>(dJA); d->AS = const_cast<double*>(dAS);
    if (withIrp(hIRP, irpBytes, [&](auto irp) { return buildRowBlocks2(d, irp, M); }) || detectUnit(d)) { freeDesc(d); return EXIT_FAILURE; }
    publish(dst, d, M, N, NZ, 0);
    return EXIT_SUCCESS;
}

int spMatCpyELL(spmat* m, spmat* dst) { return ellUpload(m, dst, m && m->dev == SPMAT_TAG_ELL_TRANSPOSED); }
int spMatCpyELLTransposed(spmat* m, spmat* dst) { return ellUpload(m, dst, true); }

int spmvHipCsrToEll(spmat* dCsr, int transposed, spmat* dEll) {
    DevMat* c = descOf(dCsr, "spmvHipCsrToEll");
    if (!c || !dEll || !csrOnly(c, "spmvHipCsrToEll", "source handle is not CSR")) return EXIT_FAILURE;
    const uint64_t K = c->maxRowNnz, rows = c->M;
    DevMat* d = new DevMat;
    d->kind = transposed ? Kind::ELL_COLMAJOR : Kind::ELL_ROWMAJOR;
    setOrigin(d, Origin::ELL_OF_CSR);
    d->M = rows; d->N = c->N; d->NZ = c->NZ; d->K = K;
    d->pitch = transposed ? (rows + 63) / 64 * 64 : (K + 1) / 2 * 2;
    const size_t cells = std::max<size_t>((transposed ? K : rows) * d->pitch, 1);
    {   // ELL size guard.  The reference's loader refuses an ELL copy whose 2*M*maxRow padded cells exceed a fixed host
        // budget (src/lib/parser.c:223-232, config.h:69-70: 6*2^27 cells); on the device the budget is what the GPU has
        // free right now -- the unclipped power-law matrix (10 M rows x 50 k slots = 6 TB) is refused here, before any
        // allocation, the same matrix clipped to 64 slots (7.7 GB) passes.
        size_t freeB = 0, totalB = 0;
        const unsigned __int128 need128 = (unsigned __int128)(transposed ? K : rows) * d->pitch * 12 + (unsigned __int128)rows * 4;
        const size_t need = need128 > (unsigned __int128)~(size_t)0 ? ~(size_t)0 : (size_t)need128;
        // best effort: what is free at this moment (other processes and cached pools count as used); when the query itself
        // fails the guard is skipped and hipMalloc decides
        const bool known = hipMemGetInfo(&freeB, &totalB) == hipSuccess;
        if (!known) (void)hipGetLastError();
        if (known && need > freeB) {
            ERR("spmvHipCsrToEll: ELL copy of %lu rows x %lu slots needs %.1f GB, device has %.1f GB free: refused "
                "(the reference refuses above 6*2^27 padded cells, parser.c:223-232)", (unsigned long)rows, (unsigned long)K,
                (double)need * 1e-9, (double)freeB * 1e-9);
            delete d;
            return EXIT_FAILURE;
        }
    }
    if (!hipOk(devMalloc(&d->JA, cells * sizeof(uint32_t)), "hipMalloc ELL JA") ||
        !hipOk(devMalloc(&d->AS, cells * sizeof(double)), "hipMalloc ELL AS") ||
        !hipOk(devMalloc(&d->RL, std::max<size_t>(rows, 1) * sizeof(uint32_t)), "hipMalloc ELL RL") ||
        !hipOk(hipMemsetAsync(d->JA, 0, cells * sizeof(uint32_t), S.stream), "memset") ||
        !hipOk(hipMemsetAsync(d->AS, 0, cells * sizeof(double), S.stream), "memset")) { freeDesc(d); return EXIT_FAILURE; }
    if (rows) {
        const dim3 grid = grid2d((rows + 3) / 4, 256);
        withIrp(c, [&](auto irp) { hipLaunchKernelGGL((csr_to_ell_kernel<IrpT<decltype(irp)>>), grid, dim3(256), 0, S.stream, (uint32_t)rows, (uint32_t)K, d->pitch, transposed, irp, c->JA, c->AS, d->JA, d->AS, d->RL); });
    }
    if (!hipOk(hipGetLastError(), "csr_to_ell launch") || !hipOk(hipStreamSynchronize(S.stream), "csr_to_ell")) { freeDesc(d); return EXIT_FAILURE; }
    d->unit = c->unit; d->unitValue = c->unitValue;   // the same values, and row lengths always
    // handle fields follow the reference's conventions (transposed: M = slots, MAX_ROW_NZ = rows)
    if (transposed) publish(dEll, d, K, rows, c->NZ, rows);
    else            publish(dEll, d, rows, c->N, c->NZ, K);
    return EXIT_SUCCESS;
}

// A^T as a handle of its own (transpose.hip builds the arrays; the contract is in spmvHip.h, the design in DESIGN.md
// section 16).  Refusals come before anything is allocated; a failure after that frees what was made, and dAT is written
// only on success.
int spmvHipCsrTranspose(spmat* dA, spmat* dAT) {
    const char* who = "spmvHipCsrTranspose";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dAT) { ERR("%s: dAT is NULL", who); return EXIT_FAILURE; }
    DevMat* a = descOf(dA, who);
    if (!a) return EXIT_FAILURE;
    if (dAT == dA) { ERR("%s: dAT is the source handle itself", who); return EXIT_FAILURE; }
    if (!csrOnly(a, who, "the source is an ELL handle (only CSR handles can be transposed)")) return EXIT_FAILURE;
    if (a->NZ >= IRP32_LIMIT) {
        ERR("%s: NZ=%lu: the map and the row pointers of the transpose are 32-bit (limit %lu)", who, (unsigned long)a->NZ,
            (unsigned long)IRP32_LIMIT);
        return EXIT_FAILURE;
    }
    if (a->N >= (1ull << 32) - 1) { ERR("%s: N=%lu columns do not fit the row ids of the transpose", who, (unsigned long)a->N); return EXIT_FAILURE; }
    if (a->NZ && (!a->JA || !a->AS)) { ERR("%s: the source has no column or value array", who); return EXIT_FAILURE; }
    bool ok = false;
    DevMat* t = newMappedCsr(Origin::TRANSPOSE, a, a->N, a->M, &ok);
    if (finishCsr(dAT, t, ok && !transposeCsr(a, t, S.stream))) { ERR("%s: building the transpose failed", who); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

int spmvHipTransposeRefresh(spmat* dAT, spmat* dA) { return mappedRefresh("spmvHipTransposeRefresh", Origin::TRANSPOSE, dAT, "dAT", dA); }

// B = P A P^T as a handle of its own (colour.hip builds the arrays; the contract is in spmvHip.h, the design in DESIGN.md
// section 21).  As the transpose: refusals come before anything is allocated for dB, and dB is written only on success.
int spmvHipCsrPermute(spmat* dA, const uint32_t* dPerm, spmat* dB) {
    const char* who = "spmvHipCsrPermute";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dB || !dPerm) { ERR("%s: %s is NULL", who, !dB ? "dB" : "dPerm"); return EXIT_FAILURE; }
    if (dB == dA) { ERR("%s: dB is the source handle itself", who); return EXIT_FAILURE; }
    DevMat* a = squareCsrOf(dA, who, "the source is an ELL handle (only CSR handles can be permuted)");
    if (!a) return EXIT_FAILURE;
    if (a->NZ && !a->AS) { ERR("%s: the source has no column or value array", who); return EXIT_FAILURE; }
    uint32_t* inv = nullptr;
    uint32_t bad = 0;
    HIP_TRY(devMalloc(&inv, std::max<size_t>(a->M, 1) * 4));
    if (invertPerm(a->M, dPerm, inv, &bad, S.stream)) { (void)devFree(inv); ERR("%s: checking dPerm failed", who); return EXIT_FAILURE; }
    if (bad) {
        (void)devFree(inv);
        ERR("%s: dPerm is not a permutation of 0..M-1 (%s)", who, bad & 1 ? "a value >= M" : "a repeated value");
        return EXIT_FAILURE;
    }
    bool ok = false;
    DevMat* t = newMappedCsr(Origin::PERMUTATION, a, a->M, a->M, &ok);
    const int rc = finishCsr(dB, t, ok && !permuteCsr(a, inv, t, S.stream));
    (void)devFree(inv);
    if (rc) ERR("%s: building the permuted matrix failed", who);
    return rc;
}

int spmvHipPermuteRefresh(spmat* dB, spmat* dA) { return mappedRefresh("spmvHipPermuteRefresh", Origin::PERMUTATION, dB, "dB", dA); }

// C = A B as a handle of its own (spgemm.hip builds the arrays; the contract is in spmvHip.h, the design in DESIGN.md
// section 22).  Refusals come first; dC and info are written only on success.
int spmvHipSpGEMM(spmat* dA, spmat* dB, const spmvSpgemmOpts* opts, spmat* dC, spmvSpgemmInfo* info) {
    const char* who = "spmvHipSpGEMM";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dA || !dB || !dC) { ERR("%s: %s is NULL", who, !dA ? "dA" : !dB ? "dB" : "dC"); return EXIT_FAILURE; }
    if (dC == dA || dC == dB) { ERR("%s: dC is a source handle itself", who); return EXIT_FAILURE; }
    DevMat* a = descOf(dA, who);
    DevMat* b = a ? descOf(dB, who) : nullptr;
    if (!a || !b) return EXIT_FAILURE;
    if (!csrOnly(a, who, "dA is an ELL handle (only CSR handles can be multiplied)") ||
        !csrOnly(b, who, "dB is an ELL handle (only CSR handles can be multiplied)"))
        return EXIT_FAILURE;
    if (a->N != b->M) { ERR("%s: A.N=%lu != B.M=%lu", who, (unsigned long)a->N, (unsigned long)b->M); return EXIT_FAILURE; }
    if (a->M >= (1ull << 32) - 1 || b->N >= (1ull << 32) - 1) {
        ERR("%s: A.M=%lu, B.N=%lu: the product has 32-bit row and column ids", who, (unsigned long)a->M, (unsigned long)b->N);
        return EXIT_FAILURE;
    }
    if ((a->NZ && (!a->JA || !a->AS)) || (b->NZ && (!b->JA || !b->AS))) { ERR("%s: a source has no column or value array", who); return EXIT_FAILURE; }
    DevMat* c = new DevMat;
    c->M = a->M; c->N = b->N;
    setOrigin(c, Origin::PRODUCT, a, b);
    spmvSpgemmInfo out{};
    if (finishCsr(dC, c, !spgemmBuild(a, b, opts, c, &out, S.stream))) { ERR("%s: building the product failed", who); return EXIT_FAILURE; }
    if (info) *info = out;
    return EXIT_SUCCESS;
}

int spmvHipSpGEMMRefresh(spmat* dC, spmat* dA, spmat* dB, spmvSpgemmInfo* info) {
    const char* who = "spmvHipSpGEMMRefresh";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dA || !dB || !dC) { ERR("%s: %s is NULL", who, !dC ? "dC" : !dA ? "dA" : "dB"); return EXIT_FAILURE; }
    DevMat* c = descOf(dC, who);
    DevMat* a = c ? descOf(dA, who) : nullptr;
    DevMat* b = a ? descOf(dB, who) : nullptr;
    if (!c || !a || !b || !madeBy(c, Origin::PRODUCT, a, b, who, "dC", "dA", "dB")) return EXIT_FAILURE;
    spmvSpgemmInfo out{};
    c->iluPending = false;                              // AS is rewritten from here on, whatever becomes of the call
    if (spgemmRefresh(c, a, b, &out, S.stream)) { ERR("%s: recomputing the values failed", who); return EXIT_FAILURE; }
    if (updateValues(dC, nullptr, true, true, S.stream, who)) return EXIT_FAILURE;
    if (info) *info = out;
    return EXIT_SUCCESS;
}

// C = alpha A + beta B as a handle of its own (add.hip builds the arrays; the contract is in spmvHip.h, the design in DESIGN.md
// section 25).  Refusals come first; dC and info are written only on success.
int spmvHipCsrAdd(double alpha, spmat* dA, double beta, spmat* dB, const spmvAddOpts* opts, spmat* dC, spmvAddInfo* info) {
    const char* who = "spmvHipCsrAdd";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dA || !dB || !dC) { ERR("%s: %s is NULL", who, !dA ? "dA" : !dB ? "dB" : "dC"); return EXIT_FAILURE; }
    if (dC == dA || dC == dB) { ERR("%s: dC is a source handle itself", who); return EXIT_FAILURE; }
    DevMat* a = descOf(dA, who);
    DevMat* b = a ? descOf(dB, who) : nullptr;
    if (!a || !b) return EXIT_FAILURE;
    if (!csrOnly(a, who, "dA is an ELL handle (only CSR handles can be added)") ||
        !csrOnly(b, who, "dB is an ELL handle (only CSR handles can be added)"))
        return EXIT_FAILURE;
    if (a->M != b->M || a->N != b->N) {
        ERR("%s: A is %lu x %lu, B is %lu x %lu", who, (unsigned long)a->M, (unsigned long)a->N, (unsigned long)b->M, (unsigned long)b->N);
        return EXIT_FAILURE;
    }
    if (a->M >= (1ull << 32) - 1 || a->N >= (1ull << 32) - 1) {
        ERR("%s: M=%lu, N=%lu: the sum has 32-bit row and column ids", who, (unsigned long)a->M, (unsigned long)a->N);
        return EXIT_FAILURE;
    }
    if ((a->NZ && (!a->JA || !a->AS)) || (b->NZ && (!b->JA || !b->AS))) { ERR("%s: a source has no column or value array", who); return EXIT_FAILURE; }
    DevMat* c = new DevMat;
    c->M = a->M; c->N = a->N;
    setOrigin(c, Origin::SUM, a, b);
    spmvAddInfo out{};
    if (finishCsr(dC, c, !addBuild(alpha, a, beta, b, opts, c, &out, S.stream))) { ERR("%s: building the sum failed", who); return EXIT_FAILURE; }
    if (info) *info = out;
    return EXIT_SUCCESS;
}

int spmvHipCsrAddRefresh(spmat* dC, double alpha, spmat* dA, double beta, spmat* dB, spmvAddInfo* info) {
    const char* who = "spmvHipCsrAddRefresh";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dA || !dB || !dC) { ERR("%s: %s is NULL", who, !dC ? "dC" : !dA ? "dA" : "dB"); return EXIT_FAILURE; }
    DevMat* c = descOf(dC, who);
    DevMat* a = c ? descOf(dA, who) : nullptr;
    DevMat* b = a ? descOf(dB, who) : nullptr;
    if (!c || !a || !b || !madeBy(c, Origin::SUM, a, b, who, "dC", "dA", "dB")) return EXIT_FAILURE;
    spmvAddInfo out{};
    c->iluPending = false;                              // AS is rewritten from here on, whatever becomes of the call
    if (addRefresh(c, alpha, a, beta, b, &out, S.stream)) { ERR("%s: recomputing the values failed", who); return EXIT_FAILURE; }
    if (updateValues(dC, nullptr, true, true, S.stream, who)) return EXIT_FAILURE;
    if (info) *info = out;
    return EXIT_SUCCESS;
}

// C = the entries of A that a predicate keeps, as a handle of its own (filter.hip builds the arrays; the contract is in
// spmvHip.h, the design in DESIGN.md section 29).  Refusals come first; dC and info are written only on success.
int spmvHipCsrFilter(spmat* dA, const spmvFilterOpts* opts, spmat* dC, spmvFilterInfo* info) {
    const char* who = "spmvHipCsrFilter";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dA || !opts || !dC) { ERR("%s: %s is NULL", who, !dA ? "dA" : !opts ? "opts" : "dC"); return EXIT_FAILURE; }
    if (dC == dA) { ERR("%s: dC is the source handle itself", who); return EXIT_FAILURE; }
    DevMat* a = descOf(dA, who);
    if (!a || !csrOnly(a, who, "the source is an ELL handle (only CSR handles can be filtered)")) return EXIT_FAILURE;
    if (opts->mode != SPMV_FILTER_BAND && opts->mode != SPMV_FILTER_ABS && opts->mode != SPMV_FILTER_STRENGTH) {
        ERR("%s: mode %d is none of SPMV_FILTER_BAND, SPMV_FILTER_ABS, SPMV_FILTER_STRENGTH", who, opts->mode);
        return EXIT_FAILURE;
    }
    if (!(opts->theta >= 0.0) || opts->theta > std::numeric_limits<double>::max()) {
        ERR("%s: theta = %g must be finite and not negative", who, opts->theta);
        return EXIT_FAILURE;
    }
    if (opts->lump && opts->mode == SPMV_FILTER_BAND) {
        ERR("%s: lump goes with SPMV_FILTER_ABS and SPMV_FILTER_STRENGTH: a band is a function of the pattern alone", who);
        return EXIT_FAILURE;
    }
    if ((opts->lump || opts->mode == SPMV_FILTER_STRENGTH) && a->M != a->N) {
        ERR("%s: M=%lu != N=%lu: SPMV_FILTER_STRENGTH and lump need the diagonal of a square matrix", who, (unsigned long)a->M, (unsigned long)a->N);
        return EXIT_FAILURE;
    }
    if (a->M >= (1ull << 32) - 1 || a->N >= (1ull << 32) - 1) {
        ERR("%s: M=%lu, N=%lu: the filtered matrix has 32-bit row and column ids", who, (unsigned long)a->M, (unsigned long)a->N);
        return EXIT_FAILURE;
    }
    if (a->NZ >= IRP32_LIMIT) {
        ERR("%s: NZ=%lu: the map and the row pointers of the filtered matrix are 32-bit (limit %lu)", who, (unsigned long)a->NZ,
            (unsigned long)IRP32_LIMIT);
        return EXIT_FAILURE;
    }
    if (a->NZ && (!a->JA || !a->AS)) { ERR("%s: the source has no column or value array", who); return EXIT_FAILURE; }
    DevMat* c = new DevMat;
    c->M = a->M; c->N = a->N;
    setOrigin(c, Origin::FILTER, a);
    if (finishCsr(dC, c, !filterBuild(a, opts, c, S.stream))) { ERR("%s: building the filtered matrix failed", who); return EXIT_FAILURE; }
    filterSetMaxRow(c);
    if (info) *info = *filterInfo(c);
    return EXIT_SUCCESS;
}

int spmvHipCsrFilterRefresh(spmat* dC, spmat* dA, spmvFilterInfo* info) {
    const char* who = "spmvHipCsrFilterRefresh";
    if (!dA || !dC) { ERR("%s: %s is NULL", who, !dC ? "dC" : "dA"); return EXIT_FAILURE; }
    if (mappedRefresh(who, Origin::FILTER, dC, "dC", dA, filterRefresh)) return EXIT_FAILURE;
    if (info) *info = *filterInfo(static_cast<DevMat*>(dC->dev));
    return EXIT_SUCCESS;
}

// C assembled from COO triplets as a handle of its own (coo.hip builds the arrays; the contract is in spmvHip.h, the design in
// DESIGN.md section 36).  What the host can decide is refused before any launch or allocation -- no kernel is handed a pointer
// that has not passed here --; an entry out of range is found by the build's first pass.  dC and info are written only on success.
int spmvHipCooAssemble(ulong M, ulong N, ulong nEntries, const uint32_t* dRow, const uint32_t* dCol, const double* dVal,
                       const spmvCooOpts* opts, spmat* dC, spmvCooInfo* info) {
    const char* who = "spmvHipCooAssemble";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dC) { ERR("%s: dC is NULL", who); return EXIT_FAILURE; }
    if (nEntries && (!dRow || !dCol || !dVal)) { ERR("%s: %s is NULL with nEntries = %lu", who, !dRow ? "dRow" : !dCol ? "dCol" : "dVal", nEntries); return EXIT_FAILURE; }
    const spmvCooOpts o = opts ? *opts : spmvCooOpts{SPMV_COO_SUM, 1};
    if (o.duplicates != SPMV_COO_SUM && o.duplicates != SPMV_COO_LAST) {
        ERR("%s: duplicates = %d is neither SPMV_COO_SUM nor SPMV_COO_LAST", who, o.duplicates);
        return EXIT_FAILURE;
    }
    if (M >= (1ull << 32) - 1 || N >= (1ull << 32) - 1) {
        ERR("%s: M=%lu, N=%lu: the assembled matrix has 32-bit row and column ids", who, M, N);
        return EXIT_FAILURE;
    }
    if (nEntries >= IRP32_LIMIT) {
        ERR("%s: nEntries=%lu: the entry order and the row pointers of the assembled matrix are 32-bit (limit %lu)", who, nEntries, (unsigned long)IRP32_LIMIT);
        return EXIT_FAILURE;
    }
    DevMat* c = new DevMat;
    c->M = M; c->N = N;
    setOrigin(c, Origin::ASSEMBLED);
    if (finishCsr(dC, c, !cooBuild(nEntries, dRow, dCol, dVal, &o, c, S.stream))) return EXIT_FAILURE;     // (the build has written its line)
    cooSetMaxRow(c);
    if (info) *info = *cooInfo(c);
    return EXIT_SUCCESS;
}

int spmvHipCooAssembleRefresh(spmat* dC, ulong nEntries, const double* dVal, spmvCooInfo* info) {
    const char* who = "spmvHipCooAssembleRefresh";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dC) { ERR("%s: dC is NULL", who); return EXIT_FAILURE; }
    DevMat* c = descOf(dC, who);
    if (!c || !madeBy(c, Origin::ASSEMBLED, nullptr, nullptr, who, "dC")) return EXIT_FAILURE;
    if (!cooHasMap(c)) { ERR("%s: dC was assembled with keepMap = 0 and keeps no map to refresh through: assemble again", who); return EXIT_FAILURE; }
    if (nEntries != cooEntries(c)) {
        ERR("%s: nEntries = %lu, but dC was assembled from %lu entries: a refresh takes the same list", who, nEntries, (unsigned long)cooEntries(c));
        return EXIT_FAILURE;
    }
    if (nEntries && !dVal) { ERR("%s: dVal is NULL", who); return EXIT_FAILURE; }
    c->iluPending = false;                              // AS is rewritten from here on, whatever becomes of the call
    if (cooRefresh(c, dVal, S.stream)) { ERR("%s: recomputing the values failed", who); return EXIT_FAILURE; }
    if (updateValues(dC, nullptr, true, true, S.stream, who)) return EXIT_FAILURE;
    if (info) *info = *cooInfo(c);
    return EXIT_SUCCESS;
}

int spmvHipCsrToCoo(spmat* dA, uint32_t* dRow, uint32_t* dCol, double* dVal) {
    const char* who = "spmvHipCsrToCoo";
    if (!ready(who)) return EXIT_FAILURE;
    DevMat* a = descOf(dA, who);
    if (!a || !csrOnly(a, who, "the source is an ELL handle (only CSR handles are written as triplets)")) return EXIT_FAILURE;
    if (a->NZ && (!dRow || !dCol)) { ERR("%s: %s is NULL with NZ = %lu", who, !dRow ? "dRow" : "dCol", (unsigned long)a->NZ); return EXIT_FAILURE; }
    if (a->M >= (1ull << 32) - 1) { ERR("%s: M=%lu rows do not fit the 32-bit row ids of the triplets", who, (unsigned long)a->M); return EXIT_FAILURE; }
    if (a->NZ && (!a->JA || !a->AS)) { ERR("%s: the source has no column or value array", who); return EXIT_FAILURE; }
    return csrToCoo(a, dRow, dCol, dVal, S.stream);
}

// ---- the approximate-inverse factor G of a square handle, G^T G ~ A^-1 (fsai.hip builds the arrays; the contract is in
// spmvHip.h, the design in DESIGN.md section 38).  dG owns G^T -- made and refreshed by the transpose path above -- and the
// workspace of an apply.  Refusals come first; dG and info are written only on success.

// hipSpILU0CSR's pattern check, made once per handle: every row strictly ascending
static bool strictRows(DevMat* d, const char* who, const char* name) {
    if (d->M && !d->iluChecked) {
        long row = -1;
        if (iluUnsortedRow(d, S.stream, &row)) { ERR("%s: the pattern check of %s failed", who, name); return false; }
        d->iluUnsortedRow = row;
        d->iluChecked = true;
    }
    if (d->M && d->iluUnsortedRow >= 0) {
        ERR("%s: row %ld of %s: its columns are not strictly ascending (unsorted, or a repeated column)", who, d->iluUnsortedRow, name);
        return false;
    }
    return true;
}

// dG as a factor of spmvHipFsaiSetup
static DevMat* fsaiOf(spmat* dG, const char* who) {
    if (!ready(who)) return nullptr;
    if (!dG) { ERR("%s: dG is NULL", who); return nullptr; }
    DevMat* g = descOf(dG, who);
    if (!g || !madeBy(g, Origin::FSAI, nullptr, nullptr, who, "dG")) return nullptr;
    return g;
}

int spmvHipFsaiSetup(spmat* dA, spmat* dS, const spmvFsaiOpts* opts, spmat* dG, spmvFsaiInfo* info) {
    const char* who = "spmvHipFsaiSetup";
    const auto t0 = std::chrono::steady_clock::now();
    if (!ready(who)) return EXIT_FAILURE;
    if (!dA || !dG) { ERR("%s: %s is NULL", who, !dA ? "dA" : "dG"); return EXIT_FAILURE; }
    if (dG == dA || dG == dS) { ERR("%s: dG is a source handle itself", who); return EXIT_FAILURE; }
    DevMat* a = squareCsrOf(dA, who, "dA is an ELL handle (only CSR handles have an approximate inverse)");
    if (!a) return EXIT_FAILURE;
    DevMat* s = dS ? squareCsrOf(dS, who, "dS is an ELL handle (the pattern is a CSR handle)") : a;
    if (!s) return EXIT_FAILURE;
    if (s->M != a->M) { ERR("%s: dS has %lu rows, dA %lu", who, (unsigned long)s->M, (unsigned long)a->M); return EXIT_FAILURE; }
    if (a->NZ && !a->AS) { ERR("%s: dA has no value array", who); return EXIT_FAILURE; }
    const unsigned lanes = opts ? opts->lanesPerRow : 0;
    if (lanes != 0 && lanes != 4 && lanes != 16 && lanes != 64) { ERR("%s: lanesPerRow %u is none of 0, 4, 16, 64", who, lanes); return EXIT_FAILURE; }
    if (!strictRows(a, who, "dA") || (s != a && !strictRows(s, who, "dS"))) return EXIT_FAILURE;
    DevMat* g = new DevMat;
    g->M = g->N = a->M;
    setOrigin(g, Origin::FSAI, a);
    FsaiPlan* p = g->fsai = new FsaiPlan;
    p->lanes = lanes;
    long longRow = -1;
    if (fsaiBuild(a, s, g, lanes, &p->info, &longRow, S.stream)) {
        if (longRow >= 0)
            ERR("%s: row %ld of the pattern gives a row of G of more than SPMV_FSAI_MAX_ROW = %d entries: filter the pattern", who, longRow,
                SPMV_FSAI_MAX_ROW);
        else ERR("%s: building the factor failed", who);
        freeDesc(g);
        return EXIT_FAILURE;
    }
    g->maxRowNnz = p->info.maxRow;
    // G^T by the transpose path; an empty factor has an empty transpose and asks for no kernel
    bool ok = false;
    DevMat* t = newMappedCsr(Origin::TRANSPOSE, g, g->M, g->M, &ok);
    if (ok && g->M == 0) ok = hipOk(hipMemset(t->IRP, 0, 4), "hipMemset");
    else if (ok) ok = !transposeCsr(g, t, S.stream);
    if (finishCsr(&p->hGT, t, ok)) { ERR("%s: building the factor's transpose failed", who); freeDesc(g); return EXIT_FAILURE; }
    p->gt = t;
    if (!hipOk(devMalloc(&p->work, std::max<size_t>(g->M, 1) * sizeof(double)), "hipMalloc the workspace")) { freeDesc(g); return EXIT_FAILURE; }
    if (finishCsr(&p->hG, g)) { ERR("%s: finishing the factor failed", who); return EXIT_FAILURE; }
    p->info.setups = 1;
    p->info.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *dG = p->hG;
    if (info) *info = p->info;
    return EXIT_SUCCESS;
}

int spmvHipFsaiRefresh(spmat* dG, spmat* dA, spmvFsaiInfo* info) {
    const char* who = "spmvHipFsaiRefresh";
    const auto t0 = std::chrono::steady_clock::now();
    DevMat* g = fsaiOf(dG, who);
    if (!g) return EXIT_FAILURE;
    if (!dA) { ERR("%s: dA is NULL", who); return EXIT_FAILURE; }
    DevMat* a = csrOf(dA, who, "dA is an ELL handle");
    if (!a || !madeBy(g, Origin::FSAI, a, nullptr, who, "dG", "dA")) return EXIT_FAILURE;
    if (a->NZ && !a->AS) { ERR("%s: dA has no value array", who); return EXIT_FAILURE; }
    FsaiPlan* p = g->fsai;
    spmvFsaiInfo out = p->info;
    out.launches = 0;
    g->iluPending = false;                              // AS is rewritten from here on, whatever becomes of the call
    if (fsaiValues(a, g, p->lanes, (uint32_t)p->info.maxRow, &out, S.stream)) { ERR("%s: recomputing the values failed", who); return EXIT_FAILURE; }
    // A factor stored in single precision: an update that fails only because a form could not follow (the array of a unit ->
    // non-unit transition refused) has left the doubles complete.  The refresh then goes on, so that G and G^T both hold the
    // new values, and the factor falls back to double storage as a whole; the call still fails, and says so.
    const bool wasF32 = p->storage == SPMV_STORAGE_F32;
    if (updateValues(dG, nullptr, true, true, S.stream, who) && !(wasF32 && !g->f32)) return EXIT_FAILURE;
    p->gt->iluPending = false;
    if (enqueueGatherValues(p->gt->AS, p->gt->tmap, p->gt->NZ, g->AS, S.stream)) return EXIT_FAILURE;
    if (updateValues(&p->hGT, nullptr, true, true, S.stream, who) && !(wasF32 && !p->gt->f32)) return EXIT_FAILURE;
    const bool lostF32 = wasF32 && !(g->f32 && p->gt->f32);
    if (lostF32) {
        valuesF32Drop(g);
        valuesF32Drop(p->gt);
        p->storage = SPMV_STORAGE_F64;
        ERR("%s: G and G^T hold the new values, but a single-precision form could not follow them: the factor is applied from its double "
            "values now (spmvHipFsaiSetStorage sets F32 again)", who);
    }
    ++out.launches;
    ++out.setups;
    out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    p->info = out;
    if (lostF32) return EXIT_FAILURE;
    if (info) *info = out;
    return EXIT_SUCCESS;
}

int spmvHipFsaiApply(spmat* dG, const double* dR, double* dZ) {
    const char* who = "spmvHipFsaiApply";
    const Ctx cx = libraryCtx();
    DevMat* g = fsaiOf(dG, who);
    if (!g) return EXIT_FAILURE;
    if (!dR || !dZ) { ERR("%s: %s is NULL", who, !dR ? "dR" : "dZ"); return EXIT_FAILURE; }
    if (dR != dZ && overlaps(dR, dZ, g->M * sizeof(double))) { ERR("%s: dR and dZ overlap without being equal", who); return EXIT_FAILURE; }
    if (g->M == 0) return nothingToLaunch(cx, g, nullptr);
    FsaiPlan* p = g->fsai;
    Launch L(cx, grid2d(g->nBlk2, WG_THREADS), dim3(WG_THREADS));
    const Ctx enqueue{cx.stream, false};                // w = G r, z = G^T w: the serial-order selection of each handle
    if (p->storage == SPMV_STORAGE_F32) {               // ... or, stored in single precision, the f32 product of each
        if (spmvHipEnqueueRowsF32(&p->hG, const_cast<double*>(dR), p->work, cx.stream) || spmvHipEnqueueRowsF32(&p->hGT, p->work, dZ, cx.stream)) {
            ERR("%s: launch failed", who);
            return EXIT_FAILURE;
        }
    } else if (autoRun(enqueue, &p->hG, const_cast<double*>(dR), p->work, 1, who) || autoRun(enqueue, &p->hGT, p->work, dZ, 1, who)) {
        ERR("%s: launch failed", who);
        return EXIT_FAILURE;
    }
    return L.finish(who);
}

int spmvHipFsaiTranspose(spmat* dG, spmat* dGT) {
    const char* who = "spmvHipFsaiTranspose";
    DevMat* g = fsaiOf(dG, who);
    if (!g) return EXIT_FAILURE;
    if (!dGT) { ERR("%s: dGT is NULL", who); return EXIT_FAILURE; }
    if (dGT == dG) { ERR("%s: dGT is the factor's handle itself", who); return EXIT_FAILURE; }
    *dGT = g->fsai->hGT;
    dGT->dev = nullptr;                                 // a view: the arrays stay the factor's
    return EXIT_SUCCESS;
}

int spmvHipFsaiInfo(spmat* dG, spmvFsaiInfo* info) {
    const char* who = "spmvHipFsaiInfo";
    DevMat* g = fsaiOf(dG, who);
    if (!g) return EXIT_FAILURE;
    if (!info) { ERR("%s: info is NULL", who); return EXIT_FAILURE; }
    *info = g->fsai->info;
    return EXIT_SUCCESS;
}

// the factor's products from single-precision storage (contract in spmvHip.h, design in DESIGN.md section 41): the form on G and
// on G^T, both or neither
int spmvHipFsaiSetStorage(spmat* dG, int storage) {
    const char* who = "spmvHipFsaiSetStorage";
    DevMat* g = fsaiOf(dG, who);
    if (!g) return EXIT_FAILURE;
    if (storage != SPMV_STORAGE_F64 && storage != SPMV_STORAGE_F32) {
        ERR("%s: storage %d is neither SPMV_STORAGE_F64 nor SPMV_STORAGE_F32", who, storage);
        return EXIT_FAILURE;
    }
    FsaiPlan* p = g->fsai;
    const int on = storage == SPMV_STORAGE_F32;
    if (valuesF32Set(g, on, S.stream, who) || valuesF32Set(p->gt, on, S.stream, who)) {
        valuesF32Drop(g);                               // (only a build fails)
        p->storage = SPMV_STORAGE_F64;
        ERR("%s: building the single-precision forms failed: the factor is applied from its double values", who);
        return EXIT_FAILURE;
    }
    p->storage = storage;
    return EXIT_SUCCESS;
}

int spmvHipFsaiStorage(spmat* dG, int* storage) {
    const char* who = "spmvHipFsaiStorage";
    DevMat* g = fsaiOf(dG, who);
    if (!g) return EXIT_FAILURE;
    if (!storage) { ERR("%s: storage is NULL", who); return EXIT_FAILURE; }
    *storage = g->fsai->storage;
    return EXIT_SUCCESS;
}

int spmvHipUpdateValues(spmat* dMat, const double* AS, int asOnDevice) {
    return updateValues(dMat, AS, asOnDevice != 0, false, S.stream, "spmvHipUpdateValues");
}
int spmvHipValuesChanged(spmat* dMat) { return updateValues(dMat, nullptr, true, true, S.stream, "spmvHipValuesChanged"); }
int spmvHipLastUpdateInfo(spmat* dMat, spmvUpdateInfo* info) {
    DevMat* d = descOf(dMat, "spmvHipLastUpdateInfo");
    if (!d || !info) return EXIT_FAILURE;
    *info = d->lastUpdate;
    return EXIT_SUCCESS;
}

int hipFreeSpmat(spmat* h) {
    if (!h || !h->dev) return EXIT_SUCCESS;
    DevMat* d = anyDescOf(h, "hipFreeSpmat");
    if (!d) return EXIT_FAILURE;
    freeDesc(d);
    memset(h, 0, sizeof *h);
    return EXIT_SUCCESS;
}

}  // extern "C"
