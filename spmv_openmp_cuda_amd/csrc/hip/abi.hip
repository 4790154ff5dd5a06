// abi.hip -- the extern "C" boundary of libspmvhip.so (declared in include/spmvHip.h): the library state, lifecycle, setters,
// vectors / memory / events and the LDS-order probe; upload.hip, launch.hip, select.hip and hostcall.hip hold the rest.
// Upload/free restate src/commons/cudaUtils.cu:20-98 + src/include/cudaUtils.h:70-78; the launchers replace
// `f<<<grid,block>>>(dMat,dVect,Conf,dOutV)` of src/main.cu:221-238 and test/SpMV_test.cu:103-146.
#include <hip/hip_runtime.h>
#include <cstring>

#include "lib.hpp"
#include "alloc_ledger.hpp"

using namespace spmvhip;

namespace {
__global__ void fill64_kernel(uint64_t* p, size_t n, uint64_t v) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}

// What the deterministic format kernels rest on is measured behaviour of the LDS, not something the ISA manual promises:
// (a) lanes of ONE ds_add_f64 instruction that meet in an address are added in ascending lane order, (b) the LDS operations
// of one wavefront execute in issue order.  This probe checks both against sums computed on the host in that order (the
// values are chosen so that other orders give other bits); the serial-order selection offers the format kernels only
// where it passes, so the bitwise contract of hipSpMVRowsCSR never depends on the property silently.
// (The accumulator of every add is read from memory: with an address the compiler can prove wavefront-uniform its atomic
// optimizer would replace the 64 adds by a wavefront reduction and ONE add -- another summation order, and not what the
// SpMV kernels, whose addresses are per-lane rows, execute.)
__global__ __launch_bounds__(64) void lds_order_probe_kernel(const double* __restrict__ v, const uint32_t* __restrict__ slot,
                                                             double* __restrict__ out) {
    __shared__ double acc[4];
    const uint32_t lane = threadIdx.x;
    if (lane < 4) acc[lane] = 0.0;
    __syncthreads();
    atomicAdd(&acc[slot[lane]], v[lane]);                    // 64 lanes, one address
    atomicAdd(&acc[slot[64 + lane]], v[64 + lane]);          // two addresses, 32 lanes each
    atomicAdd(&acc[slot[128 + lane]], v[128 + lane]);        // a second instruction into the first address: behind the first one
    if (slot[192 + lane] < 4) atomicAdd(&acc[slot[192 + lane]], v[192 + lane]);   // a sparse lane mask
    __syncthreads();
    if (lane < 4) out[lane] = acc[lane];
}
}  // namespace

namespace spmvhip {

State S;
hipStream_t libraryStream() { return S.stream; }

// The allocation chokepoint: the only two calls of the runtime's allocator in the library, behind the ledger.
static AllocLedger& ledger() {
    static AllocLedger l([](void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }, [](void* p) { return (int)hipFree(p); },
                         (int)hipErrorOutOfMemory);
    return l;
}
hipError_t devMalloc(void** p, size_t bytes) { return (hipError_t)ledger().allocate(p, bytes); }
hipError_t devFree(void* p) { return (hipError_t)ledger().release(p); }

int probeLdsOrder(hipStream_t stream) {
    if (!ready("spmvHipProbeLdsAtomicOrder")) return -1;
    if (S.ldsOrder >= 0) return S.ldsOrder;
    double h[256], expect[4] = {0, 0, 0, 0}, got[4] = {0, 0, 0, 0};
    for (int i = 0; i < 256; ++i) h[i] = (i % 2 ? -1.0 : 1.0) / (3.0 + 7.0 * i) + (i % 5) * 0x1.0p-20;
    volatile double a0 = 0, a1 = 0, a2 = 0, a3 = 0;  // (volatile: plain sequential adds, whatever the host compiler would like to do)
    for (int l = 0; l < 64; ++l) a0 = a0 + h[l];
    for (int l = 0; l < 64; ++l) { if (l & 1) a2 = a2 + h[64 + l]; else a1 = a1 + h[64 + l]; }
    for (int l = 0; l < 64; ++l) a0 = a0 + h[128 + l];
    for (int l = 0; l < 64; l += 3) a3 = a3 + h[192 + l];
    expect[0] = a0; expect[1] = a1; expect[2] = a2; expect[3] = a3;
    uint32_t slot[256];
    for (int l = 0; l < 64; ++l) { slot[l] = 0; slot[64 + l] = 1 + (l & 1); slot[128 + l] = 0; slot[192 + l] = l % 3 == 0 ? 3 : 99; }
    double *dV = nullptr, *dOut = nullptr;
    uint32_t* dSlot = nullptr;
    int ok = 0;
    if (devMalloc(&dV, sizeof h) == hipSuccess && devMalloc(&dOut, sizeof got) == hipSuccess && devMalloc(&dSlot, sizeof slot) == hipSuccess &&
        hipMemcpy(dV, h, sizeof h, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dSlot, slot, sizeof slot, hipMemcpyHostToDevice) == hipSuccess) {
        ok = 1;
        for (int rep = 0; rep < 4 && ok; ++rep) {    // a few launches: the answer must not depend on timing
            hipLaunchKernelGGL(lds_order_probe_kernel, dim3(1), dim3(64), 0, stream, dV, dSlot, dOut);
            if (hipStreamSynchronize(stream) != hipSuccess || hipMemcpy(got, dOut, sizeof got, hipMemcpyDeviceToHost) != hipSuccess) { ok = 0; break; }
            ok = memcmp(got, expect, sizeof got) == 0;
        }
    }
    (void)devFree(dV); (void)devFree(dOut); (void)devFree(dSlot);
    (void)hipGetLastError();
    S.ldsOrder = ok;
    return ok;
}

int vecFill(Ctx cx, double* dVec, size_t n, uint64_t pattern) {
    if (n == 0) return EXIT_SUCCESS;
    unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(fill64_kernel, dim3(grid), dim3(256), 0, cx.stream, reinterpret_cast<uint64_t*>(dVec), n, pattern);
    HIP_TRY(hipGetLastError());
    if (cx.sync) HIP_TRY(hipStreamSynchronize(cx.stream));
    return EXIT_SUCCESS;
}

}  // namespace spmvhip

extern "C" {

// ------------------------------------------------------------------------ lifecycle
int spmvHipDeviceCount(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

int spmvHipInit(int dev, size_t sizeofSpmat, size_t sizeofConfig) {
    if (sizeofSpmat != sizeof(spmat) || sizeofConfig != sizeof(CONFIG)) {
        ERR("spmvHipInit: layout mismatch: caller spmat/CONFIG = %zu/%zu bytes, library %zu/%zu "
            "(compile the host with this repo's include/spmv_types.h)",
            sizeofSpmat, sizeofConfig, sizeof(spmat), sizeof(CONFIG));
        return EXIT_FAILURE;
    }
    int n = spmvHipDeviceCount();
    if (n <= 0) { ERR("spmvHipInit: no HIP device visible -- this library has no CPU fallback"); return EXIT_FAILURE; }
    if (dev < 0 || dev >= n) { ERR("spmvHipInit: device %d out of range [0,%d)", dev, n); return EXIT_FAILURE; }
    HIP_TRY(hipSetDevice(dev));
    if (!S.ev0) HIP_TRY(hipEventCreate(&S.ev0));
    if (!S.ev1) HIP_TRY(hipEventCreate(&S.ev1));
    S.dev = dev;
    S.inited = true;
    return EXIT_SUCCESS;
}

int spmvHipFinalize(void) {
    if (!S.inited) return EXIT_SUCCESS;
    spmvHipDropCache();
    freeTilesWorkspace();
    freeDotWorkspace();
    peerFinalize();
    freePushStream();
    if (S.ev0) (void)hipEventDestroy(S.ev0);
    if (S.ev1) (void)hipEventDestroy(S.ev1);
    S.ev0 = S.ev1 = nullptr;
    S.inited = false;
    return EXIT_SUCCESS;
}

int spmvHipSetStream(void* stream) { S.stream = static_cast<hipStream_t>(stream); return EXIT_SUCCESS; }
int spmvHipSetSync(int sync) { S.sync = sync != 0; return EXIT_SUCCESS; }
double spmvHipLastKernelSeconds(void) { return S.lastSeconds; }
int spmvHipLastLaunch(spmvDim3* grid, spmvDim3* block) {
    if (grid) *grid = S.lastGrid;
    if (block) *block = S.lastBlock;
    return EXIT_SUCCESS;
}
int spmvHipDeviceSynchronize(void) { HIP_TRY(hipDeviceSynchronize()); return EXIT_SUCCESS; }

int spmvHipProbeLdsAtomicOrder(void) { return probeLdsOrder(S.stream); }

int spmvHipSetVariant(const char* launcher, int variant) {
    if (!launcher) return EXIT_FAILURE;
    if (!strcmp(launcher, "hipSpMVRowsCSR") && variant >= 0 && variant <= 2) { S.variantRowsCSR = variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "hipSpMVWarpPerRowCSR") && variant >= 0 && variant <= 2) { S.variantWarpCSR = variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "hipSpMVRowsELLNNTransposed") && variant >= 0 && variant <= 1) { S.variantEllRowMajor = variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "hipSpTRSVCSR") && variant >= 0 && variant <= 65536) { S.triRunRows = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "hipSpILU0CSR") && (variant == 8 || variant == 16 || variant == 64)) { S.iluGroup = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "hipSpCGCSR") && variant >= 1 && variant <= 4096) { S.krylovK[0] = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "hipSpBiCGStabCSR") && variant >= 1 && variant <= 4096) { S.krylovK[1] = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "hipSpCGBlockCSR") && variant >= 1 && variant <= 4096) { S.krylovBlockK[0] = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "hipSpBiCGStabBlockCSR") && variant >= 1 && variant <= 4096) { S.krylovBlockK[1] = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "hipSpGMRESCSR") && (variant == 0 || variant == 1)) { S.gmresFused = variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "spmvHipColourCSR") && variant >= 1 && variant <= 4096) { S.colourK = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "spmvHipAggregateCSR") && variant >= 1 && variant <= 4096) { S.aggK = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "spmvHipRcmCSR") && variant >= 0) { S.rcmT = (uint32_t)std::min(variant, 1024); return EXIT_SUCCESS; }
    if (!strcmp(launcher, "spmvHipAmgApply") && variant >= 0 && variant <= 4096) { S.amgFuseMax = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "spmvHipAmgSetGaussSeidel") && variant >= 0 && variant <= 65536) { S.amgGsSmallRows = (uint32_t)variant; return EXIT_SUCCESS; }
    if (!strcmp(launcher, "spmvHipAmgGaussSeidel") && (variant == 0 || variant == 1 || variant == 4 || variant == 8 || variant == 16 || variant == 32 || variant == 64)) {
        S.amgGsLanes = (uint32_t)variant;
        return EXIT_SUCCESS;
    }
    ERR("spmvHipSetVariant: unknown (%s, %d)", launcher, variant);
    return EXIT_FAILURE;
}
int spmvHipSetEllRowLens(int use) { S.ellRowLens = use != 0; return EXIT_SUCCESS; }
int spmvHipSetUnitValues(int on) { S.unitValues = on != 0; return EXIT_SUCCESS; }
int spmvHipUnitValue(spmat* dMat, double* value) {
    DevMat* d = descOf(dMat, "spmvHipUnitValue");
    if (!d) return -1;
    if (d->unit && value) *value = d->unitValue;
    return d->unit ? 1 : 0;
}

// ------------------------------------------------------------------------ vectors
int spmvHipVecAlloc(double** dVec, size_t n) {
    if (!ready("spmvHipVecAlloc") || !dVec) return EXIT_FAILURE;
    HIP_TRY(devMalloc(dVec, std::max<size_t>(n, 1) * sizeof(double)));
    return EXIT_SUCCESS;
}
int spmvHipVecFree(double* dVec) { HIP_TRY(devFree(dVec)); return EXIT_SUCCESS; }
int spmvHipVecUp(double* dVec, const double* hVec, size_t n) {
    HIP_TRY(hipMemcpyAsync(dVec, hVec, n * sizeof(double), hipMemcpyHostToDevice, S.stream));
    HIP_TRY(hipStreamSynchronize(S.stream));
    return EXIT_SUCCESS;
}
int spmvHipVecDown(double* hVec, const double* dVec, size_t n) {
    HIP_TRY(hipMemcpyAsync(hVec, dVec, n * sizeof(double), hipMemcpyDeviceToHost, S.stream));
    HIP_TRY(hipStreamSynchronize(S.stream));
    return EXIT_SUCCESS;
}
int spmvHipVecFill(double* dVec, size_t n, uint64_t pattern) { return vecFill(libraryCtx(), dVec, n, pattern); }

int spmvHipMalloc(void** dPtr, size_t bytes) {
    if (!ready("spmvHipMalloc") || !dPtr) return EXIT_FAILURE;
    HIP_TRY(devMalloc(dPtr, std::max<size_t>(bytes, 1)));
    return EXIT_SUCCESS;
}
int spmvHipFree(void* dPtr) { HIP_TRY(devFree(dPtr)); return EXIT_SUCCESS; }
int spmvHipMemcpyUp(void* dDst, const void* hSrc, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dDst, hSrc, bytes, hipMemcpyHostToDevice, S.stream));
    HIP_TRY(hipStreamSynchronize(S.stream));
    return EXIT_SUCCESS;
}
int spmvHipMemcpyDown(void* hDst, const void* dSrc, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(hDst, dSrc, bytes, hipMemcpyDeviceToHost, S.stream));
    HIP_TRY(hipStreamSynchronize(S.stream));
    return EXIT_SUCCESS;
}

int spmvHipAllocRefuse(long n, int fromThenOn) { ledger().arm(n, fromThenOn != 0); return EXIT_SUCCESS; }
int spmvHipAllocStats(spmvAllocStats* stats) {
    if (!stats) return EXIT_FAILURE;
    const AllocCounts c = ledger().counts();
    *stats = spmvAllocStats{c.live, c.liveBytes, c.peakBytes, c.calls, c.refused, c.badFrees};
    return EXIT_SUCCESS;
}

// ------------------------------------------------------------------------ events
int spmvHipEventCreate(void** ev) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    *ev = e;
    return EXIT_SUCCESS;
}
int spmvHipEventDestroy(void* ev) { HIP_TRY(hipEventDestroy(static_cast<hipEvent_t>(ev))); return EXIT_SUCCESS; }
int spmvHipEventRecord(void* ev) { HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(ev), S.stream)); return EXIT_SUCCESS; }
int spmvHipEventElapsedMs(void* a, void* b, float* ms) {
    HIP_TRY(hipEventSynchronize(static_cast<hipEvent_t>(b)));
    HIP_TRY(hipEventElapsedTime(ms, static_cast<hipEvent_t>(a), static_cast<hipEvent_t>(b)));
    return EXIT_SUCCESS;
}

}  // extern "C"
