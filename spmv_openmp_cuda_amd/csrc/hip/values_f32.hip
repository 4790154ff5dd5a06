// values_f32.hip -- the single-precision value form of a CSR handle (spmvHipValuesF32; contract in spmvHip.h, design in
// DESIGN.md section 41): AS32[p] = (float)AS[p], built by one elementwise pass that also counts what the rounding did, kept
// on the handle and rewritten from AS whenever the values change (updateValues, upload.hip).  The products that stream it
// are the V = float instances of csr_stream2_kernel (kernels.hpp, launched from launch.hip) and csr_spmm_kernel (spmm.hip).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

#include "lib.hpp"

using namespace spmvhip;

namespace {

constexpr uint32_t DEMOTE_THREADS = 256;
constexpr uint32_t DEMOTE_PER_LANE = 4;                       // one 16-B store, two 16-B loads
constexpr uint32_t DEMOTE_CHUNK = DEMOTE_THREADS * DEMOTE_PER_LANE;
typedef double d2_t __attribute__((ext_vector_type(2)));      // 16-B accesses as the compiler's own vector types
typedef float  f4_t __attribute__((ext_vector_type(4)));
enum { C_INEXACT = 0, C_OVERFLOW = 1, C_FLUSHED = 2, C_FIRST = 3, C_WORDS = 4 };   // the counters behind the array

// what rounding did to one entry, as bits 0 (inexact), 1 (overflowed), 2 (flushed).  The conversion is the hardware's
// v_cvt_f32_f64 in the kernel's default mode: round to nearest even, subnormal results kept.
__device__ __forceinline__ uint32_t demote_one(double d, float* out) {
    const float f = (float)d;
    *out = f;
    const bool nan = d != d;
    const bool inexact = !nan && (double)f != d;
    const bool overflow = inexact && fabs(d) <= 1.79769313486231570815e+308 && fabsf(f) > 3.40282346638528859812e+38f;
    const bool flushed = inexact && f == 0.0f;                // (d != 0 follows from inexact)
    return (inexact ? 1u : 0u) | (overflow ? 2u : 0u) | (flushed ? 4u : 0u);
}

// AS32[p] = (float)AS[p] for p in [0, n).  VEC: AS is 16-B aligned (every array the library made; an adopted one may not
// be) -- a lane takes 4 consecutive entries, two 16-B non-temporal loads and one 16-B store; otherwise one entry per lane
// and access.  AS32 is the library's own allocation and always aligned.  The counts: a wavefront in which any lane
// saw something (one ballot) sums its lanes' integer counts by shuffles, and lane 0 adds the three sums with integer atomics
// and takes the minimum of the first overflowed place.
template <bool VEC>
__global__ __launch_bounds__(DEMOTE_THREADS) void csr_demote_kernel(uint64_t n, const double* __restrict__ AS, float* __restrict__ AS32,
                                                                    unsigned long long* __restrict__ counts) {
    const uint64_t p0 = (linear_block() * DEMOTE_THREADS + threadIdx.x) * DEMOTE_PER_LANE;
    uint32_t flags[DEMOTE_PER_LANE] = {0, 0, 0, 0};
    if (VEC && p0 + DEMOTE_PER_LANE <= n) {
        const d2_t a = __builtin_nontemporal_load(reinterpret_cast<const d2_t*>(AS + p0));
        const d2_t b = __builtin_nontemporal_load(reinterpret_cast<const d2_t*>(AS + p0 + 2));
        float f0, f1, f2, f3;
        flags[0] = demote_one(a.x, &f0); flags[1] = demote_one(a.y, &f1);
        flags[2] = demote_one(b.x, &f2); flags[3] = demote_one(b.y, &f3);
        *reinterpret_cast<f4_t*>(AS32 + p0) = f4_t{f0, f1, f2, f3};
    } else {
#pragma unroll
        for (uint32_t u = 0; u < DEMOTE_PER_LANE; ++u)
            if (p0 + u < n) {
                float f;
                flags[u] = demote_one(__builtin_nontemporal_load(AS + p0 + u), &f);
                AS32[p0 + u] = f;
            }
    }
    uint32_t any = 0, nIn = 0, nOv = 0, nFl = 0;
    unsigned long long first = ~0ull;
#pragma unroll
    for (uint32_t u = 0; u < DEMOTE_PER_LANE; ++u) {
        any |= flags[u];
        nIn += flags[u] & 1u; nOv += (flags[u] >> 1) & 1u; nFl += (flags[u] >> 2) & 1u;
        if ((flags[u] & 2u) && first == ~0ull) first = p0 + u;
    }
    if (!__any(any != 0)) return;                             // (wave-uniform: the usual case costs one ballot)
    // sums over the wavefront by shuffles of integers
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        nIn += __shfl_down(nIn, off, WAVE); nOv += __shfl_down(nOv, off, WAVE); nFl += __shfl_down(nFl, off, WAVE);
        const unsigned long long o = __shfl_down(first, off, WAVE);
        first = o < first ? o : first;
    }
    if (threadIdx.x % WAVE == 0) {
        if (nIn) atomicAdd(counts + C_INEXACT, (unsigned long long)nIn);
        if (nOv) atomicAdd(counts + C_OVERFLOW, (unsigned long long)nOv);
        if (nFl) atomicAdd(counts + C_FLUSHED, (unsigned long long)nFl);
        if (first != ~0ull) atomicMin(counts + C_FIRST, first);
    }
}

size_t arrayBytes(uint64_t nz) { return (size_t)((nz * 4 + 15) / 16 * 16); }
unsigned long long* countsOf(const DevMat* d) { return reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(d->AS32) + arrayBytes(d->NZ)); }

// the rounding of one double on the host, and what it did: the same bits as demote_one (x86-64 cvtsd2ss under the default
// MXCSR: round to nearest even, subnormals kept)
uint32_t demoteHost(double d, float* out) {
    const volatile float f = (float)d;
    *out = f;
    const bool nan = d != d, inexact = !nan && (double)f != d;
    const bool overflow = inexact && std::fabs(d) <= 1.79769313486231570815e+308 && std::fabs(f) > 3.40282346638528859812e+38f;
    const bool flushed = inexact && f == 0.0f;
    return (inexact ? 1u : 0u) | (overflow ? 2u : 0u) | (flushed ? 4u : 0u);
}

}  // namespace

namespace spmvhip {

void valuesF32Drop(DevMat* d) {
    (void)devFree(d->AS32);
    d->AS32 = nullptr;
    d->f32 = false;
    d->unitValue32 = 0.0;
    d->f32Info = spmvF32Info{0, 0, 0, 0, 0, 0, 0, -1};
}

// the form brought up to the handle's current AS / unit state; `fresh`: a build, not a refresh
static int bringUp(DevMat* d, hipStream_t st, const char* who, bool fresh) {
    spmvF32Info info = d->f32Info;
    info.refreshes = fresh ? 0 : info.refreshes + 1;
    info.inexact = info.overflowed = info.flushed = 0;
    info.firstOverflow = -1;
    if (d->unit || d->NZ == 0) {                                // no stream to store: the register value (an empty handle: nothing)
        (void)devFree(d->AS32);
        d->AS32 = nullptr;
        float f = 0.0f;
        const uint32_t flags = d->unit ? demoteHost(d->unitValue, &f) : 0u;
        d->unitValue32 = (double)f;
        info.unit = d->unit ? 1 : 0;
        info.bytes = 0;
        if (flags & 1u) info.inexact = d->NZ;
        if (flags & 2u) { info.overflowed = d->NZ; info.firstOverflow = 0; }
        if (flags & 4u) info.flushed = d->NZ;
    } else {
        const size_t bytes = arrayBytes(d->NZ) + C_WORDS * sizeof(unsigned long long);
        if (!d->AS32 && !hipOk(devMalloc(&d->AS32, bytes), "hipMalloc AS32")) {
            ERR("%s: the single-precision value form could not be allocated (%zu bytes): the handle has no such form now, build it again "
                "with spmvHipValuesF32", who, bytes);
            valuesF32Drop(d);
            return EXIT_FAILURE;
        }
        unsigned long long* counts = countsOf(d);
        const unsigned long long init[C_WORDS] = {0, 0, 0, ~0ull};
        unsigned long long got[C_WORDS] = {0, 0, 0, ~0ull};
        const bool vec = ((uintptr_t)d->AS & 15u) == 0;
        const dim3 grid = grid2d((d->NZ + DEMOTE_CHUNK - 1) / DEMOTE_CHUNK, DEMOTE_THREADS);
        bool ok = hipOk(hipMemcpyAsync(counts, init, sizeof init, hipMemcpyHostToDevice, st), "hipMemcpy the counters");
        if (ok) {
            if (vec) hipLaunchKernelGGL(csr_demote_kernel<true>, grid, dim3(DEMOTE_THREADS), 0, st, d->NZ, d->AS, d->AS32, counts);
            else     hipLaunchKernelGGL(csr_demote_kernel<false>, grid, dim3(DEMOTE_THREADS), 0, st, d->NZ, d->AS, d->AS32, counts);
            ok = hipOk(hipGetLastError(), "csr_demote_kernel") &&
                 hipOk(hipMemcpyAsync(got, counts, sizeof got, hipMemcpyDeviceToHost, st), "hipMemcpy the counters") &&
                 hipOk(hipStreamSynchronize(st), "csr_demote_kernel");
        }
        if (!ok) {
            ERR("%s: rounding the values to single precision failed: the handle has no such form now", who);
            valuesF32Drop(d);
            return EXIT_FAILURE;
        }
        d->unitValue32 = 0.0;
        info.unit = 0;
        info.bytes = bytes;
        info.inexact = got[C_INEXACT]; info.overflowed = got[C_OVERFLOW]; info.flushed = got[C_FLUSHED];
        info.firstOverflow = got[C_FIRST] == ~0ull ? -1 : (long)got[C_FIRST];
    }
    info.built = 1;
    d->f32 = true;
    d->f32Info = info;
    return EXIT_SUCCESS;
}

int valuesF32Follow(DevMat* d, hipStream_t st, const char* who) { return d->f32 ? bringUp(d, st, who, false) : EXIT_SUCCESS; }

int valuesF32Set(DevMat* d, int on, hipStream_t st, const char* who) {
    if (!on) { valuesF32Drop(d); return EXIT_SUCCESS; }
    if (d->f32) return EXIT_SUCCESS;
    if (d->NZ && !d->AS && !d->unit) { ERR("%s: the handle has no value array", who); return EXIT_FAILURE; }
    return bringUp(d, st, who, true);
}

}  // namespace spmvhip

extern "C" {

int spmvHipValuesF32(spmat* dMat, int on) {
    const char* who = "spmvHipValuesF32";
    if (!ready(who)) return EXIT_FAILURE;
    if (!dMat) { ERR("%s: dMat is NULL", who); return EXIT_FAILURE; }
    if (liveShard(dMat)) { ERR("%s: the handle is a sharded matrix (spmvHipShardCSR), which has no single-precision value form", who); return EXIT_FAILURE; }
    DevMat* d = csrOf(dMat, who, "the handle is an ELL handle (only CSR handles have a single-precision value form)");
    return d ? valuesF32Set(d, on, S.stream, who) : EXIT_FAILURE;
}

int spmvHipValuesF32Info(spmat* dMat, spmvF32Info* info) {
    const char* who = "spmvHipValuesF32Info";
    if (!dMat) { ERR("%s: dMat is NULL", who); return EXIT_FAILURE; }
    if (liveShard(dMat)) { ERR("%s: the handle is a sharded matrix (spmvHipShardCSR), which has no single-precision value form", who); return EXIT_FAILURE; }
    DevMat* d = csrOf(dMat, who, "the handle is an ELL handle (only CSR handles have a single-precision value form)");
    if (!d) return EXIT_FAILURE;
    if (!info) { ERR("%s: info is NULL", who); return EXIT_FAILURE; }
    *info = d->f32Info;
    return EXIT_SUCCESS;
}

}  // extern "C"
