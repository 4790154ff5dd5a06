// hostcall.hip -- the SPMV_INTERF-style wrappers: a host matrix in, a host vector out, the device copy cached.
#include <hip/hip_runtime.h>
#include <map>
#include <vector>

#include "lib.hpp"

using namespace spmvhip;

namespace {
// Device copy of a host matrix behind the SPMV_INTERF-style wrappers.  The key is the host struct's address; the
// entry also remembers the shape and the array pointers it was uploaded from, and is re-uploaded when any of them
// differs (a freed struct whose address malloc handed out again, a matrix re-loaded in place).  Changing the VALUES
// inside the same arrays is invisible here: call spmvHipDropCache() before a cached host matrix is modified or freed.
struct Cached {
    spmat handle{}; double* dx = nullptr; double* dy = nullptr; int kind = 0;
    ulong M = 0, N = 0, NZ = 0, K = 0; const void *irp = nullptr, *ja = nullptr, *as = nullptr, *rl = nullptr;
    bool sameSource(const spmat* m, int k) const {
        return kind == k && M == m->M && N == m->N && NZ == m->NZ && K == m->MAX_ROW_NZ && irp == m->IRP && ja == m->JA && as == m->AS && rl == m->RL;
    }
    void release() { hipFreeSpmat(&handle); (void)devFree(dx); (void)devFree(dy); dx = dy = nullptr; }
};
std::map<const spmat*, Cached> g_cache;

int hostCall(spmat* mat, double* x, CONFIG* cfg, double* y, int kind, LaunchFn* fn) {
    if (!ready("spmvHip*") || !mat || !x || !y) return EXIT_FAILURE;
    auto it = g_cache.find(mat);
    if (it != g_cache.end() && !it->second.sameSource(mat, kind)) { it->second.release(); g_cache.erase(it); it = g_cache.end(); }
    if (it == g_cache.end()) {
        Cached c; c.kind = kind;
        c.M = mat->M; c.N = mat->N; c.NZ = mat->NZ; c.K = mat->MAX_ROW_NZ; c.irp = mat->IRP; c.ja = mat->JA; c.as = mat->AS; c.rl = mat->RL;
        int rc;
        if (kind == 0) rc = spMatCpyCSR(mat, &c.handle);
        else if (kind == 1) rc = spMatCpyELL(mat, &c.handle);
        else {  // column-major ELL: transposition is done on the fly from the row-major host matrix
            if (!mat->JA || !mat->AS) { ERR("spmvHipRowsELL: host matrix has no ELL arrays"); return EXIT_FAILURE; }
            spmat t = *mat;
            std::vector<ulong> ja(mat->M * mat->MAX_ROW_NZ);
            std::vector<double> as(mat->M * mat->MAX_ROW_NZ);
            for (ulong r = 0; r < mat->M; ++r)
                for (ulong c2 = 0; c2 < mat->MAX_ROW_NZ; ++c2) {
                    ja[c2 * mat->M + r] = mat->JA[r * mat->MAX_ROW_NZ + c2];
                    as[c2 * mat->M + r] = mat->AS[r * mat->MAX_ROW_NZ + c2];
                }
            t.JA = ja.data(); t.AS = as.data();
            t.M = mat->MAX_ROW_NZ; t.N = mat->M; t.MAX_ROW_NZ = mat->M;
            t.pitchJA = mat->N;                      // column count for the upload's range check
            rc = spMatCpyELLTransposed(&t, &c.handle);
        }
        if (rc) return EXIT_FAILURE;
        if (spmvHipVecAlloc(&c.dx, mat->N) || spmvHipVecAlloc(&c.dy, mat->M)) { c.release(); return EXIT_FAILURE; }
        it = g_cache.emplace(mat, c).first;
    }
    Cached& c = it->second;
    const Ctx cx{S.stream, true};                        // a host vector comes back: always synchronous
    int rc = spmvHipVecUp(c.dx, x, mat->N);
    if (!rc) rc = vecFill(cx, c.dy, mat->M, 0x7FF8DEADDEADDEADull);        // poison y
    if (!rc) rc = fn(cx, &c.handle, c.dx, cfg ? *cfg : CONFIG{}, c.dy);
    if (!rc) rc = spmvHipVecDown(y, c.dy, mat->M);
    return rc;
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------------ SPMV_INTERF wrappers
int spmvHipRowsCSR(spmat* mat, double* x, CONFIG* cfg, double* y) { return hostCall(mat, x, cfg, y, 0, &rowsCSR); }
int spmvHipWarpPerRowCSR(spmat* mat, double* x, CONFIG* cfg, double* y) { return hostCall(mat, x, cfg, y, 0, &warpPerRowCSR); }
int spmvHipRowsELL(spmat* mat, double* x, CONFIG* cfg, double* y) { return hostCall(mat, x, cfg, y, 2, &rowsELL); }
int spmvHipWarpsPerRowELL(spmat* mat, double* x, CONFIG* cfg, double* y) { return hostCall(mat, x, cfg, y, 1, &warpsPerRowELL); }
int spmvHipDropCache(void) {
    for (auto& kv : g_cache) kv.second.release();
    g_cache.clear();
    return EXIT_SUCCESS;
}

}  // extern "C"
