// jacobi.hpp -- the host's Ritz step that lanczos.hip and davidson.hip share: the cyclic-by-row Jacobi method on the
// projected matrix, operation by operation as include/spmvHip.h states it under hipSpLanczosCSR (JACOBI).  Both solvers
// hold the projected matrix and S as LZ_MAXM x LZ_MAXM host arrays, row i at [i*LZ_MAXM ..].
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace spmvhip {
namespace {

constexpr uint32_t LZ_MAXM = 64;                // columns of the basis at most; rows and columns of S at most
constexpr int      JACOBI_SWEEPS = 30;

// ------------------------------------------------------------------------------------------------ the host's Ritz step
// Cyclic-by-row Jacobi on the symmetric n x n matrix A (row i at A[i*LZ_MAXM ..]); S from the identity.  Returns the sweeps
// it took, the last of them without a rotation, or 0 when JACOBI_SWEEPS sweeps did not end so.  The conventions are the
// header's; tests/lanczos_ref.py's jacobi_ref is this loop.
int jacobi(uint32_t n, double* A, double* S) {
    auto at = [](double* M, uint32_t r, uint32_t c) -> double& { return M[(size_t)r * LZ_MAXM + c]; };
    for (uint32_t r = 0; r < n; ++r)
        for (uint32_t c = 0; c < n; ++c) at(S, r, c) = r == c ? 1.0 : 0.0;
    for (int sweep = 1; sweep <= JACOBI_SWEEPS; ++sweep) {
        bool rotated = false;
        for (uint32_t p = 0; p + 1 < n; ++p)
            for (uint32_t q = p + 1; q < n; ++q) {
                const double apq = at(A, p, q);
                if (apq == 0.0) continue;
                const double app = at(A, p, p), aqq = at(A, q, q), g = std::fabs(apq);
                if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {   // negligible: zeroed, no rotation
                    at(A, p, q) = at(A, q, p) = 0.0;
                    continue;
                }
                rotated = true;
                const double th = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (std::fabs(th) + std::sqrt(th * th + 1.0));
                if (th < 0.0) t = -t;
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c), h = t * apq;
                for (uint32_t r = 0; r < n; ++r) {
                    if (r == p || r == q) continue;
                    const double arp = at(A, r, p), arq = at(A, r, q);
                    at(A, r, p) = at(A, p, r) = arp - s * (arq + tau * arp);
                    at(A, r, q) = at(A, q, r) = arq + s * (arp - tau * arq);
                }
                at(A, p, p) = app - h;
                at(A, q, q) = aqq + h;
                at(A, p, q) = at(A, q, p) = 0.0;
                for (uint32_t r = 0; r < n; ++r) {
                    const double srp = at(S, r, p), srq = at(S, r, q);
                    at(S, r, p) = srp - s * (srq + tau * srp);
                    at(S, r, q) = srq + s * (srp - tau * srq);
                }
            }
        if (!rotated) return sweep;
    }
    return 0;
}

}  // namespace
}  // namespace spmvhip
