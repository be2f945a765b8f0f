// info_pack.h -- edge information matrices on the host (PoseGraphSolver::set_information / get_information):
// the packed layout the device reads (pg_device.hpp: info_unpack), the checks every matrix passes before anything changes, and
// the way back to full matrices.  Plain host C++: tests/host_harness_info_pack.cpp.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace apex {

// Omega travels packed: the upper triangle row-major, D (D + 1) / 2 doubles padded to an even count (16-byte loads)
constexpr int info_packed(int D) { return D * (D + 1) / 2; }
constexpr int info_stride(int D) { return (info_packed(D) + 1) & ~1; }   // D = 6: 22, D = 3: 6
template <int D>
struct InfoPack {
    static constexpr int kPacked = info_packed(D);
    static constexpr int kStride = info_stride(D);
};

// info [n_e][D * D] row-major -> *packed [n_e][info_stride(D)], zero on the padding.  Every matrix must be finite, symmetric to
// 1e-12 max|Omega| and positive definite (a Cholesky Omega = U^T U from the upper triangle, every pivot > 0).  false: *err names
// the first edge and check that failed (behind "set_information: edge <e>"), *packed is not to be used.  D <= 6.
inline bool info_validate_and_pack(int D, int64_t n_e, const double* info, std::vector<double>* packed, std::string* err) {
    const int S = info_stride(D);
    packed->assign((size_t)n_e * S, 0.0);
    for (int64_t e = 0; e < n_e; ++e) {
        const double* W = info + (size_t)e * D * D;
        const std::string who = "set_information: edge " + std::to_string(e);
        double big = 0.0;
        for (int i = 0; i < D * D; ++i) {
            if (!std::isfinite(W[i])) { *err = who + " has an entry that is not finite"; return false; }
            big = std::max(big, fabs(W[i]));
        }
        for (int i = 0; i < D; ++i)
            for (int j = i + 1; j < D; ++j)
                if (fabs(W[D * i + j] - W[D * j + i]) > 1e-12 * big) { *err = who + " is not symmetric"; return false; }
        double U[36];   // Omega = U^T U from the upper triangle
        for (int i = 0; i < D; ++i)
            for (int j = i; j < D; ++j) {
                double acc = W[D * i + j];
                for (int k = 0; k < i; ++k) acc -= U[D * k + i] * U[D * k + j];
                if (i == j) {
                    if (!(acc > 0.0)) { *err = who + " is not positive definite (Cholesky pivot " + std::to_string(i) + " <= 0)"; return false; }
                    U[D * i + i] = sqrt(acc);
                } else {
                    U[D * i + j] = acc / U[D * i + i];
                }
            }
        double* p = packed->data() + (size_t)e * S;
        for (int i = 0; i < D; ++i)
            for (int j = i; j < D; ++j) *p++ = W[D * i + j];
    }
    return true;
}

// packed [n_e][info_stride(D)] -> out [n_e][D * D], full and symmetric
inline void info_expand(int D, int64_t n_e, const double* packed, double* out) {
    const int S = info_stride(D);
    for (int64_t e = 0; e < n_e; ++e) {
        const double* p = packed + (size_t)e * S;
        double* W = out + (size_t)e * D * D;
        for (int i = 0; i < D; ++i)
            for (int j = i; j < D; ++j) { W[D * i + j] = *p; W[D * j + i] = *p; ++p; }
    }
}

}  // namespace apex
