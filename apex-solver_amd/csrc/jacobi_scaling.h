// jacobi_scaling.h -- the Jacobi column scaling of one segment of the unknowns (process_jacobian_generic, optimizer/mod.rs:749-763):
// the device vector the kernels multiply by, in internal order with 1 on the padding of the last tile, and its host copy, which
// the exports unscale by (TileBackend::export_columns).  Solver holds two (cameras, landmarks), PoseGraphSolver one; whether the
// scaling is ON is TileBackend::scaled_.  Every copy is enqueued on the caller's stream: the caller synchronises, once for all its
// holders.  The host half of set_from_caller -- permute, validate -- is gather_scaling (column_map.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "ba_kernels.h"
#include "column_map.h"
#include "device_buffer.h"

namespace apex {

struct JacobiScaling {
    int64_t n = 0, n_pad = 0;      // entries; with the padding of the last tile (n where the segment has none)
    DeviceBuffer<double> dev;      // [n_pad]
    std::vector<double> host;      // [n_pad] once a scaling was set: what dev holds

    void set_size(int64_t n_, int64_t n_pad_) { n = n_; n_pad = n_pad_; }
    // the device vector, on first use; its padding is 1 from here on for the setters that write the n entries only
    hipError_t ensure() {
        if (dev) return hipSuccess;
        const hipError_t e = dev.alloc((size_t)n_pad);
        if (e != hipSuccess || n_pad == n) return e;
        const std::vector<double> ones((size_t)(n_pad - n), 1.0);
        return hipMemcpy(dev + n, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    // The caller's vector (global column order) onto host and device.  refused, and nothing changes: an entry is not positive and
    // finite (gather_scaling).  A solver with two holders asks both before it sets either, so a refusal leaves no half of it behind
    static constexpr const char* kRefused = "column scaling must be positive and finite";
    bool accepts(const ColumnMap& map, const double* scaling, std::vector<double>* staged) const { return gather_scaling(map, scaling, n_pad, staged); }
    hipError_t set_from_caller(std::vector<double>&& staged, hipStream_t s) { host = std::move(staged); return reupload(s); }
    // the host copy to the device: to restore a scaling whose device vector was borrowed (Solver::column_norms)
    hipError_t reupload(hipStream_t s) { return hipMemcpyAsync(dev, host.data(), (size_t)n_pad * sizeof(double), hipMemcpyHostToDevice, s); }
    // s = 1 / (1 + sqrt(n2)) of `count` squared column norms, then the host copy.  n2 may be dev itself; count is n_pad where n2
    // holds 0 on the padding (-> 1), n where dev's padding is 1 already
    hipError_t from_norms_sq(const double* n2, int64_t count, hipStream_t s) {
        launch_scaling_from_norms_sq(count, n2, dev, s);
        host.assign((size_t)n_pad, 1.0);
        return hipMemcpyAsync(host.data(), dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s);
    }
};

}  // namespace apex
