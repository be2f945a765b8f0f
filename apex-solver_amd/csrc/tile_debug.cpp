// tile_debug.cpp -- tests only: the single-GPU tile Cholesky (TilePlan) on a matrix the caller chooses
// (apexgpu_debug_tiles_*, include/apexgpu.h).  The calls do what Solver does around its plan -- clear, assemble, add the
// diagonal, factor, read the flags, sweep -- with the caller's tiles in place of an assembly; nothing is reordered.
#include <hip/hip_runtime.h>
#include <string.h>

#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/apexgpu.h"
#include "tile_plan.h"

struct apexgpu_tiles {
    int device = 0;
    hipStream_t stream = nullptr;
    apex::DeviceBuffer<double> rhs, x, work;   // kept for the handle's life: the captured sweeps hold their addresses
    apex::DeviceBuffer<double> pcg_work;       // 6 * n_pad doubles, allocated by the first pcg call
    apex::TilePlan plan;                       // (declared last: its graph execs go before the buffers they point into)
};

namespace {
constexpr size_t kTile = (size_t)apex::kNB * apex::kNB;

int hip_rc(hipError_t e) { return e == hipSuccess ? APEXGPU_OK : APEXGPU_ERR_DEVICE; }

template <typename F>
int guarded(F&& f) noexcept {
    try {
        return f();
    } catch (...) {
        return APEXGPU_ERR_INVALID_INPUT;
    }
}
}  // namespace

extern "C" {

int apexgpu_debug_tiles_create(int device, int nt, const uint8_t* present, const int opts[8], apexgpu_tiles** out) {
    if (!out) return APEXGPU_ERR_INVALID_INPUT;
    *out = nullptr;
    if (nt <= 0 || !present || !opts) return APEXGPU_ERR_INVALID_INPUT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return APEXGPU_ERR_DEVICE;
    return guarded([&]() -> int {
        for (int I = 0; I < nt; ++I) {   // the diagonal is always there; nothing above it
            if (!present[(size_t)I * nt + I]) return APEXGPU_ERR_INVALID_INPUT;
            for (int J = I + 1; J < nt; ++J)
                if (present[(size_t)I * nt + J]) return APEXGPU_ERR_INVALID_INPUT;
        }
        if (hipSetDevice(device) != hipSuccess) return APEXGPU_ERR_DEVICE;
        apexgpu_tiles* h = new apexgpu_tiles();
        h->device = device;
        apex::TilePlan& tp = h->plan;
        tp.enable_graphs(opts[0] != 0);
        tp.set_factor_flow(opts[1], opts[2]);
        tp.enable_tri_flow(opts[3] != 0);
        tp.enable_overlap(opts[4] != 0);
        if (opts[4] > 1) tp.set_overlap_min(opts[4]);
        tp.set_split_u1(opts[5]);
        tp.set_two_side(opts[6]);
        tp.set_gate_min(opts[7]);
        hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        std::string err;
        if (e == hipSuccess) err = tp.build(nt, std::vector<uint8_t>(present, present + (size_t)nt * nt), h->stream);
        const size_t n = (size_t)tp.n_pad();
        if (e == hipSuccess && err.empty()) e = h->rhs.alloc(n);
        if (e == hipSuccess && err.empty()) e = h->x.alloc(n);
        if (e == hipSuccess && err.empty()) e = h->work.alloc(2 * n);
        if (e != hipSuccess || !err.empty()) {
            apexgpu_debug_tiles_destroy(h);
            return e != hipSuccess ? APEXGPU_ERR_DEVICE : APEXGPU_ERR_INVALID_STATE;
        }
        *out = h;
        return APEXGPU_OK;
    });
}

void apexgpu_debug_tiles_destroy(apexgpu_tiles* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    hipStream_t s = h->stream;
    if (s) (void)hipStreamSynchronize(s);   // in this order: the stream drained, then the plan and the buffers, then the stream
    delete h;
    if (s) (void)hipStreamDestroy(s);
}

int apexgpu_debug_tiles_pattern(apexgpu_tiles* h, int32_t* slot_out, int64_t info[8]) {
    if (!h || !info) return APEXGPU_ERR_INVALID_INPUT;
    const apex::TilePlan& tp = h->plan;
    if (slot_out) memcpy(slot_out, tp.slot_host(), (size_t)tp.nt() * tp.nt() * sizeof(int32_t));
    info[0] = tp.n_slots(); info[1] = tp.n_touched_slots(); info[2] = tp.n_levels(); info[3] = tp.first_writers_flagged();
    info[4] = tp.factor_flow_units(); info[5] = tp.factor_flow_groups(); info[6] = tp.n_pad(); info[7] = apex::kNB;
    return APEXGPU_OK;
}

int apexgpu_debug_tiles_set(apexgpu_tiles* h, const double* touched, int n_valid, double add_diag, int fill_mode) {
    if (!h || !touched || n_valid < 0 || n_valid > h->plan.n_pad() || fill_mode < 0 || fill_mode > 1) return APEXGPU_ERR_INVALID_INPUT;
    apex::TilePlan& tp = h->plan;
    if (fill_mode == 1 && !tp.first_writers_flagged()) return APEXGPU_ERR_INVALID_STATE;
    return guarded([&]() -> int {
        if (hipSetDevice(h->device) != hipSuccess) return APEXGPU_ERR_DEVICE;
        // (as Solver::assemble: the fill tiles are left alone where the plan's first writers do not read them)
        hipError_t e = tp.zero_tiles(false, /*skip_fill=*/true);
        if (e == hipSuccess)
            e = hipMemcpyAsync(tp.tiles(), touched, (size_t)tp.n_touched_slots() * kTile * sizeof(double), hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) return hip_rc(e);
        tp.add_diag(n_valid, add_diag, 1.0);
        std::vector<double> nan;
        if (fill_mode == 1 && tp.n_slots() > tp.n_touched_slots()) {
            nan.assign((size_t)(tp.n_slots() - tp.n_touched_slots()) * kTile, std::numeric_limits<double>::quiet_NaN());
            e = hipMemcpyAsync(tp.tiles() + (size_t)tp.n_touched_slots() * kTile, nan.data(), nan.size() * sizeof(double),
                               hipMemcpyHostToDevice, h->stream);
        }
        if (e == hipSuccess) e = hipGetLastError();
        const hipError_t se = hipStreamSynchronize(h->stream);
        return hip_rc(e != hipSuccess ? e : se);
    });
}

int apexgpu_debug_tiles_factor(apexgpu_tiles* h, int* failed_at) {
    if (!h || !failed_at) return APEXGPU_ERR_INVALID_INPUT;
    if (hipSetDevice(h->device) != hipSuccess) return APEXGPU_ERR_DEVICE;
    apex::TilePlan& tp = h->plan;
    *failed_at = 0;
    const hipError_t e = tp.factor(failed_at);
    if (e != hipSuccess) return APEXGPU_ERR_DEVICE;
    if (tp.factor_flow_gave_up()) return APEXGPU_ERR_DEVICE;   // (the dataflow launch timed out: not a result)
    tp.set_factor_valid(*failed_at == 0);
    return APEXGPU_OK;
}

int apexgpu_debug_tiles_solve(apexgpu_tiles* h, int n_rhs, const double* rhs, double* x) {
    if (!h || n_rhs < 0 || (n_rhs > 0 && (!rhs || !x))) return APEXGPU_ERR_INVALID_INPUT;
    apex::TilePlan& tp = h->plan;
    if (!tp.factor_valid()) return APEXGPU_ERR_INVALID_STATE;
    if (hipSetDevice(h->device) != hipSuccess) return APEXGPU_ERR_DEVICE;
    const size_t n = (size_t)tp.n_pad();
    for (int k = 0; k < n_rhs; ++k) {
        hipError_t e = hipMemcpyAsync(h->rhs, rhs + k * n, n * sizeof(double), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = tp.solve(h->rhs, h->x, h->work);
        if (e == hipSuccess) e = hipMemcpyAsync(x + k * n, h->x, n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        const hipError_t se = hipStreamSynchronize(h->stream);
        if (e != hipSuccess || se != hipSuccess) return APEXGPU_ERR_DEVICE;
        if (tp.sweep_timed_out()) return APEXGPU_ERR_DEVICE;   // (a sweep that gave up leaves a wrong x)
    }
    return APEXGPU_OK;
}

int apexgpu_debug_tiles_matvec(apexgpu_tiles* h, const double* x, double* y) {
    if (!h || !x || !y) return APEXGPU_ERR_INVALID_INPUT;
    if (hipSetDevice(h->device) != hipSuccess) return APEXGPU_ERR_DEVICE;
    apex::TilePlan& tp = h->plan;
    const size_t n = (size_t)tp.n_pad();
    hipError_t e = hipMemcpyAsync(h->rhs, x, n * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        tp.sym_matvec(h->rhs, h->x);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(y, h->x, n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t se = hipStreamSynchronize(h->stream);
    return hip_rc(e != hipSuccess ? e : se);
}

int apexgpu_debug_tiles_pcg(apexgpu_tiles* h, const double* rhs, int max_iter, double tol, double* x, int* iters, double scal_out[5]) {
    if (!h || !rhs || !x || !iters || !scal_out) return APEXGPU_ERR_INVALID_INPUT;
    if (hipSetDevice(h->device) != hipSuccess) return APEXGPU_ERR_DEVICE;
    apex::TilePlan& tp = h->plan;
    const size_t n = (size_t)tp.n_pad();
    *iters = 0;
    if (!h->pcg_work && h->pcg_work.alloc(6 * n) != hipSuccess) return APEXGPU_ERR_DEVICE;
    hipError_t e = hipMemcpyAsync(h->rhs, rhs, n * sizeof(double), hipMemcpyHostToDevice, h->stream);
    // (as Solver::pcg_solve: the caller's limits go through unchanged; the plan's factor is void from here on)
    if (e == hipSuccess) e = tp.pcg(h->rhs, h->x, h->pcg_work, max_iter, tol, iters);
    if (e == hipSuccess) e = hipMemcpyAsync(x, h->x, n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(scal_out, tp.pcg_scalars(), 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t se = hipStreamSynchronize(h->stream);
    return hip_rc(e != hipSuccess ? e : se);
}

int apexgpu_debug_tiles_get(apexgpu_tiles* h, int which, double* out, int* recomputed_out) {
    if (!h || !out || which < 0 || which > 2) return APEXGPU_ERR_INVALID_INPUT;
    if (recomputed_out) *recomputed_out = 0;
    if (hipSetDevice(h->device) != hipSuccess) return APEXGPU_ERR_DEVICE;
    apex::TilePlan& tp = h->plan;
    const double* src = tp.tiles();
    size_t count = (size_t)tp.n_slots();
    if (which == 1) { src = tp.linv(); count = (size_t)tp.nt(); }
    if (which == 2) {
        bool recomputed = false;
        std::string err;
        apex::SelectedInverse& inv = tp.inverse();
        const int rc = inv.ensure(&recomputed, &err);
        if (rc == 1) return APEXGPU_ERR_INVALID_STATE;
        if (rc != 0) return APEXGPU_ERR_DEVICE;
        src = inv.map().tiles;
        if (recomputed_out) *recomputed_out = recomputed ? 1 : 0;
    }
    hipError_t e = hipMemcpyAsync(out, src, count * kTile * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t se = hipStreamSynchronize(h->stream);
    return hip_rc(e != hipSuccess ? e : se);
}

}  // extern "C"
