// tile_debug.cpp -- tests only: the single-GPU tile Cholesky (TilePlan) on a matrix the caller chooses
// (apexgpu_debug_tiles_*, include/apexgpu.h).  The calls do what Solver does around its plan -- clear, assemble, add the
// diagonal, factor, read the flags, sweep -- with the caller's tiles in place of an assembly; nothing is reordered.
// A null handle is APEXGPU_ERR_INVALID_INPUT here, as it always was; the body then runs through with_handle() (capi_guard.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "capi_handles.h"

namespace {
constexpr size_t kTile = (size_t)apex::kNB * apex::kNB;

int hip_rc(hipError_t e) { return e == hipSuccess ? APEXGPU_OK : APEXGPU_ERR_DEVICE; }
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
        std::unique_ptr<apexgpu_tiles, void (*)(apexgpu_tiles*)> h(new apexgpu_tiles(), apexgpu_debug_tiles_destroy);
        apex::TileSession& t = *(apex::HandleOwner::solver(h.get()) = new apex::TileSession());
        t.device = device;
        apex::TilePlan& tp = t.plan;
        tp.enable_graphs((opts[0] & 1) != 0);
        tp.set_diag_lower((opts[0] & 2) == 0);
        tp.set_factor_flow(opts[1], opts[2]);
        tp.enable_tri_flow(opts[3] != 0);
        tp.enable_overlap(opts[4] != 0);
        if (opts[4] > 1) tp.set_overlap_min(opts[4]);
        tp.set_split_u1(opts[5]);
        tp.set_two_side(opts[6]);
        tp.set_gate_min(opts[7]);
        hipError_t e = hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking);
        std::string err;
        if (e == hipSuccess) err = tp.build(nt, std::vector<uint8_t>(present, present + (size_t)nt * nt), t.stream);
        const size_t n = (size_t)tp.n_pad();
        if (e == hipSuccess && err.empty()) e = t.rhs.alloc(n);
        if (e == hipSuccess && err.empty()) e = t.x.alloc(n);
        if (e == hipSuccess && err.empty()) e = t.work.alloc(2 * n);
        if (e != hipSuccess || !err.empty()) return e != hipSuccess ? APEXGPU_ERR_DEVICE : APEXGPU_ERR_INVALID_STATE;   // (h goes through destroy)
        *out = h.release();
        return APEXGPU_OK;
    });
}

void apexgpu_debug_tiles_destroy(apexgpu_tiles* h) {
    if (!h) return;
    apex::TileSession* t = apex::HandleOwner::solver(h);
    hipStream_t s = nullptr;
    if (t) {
        (void)hipSetDevice(t->device);
        s = t->stream;
        if (s) (void)hipStreamSynchronize(s);   // in this order: the stream drained, then the plan and the buffers, then the stream
    }
    delete t;
    delete h;
    if (s) (void)hipStreamDestroy(s);
}

int apexgpu_debug_tiles_pattern(apexgpu_tiles* h, int32_t* slot_out, int64_t info[8]) {
    if (!h || !info) return APEXGPU_ERR_INVALID_INPUT;
    return with_handle(h, [&](auto& t) {
        const apex::TilePlan& tp = t.plan;
        if (slot_out) memcpy(slot_out, tp.slot_host(), (size_t)tp.nt() * tp.nt() * sizeof(int32_t));
        info[0] = tp.n_slots(); info[1] = tp.n_touched_slots(); info[2] = tp.n_levels(); info[3] = tp.first_writers_flagged();
        info[4] = tp.factor_flow_units(); info[5] = tp.factor_flow_groups(); info[6] = tp.n_pad(); info[7] = apex::kNB;
        return APEXGPU_OK;
    });
}

int apexgpu_debug_tiles_set(apexgpu_tiles* h, const double* touched, int n_valid, double add_diag, int fill_mode) {
    if (!h) return APEXGPU_ERR_INVALID_INPUT;
    return with_handle(h, [&](auto& t) -> int {
        if (!touched || n_valid < 0 || n_valid > t.plan.n_pad() || fill_mode < 0 || fill_mode > 1) return APEXGPU_ERR_INVALID_INPUT;
        apex::TilePlan& tp = t.plan;
        if (fill_mode == 1 && !tp.first_writers_flagged()) return APEXGPU_ERR_INVALID_STATE;
        if (hipSetDevice(t.device) != hipSuccess) return APEXGPU_ERR_DEVICE;
        // (as Solver::assemble: the fill tiles are left alone where the plan's first writers do not read them)
        hipError_t e = tp.zero_tiles(false, /*skip_fill=*/true);
        if (e == hipSuccess)
            e = hipMemcpyAsync(tp.tiles(), touched, (size_t)tp.n_touched_slots() * kTile * sizeof(double), hipMemcpyHostToDevice, t.stream);
        if (e != hipSuccess) return hip_rc(e);
        tp.add_diag(n_valid, add_diag, 1.0);
        std::vector<double> nan;
        if (fill_mode == 1 && tp.n_slots() > tp.n_touched_slots()) {
            nan.assign((size_t)(tp.n_slots() - tp.n_touched_slots()) * kTile, std::numeric_limits<double>::quiet_NaN());
            e = hipMemcpyAsync(tp.tiles() + (size_t)tp.n_touched_slots() * kTile, nan.data(), nan.size() * sizeof(double),
                               hipMemcpyHostToDevice, t.stream);
        }
        if (e == hipSuccess) e = hipGetLastError();
        const hipError_t se = hipStreamSynchronize(t.stream);
        return hip_rc(e != hipSuccess ? e : se);
    });
}

int apexgpu_debug_tiles_factor(apexgpu_tiles* h, int* failed_at) {
    if (!h || !failed_at) return APEXGPU_ERR_INVALID_INPUT;
    return with_handle(h, [&](auto& t) {
        if (hipSetDevice(t.device) != hipSuccess) return APEXGPU_ERR_DEVICE;
        apex::TilePlan& tp = t.plan;
        *failed_at = 0;
        const hipError_t e = tp.factor(failed_at);
        if (e != hipSuccess) return APEXGPU_ERR_DEVICE;
        if (tp.factor_flow_gave_up()) return APEXGPU_ERR_DEVICE;   // (the dataflow launch timed out: not a result)
        tp.set_factor_valid(*failed_at == 0);
        return APEXGPU_OK;
    });
}

int apexgpu_debug_tiles_solve(apexgpu_tiles* h, int n_rhs, const double* rhs, double* x) {
    if (!h || n_rhs < 0 || (n_rhs > 0 && (!rhs || !x))) return APEXGPU_ERR_INVALID_INPUT;
    return with_handle(h, [&](auto& t) {
        apex::TilePlan& tp = t.plan;
        if (!tp.factor_valid()) return APEXGPU_ERR_INVALID_STATE;
        if (hipSetDevice(t.device) != hipSuccess) return APEXGPU_ERR_DEVICE;
        const size_t n = (size_t)tp.n_pad();
        for (int k = 0; k < n_rhs; ++k) {
            hipError_t e = hipMemcpyAsync(t.rhs, rhs + k * n, n * sizeof(double), hipMemcpyHostToDevice, t.stream);
            if (e == hipSuccess) e = tp.solve(t.rhs, t.x, t.work);
            if (e == hipSuccess) e = hipMemcpyAsync(x + k * n, t.x, n * sizeof(double), hipMemcpyDeviceToHost, t.stream);
            const hipError_t se = hipStreamSynchronize(t.stream);
            if (e != hipSuccess || se != hipSuccess) return APEXGPU_ERR_DEVICE;
            if (tp.sweep_timed_out()) return APEXGPU_ERR_DEVICE;   // (a sweep that gave up leaves a wrong x)
        }
        return APEXGPU_OK;
    });
}

int apexgpu_debug_tiles_matvec(apexgpu_tiles* h, const double* x, double* y) {
    if (!h || !x || !y) return APEXGPU_ERR_INVALID_INPUT;
    return with_handle(h, [&](auto& t) {
        if (hipSetDevice(t.device) != hipSuccess) return APEXGPU_ERR_DEVICE;
        apex::TilePlan& tp = t.plan;
        const size_t n = (size_t)tp.n_pad();
        hipError_t e = hipMemcpyAsync(t.rhs, x, n * sizeof(double), hipMemcpyHostToDevice, t.stream);
        if (e == hipSuccess) {
            tp.sym_matvec(t.rhs, t.x);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(y, t.x, n * sizeof(double), hipMemcpyDeviceToHost, t.stream);
        const hipError_t se = hipStreamSynchronize(t.stream);
        return hip_rc(e != hipSuccess ? e : se);
    });
}

int apexgpu_debug_tiles_pcg(apexgpu_tiles* h, const double* rhs, int max_iter, double tol, double* x, int* iters, double scal_out[5]) {
    if (!h || !rhs || !x || !iters || !scal_out) return APEXGPU_ERR_INVALID_INPUT;
    return with_handle(h, [&](auto& t) {
        if (hipSetDevice(t.device) != hipSuccess) return APEXGPU_ERR_DEVICE;
        apex::TilePlan& tp = t.plan;
        const size_t n = (size_t)tp.n_pad();
        *iters = 0;
        if (!t.pcg_work && t.pcg_work.alloc(6 * n) != hipSuccess) return APEXGPU_ERR_DEVICE;
        hipError_t e = hipMemcpyAsync(t.rhs, rhs, n * sizeof(double), hipMemcpyHostToDevice, t.stream);
        // (as Solver::pcg_solve: the caller's limits go through unchanged; the plan's factor is void from here on)
        if (e == hipSuccess) e = tp.pcg(t.rhs, t.x, t.pcg_work, max_iter, tol, iters);
        if (e == hipSuccess) e = hipMemcpyAsync(x, t.x, n * sizeof(double), hipMemcpyDeviceToHost, t.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(scal_out, tp.pcg_scalars(), 5 * sizeof(double), hipMemcpyDeviceToHost, t.stream);
        const hipError_t se = hipStreamSynchronize(t.stream);
        return hip_rc(e != hipSuccess ? e : se);
    });
}

int apexgpu_debug_tiles_get(apexgpu_tiles* h, int which, double* out, int* recomputed_out) {
    if (!h || !out || which < 0 || which > 2) return APEXGPU_ERR_INVALID_INPUT;
    return with_handle(h, [&](auto& t) {
        if (recomputed_out) *recomputed_out = 0;
        if (hipSetDevice(t.device) != hipSuccess) return APEXGPU_ERR_DEVICE;
        apex::TilePlan& tp = t.plan;
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
        hipError_t e = hipMemcpyAsync(out, src, count * kTile * sizeof(double), hipMemcpyDeviceToHost, t.stream);
        const hipError_t se = hipStreamSynchronize(t.stream);
        return hip_rc(e != hipSuccess ? e : se);
    });
}

}  // extern "C"
