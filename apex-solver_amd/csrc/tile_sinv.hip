// tile_sinv.hip -- see tile_sinv.h
#include "tile_sinv.h"

#include <algorithm>

#include "sinv_lists.h"

namespace apex {

void SelectedInverse::release() {
    z_.reset(); y_.reset(); tasks_.reset(); prods_.reset();   // (null z_: enqueue sets up again)
    groups_.clear(); group_ms_.clear();
    n_[0] = n_[1] = n_[2] = 0;
    bytes_ = 0;
    z_epoch_ = 0;
}

// The lists of the recurrence from the slot map and the level groups of the factorisation (nothing of the step path changes),
// then the memory they need, then their tile names resolved to addresses in L, Linv, Z and the group's Y tiles.
std::string SelectedInverse::setup() {
    SinvLists lists;
    const std::string refusal = build_sinv_lists(v_.nt, v_.slot_host, *v_.group_cols, &lists);
    if (!refusal.empty()) return refusal;
    const size_t te = (size_t)kNB * kNB;
    const size_t n_y = (size_t)std::max<int64_t>(lists.y_max, 1);
    const size_t need = ((size_t)v_.n_slots + n_y) * te * sizeof(double);
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    if ((double)need > 0.9 * (double)free_b)
        return "the covariance tiles need " + std::to_string(need / 1e9) + " GB; only " + std::to_string(free_b / 1e9) + " GB free";
    hipError_t e = z_.alloc((size_t)v_.n_slots * te);
    if (e == hipSuccess) e = y_.alloc(n_y * te);
    if (e != hipSuccess) { release(); return std::string("HIP error allocating the covariance tiles: ") + hipGetErrorString(e); }
    const double* const base[4] = {v_.tiles, v_.linv, z_, y_};   // by SinvArray
    auto at = [&](const SinvRef& r) { return const_cast<double*>(base[r.array]) + (size_t)r.tile * te; };
    std::vector<SinvTask> tasks;
    std::vector<SinvProd> prods;
    tasks.reserve(lists.tasks.size()); prods.reserve(lists.prods.size());
    for (const SinvTaskH& t : lists.tasks) tasks.push_back({at(t.C), t.first, t.count});
    for (const SinvProdH& p : lists.prods) prods.push_back({at(p.A), at(p.B), p.op, 0});
    e = tasks_.upload(tasks);
    if (e == hipSuccess) e = prods_.upload(prods);
    if (e != hipSuccess) { release(); return std::string("HIP error uploading the covariance lists: ") + hipGetErrorString(e); }
    groups_ = std::move(lists.groups);
    for (int k = 0; k < 3; ++k) n_[k] = lists.n[k];
    bytes_ = need + tasks.size() * sizeof(SinvTask) + prods.size() * sizeof(SinvProd);
    return "";
}

int SelectedInverse::check(std::string* err) const {
    if (v_.distributed) { *err = "covariances of a distributed plan are not supported (single rank only)"; return 1; }
    if (!v_.factor_valid || !v_.tiles) {
        *err = "the tiles hold no valid factor: covariances need a successful direct (Cholesky) solve, and nothing may re-assemble the tiles in between";
        return 1;
    }
    return 0;
}

int SelectedInverse::enqueue(std::vector<hipEvent_t>* ev, std::string* err) {
    if (!z_) {
        const std::string e = setup();
        if (!e.empty()) { *err = e; return 2; }
    }
    if (timing_) {
        ev->assign(groups_.size() + 1, nullptr);
        for (hipEvent_t& x : *ev) {
            const hipError_t e = hipEventCreate(&x);
            if (e != hipSuccess) { collect(*ev, false); *err = std::string("HIP error in hipEventCreate: ") + hipGetErrorString(e); return 2; }
        }
        (void)hipEventRecord((*ev)[0], v_.stream);
    }
    for (size_t gi = 0; gi < groups_.size(); ++gi) {
        const std::array<int, 4>& g = groups_[gi];
        for (int k = 0; k < 3; ++k) launch_sinv_gemm(tasks_ + g[k], g[k + 1] - g[k], prods_, v_.stream);
        if (timing_) (void)hipEventRecord((*ev)[gi + 1], v_.stream);
    }
    return 0;
}

void SelectedInverse::collect(std::vector<hipEvent_t>& ev, bool ok) {
    if (ev.empty()) return;
    group_ms_.assign(ev.size() - 1, 0.0);
    for (size_t gi = 0; gi + 1 < ev.size(); ++gi) {
        float ms = 0.0f;
        if (ok && ev[gi] && ev[gi + 1] && hipEventElapsedTime(&ms, ev[gi], ev[gi + 1]) == hipSuccess) group_ms_[gi] = ms;
    }
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
    ev.clear();
}

int SelectedInverse::blocks(const int64_t* pos, int64_t n_var, int d, double* out, std::string* err) {
    if (const int rc = check(err)) return rc;
    const int64_t n_pad = (int64_t)v_.nt * kNB;
    for (int64_t v = 0; v < n_var; ++v)
        if (pos[v] < 0 || pos[v] + d > n_pad || pos[v] / kNB != (pos[v] + d - 1) / kNB) { *err = "variable block outside one diagonal tile"; return 1; }
    std::vector<hipEvent_t> ev;
    if (const int rc = enqueue(&ev, err)) return rc;
    DeviceBuffer<int64_t> dpos;
    DeviceBuffer<double> dout;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = dpos.alloc((size_t)std::max<int64_t>(n_var, 0));
    if (e == hipSuccess) e = dout.alloc((size_t)std::max<int64_t>(n_var * d * d, 0));
    if (e == hipSuccess && n_var > 0) e = hipMemcpyAsync(dpos, pos, (size_t)n_var * sizeof(int64_t), hipMemcpyHostToDevice, v_.stream);
    if (e == hipSuccess) {
        launch_sinv_diag_blocks(z_, v_.diag_slot, dpos, n_var, d, dout, v_.stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n_var > 0) e = hipMemcpyAsync(out, dout, (size_t)n_var * d * d * sizeof(double), hipMemcpyDeviceToHost, v_.stream);
    const hipError_t se = hipStreamSynchronize(v_.stream);
    if (e == hipSuccess) e = se;
    collect(ev, e == hipSuccess);
    if (e != hipSuccess) { *err = std::string("HIP error in covariance_blocks: ") + hipGetErrorString(e); return 2; }
    z_epoch_ = v_.factor_epoch;
    return 0;
}

int SelectedInverse::ensure(bool* recomputed, std::string* err) {
    *recomputed = false;
    if (const int rc = check(err)) return rc;
    if (current()) return 0;
    std::vector<hipEvent_t> ev;
    if (const int rc = enqueue(&ev, err)) return rc;
    hipError_t e = hipGetLastError();
    const hipError_t se = hipStreamSynchronize(v_.stream);
    if (e == hipSuccess) e = se;
    collect(ev, e == hipSuccess);
    if (e != hipSuccess) { *err = std::string("HIP error in ensure_inverse: ") + hipGetErrorString(e); return 2; }
    z_epoch_ = v_.factor_epoch;
    *recomputed = true;
    return 0;
}

}  // namespace apex
