// tile_backend.hip -- see tile_backend.h
#include "tile_backend.h"

#include <stddef.h>

#include <vector>

namespace apex {

int TileBackend::check_hip(hipError_t e, const char* what, std::string* err) {
    if (e == hipSuccess) return kOk;
    *(err ? err : &err_) = std::string("HIP error in ") + what + ": " + hipGetErrorString(e);
    return kDeviceError;
}

// The dataflow launch of the top groups timed out (TilePlan::factor_flow_gave_up: the tiles are half updated and the plan has gone
// back to the level launches, in a distributed plan on every rank alike): the system is built again and factorised once more.
int TileBackend::factor_again(double lambda, double reg, int* failed) {
    ++n_factor_flow_timeouts_;
    int rc = rebuild_system(lambda, reg);
    if (rc == kOk) rc = factor_now(failed, false);
    if (rc == kOk && tp_.factor_flow_gave_up()) return fail(kDeviceError, "dataflow factorisation timed out twice");
    return rc;
}

int TileBackend::factor_fresh(double lambda, double reg, int* failed) {
    const int rc = factor_now(failed, false);
    return (rc != kOk || !tp_.factor_flow_gave_up()) ? rc : factor_again(lambda, reg, failed);
}

// ONE host wait per direct solve.  The factorisation, the sweeps and what finish_step() adds are enqueued back to back, and the
// pivot flag, the dataflow launch's time-out word and the solver's own flag are read at the final wait; what was enqueued behind
// a bad factorisation is then void, recover_factor() takes the waited-for path from the assembly on, and the sweeps run once more.
int TileBackend::direct_solve(bool speculative, double lambda, double* step_out, double* grad_out) {
    int failed = 0;
    int rc = speculative ? factor_now(&failed, /*defer_flags=*/true) : kOk;
    for (int attempt = 0; rc == kOk; ++attempt) {
        rc = enqueue_sweeps();
        if (rc == kOk) rc = finish_step(step_out, grad_out);   // (synchronises: the sweeps' error word is on the host now)
        if (rc != kOk) break;
        if (speculative) {   // the flags the waited-for path read before going on
            speculative = false;
            int own = 0;
            if (own_flag()) HIP_TRY(hipMemcpyAsync(&own, own_flag(), sizeof(int), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(tp_.read_flags(&failed));   // (synchronises; raises factor_flow_gave_up() on a dataflow time-out)
            if (own) { st_.invalidate_step(); return own_flag_raised(); }
            const bool gave_up = tp_.factor_flow_gave_up();
            if (failed || gave_up) {
                st_.invalidate_step();
                (void)tp_.sweep_timed_out();   // (clears the word a sweep over a broken factor may have raised)
                rc = recover_factor(lambda, failed, gave_up);
                attempt = -1;   // (the loop's counter is for the sweep time-outs of the solve that follows)
                continue;       // the sweeps and the step once more, over the good factor
            }
        }
        if (!tp_.sweep_timed_out()) { keep_factor(); return kOk; }
        // A dataflow sweep of THIS solve ran into its spin limit (chol_kernels.hip, flow_wait): the step is wrong.  The factor is
        // intact, so the solve is repeated with the level-by-level sweeps -- for this call and for the rest of the plan's
        // life (a device that starved a sweep once will do it again, and every time-out costs ~2 s).  In a distributed plan
        // the word was max-reduced: every rank is here.
        st_.invalidate_step();
        if (attempt > 0 || !tp_.tri_flow()) return fail(kDeviceError, "triangular sweep timed out");
        tp_.enable_tri_flow(false);
    }
    return rc;
}

// ---- exports in the caller's column order (column_map.h) ---------------------------------------------------------------------
int TileBackend::export_columns(std::initializer_list<ExportSegment> segs, ExportAs as, double* out) {
    std::vector<std::vector<double>> h;
    for (const ExportSegment& sg : segs) {
        h.emplace_back((size_t)sg.map->size());
        HIP_TRY(hipMemcpyAsync(h.back().data(), sg.dev, h.back().size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
    }
    HIP_TRY(hipStreamSynchronize(stream_));
    size_t k = 0;
    for (const ExportSegment& sg : segs) {
        const double* v = h[k++].data();
        const double* s = (scaled_ && as != ExportAs::kPlain) ? sg.scale->host.data() : nullptr;
        if (!s) sg.map->scatter(v, out, 0.0);
        else if (as == ExportAs::kStep) sg.map->scatter(v, out, 0.0, [s](double x, int64_t i) { return x / s[i]; });
        else sg.map->scatter(v, out, 0.0, [s](double x, int64_t i) { return x * s[i]; });
    }
    return kOk;
}

int TileBackend::export_tiles_dense(const ColumnMap& map, int64_t ld, int64_t slot_bound, double* out) {
    const size_t tile_elems = (size_t)kNB * kNB;
    const int64_t n = map.size();
    std::vector<double> t(tile_elems);
    for (int I = 0; I < tp_.nt(); ++I)
        for (int J = 0; J <= I; ++J) {
            const int s = tp_.slot(I, J);
            if (s < 0 || s >= slot_bound) continue;
            HIP_TRY(hipMemcpyAsync(t.data(), tp_.tiles() + (size_t)s * tile_elems, tile_elems * sizeof(double), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(hipStreamSynchronize(stream_));
            for (int r = 0; r < kNB; ++r)
                for (int c = 0; c < kNB; ++c) {
                    const int64_t gi = (int64_t)I * kNB + r, gj = (int64_t)J * kNB + c;
                    if (gi >= n || gj >= n || gj > gi) continue;
                    const double val = t[(size_t)r * kNB + c];
                    out[map.col[gi] * ld + map.col[gj]] = val;
                    out[map.col[gj] * ld + map.col[gi]] = val;
                }
        }
    return kOk;
}

// ---- the trial-step protocol (lm_loop.h) ---------------------------------------------------------------------------------
int TileBackend::enqueue_eager_eval() {
    if (!eager_host_) HIP_TRY(eager_host_.alloc(8));
    int n = 0;
    double* sums = step_sums(&n);
    int rc = enqueue_step_stats();
    if (rc == kOk) rc = enqueue_trial_point(sums + n);
    if (rc != kOk) return rc;
    HIP_TRY(hipMemcpyAsync(eager_host_, sums, (n + 1) * sizeof(double), hipMemcpyDeviceToHost, stream_));
    return kOk;
}

// The answers of the last solve: posted at its wait, else the statistics -- or the trial point and its sum of squares -- are
// enqueued and read back with one wait.
int TileBackend::answers_of_step(bool trial, StepAnswers* out) {
    const StepAnswers* posted = nullptr;
    if (const Status rc = trial ? st_.ask_trial(&posted) : st_.ask_stats(&posted)) return fail(rc, st_.refusal);
    if (posted) { *out = *posted; return kOk; }
    HIP_TRY(hipSetDevice(device_));
    int n = 0;
    double* sums = step_sums(&n);
    if (trial) st_.trial_written();
    const int rc = trial ? enqueue_trial_point(sums + n) : enqueue_step_stats();
    if (rc != kOk) return rc;
    HIP_TRY(hipGetLastError());
    double h[8] = {};
    HIP_TRY(hipMemcpyAsync(h + (trial ? n : 0), sums + (trial ? n : 0), (trial ? 1 : n) * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    *out = answers_from_sums(h);
    return kOk;
}
int TileBackend::step_stats(double out3[3]) {
    StepAnswers a;
    const int rc = answers_of_step(false, &a);
    if (rc == kOk) { out3[0] = a.gradient_norm; out3[1] = a.step_norm; out3[2] = a.predicted_reduction; }
    return rc;
}
int TileBackend::eval_step(double* trial_cost) {
    StepAnswers a;
    const int rc = answers_of_step(true, &a);
    if (rc == kOk) *trial_cost = cost_from_sumsq(a.trial_sumsq);
    return rc;
}
int TileBackend::commit_step() {
    if (const Status rc = st_.commit()) return fail(rc, st_.refusal);
    params_moved();
    return kOk;
}
// apply_negative_parameter_step (optimizer/mod.rs:343-356): the rejected trial point is moved back by the inverse retraction,
// it is NOT restored from a snapshot.  The one exception is a backend that answers keeps_current_on_discard(): the trial point
// lives in the other parameter set (enqueue_trial_point writes st_.cur ^ 1 only), so the current set still holds x with its bits
// and nothing is enqueued -- an SO3 pose graph (pg_solver.h).
int TileBackend::discard_step() {
    if (const Status rc = st_.begin_discard()) return fail(rc, st_.refusal);
    HIP_TRY(hipSetDevice(device_));
    if (!keeps_current_on_discard()) {
        const int rc = enqueue_retract(st_.cur ^ 1, -1.0, st_.cur);
        if (rc != kOk) return rc;
    }
    HIP_TRY(hipStreamSynchronize(stream_));
    (void)st_.finish_discard();
    params_moved();
    return kOk;
}

// ---- the Dog-Leg step (tr_loop.h; DESIGN.md §5, "The Dog-Leg step, held once") ------------------------------------------------
// Everything is in the SCALED variables when Jacobi scaling is on: g_s = D g, y = D^-1 d with d the unscaled step the solve left;
// g_s.H_s g_s = |J D g_s|^2, g_s.H_s y = (J D g_s).(J d), y.H_s y = |J d|^2 -- the Gram pass is handed D^2 g and d and never sees D.
int TileBackend::enqueue_dogleg_tail(bool fresh) {
    constexpr size_t kSums = offsetof(DoglegScalars, sums) / sizeof(double), kCombined = offsetof(DoglegScalars, alpha) / sizeof(double),
                     kCoef = offsetof(DoglegScalars, c_g) / sizeof(double), kStep = offsetof(DoglegScalars, step_sumsq) / sizeof(double),
                     kTrial = offsetof(DoglegScalars, trial_sumsq) / sizeof(double);
    static_assert(offsetof(DoglegScalars, c_h) == offsetof(DoglegScalars, c_g) + sizeof(double), "k_dl_blend reads {c_g, c_h}");
    double* const s = reinterpret_cast<double*>(dls_.get());
    DlSegment segs[2];
    const int n_seg = dogleg_segments(segs);
    const double *a[2] = {}, *b[2] = {};   // what the Gram pass prices: D^2 g (g itself without scaling) and the step
    for (int k = 0; k < n_seg; ++k) {
        segs[k].a = scaled_ ? dl_a_[k].get() : nullptr; segs[k].h = dl_h_[k];
        a[k] = scaled_ ? segs[k].a : segs[k].g; b[k] = segs[k].d;
    }
    timer_.begin(stats_stage_, stream_);
    if (fresh) {
        launch_dl_dots(segs, n_seg, partial_, n_partial_, s + kSums, stream_);
        enqueue_jv_gram(a, b, s + kSums + 3);
    }
    launch_dl_combine(s + kSums, dl_radius_, s + kCombined, stream_);
    launch_dl_blend(segs, n_seg, s + kCoef, partial_, n_partial_, s + kStep, stream_);
    timer_.end(stats_stage_, stream_);
    dogleg_trial_begins();
    const int rc = enqueue_trial_point(s + kTrial);
    if (rc != kOk) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dl_host_, dls_, sizeof(DoglegScalars), hipMemcpyDeviceToHost, stream_));
    return kOk;
}

int TileBackend::dogleg_step(double mu, double radius, int reuse, DoglegStepInfo* out) {
    { const int rc = dogleg_refusal(); if (rc != kOk) return rc; }
    if (!(radius > 0.0) || !(mu >= 0.0)) return fail(kInvalidInput, "dogleg_step: the radius must be positive and mu non-negative");
    if (reuse && !have_dl_cache_) return fail(kInvalidState, "no cached Dog-Leg solve to reuse");
    HIP_TRY(hipSetDevice(device_));
    DlSegment segs[2];
    const int n_seg = dogleg_segments(segs);
    if (n_partial_ < n_seg) return fail(kInvalidState, "Dog-Leg: the reductions need a partial slot per segment");
    if (!dls_) {
        for (int k = 0; k < n_seg; ++k) { HIP_TRY(dl_h_[k].alloc_zero(segs[k].n_alloc)); HIP_TRY(dl_a_[k].alloc_zero(segs[k].n_alloc)); }
        HIP_TRY(dls_.alloc_zero(1));
        HIP_TRY(hipDeviceSynchronize());   // (null-stream memsets ahead of the work on stream_)
    }
    if (!dl_host_) HIP_TRY(dl_host_.alloc(1));
    dl_radius_ = radius;
    int rc;
    if (reuse) {
        begin_solve(last_lambda_);
        rc = enqueue_dogleg_tail(false);
        if (rc == kOk) rc = check_hip(hipStreamSynchronize(stream_), "dogleg_step");
        if (rc == kOk) st_.step_computed();
    } else {
        // (cleared on every way out, an exception caught at the C boundary included: a flag left on would take the ladder, the
        // export and the eager evaluation away from every later solve_augmented)
        struct ModeGuard { bool& on; explicit ModeGuard(bool& f) : on(f) { on = true; } ~ModeGuard() { on = false; } };
        { ModeGuard in_dogleg(dl_mode_); rc = solve_for_dogleg(mu); }
        if (rc == kOk) have_dl_cache_ = true;
    }
    if (rc != kOk) return rc;
    st_.post_answers(dogleg_answers(*dl_host_));   // (the trial point is in place)
    if (out) *out = dogleg_step_info(*dl_host_, reuse != 0);
    return kOk;
}

int TileBackend::jv_gram_columns(const double* a, const double* b, double out3[3]) {
    HIP_TRY(hipSetDevice(device_));
    DlSegment segs[2];
    const int n_seg = dogleg_segments(segs);
    DeviceBuffer<double> da[2], db[2];
    HIP_TRY(hipStreamSynchronize(stream_));
    for (int k = 0; k < n_seg; ++k) {
        std::vector<double> ha((size_t)segs[k].n_alloc, 0.0), hb((size_t)segs[k].n_alloc, 0.0);
        segs[k].map->gather(a, ha.data());
        segs[k].map->gather(b, hb.data());
        HIP_TRY(da[k].upload(ha));
        HIP_TRY(db[k].upload(hb));
    }
    if (!jv_out_) HIP_TRY(jv_out_.alloc(3));
    const double* const pa[2] = {da[0], da[1]};
    const double* const pb[2] = {db[0], db[1]};
    timer_.begin(stats_stage_, stream_);   // (with stage timing on, this call's time under the stage is the Gram pass alone)
    enqueue_jv_gram(pa, pb, jv_out_);
    timer_.end(stats_stage_, stream_);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out3, jv_out_, 3 * sizeof(double), hipMemcpyDeviceToHost, stream_);
    (void)hipStreamSynchronize(stream_);   // (before the staging buffers are freed)
    return check_hip(e, "jv_gram");
}

}  // namespace apex
