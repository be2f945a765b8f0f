// pg_solver.hip -- see pg_solver.h
#include "pg_solver.h"

#include <math.h>
#include <string.h>

#include <algorithm>

#include "info_pack.h"
#include "pg2_device.hpp"
#include "pg2_lists.h"
#include "pg_device.hpp"
#include "pg_so3_device.hpp"
#include "prior_lists.h"

namespace apex {

namespace {
// the sizes of a manifold trait as values: {dof, amb, stride, prior stride}
struct ManifoldSizes { int dof, amb, stride, prior_stride; };
template <class M>
constexpr ManifoldSizes sizes_of() { return {M::kDof, M::kAmb, M::kStride, M::kPriorStride}; }
ManifoldSizes manifold_sizes(int manifold) {
    if (manifold == kManifoldSE2) return sizes_of<Se2Manifold>();
    if (manifold == kManifoldSO3) return sizes_of<So3Manifold>();
    return sizes_of<Se3Manifold>();
}
int known_manifold(int manifold) { return manifold == kManifoldSE2 || manifold == kManifoldSO3 ? manifold : kManifoldSE3; }
}  // namespace

PoseGraphSolver::PoseGraphSolver(int64_t n_v, int64_t n_e, int device, int manifold)
    : TileBackend(device, kPgNumStages, /*nd_leaf=*/2, kPgStats, /*n_partial=*/256), n_v_(n_v), n_e_(n_e), manifold_(known_manifold(manifold)),
      dof_(manifold_sizes(manifold_).dof), amb_(manifold_sizes(manifold_).amb), stride_(manifold_sizes(manifold_).stride),
      prior_stride_(manifold_sizes(manifold_).prior_stride), vpt_(kNB / dof_), row_owned_(pg_row_owned(manifold_)) {}

PoseGraphSolver::~PoseGraphSolver() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);   // before any buffer is freed; stream_last_ destroys the stream after them
}

// (the members of a row-owned handle are empty buffers, so null, on an SE3 graph assembled with atomics)
PGView PoseGraphSolver::view(int which) const {
    PGView v;
    v.n_v = n_v_; v.n_e = n_e_;
    v.posep = posep_[which]; v.e_from = e_from_; v.e_to = e_to_; v.meas = meas_;
    // set_loss: no loss, L2 and Huber are what the huber_delta kernels compute, so they run there (the same bits as a delta given
    // to set_structure); every other kind selects the general-loss instantiations through v.loss.kind
    v.huber_delta = huber_delta_;
    if (loss_set_) {
        const bool legacy = loss_.kind == kLossNone || loss_.kind == kLossL2 || loss_.kind == kLossHuber;
        v.huber_delta = loss_.kind == kLossHuber ? loss_.p0 : -1.0;
        if (!legacy) v.loss = loss_;
    }
    // information matrices: the weighted instantiations take every loss as a PgLoss, no loss, L2 and Huber included
    if (info_) {
        v.info = info_;
        if (loss_set_) v.loss = loss_;
        else if (huber_delta_ > 0.0) (void)pg_loss_make(kLossHuber, huber_delta_, 0.0, &v.loss);
    }
    v.n_prior = n_prior_; v.prior_v = prior_v_; v.prior_data = prior_data_;
    if (row_owned_) {
        v.poses = poses_[which]; v.inc_ptr = inc_ptr_; v.inc_edge = inc_edge_; v.prior_slot = prior_slot_;
    }
    return v;
}

int PoseGraphSolver::enqueue_retract(int from, double sign, int to) {
    timer_.begin(kPgRetract, stream_);
    launch_pg_retract(manifold_, n_v_, poses_[from], d_, sign, fix_, poses_[to], stream_);
    launch_pg_prepare(manifold_, n_v_, poses_[to], posep_[to], stream_);
    timer_.end(kPgRetract, stream_);
    return kOk;
}

// What a change voids ("What a change voids"): on a pose graph every setter drops the pending step and the Dog-Leg
// cache, nothing else.  The factor stays valid through all of them: covariance() is by contract of the matrix the LAST solve
// factorised, whatever was set since (pg_solver.h); the next assembly writes the tiles and voids it there.
void PoseGraphSolver::voided_by(Change why) {
    switch (why) {
        case Change::kStructure:     // (the vectors and the tiles are new)
        case Change::kParams:        // (the current set is overwritten under the step)
        case Change::kLoss:          // (the step and the cached gradient are of the system under the old loss,
        case Change::kPriors:        //  ... without these rows,
        case Change::kInformation:   //  ... under the old whitening)
            st_.invalidate();        // the trial point too: its cost was taken under the old factors
            drop_dogleg_cache();
            break;
        case Change::kScalingOff:
        case Change::kScalingVectors:   // the step is of the system under the old scaling; a trial point already written stays committable
            st_.invalidate_step();
            drop_dogleg_cache();       // (the cache holds for the scaling it was taken under)
            break;
    }
}

// PriorFactor blocks (prior_factor.rs:96-108); replaces the set.  data7 in to_vector order [t, w, i, j, k].
int PoseGraphSolver::set_priors(int64_t n, const uint32_t* vertex, const double* data7, const double* huber_delta) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    if (!prior_count_in_range(n)) return fail(kInvalidInput, "prior count out of range");
    { const std::string why = pg_prior_refusal(n, vertex, n_v_); if (!why.empty()) return fail(kInvalidInput, why); }
    // Row-owned handles: the blocks go to the device sorted by vertex (stable), so that one lane sums the run of a vertex in a
    // fixed order (k_pg2_priors); prior_slot_ keeps the caller's index for the export.  SE3 with atomics: the caller's order, as ever.
    const PriorLists pl = build_prior_lists(n, vertex, vmap_, {amb_, prior_stride_, false}, data7, huber_delta, nullptr, row_owned_, 0);
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipStreamSynchronize(stream_));
    voided_by(Change::kPriors);   // (ahead of the uploads: a call whose upload fails has voided the step all the same)
    // The new set goes up into locals and replaces the members (and n_prior_) only when every upload has succeeded: a failed
    // call leaves the old priors fully in place, a call with n = 0 none at all.
    DeviceBuffer<uint32_t> new_v;
    DeviceBuffer<double> new_data;
    DeviceBuffer<int> new_slot;
    if (n > 0) {
        if (row_owned_) HIP_TRY(new_slot.upload(pl.slot));
        HIP_TRY(new_v.upload(pl.owner));
        HIP_TRY(new_data.upload(pl.data));
    }
    prior_v_ = std::move(new_v); prior_data_ = std::move(new_data); prior_slot_ = std::move(new_slot);
    prior_res_.reset();   // (sized by the old count: get_prior_residual allocates it again)
    n_prior_ = (int)n;
    return kOk;
}

int PoseGraphSolver::set_loss(int kind, double p0, double p1) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l)) return fail(kInvalidInput, "set_loss: unknown loss kind or a parameter its constructor refuses");
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipStreamSynchronize(stream_));
    loss_ = l;
    loss_set_ = true;
    voided_by(Change::kLoss);
    return kOk;
}

int PoseGraphSolver::set_information(const double* info) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    std::vector<double> packed;
    std::string why;
    if (info && !info_validate_and_pack(dof_, n_e_, info, &packed, &why)) return fail(kInvalidInput, why);
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipStreamSynchronize(stream_));
    DeviceBuffer<double> fresh;   // the members change only when the upload has succeeded
    if (info && n_e_ > 0) HIP_TRY(fresh.upload(packed));
    info_ = std::move(fresh);
    info_host_ = std::move(packed);
    voided_by(Change::kInformation);
    return kOk;
}

int PoseGraphSolver::get_information(int* present, double* info_out) const {
    const bool have = !info_host_.empty();
    if (present) *present = have ? 1 : 0;
    if (have && info_out) info_expand(dof_, n_e_, info_host_.data(), info_out);
    return kOk;
}

// what the edges carry: the loss of set_loss, else set_structure's Huber delta (or none)
void PoseGraphSolver::get_loss(int* kind, double out2[2]) const {
    out2[0] = out2[1] = 0.0;
    if (loss_set_) { *kind = loss_.kind; out2[0] = loss_.p0; out2[1] = loss_.p1; }
    else if (huber_delta_ > 0.0) { *kind = kLossHuber; out2[0] = huber_delta_; }
    else *kind = kLossNone;
}

int PoseGraphSolver::get_prior_residual(double* r7_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    if (n_prior_ == 0) return kOk;
    HIP_TRY(hipSetDevice(device_));
    if (!prior_res_) HIP_TRY(prior_res_.alloc((size_t)n_prior_ * amb_));   // kept with the priors (set_priors frees it)
    launch_pg_prior_export(manifold_, view(st_.cur), prior_res_, stream_);
    HIP_TRY(hipMemcpyAsync(r7_out, prior_res_, (size_t)n_prior_ * amb_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    return kOk;
}

int PoseGraphSolver::set_structure(const uint32_t* e_from, const uint32_t* e_to, const double* meas7,
                                   const int64_t* pose_col, const uint8_t* fix6, double huber_delta) {
    if (n_v_ <= 0) return fail(kInvalidInput, "No pose variables found");
    if (n_e_ < 0 || n_e_ > 2000000000LL) return fail(kInvalidInput, "edge count out of range");
    for (int64_t e = 0; e < n_e_; ++e)
        if (e_from[e] >= (uint64_t)n_v_ || e_to[e] >= (uint64_t)n_v_)
            return fail(kInvalidInput, "edge " + std::to_string(e) + " references a missing variable");
    HIP_TRY(hipSetDevice(device_));
    if (!stream_) HIP_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    huber_delta_ = huber_delta;
    loss_set_ = false;
    loss_ = PgLoss{};
    info_.reset(); info_host_.clear();
    n_ = dof_ * n_v_;
    const int nt = (int)((n_ + kNB - 1) / kNB);
    n_pad_ = (int64_t)nt * kNB;

    // ---- internal vertex order: whole tiles of kNB / dof consecutive vertices, permuted by a nested-dissection
    // ordering of the tile graph (see tile_order, plan_lists.h) -----------------------------------------------
    std::vector<uint8_t> adjm((size_t)nt * nt, 0);
    for (int64_t e = 0; e < n_e_; ++e) {
        const int a = (int)(e_from[e] / vpt_), b = (int)(e_to[e] / vpt_);
        if (a != b) { adjm[(size_t)a * nt + b] = 1; adjm[(size_t)b * nt + a] = 1; }
    }
    const std::vector<int> tperm = tile_order(nt, adjm, use_nd_, nd_leaf_);
    vmap_.resize(n_v_);
    for (int64_t v = 0; v < n_v_; ++v) vmap_[v] = (int)((int64_t)tperm[v / vpt_] * vpt_ + v % vpt_);
    map_ = block_column_map(std::vector<int64_t>(pose_col, pose_col + n_v_), vmap_, dof_);
    scale_.set_size(n_, n_pad_);
    std::vector<uint8_t> present((size_t)nt * nt, 0);
    for (int I = 0; I < nt; ++I) present[(size_t)I * nt + I] = 1;
    std::vector<uint32_t> ef(n_e_), et(n_e_);
    for (int64_t e = 0; e < n_e_; ++e) {
        ef[e] = (uint32_t)vmap_[e_from[e]]; et[e] = (uint32_t)vmap_[e_to[e]];
        int a = (int)(ef[e] / vpt_), b = (int)(et[e] / vpt_);
        if (a < b) std::swap(a, b);
        present[(size_t)a * nt + b] = 1;
    }
    {
        const std::string err = tp_.build(nt, present, stream_);
        if (!err.empty()) return fail(kInvalidInput, "Hessian tiles: " + err);
    }
    // measurements are constants: normalise once (SE3::from_translation_quaternion, se3.rs:107-113)
    // (SE2: BetweenFactor::new keeps SE2::from_xy_angle of the measurement, se2.rs:106-110)
    // (SO3: the measurement is an SO3 built from its quaternion, so3.rs:225-229 -- the vertex's own preparation)
    std::vector<double> mp((size_t)n_e_ * stride_, 0.0);
    for (int64_t e = 0; e < n_e_; ++e) {
        if (manifold_ == kManifoldSE2) se2_prepare(meas7 + 3 * e, mp.data() + (size_t)stride_ * e);
        else if (manifold_ == kManifoldSO3) So3Manifold::prepare(meas7 + 4 * e, mp.data() + (size_t)stride_ * e);
        else pose_normalise(meas7 + 7 * e, mp.data() + (size_t)stride_ * e);
    }
    std::vector<uint8_t> fx((size_t)dof_ * n_v_, 0);
    if (fix6) blocks_to_internal(vmap_, dof_, fix6, fx.data());
    // Row-owned from here on: the manifold's only assembly, or the option as it stands now.  Prior blocks are stored in the
    // order of the assembly they were given for, so a structure that changes the assembly starts without them.
    const bool row_owned = pg_row_owned(manifold_) || opt_row_owned_;
    if (row_owned != row_owned_) {
        prior_v_.reset(); prior_data_.reset(); prior_slot_.reset(); prior_res_.reset();
        n_prior_ = 0;
    }
    row_owned_ = row_owned;
    inc_ptr_.reset(); inc_edge_.reset();
    if (row_owned_) {   // the row-owned assembly walks each vertex's incident edges
        IncidentLists inc;
        if (!build_incident_lists(n_v_, n_e_, ef.data(), et.data(), &inc)) return fail(kInvalidInput, "incident-edge lists: out of range");
        HIP_TRY(inc_ptr_.upload(inc.ptr));
        HIP_TRY(inc_edge_.upload(inc.edge));
    }
    HIP_TRY(e_from_.upload(ef));
    HIP_TRY(e_to_.upload(et));
    HIP_TRY(meas_.upload(mp));
    HIP_TRY(fix_.upload(fx));
    for (int w = 0; w < 2; ++w) {
        HIP_TRY(poses_[w].alloc_zero(amb_ * (size_t)n_v_));
        HIP_TRY(posep_[w].alloc_zero(stride_ * (size_t)n_v_));
    }
    HIP_TRY(g_.alloc_zero(n_pad_));
    HIP_TRY(rhs_.alloc_zero(n_pad_));
    HIP_TRY(d_.alloc_zero(n_pad_));
    HIP_TRY(work_.alloc_zero(6 * (size_t)n_pad_));   // (TilePlan::solve workspace)
    HIP_TRY(partial_.alloc_zero(3 * (size_t)n_partial_));
    HIP_TRY(scal_.alloc_zero(16));
    HIP_TRY(hipDeviceSynchronize());
    have_structure_ = true;
    have_params_ = false;
    voided_by(Change::kStructure);
    release_dogleg_buffers();
    st_.cur = 0;
    return kOk;
}

int PoseGraphSolver::set_params(const double* poses7) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    HIP_TRY(hipSetDevice(device_));
    std::vector<double> hp(amb_ * (size_t)n_v_);
    blocks_to_internal(vmap_, amb_, poses7, hp.data());
    if (manifold_ == kManifoldSE2)   // the variable is held as SE2 -> DVector gives it: theta in (-pi, pi] (se2.rs:55-63)
        for (int64_t v = 0; v < n_v_; ++v) hp[3 * (size_t)v + 2] = se2_wrap_angle(hp[3 * (size_t)v + 2]);
    HIP_TRY(hipMemcpyAsync(poses_[st_.cur], hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
    launch_pg_prepare(manifold_, n_v_, poses_[st_.cur], posep_[st_.cur], stream_);
    HIP_TRY(hipStreamSynchronize(stream_));
    have_params_ = true;
    voided_by(Change::kParams);
    return kOk;
}

int PoseGraphSolver::get_params(double* poses7) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    std::vector<double> hp(amb_ * (size_t)n_v_);
    HIP_TRY(hipMemcpyAsync(hp.data(), poses_[st_.cur], hp.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    blocks_to_caller(vmap_, amb_, hp.data(), poses7);
    return kOk;
}

int PoseGraphSolver::cost(double* out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    timer_.begin(kPgCost, stream_);
    launch_pg_cost(manifold_, view(st_.cur), partial_, n_partial_, scal_, stream_);
    timer_.end(kPgCost, stream_);
    double ss = 0.0;
    HIP_TRY(hipMemcpyAsync(&ss, scal_, sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    *out = cost_from_sumsq(ss);
    return kOk;
}

// H + lambda I (tiles) and g = J^T r at the current parameters
int PoseGraphSolver::assemble(double lambda) {
    drop_dogleg_cache();   // (g_ is overwritten)
    timer_.begin(kPgAssemble, stream_);
    HIP_TRY(tp_.zero_tiles());
    HIP_TRY(hipMemsetAsync(g_, 0, n_pad_ * sizeof(double), stream_));
    tp_.add_diag((int)n_, scaled_ ? 0.0 : lambda, 1.0);  // lambda on the real rows, identity on the padding rows
    launch_pg_assemble(manifold_, row_owned_, view(st_.cur), tp_.tilemap(), g_, stream_);
    if (scaled_) {  // Jacobi scaling: H := D H D, then the damping of the scaled system
        tp_.scale_sym(scale_.dev);
        tp_.add_diag((int)n_, lambda, 1.0);
    }
    timer_.end(kPgAssemble, stream_);
    return kOk;
}

// the damped system (J^T J + lambda I) dx = -J^T r at the current parameters, ready to factorise
int PoseGraphSolver::rebuild_system(double lambda, double) {
    const int rc = assemble(lambda);
    if (rc != kOk) return rc;
    launch_pg_negate(n_pad_, g_, rhs_, stream_);
    if (scaled_) launch_vec_mul(n_pad_, rhs_, scale_.dev, rhs_, stream_);  // -D g
    return kOk;
}

int PoseGraphSolver::factor_now(int* failed, bool defer_flags) {
    timer_.begin(kPgFactor, stream_);
    HIP_TRY(tp_.factor(failed, defer_flags));
    timer_.end(kPgFactor, stream_);
    return kOk;
}

// No ladder here: a give-up is repaired (H again, the level launches), a failed pivot is the caller's error.
int PoseGraphSolver::recover_factor(double lambda, int failed, bool gave_up) {
    if (gave_up) {
        const int rc = factor_again(lambda, 0.0, &failed);
        if (rc != kOk) return rc;
    }
    return failed ? fail(kSingularMatrix, "Cholesky factorization failed (matrix may be singular)") : kOk;
}

// SparseCholeskySolver::solve_augmented_equation (cholesky.rs:159-230): (J^T J + lambda I) dx = -J^T r
int PoseGraphSolver::solve_augmented(double lambda, int variant, double* step_out, double* grad_out) {
    if (!have_params_) return fail(kInvalidState, "Block structure not built or parameters not set");
    if (variant != 0) return fail(kInvalidInput, "the pose-graph backend has the sparse Cholesky solver only");
    HIP_TRY(hipSetDevice(device_));
    return solve_damped(lambda, step_out, grad_out);
}
int PoseGraphSolver::solve_damped(double lambda, double* step_out, double* grad_out) {
    begin_solve(lambda);
    int rc = rebuild_system(lambda, 0.0);   // (drops the Dog-Leg cache)
    if (rc == kOk && !one_wait_) {   // the flags are waited for right behind the factorisation
        int failed = 0;
        rc = factor_fresh(lambda, 0.0, &failed);
        if (rc == kOk) rc = recover_factor(lambda, failed, false);   // (a failed pivot)
    }
    return rc != kOk ? rc : direct_solve(one_wait_, lambda, step_out, grad_out);
}

int PoseGraphSolver::enqueue_sweeps() {
    timer_.begin(kPgTriSolve, stream_);
    HIP_TRY(tp_.solve(rhs_, d_, work_));
    if (scaled_) launch_vec_mul(n_pad_, d_, scale_.dev, d_, stream_);  // apply_inverse_scaling: step = D y
    timer_.end(kPgTriSolve, stream_);
    return kOk;
}

int PoseGraphSolver::finish_step(double* step_out, double* grad_out) {
    st_.step_computed();
    if (dl_mode_) {   // TileBackend::dogleg_step: the sweeps have left the Gauss-Newton step in d_
        const int rc = enqueue_dogleg_tail(true);
        if (rc != kOk) return rc;
        HIP_TRY(hipStreamSynchronize(stream_));
        return kOk;
    }
    if (eager_eval_) { const int rc = enqueue_eager_eval(); if (rc != kOk) return rc; }   // what the LM loop asks next rides on this solve's wait
    if (step_out) { const int rc = export_columns({{d_, &map_, &scale_}}, ExportAs::kStep, step_out); if (rc != kOk) return rc; }
    if (grad_out) { const int rc = export_columns({{g_, &map_, &scale_}}, ExportAs::kGradient, grad_out); if (rc != kOk) return rc; }
    if (!step_out && !grad_out) HIP_TRY(hipStreamSynchronize(stream_));
    if (eager_eval_) post_eager_answers();
    return kOk;
}

int PoseGraphSolver::enqueue_step_stats() {
    timer_.begin(kPgStats, stream_);
    launch_step_stats(n_, g_, d_, last_lambda_, scaled_ ? scale_.dev.get() : nullptr, partial_, n_partial_, scal_ + 1, stream_);
    timer_.end(kPgStats, stream_);
    return kOk;
}
int PoseGraphSolver::enqueue_trial_point(double* sumsq_out) {
    const int t = st_.cur ^ 1;
    enqueue_retract(st_.cur, 1.0, t);
    timer_.begin(kPgCost, stream_);
    launch_pg_cost(manifold_, view(t), partial_, n_partial_, sumsq_out, stream_);
    timer_.end(kPgCost, stream_);
    return kOk;
}

int PoseGraphSolver::parameter_norm(double* out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    launch_sumsq(amb_ * n_v_, poses_[st_.cur], partial_, n_partial_, scal_ + 4, stream_);
    double h = 0.0;
    HIP_TRY(hipMemcpyAsync(&h, scal_ + 4, sizeof h, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    *out = sqrt(h);
    return kOk;
}

// ---- Jacobi column scaling (process_jacobian_generic, optimizer/mod.rs:749-763) -------------------
// compute_column_norms (linearizer/mod.rs:229-239): the squared column norms of the corrected Jacobian are the
// diagonal of J^T J, which the edge kernel already assembles.
int PoseGraphSolver::column_norms(double* norms_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    const bool was = scaled_;
    scaled_ = false;
    int rc = assemble(0.0);
    scaled_ = was;
    if (rc != kOk) return rc;
    st_.invalidate_step();
    tp_.diag(work_);
    std::vector<double> h(n_);
    HIP_TRY(hipMemcpyAsync(h.data(), work_, n_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    map_.scatter(h.data(), norms_out, 0.0, [](double n2, int64_t) { return sqrt(n2); });
    return kOk;
}

int PoseGraphSolver::set_column_scaling(const double* scaling) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built");
    HIP_TRY(hipSetDevice(device_));
    if (!scaling) { scaled_ = false; voided_by(Change::kScalingOff); return kOk; }
    voided_by(Change::kScalingVectors);   // (ahead of the checks: a refused vector has voided the step all the same)
    HIP_TRY(scale_.ensure());
    std::vector<double> staged;
    if (!scale_.accepts(map_, scaling, &staged)) return fail(kInvalidInput, JacobiScaling::kRefused);
    HIP_TRY(scale_.set_from_caller(std::move(staged), stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    scaled_ = true;
    return kOk;
}

int PoseGraphSolver::set_jacobi_scaling(bool on) {
    if (!on) { scaled_ = false; voided_by(Change::kScalingOff); return kOk; }
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(scale_.ensure());
    scaled_ = false;
    const int rc = assemble(0.0);
    if (rc != kOk) return rc;
    tp_.diag(work_);
    HIP_TRY(scale_.from_norms_sq(work_, n_, stream_));  // the padding keeps its 1
    HIP_TRY(hipStreamSynchronize(stream_));
    scaled_ = true;
    voided_by(Change::kScalingVectors);   // (the assembly above has dropped the Dog-Leg cache already)
    return kOk;
}

int PoseGraphSolver::lm_optimize(LmConfig* cfg, LmResult* res, LmIterRecord* hist, int hist_cap) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    return run_lm(*this, cfg, res, hist, hist_cap);
}

// ---- Gauss-Newton and Dog-Leg (tr_loop.h) -------------------------------------------------------------------------
int PoseGraphSolver::dogleg_segments(DlSegment out[2]) {
    out[0] = DlSegment{n_, g_, d_, scaled_ ? scale_.dev.get() : nullptr, nullptr, nullptr, n_pad_, &map_};
    return 1;
}

void PoseGraphSolver::enqueue_jv_gram(const double* const a[2], const double* const b[2], double* out3) {
    launch_pg_jv_gram(manifold_, view(st_.cur), a[0], b[0], partial_, n_partial_, out3, stream_);
}

int PoseGraphSolver::gn_optimize(GnConfig* cfg, LmResult* res, LmIterRecord* hist, int hist_cap) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    if (cfg->variant != 0) return fail(kInvalidInput, "the pose-graph backend has the sparse Cholesky solver only");
    return run_gauss_newton(*this, cfg, res, hist, hist_cap);
}

int PoseGraphSolver::dogleg_optimize(DlConfig* cfg, LmResult* res, DlIterRecord* hist, int hist_cap) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    if (cfg->variant != 0) return fail(kInvalidInput, "the pose-graph backend has the sparse Cholesky solver only");
    if (!(cfg->trust_region_radius > 0.0) || !(cfg->mu >= 0.0)) return fail(kInvalidInput, "Dog-Leg: the radius must be positive and mu non-negative");
    return run_dogleg(*this, cfg, res, hist, hist_cap);
}

int PoseGraphSolver::jv_gram(const double* a, const double* b, double out3[3]) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    return jv_gram_columns(a, b, out3);
}

// ---- parity / debug exports ------------------------------------------------------------------
int PoseGraphSolver::get_residual(double* r_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    DeviceBuffer<double> d;
    HIP_TRY(d.alloc(dof_ * (size_t)n_e_));
    launch_pg_export(manifold_, view(st_.cur), d, nullptr, stream_);
    hipError_t e = hipMemcpyAsync(r_out, d, dof_ * n_e_ * sizeof(double), hipMemcpyDeviceToHost, stream_);
    (void)hipStreamSynchronize(stream_);
    return check_hip(e, "get_residual");
}

int PoseGraphSolver::get_jacobian_blocks(double* j_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    DeviceBuffer<double> d;
    const size_t jn = 2 * (size_t)dof_ * dof_;   // [dof][2 dof] per edge
    HIP_TRY(d.alloc(jn * (size_t)n_e_));
    launch_pg_export(manifold_, view(st_.cur), nullptr, d, stream_);
    hipError_t e = hipMemcpyAsync(j_out, d, jn * n_e_ * sizeof(double), hipMemcpyDeviceToHost, stream_);
    (void)hipStreamSynchronize(stream_);
    return check_hip(e, "get_jacobian_blocks");
}

int PoseGraphSolver::get_hessian(double lambda, double* H_out, double* g_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    int rc = assemble(lambda);
    if (rc != kOk) return rc;
    st_.invalidate_step();
    if (g_out) { rc = export_columns({{g_, &map_, &scale_}}, ExportAs::kGradient, g_out); if (rc != kOk) return rc; }
    if (H_out) {
        memset(H_out, 0, (size_t)n_ * (size_t)n_ * sizeof(double));
        return export_tiles_dense(map_, n_, tp_.n_touched_slots(), H_out);
    }
    return kOk;
}

int PoseGraphSolver::covariance(double* out) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    if (!out) return fail(kInvalidInput, "cov_out is NULL");
    HIP_TRY(hipSetDevice(device_));
    std::string err;
    const int rc = tp_.inverse().blocks(map_.pos.data(), n_v_, dof_, out, &err);
    if (rc == 1) return fail(kInvalidState, "covariance: " + err);
    if (rc != 0) return fail(kDeviceError, "covariance: " + err);
    return kOk;
}

}  // namespace apex
