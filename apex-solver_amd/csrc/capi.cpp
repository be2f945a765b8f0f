// capi.cpp -- extern "C" surface declared in include/apexgpu.h: the bundle-adjustment handle.  (capi_pg.cpp: the pose-graph
// handle; capi_debug.cpp: the host-arithmetic debug entries and the lockstep solve; tile_debug.cpp: the tile Cholesky alone.)
// Every entry that takes the handle runs through with_handle() (capi_guard.h): handle first, then the argument checks.
#include <string.h>

#include <algorithm>
#include <string>

#include "capi_handles.h"
#ifdef APEX_WITH_RCCL
#include <rccl/rccl.h>
#endif

// APEX_SEGV_BACKTRACE=1 (debugging aid): the native stack of a crash on stderr (the GPU boxes have no debugger)
#include <execinfo.h>
#include <signal.h>
namespace {
void segv_backtrace(int sig) {
    void* frames[64];
    const int n = backtrace(frames, 64);
    backtrace_symbols_fd(frames, n, 2);
    raise(sig);
}
void segv_hook() {   // (on an alternate stack: a stack overflow is a SIGSEGV too)
    static const bool on = [] { const char* e = getenv("APEX_SEGV_BACKTRACE"); return e && e[0] == '1'; }();
    if (!on) return;
    static thread_local char alt[1 << 16];
    stack_t ss; ss.ss_sp = alt; ss.ss_size = sizeof(alt); ss.ss_flags = 0;
    (void)sigaltstack(&ss, nullptr);
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_handler = segv_backtrace; sa.sa_flags = SA_ONSTACK | SA_RESETHAND;
    (void)sigaction(SIGSEGV, &sa, nullptr);
}
}  // namespace

extern "C" {

const char* apexgpu_version(void) { return "apexgpu 0.1 (gfx950)"; }

int apexgpu_create(int64_t n_cam, int64_t n_pt, int64_t n_obs, int mode, int device, apexgpu_solver** out) {
    if (!out) return APEXGPU_ERR_INVALID_INPUT;
    *out = nullptr;
    if (mode < APEXGPU_MODE_BUNDLE_ADJUSTMENT || mode > APEXGPU_MODE_LANDMARKS_AND_INTRINSICS) return APEXGPU_ERR_INVALID_INPUT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return APEXGPU_ERR_DEVICE;
    return apex::HandleOwner::create(out, n_cam, n_pt, n_obs, mode, device);
}

void apexgpu_destroy(apexgpu_solver* h) { apex::HandleOwner::destroy(h); }

const char* apexgpu_last_error(const apexgpu_solver* h) {
    const char* e = "invalid handle";
    with_handle(h, [&](auto& s) { e = s.last_error(); return APEXGPU_OK; });
    return e;
}

int apexgpu_set_structure(apexgpu_solver* h, const uint32_t* cam_idx, const uint32_t* pt_idx, const double* obs_uv,
                          const int64_t* intr_col, const int64_t* pose_col, const int64_t* pt_col,
                          const uint8_t* fix_pose, const uint8_t* fix_intr, const uint8_t* fix_pt, double huber_delta) {
    return with_handle(h, [&](auto& s) {
        if (!cam_idx || !pt_idx || !obs_uv || !intr_col || !pose_col || !pt_col) return APEXGPU_ERR_INVALID_INPUT;
        return s.set_structure(cam_idx, pt_idx, obs_uv, intr_col, pose_col, pt_col, fix_pose, fix_intr, fix_pt, huber_delta);
    });
}
int apexgpu_set_cg_params(apexgpu_solver* h, int max_iterations, double tolerance) {
    return with_handle(h, [&](auto& s) {
        s.set_cg_params(max_iterations, tolerance);
        return APEXGPU_OK;
    });
}
int apexgpu_set_params(apexgpu_solver* h, const double* poses, const double* intr, const double* points) {
    return with_handle(h, [&](auto& s) {
        if (!poses || !intr || !points) return APEXGPU_ERR_INVALID_INPUT;
        return s.set_params(poses, intr, points);
    });
}
int apexgpu_set_loss(apexgpu_solver* h, int kind, double p0, double p1) {
    return with_handle(h, [&](auto& s) { return s.set_loss(kind, p0, p1); });
}
int apexgpu_get_loss(const apexgpu_solver* h, int* kind, double out2[2]) {
    return with_handle(h, [&](auto& s) {
        if (!kind || !out2) return APEXGPU_ERR_INVALID_INPUT;
        s.get_loss(kind, out2);
        return APEXGPU_OK;
    });
}
int apexgpu_set_pose_priors(apexgpu_solver* h, int64_t n, const uint32_t* cam, const double* data7, const double* huber_delta, const double* weight) {
    return with_handle(h, [&](auto& s) { return s.set_priors(false, n, cam, data7, huber_delta, weight); });
}
int apexgpu_set_intrinsic_priors(apexgpu_solver* h, int64_t n, const uint32_t* cam, const double* data3, const double* huber_delta, const double* weight) {
    return with_handle(h, [&](auto& s) { return s.set_priors(true, n, cam, data3, huber_delta, weight); });
}
int apexgpu_get_prior_residual(apexgpu_solver* h, double* pose_r7_out, double* intr_r3_out) {
    return with_handle(h, [&](auto& s) { return s.get_prior_residual(pose_r7_out, intr_r3_out); });
}
int apexgpu_get_params(apexgpu_solver* h, double* poses, double* intr, double* points) {
    return with_handle(h, [&](auto& s) {
        if (!poses || !intr || !points) return APEXGPU_ERR_INVALID_INPUT;
        return s.get_params(poses, intr, points);
    });
}
int apexgpu_cost(apexgpu_solver* h, double* cost) { return with_handle(h, [&](auto& s) { return s.cost(cost); }); }
int apexgpu_solve_augmented(apexgpu_solver* h, double lambda, int variant, double* step_out, double* grad_out) {
    return with_handle(h, [&](auto& s) {
        if (variant != APEXGPU_VARIANT_SPARSE && variant != APEXGPU_VARIANT_ITERATIVE && variant != APEXGPU_VARIANT_IMPLICIT)
            return APEXGPU_ERR_INVALID_INPUT;
        segv_hook();
        return s.solve_augmented(lambda, variant, step_out, grad_out);
    });
}
int apexgpu_assemble(apexgpu_solver* h, double lambda) { return with_handle(h, [&](auto& s) { return s.assemble_only(lambda); }); }
int apexgpu_step_stats(apexgpu_solver* h, double out3[3]) { return with_handle(h, [&](auto& s) { return s.step_stats(out3); }); }
int apexgpu_eval_step(apexgpu_solver* h, double* trial_cost) { return with_handle(h, [&](auto& s) { return s.eval_step(trial_cost); }); }
int apexgpu_commit_step(apexgpu_solver* h) { return with_handle(h, [&](auto& s) { return s.commit_step(); }); }
int apexgpu_discard_step(apexgpu_solver* h) { return with_handle(h, [&](auto& s) { return s.discard_step(); }); }
int apexgpu_parameter_norm(apexgpu_solver* h, double* out) { return with_handle(h, [&](auto& s) { return s.parameter_norm(out); }); }

int apexgpu_column_norms(apexgpu_solver* h, double* norms_out) {
    return with_handle(h, [&](auto& s) {
        if (!norms_out) return APEXGPU_ERR_INVALID_INPUT;
        return s.column_norms(norms_out);
    });
}
int apexgpu_set_column_scaling(apexgpu_solver* h, const double* scaling) { return with_handle(h, [&](auto& s) { return s.set_column_scaling(scaling); }); }

int apexgpu_lm_optimize(apexgpu_solver* h, apexgpu_lm_config* cfg, apexgpu_lm_result* result, apexgpu_lm_iter* history,
                        int history_capacity) {
    return with_handle(h, [&](auto& s) { return optimize_call(s, &apex::Solver::lm_optimize, cfg, result, history, history_capacity); });
}

int apexgpu_get_residual(apexgpu_solver* h, double* r_out) { return with_handle(h, [&](auto& s) { return s.get_residual(r_out); }); }
int apexgpu_get_jacobian_blocks(apexgpu_solver* h, double* jc_out, double* jl_out) {
    return with_handle(h, [&](auto& s) { return s.get_jacobian_blocks(jc_out, jl_out); });
}
int apexgpu_get_schur(apexgpu_solver* h, double* S_out, double* gred_out) { return with_handle(h, [&](auto& s) { return s.get_schur(S_out, gred_out); }); }
int apexgpu_camera_covariance(apexgpu_solver* h, double* cov_out) { return with_handle(h, [&](auto& s) { return s.camera_covariance(cov_out); }); }
int apexgpu_covariance_stats(apexgpu_solver* h, double out[6], double* group_ms, int group_cap) {
    return with_handle(h, [&](auto& s) { return covariance_stats(&s, out, group_ms, group_cap); });
}
int apexgpu_landmark_covariance(apexgpu_solver* h, double* cov_out) { return with_handle(h, [&](auto& s) { return s.landmark_covariance(cov_out); }); }
int apexgpu_landmark_covariance_stats(apexgpu_solver* h, double out[4]) {
    return with_handle(h, [&](auto& s) {
        if (!out) return APEXGPU_ERR_INVALID_INPUT;
        s.landmark_covariance_stats(out);
        return APEXGPU_OK;
    });
}
int apexgpu_get_landmark_blocks(apexgpu_solver* h, double* hinv_out, double* gl_out) {
    return with_handle(h, [&](auto& s) { return s.get_landmark_blocks(hinv_out, gl_out); });
}

int apexgpu_get_hessian_csc(apexgpu_solver* h, int64_t* nnz_out, int64_t* colptr_out, int64_t* rowidx_out, double* values_out) {
    return with_handle(h, [&](auto& s) { return s.get_hessian_csc(nnz_out, colptr_out, rowidx_out, values_out); });
}

int apexgpu_schur_matvec(apexgpu_solver* h, double lambda, const double* x_in, double* y_explicit, double* y_implicit) {
    return with_handle(h, [&](auto& s) {
        if (!x_in) return APEXGPU_ERR_INVALID_INPUT;
        return s.schur_matvec(lambda, x_in, y_explicit, y_implicit);
    });
}

int apexgpu_owned_landmarks(apexgpu_solver* h, uint8_t* mask) {
    return with_handle(h, [&](auto& s) {
        if (!mask) return APEXGPU_ERR_INVALID_INPUT;
        return s.owned_landmarks(mask);
    });
}
int apexgpu_export_step(apexgpu_solver* h, double* step_out, double* grad_out) { return with_handle(h, [&](auto& s) { return s.export_step(step_out, grad_out); }); }

int apexgpu_set_option(apexgpu_solver* h, const char* name, int value) {
    return with_handle(h, [&](auto& s) {
    const std::string n = name ? name : "";
    // Switches that shape what set_structure builds (task lists, tile order, partition) or what the captured hipGraphs
    // hold are rejected once the structure exists: flipping them later would launch kernels over lists that were never built.
    static const char* const structural[] = {"schur_form", "hubs_last", "dist_factor", "tree_sharding", "dist_selftest", "nested_dissection", "update_overlap",
                                             "split_u1", "flood_gate", "two_side", "factor_flow", "factor_flow_rows", "device_pair_list", "matrix_free_only",
                                             "auto_variant", "variant_cost_permille", "max_tile_updates"};
    if (s.has_structure())
        for (const char* k : structural)
            if (n == k) return APEXGPU_ERR_INVALID_STATE;
    if (n == "schur_form") {   // 4 the queued pair list (default; nine-column cameras), 3 the pair list with one running block per wave
        if (value != 3 && value != 4) return APEXGPU_ERR_INVALID_INPUT;
        s.set_schur_form(value);
    }
    else if (shared_option(&s, n, value)) return APEXGPU_OK;
    else if (n == "matrix_free_only") s.set_matrix_free_only(value != 0);
    else if (n == "auto_variant") s.set_auto_variant(value != 0);
    else if (n == "variant_cost_permille") s.set_variant_cost_permille(value);
    else if (n == "device_pair_list") s.set_device_pair_recs(value != 0);
    else if (n == "max_tile_updates") s.set_max_tile_updates(value);
    else if (n == "debug_occupy_cus") return s.debug_occupy_cus(value, 40000);   /* tests: block `value` CUs for 40 ms, starting now */
    else if (n == "hubs_last") s.set_hubs_last(value != 0);
    else if (n == "dist_factor") s.set_dist_factor(value != 0);
    else if (n == "tree_sharding") s.set_tree_sharding(value != 0);
    else if (n == "dist_selftest") s.set_dist_selftest(value);
    else return APEXGPU_ERR_INVALID_INPUT;
    return APEXGPU_OK;
    });
}
int apexgpu_enable_stage_timing(apexgpu_solver* h, int on) { return with_handle(h, [&](auto& s) { return stage_timing(&s, on); }); }
int apexgpu_reset_stage_times(apexgpu_solver* h) { return with_handle(h, [&](auto& s) { s.reset_stage_times(); return APEXGPU_OK; }); }
int apexgpu_stage_times(apexgpu_solver* h, double ms[APEXGPU_NUM_STAGES], int64_t calls[APEXGPU_NUM_STAGES]) {
    return with_handle(h, [&](auto& s) {
        s.stage_times(ms, calls);
        return APEXGPU_OK;
    });
}
int apexgpu_setup_times(apexgpu_solver* h, double seconds[6], double counts[4]) {
    return with_handle(h, [&](auto& s) {
        if (!seconds) return APEXGPU_ERR_INVALID_INPUT;
        for (int k = 0; k < 6; ++k) seconds[k] = s.setup_seconds()[k];
        if (counts) { counts[0] = s.n_hubs(); counts[1] = s.pair_blocks(); counts[2] = s.pair_slots(); counts[3] = s.schur_form(); }
        return APEXGPU_OK;
    });
}
int apexgpu_info(apexgpu_solver* h, double info[17]) {
    return with_handle(h, [&](auto& s) {
        info[0] = s.n_tile_rows(); info[1] = (double)s.tile_count(); info[2] = s.schur_scatter_pairs();
        info[3] = (double)s.cam_dof_internal(); info[4] = s.last_reg(); info[5] = s.last_pcg_iters();
        info[6] = s.touched_tiles(); info[7] = s.local_obs();
        info[8] = s.n_levels();
        int64_t a = 0, b = 0, c = 0;
        s.plan().op_counts(&a, &b, &c);
        info[9] = (double)a; info[10] = (double)b; info[11] = (double)c;
        info[12] = s.dist_top_columns(); info[13] = s.dist_local_fraction();
        info[14] = s.tree_sharded() ? 1.0 : 0.0;
        info[15] = s.schur_form();
        info[16] = (double)s.plan().n_diag_updates();
        return APEXGPU_OK;
    });
}

int apexgpu_debug_get_pair_records(apexgpu_solver* h, uint32_t* recs4_out, int64_t cap_slots) {
    return with_handle(h, [&](auto& s) {
        if (!recs4_out) return APEXGPU_ERR_INVALID_INPUT;
        return s.get_pair_records(recs4_out, cap_slots);
    });
}
int apexgpu_trim_host_cache(int64_t* released_bytes) {
    const size_t n = apex::HostBlockCache::get().trim();
    if (released_bytes) *released_bytes = (int64_t)n;
    return APEXGPU_OK;
}
int apexgpu_variant_costs(apexgpu_solver* h, double out[4]) {
    return with_handle(h, [&](auto& s) {
        if (!out) return APEXGPU_ERR_INVALID_INPUT;
        s.variant_costs(out);
        return APEXGPU_OK;
    });
}
int64_t apexgpu_host_cache_bytes(void) { return (int64_t)apex::HostBlockCache::get().kept_bytes(); }
int apexgpu_variant_info(apexgpu_solver* h, int asked_variant, int* used_variant, char* reason, int reason_len) {
    return with_handle(h, [&](auto& s) {
        if (asked_variant != APEXGPU_VARIANT_SPARSE && asked_variant != APEXGPU_VARIANT_ITERATIVE && asked_variant != APEXGPU_VARIANT_IMPLICIT)
            return APEXGPU_ERR_INVALID_INPUT;
        if (used_variant) *used_variant = s.variant_used(asked_variant);
        if (reason && reason_len > 0) {
            const std::string& r = s.variant_reason();
            const size_t n = std::min<size_t>(r.size(), (size_t)reason_len - 1);
            memcpy(reason, r.data(), n);
            reason[n] = 0;
        }
        return APEXGPU_OK;
    });
}

int apexgpu_counters(apexgpu_solver* h, int64_t out[4]) { return with_handle(h, [&](auto& s) { return counters(&s, out); }); }

int apexgpu_get_unique_id(void* out128) {
#ifdef APEX_WITH_RCCL
    if (!out128) return APEXGPU_ERR_INVALID_INPUT;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return APEXGPU_ERR_DEVICE;
    memcpy(out128, &id, 128);
    return APEXGPU_OK;
#else
    (void)out128;
    return APEXGPU_ERR_INVALID_STATE;
#endif
}
int apexgpu_comm_init(apexgpu_solver* h, int world, int rank, const void* unique_id128) {
    return with_handle(h, [&](auto& s) {
        if (!unique_id128) return APEXGPU_ERR_INVALID_INPUT;
        return s.comm_init(world, rank, unique_id128);
    });
}
int apexgpu_comm_init_shm(apexgpu_solver* h, int world, int rank, const char* name) {
    return with_handle(h, [&](auto& s) {
        if (!name) return APEXGPU_ERR_INVALID_INPUT;
        return s.comm_init_shm(world, rank, name);
    });
}
int apexgpu_set_shard(apexgpu_solver* h, int rank, int world) { return with_handle(h, [&](auto& s) { return s.set_shard(rank, world); }); }

int apexgpu_jv_gram(apexgpu_solver* h, const double* a, const double* b, double out3[3]) {
    return with_handle(h, [&](auto& s) {
        if (!a || !b || !out3) return APEXGPU_ERR_INVALID_INPUT;
        return s.jv_gram(a, b, out3);
    });
}
int apexgpu_dogleg_step(apexgpu_solver* h, double mu, double radius, int reuse, double out8[8]) {
    return with_handle(h, [&](auto& s) { return s.dogleg_step(mu, radius, reuse, reinterpret_cast<apex::DoglegStepInfo*>(out8)); });
}
int apexgpu_dogleg_optimize(apexgpu_solver* h, apexgpu_dl_config* cfg, apexgpu_lm_result* result, apexgpu_dl_iter* history,
                            int history_capacity) {
    return with_handle(h, [&](auto& s) { return optimize_call(s, &apex::Solver::dogleg_optimize, cfg, result, history, history_capacity); });
}

}  // extern "C"
