// capi_pg.cpp -- extern "C" surface declared in include/apexgpu.h: the pose-graph handle (SE3, SE2, SO3) and
// apexgpu_loss_evaluate.  Every entry that takes the handle runs through with_handle() (capi_guard.h).
#include <string>

#include "capi_handles.h"

static int pg_create(int64_t n_vertices, int64_t n_edges, int device, int manifold, apexgpu_pg_solver** out) {
    if (!out) return APEXGPU_ERR_INVALID_INPUT;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return APEXGPU_ERR_DEVICE;
    return apex::HandleOwner::create(out, n_vertices, n_edges, device, manifold);
}

extern "C" {

int apexgpu_pg_create(int64_t n_vertices, int64_t n_edges, int device, apexgpu_pg_solver** out) {
    return pg_create(n_vertices, n_edges, device, APEXGPU_MANIFOLD_SE3, out);
}
int apexgpu_pg_create_se2(int64_t n_vertices, int64_t n_edges, int device, apexgpu_pg_solver** out) {
    return pg_create(n_vertices, n_edges, device, APEXGPU_MANIFOLD_SE2, out);
}
int apexgpu_pg_create_so3(int64_t n_vertices, int64_t n_edges, int device, apexgpu_pg_solver** out) {
    return pg_create(n_vertices, n_edges, device, APEXGPU_MANIFOLD_SO3, out);
}
int apexgpu_pg_manifold(const apexgpu_pg_solver* h, int out3[3]) {
    return with_handle(h, [&](auto& s) {
        if (!out3) return APEXGPU_ERR_INVALID_INPUT;
        out3[0] = s.manifold(); out3[1] = s.ambient(); out3[2] = s.dof();
        return APEXGPU_OK;
    });
}
void apexgpu_pg_destroy(apexgpu_pg_solver* h) { apex::HandleOwner::destroy(h); }
const char* apexgpu_pg_last_error(const apexgpu_pg_solver* h) {
    const char* e = "invalid handle";
    with_handle(h, [&](auto& s) { e = s.last_error(); return APEXGPU_OK; });
    return e;
}
int apexgpu_pg_set_structure(apexgpu_pg_solver* h, const uint32_t* e_from, const uint32_t* e_to, const double* meas7,
                             const int64_t* pose_col, const uint8_t* fix6, double huber_delta) {
    return with_handle(h, [&](auto& s) {
        if (!e_from || !e_to || !meas7 || !pose_col) return APEXGPU_ERR_INVALID_INPUT;
        return s.set_structure(e_from, e_to, meas7, pose_col, fix6, huber_delta);
    });
}
int apexgpu_pg_set_params(apexgpu_pg_solver* h, const double* poses7) {
    return with_handle(h, [&](auto& s) {
        if (!poses7) return APEXGPU_ERR_INVALID_INPUT;
        return s.set_params(poses7);
    });
}
int apexgpu_pg_get_params(apexgpu_pg_solver* h, double* poses7) {
    return with_handle(h, [&](auto& s) {
        if (!poses7) return APEXGPU_ERR_INVALID_INPUT;
        return s.get_params(poses7);
    });
}
int apexgpu_pg_cost(apexgpu_pg_solver* h, double* cost) { return with_handle(h, [&](auto& s) { return s.cost(cost); }); }
int apexgpu_pg_solve_augmented(apexgpu_pg_solver* h, double lambda, double* step_out, double* grad_out) {
    return with_handle(h, [&](auto& s) { return s.solve_augmented(lambda, 0, step_out, grad_out); });
}
int apexgpu_pg_step_stats(apexgpu_pg_solver* h, double out3[3]) { return with_handle(h, [&](auto& s) { return s.step_stats(out3); }); }
int apexgpu_pg_eval_step(apexgpu_pg_solver* h, double* trial_cost) { return with_handle(h, [&](auto& s) { return s.eval_step(trial_cost); }); }
int apexgpu_pg_commit_step(apexgpu_pg_solver* h) { return with_handle(h, [&](auto& s) { return s.commit_step(); }); }
int apexgpu_pg_discard_step(apexgpu_pg_solver* h) { return with_handle(h, [&](auto& s) { return s.discard_step(); }); }
int apexgpu_pg_parameter_norm(apexgpu_pg_solver* h, double* out) { return with_handle(h, [&](auto& s) { return s.parameter_norm(out); }); }
int apexgpu_pg_column_norms(apexgpu_pg_solver* h, double* norms_out) {
    return with_handle(h, [&](auto& s) {
        if (!norms_out) return APEXGPU_ERR_INVALID_INPUT;
        return s.column_norms(norms_out);
    });
}
int apexgpu_pg_set_column_scaling(apexgpu_pg_solver* h, const double* scaling) { return with_handle(h, [&](auto& s) { return s.set_column_scaling(scaling); }); }

int apexgpu_pg_lm_optimize(apexgpu_pg_solver* h, apexgpu_lm_config* cfg, apexgpu_lm_result* result, apexgpu_lm_iter* history,
                           int history_capacity) {
    return with_handle(h, [&](auto& s) { return optimize_call(s, &apex::PoseGraphSolver::lm_optimize, cfg, result, history, history_capacity); });
}
int apexgpu_pg_jv_gram(apexgpu_pg_solver* h, const double* a, const double* b, double out3[3]) {
    return with_handle(h, [&](auto& s) {
        if (!a || !b || !out3) return APEXGPU_ERR_INVALID_INPUT;
        return s.jv_gram(a, b, out3);
    });
}
int apexgpu_pg_dogleg_step(apexgpu_pg_solver* h, double mu, double radius, int reuse, double out8[8]) {
    return with_handle(h, [&](auto& s) { return s.dogleg_step(mu, radius, reuse, reinterpret_cast<apex::DoglegStepInfo*>(out8)); });
}
int apexgpu_pg_gn_optimize(apexgpu_pg_solver* h, apexgpu_gn_config* cfg, apexgpu_lm_result* result, apexgpu_lm_iter* history,
                           int history_capacity) {
    return with_handle(h, [&](auto& s) { return optimize_call(s, &apex::PoseGraphSolver::gn_optimize, cfg, result, history, history_capacity); });
}
int apexgpu_pg_dogleg_optimize(apexgpu_pg_solver* h, apexgpu_dl_config* cfg, apexgpu_lm_result* result, apexgpu_dl_iter* history,
                               int history_capacity) {
    return with_handle(h, [&](auto& s) { return optimize_call(s, &apex::PoseGraphSolver::dogleg_optimize, cfg, result, history, history_capacity); });
}
int apexgpu_pg_get_residual(apexgpu_pg_solver* h, double* r_out) { return with_handle(h, [&](auto& s) { return s.get_residual(r_out); }); }
int apexgpu_pg_get_jacobian_blocks(apexgpu_pg_solver* h, double* j_out) { return with_handle(h, [&](auto& s) { return s.get_jacobian_blocks(j_out); }); }
int apexgpu_pg_set_priors(apexgpu_pg_solver* h, int64_t n, const uint32_t* vertex, const double* data7, const double* huber_delta) {
    return with_handle(h, [&](auto& s) {
        if (n > 0 && (!vertex || !data7)) return APEXGPU_ERR_INVALID_INPUT;
        return s.set_priors(n, vertex, data7, huber_delta);
    });
}
int apexgpu_pg_set_loss(apexgpu_pg_solver* h, int kind, double p0, double p1) {
    return with_handle(h, [&](auto& s) { return s.set_loss(kind, p0, p1); });
}
int apexgpu_pg_get_loss(const apexgpu_pg_solver* h, int* kind, double out2[2]) {
    return with_handle(h, [&](auto& s) {
        if (!kind || !out2) return APEXGPU_ERR_INVALID_INPUT;
        s.get_loss(kind, out2);
        return APEXGPU_OK;
    });
}
int apexgpu_pg_set_information(apexgpu_pg_solver* h, const double* info) {
    return with_handle(h, [&](auto& s) { return s.set_information(info); });
}
int apexgpu_pg_get_information(apexgpu_pg_solver* h, int* present, double* info_out) {
    return with_handle(h, [&](auto& s) {
        if (!present) return APEXGPU_ERR_INVALID_INPUT;
        return s.get_information(present, info_out);
    });
}
int apexgpu_loss_evaluate(int kind, double p0, double p1, double s, double out6[6]) {
    apex::PgLoss l;
    if (!out6 || !apex::pg_loss_make(kind, p0, p1, &l)) return APEXGPU_ERR_INVALID_INPUT;
    apex::pg_loss_evaluate(l, s, out6);
    const apex::PgCorrector c = apex::pg_corrector(out6, s);
    out6[3] = c.sqrt_rho1; out6[4] = c.residual_scaling; out6[5] = c.alpha_sq_norm;
    return APEXGPU_OK;
}
int apexgpu_pg_get_prior_residual(apexgpu_pg_solver* h, double* r7_out) {
    return with_handle(h, [&](auto& s) { return s.get_prior_residual(r7_out); });
}
int apexgpu_pg_get_hessian(apexgpu_pg_solver* h, double lambda, double* H_out, double* g_out) {
    return with_handle(h, [&](auto& s) { return s.get_hessian(lambda, H_out, g_out); });
}
int apexgpu_pg_covariance(apexgpu_pg_solver* h, double* cov_out) {
    return with_handle(h, [&](auto& s) { return s.covariance(cov_out); });
}
int apexgpu_pg_covariance_stats(apexgpu_pg_solver* h, double out[6], double* group_ms, int group_cap) {
    return with_handle(h, [&](auto& s) { return covariance_stats(&s, out, group_ms, group_cap); });
}
int apexgpu_pg_set_option(apexgpu_pg_solver* h, const char* name, int value) {
    return with_handle(h, [&](auto& s) {
        const std::string n = name ? name : "";
        if (n == "row_owned_assembly")   /* read by the next set_structure; SE2 and SO3 have no other assembly and refuse 0 */
            return (value == 0 || value == 1) && s.set_row_owned_option(value == 1) ? APEXGPU_OK : APEXGPU_ERR_INVALID_INPUT;
        return shared_option(&s, n, value) ? APEXGPU_OK : APEXGPU_ERR_INVALID_INPUT;
    });
}
int apexgpu_pg_enable_stage_timing(apexgpu_pg_solver* h, int on) { return with_handle(h, [&](auto& s) { return stage_timing(&s, on); }); }
int apexgpu_pg_reset_stage_times(apexgpu_pg_solver* h) { return with_handle(h, [&](auto& s) { s.reset_stage_times(); return APEXGPU_OK; }); }
int apexgpu_pg_stage_times(apexgpu_pg_solver* h, double ms[APEXGPU_PG_NUM_STAGES], int64_t calls[APEXGPU_PG_NUM_STAGES]) {
    return with_handle(h, [&](auto& s) {
        s.stage_times(ms, calls);
        return APEXGPU_OK;
    });
}
int apexgpu_pg_counters(apexgpu_pg_solver* h, int64_t out[4]) { return with_handle(h, [&](auto& s) { return counters(&s, out); }); }
int apexgpu_pg_info(apexgpu_pg_solver* h, double info[9]) {
    return with_handle(h, [&](auto& s) {
        info[0] = s.n_tile_rows(); info[1] = (double)s.tile_count(); info[2] = (double)s.touched_tiles();
        info[3] = s.n_levels(); info[4] = (double)s.dof() * (double)s.n_vertices();
        int64_t a = 0, b = 0, c = 0;
        s.plan().op_counts(&a, &b, &c);
        info[5] = (double)a; info[6] = (double)b; info[7] = (double)c;
        info[8] = (double)s.plan().n_diag_updates();
        return APEXGPU_OK;
    });
}

}  // extern "C"
