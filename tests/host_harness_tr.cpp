// host_harness_tr.cpp -- tr_loop.cpp + lm_loop.cpp + dogleg_combine.hpp as a stand-alone host program (no HIP): the loops drive a
// small dense nonlinear problem in plain C++, the reference's Rosenbrock factor pair (dog_leg.rs:1426-1485: r1 = 10 (x2 - x1^2),
// r2 = 1 - x1 on two one-dimensional variables), and print their histories for tests/test_tr_loop_host.py to compare with the
// numpy loops of tests/np_ref_trust_region.py.
//
//   host_harness_tr combine gg hh gh uu uw ww delta           -> alpha beta c_g c_h step_norm predicted type
//   host_harness_tr dl x1 x2 radius mu scaling reuse maxit    -> status iterations, then one history row per line
//   host_harness_tr gn x1 x2 scaling maxit
//   host_harness_tr lm x1 x2 scaling maxit
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dogleg_combine.hpp"
#include "tr_loop.h"

using namespace apex;

namespace {

struct Rosenbrock : TrBackend {
    double x[2], xt[2], d[2] = {0, 0}, s[2] = {1, 1}, g[2] = {0, 0}, h[2] = {0, 0}, H[3] = {0, 0, 0};   // g, h, H: scaled; H = (00, 01, 11) undamped
    double lambda = 0.0;
    DoglegSums sums{};
    bool have_cache = false, have_step = false, have_trial = false, is_dl = false;
    DoglegStepInfo info{};
    std::string err;

    static void residual(const double* p, double r[2]) { r[0] = 10.0 * (p[1] - p[0] * p[0]); r[1] = 1.0 - p[0]; }
    static double cost_at(const double* p) {
        double r[2];
        residual(p, r);
        const double nrm = sqrt(r[0] * r[0] + r[1] * r[1]);
        return 0.5 * nrm * nrm;
    }
    void linearize() {   // H = D J^T J D, g = D J^T r
        double r[2];
        residual(x, r);
        const double J[2][2] = {{-20.0 * x[0] * s[0], 10.0 * s[1]}, {-1.0 * s[0], 0.0}};
        H[0] = J[0][0] * J[0][0] + J[1][0] * J[1][0];
        H[1] = J[0][0] * J[0][1] + J[1][0] * J[1][1];
        H[2] = J[0][1] * J[0][1] + J[1][1] * J[1][1];
        g[0] = J[0][0] * r[0] + J[1][0] * r[1];
        g[1] = J[0][1] * r[0] + J[1][1] * r[1];
    }
    int solve(double lam, double y[2]) {   // (H + lam I) y = -g by Cholesky
        const double a = H[0] + lam, b = H[1], c = H[2] + lam;
        if (!(a > 0.0)) return kSingularMatrix;
        const double l00 = sqrt(a), l10 = b / l00, p = c - l10 * l10;
        if (!(p > 0.0)) return kSingularMatrix;
        const double l11 = sqrt(p);
        const double z0 = -g[0] / l00, z1 = (-g[1] - l10 * z0) / l11;
        y[1] = z1 / l11;
        y[0] = (z0 - l10 * y[1]) / l00;
        return kOk;
    }

    int cost(double* out) override { *out = cost_at(x); return kOk; }
    int solve_augmented(double lam, int variant, double*, double*) override {
        have_step = have_trial = is_dl = false; have_cache = false;
        if (variant != 0) { err = "variant"; return kInvalidInput; }
        linearize();
        lambda = lam;
        const int rc = solve(lam, h);
        if (rc != kOk) { err = "Cholesky factorization failed (matrix may be singular)"; return rc; }
        d[0] = s[0] * h[0]; d[1] = s[1] * h[1];
        have_step = true;
        return kOk;
    }
    int step_stats(double out3[3]) override {
        if (!have_step) return kInvalidState;
        if (is_dl) { out3[0] = info.gradient_norm; out3[1] = info.step_norm; out3[2] = info.predicted_reduction; return kOk; }
        out3[0] = sqrt(g[0] * g[0] + g[1] * g[1]);
        out3[1] = sqrt(d[0] * d[0] + d[1] * d[1]);
        out3[2] = 0.5 * (d[0] * (lambda * d[0] - g[0]) + d[1] * (lambda * d[1] - g[1]));   // (levenberg_marquardt.rs:721-727, as coded)
        return kOk;
    }
    int eval_step(double* trial_cost) override {
        if (!have_step) return kInvalidState;
        xt[0] = x[0] + d[0]; xt[1] = x[1] + d[1];
        have_trial = true;
        *trial_cost = cost_at(xt);
        return kOk;
    }
    int commit_step() override {
        if (!have_trial) return kInvalidState;
        x[0] = xt[0]; x[1] = xt[1];
        have_trial = have_step = false;
        return kOk;
    }
    int discard_step() override {
        if (!have_trial) return kInvalidState;
        x[0] = xt[0] - d[0]; x[1] = xt[1] - d[1];   // apply_negative_parameter_step
        have_trial = have_step = false;
        return kOk;
    }
    int parameter_norm(double* out) override { *out = sqrt(x[0] * x[0] + x[1] * x[1]); return kOk; }
    int set_jacobi_scaling(bool on) override {
        have_cache = false;
        s[0] = s[1] = 1.0;
        if (!on) return kOk;
        linearize();
        s[0] = 1.0 / (1.0 + sqrt(H[0])); s[1] = 1.0 / (1.0 + sqrt(H[2]));
        return kOk;
    }
    const char* last_error() const override { return err.c_str(); }

    int dogleg_step(double mu, double radius, int reuse, DoglegStepInfo* out) override {
        have_step = have_trial = false;
        if (reuse) {
            if (!have_cache) { err = "no cache"; return kInvalidState; }
        } else {
            have_cache = false;
            linearize();
            const int rc = solve(mu, h);
            if (rc != kOk) { err = "Cholesky factorization failed (matrix may be singular)"; return rc; }
            const double Hg[2] = {H[0] * g[0] + H[1] * g[1], H[1] * g[0] + H[2] * g[1]};
            const double Hh[2] = {H[0] * h[0] + H[1] * h[1], H[1] * h[0] + H[2] * h[1]};
            sums = DoglegSums{g[0] * g[0] + g[1] * g[1], h[0] * h[0] + h[1] * h[1], g[0] * h[0] + g[1] * h[1],
                              g[0] * Hg[0] + g[1] * Hg[1], g[0] * Hh[0] + g[1] * Hh[1], h[0] * Hh[0] + h[1] * Hh[1]};
            have_cache = true;
        }
        const DoglegStep st = dogleg_combine(sums, radius);
        for (int i = 0; i < 2; ++i) d[i] = s[i] * (st.c_g * -g[i] + st.c_h * h[i]);
        info = DoglegStepInfo{sqrt(sums.gg), sqrt(d[0] * d[0] + d[1] * d[1]), st.predicted_reduction, (double)st.type, st.alpha, st.beta,
                              st.step_norm, reuse ? 1.0 : 0.0};
        have_step = is_dl = true;
        if (out) *out = info;
        return kOk;
    }
};

int usage() {
    fprintf(stderr, "usage: host_harness_tr combine|dl|gn|lm ...\n");
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    const std::string mode = argv[1];
    auto num = [&](int i) { return strtod(argv[i], nullptr); };
    if (mode == "combine" && argc == 9) {
        const DoglegStep o = dogleg_combine(DoglegSums{num(2), num(3), num(4), num(5), num(6), num(7)}, num(8));
        printf("%.17g %.17g %.17g %.17g %.17g %.17g %d\n", o.alpha, o.beta, o.c_g, o.c_h, o.step_norm, o.predicted_reduction, o.type);
        return 0;
    }
    Rosenbrock b;
    LmResult res;
    if (mode == "dl" && argc == 9) {
        b.x[0] = num(2); b.x[1] = num(3);
        DlConfig c{atoi(argv[8]), 1e-6, 1e-8, 1e-10, num(4), 1e-12, 1e12, 0.5, 0.75, 0.25, num(5), 1e-8, 1.0, 10.0, -1.0, -1.0, 0, atoi(argv[6]), atoi(argv[7])};
        std::vector<DlIterRecord> hist(c.max_iterations + 2);
        const int rc = run_dogleg(b, &c, &res, hist.data(), (int)hist.size());
        if (rc != kOk) { fprintf(stderr, "run_dogleg: %d %s\n", rc, b.last_error()); return 1; }
        printf("%d %d %.17g %.17g %d\n", res.status, res.iterations, c.trust_region_radius, c.mu, res.jacobian_evaluations);
        for (int i = 0; i < res.iterations; ++i) {
            const double* r = &hist[i].cost;
            for (int k = 0; k < 12; ++k) printf("%.17g%c", r[k], k == 11 ? '\n' : ' ');
        }
        return 0;
    }
    if ((mode == "gn" || mode == "lm") && argc == 6) {
        b.x[0] = num(2); b.x[1] = num(3);
        std::vector<LmIterRecord> hist(atoi(argv[5]) + 2);
        int rc;
        if (mode == "gn") {
            GnConfig c{atoi(argv[5]), 1e-6, 1e-8, 1e-10, -1.0, -1.0, 0, atoi(argv[4])};
            rc = run_gauss_newton(b, &c, &res, hist.data(), (int)hist.size());
        } else {
            LmConfig c{atoi(argv[5]), 1e-6, 1e-8, 1e-10, 1e-3, 1e-12, 1e12, 2.0, 1e4, 1e-32, -1.0, -1.0, 0, atoi(argv[4])};
            rc = run_lm(b, &c, &res, hist.data(), (int)hist.size());
        }
        if (rc != kOk) { fprintf(stderr, "loop: %d %s\n", rc, b.last_error()); return 1; }
        printf("%d %d %.17g %.17g %d\n", res.status, res.iterations, 0.0, 0.0, res.jacobian_evaluations);
        for (int i = 0; i < res.iterations; ++i) {
            const double* r = &hist[i].cost;
            for (int k = 0; k < 8; ++k) printf("%.17g%c", r[k], k == 7 ? '\n' : ' ');
        }
        return 0;
    }
    return usage();
}
