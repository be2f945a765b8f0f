// host_harness_loss.cpp -- pg_loss.hpp and the general-loss paths of pg_device.hpp / pg2_device.hpp compiled for the host, for
// tests/test_loss_device_math_host.py (shared library) and, with -DHL_MAIN, as a stand-alone program that walks the same
// code over a grid (the build that runs under -fsanitize=address,undefined).
//
// Poses and measurements come in stored form (SE3: t, qw qx qy qz; SE2: x y theta) and are prepared here as k_pg_prepare
// and set_structure do.  Every per-edge result is in the form the kernels use:
//   hl_edge    M::export_edge     corrected residual and the literal J~ = [dr/dk0 | dr/dk1]
//   hl_blocks  SE3: the body of k_pg_edges (EdgeNormal6: the normal-equation form of the second arm); SE2: pg2_assemble_row on
//              the graph that holds just this edge.  H_aa, H_bb (a = from, b = to), H_ba = J~_b^T J~_a, g_a, g_b; a self-loop
//              puts everything on H_aa, g_a as the kernels do.
//   hl_jv      M::edge_jv         u = J~ [a0; a1], w = J~ [b0; b1]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pg2_device.hpp"
#include "pg_device.hpp"
#include "pg_loss.hpp"

using namespace apex;

namespace {

template <class M>
void prepare3(const double* k0, const double* k1, const double* m, double* p0, double* p1, double* pm) {
    memset(p0, 0, sizeof(double) * M::kStride); memset(p1, 0, sizeof(double) * M::kStride); memset(pm, 0, sizeof(double) * M::kStride);
    M::prepare(k0, p0); M::prepare(k1, p1); M::prepare(m, pm);
}

void se3_blocks(const double* k0, const double* k1, const double* m, const PgLoss& loss, int self_loop, double* Haa, double* Hbb,
                double* Hba, double* ga, double* gb) {
    double r[6], H[36];
    Jac6 J0, J1;
    EdgeNormal6 nf;
    memset(Haa, 0, 36 * sizeof(double)); memset(Hbb, 0, 36 * sizeof(double)); memset(Hba, 0, 36 * sizeof(double));
    memset(ga, 0, 6 * sizeof(double)); memset(gb, 0, 6 * sizeof(double));
    if (!between_linearize_general(k0, k1, m, loss, r, J0, J1, nf)) return;
    jtj(J0, J0, H); nf.correct(H, nf.w0, nf.w0);
    for (int i = 0; i < 36; ++i) Haa[i] += H[i];
    jtj(J1, J1, H); nf.correct(H, nf.w1, nf.w1);
    for (int i = 0; i < 36; ++i) (self_loop ? Haa : Hbb)[i] += H[i];
    if (!self_loop) {
        jtj(J1, J0, H); nf.correct(H, nf.w1, nf.w0);
        for (int i = 0; i < 36; ++i) Hba[i] = H[i];
    } else {
        jtj(J0, J1, H); nf.correct(H, nf.w0, nf.w1);
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) Haa[6 * i + j] += H[6 * i + j] + H[6 * j + i];
    }
    double gv[6];
    nf.grad(nf.w0, gv);
    for (int i = 0; i < 6; ++i) ga[i] += gv[i];
    nf.grad(nf.w1, gv);
    for (int i = 0; i < 6; ++i) (self_loop ? ga : gb)[i] += gv[i];
}

void se2_blocks(const double* p0, const double* p1, const double* pm, const PgLoss& loss, int self_loop, double* Haa, double* Hbb,
                double* Hba, double* ga, double* gb) {
    double posep[2 * kPose2Stride];
    memcpy(posep, p0, sizeof(double) * kPose2Stride); memcpy(posep + kPose2Stride, p1, sizeof(double) * kPose2Stride);
    const uint32_t e_from[1] = {0}, e_to[1] = {self_loop ? 0u : 1u}, inc_edge[2] = {0, 0};
    const int inc_ptr[3] = {0, 1, 2};
    memset(Hbb, 0, 9 * sizeof(double)); memset(Hba, 0, 9 * sizeof(double)); memset(gb, 0, 3 * sizeof(double));
    pg2_assemble_row(0u, posep, pm, e_from, e_to, inc_ptr, inc_edge, loss, Haa, ga, [&](uint32_t, const double*) {});
    if (!self_loop)
        pg2_assemble_row(1u, posep, pm, e_from, e_to, inc_ptr, inc_edge, loss, Hbb, gb,
                         [&](uint32_t, const double* B) { for (int i = 0; i < 9; ++i) Hba[i] += B[i]; });
}

}  // namespace

extern "C" {

// out6 = {rho, rho', rho'', sqrt_rho1, residual_scaling, alpha_sq_norm}; 0, or -1 where the constructor refuses
int hl_loss(int kind, double p0, double p1, double s, double* out6) {
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l)) return -1;
    pg_loss_evaluate(l, s, out6);
    const PgCorrector c = pg_corrector(out6, s);
    out6[3] = c.sqrt_rho1; out6[4] = c.residual_scaling; out6[5] = c.alpha_sq_norm;
    return 0;
}

// Corrector::new on a given (rho, rho', rho''): out3 = {sqrt_rho1, residual_scaling, alpha_sq_norm}
void hl_corrector(const double* rho3, double s, double* out3) {
    const PgCorrector c = pg_corrector(rho3, s);
    out3[0] = c.sqrt_rho1; out3[1] = c.residual_scaling; out3[2] = c.alpha_sq_norm;
}

int hl_edge(int manifold, const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, double* r, double* J) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[8], p1[8], pm[8];
    if (manifold == 1) { prepare3<Se2Manifold>(k0, k1, m, p0, p1, pm); Se2Manifold::export_edge(p0, p1, pm, l, r, J); }
    else { prepare3<Se3Manifold>(k0, k1, m, p0, p1, pm); Se3Manifold::export_edge(p0, p1, pm, l, r, J); }
    return 0;
}

int hl_blocks(int manifold, const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, int self_loop,
              double* Haa, double* Hbb, double* Hba, double* ga, double* gb) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[8], p1[8], pm[8];
    if (manifold == 1) { prepare3<Se2Manifold>(k0, self_loop ? k0 : k1, m, p0, p1, pm); se2_blocks(p0, p1, pm, l, self_loop, Haa, Hbb, Hba, ga, gb); }
    else { prepare3<Se3Manifold>(k0, self_loop ? k0 : k1, m, p0, p1, pm); se3_blocks(p0, p1, pm, l, self_loop, Haa, Hbb, Hba, ga, gb); }
    return 0;
}

int hl_jv(int manifold, const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, const double* a0,
          const double* a1, const double* b0, const double* b1, double* u, double* w) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[8], p1[8], pm[8];
    if (manifold == 1) { prepare3<Se2Manifold>(k0, k1, m, p0, p1, pm); Se2Manifold::edge_jv(p0, p1, pm, l, a0, a1, b0, b1, u, w); }
    else { prepare3<Se3Manifold>(k0, k1, m, p0, p1, pm); Se3Manifold::edge_jv(p0, p1, pm, l, a0, a1, b0, b1, u, w); }
    return 0;
}

// |r~|^2 = residual_scaling^2 s as k_pg_cost_partial<M, LossGeneral> forms it: M::residual, s summed left to right
int hl_cost(int manifold, const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, double* out) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[8], p1[8], pm[8], r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (manifold == 1) { prepare3<Se2Manifold>(k0, k1, m, p0, p1, pm); Se2Manifold::residual(p0, p1, pm, r); }
    else { prepare3<Se3Manifold>(k0, k1, m, p0, p1, pm); Se3Manifold::residual(p0, p1, pm, r); }
    double s = 0.0;
    for (int i = 0; i < (manifold == 1 ? 3 : 6); ++i) s += r[i] * r[i];
    const double sc = pg_loss_corrector(l, s).residual_scaling;
    *out = (sc * sc) * s;
    return 0;
}

}  // extern "C"

#ifdef HL_MAIN
// every kind on the grid of squared norms the test uses, then every per-edge entry point on pseudo-random edges of both manifolds
int main() {
    const double params[kLossKindCount][2] = {{0, 0}, {0, 0}, {0, 0}, {1.345, 0}, {2.3849, 0}, {1.3999, 0}, {1.0, 0}, {2.9846, 0},
                                              {4.6851, 0}, {1.339, 0}, {0.3, 0}, {2.0, 0}, {3.0, 0}, {1.0, 1.0}, {5.0, 0}};
    double sum = 0.0;
    long n = 0;
    for (int k = 0; k < kLossKindCount; ++k) {
        const double c = params[k][0] > 0 ? params[k][0] : 1.0;
        const double pts[] = {0.0, 1e-300, 1e-17, 2.2e-16, 2.3e-16, c * c * (1 - 1e-9), c * c, c * c * (1 + 1e-9),
                              M_PI * M_PI * c * c * (1 - 1e-9), M_PI * M_PI * c * c * (1 + 1e-9), M_PI * M_PI * c * c / 4};
        double out[6];
        for (double s : pts) { if (hl_loss(k, params[k][0], params[k][1], s, out) != 0) return 2; for (double v : out) if (v == v) sum += v; ++n; }
        for (int e = -12; e <= 6; ++e)
            for (int j = 1; j < 10; j += 3) { hl_loss(k, params[k][0], params[k][1], j * pow(10.0, e), out); for (double v : out) if (v == v) sum += v; ++n; }
    }
    if (hl_loss(8, -1.0, 0, 1.0, &sum) != -1 || hl_loss(99, 1.0, 0, 1.0, &sum) != -1) return 3;
    uint64_t st = 12345;
    auto rnd = [&] { st = st * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(st >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
    for (int it = 0; it < 200; ++it)
        for (int man = 0; man < 2; ++man)
            for (int k = 1; k < kLossKindCount; ++k) {
                double q[3][7];
                for (auto& p : q) { for (double& v : p) v = rnd(); if (man == 0) { p[0] *= 3; p[1] *= 3; p[2] *= 3; } }
                const int D = man ? 3 : 6;
                double r[6], J[72], Haa[36], Hbb[36], Hba[36], ga[6], gb[6], a0[6], a1[6], b0[6], b1[6], u[6], w[6];
                for (int i = 0; i < 6; ++i) { a0[i] = rnd(); a1[i] = rnd(); b0[i] = rnd(); b1[i] = rnd(); }
                hl_edge(man, q[0], q[1], q[2], k, params[k][0], params[k][1], r, J);
                hl_blocks(man, q[0], q[1], q[2], k, params[k][0], params[k][1], it % 7 == 0, Haa, Hbb, Hba, ga, gb);
                hl_jv(man, q[0], q[1], q[2], k, params[k][0], params[k][1], a0, a1, b0, b1, u, w);
                for (int i = 0; i < D; ++i) sum += r[i] + ga[i] + gb[i] + u[i] + w[i] + Haa[i * D + i] + Hbb[i * D + i] + Hba[i] + J[i];
                ++n;
            }
    printf("host_harness_loss: %ld evaluations, checksum %.17g\n", n, sum);
    return 0;
}
#endif
