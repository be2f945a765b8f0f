// host_harness_info.cpp -- the edge-information paths of pg_device.hpp / pg2_device.hpp compiled for the host,
// for tests/test_info_device_math_host.py (shared library) and, with -DHI_MAIN, as a stand-alone program that walks the same
// code over pseudo-random edges (the build that runs under -fsanitize=address,undefined).
//
// Poses and measurements come in stored form (SE3: t, qw qx qy qz; SE2: x y theta) and are prepared here as k_pg_prepare and
// set_structure do; W is Omega, full, row-major D x D.  Every result is in the form the kernels use:
//   hi_edge    M::export_edge_info   the literal whitened, corrected residual and Jacobian [dr/dk0 | dr/dk1]
//   hi_blocks  SE3: the body of k_pg_edges<LossWeighted> (pg_edge_weighted), SE2: pg2_assemble_row_info on the graph that holds
//              just this edge.  order 0: from < to, 1: from > to, 2: self-loop.  H_ff, H_tt (f = from, t = to), the cross block
//              of row vertex max(from, to) and column vertex min(from, to), g_f, g_t; a self-loop puts everything on H_ff, g_f.
//   hi_jv      M::edge_jv_info closed with Omega as k_pg_jv_gram does: out3 = {(J~ a).(J~ a), (J~ a).(J~ b), (J~ b).(J~ b)}
//   hi_cost    M::residual and info_sqnorm as k_pg_cost_partial does: |r~|^2
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

void add36(double* dst, const double* H) { for (int i = 0; i < 36; ++i) dst[i] += H[i]; }

// a, b: the vertex numbers of from and to
void se3_blocks(const double* k0, const double* k1, const double* m, const PgLoss& loss, const double* W, uint32_t a, uint32_t b,
                double* Hff, double* Htt, double* Hx, double* gf, double* gt) {
    double r[6], M[36], H[36], gv[6];
    Jac6 J0, J1;
    EdgeNormal6 nf;
    memset(Hff, 0, 36 * sizeof(double)); memset(Htt, 0, 36 * sizeof(double)); memset(Hx, 0, 36 * sizeof(double));
    memset(gf, 0, 6 * sizeof(double)); memset(gt, 0, 6 * sizeof(double));
    if (!between_linearize_weighted(k0, k1, m, loss, W, r, J0, J1, nf)) return;
    info_mul_jac(W, J0, M);
    jt_mul(J0, M, H); nf.correct(H, nf.w0, nf.w0); add36(Hff, H);
    if (a < b) { jt_mul(J1, M, H); nf.correct(H, nf.w1, nf.w0); add36(Hx, H); }
    info_mul_jac(W, J1, M);
    jt_mul(J1, M, H); nf.correct(H, nf.w1, nf.w1); add36(a == b ? Hff : Htt, H);
    if (a > b) { jt_mul(J0, M, H); nf.correct(H, nf.w0, nf.w1); add36(Hx, H); }
    else if (a == b) {
        jt_mul(J0, M, H); nf.correct(H, nf.w0, nf.w1);
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) Hff[6 * i + j] += H[6 * i + j] + H[6 * j + i];
    }
    nf.grad(nf.w0, gv);
    for (int i = 0; i < 6; ++i) gf[i] += gv[i];
    nf.grad(nf.w1, gv);
    for (int i = 0; i < 6; ++i) (a == b ? gf : gt)[i] += gv[i];
}

void se2_blocks(const double* p0, const double* p1, const double* pm, const PgLoss& loss, const double* W, uint32_t a, uint32_t b,
                double* Hff, double* Htt, double* Hx, double* gf, double* gt) {
    double posep[2 * kPose2Stride], info[InfoPack<3>::kStride];
    memcpy(posep + kPose2Stride * a, p0, sizeof(double) * kPose2Stride);
    if (a != b) memcpy(posep + kPose2Stride * b, p1, sizeof(double) * kPose2Stride);
    int k = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) info[k++] = W[3 * i + j];
    const uint32_t e_from[1] = {a}, e_to[1] = {b}, inc_edge[2] = {0, 0};
    const int inc_ptr[3] = {0, 1, 2};
    memset(Htt, 0, 9 * sizeof(double)); memset(Hx, 0, 9 * sizeof(double)); memset(gt, 0, 3 * sizeof(double));
    const auto off = [&](uint32_t, const double* B) { for (int i = 0; i < 9; ++i) Hx[i] += B[i]; };
    pg2_assemble_row_info(a, posep, pm, e_from, e_to, inc_ptr, inc_edge, info, loss, Hff, gf, off);
    if (a != b) pg2_assemble_row_info(b, posep, pm, e_from, e_to, inc_ptr, inc_edge, info, loss, Htt, gt, off);
}

template <class M>
void jv(const double* p0, const double* p1, const double* pm, const PgLoss& l, const double* W, const double* a0, const double* a1,
        const double* b0, const double* b1, double* out3) {
    constexpr int D = M::kDof;
    double u[D], w[D], Wu[D], Ww[D];
    M::edge_jv_info(p0, p1, pm, l, W, a0, a1, b0, b1, u, w);
    info_mv<D>(W, u, Wu);
    info_mv<D>(W, w, Ww);
    out3[0] = dotn<D>(u, Wu); out3[1] = dotn<D>(u, Ww); out3[2] = dotn<D>(w, Ww);
}

template <class M>
double cost(const double* p0, const double* p1, const double* pm, const PgLoss& l, const double* W) {
    double r[M::kDof];
    M::residual(p0, p1, pm, r);
    const double s = info_sqnorm<M::kDof>(W, r);
    const double sc = pg_loss_corrector(l, s).residual_scaling;
    return (sc * sc) * s;
}

}  // namespace

extern "C" {

int hi_edge(int manifold, const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, const double* W,
            double* r, double* J) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[8], p1[8], pm[8];
    if (manifold == 1) { prepare3<Se2Manifold>(k0, k1, m, p0, p1, pm); Se2Manifold::export_edge_info(p0, p1, pm, l, W, r, J); }
    else { prepare3<Se3Manifold>(k0, k1, m, p0, p1, pm); Se3Manifold::export_edge_info(p0, p1, pm, l, W, r, J); }
    return 0;
}

int hi_blocks(int manifold, const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, const double* W,
              int order, double* Hff, double* Htt, double* Hx, double* gf, double* gt) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l) || order < 0 || order > 2) return -1;
    const uint32_t a = order == 1 ? 1u : 0u, b = order == 0 ? 1u : 0u;
    double p0[8], p1[8], pm[8];
    if (manifold == 1) { prepare3<Se2Manifold>(k0, order == 2 ? k0 : k1, m, p0, p1, pm); se2_blocks(p0, p1, pm, l, W, a, b, Hff, Htt, Hx, gf, gt); }
    else { prepare3<Se3Manifold>(k0, order == 2 ? k0 : k1, m, p0, p1, pm); se3_blocks(p0, p1, pm, l, W, a, b, Hff, Htt, Hx, gf, gt); }
    return 0;
}

int hi_jv(int manifold, const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, const double* W,
          const double* a0, const double* a1, const double* b0, const double* b1, double* out3) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[8], p1[8], pm[8];
    if (manifold == 1) { prepare3<Se2Manifold>(k0, k1, m, p0, p1, pm); jv<Se2Manifold>(p0, p1, pm, l, W, a0, a1, b0, b1, out3); }
    else { prepare3<Se3Manifold>(k0, k1, m, p0, p1, pm); jv<Se3Manifold>(p0, p1, pm, l, W, a0, a1, b0, b1, out3); }
    return 0;
}

int hi_cost(int manifold, const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, const double* W,
            double* out) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[8], p1[8], pm[8];
    if (manifold == 1) { prepare3<Se2Manifold>(k0, k1, m, p0, p1, pm); *out = cost<Se2Manifold>(p0, p1, pm, l, W); }
    else { prepare3<Se3Manifold>(k0, k1, m, p0, p1, pm); *out = cost<Se3Manifold>(p0, p1, pm, l, W); }
    return 0;
}

}  // extern "C"

#ifdef HI_MAIN
// every entry point on pseudo-random edges of both manifolds, every loss kind, all three vertex orders, random SPD Omega
int main() {
    const double params[kLossKindCount][2] = {{0, 0}, {0, 0}, {0, 0}, {1.345, 0}, {2.3849, 0}, {1.3999, 0}, {1.0, 0}, {2.9846, 0},
                                              {4.6851, 0}, {1.339, 0}, {0.3, 0}, {2.0, 0}, {3.0, 0}, {1.0, 1.0}, {5.0, 0}};
    uint64_t st = 2468;
    auto rnd = [&] { st = st * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(st >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
    double sum = 0.0;
    long n = 0;
    for (int it = 0; it < 150; ++it)
        for (int man = 0; man < 2; ++man)
            for (int k = 0; k < kLossKindCount; ++k) {
                const int D = man ? 3 : 6;
                double q[3][7];
                for (auto& p : q) { for (double& v : p) v = rnd(); if (man == 0) { p[0] *= 3; p[1] *= 3; p[2] *= 3; } }
                double A[36], W[36];
                for (int i = 0; i < D * D; ++i) A[i] = rnd();
                for (int i = 0; i < D; ++i)
                    for (int j = 0; j < D; ++j) {
                        double acc = i == j ? 0.5 : 0.0;
                        for (int c = 0; c < D; ++c) acc += A[D * i + c] * A[D * j + c];
                        W[D * i + j] = acc;
                    }
                double r[6], J[72], Hff[36], Htt[36], Hx[36], gf[6], gt[6], a0[6], a1[6], b0[6], b1[6], o3[3], c = 0.0;
                for (int i = 0; i < 6; ++i) { a0[i] = rnd(); a1[i] = rnd(); b0[i] = rnd(); b1[i] = rnd(); }
                if (hi_edge(man, q[0], q[1], q[2], k, params[k][0], params[k][1], W, r, J) != 0) return 2;
                if (hi_blocks(man, q[0], q[1], q[2], k, params[k][0], params[k][1], W, it % 3, Hff, Htt, Hx, gf, gt) != 0) return 2;
                if (hi_jv(man, q[0], q[1], q[2], k, params[k][0], params[k][1], W, a0, a1, b0, b1, o3) != 0) return 2;
                if (hi_cost(man, q[0], q[1], q[2], k, params[k][0], params[k][1], W, &c) != 0) return 2;
                for (int i = 0; i < D; ++i) sum += r[i] + gf[i] + gt[i] + Hff[i * D + i] + Htt[i * D + i] + Hx[i] + J[i];
                sum += o3[0] + o3[1] + o3[2] + c;
                ++n;
            }
    if (!(sum == sum)) return 3;
    printf("host_harness_info: %ld edges, checksum %.17g\n", n, sum);
    return 0;
}
#endif
