// Host build of the SO3 device math (apex-solver_amd/csrc/pg_so3_device.hpp) and of the row-owned assembly over the
// incident-edge lists (pg2_device.hpp, pg2_lists.h) for the CPU tests: g++ -O2 -ffp-contract=off, no hipcc.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "pg2_lists.h"
#include "pg_so3_device.hpp"

using namespace apex;

extern "C" {

void hs3_prepare(const double* q4, double* o4) { So3Manifold::prepare(q4, o4); }
// the SE3 preparation of [0, 0, 0, q]: its quaternion must have the bits of hs3_prepare's
void hs3_prepare_as_se3(const double* q4, double* o4) {
    double v[7] = {0.0, 0.0, 0.0, q4[0], q4[1], q4[2], q4[3]}, o[7];
    pose_normalise(v, o);
    memcpy(o4, o + 3, 4 * sizeof(double));
}

// r [3], J [3][6] = [dr/dk0 | dr/dk1] under set_structure's Huber delta (<= 0: none); inputs as stored (not normalised)
void hs3_between_linearize(const double* k0, const double* k1, const double* m, double delta, double* r, double* J) {
    double p0[4], p1[4], pm[4];
    So3Manifold::prepare(k0, p0); So3Manifold::prepare(k1, p1); So3Manifold::prepare(m, pm);
    So3Manifold::export_edge(p0, p1, pm, delta, r, J);
}
void hs3_residual(const double* k0, const double* k1, const double* m, double* r) {
    double p0[4], p1[4], pm[4];
    So3Manifold::prepare(k0, p0); So3Manifold::prepare(k1, p1); So3Manifold::prepare(m, pm);
    So3Manifold::residual(p0, p1, pm, r);
}
void hs3_log(const double* q4, double* t) { double p[4]; So3Manifold::prepare(q4, p); so3_log(p, t); }
void hs3_exp(const double* t, double* q4) { so3_exp(t, q4); }
void hs3_plus(const double* q4, const double* d, double* o4) { So3Manifold::plus(q4, d, o4); }
void hs3_right_jacobian_inv(const double* t, double* J) {
    double Jl[9];
    so3_left_jacobian_inv(t, Jl);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) J[3 * i + j] = Jl[3 * j + i];
}
// corrected prior residual [4] of a stored vertex against data; returns sqrt(rho')
double hs3_prior(const double* q4, const double* data4, double delta, double* r4) {
    double p[4];
    So3Manifold::prepare(q4, p);
    return So3Manifold::prior_residual(p, data4, delta, r4);
}

// The loop of k_pg2_assemble<So3Manifold, *> over every vertex, into a dense lower-triangular H [3 n_v]^2 and g.  kind / p0 / p1:
// a loss of pg_loss.hpp (kind 0 with delta: the legacy Huber path); info: [n_e][9] full matrices or null.  `writes` [n_v]^2 counts
// the read-add-writes per block (row vertex, column vertex), `writer` records which row's owner made them.  Returns 0, -1 on a bad endpoint or loss.
int hs3_assemble_dense(int64_t n_v, int64_t n_e, const double* poses4, const uint32_t* ef, const uint32_t* et, const double* meas4,
                       int kind, double p0, double p1, double delta, const double* info, double* H, double* g, int* writes, int* writer) {
    IncidentLists inc;
    if (!build_incident_lists(n_v, n_e, ef, et, &inc)) return -1;
    PgLoss loss;
    if (!pg_loss_make(kind, p0, p1, &loss)) return -1;
    if (info && kind == kLossNone && delta > 0.0 && !pg_loss_make(kLossHuber, delta, 0.0, &loss)) return -1;
    std::vector<double> pp(4 * (size_t)n_v), mp(4 * (size_t)n_e), packed;
    for (int64_t v = 0; v < n_v; ++v) So3Manifold::prepare(poses4 + 4 * v, pp.data() + 4 * v);
    for (int64_t e = 0; e < n_e; ++e) So3Manifold::prepare(meas4 + 4 * e, mp.data() + 4 * e);
    if (info) {
        packed.assign((size_t)n_e * InfoPack<3>::kStride, 0.0);
        for (int64_t e = 0; e < n_e; ++e) {
            double* p = packed.data() + (size_t)e * InfoPack<3>::kStride;
            for (int i = 0; i < 3; ++i)
                for (int j = i; j < 3; ++j) *p++ = info[9 * e + 3 * i + j];
        }
    }
    const size_t n = 3 * (size_t)n_v;
    for (uint32_t v = 0; v < (uint32_t)n_v; ++v) {
        double Hvv[9], gv[3];
        auto off = [&](uint32_t u, const double* B) {
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) H[(3 * (size_t)v + a) * n + 3 * (size_t)u + b] += B[3 * a + b];
            writes[(size_t)v * n_v + u]++;
            writer[(size_t)v * n_v + u] = (int)v;
        };
        if (info)
            pg_row_assemble_info<So3Manifold>(v, pp.data(), mp.data(), ef, et, inc.ptr.data(), inc.edge.data(), packed.data(), loss, Hvv, gv, off);
        else if (kind == kLossNone)
            pg_row_assemble<So3Manifold>(v, pp.data(), mp.data(), ef, et, inc.ptr.data(), inc.edge.data(), delta, Hvv, gv, off);
        else
            pg_row_assemble<So3Manifold>(v, pp.data(), mp.data(), ef, et, inc.ptr.data(), inc.edge.data(), loss, Hvv, gv, off);
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b <= a; ++b) H[(3 * (size_t)v + a) * n + 3 * (size_t)v + b] += Hvv[3 * a + b];
            g[3 * (size_t)v + a] = gv[a];
        }
    }
    return 0;
}

// The per-edge forms under a loss of pg_loss.hpp, with Omega (info9: full, row-major) or without (null), as the kernels call them:
//   hs3_edge  k_pg_export     the literal corrected (whitened) residual [3] and Jacobian [3][6]
//   hs3_jv    k_pg_jv_gram    out3 = {(J~ a).(J~ a), (J~ a).(J~ b), (J~ b).(J~ b)}, closed with Omega where there is one
//   hs3_cost  k_pg_cost_partial  |r~|^2 = residual_scaling^2 s
// 0, or -1 where the loss is refused.
int hs3_edge(const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, const double* info9, double* r, double* J) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[4], p1[4], pm[4];
    So3Manifold::prepare(k0, p0); So3Manifold::prepare(k1, p1); So3Manifold::prepare(m, pm);
    if (info9) So3Manifold::export_edge_info(p0, p1, pm, l, info9, r, J);
    else So3Manifold::export_edge(p0, p1, pm, l, r, J);
    return 0;
}
int hs3_jv(const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, const double* info9, const double* a0,
           const double* a1, const double* b0, const double* b1, double* out3) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[4], p1[4], pm[4], u[3], w[3], Wu[3], Ww[3];
    So3Manifold::prepare(k0, p0); So3Manifold::prepare(k1, p1); So3Manifold::prepare(m, pm);
    if (info9) {
        So3Manifold::edge_jv_info(p0, p1, pm, l, info9, a0, a1, b0, b1, u, w);
        info_mv<3>(info9, u, Wu); info_mv<3>(info9, w, Ww);
    } else {
        So3Manifold::edge_jv(p0, p1, pm, l, a0, a1, b0, b1, u, w);
        for (int i = 0; i < 3; ++i) { Wu[i] = u[i]; Ww[i] = w[i]; }
    }
    out3[0] = dotn<3>(u, Wu); out3[1] = dotn<3>(u, Ww); out3[2] = dotn<3>(w, Ww);
    return 0;
}
int hs3_cost(const double* k0, const double* k1, const double* m, int kind, double lp0, double lp1, const double* info9, double* out) {
    PgLoss l;
    if (!pg_loss_make(kind, lp0, lp1, &l)) return -1;
    double p0[4], p1[4], pm[4], r[3];
    So3Manifold::prepare(k0, p0); So3Manifold::prepare(k1, p1); So3Manifold::prepare(m, pm);
    So3Manifold::residual(p0, p1, pm, r);
    const double s = info9 ? info_sqnorm<3>(info9, r) : (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    const double sc = pg_loss_corrector(l, s).residual_scaling;
    *out = (sc * sc) * s;
    return 0;
}

// the incident list of vertex v (ascending edge index, a self-loop once): the order in which its diagonal block is summed
int64_t hs3_incident(int64_t n_v, int64_t n_e, const uint32_t* ef, const uint32_t* et, int64_t v, uint32_t* out) {
    IncidentLists inc;
    if (!build_incident_lists(n_v, n_e, ef, et, &inc)) return -1;
    const int64_t n = inc.ptr[v + 1] - inc.ptr[v];
    for (int64_t k = 0; k < n; ++k) out[k] = inc.edge[inc.ptr[v] + k];
    return n;
}

}  // extern "C"
