// Host build of the SE2 device math (apex-solver_amd/csrc/pg2_device.hpp) and of the incident-edge lists
// (pg2_lists.h) for the CPU tests: g++ -O2 -ffp-contract=off, no hipcc.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "pg2_device.hpp"
#include "pg2_lists.h"

using namespace apex;

extern "C" {

void hh2_between_linearize(const double* k0, const double* k1, const double* m, double delta, double* r, double* J /* 3 x 6 */) {
    double p0[4], p1[4], pm[4], J0[9], J1[9];
    se2_prepare(k0, p0); se2_prepare(k1, p1); se2_prepare(m, pm);
    between2_corrected(p0, p1, pm, delta, r, J0, J1);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { J[6 * i + j] = J0[3 * i + j]; J[6 * i + 3 + j] = J1[3 * i + j]; }
}

void hh2_between_normal(const double* k0, const double* k1, const double* m, double* H00, double* H11, double* H10, double* g0, double* g1) {
    double p0[4], p1[4], pm[4], r[3], J0[9], J1[9];
    se2_prepare(k0, p0); se2_prepare(k1, p1); se2_prepare(m, pm);
    between2_linearize(p0, p1, pm, r, J0, J1);
    memset(H00, 0, 72); memset(H11, 0, 72); memset(H10, 0, 72); memset(g0, 0, 24); memset(g1, 0, 24);
    jtj3_acc(J0, J0, H00); jtj3_acc(J1, J1, H11); jtj3_acc(J1, J0, H10);
    jtr3_acc(J0, r, g0); jtr3_acc(J1, r, g1);
}

void hh2_exp(const double* t, double* v3) { double p[4]; se2_exp(t, p); v3[0] = p[0]; v3[1] = p[1]; v3[2] = se2_angle(p); }
void hh2_log(const double* v3, double* t) { double p[4]; se2_prepare(v3, p); se2_log(p, t); }
void hh2_plus(const double* v3, const double* d, double* o3) { se2_plus(v3, d, o3); }
double hh2_wrap(double th) { return se2_wrap_angle(th); }
void hh2_right_jacobians(const double* t, double* Jr, double* Jrinv) { se2_right_jacobian(t, Jr); se2_right_jacobian_inv(t, Jrinv); }

// ptr_out[n_v + 1], edge_out[2 n_e]; returns the list length, -1 on a bad endpoint
int64_t hh2_lists(int64_t n_v, int64_t n_e, const uint32_t* ef, const uint32_t* et, int* ptr_out, uint32_t* edge_out) {
    IncidentLists inc;
    if (!build_incident_lists(n_v, n_e, ef, et, &inc)) return -1;
    memcpy(ptr_out, inc.ptr.data(), inc.ptr.size() * sizeof(int));
    if (!inc.edge.empty()) memcpy(edge_out, inc.edge.data(), inc.edge.size() * sizeof(uint32_t));
    return (int64_t)inc.edge.size();
}

// the loop of k_pg2_assemble over every vertex, into a dense lower-triangular H [3 n_v]^2 and g; `writes` [n_v]^2 counts
// the read-add-writes per block (row vertex, column vertex) and `writer` records which row's owner made them
int hh2_assemble_dense(int64_t n_v, int64_t n_e, const double* poses3, const uint32_t* ef, const uint32_t* et, const double* meas3,
                       double delta, double* H, double* g, int* writes, int* writer) {
    IncidentLists inc;
    if (!build_incident_lists(n_v, n_e, ef, et, &inc)) return -1;
    std::vector<double> pp(4 * (size_t)n_v), mp(4 * (size_t)n_e);
    for (int64_t v = 0; v < n_v; ++v) se2_prepare(poses3 + 3 * v, pp.data() + 4 * v);
    for (int64_t e = 0; e < n_e; ++e) se2_prepare(meas3 + 3 * e, mp.data() + 4 * e);
    const size_t n = 3 * (size_t)n_v;
    for (uint32_t v = 0; v < (uint32_t)n_v; ++v) {
        double Hvv[9], gv[3];
        pg2_assemble_row(v, pp.data(), mp.data(), ef, et, inc.ptr.data(), inc.edge.data(), delta, Hvv, gv,
                         [&](uint32_t u, const double* B) {
                             for (int a = 0; a < 3; ++a)
                                 for (int b = 0; b < 3; ++b) H[(3 * (size_t)v + a) * n + 3 * (size_t)u + b] += B[3 * a + b];
                             writes[(size_t)v * n_v + u]++;
                             writer[(size_t)v * n_v + u] = (int)v;
                         });
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b <= a; ++b) H[(3 * (size_t)v + a) * n + 3 * (size_t)v + b] += Hvv[3 * a + b];
            g[3 * (size_t)v + a] = gv[a];
        }
    }
    return 0;
}

}  // extern "C"
