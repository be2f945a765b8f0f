// Host build of the row-owned SE3 assembly (pg_row_assemble6 of apex-solver_amd/csrc/pg_device.hpp) over the incident-edge
// lists of pg2_lists.h for the CPU tests: g++ -O2 -ffp-contract=off, no hipcc.  With -DHS6_MAIN it is a program of its own
// (a small graph with parallel edges, a self-loop, a hub and an isolated vertex under the three policies), which is the
// form to build with -fsanitize=address,undefined.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "pg2_lists.h"
#include "pg_device.hpp"

using namespace apex;

namespace {
// The policy a handle's view selects (PoseGraphSolver::view, with_loss): weighted when information is given (every loss as a
// PgLoss), else the huber_delta instantiation for no loss / L2 / Huber and the general one for the rest.  0 legacy, 1 general,
// 2 weighted; -1: the loss is refused.
int pick_policy(int kind, double p0, double p1, double delta, bool info, PgLoss* loss, double* huber) {
    *huber = delta;
    *loss = PgLoss{};
    if (kind != kLossNone && !pg_loss_make(kind, p0, p1, loss)) return -1;
    if (info) {
        if (kind == kLossNone && delta > 0.0 && !pg_loss_make(kLossHuber, delta, 0.0, loss)) return -1;
        return 2;
    }
    if (kind == kLossNone) return 0;
    if (kind == kLossL2) { *huber = -1.0; return 0; }
    if (kind == kLossHuber) { *huber = p0; return 0; }
    return 1;
}
}  // namespace

extern "C" {

// The loop of k_pg6_assemble<LP> over every vertex and of k_pg2_priors<Se3Manifold> over the prior blocks, into a dense
// lower-triangular H [6 n_v]^2 (lam on the diagonal first, as add_diag leaves it) and g.  kind / p0 / p1: a loss of
// pg_loss.hpp (kind 0 with delta: set_structure's Huber delta); info: [n_e][36] full matrices or null.  Priors: vertex,
// data [7], delta per block in the caller's order; pres_out [n_prior][7] and psc_out [n_prior] come back in that order.
// r_out [n_e][6], j_out [n_e][6][12]: the corrected (whitened) blocks as the handle's exports give them.  `writes` [n_v]^2 counts
// the read-add-writes per block (row vertex, column vertex), `writer` records which row's owner made them.
// Returns the policy that ran (0 legacy, 1 general, 2 weighted), -1 on a bad endpoint or loss.
int hs6_assemble_dense(int64_t n_v, int64_t n_e, const double* poses7, const uint32_t* ef, const uint32_t* et, const double* meas7,
                       int kind, double p0, double p1, double delta, const double* info, double lam, int64_t n_prior,
                       const uint32_t* prior_v, const double* prior_data7, const double* prior_delta, double* H, double* g,
                       int* writes, int* writer, double* r_out, double* j_out, double* pres_out, double* psc_out) {
    IncidentLists inc;
    if (!build_incident_lists(n_v, n_e, ef, et, &inc)) return -1;
    PgLoss loss;
    double huber;
    const int policy = pick_policy(kind, p0, p1, delta, info != nullptr, &loss, &huber);
    if (policy < 0) return -1;
    std::vector<double> pp(8 * (size_t)n_v, 0.0), mp(8 * (size_t)n_e, 0.0), packed;
    for (int64_t v = 0; v < n_v; ++v) pose_normalise(poses7 + 7 * v, pp.data() + 8 * v);
    for (int64_t e = 0; e < n_e; ++e) pose_normalise(meas7 + 7 * e, mp.data() + 8 * e);
    if (info) {
        packed.assign((size_t)n_e * InfoPack<6>::kStride, 0.0);
        for (int64_t e = 0; e < n_e; ++e) {
            double* p = packed.data() + (size_t)e * InfoPack<6>::kStride;
            for (int i = 0; i < 6; ++i)
                for (int j = i; j < 6; ++j) *p++ = info[36 * e + 6 * i + j];
        }
    }
    const size_t n = 6 * (size_t)n_v;
    for (size_t i = 0; i < n; ++i) H[i * n + i] = lam;
    for (uint32_t v = 0; v < (uint32_t)n_v; ++v) {
        double Hvv[36], gv[6];
        auto off = [&](uint32_t u, const double* B) {
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b < 6; ++b) H[(6 * (size_t)v + a) * n + 6 * (size_t)u + b] += B[6 * a + b];
            writes[(size_t)v * n_v + u]++;
            writer[(size_t)v * n_v + u] = (int)v;
        };
        if (policy == 2)
            pg_row_assemble6<LossWeighted>(v, pp.data(), mp.data(), ef, et, inc.ptr.data(), inc.edge.data(), packed.data(), loss, Hvv, gv, off);
        else if (policy == 1)
            pg_row_assemble6<LossGeneral>(v, pp.data(), mp.data(), ef, et, inc.ptr.data(), inc.edge.data(), nullptr, loss, Hvv, gv, off);
        else
            pg_row_assemble6<LossLegacy>(v, pp.data(), mp.data(), ef, et, inc.ptr.data(), inc.edge.data(), nullptr, huber, Hvv, gv, off);
        for (int a = 0; a < 6; ++a) {
            for (int b = 0; b <= a; ++b) H[(6 * (size_t)v + a) * n + 6 * (size_t)v + b] += Hvv[6 * a + b];
            g[6 * (size_t)v + a] = gv[a];
        }
    }
    // priors: sorted by vertex (stable), the first block of a vertex sums the whole run in order (k_pg2_priors)
    std::vector<int> order((size_t)n_prior);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return prior_v[a] < prior_v[b]; });
    for (int64_t k = 0; k < n_prior; ++k) {
        const uint32_t a = prior_v[order[k]];
        if (a >= (uint64_t)n_v) return -1;
        if (k > 0 && prior_v[order[k - 1]] == a) continue;
        double h = 0.0, gv[6] = {};
        for (int64_t j = k; j < n_prior && prior_v[order[j]] == a; ++j) {
            const int src = order[j];
            double r[7];
            const double sc = prior_eval(pp.data() + 8 * (size_t)a, prior_data7 + 7 * (size_t)src, prior_delta[src], r);
            h += sc * sc;
            for (int i = 0; i < 6; ++i) gv[i] += sc * r[i];
            if (pres_out) memcpy(pres_out + 7 * (size_t)src, r, sizeof r);
            if (psc_out) psc_out[src] = sc;
        }
        for (int i = 0; i < 6; ++i) {
            H[(6 * (size_t)a + i) * n + 6 * (size_t)a + i] += h;
            g[6 * (size_t)a + i] += gv[i];
        }
    }
    for (int64_t e = 0; e < n_e; ++e) {
        const double *k0 = pp.data() + 8 * (size_t)ef[e], *k1 = pp.data() + 8 * (size_t)et[e], *m = mp.data() + 8 * (size_t)e;
        double* ro = r_out ? r_out + 6 * e : nullptr;
        double* jo = j_out ? j_out + 72 * e : nullptr;
        if (policy == 2) {
            double W[36];
            info_unpack<6>(packed.data() + (size_t)e * InfoPack<6>::kStride, W);
            Se3Manifold::export_edge_info(k0, k1, m, loss, W, ro, jo);
        } else if (policy == 1) {
            Se3Manifold::export_edge(k0, k1, m, loss, ro, jo);
        } else {
            Se3Manifold::export_edge(k0, k1, m, huber, ro, jo);
        }
    }
    return policy;
}

// the incident list of vertex v (ascending edge index, a self-loop once): the order in which its diagonal block is summed
int64_t hs6_incident(int64_t n_v, int64_t n_e, const uint32_t* ef, const uint32_t* et, int64_t v, uint32_t* out) {
    IncidentLists inc;
    if (!build_incident_lists(n_v, n_e, ef, et, &inc)) return -1;
    const int64_t n = inc.ptr[v + 1] - inc.ptr[v];
    for (int64_t k = 0; k < n; ++k) out[k] = inc.edge[inc.ptr[v] + k];
    return n;
}

}  // extern "C"

#ifdef HS6_MAIN
// A program of its own: every policy on one small graph; the dense result must be finite, strictly lower-triangular plus
// diagonal, and equal on a second pass.
int main() {
    const int64_t n_v = 9;
    std::vector<uint32_t> ef, et;
    for (uint32_t v = 0; v + 2 < n_v; ++v) { ef.push_back(v); et.push_back(v + 1); }   // a chain over 0..7 (8 stays isolated)
    for (int k = 0; k < 5; ++k) { ef.push_back(k % 2 ? 6u : 1u); et.push_back(k % 2 ? 1u : 6u); }   // parallel edges, both directions
    ef.push_back(3); et.push_back(3);                                                    // a self-loop
    for (uint32_t v = 1; v < 8; ++v) { ef.push_back(v % 2 ? 0u : v); et.push_back(v % 2 ? v : 0u); }   // a hub at 0
    const int64_t n_e = (int64_t)ef.size();
    uint64_t st = 88172645463325252ULL;
    auto rnd = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) / 9007199254740992.0 - 0.5; };
    auto pose = [&](double* p) { for (int i = 0; i < 3; ++i) p[i] = 2.0 * rnd(); p[3] = 1.0; for (int i = 4; i < 7; ++i) p[i] = 0.4 * rnd(); };
    std::vector<double> poses(7 * n_v), meas(7 * n_e), info(36 * n_e, 0.0);
    for (int64_t v = 0; v < n_v; ++v) pose(poses.data() + 7 * v);
    for (int64_t e = 0; e < n_e; ++e) {
        pose(meas.data() + 7 * e);
        double A[36];
        for (double& x : A) x = rnd();
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) {
                double acc = i == j ? 1.0 : 0.0;
                for (int k = 0; k < 6; ++k) acc += A[6 * k + i] * A[6 * k + j];
                info[36 * e + 6 * i + j] = acc;
            }
    }
    const uint32_t pv[4] = {7, 2, 7, 0};
    std::vector<double> pdata(7 * 4);
    for (int k = 0; k < 4; ++k) { pose(pdata.data() + 7 * k); }
    const double pdelta[4] = {-1.0, 0.05, 1e3, 0.05};
    const size_t n = 6 * (size_t)n_v;
    int failures = 0;
    struct Run { int kind; double p0, delta; bool info; int want; };
    const Run runs[] = {{kLossNone, 0.0, -1.0, false, 0}, {kLossNone, 0.0, 0.7, false, 0}, {kLossCauchy, 1.0, -1.0, false, 1},
                        {kLossTukey, 1.5, -1.0, false, 1}, {kLossCauchy, 1.0, -1.0, true, 2}, {kLossNone, 0.0, 0.7, true, 2}};
    for (const Run& q : runs) {
        std::vector<double> H[2], g[2];
        for (int pass = 0; pass < 2; ++pass) {
            H[pass].assign(n * n, 0.0); g[pass].assign(n, 0.0);
            std::vector<int> writes((size_t)n_v * n_v, 0), writer((size_t)n_v * n_v, -1);
            std::vector<double> r(6 * n_e), J(72 * n_e), pres(7 * 4), psc(4);
            const int rc = hs6_assemble_dense(n_v, n_e, poses.data(), ef.data(), et.data(), meas.data(), q.kind, q.p0, 0.0, q.delta,
                                              q.info ? info.data() : nullptr, 0.5, 4, pv, pdata.data(), pdelta, H[pass].data(), g[pass].data(),
                                              writes.data(), writer.data(), r.data(), J.data(), pres.data(), psc.data());
            if (rc != q.want) { printf("policy %d, wanted %d\n", rc, q.want); ++failures; }
            for (size_t i = 0; i < n; ++i)
                for (size_t j = 0; j < n; ++j) {
                    if (!isfinite(H[pass][i * n + j])) ++failures;
                    if (j / 6 > i / 6 && H[pass][i * n + j] != 0.0) ++failures;   // blocks above the diagonal are never written
                }
            for (size_t i = 6 * 8; i < n; ++i)   // the isolated vertex: lam I, no gradient
                if (H[pass][i * n + i] != 0.5 || g[pass][i] != 0.0) ++failures;
        }
        if (H[0] != H[1] || g[0] != g[1]) { printf("two passes differ\n"); ++failures; }
    }
    printf(failures ? "FAILED %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
#endif
