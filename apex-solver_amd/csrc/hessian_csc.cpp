// hessian_csc.cpp -- see hessian_csc.h
#include "hessian_csc.h"

#include <algorithm>
#include <numeric>

namespace apex {

int64_t hessian_csc(const HessianCscInput& in, int64_t* colptr, int64_t* rowidx, double* values) {
    const int64_t n_cam = in.n_cam, n_pt = in.n_pt, n_obs = in.n_obs, total = 9 * n_cam + 3 * n_pt;
    const int dc = in.dc;
    const uint32_t *cam_idx = in.cam_idx, *pt_idx = in.pt_idx;
    // unique (camera, landmark) couplings and the variables that carry entries
    std::vector<int64_t> order(n_obs);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return pt_idx[a] != pt_idx[b] ? pt_idx[a] < pt_idx[b] : cam_idx[a] < cam_idx[b];
    });
    std::vector<uint8_t> cam_seen(n_cam, 0), pt_seen(n_pt, 0);
    int64_t n_cl = 0;
    for (int64_t k = 0; k < n_obs; ++k) {
        const int64_t i = order[k];
        cam_seen[cam_idx[i]] = 1; pt_seen[pt_idx[i]] = 1;
        if (k == 0 || pt_idx[i] != pt_idx[order[k - 1]] || cam_idx[i] != cam_idx[order[k - 1]]) ++n_cl;
    }
    // diag(P) of the camera priors: their cameras carry a diagonal block even when unobserved
    const bool priors = in.prior_diag && !in.prior_diag->empty();
    const auto pd = [&](int64_t c, int a) { return (*in.prior_diag)[(size_t)(*in.cmap)[c] * dc + a]; };
    if (priors)
        for (int64_t c = 0; c < n_cam; ++c)
            for (int a = 0; a < dc; ++a)
                if (pd(c, a) != 0.0) cam_seen[c] = 1;
    int64_t nnz = 2 * n_cl * dc * 3;
    for (int64_t c = 0; c < n_cam; ++c) if (cam_seen[c]) nnz += dc * dc;
    for (int64_t l = 0; l < n_pt; ++l) if (pt_seen[l]) nnz += 9;
    if (!in.jc || !in.jl) return nnz;
    // column a of the caller's camera c: cc[cp[c] + a]; column b of its landmark l: pc[pp[l] + b]
    const std::vector<int64_t>&cc = in.cam_map->col, &cp = in.cam_map->pos, &pc = in.pt_map->col, &pp = in.pt_map->pos;
    struct Trip { int64_t col, row; double v; };
    std::vector<Trip> t;
    t.reserve((size_t)nnz);
    {   // camera blocks
        std::vector<double> hcc((size_t)n_cam * dc * dc, 0.0);
        for (int64_t i = 0; i < n_obs; ++i) {
            const double* J = in.jc + (size_t)2 * dc * i;
            double* H = hcc.data() + (size_t)cam_idx[i] * dc * dc;
            for (int a = 0; a < dc; ++a)
                for (int b = 0; b < dc; ++b) H[a * dc + b] += J[a] * J[b] + J[dc + a] * J[dc + b];
        }
        if (priors)
            for (int64_t c = 0; c < n_cam; ++c)
                for (int a = 0; a < dc; ++a) hcc[(size_t)c * dc * dc + a * dc + a] += pd(c, a);
        for (int64_t c = 0; c < n_cam; ++c)
            if (cam_seen[c])
                for (int a = 0; a < dc; ++a)
                    for (int b = 0; b < dc; ++b) t.push_back({cc[cp[c] + b], cc[cp[c] + a], hcc[(size_t)c * dc * dc + a * dc + b]});
    }
    {   // landmark blocks
        std::vector<double> hll((size_t)n_pt * 9, 0.0);
        for (int64_t i = 0; i < n_obs; ++i) {
            const double* J = in.jl + (size_t)6 * i;
            double* H = hll.data() + (size_t)pt_idx[i] * 9;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) H[3 * a + b] += J[a] * J[b] + J[3 + a] * J[3 + b];
        }
        for (int64_t l = 0; l < n_pt; ++l)
            if (pt_seen[l])
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) t.push_back({pc[pp[l] + b], pc[pp[l] + a], hll[(size_t)l * 9 + 3 * a + b]});
    }
    {   // couplings, duplicated (camera, landmark) factors merged
        std::vector<double> w((size_t)dc * 3);
        for (int64_t k = 0; k < n_obs;) {
            const int64_t i0 = order[k];
            const uint32_t c = cam_idx[i0], l = pt_idx[i0];
            std::fill(w.begin(), w.end(), 0.0);
            for (; k < n_obs && cam_idx[order[k]] == c && pt_idx[order[k]] == l; ++k) {
                const double* Jc = in.jc + (size_t)2 * dc * order[k];
                const double* Jl = in.jl + (size_t)6 * order[k];
                for (int a = 0; a < dc; ++a)
                    for (int b = 0; b < 3; ++b) w[a * 3 + b] += Jc[a] * Jl[b] + Jc[dc + a] * Jl[3 + b];
            }
            for (int a = 0; a < dc; ++a)
                for (int b = 0; b < 3; ++b) {
                    t.push_back({pc[pp[l] + b], cc[cp[c] + a], w[a * 3 + b]});
                    t.push_back({cc[cp[c] + a], pc[pp[l] + b], w[a * 3 + b]});
                }
        }
    }
    if ((int64_t)t.size() != nnz) return -1;
    std::sort(t.begin(), t.end(), [](const Trip& a, const Trip& b) { return a.col != b.col ? a.col < b.col : a.row < b.row; });
    std::fill(colptr, colptr + total + 1, 0);
    for (const Trip& e : t) colptr[e.col + 1]++;
    for (int64_t j = 0; j < total; ++j) colptr[j + 1] += colptr[j];
    for (int64_t k = 0; k < nnz; ++k) { rowidx[k] = t[k].row; values[k] = t[k].v; }
    return nnz;
}

}  // namespace apex
