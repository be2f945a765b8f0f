// host_harness_hessian_csc.cpp -- hessian_csc (csrc/hessian_csc.cpp) against a dense J^T J + prior diagonal formed naively
// here: g++, no GPU, no HIP.  Jacobian entries are small integers, so every sum is exact and the comparison is ==.  Prints
// "ok <n checks>" and returns 0, or names the first check that failed (tests/test_setter_lists_host.py).
#include <stdio.h>

#include <set>
#include <utility>
#include <vector>

#include "column_map.h"
#include "hessian_csc.h"

using namespace apex;

static int n_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++n_checks;                                                      \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

// 3 cameras in a non-identity internal order, intrinsics-first caller columns with the blocks out of order inside each family
// (as tests/host_harness_column_map.cpp crafts them), 4 landmarks behind them
static const int64_t n_cam = 3, n_pt = 4, n_obs = 7, total = 9 * n_cam + 3 * n_pt;
static const std::vector<int> cmap = {2, 0, 1}, lmap = {3, 1, 0, 2};
static const std::vector<int64_t> intr_col = {3, 6, 0}, pose_col = {9 + 12, 9 + 0, 9 + 6}, pt_col = {27 + 6, 27 + 0, 27 + 9, 27 + 3};
// factor 4 repeats factor 2 (camera 0, landmark 1); camera 2 has no factor; landmark 3 is never observed; factor 3 -- the
// only one of (camera 1, landmark 2) -- has all-zero blocks: a structural zero
static const uint32_t cam_idx[n_obs] = {0, 1, 0, 1, 0, 1, 0}, pt_idx[n_obs] = {0, 0, 1, 2, 1, 1, 2};
static const int kZeroFactor = 3;

static int64_t cam_column(int dc, int64_t c, int a) { (void)dc; return a < 6 ? pose_col[c] + a : intr_col[c] + (a - 6); }

static int one_case(int dc, bool with_priors) {
    const ColumnMap cam_map = camera_column_map(pose_col, intr_col, cmap, dc), pt_map = block_column_map(pt_col, lmap, 3);
    std::vector<double> jc((size_t)2 * dc * n_obs), jl((size_t)6 * n_obs);
    for (int64_t i = 0; i < n_obs; ++i)
        for (int r = 0; r < 2; ++r) {
            for (int a = 0; a < dc; ++a) jc[(size_t)2 * dc * i + r * dc + a] = i == kZeroFactor ? 0.0 : (double)((int)((i * 3 + r * 5 + a * 7) % 5) - 2);
            for (int b = 0; b < 3; ++b) jl[(size_t)6 * i + r * 3 + b] = i == kZeroFactor ? 0.0 : (double)((int)((i * 2 + r * 3 + b * 4 + 1) % 7) - 3);
        }
    // diag(P), INTERNAL camera order: all of camera 2's columns (it is seen through its prior alone), one column of camera 0
    // (added to an observed block), none of camera 1
    std::vector<double> pd;
    if (with_priors) {
        pd.assign((size_t)n_cam * dc, 0.0);
        for (int a = 0; a < dc; ++a) pd[(size_t)cmap[2] * dc + a] = 1.0 + a;
        pd[(size_t)cmap[0] * dc + 2] = 5.0;
    }
    // ---- naive: the dense Jacobian in the caller's columns, H = J^T J + diag, and the structural pattern -----------------
    std::vector<double> J((size_t)2 * n_obs * total, 0.0), H((size_t)total * total, 0.0);
    std::set<std::pair<int64_t, int64_t>> pattern;   // (col, row)
    for (int64_t i = 0; i < n_obs; ++i) {
        std::vector<int64_t> cols;
        for (int a = 0; a < dc; ++a) cols.push_back(cam_column(dc, cam_idx[i], a));
        for (int b = 0; b < 3; ++b) cols.push_back(pt_col[pt_idx[i]] + b);
        for (int r = 0; r < 2; ++r) {
            for (int a = 0; a < dc; ++a) J[(size_t)(2 * i + r) * total + cols[a]] = jc[(size_t)2 * dc * i + r * dc + a];
            for (int b = 0; b < 3; ++b) J[(size_t)(2 * i + r) * total + cols[dc + b]] = jl[(size_t)6 * i + r * 3 + b];
        }
        for (int64_t u : cols)
            for (int64_t v : cols) pattern.insert({u, v});
    }
    for (int64_t u = 0; u < total; ++u)
        for (int64_t v = 0; v < total; ++v) {
            double acc = 0.0;
            for (int64_t r = 0; r < 2 * n_obs; ++r) acc += J[(size_t)r * total + u] * J[(size_t)r * total + v];
            H[(size_t)u * total + v] = acc;
        }
    if (with_priors)
        for (int64_t c = 0; c < n_cam; ++c) {
            bool any = false;
            for (int a = 0; a < dc; ++a) {
                const double p = pd[(size_t)cmap[c] * dc + a];
                H[(size_t)cam_column(dc, c, a) * total + cam_column(dc, c, a)] += p;
                any = any || p != 0.0;
            }
            if (any)   // a camera a prior touches carries its whole diagonal block
                for (int a = 0; a < dc; ++a)
                    for (int b = 0; b < dc; ++b) pattern.insert({cam_column(dc, c, a), cam_column(dc, c, b)});
        }
    // ---- the function: the count alone, then the matrix -----------------------------------------------------------------
    HessianCscInput in;
    in.n_cam = n_cam; in.n_pt = n_pt; in.n_obs = n_obs; in.dc = dc;
    in.cam_idx = cam_idx; in.pt_idx = pt_idx;
    in.cmap = &cmap; in.cam_map = &cam_map; in.pt_map = &pt_map;
    if (with_priors) in.prior_diag = &pd;
    const int64_t nnz = hessian_csc(in, nullptr, nullptr, nullptr);
    CHECK(nnz == (int64_t)pattern.size());
    // by the rule: 6 distinct couplings (7 factors, one repeated), the cameras and landmarks that carry entries
    CHECK(nnz == 2 * 6 * dc * 3 + (with_priors ? 3 : 2) * dc * dc + 3 * 9);
    in.jc = jc.data(); in.jl = jl.data();
    std::vector<int64_t> colptr(total + 1, -1), rowidx(nnz + 1, -1);
    std::vector<double> values(nnz + 1, -777.0);
    CHECK(hessian_csc(in, colptr.data(), rowidx.data(), values.data()) == nnz);
    CHECK(colptr[0] == 0 && colptr[total] == nnz);
    CHECK(rowidx[nnz] == -1 && values[nnz] == -777.0);   // nothing behind the end
    std::set<std::pair<int64_t, int64_t>> got;
    std::vector<double> dense((size_t)total * total, 0.0);
    bool zero_kept = false;
    for (int64_t j = 0; j < total; ++j) {
        CHECK(colptr[j] <= colptr[j + 1]);
        for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) {
            CHECK(rowidx[k] >= 0 && rowidx[k] < total);
            if (k > colptr[j]) CHECK(rowidx[k - 1] < rowidx[k]);   // ascending, no entry twice (the duplicated factor is merged)
            CHECK(got.insert({j, rowidx[k]}).second);
            CHECK(values[k] == H[(size_t)rowidx[k] * total + j]);
            dense[(size_t)rowidx[k] * total + j] = values[k];
            if (j == cam_column(dc, 1, 0) && rowidx[k] == pt_col[2]) zero_kept = values[k] == 0.0;
        }
    }
    CHECK(got == pattern);
    CHECK(dense == H);       // ... so nothing of H lies outside the pattern
    CHECK(zero_kept);        // the coupling of the all-zero factor is stored, as a zero
    for (int b = 0; b < 3; ++b) CHECK(colptr[pt_col[3] + b + 1] == colptr[pt_col[3] + b]);   // the unobserved landmark: empty columns
    for (int a = 0; a < dc; ++a)   // camera 2: its diagonal block with the priors, nothing without
        CHECK(colptr[cam_column(dc, 2, a) + 1] - colptr[cam_column(dc, 2, a)] == (with_priors ? dc : 0));
    if (dc == 6)
        for (int64_t c = 0; c < n_cam; ++c)
            for (int a = 0; a < 3; ++a) CHECK(colptr[intr_col[c] + a + 1] == colptr[intr_col[c] + a]);   // no intrinsic columns on the device
    // an all-zero prior diagonal touches no camera
    std::vector<double> none((size_t)n_cam * dc, 0.0);
    in.prior_diag = &none; in.jc = in.jl = nullptr;
    CHECK(hessian_csc(in, nullptr, nullptr, nullptr) == 2 * 6 * dc * 3 + 2 * dc * dc + 3 * 9);
    return 0;
}

int main() {
    for (int dc : {9, 6})
        for (bool with_priors : {false, true})
            if (one_case(dc, with_priors)) return 1;
    {   // no factor at all: an empty matrix
        const ColumnMap cam_map = camera_column_map(pose_col, intr_col, cmap, 9), pt_map = block_column_map(pt_col, lmap, 3);
        HessianCscInput in;
        in.n_cam = n_cam; in.n_pt = n_pt; in.n_obs = 0; in.dc = 9;
        in.cmap = &cmap; in.cam_map = &cam_map; in.pt_map = &pt_map;
        CHECK(hessian_csc(in, nullptr, nullptr, nullptr) == 0);
    }
    printf("ok %d checks\n", n_checks);
    return 0;
}
