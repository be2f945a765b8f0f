// host_harness_column_map.cpp -- ColumnMap, its builders, the block permutes and the host half of the scaling holder
// (csrc/column_map.h) against the loops written out naively here: g++, no GPU, no HIP.  Prints "ok <n checks>" and returns 0, or
// names the first check that failed (tests/test_column_map_host.py).
#include <math.h>
#include <stdio.h>

#include <limits>
#include <set>
#include <vector>

#include "column_map.h"

using namespace apex;

static int n_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++n_checks;                                                      \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static const double kMark = -777.0;   // what an output holds before a scatter: no export writes it

// scatter then gather is the identity on the internal vector; the scatter writes exactly col and untouched; col is injective
static int round_trip(const ColumnMap& m, int64_t n_cols, double rest) {
    const int64_t n = m.size();
    std::set<int64_t> seen(m.col.begin(), m.col.end());
    CHECK((int64_t)seen.size() == n);                                  // injective
    for (int64_t u : m.untouched) CHECK(seen.insert(u).second);        // ... and disjoint from the untouched columns
    CHECK(*seen.begin() >= 0 && *seen.rbegin() < n_cols);
    std::vector<double> h(n), out(n_cols, kMark), back(n + 5, kMark);
    for (int64_t i = 0; i < n; ++i) h[i] = 1000.0 + (double)i;
    m.scatter(h.data(), out.data(), rest);
    for (int64_t j = 0; j < n_cols; ++j) CHECK((out[j] != kMark) == (seen.count(j) == 1));   // nothing else is written
    for (int64_t u : m.untouched) CHECK(out[u] == rest);
    m.gather(out.data(), back.data());
    for (int64_t i = 0; i < n; ++i) CHECK(back[i] == h[i]);
    for (int64_t i = n; i < n + 5; ++i) CHECK(back[i] == kMark);      // the padding behind the map stays as it is
    std::vector<double> out2(n_cols, kMark);                          // the functor sees the value and the INTERNAL index
    m.scatter(h.data(), out2.data(), rest, [](double v, int64_t i) { return 2.0 * v + (double)i; });
    for (int64_t i = 0; i < n; ++i) CHECK(out2[m.col[i]] == 2.0 * h[i] + (double)i);
    return 0;
}

template <typename T>
static int permute_round_trip(const std::vector<int>& map, int w) {
    const size_t n = map.size();
    std::vector<T> caller(n * w), internal(n * w, (T)0), naive(n * w, (T)0), back(n * w, (T)0);
    for (size_t i = 0; i < caller.size(); ++i) caller[i] = (T)(1 + (i * 7) % 250);
    for (size_t k = 0; k < n; ++k)
        for (int a = 0; a < w; ++a) naive[(size_t)w * map[k] + a] = caller[(size_t)w * k + a];
    blocks_to_internal(map, w, caller.data(), internal.data());
    CHECK(internal == naive);
    blocks_to_caller(map, w, internal.data(), back.data());
    CHECK(back == caller);
    return 0;
}

int main() {
    // 4 cameras in a non-identity internal order; intrinsics-first caller columns as the layout deals them, with the cameras'
    // blocks out of order inside each family; 5 landmarks behind them
    const std::vector<int> cmap = {2, 0, 3, 1}, lmap = {4, 2, 0, 1, 3};
    const std::vector<int64_t> intr_col = {3, 9, 0, 6}, pose_col = {12 + 18, 12 + 0, 12 + 6, 12 + 12}, pt_col = {36 + 6, 36 + 0, 36 + 12, 36 + 3, 36 + 9};
    const int64_t n_cam = 4, cam_cols = 9 * n_cam, total = cam_cols + 15;
    for (int dc : {9, 6}) {
        const ColumnMap m = camera_column_map(pose_col, intr_col, cmap, dc);
        CHECK(m.size() == n_cam * dc && (int64_t)m.pos.size() == n_cam);
        for (int64_t c = 0; c < n_cam; ++c) {                          // the loop every export used to write out
            CHECK(m.pos[c] == (int64_t)cmap[c] * dc);
            for (int a = 0; a < 6; ++a) CHECK(m.col[cmap[c] * dc + a] == pose_col[c] + a);
            if (dc == 9) for (int a = 0; a < 3; ++a) CHECK(m.col[cmap[c] * dc + 6 + a] == intr_col[c] + a);
        }
        CHECK((int64_t)m.untouched.size() == (dc == 6 ? 3 * n_cam : 0));
        std::set<int64_t> all(m.col.begin(), m.col.end());
        all.insert(m.untouched.begin(), m.untouched.end());
        CHECK((int64_t)all.size() == cam_cols && *all.begin() == 0 && *all.rbegin() == cam_cols - 1);   // covers the camera side
        if (dc == 6) {
            std::set<int64_t> want;
            for (int64_t c = 0; c < n_cam; ++c) for (int a = 0; a < 3; ++a) want.insert(intr_col[c] + a);
            CHECK(std::set<int64_t>(m.untouched.begin(), m.untouched.end()) == want);
        }
        if (round_trip(m, total, 0.0) || round_trip(m, total, 0.125)) return 1;
    }
    {
        const ColumnMap m = block_column_map(pt_col, lmap, 3);
        CHECK(m.size() == 15 && m.untouched.empty());
        for (int l = 0; l < 5; ++l) {
            CHECK(m.pos[l] == 3 * lmap[l]);
            for (int a = 0; a < 3; ++a) CHECK(m.col[3 * lmap[l] + a] == pt_col[l] + a);
        }
        if (round_trip(m, total, 0.0)) return 1;
    }
    // a pose graph of 4 vertices, six and three columns each, columns in sorted-name order rather than vertex order
    const std::vector<int> vmap = {1, 3, 0, 2};
    for (int dof : {6, 3}) {
        const std::vector<int64_t> col = {2 * (int64_t)dof, 0, 3 * (int64_t)dof, (int64_t)dof};
        const ColumnMap m = block_column_map(col, vmap, dof);
        CHECK(m.size() == 4 * dof && m.untouched.empty());
        for (int v = 0; v < 4; ++v)
            for (int a = 0; a < dof; ++a) CHECK(m.col[dof * vmap[v] + a] == col[v] + a);
        if (round_trip(m, 4 * dof, 0.0)) return 1;
    }
    // whole blocks: points / intrinsics 3, poses 7, cameras 9, fixed-DOF masks as bytes
    for (int w : {3, 7, 9}) {
        if (permute_round_trip<double>(cmap, w) || permute_round_trip<double>(lmap, w)) return 1;
        if (permute_round_trip<unsigned char>(cmap, w == 7 ? 6 : w) || permute_round_trip<unsigned char>(lmap, 3)) return 1;
    }
    {   // the host half of the scaling holder: permuted, 1.0 on the padding, refused without a trace
        const ColumnMap m = camera_column_map(pose_col, intr_col, cmap, 6);
        std::vector<double> s(total), host = {-1.0, -2.0};
        for (int64_t j = 0; j < total; ++j) s[j] = 0.5 + (double)j;
        for (int64_t u : m.untouched) s[u] = -5.0;   // a six-column camera's intrinsic entries are never read
        const int64_t n_pad = m.size() + 7;
        CHECK(gather_scaling(m, s.data(), n_pad, &host));
        CHECK((int64_t)host.size() == n_pad);
        for (int64_t i = 0; i < m.size(); ++i) CHECK(host[i] == s[m.col[i]]);
        for (int64_t i = m.size(); i < n_pad; ++i) CHECK(host[i] == 1.0);
        const std::vector<double> kept = host;
        const double inf = std::numeric_limits<double>::infinity(), bad[5] = {0.0, -1.0, inf, -inf, std::numeric_limits<double>::quiet_NaN()};
        for (double b : bad)
            for (int64_t at : {m.col.front(), m.col.back(), m.col[7]}) {
                std::vector<double> t = s;
                t[at] = b;
                CHECK(!gather_scaling(m, t.data(), n_pad, &host));
                CHECK(host == kept);
            }
    }
    printf("ok %d checks\n", n_checks);
    return 0;
}
