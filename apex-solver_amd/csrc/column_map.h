// column_map.h -- the permutation between the caller's global column order and the device's internal order, once.  Vectors
// cross the C ABI in the caller's columns (a first column per camera pose, per camera's intrinsics, per landmark, per vertex);
// the device keeps whole blocks in an order of its own (cmap_ / lmap_ of solver.h, vmap_ of pg_solver.h) with the padding of the
// last tile behind them.  A ColumnMap is that permutation per degree of freedom, built in set_structure; every export and import
// of solver.hip and pg_solver.hip goes through one.  No HIP here: tests/host_harness_column_map.cpp walks it on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

namespace apex {

struct ColumnMap {
    std::vector<int64_t> col;         // col[i]: the caller's column of internal DOF i.  The padding is not in the map
    std::vector<int64_t> pos;         // pos[k]: the internal DOF at which the caller's block k starts
    std::vector<int64_t> untouched;   // caller columns no internal DOF maps to (a six-column camera's intrinsics), else empty

    int64_t size() const { return (int64_t)col.size(); }

    // out[col[i]] = f(h[i], i), and `rest` to the untouched columns
    template <typename F>
    void scatter(const double* h, double* out, double rest, F&& f) const {
        for (size_t i = 0; i < col.size(); ++i) out[col[i]] = f(h[i], (int64_t)i);
        for (int64_t u : untouched) out[u] = rest;
    }
    void scatter(const double* h, double* out, double rest) const {
        scatter(h, out, rest, [](double v, int64_t) { return v; });
    }
    // h[i] = in[col[i]]: the reverse.  h holds size() entries or more (padding stays as it is)
    void gather(const double* in, double* h) const {
        for (size_t i = 0; i < col.size(); ++i) h[i] = in[col[i]];
    }
};

// Blocks of `dof` columns each: the caller's block k starts at column first_col[k] and is internal block block_map[k]
// (landmarks: 3, lmap_; pose-graph vertices: 6 | 3, vmap_).
inline ColumnMap block_column_map(const std::vector<int64_t>& first_col, const std::vector<int>& block_map, int dof) {
    ColumnMap m;
    m.col.assign(first_col.size() * (size_t)dof, -1);
    m.pos.resize(first_col.size());
    for (size_t k = 0; k < first_col.size(); ++k) {
        m.pos[k] = (int64_t)block_map[k] * dof;
        for (int a = 0; a < dof; ++a) m.col[(size_t)m.pos[k] + a] = first_col[k] + a;
    }
    return m;
}

// The camera side: camera c is internal camera cmap[c] with dc columns, its pose's six at pose_col[c] and, when dc == 9, its
// three intrinsics at intr_col[c].  dc == 6: the intrinsic columns exist for the caller but not on the device -- untouched.
inline ColumnMap camera_column_map(const std::vector<int64_t>& pose_col, const std::vector<int64_t>& intr_col,
                                   const std::vector<int>& cmap, int dc) {
    ColumnMap m;
    m.col.assign(pose_col.size() * (size_t)dc, -1);
    m.pos.resize(pose_col.size());
    for (size_t c = 0; c < pose_col.size(); ++c) {
        m.pos[c] = (int64_t)cmap[c] * dc;
        for (int a = 0; a < 6; ++a) m.col[(size_t)m.pos[c] + a] = pose_col[c] + a;
        for (int a = 0; a < 3; ++a) {
            if (dc == 9) m.col[(size_t)m.pos[c] + 6 + a] = intr_col[c] + a;
            else m.untouched.push_back(intr_col[c] + a);
        }
    }
    return m;
}

// Whole blocks of w elements (poses 7, cameras 9, points and intrinsics 3, fixed-DOF masks as bytes) between the caller's block
// order and the internal one: internal block block_map[k] is the caller's block k.  src and dst do not overlap.
template <typename T>
void blocks_to_internal(const std::vector<int>& block_map, int w, const T* caller, T* internal) {
    for (size_t k = 0; k < block_map.size(); ++k) memcpy(internal + (size_t)w * block_map[k], caller + (size_t)w * k, (size_t)w * sizeof(T));
}
template <typename T>
void blocks_to_caller(const std::vector<int>& block_map, int w, const T* internal, T* caller) {
    for (size_t k = 0; k < block_map.size(); ++k) memcpy(caller + (size_t)w * k, internal + (size_t)w * block_map[k], (size_t)w * sizeof(T));
}

// The host half of a column scaling set by the caller (jacobi_scaling.h): the caller's vector in internal order, n_pad entries
// with 1 on the padding.  false, and *host is untouched: an entry is not positive and finite.
inline bool gather_scaling(const ColumnMap& map, const double* scaling, int64_t n_pad, std::vector<double>* host) {
    std::vector<double> h((size_t)n_pad, 1.0);
    map.gather(scaling, h.data());
    for (int64_t i = 0; i < map.size(); ++i)
        if (!(h[i] > 0.0) || !std::isfinite(h[i])) return false;
    host->swap(h);
    return true;
}

}  // namespace apex
