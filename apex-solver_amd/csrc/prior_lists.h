// prior_lists.h -- the host lists of a set of PriorFactor blocks, for both solvers (Solver::set_priors, DESIGN.md §17;
// PoseGraphSolver::set_priors): the caller's blocks in the order the device sums them, each packed as
// [data (amb) | Huber delta or -1 | weight or 1 (where the block has one) | zero padding], with the internal owner and the
// caller's index per block and, where asked for, a CSR over the owners.  The refusals of the two setters stand beside the
// builder as functions that return the text (empty: accepted).  Plain host C++: tests/host_harness_prior_lists.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

namespace apex {

constexpr int kPosePriorStride = 10;   // doubles per pose block: data [t, qw qx qy qz] (7) | Huber delta (<= 0: none) | w | pad
constexpr int kIntrPriorStride = 6;    // doubles per intrinsics block: data [f, k1, k2] (3) | Huber delta | w | pad

struct PriorLists {
    std::vector<int> owner;     // [n] the internal index of the block's camera / vertex
    std::vector<int> slot;      // [n] the caller's index of the block (export order)
    std::vector<int> ptr;       // [n_owners + 1] run of owner o: [ptr[o], ptr[o + 1]); empty when not asked for
    std::vector<double> data;   // [n][stride]
};

struct PriorLayout {
    int amb, stride;   // doubles of the datum, doubles per block
    bool weighted;     // the block carries a weight behind its Huber delta (bundle adjustment), else padding (pose graphs)
};

// index[k]: the caller's owner of block k, map: caller's owner -> internal.  sorted: by internal owner, stable, so that one lane
// sums an owner's run in the caller's order; else the caller's order, slot the identity.  n_owners > 0: the CSR (sorted sets).
inline PriorLists build_prior_lists(int64_t n, const uint32_t* index, const std::vector<int>& map, PriorLayout lay, const double* data,
                                    const double* huber_delta, const double* weight, bool sorted, int64_t n_owners) {
    PriorLists p;
    p.slot.resize((size_t)n);
    std::iota(p.slot.begin(), p.slot.end(), 0);
    if (sorted) std::stable_sort(p.slot.begin(), p.slot.end(), [&](int a, int b) { return map[index[a]] < map[index[b]]; });
    p.owner.resize((size_t)n);
    p.data.assign((size_t)n * lay.stride, 0.0);
    if (n_owners > 0) p.ptr.assign((size_t)n_owners + 1, 0);
    for (int64_t k = 0; k < n; ++k) {
        const int src = p.slot[k];
        p.owner[k] = map[index[src]];
        if (n_owners > 0) p.ptr[p.owner[k] + 1]++;
        double* d = p.data.data() + (size_t)k * lay.stride;
        memcpy(d, data + (size_t)lay.amb * src, lay.amb * sizeof(double));
        d[lay.amb] = huber_delta ? huber_delta[src] : -1.0;
        if (lay.weighted) d[lay.amb + 1] = weight ? weight[src] : 1.0;
    }
    for (int64_t o = 0; o < n_owners; ++o) p.ptr[o + 1] += p.ptr[o];
    return p;
}

inline bool prior_count_in_range(int64_t n) { return n >= 0 && n <= (1 << 24); }

// Solver::set_priors, block by block: a camera that does not exist, NaN data, a NaN Huber delta, a weight that is not finite and
// positive.  `what` is the entry's name (set_pose_priors / set_intrinsic_priors).
inline std::string ba_prior_refusal(const std::string& what, int64_t n, const uint32_t* cam, int64_t n_cam, int amb, const double* data,
                                    const double* huber_delta, const double* weight) {
    for (int64_t k = 0; k < n; ++k) {
        if ((int64_t)cam[k] >= n_cam) return what + ": prior " + std::to_string(k) + " is on a camera that does not exist";
        for (int a = 0; a < amb; ++a)
            if (std::isnan(data[amb * k + a])) return what + ": prior " + std::to_string(k) + " has NaN data";
        if (huber_delta && std::isnan(huber_delta[k])) return what + ": prior " + std::to_string(k) + " has a NaN Huber delta";
        if (weight && !(std::isfinite(weight[k]) && weight[k] > 0.0))
            return what + ": the weight of prior " + std::to_string(k) + " must be finite and positive";
    }
    return "";
}

// PoseGraphSolver::set_priors: the range alone
inline std::string pg_prior_refusal(int64_t n, const uint32_t* vertex, int64_t n_v) {
    for (int64_t k = 0; k < n; ++k)
        if ((int64_t)vertex[k] >= n_v) return "prior on a vertex that does not exist";
    return "";
}

}  // namespace apex
