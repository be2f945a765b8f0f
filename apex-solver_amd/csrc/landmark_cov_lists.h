// landmark_cov_lists.h -- the landmark lists of the covariance pass (Solver::landmark_covariance, cov_kernels.hip)
// from the observation pointers, as a value.  Plain host C++: tests/host_harness_landmark_cov_lists.cpp.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace apex {

// a landmark with at most kLcSmallK observations takes 8 lanes; the others a 64-lane workgroup each, chunks of kLcChunk
// observations (cov_kernels.hip)
constexpr int kLcSmallK = 8, kLcChunk = 32;

struct LandmarkCovLists {
    std::vector<int> lists;   // [n_small | n_large] landmarks
    int n_small = 0, n_large = 0;
    int64_t pairs = 0;        // observation pairs: sum k (k + 1) / 2
};

// ptr [n_pt + 1]: landmark l has ptr[l + 1] - ptr[l] observations.  The landmarks with at most small_k of them in the
// landmark-major order of the assembly (neighbours share cameras, so their Z blocks meet in L2), then the others by decreasing
// count, stable (one workgroup each, launched first: the longest start earliest).
inline LandmarkCovLists build_landmark_cov_lists(int64_t n_pt, const int* ptr, int small_k) {
    LandmarkCovLists r;
    std::vector<int> large;
    for (int64_t l = 0; l < n_pt; ++l) {
        const int64_t k = ptr[l + 1] - ptr[l];
        r.pairs += k * (k + 1) / 2;
        (k <= small_k ? r.lists : large).push_back((int)l);
    }
    std::stable_sort(large.begin(), large.end(), [&](int a, int b) { return ptr[a + 1] - ptr[a] > ptr[b + 1] - ptr[b]; });
    r.n_small = (int)r.lists.size();
    r.n_large = (int)large.size();
    r.lists.insert(r.lists.end(), large.begin(), large.end());
    return r;
}

}  // namespace apex
