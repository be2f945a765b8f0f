// host_harness_landmark_cov_lists.cpp -- build_landmark_cov_lists (csrc/landmark_cov_lists.h) against loops written out
// naively here: g++, no GPU, no HIP.  Prints "ok <n checks>" and returns 0, or names the first check that failed
// (tests/test_setter_lists_host.py).
#include <stdio.h>

#include <vector>

#include "landmark_cov_lists.h"

using namespace apex;

static int n_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++n_checks;                                                      \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static int one_case(const std::vector<int>& count, int small_k, const std::vector<int>& want_small, const std::vector<int>& want_large) {
    const int64_t n_pt = (int64_t)count.size();
    std::vector<int> ptr(n_pt + 1, 0);
    int64_t pairs = 0;
    for (int64_t l = 0; l < n_pt; ++l) {
        ptr[l + 1] = ptr[l] + count[l];
        for (int i = 0; i < count[l]; ++i)
            for (int j = i; j < count[l]; ++j) ++pairs;   // the pairs (i <= j) of one landmark's observations
    }
    const LandmarkCovLists r = build_landmark_cov_lists(n_pt, ptr.data(), small_k);
    CHECK(r.n_small == (int)want_small.size() && r.n_large == (int)want_large.size());
    CHECK((int64_t)r.lists.size() == n_pt);
    CHECK(std::vector<int>(r.lists.begin(), r.lists.begin() + r.n_small) == want_small);
    CHECK(std::vector<int>(r.lists.begin() + r.n_small, r.lists.end()) == want_large);
    CHECK(r.pairs == pairs);
    return 0;
}

int main() {
    const int K = kLcSmallK;
    CHECK(K == 8 && kLcChunk == 32);   // what tests/landmark_cov_ref.py restates
    // counts 0, 1, K and K + 1; two large landmarks of equal count keep their order (3 before 6), the longest comes first
    if (one_case({0, 1, K, K + 1, 2, 3 * K, K + 1, K, 40}, K, {0, 1, 2, 4, 7}, {8, 5, 3, 6})) return 1;
    if (one_case({K + 1, K + 1, K + 1}, K, {}, {0, 1, 2})) return 1;           // all large, all equal: the assembly order
    if (one_case({K, 0, K}, K, {0, 1, 2}, {})) return 1;                        // all small
    if (one_case({5, 2, 3, 9}, 2, {1}, {3, 0, 2})) return 1;                    // another threshold
    if (one_case({}, K, {}, {})) return 1;                                     // no landmark
    printf("ok %d checks\n", n_checks);
    return 0;
}
