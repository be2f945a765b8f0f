// host_harness_prior_lists.cpp -- build_prior_lists and the refusals of the two set_priors (csrc/prior_lists.h) against the loops
// written out naively here: g++, no GPU, no HIP.  Prints "ok <n checks>" and returns 0, or names the first check that failed
// (tests/test_setter_lists_host.py).
#include <math.h>
#include <stdio.h>

#include <limits>
#include <string>
#include <vector>

#include "prior_lists.h"

using namespace apex;

static int n_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++n_checks;                                                      \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

// 4 owners with a non-identity map; 7 blocks: three on owner 2 in non-sorted caller order (0, 3, 4 -- the last two in a row),
// owner 1 with none, owner 3 and owner 0 out of order between them
static const std::vector<int> kMap = {2, 0, 3, 1};
static const uint32_t kIndex[7] = {2, 3, 0, 2, 2, 3, 0};

static double datum(int k, int a) { return 100.0 * (k + 1) + a + 0.5; }

static int one_layout(PriorLayout lay, bool with_delta, bool with_weight) {
    const int64_t n = 7, n_owners = 4;
    std::vector<double> data((size_t)n * lay.amb), delta(n), weight(n);
    for (int k = 0; k < n; ++k) {
        for (int a = 0; a < lay.amb; ++a) data[(size_t)lay.amb * k + a] = datum(k, a);
        delta[k] = k % 2 ? 0.25 * k : -1.0;
        weight[k] = 1.0 + 0.125 * k;
    }
    const double* dl = with_delta ? delta.data() : nullptr;
    const double* w = with_weight ? weight.data() : nullptr;
    for (bool sorted : {true, false}) {
        // the naive order: for every internal owner in turn, the caller's blocks on it in the caller's order
        std::vector<int> want;
        if (sorted) {
            for (int o = 0; o < n_owners; ++o)
                for (int k = 0; k < n; ++k)
                    if (kMap[kIndex[k]] == o) want.push_back(k);
        } else {
            for (int k = 0; k < n; ++k) want.push_back(k);
        }
        const PriorLists p = build_prior_lists(n, kIndex, kMap, lay, data.data(), dl, w, sorted, sorted ? n_owners : 0);
        CHECK(p.slot == want);
        CHECK((int64_t)p.owner.size() == n && (int64_t)p.data.size() == n * lay.stride);
        for (int k = 0; k < n; ++k) {
            const int src = want[k];
            CHECK(p.owner[k] == kMap[kIndex[src]]);
            if (sorted && k > 0) CHECK(p.owner[k - 1] <= p.owner[k]);
            const double* d = p.data.data() + (size_t)k * lay.stride;
            for (int a = 0; a < lay.amb; ++a) CHECK(d[a] == datum(src, a));
            CHECK(d[lay.amb] == (with_delta ? delta[src] : -1.0));
            int used = lay.amb + 1;
            if (lay.weighted) { CHECK(d[lay.amb + 1] == (with_weight ? weight[src] : 1.0)); ++used; }
            for (int a = used; a < lay.stride; ++a) CHECK(d[a] == 0.0 && !std::signbit(d[a]));   // the padding
        }
        if (sorted) {   // the CSR: owner o's run is [ptr[o], ptr[o + 1])
            CHECK((int64_t)p.ptr.size() == n_owners + 1 && p.ptr[0] == 0 && p.ptr[n_owners] == n);
            for (int o = 0; o < n_owners; ++o) {
                int count = 0;
                for (int k = 0; k < n; ++k) count += kMap[kIndex[k]] == o;
                CHECK(p.ptr[o + 1] - p.ptr[o] == count);
                for (int k = p.ptr[o]; k < p.ptr[o + 1]; ++k) CHECK(p.owner[k] == o);
            }
            CHECK(p.ptr[1] - p.ptr[0] == 0);   // internal owner 0 is the caller's 1: no block
        } else {
            CHECK(p.ptr.empty());
        }
    }
    // the run of internal owner 3 (the caller's 2) keeps the caller's order 0, 3, 4
    const PriorLists p = build_prior_lists(n, kIndex, kMap, lay, data.data(), dl, w, true, n_owners);
    CHECK(p.ptr[4] - p.ptr[3] == 3 && p.slot[p.ptr[3]] == 0 && p.slot[p.ptr[3] + 1] == 3 && p.slot[p.ptr[3] + 2] == 4);
    // n = 0: empty lists, a CSR of zeros when asked for
    const PriorLists e = build_prior_lists(0, nullptr, kMap, lay, nullptr, nullptr, nullptr, true, n_owners);
    CHECK(e.owner.empty() && e.slot.empty() && e.data.empty() && e.ptr == std::vector<int>(n_owners + 1, 0));
    const PriorLists e2 = build_prior_lists(0, nullptr, kMap, lay, nullptr, nullptr, nullptr, false, 0);
    CHECK(e2.owner.empty() && e2.slot.empty() && e2.data.empty() && e2.ptr.empty());
    return 0;
}

int main() {
    // every real use: BA pose and intrinsics blocks (weighted), and the blocks of the three pose-graph manifolds -- SE3 (7 | 8),
    // SE2 (3 | 4), SO3 (4 | 6): Se3Manifold / Se2Manifold / So3Manifold ::kAmb | ::kPriorStride
    const PriorLayout lays[5] = {{7, kPosePriorStride, true}, {3, kIntrPriorStride, true}, {7, 8, false}, {3, 4, false}, {4, 6, false}};
    for (const PriorLayout& lay : lays)
        for (int opt = 0; opt < 4; ++opt)
            if (one_layout(lay, opt & 1, lay.weighted && (opt & 2))) return 1;
    CHECK(kPosePriorStride >= 7 + 2 && kIntrPriorStride >= 3 + 2);

    // the refusals, each with the text the C ABI's callers see
    CHECK(prior_count_in_range(0) && prior_count_in_range(1 << 24) && !prior_count_in_range(-1) && !prior_count_in_range((1 << 24) + 1));
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const uint32_t cam[3] = {1, 3, 0};
    std::vector<double> data(21, 1.0), delta(3, -1.0), weight(3, 2.0);
    const std::string w = "set_pose_priors";
    CHECK(ba_prior_refusal(w, 3, cam, 4, 7, data.data(), delta.data(), weight.data()).empty());
    CHECK(ba_prior_refusal(w, 3, cam, 4, 7, data.data(), nullptr, nullptr).empty());
    CHECK(ba_prior_refusal(w, 0, nullptr, 4, 7, nullptr, nullptr, nullptr).empty());
    CHECK(ba_prior_refusal(w, 3, cam, 3, 7, data.data(), nullptr, nullptr) == "set_pose_priors: prior 1 is on a camera that does not exist");
    data[2 * 7 + 6] = nan;
    CHECK(ba_prior_refusal(w, 3, cam, 4, 7, data.data(), nullptr, nullptr) == "set_pose_priors: prior 2 has NaN data");
    CHECK(ba_prior_refusal("set_intrinsic_priors", 3, cam, 4, 3, data.data(), nullptr, nullptr).empty());   // (the first nine doubles are fine)
    data[4] = nan;
    CHECK(ba_prior_refusal("set_intrinsic_priors", 3, cam, 4, 3, data.data(), nullptr, nullptr) == "set_intrinsic_priors: prior 1 has NaN data");
    data[4] = 1.0; data[2 * 7 + 6] = inf;   // an infinite datum is not refused (NaN alone is)
    CHECK(ba_prior_refusal(w, 3, cam, 4, 7, data.data(), nullptr, nullptr).empty());
    delta[1] = nan;
    CHECK(ba_prior_refusal(w, 3, cam, 4, 7, data.data(), delta.data(), weight.data()) == "set_pose_priors: prior 1 has a NaN Huber delta");
    delta[1] = 0.0;
    for (double bad : {0.0, -1.0, inf, nan}) {
        weight[2] = bad;
        CHECK(ba_prior_refusal(w, 3, cam, 4, 7, data.data(), delta.data(), weight.data()) == "set_pose_priors: the weight of prior 2 must be finite and positive");
    }
    // block by block: the first block that fails any check is the one named, whatever a later block fails
    weight[2] = 2.0; weight[1] = -1.0; data[2 * 7] = nan;
    CHECK(ba_prior_refusal(w, 3, cam, 4, 7, data.data(), delta.data(), weight.data()) == "set_pose_priors: the weight of prior 1 must be finite and positive");
    // the pose graph checks the range alone
    CHECK(pg_prior_refusal(3, cam, 4).empty() && pg_prior_refusal(0, nullptr, 4).empty());
    CHECK(pg_prior_refusal(3, cam, 3) == "prior on a vertex that does not exist");
    printf("ok %d checks\n", n_checks);
    return 0;
}
