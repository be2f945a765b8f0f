// host_harness_info_pack.cpp -- info_validate_and_pack and info_expand (csrc/info_pack.h) against loops written out naively
// here: g++, no GPU, no HIP.  Prints "ok <n checks>" and returns 0, or names the first check that failed
// (tests/test_setter_lists_host.py).
#include <math.h>
#include <stdio.h>

#include <limits>
#include <string>
#include <vector>

#include "info_pack.h"

using namespace apex;

static int n_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++n_checks;                                                      \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

// an SPD matrix of small integers: A A^T + 2 D I, A's entries in -2 .. 2
static void spd(int D, int e, double* W) {
    std::vector<int> A(D * D);
    for (int i = 0; i < D * D; ++i) A[i] = (int)((i * 7 + e * 5 + (i / D) * 3) % 5) - 2;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            int acc = i == j ? 2 * D : 0;
            for (int k = 0; k < D; ++k) acc += A[D * i + k] * A[D * j + k];
            W[D * i + j] = (double)acc;
        }
}

static std::string refusal(int D, int64_t n_e, const std::vector<double>& info) {
    std::vector<double> packed;
    std::string err;
    return info_validate_and_pack(D, n_e, info.data(), &packed, &err) ? std::string("accepted") : err;
}

static int one_width(int D, int want_stride) {
    const int64_t n_e = 3;
    const int S = info_stride(D), DD = D * D;
    CHECK(S == want_stride && S % 2 == 0 && S >= info_packed(D) && S - info_packed(D) <= 1);
    std::vector<double> info((size_t)n_e * DD), packed, back((size_t)n_e * DD, -7.0);
    for (int e = 0; e < n_e; ++e) spd(D, e, info.data() + (size_t)e * DD);
    std::string err = "untouched";
    CHECK(info_validate_and_pack(D, n_e, info.data(), &packed, &err) && err == "untouched");
    CHECK((int64_t)packed.size() == n_e * S);
    for (int e = 0; e < n_e; ++e) {   // the upper triangle in row order, zero behind it
        int k = 0;
        for (int i = 0; i < D; ++i)
            for (int j = i; j < D; ++j) CHECK(packed[(size_t)e * S + k++] == info[(size_t)e * DD + D * i + j]);
        for (; k < S; ++k) CHECK(packed[(size_t)e * S + k] == 0.0);
    }
    info_expand(D, n_e, packed.data(), back.data());
    CHECK(back == info);
    CHECK(refusal(D, 0, {}) == "accepted");

    // refusals; the matrix at fault is edge 2, the text names it
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const size_t at = (size_t)2 * DD;
    for (double bad : {inf, -inf, nan})
        for (int where : {0, D - 1, DD - 1}) {
            std::vector<double> t = info;
            t[at + where] = bad;
            CHECK(refusal(D, n_e, t) == "set_information: edge 2 has an entry that is not finite");
        }
    {   // symmetric to 1e-12 max|W|: max|W| = 4 is a power of two, so the bound 1e-12 * 4 is the double 1e-12 scaled exactly; the
        // upper entry is 0, so the difference is the lower entry itself
        std::vector<double> t = info;
        double* W = t.data() + at;
        for (int i = 0; i < DD; ++i) W[i] = 0.0;
        for (int i = 0; i < D; ++i) W[D * i + i] = i == 0 ? 4.0 : 1.0;
        const double bound = 1e-12 * 4.0;
        const int lower = D * (D - 1) + 0;   // (D - 1, 0) against (0, D - 1)
        for (double d : {bound, nextafter(bound, 0.0), 0.5 * bound, -bound}) {
            W[lower] = d;
            CHECK(refusal(D, n_e, t) == "accepted");
        }
        for (double d : {nextafter(bound, 1.0), 2.0 * bound, -nextafter(bound, 1.0)}) {
            W[lower] = d;
            CHECK(refusal(D, n_e, t) == "set_information: edge 2 is not symmetric");
        }
        W[lower] = 0.0;
        // the same asymmetry on edge 0: edge 0 is named
        t[(size_t)D * 1 + 0] = t[(size_t)0 * D + 1] + 1.0;
        CHECK(refusal(D, n_e, t) == "set_information: edge 0 is not symmetric");
    }
    {   // pivots: the first that is not positive is named
        std::vector<double> t = info;
        double* W = t.data() + at;
        for (int i = 0; i < DD; ++i) W[i] = 0.0;
        for (int i = 0; i < D; ++i) W[D * i + i] = 1.0;
        W[1] = W[D] = 1.0;   // [1 1; 1 1] in the corner: singular, pivot 1 is exactly 0
        CHECK(refusal(D, n_e, t) == "set_information: edge 2 is not positive definite (Cholesky pivot 1 <= 0)");
        W[1] = W[D] = 2.0;   // [1 2; 2 1]: indefinite, pivot 1 is -3
        CHECK(refusal(D, n_e, t) == "set_information: edge 2 is not positive definite (Cholesky pivot 1 <= 0)");
        W[1] = W[D] = 0.0;
        W[0] = 0.0;          // pivot 0 is exactly 0
        CHECK(refusal(D, n_e, t) == "set_information: edge 2 is not positive definite (Cholesky pivot 0 <= 0)");
        W[0] = -1.0;
        CHECK(refusal(D, n_e, t) == "set_information: edge 2 is not positive definite (Cholesky pivot 0 <= 0)");
        W[0] = 1.0;
        W[DD - 1] = 0.0;     // the last pivot is exactly 0
        CHECK(refusal(D, n_e, t) == "set_information: edge 2 is not positive definite (Cholesky pivot " + std::to_string(D - 1) + " <= 0)");
        // singular through the last row: rows D - 2 and D - 1 equal -> the last pivot is 1 - 1 * 1 = 0
        W[DD - 1] = 1.0; W[D * (D - 2) + D - 1] = W[D * (D - 1) + D - 2] = 1.0;
        CHECK(refusal(D, n_e, t) == "set_information: edge 2 is not positive definite (Cholesky pivot " + std::to_string(D - 1) + " <= 0)");
        W[D * (D - 2) + D - 1] = W[D * (D - 1) + D - 2] = 0.5;   // ... and positive definite again
        CHECK(refusal(D, n_e, t) == "accepted");
    }
    return 0;
}

int main() {
    if (one_width(3, 6) || one_width(6, 22)) return 1;
    static_assert(InfoPack<3>::kStride == info_stride(3) && InfoPack<6>::kStride == info_stride(6), "one definition of the stride");
    static_assert(InfoPack<3>::kPacked == 6 && InfoPack<6>::kPacked == 21, "the upper triangle");
    printf("ok %d checks\n", n_checks);
    return 0;
}
