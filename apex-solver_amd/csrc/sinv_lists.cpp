// sinv_lists.cpp -- see sinv_lists.h
#include "sinv_lists.h"

#include <algorithm>

namespace apex {

std::string build_sinv_lists(int nt, const int* slot, const std::vector<std::vector<int>>& group_cols, SinvLists* out) {
    *out = SinvLists();
    auto at = [&](int I, int J) { return slot[(size_t)I * nt + J]; };
    std::vector<std::vector<int>> col_rows(nt);
    for (int K = 0; K < nt; ++K)
        for (int I = K + 1; I < nt; ++I)
            if (at(I, K) >= 0) col_rows[K].push_back(I);
    for (int K = 0; K < nt; ++K) {
        const auto& rows = col_rows[K];
        for (size_t a = 0; a < rows.size(); ++a)
            for (size_t b = 0; b < a; ++b)
                if (at(rows[a], rows[b]) < 0)
                    return "tile (" + std::to_string(rows[a]) + ", " + std::to_string(rows[b]) + ") of column " + std::to_string(K) +
                           "'s rows is not a tile of the factor: the tile structure is not closed under fill";
    }
    auto& tasks = out->tasks;
    auto& prods = out->prods;
    auto L = [&](int I, int J) { return SinvRef{kSinvL, at(I, J)}; };
    auto Z = [&](int I, int J) { return SinvRef{kSinvZ, at(I, J)}; };
    auto Linv = [](int j) { return SinvRef{kSinvLinv, j}; };
    for (int gi = (int)group_cols.size() - 1; gi >= 0; --gi) {
        const auto& cols = group_cols[gi];
        std::array<int, 4> g;
        std::vector<int64_t> ybase(cols.size());
        int64_t ny = 0;
        for (size_t c = 0; c < cols.size(); ++c) { ybase[c] = ny; ny += (int64_t)col_rows[cols[c]].size(); }
        out->y_max = std::max(out->y_max, ny);
        auto Y = [&](size_t c, size_t a) { return SinvRef{kSinvY, ybase[c] + (int64_t)a}; };
        g[0] = (int)tasks.size();
        for (size_t c = 0; c < cols.size(); ++c) {   // Y_r = L_rj Linv_j
            const int j = cols[c];
            for (size_t a = 0; a < col_rows[j].size(); ++a) {
                tasks.push_back({Y(c, a), (int)prods.size(), 1});
                prods.push_back({L(col_rows[j][a], j), Linv(j), 0});
            }
        }
        g[1] = (int)tasks.size();
        for (size_t c = 0; c < cols.size(); ++c) {   // Z_rj = - sum_s Z~_rs Y_s
            const int j = cols[c];
            const auto& rows = col_rows[j];
            for (size_t a = 0; a < rows.size(); ++a) {
                const int r = rows[a];
                tasks.push_back({Z(r, j), (int)prods.size(), (int)rows.size()});
                for (size_t b = 0; b < rows.size(); ++b) {
                    const int s = rows[b];
                    if (r >= s) prods.push_back({Z(r, s), Y(c, b), kSinvNeg});
                    else prods.push_back({Z(s, r), Y(c, b), kSinvNeg | kSinvTransA});
                }
            }
        }
        g[2] = (int)tasks.size();
        for (size_t c = 0; c < cols.size(); ++c) {   // Z_jj = Linv_j^T Linv_j - sum_r Y_r^T Z_rj
            const int j = cols[c];
            const auto& rows = col_rows[j];
            tasks.push_back({Z(j, j), (int)prods.size(), 1 + (int)rows.size()});
            prods.push_back({Linv(j), Linv(j), kSinvTransA});
            for (size_t a = 0; a < rows.size(); ++a) prods.push_back({Y(c, a), Z(rows[a], j), kSinvNeg | kSinvTransA});
        }
        g[3] = (int)tasks.size();
        for (int k = 0; k < 3; ++k)
            for (int t = g[k]; t < g[k + 1]; ++t) out->n[k] += tasks[t].count;
        out->groups.push_back(g);
    }
    return "";
}

}  // namespace apex
