// pg2_lists.h -- the incident-edge lists of the row-owned SE2 assembly (k_pg2_assemble).  Plain host C++.
//
// CSR over the vertices (internal numbering): list v holds, in ascending edge index, every edge with v as an
// endpoint; a self-loop appears once.  The owner of the off-diagonal block of an edge is its larger endpoint.
#pragma once
#include <stdint.h>

#include <vector>

namespace apex {

struct IncidentLists {
    std::vector<int> ptr;        // [n_v + 1]
    std::vector<uint32_t> edge;  // [ptr[n_v]]
};

// false when an endpoint is out of range or the list would not fit an int
inline bool build_incident_lists(int64_t n_v, int64_t n_e, const uint32_t* e_from, const uint32_t* e_to, IncidentLists* out) {
    if (n_v < 0 || n_e < 0 || 2 * n_e > 2000000000LL) return false;
    out->ptr.assign((size_t)n_v + 1, 0);
    for (int64_t e = 0; e < n_e; ++e) {
        if (e_from[e] >= (uint64_t)n_v || e_to[e] >= (uint64_t)n_v) return false;
        out->ptr[e_from[e] + 1]++;
        if (e_to[e] != e_from[e]) out->ptr[e_to[e] + 1]++;
    }
    for (int64_t v = 0; v < n_v; ++v) out->ptr[v + 1] += out->ptr[v];
    out->edge.assign((size_t)out->ptr[n_v], 0);
    std::vector<int> fill(out->ptr.begin(), out->ptr.end() - 1);
    for (int64_t e = 0; e < n_e; ++e) {   // ascending e: every list comes out sorted
        out->edge[fill[e_from[e]]++] = (uint32_t)e;
        if (e_to[e] != e_from[e]) out->edge[fill[e_to[e]]++] = (uint32_t)e;
    }
    return true;
}

}  // namespace apex
