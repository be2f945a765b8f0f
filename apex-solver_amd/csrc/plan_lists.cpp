// plan_lists.cpp -- see plan_lists.h.  Host only: index arithmetic on nt x nt maps, no device call.
#include "plan_lists.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <iterator>
#include <numeric>

#include "host_parallel.h"

namespace apex {

namespace {
// (swept 0 / 4 / 8 / 16 / 32 / all: profiles/r05_sweep_tri_inline.txt) the dataflow sweeps: in levels of at most this many columns
// a block's solve task forms its last-arriving product itself (FlowTask::mat2)
constexpr int kTriInline = 8;

double* tile_at(double* base, int64_t i) { return base + (size_t)i * kNB * kNB; }   // tile i of an array of tiles

// Nested-dissection order of the nodes of an undirected graph: recursive bisection by BFS level
// structures from a pseudo-peripheral node; the middle level is the separator and is ordered after
// both halves.  Sub-graphs of at most `leaf` nodes (or that a level structure cannot split, e.g. a
// clique) keep their natural order.  Deterministic.
void nested_dissection(const std::vector<std::vector<int>>& adj, std::vector<int> nodes, std::vector<int>& out,
                              int leaf) {
    std::sort(nodes.begin(), nodes.end());
    if ((int)nodes.size() <= leaf) { out.insert(out.end(), nodes.begin(), nodes.end()); return; }
    const int n = (int)adj.size();
    std::vector<int> mark(n, -1), dist(n, -1);
    for (int v : nodes) mark[v] = 0;
    auto bfs = [&](int src, std::vector<int>& order) {
        for (int v : nodes) dist[v] = -1;
        order.clear();
        order.push_back(src); dist[src] = 0;
        for (size_t h = 0; h < order.size(); ++h)
            for (int w : adj[order[h]])
                if (mark[w] == 0 && dist[w] < 0) { dist[w] = dist[order[h]] + 1; order.push_back(w); }
    };
    std::vector<int> order;
    bfs(nodes[0], order);
    if (order.size() < nodes.size()) {  // disconnected: order the components independently
        std::vector<int> comp(order), rest;
        std::vector<char> in(n, 0);
        for (int v : comp) in[v] = 1;
        for (int v : nodes) if (!in[v]) rest.push_back(v);
        nested_dissection(adj, comp, out, leaf);
        nested_dissection(adj, rest, out, leaf);
        return;
    }
    bfs(order.back(), order);  // from a far node: long, thin level structure
    const int depth = dist[order.back()];
    if (depth < 2) { out.insert(out.end(), nodes.begin(), nodes.end()); return; }
    std::vector<int> cnt(depth + 1, 0);
    for (int v : nodes) cnt[dist[v]]++;
    int best = 1; long bestcost = -1; long below = cnt[0];
    for (int m = 1; m < depth; ++m) {
        const long above = (long)nodes.size() - below - cnt[m];
        const long cost = std::labs(below - above) + 2L * cnt[m];  // balance + separator size
        if (bestcost < 0 || cost < bestcost) { bestcost = cost; best = m; }
        below += cnt[m];
    }
    std::vector<int> A, B, S;
    for (int v : nodes) (dist[v] < best ? A : (dist[v] > best ? B : S)).push_back(v);
    nested_dissection(adj, A, out, leaf);
    nested_dissection(adj, B, out, leaf);
    std::sort(S.begin(), S.end());
    out.insert(out.end(), S.begin(), S.end());
}
}  // namespace

std::vector<int> tile_order(int nt, const std::vector<uint8_t>& adjm, bool nd, int leaf, int n_fixed_last) {
    std::vector<int> perm(nt);
    std::iota(perm.begin(), perm.end(), 0);
    const int nf = nt - std::max(1, std::min(n_fixed_last, nt));   // tiles that take part in the dissection
    if (!nd || nf < 23) return perm;
    std::vector<std::vector<int>> adj(nf);
    for (int a = 0; a < nf; ++a)
        for (int b = 0; b < nf; ++b)
            if (a != b && adjm[(size_t)a * nt + b]) adj[a].push_back(b);
    std::vector<int> nodes(nf), ord;
    std::iota(nodes.begin(), nodes.end(), 0);
    nested_dissection(adj, nodes, ord, leaf);
    for (int pos = 0; pos < (int)ord.size(); ++pos) perm[ord[pos]] = pos;
    return perm;
}

double predict_solve_ms(int64_t n_potrf, int64_t n_trsm, int64_t n_upd, int64_t n_tiles, int n_levels) {
    const double prod = (double)n_upd + (double)n_trsm * (45.0 / 81.0) + (double)n_potrf / 3.0;
    return prod * (2.0 * kNB * kNB * kNB) / 40e12 * 1e3 + 2.0 * (double)n_tiles * kNB * kNB * 8.0 / 4.2e12 * 1e3 + 0.03 * n_levels;
}

namespace {
struct Partition {
    std::vector<int> cls, owner;   // PlanStructure::cls, owner
    int n_top_cols = 0;
    double local_frac = 1.0;
};

// Cut the elimination tree into `world` groups of subtrees plus a shared top.  Deterministic: every rank
// computes the same cut.  Starting from the roots, the heaviest subtree is split (its root joins the top, its
// children become subtrees) until a longest-processing-time assignment of the subtrees balances within 8 %.
Partition partition_columns(int nt, const PlanCols& col_rows, int rank, int world, bool own_all) {
    Partition p;
    p.cls.assign(nt, 1);
    p.owner.assign(nt, 0);
    if (world <= 1) return p;
    const int N = world;
    std::vector<int> parent(nt, -1);
    std::vector<std::vector<int>> children(nt);
    std::vector<double> sub(nt, 0.0);
    for (int K = 0; K < nt; ++K) {
        const double m = (double)col_rows[K].size();
        sub[K] += 1.0 + m + 0.5 * m * (m + 1.0);   // potrf + panel products + trailing updates of column K
        if (!col_rows[K].empty()) {
            parent[K] = col_rows[K][0];
            children[parent[K]].push_back(K);
            sub[parent[K]] += sub[K];               // parent > K: its subtree sum is complete before it is read
        }
    }
    std::vector<int> S;
    for (int K = 0; K < nt; ++K) if (parent[K] < 0) S.push_back(K);
    std::vector<char> top(nt, 0);
    std::vector<int> owner_of_root;
    auto lpt = [&](const std::vector<int>& roots, std::vector<int>* assign) {
        std::vector<int> idx(roots.size());
        std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return sub[roots[a]] > sub[roots[b]]; });
        std::vector<double> load(N, 0.0);
        if (assign) assign->assign(roots.size(), 0);
        for (int i : idx) {
            const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
            load[r] += sub[roots[i]];
            if (assign) (*assign)[i] = r;
        }
        return load;
    };
    // Walk down the tree (always splitting the heaviest subtree) and keep the cut with the smallest estimated
    // critical path: the most loaded rank's subtrees plus the replicated top, whose columns are latency-bound
    // (three dependent launches each, ~200 tile products' worth) and run at a fraction of the batched rate.
    std::vector<double> own_w(nt);
    for (int K = 0; K < nt; ++K) { const double m = (double)col_rows[K].size(); own_w[K] = 1.0 + m + 0.5 * m * (m + 1.0); }
    int n_top = 0;
    double top_cost = 0.0, best_cost = -1.0;
    std::vector<int> best_S;
    std::vector<char> best_top;
    int best_ntop = 0;
    for (;;) {
        if ((int)S.size() >= N && n_top > 0) {
            const std::vector<double> load = lpt(S, nullptr);
            const double cost = *std::max_element(load.begin(), load.end()) + top_cost;
            if (best_cost < 0.0 || cost < best_cost) { best_cost = cost; best_S = S; best_top = top; best_ntop = n_top; }
        }
        int best = -1;
        for (int i = 0; i < (int)S.size(); ++i)
            if (!children[S[i]].empty() && (best < 0 || sub[S[i]] > sub[S[best]])) best = i;
        if (best < 0 || n_top + 1 > nt / 2) break;
        const int R = S[best];
        top[R] = 1; ++n_top;
        top_cost += std::max(3.0 * own_w[R], 200.0);
        S.erase(S.begin() + best);
        S.insert(S.end(), children[R].begin(), children[R].end());
        std::sort(S.begin(), S.end());
    }
    if (best_cost < 0.0) return p;  // nothing to share (a forest, or no cut with a subtree per rank): replicated factorisation
    S = best_S; top = best_top; n_top = best_ntop;
    if (n_top == 0) return p;  // nothing shared (a forest that balances as it is): keep the replicated factorisation
    std::vector<int> assign;
    const std::vector<double> load = lpt(S, &assign);
    std::vector<int> owner(nt, -1);
    for (size_t i = 0; i < S.size(); ++i) owner[S[i]] = assign[i];
    for (int K = nt - 1; K >= 0; --K)
        if (!top[K] && owner[K] < 0) owner[K] = owner[parent[K]];
    double sum = 0.0;
    for (double l : load) sum += l;
    p.local_frac = sum > 0.0 ? load[rank] / sum : 0.0;
    // own_all: self-test: one rank plays every owner (the two-phase schedule without exchanges)
    for (int K = 0; K < nt; ++K) p.cls[K] = top[K] ? 2 : ((owner[K] == rank || own_all) ? 1 : 0);
    for (int K = 0; K < nt; ++K) p.owner[K] = top[K] ? -1 : owner[K];
    p.n_top_cols = n_top;
    return p;
}

// symbolic Cholesky at tile granularity: struct(L_K) \ {parent} merges into the parent column
PlanCols symbolic_fill(int nt, const std::vector<uint8_t>& present) {
    std::vector<std::vector<int>> col_rows(nt);
    for (int K = 0; K < nt; ++K)
        for (int I = K + 1; I < nt; ++I)
            if (present[(size_t)I * nt + K]) col_rows[K].push_back(I);
    for (int K = 0; K < nt; ++K) {
        auto& rows = col_rows[K];
        if (rows.size() < 2) continue;
        const int parent = rows[0];
        std::vector<int> merged;
        std::set_union(col_rows[parent].begin(), col_rows[parent].end(), rows.begin() + 1, rows.end(),
                       std::back_inserter(merged));
        col_rows[parent].swap(merged);
    }
    return col_rows;
}

// The slot map and the operation counts of a filled, partitioned structure (s->nt, col_rows, cls, owner, n_top_cols).
void symbolic_slots(const std::vector<uint8_t>& present, int world, PlanStructure* s) {
    const int nt = s->nt;
    const PlanCols& col_rows = s->col_rows;
    // slots: first every tile the matrix itself touches (diagonal + structural non-zeros), then the
    // tiles that exist only because of fill -- a multi-GPU all-reduce then moves the first group only
    // A distributed plan (partition_columns) keeps the tiles of the shared top columns at the end of either group:
    // touched non-top | touched top | fill non-top | fill top.
    s->slot.assign((size_t)nt * nt, -1);
    s->diag_slot.assign(nt, 0);
    s->n_slots = 0;
    const int n_owner = s->n_top_cols > 0 ? world : 1;
    s->own_range.assign(n_owner, {0, 0});
    for (int pass = 0; pass <= n_owner; ++pass) {   // owners 0..n_owner-1 (their columns contiguous), then the top
        const int64_t first = s->n_slots;
        for (int K = 0; K < nt; ++K) {
            const bool is_top = s->cls[K] == 2;
            if (pass < n_owner ? (is_top || (s->n_top_cols > 0 && s->owner[K] != pass)) : !is_top) continue;
            s->diag_slot[K] = (int)s->n_slots;
            s->slot[(size_t)K * nt + K] = (int)s->n_slots++;
            for (int I : col_rows[K])
                if (present[(size_t)I * nt + K]) s->slot[(size_t)I * nt + K] = (int)s->n_slots++;
        }
        if (pass < n_owner) s->own_range[pass] = {first, s->n_slots - first};
        if (pass == n_owner - 1) s->n_t_nt = s->n_slots;
    }
    s->n_touched = s->n_slots;
    s->own_fill.assign(n_owner, {0, 0});
    for (int pass = 0; pass <= n_owner; ++pass) {   // the fill tiles in the same order: owner by owner, then the top
        const int64_t first = s->n_slots;
        for (int K = 0; K < nt; ++K) {
            const bool is_top = s->cls[K] == 2;
            if (pass < n_owner ? (is_top || (s->n_top_cols > 0 && s->owner[K] != pass)) : !is_top) continue;
            for (int I : col_rows[K])
                if (!present[(size_t)I * nt + K]) s->slot[(size_t)I * nt + K] = (int)s->n_slots++;
        }
        if (pass < n_owner) s->own_fill[pass] = {first, s->n_slots - first};
        if (pass == n_owner - 1) s->n_f_nt = s->n_slots;
    }
    s->n_potrf = nt; s->n_trsm = 0; s->n_upd = 0;
    for (int K = 0; K < nt; ++K) {
        s->n_trsm += (int64_t)col_rows[K].size();
        s->n_upd += (int64_t)col_rows[K].size() * ((int64_t)col_rows[K].size() + 1) / 2;
    }
}

// The level groups (plan_lists.h) of a filled, partitioned structure.  parent(K) = first off-diagonal row of column K.
void level_groups(PlanStructure* s) {
    const int nt = s->nt;
    const PlanCols& col_rows = s->col_rows;
    std::vector<int> level(nt, 0);
    for (int K = 0; K < nt; ++K)
        if (!col_rows[K].empty()) level[col_rows[K][0]] = std::max(level[col_rows[K][0]], level[K] + 1);
    s->n_true_levels = 1 + *std::max_element(level.begin(), level.end());
    s->group_of.assign(nt, -1);
    for (int want = 1; want <= 2; ++want) {
        for (int lv = 0; lv < s->n_true_levels; ++lv) {
            std::vector<int> cols;
            for (int K = 0; K < nt; ++K)
                if (level[K] == lv && s->cls[K] == want) cols.push_back(K);
            if (cols.empty()) continue;
            for (int K : cols) s->group_of[K] = (int)s->group_cols.size();
            s->group_cols.push_back(std::move(cols));
        }
        if (want == 1) s->n_local_groups = (int)s->group_cols.size();
    }
    s->row_cols.assign(nt, {});
    for (int K = 0; K < nt; ++K)
        if (s->cls[K] != 0)
            for (int I : col_rows[K]) s->row_cols[I].push_back(K);
}
}  // namespace

std::vector<int> plan_owners(int nt, const std::vector<uint8_t>& present, int world) {
    Partition p = partition_columns(nt, symbolic_fill(nt, present), 0, world, false);
    return p.n_top_cols > 0 ? std::move(p.owner) : std::vector<int>();
}

PlanStructure plan_structure(int nt, const std::vector<uint8_t>& present, const PlanOptions& o) {
    PlanStructure s;
    s.nt = nt;
    s.col_rows = symbolic_fill(nt, present);
    Partition p = partition_columns(nt, s.col_rows, o.rank, o.world, o.own_all);
    s.cls = std::move(p.cls); s.owner = std::move(p.owner); s.n_top_cols = p.n_top_cols; s.local_frac = p.local_frac;
    symbolic_slots(present, o.world, &s);
    level_groups(&s);
    // what this plan is predicted to cost per solve (reported whatever follows), then the refusal rules that are host arithmetic on
    // the structure (every rank of a distributed plan decides alike): the size rule first ...
    s.predicted_ms = predict_solve_ms(s.n_potrf, s.n_trsm, s.n_upd, s.n_slots, s.n_true_levels);
    if (s.n_upd > o.max_updates) {
        s.refused = 1;
        s.message = "tile update list too large (" + std::to_string(s.n_upd) + " tile products per factorisation, limit " + std::to_string(o.max_updates) + ")";
    } else if (o.cost_limit_ms > 0.0 && s.predicted_ms > o.cost_limit_ms) {
        // (round 6) ... then the cost rule: a caller that owns a cheaper way to the same step (the matrix-free PCG,
        // Solver::set_structure) hands in what that way costs, and a plan predicted to cost more is not built
        s.refused = 3;
        char buf[160];
        snprintf(buf, sizeof buf, "predicted cost of the direct factorisation %.1f ms per solve, above the %.1f ms of the alternative", s.predicted_ms, o.cost_limit_ms);
        s.message = buf;
    }
    return s;
}

namespace {
// ---- task lists scheduled by elimination-tree LEVEL ------------------------------------------------
// Columns of one level are independent: their potrf / panel solves / trailing updates run as ONE batched launch
// each.  Two columns of a level may update the same ancestor tile: those updates are split into
// conflict-free rounds (deterministic), one launch per round.
void level_lists(const PlanStructure& s, double* tiles, double* linv, PlanLists* out) {
    const int nt = s.nt, n_levels = s.n_levels();
    const PlanCols& col_rows = s.col_rows;
    std::vector<Level>& levels = out->lv;
    auto tile_ptr = [&](int I, int J) { return tile_at(tiles, s.slot_of(I, J)); };
    levels.assign(n_levels + 1, Level());
    out->upd.reserve(s.n_upd);
    for (int lv = 0; lv < n_levels; ++lv) {
        struct U { int64_t key; int K; GemmTask t; };
        std::vector<U> us;
        for (int K : s.group_cols[lv]) {
            const auto& rows = col_rows[K];
            out->potrf.push_back({tile_ptr(K, K), tile_at(linv, K), K});
            for (int I : rows)
                if (s.group_of[I] == lv + 1) out->panel.push_back({tile_ptr(I, K), tile_ptr(I, K), tile_at(linv, K)});   // (first: see below)
            for (size_t a = 0; a < rows.size(); ++a)
                for (size_t b = 0; b <= a; ++b)
                    us.push_back({(int64_t)rows[a] * nt + rows[b], K, {tile_ptr(rows[a], rows[b]), tile_ptr(rows[a], K), tile_ptr(rows[b], K)}});
        }
        // the panel solves of the level: first the tiles whose ROW belongs to the next level (all that U1d(lv) reads), then the
        // others; by column inside each part
        for (int K : s.group_cols[lv])
            for (int I : col_rows[K])
                if (s.group_of[I] != lv + 1) out->panel.push_back({tile_ptr(I, K), tile_ptr(I, K), tile_at(linv, K)});
        std::stable_sort(us.begin(), us.end(), [](const U& x, const U& y) { return x.key < y.key; });
        // U1d: targets = DIAGONAL tiles of the next level's columns (what its potrf needs);
        // U1o: the other tiles of the next level's columns (what its panel solves need) -- on a third stream, beside the
        //      next potrf;
        // U2: targets further up the tree -- these run on the side stream, overlapped with the next
        // level's potrf and panel solves (see factor_schedule)
        // U2 itself in two parts: U2a = targets in the columns of level lv+2 -- the only ones the NEXT level's U1 updates also
        // write, so U1(lv+1) waits for U2a(lv) alone -- and U2b = everything higher, which then runs beside them.
        // ... and U2b in two: U2b1 = targets in level lv+3 (all that U2a of the NEXT level collides with), which stays on U2a's
        // stream, and U2b2 = level lv+4 and above, the bulk, on a stream of its own (factor_schedule).
        int* const part_end[4] = {&levels[lv].u1o, &levels[lv].u2a, &levels[lv].u2b1, &levels[lv].u2b2};
        for (int part = 0; part < 5; ++part) {
            std::vector<const U*> mine;
            for (const U& u : us) {
                const int tcol = (int)(u.key % nt), trow = (int)(u.key / nt);
                const int d = s.group_of[tcol] - lv;
                const int cls = d == 1 ? (trow == tcol ? 0 : 1) : (d == 2 ? 2 : (d == 3 ? 3 : 4));
                if (cls == part) mine.push_back(&u);
            }
            std::vector<int> round(mine.size(), 0);
            int n_rounds = 0;
            for (size_t i = 0; i < mine.size(); ++i) {
                round[i] = (i > 0 && mine[i]->key == mine[i - 1]->key) ? round[i - 1] + 1 : 0;
                n_rounds = std::max(n_rounds, round[i] + 1);
            }
            for (int r = 0; r < n_rounds; ++r) {
                // inside a round: by source column, so that tasks sharing operand tiles are neighbours
                std::vector<const U*> sel;
                for (size_t i = 0; i < mine.size(); ++i)
                    if (round[i] == r) sel.push_back(mine[i]);
                std::stable_sort(sel.begin(), sel.end(), [](const U* x, const U* y) { return x->K < y->K; });
                const int64_t off = (int64_t)out->upd.size();
                for (const U* u : sel) out->upd.push_back(u->t);
                out->upd_rounds.push_back({off, (int64_t)out->upd.size() - off});
            }
            if (part < 4) *part_end[part] = (int)out->upd_rounds.size();
        }
        levels[lv + 1].potrf = (int)out->potrf.size();
        levels[lv + 1].panel = (int)out->panel.size();
        levels[lv + 1].upd = (int)out->upd_rounds.size();
    }
}

// The triangular sweeps, level by level (forward by group, backward from the root group down) and as dataflow launches.
void sweep_lists(const PlanStructure& s, double* tiles, double* linv, PlanLists* sw) {
    const int nt = s.nt, n_levels = s.n_levels();
    const PlanCols &col_rows = s.col_rows, &row_cols = s.row_cols;
    std::vector<Level>& levels = sw->lv;
    auto tile_ptr = [&](int I, int J) { return tile_at(tiles, s.slot_of(I, J)); };
    for (int lv = 0; lv < n_levels; ++lv) {
        for (int K : s.group_cols[lv]) {
            // The top columns of a distributed plan are swept by every rank, and the ranks' copies of the top solution
            // must be BITWISE equal (a rank's own blocks are back-substituted from its copy, the result takes rank 0's;
            // with cond(S) ~ 1e9 a last-bit difference shows up as a 1e-11 residual).  The forward step adds into shared
            // ancestor blocks with atomics, which is order-dependent when two columns of a level run in one launch:
            // top columns therefore get one launch each.
            if (s.cls[K] == 2) levels[lv].fwd_cut.push_back((int)sw->fwd.size());
            sw->fwd.push_back({tile_at(linv, K), nullptr, K, -1});
            for (int I : col_rows[K]) sw->fwd.push_back({tile_at(linv, K), tile_ptr(I, K), K, I});
        }
        levels[lv + 1].fwd = (int)sw->fwd.size();
    }
    sw->bwd_step.assign(n_levels + 1, 0);
    for (int lv = n_levels - 1; lv >= 0; --lv) {
        for (int I : s.group_cols[lv]) {
            sw->bwd.push_back({tile_at(linv, I), nullptr, I, -1});
            for (int J : s.row_cols[I]) sw->bwd.push_back({tile_at(linv, I), tile_ptr(I, J), I, J});
        }
        sw->bwd_step[n_levels - lv] = (int)sw->bwd.size();
    }
    // both sweeps as one dataflow launch each (k_tri_fwd_flow / k_tri_bwd_flow; plans that are not distributed): level
    // by level the solve tasks of the level's blocks, then the product tasks of the tiles those solutions multiply.
    // A block's products own consecutive slots of the partial array, in the order the solve task folds them.
    std::vector<FlowTask> &ft = sw->flow_fwd, &bt = sw->flow_bwd;
    // forward: slots by block row.  In a distributed plan a shared top row takes products from this rank's columns
    // (phase 0: folded into the exchange vector, no solve) and from top columns (phase 1): the rank's sources get the
    // first slots of the row, the top sources the rest, each in column order -- so the fold of the top sources is
    // the same sequence of additions on every rank (the ranks' copies of the top solution must be bitwise equal).
    std::vector<int> first(nt + 1, 0), own_src(nt, 0);
    std::vector<std::vector<int>> slot_of(nt);
    for (int K = 0; K < nt; ++K) {
        first[K + 1] = first[K] + (int)row_cols[K].size();
        for (int J : row_cols[K]) own_src[K] += s.cls[J] == 1;
        int a = 0, b = own_src[K];
        slot_of[K].reserve(row_cols[K].size());
        for (int J : row_cols[K]) slot_of[K].push_back(s.cls[J] == 1 ? a++ : b++);
    }
    // Single-GPU plans (kTriInline, round 5): the solve task of a block forms the product of its LAST-ARRIVING source itself
    // (FlowTask::mat2 / src2 / slot2: the source solved latest, i.e. of the highest level forward, of the lowest backward) --
    // the link of the dependency chain loses a flag hop and a trip through memory; that product task leaves the list.
    // Only in the NARROW levels (at most kTriInline columns): where a level is wide the sweeps are bound by HBM and the
    // second tile of a solve task only serialises two products (final-13682 with every block inlined: sweeps 0.71 -> 0.79 ms;
    // ladybug-1723, narrow everywhere: 0.35 -> 0.28).
    const bool inl = kTriInline > 0 && !s.distributed();
    std::vector<int> fwd_inl(nt, -1), bwd_inl(nt, -1);
    if (inl)
        for (int K = 0; K < nt; ++K) {
            if ((int)s.group_cols[(size_t)s.group_of[K]].size() > kTriInline) continue;
            for (int J : row_cols[K]) if (fwd_inl[K] < 0 || s.group_of[J] >= s.group_of[fwd_inl[K]]) fwd_inl[K] = J;
            for (int I : col_rows[K]) if (bwd_inl[K] < 0 || s.group_of[I] < s.group_of[bwd_inl[K]]) bwd_inl[K] = I;
        }
    auto products_of = [&](int K) {
        for (int I : col_rows[K]) {
            if (fwd_inl[I] == K) continue;   // (formed by the solve task of block I)
            const auto& rc = row_cols[I];
            const int pos = (int)(std::lower_bound(rc.begin(), rc.end(), K) - rc.begin());
            ft.push_back({tile_ptr(I, K), K, I, first[I] + slot_of[I][pos], 0});
        }
    };
    auto fwd_solve = [&](int K) {
        FlowTask t{tile_at(linv, K), -1, K, first[K], (int)row_cols[K].size()};
        if (fwd_inl[K] >= 0) {
            const auto& rc = row_cols[K];
            const int pos = (int)(std::lower_bound(rc.begin(), rc.end(), fwd_inl[K]) - rc.begin());
            t.mat2 = tile_ptr(K, fwd_inl[K]); t.src2 = fwd_inl[K]; t.slot2 = slot_of[K][pos];
        }
        return t;
    };
    if (!s.distributed()) {
        for (int lv = 0; lv < n_levels; ++lv) {
            for (int K : s.group_cols[lv]) ft.push_back(fwd_solve(K));
            for (int K : s.group_cols[lv]) products_of(K);
        }
    } else {
        for (int lv = 0; lv < s.n_local_groups; ++lv) {          // phase 0: this rank's columns ...
            for (int K : s.group_cols[lv]) ft.push_back({tile_at(linv, K), -1, K, first[K], (int)row_cols[K].size()});
            for (int K : s.group_cols[lv]) products_of(K);
        }
        for (int lv = s.n_local_groups; lv < n_levels; ++lv)    // ... and what they add to the shared top blocks
            for (int K : s.group_cols[lv]) ft.push_back({tile_at(linv, K), -2, K, first[K], own_src[K]});
        sw->n_flow_local = (int)ft.size();
        for (int lv = s.n_local_groups; lv < n_levels; ++lv) {  // phase 1: the top columns, every rank alike
            for (int K : s.group_cols[lv])
                ft.push_back({tile_at(linv, K), -1, K, first[K] + own_src[K], (int)row_cols[K].size() - own_src[K]});
            for (int K : s.group_cols[lv]) products_of(K);
        }
    }
    if (!ft.empty()) {
        for (int K = 0; K < nt; ++K) first[K + 1] = first[K] + (int)col_rows[K].size();      // backward: by block column
        for (int lv = n_levels - 1; lv >= 0; --lv) {
            for (int I : s.group_cols[lv]) {
                FlowTask t{tile_at(linv, I), -1, I, first[I], (int)col_rows[I].size()};
                if (bwd_inl[I] >= 0) {
                    const auto& cr = col_rows[I];
                    t.mat2 = tile_ptr(bwd_inl[I], I); t.src2 = bwd_inl[I];
                    t.slot2 = (int)(std::lower_bound(cr.begin(), cr.end(), bwd_inl[I]) - cr.begin());
                }
                bt.push_back(t);
            }
            for (int I : s.group_cols[lv])
                for (int J : row_cols[I]) {
                    if (bwd_inl[J] == I) continue;   // (formed by the solve task of block J)
                    const auto& cr = col_rows[J];
                    const int pos = (int)(std::lower_bound(cr.begin(), cr.end(), I) - cr.begin());
                    bt.push_back({tile_ptr(I, J), I, J, first[J] + pos, 0});
                }
        }
    }
    int64_t a = 0, b = 0;
    for (int K = 0; K < nt; ++K) { a += (int64_t)row_cols[K].size(); b += (int64_t)col_rows[K].size(); }
    sw->n_flow_parts = (int)std::max(a, b);
}

// symmetric matvec of the PCG variant: only tiles that are non-zero before fill
void sym_lists(const PlanStructure& s, const std::vector<uint8_t>& present, PlanLists* out) {
    const int nt = s.nt;
    std::vector<SymEntry>& sym = out->sym_entries;
    out->sym_row_ptr.assign(nt + 1, 0);
    for (int I = 0; I < nt; ++I) {
        for (int J = 0; J < I; ++J)
            if (present[(size_t)I * nt + J]) sym.push_back({s.slot_of(I, J), J, 0});
        sym.push_back({s.diag_slot[I], I, 2});
        for (int I2 = I + 1; I2 < nt; ++I2)
            if (present[(size_t)I2 * nt + I]) sym.push_back({s.slot_of(I2, I), I2, 1});
        out->sym_row_ptr[I + 1] = (int)sym.size();
        for (int J = 0; J <= I; ++J)
            if (J == I || present[(size_t)I * nt + J]) out->sym_tiles.push_back({s.slot_of(I, J), I, J});
    }
}

int inc_of(const FactorUnit& u) { return (u.kind == 0 || u.kind == 3) ? kFlowUnitsPerTile : 1; }   // what a unit publishes

// `running` replays the version counters: a unit may only wait for what EARLIER units publish (the no-deadlock argument)
bool topological(const std::vector<FactorUnit>& units, size_t n_slots) {
    std::vector<int> running(n_slots, 0);
    for (const FactorUnit& u : units) {
        for (int q = 0; q < 3; ++q)
            if (u.wait_flag[q] >= 0 && running[(size_t)u.wait_flag[q]] < u.wait_val[q]) return false;
        running[(size_t)u.pub] += inc_of(u);
    }
    return true;
}

// ---- dispatch order of the dataflow units = the start order of a simulated list schedule -----------------------------------
// Workgroups are dispatched in list order, one per CU: the launch works through a WINDOW of ~256 consecutive units.
// In plain left-looking order that window fills up with units that wait for the current column while units further
// down the list -- updates whose sources were finished long ago -- cannot start: the bulk ends up serialised behind
// the critical chain, and the chain then waits for the bulk (measured: tools/flow_bench).  So the units are listed in
// the order in which a 240-processor list schedule STARTS them (a unit becomes ready when the versions it waits for
// are reached; among ready units the one with the longest remaining chain goes first).  A unit starts after its
// producers finish, hence after they started: still a topological order, re-checked below.
// src_of: per tile slot, the sources of the updates into it inside the launch.  *sim_us: the makespan of the schedule.
std::string list_schedule(const std::vector<std::vector<int>>& src_of, std::vector<FactorUnit>* units, double* sim_us) {
    constexpr int W = kFlowUnitsPerTile;
    std::vector<FactorUnit>& funits = *units;
    const size_t n_slots = src_of.size();
    const int n = (int)funits.size();
    auto cost_of = [](const FactorUnit& u) { return u.kind == 0 ? 34.0 : (u.kind == 1 ? 10.0 : (u.kind == 3 ? 30.0 : 8.0)); };   // us, with the hop
    std::vector<int> writer(n);           // which writer of its tile a unit belongs to
    {
        std::vector<int> cnt(n_slots, 0);
        for (int x = 0; x < n; ++x) { const FactorUnit& u = funits[x]; writer[x] = cnt[(size_t)u.pub] / W; cnt[(size_t)u.pub] += inc_of(u); }
    }
    // remaining chain (bottom level) through the tile-version nodes (slot, writer)
    std::vector<int> node0(n_slots + 1, 0);
    for (size_t sl = 0; sl < n_slots; ++sl) node0[sl + 1] = node0[sl] + (int)src_of[sl].size() + 1;
    std::vector<double> node_bl((size_t)node0[n_slots], 0.0), bl(n, 0.0);
    for (int x = n - 1; x >= 0; --x) {
        const FactorUnit& u = funits[x];
        bl[x] = cost_of(u) + node_bl[(size_t)node0[(size_t)u.pub] + writer[x]];
        for (int q = 0; q < 3; ++q)
            if (u.wait_flag[q] >= 0) {
                double& nb = node_bl[(size_t)node0[(size_t)u.wait_flag[q]] + u.wait_val[q] / W - 1];
                nb = std::max(nb, bl[x]);
            }
    }
    // event simulation
    std::vector<std::vector<std::pair<int, int>>> waiters(n_slots);   // per flag: (value, unit)
    std::vector<int> pending(n, 0), ver_sim(n_slots, 0), order;
    order.reserve(n);
    for (int x = 0; x < n; ++x) {
        const FactorUnit& u = funits[x];
        for (int q = 0; q < 3; ++q)
            if (u.wait_flag[q] >= 0) { waiters[(size_t)u.wait_flag[q]].push_back({u.wait_val[q], x}); ++pending[x]; }
    }
    std::vector<size_t> woke(n_slots, 0);
    for (auto& wl : waiters) std::sort(wl.begin(), wl.end());
    auto worse = [&](int a, int b) { return bl[a] != bl[b] ? bl[a] < bl[b] : a > b; };   // heap top = longest chain, then list order
    std::vector<int> ready;
    for (int x = 0; x < n; ++x) if (pending[x] == 0) ready.push_back(x);
    std::make_heap(ready.begin(), ready.end(), worse);
    std::vector<std::pair<double, int>> running_ev;   // min-heap of (finish time, unit)
    auto later = [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a > b; };
    int free_p = 240;
    double now = 0.0;
    while ((int)order.size() < n) {
        while (free_p > 0 && !ready.empty()) {
            std::pop_heap(ready.begin(), ready.end(), worse);
            const int x = ready.back(); ready.pop_back();
            order.push_back(x); --free_p;
            running_ev.push_back({now + cost_of(funits[x]), x});
            std::push_heap(running_ev.begin(), running_ev.end(), later);
        }
        if (running_ev.empty()) return "internal error: the dataflow units do not form a schedule";
        std::pop_heap(running_ev.begin(), running_ev.end(), later);
        const std::pair<double, int> ev = running_ev.back(); running_ev.pop_back();
        now = ev.first; ++free_p;
        const FactorUnit& u = funits[ev.second];
        const size_t f = (size_t)u.pub;
        ver_sim[f] += inc_of(u);
        while (woke[f] < waiters[f].size() && waiters[f][woke[f]].first <= ver_sim[f]) {
            const int x = waiters[f][woke[f]++].second;
            if (--pending[x] == 0) { ready.push_back(x); std::push_heap(ready.begin(), ready.end(), worse); }
        }
    }
    *sim_us = now;
    std::vector<FactorUnit> sorted(n);
    for (int i = 0; i < n; ++i) sorted[i] = funits[order[i]];
    funits.swap(sorted);
    return topological(funits, n_slots) ? "" : "internal error: the scheduled dataflow order is not topological";
}

// ---- the trailing level groups [gf, g1) of a phase as ONE dataflow launch (k_factor_flow, chol_kernels.hip) ----------------
// Units in left-looking order: per column of the region the updates into its tiles (per target in source order = the
// order of the level launches), its potrf, its panel solves; last the updates into tiles whose column is outside
// the launch (the local phase of a distributed plan adding to the shared top).  Checked topological (`running`), then put in
// list-schedule order (list_schedule).
std::string flow_units(const PlanStructure& s, int gf, int g1, double* tiles, double* linv, std::vector<FactorUnit>* units, double* sim_us) {
    const int nt = s.nt;
    const PlanCols& col_rows = s.col_rows;
    auto tile_ptr = [&](int I, int J) { return tile_at(tiles, s.slot_of(I, J)); };
    std::vector<FactorUnit>& funits = *units;
    funits.clear();
    std::vector<int> cols;
    std::vector<char> in_reg(nt, 0);
    for (int grp = gf; grp < g1; ++grp)
        for (int K : s.group_cols[grp]) { cols.push_back(K); in_reg[K] = 1; }
    std::vector<std::vector<int>> src_of((size_t)s.n_slots);
    std::vector<std::pair<int, int>> outside;   // (J, I) of targets whose column is not in the launch
    for (int K : cols) {
        const auto& rows = col_rows[K];
        for (size_t a = 0; a < rows.size(); ++a)
            for (size_t b = 0; b <= a; ++b) {
                std::vector<int>& v = src_of[(size_t)s.slot_of(rows[a], rows[b])];
                if (v.empty() && !in_reg[rows[b]]) outside.push_back({rows[b], rows[a]});
                v.push_back(K);
            }
    }
    std::sort(outside.begin(), outside.end());
    constexpr int W = kFlowUnitsPerTile;
    auto n_upd_of = [&](int st) { return (int)src_of[(size_t)st].size(); };
    // An update whose target column lies TWO level groups or more above its source column is not on the chain
    // potrf -> panel solves -> updates of the next group's tiles -> potrf: it runs as ONE whole-tile unit (kind 3, the level
    // kernels' rate per CU) instead of nine 48 x 48 units made for latency (round 5; "factor_flow_tile" 0: nine everywhere).
    auto emit_updates = [&](int I, int J) {
        const int st = s.slot_of(I, J);
        for (int n = 0; n < n_upd_of(st); ++n) {
            const int K = src_of[(size_t)st][n], sa = s.slot_of(I, K), sb = s.slot_of(J, K);
            const bool whole = s.group_of[J] > s.group_of[K] + 1;
            if (whole) {
                funits.push_back(FactorUnit{tile_ptr(I, J), tile_ptr(I, K), tile_ptr(J, K), {n > 0 ? st : -1, sa, sb},
                                {W * n, W * (n_upd_of(sa) + 1), W * (n_upd_of(sb) + 1)}, st, 3, 0, 0});
                continue;
            }
            for (int sp = 0; sp < W; ++sp)
                funits.push_back(FactorUnit{tile_ptr(I, J), tile_ptr(I, K), tile_ptr(J, K), {n > 0 ? st : -1, sa, sb},
                                {W * n, W * (n_upd_of(sa) + 1), W * (n_upd_of(sb) + 1)}, st, 2, sp, 0});
        }
    };
    for (int J : cols) {
        const int sd = s.slot_of(J, J), nd = n_upd_of(sd);
        emit_updates(J, J);
        for (int I : col_rows[J]) emit_updates(I, J);
        funits.push_back(FactorUnit{tile_ptr(J, J), tile_at(linv, J), nullptr, {nd > 0 ? sd : -1, -1, -1}, {W * nd, 0, 0}, sd, 0, J, 0});
        for (int I : col_rows[J]) {
            const int st = s.slot_of(I, J), n = n_upd_of(st);
            for (int sp = 0; sp < W; ++sp)
                funits.push_back(FactorUnit{tile_ptr(I, J), tile_ptr(I, J), tile_at(linv, J), {n > 0 ? st : -1, -1, sd}, {W * n, 0, W * (nd + 1)}, st, 1, sp, 0});
        }
    }
    for (const auto& t : outside) emit_updates(t.second, t.first);
    if (!topological(funits, (size_t)s.n_slots)) return "internal error: a dataflow factorisation unit waits for a later one";
    return list_schedule(src_of, units, sim_us);
}

// Where the dataflow launch of each phase (local groups / top groups) starts.  "factor_flow" > 0: the trailing groups with at
// most that many columns (and "factor_flow_rows" off-diagonal tiles per column).  < 0 (default): by a model -- the level
// launches cost max(80 us of launch chain, 0.14 us per tile product) per group, the dataflow launch what its list schedule
// says (it runs a tile product on one CU at a time and reads every operand past the L2: ~0.22 us per product with all CUs
// busy, but a level costs it ~55 us of chain instead of 80); the start with the smallest sum wins, no launch if none beats
// the level launches.  The units of both phases go to out->units, where they start and end to out->flow.
std::string flow_regions(const PlanStructure& s, int flow_cols, int flow_rows, double* tiles, double* linv, PlanLists* out) {
    const int n_levels = s.n_levels();
    const PlanCols& col_rows = s.col_rows;
    auto level_us = [&](int grp) {
        double prod = 0.0;
        for (int K : s.group_cols[grp]) { const double m = (double)col_rows[K].size(); prod += m + 0.5 * m * (m + 1.0); }
        // (round 5: by the timeline a middle level of final-13682 really takes 140-250 us, ~90 + 0.11 prod -- but the launch's
        // own simulated time is as optimistic there, and the starts this pair of models picks ARE the measured optima:
        // profiles/r05_flow_dyn_sweep.txt.  Both left as they are.)
        return std::max(80.0, 0.14 * prod);
    };
    for (int ph = 0; ph < 2; ++ph) {
        const int g0 = ph == 0 ? 0 : s.n_local_groups, g1 = ph == 0 ? s.n_local_groups : n_levels;
        PlanLists::Flow& fl = out->flow[ph];
        fl = PlanLists::Flow{g1, g1, (int)out->units.size(), 0, 0.0};
        if (flow_cols == 0 || g1 - g0 < 2) continue;
        int best_gf = g1;
        if (flow_cols > 0) {
            while (best_gf > g0) {
                const std::vector<int>& cols = s.group_cols[best_gf - 1];
                bool ok = (int)cols.size() <= flow_cols;
                for (int K : cols) ok = ok && (int)col_rows[K].size() <= flow_rows;
                if (!ok) break;
                --best_gf;
            }
        } else {
            double level_tail = 0.0, best_total = 0.0;   // cost of the groups [gf, g1) by level launches; best (level head dropped: common)
            int64_t units = 0;
            // the candidate starts, from the top down, with what the level launches would cost from there
            std::vector<std::pair<int, double>> cands;
            for (int gf = g1 - 1; gf >= g0; --gf) {
                bool ok = (int)s.group_cols[gf].size() <= 64;
                for (int K : s.group_cols[gf]) {
                    const int64_t m = (int64_t)col_rows[K].size();
                    ok = ok && m <= 96;
                    units += 1 + kFlowUnitsPerTile * (m + m * (m + 1) / 2);
                }
                if (!ok || units > 400000) break;   // (the model is evaluated per candidate start: keep plan building in the milliseconds)
                level_tail += level_us(gf);
                if (g1 - gf >= 2) cands.push_back({gf, level_tail});
            }
            // The model of every candidate (its units in list-scheduled order, simulated) was half of the plan's build time on
            // final-13682 -- 50 of 95 ms, evaluated one after the other.  They are independent: a batch at a time on the host
            // pool, the choice replayed over the batch in the old order (same rule, same start), the winner's units built once
            // more at the end (round 5).
            const int batch = std::max(1, std::min<int>(8, (int)host_threads()));
            bool past = false;
            for (size_t c0 = 0; c0 < cands.size() && !past; c0 += (size_t)batch) {
                const size_t c1 = std::min(cands.size(), c0 + (size_t)batch);
                std::vector<double> sims(c1 - c0, 0.0);
                std::vector<std::string> errs(c1 - c0);
                parallel_rows((int64_t)(c1 - c0), [&](int64_t i) {
                    std::vector<FactorUnit> scratch;
                    errs[(size_t)i] = flow_units(s, cands[c0 + (size_t)i].first, g1, tiles, linv, &scratch, &sims[(size_t)i]);
                }, 1);
                for (size_t i = 0; i < c1 - c0 && !past; ++i) {
                    if (!errs[i].empty()) return errs[i];
                    // gain of starting the launch at gf = what the level launches would have cost from there - the launch
                    const double gain = cands[c0 + i].second - (sims[i] + 15.0);
                    if (gain > best_total) { best_total = gain; best_gf = cands[c0 + i].first; }
                    else if (gain < best_total - 300.0) past = true;   // past the optimum: the launch is swallowing throughput-bound levels
                }
            }
        }
        if (g1 - best_gf < 2) continue;   // no launch, or a single group: nothing to chain
        std::vector<FactorUnit> best_units;
        double sim = 0.0;
        const std::string e = flow_units(s, best_gf, g1, tiles, linv, &best_units, &sim);
        if (!e.empty()) return e;
        fl.g0 = best_gf; fl.n = (int)best_units.size(); fl.sim_us = sim;
        out->units.insert(out->units.end(), best_units.begin(), best_units.end());
    }
    return "";
}

// ---- first writers of the fill tiles (plan_lists.h, first_ok) ------------------------------------------------------------
// Two execution orders exist: the level launches alone (the lists of every level, in list order) and the level launches of
// the levels below a dataflow launch followed by its units (in unit order: the writers of a tile are chained in that order).
// A fill tile's first writer is flagged in both; touched tiles hold S and are never "first written".
void flag_first_writers(const PlanStructure& s, const double* tiles, PlanLists* out) {
    const PlanLists::Flow* flow = out->flow;
    out->first_ok = false;
    if (s.distributed() || s.n_slots <= s.n_touched || flow[1].n != 0) return;
    auto slot_of_ptr = [&](const double* c) { return (int64_t)((c - tiles) / (ptrdiff_t)(kNB * kNB)); };
    std::vector<char> seen_a((size_t)s.n_slots, 0);
    for (int64_t sl = 0; sl < s.n_touched; ++sl) seen_a[(size_t)sl] = 1;
    std::vector<char> seen_b(seen_a);
    int64_t upd_before_flow = (int64_t)out->upd.size();   // the level lists that run in front of the dataflow launch
    if (flow[0].n > 0) {
        const int r = out->lv[(size_t)flow[0].g0].upd;
        if (r < (int)out->upd_rounds.size()) upd_before_flow = out->upd_rounds[(size_t)r].first;
    }
    for (size_t q = 0; q < out->upd.size(); ++q) {
        const int64_t sl = slot_of_ptr(out->upd[q].C);
        if ((int64_t)q < upd_before_flow) seen_b[(size_t)sl] = 1;
        if (!seen_a[(size_t)sl]) { seen_a[(size_t)sl] = 1; out->upd[q].C = reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(out->upd[q].C) | 1); }
    }
    // the dataflow units: the first (tile, writer) of a tile not written below the launch; its nine block units share C, A, B
    std::vector<const double*> first_a((size_t)s.n_slots, nullptr), first_b((size_t)s.n_slots, nullptr);
    for (FactorUnit& u : out->units) {
        if (u.kind != 2 && u.kind != 3) continue;
        const int64_t sl = slot_of_ptr(u.C);
        if (!seen_b[(size_t)sl]) { seen_b[(size_t)sl] = 1; first_a[(size_t)sl] = u.A; first_b[(size_t)sl] = u.B; }
        if (first_a[(size_t)sl] == u.A && first_b[(size_t)sl] == u.B && first_a[(size_t)sl] != nullptr) u.kind |= kFlowFirstWriter;
    }
    bool all = true;
    for (int64_t sl = s.n_touched; sl < s.n_slots; ++sl) all = all && seen_a[(size_t)sl] && (flow[0].n == 0 || seen_b[(size_t)sl]);
    if (all) out->first_ok = true;
    else {   // (a fill tile without an update: cannot be -- take the flags back and clear everything as before)
        for (GemmTask& t : out->upd) t.C = reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(t.C) & ~uintptr_t(7));
        for (FactorUnit& u : out->units) u.kind &= 15;
    }
}
}  // namespace

std::string build_plan_lists(const PlanStructure& s, const std::vector<uint8_t>& present, const PlanOptions& o, double* tiles, double* linv, PlanLists* out) {
    *out = PlanLists();
    if (s.refused) return s.message;
    level_lists(s, tiles, linv, out);
    sweep_lists(s, tiles, linv, out);
    sym_lists(s, present, out);
    // The second side stream (factor_schedule), for the whole plan or not at all: it pays where a level carries a bulk worth
    // overlapping (final-13682: ~1,000 tile products per level, 7.95 -> 7.5 ms; synthetic-10k 6.4 -> 6.1) and costs where the
    // levels are small and the factorisation is its launch chain (the ladybug / venice shapes, ~100 products per level: one
    // more stream is one more edge per level, 3.1 -> 3.5 ms).
    out->two_side_plan = o.two_side == 2 || (o.two_side == 1 && (int64_t)out->upd.size() >= 256 * (int64_t)s.n_levels());
    const std::string e = flow_regions(s, o.flow_cols, o.flow_rows, tiles, linv, out);
    if (!e.empty()) return e;
    flag_first_writers(s, tiles, out);
    // The updates of diagonal tiles (PlanOptions::diag_lower), counted as they run: the level lists in front of each phase's
    // dataflow launch, then its units.  A diagonal tile is a tile of S, so none of them may be a first writer.
    for (int ph = 0; ph < 2; ++ph) {
        const int g0 = ph == 0 ? 0 : s.n_local_groups;
        const size_t r0 = (size_t)out->lv[(size_t)g0].upd, r1 = (size_t)out->lv[(size_t)out->flow[ph].g0].upd;
        for (size_t r = r0; r < r1 && r < out->upd_rounds.size(); ++r)
            for (int64_t q = out->upd_rounds[r].first; q < out->upd_rounds[r].first + out->upd_rounds[r].second; ++q) {
                const GemmTask& t = out->upd[(size_t)q];
                if (t.A != t.B) continue;
                if (reinterpret_cast<uintptr_t>(t.C) & 1) return "internal error: the first writer of a fill tile targets a diagonal tile";
                ++out->n_diag_upd[0];
            }
    }
    for (const FactorUnit& u : out->units) {
        const int kind = u.kind & 15;
        if ((kind != 2 && kind != 3) || u.A != u.B || (kind == 2 && u.strip != 0)) continue;
        if (u.kind & kFlowFirstWriter) return "internal error: the first writer of a fill tile targets a diagonal tile";
        ++out->n_diag_upd[1];
    }
    return "";
}

}  // namespace apex
