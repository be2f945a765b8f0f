// tile_plan.hip -- see tile_plan.h
#include "tile_plan.h"
#include "host_parallel.h"

#include <chrono>
#include <thread>

#include <stdlib.h>

#include <math.h>

#include <algorithm>
#include <numeric>

namespace apex {

static double* tile_at(double* base, int64_t i) { return base + (size_t)i * kNB * kNB; }   // tile i of an array of tiles

// Nested-dissection order of the nodes of an undirected graph: recursive bisection by BFS level
// structures from a pseudo-peripheral node; the middle level is the separator and is ordered after
// both halves.  Sub-graphs of at most `leaf` nodes (or that a level structure cannot split, e.g. a
// clique) keep their natural order.  Deterministic.
static void nested_dissection(const std::vector<std::vector<int>>& adj, std::vector<int> nodes, std::vector<int>& out,
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

std::vector<int> TilePlan::order(int nt, const std::vector<uint8_t>& adjm, bool nd, int leaf, int n_fixed_last) {
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

void TilePlan::release() {
    for (int i = 0; i < kGraphs; ++i) {   // the graph execs first: their nodes point into the buffers freed below
        if (graph_exec_[i]) { (void)hipGraphExecDestroy(graph_exec_[i]); graph_exec_[i] = nullptr; }
        graph_failed_[i] = false;
    }
    inverse_.release();
    tiles_written();
    static_cast<TilePlanMemory&>(*this) = TilePlanMemory();   // frees every device and pinned block of the plan
    n_flow_tasks_ = 0; flow_n_[0] = flow_n_[1] = 0; flow_on_ = true; flow_gave_up_ = false;
    flow_err_host_dev_ = nullptr;
    for (hipEvent_t& ev : pcg_ev_) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
    if (occ_stream_) { (void)hipStreamSynchronize(occ_stream_); (void)hipStreamDestroy(occ_stream_); occ_stream_ = nullptr; }
    for (const auto& evs : ev_) for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    ev_.clear();
}

TilePlan::~TilePlan() {
    release();
    for (hipStream_t s : {side_, side2_, so_})
        if (s) (void)hipStreamDestroy(s);
}

// Cut the elimination tree into part_world_ groups of subtrees plus a shared top.  Deterministic: every rank
// computes the same cut.  Starting from the roots, the heaviest subtree is split (its root joins the top, its
// children become subtrees) until a longest-processing-time assignment of the subtrees balances within 8 %.
void TilePlan::partition_columns(const std::vector<std::vector<int>>& col_rows) {
    cls_h_.assign(nt_, 1);
    owner_h_.assign(nt_, 0);
    n_top_cols_ = 0; local_frac_ = 1.0;
    if (part_world_ <= 1) return;
    const int N = part_world_;
    std::vector<int> parent(nt_, -1);
    std::vector<std::vector<int>> children(nt_);
    std::vector<double> sub(nt_, 0.0);
    for (int K = 0; K < nt_; ++K) {
        const double m = (double)col_rows[K].size();
        sub[K] += 1.0 + m + 0.5 * m * (m + 1.0);   // potrf + panel products + trailing updates of column K
        if (!col_rows[K].empty()) {
            parent[K] = col_rows[K][0];
            children[parent[K]].push_back(K);
            sub[parent[K]] += sub[K];               // parent > K: its subtree sum is complete before it is read
        }
    }
    std::vector<int> S;
    for (int K = 0; K < nt_; ++K) if (parent[K] < 0) S.push_back(K);
    std::vector<char> top(nt_, 0);
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
    std::vector<double> own_w(nt_);
    for (int K = 0; K < nt_; ++K) { const double m = (double)col_rows[K].size(); own_w[K] = 1.0 + m + 0.5 * m * (m + 1.0); }
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
        if (best < 0 || n_top + 1 > nt_ / 2) break;
        const int R = S[best];
        top[R] = 1; ++n_top;
        top_cost += std::max(3.0 * own_w[R], 200.0);
        S.erase(S.begin() + best);
        S.insert(S.end(), children[R].begin(), children[R].end());
        std::sort(S.begin(), S.end());
    }
    if (best_cost < 0.0) return;  // nothing to share (a forest, or no cut with a subtree per rank): replicated factorisation
    S = best_S; top = best_top; n_top = best_ntop;
    if (n_top == 0) return;  // nothing shared (a forest that balances as it is): keep the replicated factorisation
    std::vector<int> assign;
    const std::vector<double> load = lpt(S, &assign);
    std::vector<int> owner(nt_, -1);
    for (size_t i = 0; i < S.size(); ++i) owner[S[i]] = assign[i];
    for (int K = nt_ - 1; K >= 0; --K)
        if (!top[K] && owner[K] < 0) owner[K] = owner[parent[K]];
    double sum = 0.0;
    for (double l : load) sum += l;
    local_frac_ = sum > 0.0 ? load[part_rank_] / sum : 0.0;
    const bool own_all = own_all_;  // self-test: one rank plays every owner (the two-phase schedule without exchanges)
    for (int K = 0; K < nt_; ++K) cls_h_[K] = top[K] ? 2 : ((owner[K] == part_rank_ || own_all) ? 1 : 0);
    for (int K = 0; K < nt_; ++K) owner_h_[K] = top[K] ? -1 : owner[K];
    n_top_cols_ = n_top;
}

// symbolic Cholesky at tile granularity: struct(L_K) \ {parent} merges into the parent column
static std::vector<std::vector<int>> symbolic_fill(int nt, const std::vector<uint8_t>& present) {
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

// The owner rank of every tile column (-1: shared top) that build() will arrive at for the same structure and
// partition; empty when the plan will not be distributed.  Host arithmetic only.
std::vector<int> TilePlan::preview_owners(int nt, const std::vector<uint8_t>& present) {
    const int keep = nt_;
    nt_ = nt;
    partition_columns(symbolic_fill(nt, present));
    nt_ = keep;
    return n_top_cols_ > 0 ? owner_h_ : std::vector<int>();
}

// host half of build(): symbolic fill, partition, slot map.  Returns the filled column structure.
std::vector<std::vector<int>> TilePlan::symbolic_slots(const std::vector<uint8_t>& present) {
    std::vector<std::vector<int>> col_rows = symbolic_fill(nt_, present);
    // slots: first every tile the matrix itself touches (diagonal + structural non-zeros), then the
    // tiles that exist only because of fill -- a multi-GPU all-reduce then moves the first group only
    // A distributed plan (partition_columns) keeps the tiles of the shared top columns at the end of either group:
    // touched non-top | touched top | fill non-top | fill top.
    partition_columns(col_rows);
    slot_h_.assign((size_t)nt_ * nt_, -1);
    diag_slot_h_.assign(nt_, 0);
    n_slots_ = 0;
    const int n_owner = n_top_cols_ > 0 ? part_world_ : 1;
    own_range_.assign(n_owner, {0, 0});
    for (int pass = 0; pass <= n_owner; ++pass) {   // owners 0..n_owner-1 (their columns contiguous), then the top
        const int64_t first = n_slots_;
        for (int K = 0; K < nt_; ++K) {
            const bool is_top = cls_h_[K] == 2;
            if (pass < n_owner ? (is_top || (n_top_cols_ > 0 && owner_h_[K] != pass)) : !is_top) continue;
            diag_slot_h_[K] = (int)n_slots_;
            slot_h_[(size_t)K * nt_ + K] = (int)n_slots_++;
            for (int I : col_rows[K])
                if (present[(size_t)I * nt_ + K]) slot_h_[(size_t)I * nt_ + K] = (int)n_slots_++;
        }
        if (pass < n_owner) own_range_[pass] = {first, n_slots_ - first};
        if (pass == n_owner - 1) n_t_nt_ = n_slots_;
    }
    n_touched_ = n_slots_;
    own_fill_.assign(n_owner, {0, 0});
    for (int pass = 0; pass <= n_owner; ++pass) {   // the fill tiles in the same order: owner by owner, then the top
        const int64_t first = n_slots_;
        for (int K = 0; K < nt_; ++K) {
            const bool is_top = cls_h_[K] == 2;
            if (pass < n_owner ? (is_top || (n_top_cols_ > 0 && owner_h_[K] != pass)) : !is_top) continue;
            for (int I : col_rows[K])
                if (!present[(size_t)I * nt_ + K]) slot_h_[(size_t)I * nt_ + K] = (int)n_slots_++;
        }
        if (pass < n_owner) own_fill_[pass] = {first, n_slots_ - first};
        if (pass == n_owner - 1) n_f_nt_ = n_slots_;
    }
    n_potrf_ = nt_; n_trsm_ = 0; n_upd_ = 0;
    for (int K = 0; K < nt_; ++K) {
        n_trsm_ += (int64_t)col_rows[K].size();
        n_upd_ += (int64_t)col_rows[K].size() * ((int64_t)col_rows[K].size() + 1) / 2;
    }
    return col_rows;
}

// The level groups (tile_plan.h, Groups).  parent(K) = first off-diagonal row of column K.
TilePlan::Groups TilePlan::level_groups(const Cols& col_rows) const {
    Groups g;
    std::vector<int> level(nt_, 0);
    for (int K = 0; K < nt_; ++K)
        if (!col_rows[K].empty()) level[col_rows[K][0]] = std::max(level[col_rows[K][0]], level[K] + 1);
    g.n_true_levels = 1 + *std::max_element(level.begin(), level.end());
    g.group_of.assign(nt_, -1);
    for (int want = 1; want <= 2; ++want) {
        for (int lv = 0; lv < g.n_true_levels; ++lv) {
            std::vector<int> cols;
            for (int K = 0; K < nt_; ++K)
                if (level[K] == lv && cls_h_[K] == want) cols.push_back(K);
            if (cols.empty()) continue;
            for (int K : cols) g.group_of[K] = (int)g.cols.size();
            g.cols.push_back(std::move(cols));
        }
        if (want == 1) g.n_local = (int)g.cols.size();
    }
    g.row_cols.assign(nt_, {});
    for (int K = 0; K < nt_; ++K)
        if (cls_h_[K] != 0)
            for (int I : col_rows[K]) g.row_cols[I].push_back(K);
    return g;
}

void TilePlan::build_symbolic(int nt, const std::vector<uint8_t>& present) {
    nt_ = nt;
    n_levels_ = n_local_groups_ = level_groups(symbolic_slots(present)).n_true_levels;
}

// what this plan is predicted to cost per solve (reported whatever follows), then the refusal rules that are host arithmetic on
// the structure (every rank of a distributed plan decides alike): the size rule first ...
std::string TilePlan::refuse_by_size_or_cost(int n_true_levels) {
    predicted_ms_ = predict_solve_ms(n_potrf_, n_trsm_, n_upd_, n_slots_, n_true_levels);
    if (n_upd_ > max_updates_) { refused_ = 1; return "tile update list too large (" + std::to_string(n_upd_) + " tile products per factorisation, limit " + std::to_string(max_updates_) + ")"; }
    // (round 6) ... then the cost rule: a caller that owns a cheaper way to the same step (the matrix-free PCG,
    // Solver::set_structure) hands in what that way costs, and a plan predicted to cost more is not built
    if (cost_limit_ms_ > 0.0 && predicted_ms_ > cost_limit_ms_) {
        refused_ = 3;
        char buf[160];
        snprintf(buf, sizeof buf, "predicted cost of the direct factorisation %.1f ms per solve, above the %.1f ms of the alternative", predicted_ms_, cost_limit_ms_);
        return buf;
    }
    return "";
}

std::string TilePlan::refuse_by_memory() {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const double need = (double)(n_slots_ + nt_) * kNB * kNB * 8.0;
    if (need <= 0.9 * (double)free_b) return "";
    refused_ = 2;
    return "the tile matrix needs " + std::to_string(need / 1e9) + " GB; only " + std::to_string(free_b / 1e9) + " GB free";
}

#define TP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return std::string("HIP error in " #expr ": ") + hipGetErrorString(_e); } while (0)

std::string TilePlan::build(int nt, const std::vector<uint8_t>& present, hipStream_t stream) {
    release();
    nt_ = nt; stream_ = stream; refused_ = 0;
    SetupTrace ptr_trace;
    const Cols col_rows = symbolic_slots(present);
    const Groups g = level_groups(col_rows);
    std::string e = refuse_by_size_or_cost(g.n_true_levels);
    if (e.empty()) e = refuse_by_memory();
    if (!e.empty()) return e;
    ptr_trace.mark("plan: symbolic fill, slots");
    TP_TRY(tiles_.alloc_zero((size_t)n_slots_ * kNB * kNB));
    TP_TRY(linv_.alloc_zero((size_t)nt_ * kNB * kNB));
    ptr_trace.mark("plan: tiles allocated, cleared");
    Lists lists;
    e = host_lists(present, col_rows, g, tiles_, linv_, &lists);
    if (!e.empty()) return e;
    ptr_trace.mark("plan: task lists, dataflow units");
    e = upload(lists);
    if (e.empty()) ptr_trace.mark("plan: uploads, streams, events");
    return e;
}

// Host-only twin of build() (tests: no device is touched): the same host steps on a plan that owns no device resources,
// with stand-in tile and linv addresses that identify tiles, nothing more.
std::string TilePlan::build_host_only(int nt, const std::vector<uint8_t>& present) {
    nt_ = nt; refused_ = 0;
    const Cols col_rows = symbolic_slots(present);
    const Groups g = level_groups(col_rows);
    const std::string e = refuse_by_size_or_cost(g.n_true_levels);
    if (!e.empty()) return e;
    Lists lists;   // (uploaded nowhere)
    return host_lists(present, col_rows, g, reinterpret_cast<double*>(uintptr_t(1) << 44), reinterpret_cast<double*>(uintptr_t(1) << 45), &lists);
}

// The lists of a plan, in this order: the level task lists, the two sweeps, the PCG lists, the dataflow launches, the first writers.
std::string TilePlan::host_lists(const std::vector<uint8_t>& present, const Cols& col_rows, const Groups& g, double* tiles, double* linv, Lists* out) {
    n_levels_ = (int)g.cols.size(); n_local_groups_ = g.n_local;
    group_cols_ = g.cols;
    level_lists(col_rows, g, tiles, linv);
    sweep_lists(col_rows, g, tiles, linv, out);
    sym_lists(present, out);
    n_potrf_ = (int64_t)potrf_h_.size(); n_trsm_ = (int64_t)trsm_h_.size(); n_upd_ = (int64_t)upd_h_.size();
    // The second side stream (factor_schedule), for the whole plan or not at all: it pays where a level carries a bulk worth
    // overlapping (final-13682: ~1,000 tile products per level, 7.95 -> 7.5 ms; synthetic-10k 6.4 -> 6.1) and costs where the
    // levels are small and the factorisation is its launch chain (the ladybug / venice shapes, ~100 products per level: one
    // more stream is one more edge per level, 3.1 -> 3.5 ms).
    two_side_plan_ = two_side_ == 2 || (two_side_ == 1 && n_upd_ >= 256 * (int64_t)n_levels_);
    const std::string e = flow_regions(col_rows, g, tiles, linv);
    if (e.empty()) flag_first_writers(tiles);
    return e;
}

// ---- task lists scheduled by elimination-tree LEVEL ------------------------------------------------
// Columns of one level are independent: their potrf / panel solves / trailing updates run as ONE batched launch
// each.  Two columns of a level may update the same ancestor tile: those updates are split into
// conflict-free rounds (deterministic), one launch per round.
void TilePlan::level_lists(const Cols& col_rows, const Groups& g, double* tiles, double* linv) {
    auto tile_ptr = [&](int I, int J) { return tile_at(tiles, slot(I, J)); };
    potrf_h_.clear(); trsm_h_.clear(); upd_h_.clear(); upd_rounds_.clear();
    lv_.assign(n_levels_ + 1, Level());
    upd_h_.reserve(n_upd_);
    for (int lv = 0; lv < n_levels_; ++lv) {
        struct U { int64_t key; int K; GemmTask t; };
        std::vector<U> us;
        for (int K : g.cols[lv]) {
            const auto& rows = col_rows[K];
            potrf_h_.push_back({tile_ptr(K, K), tile_at(linv, K), K});
            for (int I : rows)
                if (g.group_of[I] == lv + 1) trsm_h_.push_back({tile_ptr(I, K), tile_ptr(I, K), tile_at(linv, K)});   // (first: see below)
            for (size_t a = 0; a < rows.size(); ++a)
                for (size_t b = 0; b <= a; ++b)
                    us.push_back({(int64_t)rows[a] * nt_ + rows[b], K, {tile_ptr(rows[a], rows[b]), tile_ptr(rows[a], K), tile_ptr(rows[b], K)}});
        }
        // the panel solves of the level: first the tiles whose ROW belongs to the next level (all that U1d(lv) reads), then the
        // others; by column inside each part
        for (int K : g.cols[lv])
            for (int I : col_rows[K])
                if (g.group_of[I] != lv + 1) trsm_h_.push_back({tile_ptr(I, K), tile_ptr(I, K), tile_at(linv, K)});
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
        int* const part_end[4] = {&lv_[lv].u1o, &lv_[lv].u2a, &lv_[lv].u2b1, &lv_[lv].u2b2};
        for (int part = 0; part < 5; ++part) {
            std::vector<const U*> mine;
            for (const U& u : us) {
                const int tcol = (int)(u.key % nt_), trow = (int)(u.key / nt_);
                const int d = g.group_of[tcol] - lv;
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
                const int64_t off = (int64_t)upd_h_.size();
                for (const U* u : sel) upd_h_.push_back(u->t);
                upd_rounds_.push_back({off, (int64_t)upd_h_.size() - off});
            }
            if (part < 4) *part_end[part] = (int)upd_rounds_.size();
        }
        lv_[lv + 1].potrf = (int)potrf_h_.size();
        lv_[lv + 1].panel = (int)trsm_h_.size();
        lv_[lv + 1].upd = (int)upd_rounds_.size();
    }
}

// The triangular sweeps, level by level (forward by group, backward from the root group down) and as dataflow launches.
void TilePlan::sweep_lists(const Cols& col_rows, const Groups& g, double* tiles, double* linv, Lists* sw) {
    auto tile_ptr = [&](int I, int J) { return tile_at(tiles, slot(I, J)); };
    for (int lv = 0; lv < n_levels_; ++lv) {
        for (int K : g.cols[lv]) {
            // The top columns of a distributed plan are swept by every rank, and the ranks' copies of the top solution
            // must be BITWISE equal (a rank's own blocks are back-substituted from its copy, the result takes rank 0's;
            // with cond(S) ~ 1e9 a last-bit difference shows up as a 1e-11 residual).  The forward step adds into shared
            // ancestor blocks with atomics, which is order-dependent when two columns of a level run in one launch:
            // top columns therefore get one launch each.
            if (cls_h_[K] == 2) lv_[lv].fwd_cut.push_back((int)sw->fwd.size());
            sw->fwd.push_back({tile_at(linv, K), nullptr, K, -1});
            for (int I : col_rows[K]) sw->fwd.push_back({tile_at(linv, K), tile_ptr(I, K), K, I});
        }
        lv_[lv + 1].fwd = (int)sw->fwd.size();
    }
    bwd_step_.assign(n_levels_ + 1, 0);
    for (int lv = n_levels_ - 1; lv >= 0; --lv) {
        for (int I : g.cols[lv]) {
            sw->bwd.push_back({tile_at(linv, I), nullptr, I, -1});
            for (int J : g.row_cols[I]) sw->bwd.push_back({tile_at(linv, I), tile_ptr(I, J), I, J});
        }
        bwd_step_[n_levels_ - lv] = (int)sw->bwd.size();
    }
    // both sweeps as one dataflow launch each (k_tri_fwd_flow / k_tri_bwd_flow; plans that are not distributed): level
    // by level the solve tasks of the level's blocks, then the product tasks of the tiles those solutions multiply.
    // A block's products own consecutive slots of the partial array, in the order the solve task folds them.
    const Cols& row_cols = g.row_cols;
    std::vector<FlowTask> &ft = sw->flow_fwd, &bt = sw->flow_bwd;
    n_flow_local_ = 0;
    // forward: slots by block row.  In a distributed plan a shared top row takes products from this rank's columns
    // (phase 0: folded into the exchange vector, no solve) and from top columns (phase 1): the rank's sources get the
    // first slots of the row, the top sources the rest, each in column order -- so the fold of the top sources is
    // the same sequence of additions on every rank (the ranks' copies of the top solution must be bitwise equal).
    std::vector<int> first(nt_ + 1, 0), own_src(nt_, 0);
    std::vector<std::vector<int>> slot_of(nt_);
    for (int K = 0; K < nt_; ++K) {
        first[K + 1] = first[K] + (int)row_cols[K].size();
        for (int J : row_cols[K]) own_src[K] += cls_h_[J] == 1;
        int a = 0, b = own_src[K];
        slot_of[K].reserve(row_cols[K].size());
        for (int J : row_cols[K]) slot_of[K].push_back(cls_h_[J] == 1 ? a++ : b++);
    }
    // Single-GPU plans (kTriInline, round 5): the solve task of a block forms the product of its LAST-ARRIVING source itself
    // (FlowTask::mat2 / src2 / slot2: the source solved latest, i.e. of the highest level forward, of the lowest backward) --
    // the link of the dependency chain loses a flag hop and a trip through memory; that product task leaves the list.
    // Only in the NARROW levels (at most kTriInline columns): where a level is wide the sweeps are bound by HBM and the
    // second tile of a solve task only serialises two products (final-13682 with every block inlined: sweeps 0.71 -> 0.79 ms;
    // ladybug-1723, narrow everywhere: 0.35 -> 0.28).
    const bool inl = kTriInline > 0 && !distributed();
    std::vector<int> fwd_inl(nt_, -1), bwd_inl(nt_, -1);
    if (inl)
        for (int K = 0; K < nt_; ++K) {
            if ((int)g.cols[(size_t)g.group_of[K]].size() > kTriInline) continue;
            for (int J : row_cols[K]) if (fwd_inl[K] < 0 || g.group_of[J] >= g.group_of[fwd_inl[K]]) fwd_inl[K] = J;
            for (int I : col_rows[K]) if (bwd_inl[K] < 0 || g.group_of[I] < g.group_of[bwd_inl[K]]) bwd_inl[K] = I;
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
    if (!distributed()) {
        for (int lv = 0; lv < n_levels_; ++lv) {
            for (int K : g.cols[lv]) ft.push_back(fwd_solve(K));
            for (int K : g.cols[lv]) products_of(K);
        }
    } else {
        for (int lv = 0; lv < n_local_groups_; ++lv) {          // phase 0: this rank's columns ...
            for (int K : g.cols[lv]) ft.push_back({tile_at(linv, K), -1, K, first[K], (int)row_cols[K].size()});
            for (int K : g.cols[lv]) products_of(K);
        }
        for (int lv = n_local_groups_; lv < n_levels_; ++lv)    // ... and what they add to the shared top blocks
            for (int K : g.cols[lv]) ft.push_back({tile_at(linv, K), -2, K, first[K], own_src[K]});
        n_flow_local_ = (int)ft.size();
        for (int lv = n_local_groups_; lv < n_levels_; ++lv) {  // phase 1: the top columns, every rank alike
            for (int K : g.cols[lv])
                ft.push_back({tile_at(linv, K), -1, K, first[K] + own_src[K], (int)row_cols[K].size() - own_src[K]});
            for (int K : g.cols[lv]) products_of(K);
        }
    }
    if (!ft.empty()) {
        for (int K = 0; K < nt_; ++K) first[K + 1] = first[K] + (int)col_rows[K].size();      // backward: by block column
        for (int lv = n_levels_ - 1; lv >= 0; --lv) {
            for (int I : g.cols[lv]) {
                FlowTask t{tile_at(linv, I), -1, I, first[I], (int)col_rows[I].size()};
                if (bwd_inl[I] >= 0) {
                    const auto& cr = col_rows[I];
                    t.mat2 = tile_ptr(bwd_inl[I], I); t.src2 = bwd_inl[I];
                    t.slot2 = (int)(std::lower_bound(cr.begin(), cr.end(), bwd_inl[I]) - cr.begin());
                }
                bt.push_back(t);
            }
            for (int I : g.cols[lv])
                for (int J : row_cols[I]) {
                    if (bwd_inl[J] == I) continue;   // (formed by the solve task of block J)
                    const auto& cr = col_rows[J];
                    const int pos = (int)(std::lower_bound(cr.begin(), cr.end(), I) - cr.begin());
                    bt.push_back({tile_ptr(I, J), I, J, first[J] + pos, 0});
                }
        }
    }
    int64_t a = 0, b = 0;
    for (int K = 0; K < nt_; ++K) { a += (int64_t)row_cols[K].size(); b += (int64_t)col_rows[K].size(); }
    n_flow_parts_ = (int)std::max(a, b);
    n_flow_bwd_ = (int)bt.size();
    n_flow_tasks_ = (int)ft.size();
}

// symmetric matvec of the PCG variant: only tiles that are non-zero before fill
void TilePlan::sym_lists(const std::vector<uint8_t>& present, Lists* out) const {
    std::vector<SymEntry>& sym = out->sym_entries;
    out->sym_row_ptr.assign(nt_ + 1, 0);
    for (int I = 0; I < nt_; ++I) {
        for (int J = 0; J < I; ++J)
            if (present[(size_t)I * nt_ + J]) sym.push_back({slot(I, J), J, 0});
        sym.push_back({diag_slot_h_[I], I, 2});
        for (int I2 = I + 1; I2 < nt_; ++I2)
            if (present[(size_t)I2 * nt_ + I]) sym.push_back({slot(I2, I), I2, 1});
        out->sym_row_ptr[I + 1] = (int)sym.size();
        for (int J = 0; J <= I; ++J)
            if (J == I || present[(size_t)I * nt_ + J]) out->sym_tiles.push_back({slot(I, J), I, J});
    }
}

namespace {
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
}  // namespace

// ---- the trailing level groups [gf, g1) of a phase as ONE dataflow launch (k_factor_flow, chol_kernels.hip) ----------------
// Units in left-looking order: per column of the region the updates into its tiles (per target in source order = the
// order of the level launches), its potrf, its panel solves; last the updates into tiles whose column is outside
// the launch (the local phase of a distributed plan adding to the shared top).  Checked topological (`running`), then put in
// list-schedule order (list_schedule).
std::string TilePlan::flow_units(int gf, int g1, const Cols& col_rows, const Groups& g, double* tiles, double* linv, std::vector<FactorUnit>* units, double* sim_us) const {
    auto tile_ptr = [&](int I, int J) { return tile_at(tiles, slot(I, J)); };
    std::vector<FactorUnit>& funits = *units;
    funits.clear();
    std::vector<int> cols;
    std::vector<char> in_reg(nt_, 0);
    for (int grp = gf; grp < g1; ++grp)
        for (int K : g.cols[grp]) { cols.push_back(K); in_reg[K] = 1; }
    std::vector<std::vector<int>> src_of((size_t)n_slots_);
    std::vector<std::pair<int, int>> outside;   // (J, I) of targets whose column is not in the launch
    for (int K : cols) {
        const auto& rows = col_rows[K];
        for (size_t a = 0; a < rows.size(); ++a)
            for (size_t b = 0; b <= a; ++b) {
                std::vector<int>& v = src_of[(size_t)slot(rows[a], rows[b])];
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
        const int st = slot(I, J);
        for (int n = 0; n < n_upd_of(st); ++n) {
            const int K = src_of[(size_t)st][n], sa = slot(I, K), sb = slot(J, K);
            const bool whole = g.group_of[J] > g.group_of[K] + 1;
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
        const int sd = slot(J, J), nd = n_upd_of(sd);
        emit_updates(J, J);
        for (int I : col_rows[J]) emit_updates(I, J);
        funits.push_back(FactorUnit{tile_ptr(J, J), tile_at(linv, J), nullptr, {nd > 0 ? sd : -1, -1, -1}, {W * nd, 0, 0}, sd, 0, J, 0});
        for (int I : col_rows[J]) {
            const int st = slot(I, J), n = n_upd_of(st);
            for (int sp = 0; sp < W; ++sp)
                funits.push_back(FactorUnit{tile_ptr(I, J), tile_ptr(I, J), tile_at(linv, J), {n > 0 ? st : -1, -1, sd}, {W * n, 0, W * (nd + 1)}, st, 1, sp, 0});
        }
    }
    for (const auto& t : outside) emit_updates(t.second, t.first);
    if (!topological(funits, (size_t)n_slots_)) return "internal error: a dataflow factorisation unit waits for a later one";
    return list_schedule(src_of, units, sim_us);
}

// Where the dataflow launch of each phase (local groups / top groups) starts.  "factor_flow" > 0: the trailing groups with at
// most that many columns (and "factor_flow_rows" off-diagonal tiles per column).  < 0 (default): by a model -- the level
// launches cost max(80 us of launch chain, 0.14 us per tile product) per group, the dataflow launch what its list schedule
// says (it runs a tile product on one CU at a time and reads every operand past the L2: ~0.22 us per product with all CUs
// busy, but a level costs it ~55 us of chain instead of 80); the start with the smallest sum wins, no launch if none beats
// the level launches.  The units of both phases go to flow_units_h_.
std::string TilePlan::flow_regions(const Cols& col_rows, const Groups& g, double* tiles, double* linv) {
    auto level_us = [&](int grp) {
        double prod = 0.0;
        for (int K : g.cols[grp]) { const double m = (double)col_rows[K].size(); prod += m + 0.5 * m * (m + 1.0); }
        // (round 5: by the timeline a middle level of final-13682 really takes 140-250 us, ~90 + 0.11 prod -- but the launch's
        // own simulated time is as optimistic there, and the starts this pair of models picks ARE the measured optima:
        // profiles/r05_flow_dyn_sweep.txt.  Both left as they are.)
        return std::max(80.0, 0.14 * prod);
    };
    flow_units_h_.clear();
    for (int ph = 0; ph < 2; ++ph) {
        const int g0 = ph == 0 ? 0 : n_local_groups_, g1 = ph == 0 ? n_local_groups_ : n_levels_;
        flow_g0_[ph] = flow_g1_[ph] = g1; flow_first_[ph] = (int)flow_units_h_.size(); flow_n_[ph] = 0; flow_sim_us_[ph] = 0.0;
        if (flow_cols_ == 0 || g1 - g0 < 2) continue;
        int best_gf = g1;
        if (flow_cols_ > 0) {
            while (best_gf > g0) {
                const std::vector<int>& cols = g.cols[best_gf - 1];
                bool ok = (int)cols.size() <= flow_cols_;
                for (int K : cols) ok = ok && (int)col_rows[K].size() <= flow_rows_;
                if (!ok) break;
                --best_gf;
            }
        } else {
            double level_tail = 0.0, best_total = 0.0;   // cost of the groups [gf, g1) by level launches; best (level head dropped: common)
            int64_t units = 0;
            // the candidate starts, from the top down, with what the level launches would cost from there
            std::vector<std::pair<int, double>> cands;
            for (int gf = g1 - 1; gf >= g0; --gf) {
                bool ok = (int)g.cols[gf].size() <= 64;
                for (int K : g.cols[gf]) {
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
                    errs[(size_t)i] = flow_units(cands[c0 + (size_t)i].first, g1, col_rows, g, tiles, linv, &scratch, &sims[(size_t)i]);
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
        const std::string e = flow_units(best_gf, g1, col_rows, g, tiles, linv, &best_units, &sim);
        if (!e.empty()) return e;
        flow_g0_[ph] = best_gf;
        flow_n_[ph] = (int)best_units.size();
        flow_sim_us_[ph] = sim;
        flow_units_h_.insert(flow_units_h_.end(), best_units.begin(), best_units.end());
    }
    return "";
}

// ---- first writers of the fill tiles (tile_plan.h, first_ok_) ------------------------------------------------------------
// Two execution orders exist: the level launches alone (the lists of every level, in list order) and the level launches of
// the levels below a dataflow launch followed by its units (in unit order: the writers of a tile are chained in that order).
// A fill tile's first writer is flagged in both; touched tiles hold S and are never "first written".
void TilePlan::flag_first_writers(const double* tiles) {
    first_ok_ = false;
    if (distributed() || n_slots_ <= n_touched_ || flow_n_[1] != 0) return;
    auto slot_of_ptr = [&](const double* c) { return (int64_t)((c - tiles) / (ptrdiff_t)(kNB * kNB)); };
    std::vector<char> seen_a((size_t)n_slots_, 0);
    for (int64_t sl = 0; sl < n_touched_; ++sl) seen_a[(size_t)sl] = 1;
    std::vector<char> seen_b(seen_a);
    int64_t upd_before_flow = (int64_t)upd_h_.size();   // the level lists that run in front of the dataflow launch
    if (flow_n_[0] > 0) {
        const int r = lv_[(size_t)flow_g0_[0]].upd;
        if (r < (int)upd_rounds_.size()) upd_before_flow = upd_rounds_[(size_t)r].first;
    }
    for (size_t q = 0; q < upd_h_.size(); ++q) {
        const int64_t sl = slot_of_ptr(upd_h_[q].C);
        if ((int64_t)q < upd_before_flow) seen_b[(size_t)sl] = 1;
        if (!seen_a[(size_t)sl]) { seen_a[(size_t)sl] = 1; upd_h_[q].C = reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(upd_h_[q].C) | 1); }
    }
    // the dataflow units: the first (tile, writer) of a tile not written below the launch; its nine block units share C, A, B
    std::vector<const double*> first_a((size_t)n_slots_, nullptr), first_b((size_t)n_slots_, nullptr);
    for (FactorUnit& u : flow_units_h_) {
        if (u.kind != 2 && u.kind != 3) continue;
        const int64_t sl = slot_of_ptr(u.C);
        if (!seen_b[(size_t)sl]) { seen_b[(size_t)sl] = 1; first_a[(size_t)sl] = u.A; first_b[(size_t)sl] = u.B; }
        if (first_a[(size_t)sl] == u.A && first_b[(size_t)sl] == u.B && first_a[(size_t)sl] != nullptr) u.kind |= kFlowFirstWriter;
    }
    bool all = true;
    for (int64_t sl = n_touched_; sl < n_slots_; ++sl) all = all && seen_a[(size_t)sl] && (flow_n_[0] == 0 || seen_b[(size_t)sl]);
    if (all) first_ok_ = true;
    else {   // (a fill tile without an update: cannot be -- take the flags back and clear everything as before)
        for (GemmTask& t : upd_h_) t.C = reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(t.C) & ~uintptr_t(7));
        for (FactorUnit& u : flow_units_h_) u.kind &= 15;
    }
}

// The device step of build(): the lists and maps to the device, the work arrays, the streams and events.
std::string TilePlan::upload(const Lists& lists) {
    TP_TRY(slot_.upload(slot_h_));
    TP_TRY(diag_slot_.upload(diag_slot_h_));
    TP_TRY(flag_.alloc_zero(4));
    TP_TRY(flow_units_.upload(flow_units_h_));
    TP_TRY(flow_ver_.alloc_zero((size_t)n_slots_));
    n_sym_tiles_ = (int)lists.sym_tiles.size();
    TP_TRY(sym_tiles_.upload(lists.sym_tiles));
    TP_TRY(sym_part_.alloc_zero((size_t)n_slots_ * 2 * kNB));
    TP_TRY(row_dot_.alloc_zero((size_t)nt_));
    TP_TRY(blk_part_.alloc_zero(2 * (size_t)((n_pad() + 255) / 256)));
    TP_TRY(scal_.alloc_zero(8));
    TP_TRY(tri_fwd_.upload(lists.fwd));
    TP_TRY(tri_bwd_.upload(lists.bwd));
    TP_TRY(flow_fwd_.upload(lists.flow_fwd));
    TP_TRY(flow_bwd_.upload(lists.flow_bwd));
    TP_TRY(flow_part_.alloc_zero((size_t)std::max(n_flow_parts_, 1) * kNB));
    TP_TRY(flow_flags_.alloc_zero((size_t)2 * nt_ + 1));   // cnt[nt] | done[nt] | error word of the dataflow sweeps
    if (!flow_err_host_) {
        TP_TRY(flow_err_host_.alloc(4));
        flow_err_host_[0] = flow_err_host_[1] = flow_err_host_[2] = flow_err_host_[3] = 0;
        void* dp = nullptr;   // (pinned host memory is mapped: the kernels that post a word write it through this address)
        flow_err_host_dev_ = hipHostGetDevicePointer(&dp, flow_err_host_, 0) == hipSuccess ? static_cast<int*>(dp) : nullptr;
        (void)hipGetLastError();
    }
    TP_TRY(potrf_tasks_.upload(potrf_h_));
    TP_TRY(trsm_tasks_.upload(trsm_h_));
    TP_TRY(upd_tasks_.upload(upd_h_));
    TP_TRY(sym_row_ptr_.upload(lists.sym_row_ptr));
    TP_TRY(cls_.upload(cls_h_));
    TP_TRY(exch_.alloc_zero((size_t)n_pad()));
    TP_TRY(sym_entries_.upload(lists.sym_entries));
    // (a lowest-priority side stream was tried: no gain without graphs, +2.7 ms with them)
    // (and so was a CU-masked one that leaves 1 CU in 8 / 4 / 2 to the critical path: the same, either way)
    for (hipStream_t* s : {&side_, &so_, &side2_})
        if (!*s) TP_TRY(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    ev_.assign(n_levels_, {});
    for (auto& evs : ev_)
        for (hipEvent_t& ev : evs) TP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    TP_TRY(gate_cnt_.alloc((size_t)(n_levels_ + 1)));
    TP_TRY(hipDeviceSynchronize());  // the null-stream memsets above precede any work on the stream
    return "";
}
#undef TP_TRY

hipError_t TilePlan::zero_tiles(bool own_touched_only, bool skip_fill) {
    tiles_written();
    const size_t te = (size_t)kNB * kNB * sizeof(double);
    hipError_t e = hipSuccess;
    auto clear = [&](int64_t first, int64_t count) {
        if (e == hipSuccess && count > 0) e = hipMemsetAsync(tiles_ + (size_t)first * kNB * kNB, 0, (size_t)count * te, stream_);
    };
    if (distributed() && !own_all_ && part_rank_ < (int)own_range_.size()) {
        // a rank of a distributed plan factorises its own columns and the shared top: the fill tiles of the other ranks'
        // columns are never touched; their touched tiles only when this rank's landmarks may add to them (range sharding)
        if (own_touched_only) { clear(own_range_[part_rank_].first, own_range_[part_rank_].second); clear(n_t_nt_, n_touched_ - n_t_nt_); }
        else clear(0, n_touched_);
        clear(own_fill_[part_rank_].first, own_fill_[part_rank_].second);
        clear(n_f_nt_, n_slots_ - n_f_nt_);
    } else {
        clear(0, (skip_fill && first_ok_) ? n_touched_ : n_slots_);
    }
    if (e != hipSuccess) return e;
    launch_clear_i32(flag_, 4, stream_);
    return hipGetLastError();
}

void TilePlan::add_diag(int n_valid, double add_valid, double pad_value) {
    tiles_written();
    launch_tile_add_diag(tiles_, diag_slot_, n_valid, (int)n_pad(), add_valid, pad_value, stream_);
}

void TilePlan::scale_sym(const double* scale) { tiles_written(); launch_tile_scale_sym(sym_tiles_, n_sym_tiles_, tiles_, scale, stream_); }

void TilePlan::diag(double* out) const { launch_tile_diag(tiles_, diag_slot_, nt_, out, stream_); }

// forward step of level group lv: one launch, or one per column where the plan asks for it (Level::fwd_cut)
void TilePlan::launch_fwd_group(int lv, double* bvec, double* yvec, hipStream_t s) {
    const std::vector<int>& cut = lv_[lv].fwd_cut;
    if (cut.size() < 2) {
        launch_tri_step(false, tri_fwd_ + lv_[lv].fwd, lv_[lv + 1].fwd - lv_[lv].fwd, bvec, yvec, s);
        return;
    }
    for (size_t i = 0; i < cut.size(); ++i) {
        const int b = cut[i], e = i + 1 < cut.size() ? cut[i + 1] : lv_[lv + 1].fwd;
        launch_tri_step(false, tri_fwd_ + b, e - b, bvec, yvec, s);
    }
}

// The factorisation and the triangular solves are static launch sequences for a given structure:
// they are captured once into hipGraphs (a few hundred dependent launches would otherwise be paced by
// host launch overhead) and replayed every iteration.
ScheduleInput TilePlan::input() const {
    return ScheduleInput{lv_, upd_rounds_, n_levels_, n_local_groups_, overlap_, overlap_min_, split_u1_, split_u1_min_, two_side_plan_,
                         gate_min_, debug_skip_idle_wait_, flow_on_,
                         {{flow_g0_[0], flow_g1_[0], flow_first_[0], flow_n_[0]}, {flow_g0_[1], flow_g1_[1], flow_first_[1], flow_n_[1]}}};
}

// The factorisation's launch sequence (factor_schedule), call by call: the list check_schedule proves is the list issued.
void TilePlan::issue(const std::vector<SchedOp>& ops) {
    for (const SchedOp& o : ops) {
        const hipStream_t s = stream_of(o.stream);
        switch (o.op) {
            case kOpLaunch:
                if (o.list == 0) launch_potrf_inv(potrf_tasks_ + o.first, o.count, flag_, s, o.arrive >= 0 ? gate_cnt_ + o.arrive : nullptr);
                else if (o.list == 1) launch_tile_gemm_nt(trsm_tasks_ + o.first, o.count, 1.0, 0.0, s, /*tri_b=*/true);
                else if (o.list == 2) launch_tile_gemm_nt(upd_tasks_ + o.first, o.count, -1.0, 1.0, s);
                else launch_factor_flow(flow_units_ + o.first, o.count, flow_ver_, flag_, flag_ + 1, s, flow_trace_ ? flow_trace_ + 3 * (size_t)o.first : nullptr);
                break;
            case kOpRecord: (void)hipEventRecord(ev_[o.event / kLevelEvents][o.event % kLevelEvents], s); break;
            case kOpWait: (void)hipStreamWaitEvent(s, ev_[o.event / kLevelEvents][o.event % kLevelEvents], 0); break;
            case kOpGate: launch_gate(gate_cnt_ + o.first, o.count, 150, s); break;
            case kOpClearGates: launch_clear_i32(gate_cnt_, o.count, s); break;
            case kOpClearVersions:
                launch_clear_i32(flow_ver_, n_slots_, s);
                if (poison_factor_)   // (tests: the version of the first unit's tile starts hugely negative and is never reached)
                    (void)hipMemsetAsync(flow_ver_ + flow_units_h_[(size_t)o.first].pub, 0x80, sizeof(int), s);
                break;
        }
    }
}

void TilePlan::enqueue_solve(const double* rhs, double* x, double* work) {
    // L y = rhs (work vector bvec), then L^T x = y (work vector yvec); level by level
    double* bvec = work;
    double* yvec = work + n_pad();
    const bool flow = tri_flow_ && n_flow_tasks_ > 0;
    if (flow) {
        launch_tri_flow(false, flow_fwd_, n_flow_tasks_, rhs, yvec, flow_part_, flow_flags_, nt_, stream_, nullptr, nullptr,
                        poison_ == 1 ? nt_ - 1 : -1);
    } else {
        (void)hipMemcpyAsync(bvec, rhs, n_pad() * sizeof(double), hipMemcpyDeviceToDevice, stream_);
        for (int lv = 0; lv < n_levels_; ++lv)
            launch_fwd_group(lv, bvec, yvec, stream_);
    }
    if (flow) {
        launch_tri_flow(true, flow_bwd_, n_flow_bwd_, yvec, x, flow_part_, flow_flags_, nt_, stream_, nullptr, nullptr,
                        poison_ == 2 ? nt_ - 1 : -1);
        return;
    }
    for (int s = 0; s < n_levels_; ++s)
        launch_tri_step(true, tri_bwd_ + bwd_step_[s], bwd_step_[s + 1] - bwd_step_[s], yvec, x, stream_);
}

// The distributed triangular solves (see tile_plan.h).  bvec/yvec as in enqueue_solve; masks: bit (1 << class).
void TilePlan::enqueue_dist_solve(int phase, const double* rhs, double* x, double* work) {
    double* bvec = work;
    double* yvec = work + n_pad();
    const int n = (int)n_pad();
    const int L1 = n_local_groups_;
    const bool flow = tri_flow_ && n_flow_local_ > 0;
    if (phase == 0 && flow) {
        // dataflow form: this rank's columns in one launch; its contributions to the shared top blocks are folded
        // straight into the exchange vector (the top blocks of the right-hand side enter the sum once, on rank 0)
        (void)hipMemsetAsync(exch_, 0, n_pad() * sizeof(double), stream_);
        launch_tri_flow(false, flow_fwd_, n_flow_local_, rhs, yvec, flow_part_, flow_flags_, nt_, stream_,
                        part_rank_ == 0 ? rhs : nullptr, exch_);
    } else if (phase == 1 && flow) {
        // the top columns forward (right-hand side = the summed exchange vector), then everything backward, top first.
        // Pull form, fixed fold order: the ranks' copies of the top solution are bitwise equal by construction.
        launch_tri_flow(false, flow_fwd_ + n_flow_local_, n_flow_tasks_ - n_flow_local_, exch_, yvec, flow_part_, flow_flags_, nt_,
                        stream_, nullptr, nullptr);
        launch_tri_flow(true, flow_bwd_, n_flow_bwd_, yvec, x, flow_part_, flow_flags_, nt_, stream_, nullptr, nullptr);
        launch_vec_select(n, x, cls_, part_rank_ == 0 ? 6 : 2, exch_, stream_);
    } else if (phase == 0) {
        // the top blocks of the right-hand side enter the sum once (rank 0); every rank adds its columns' updates
        launch_vec_select(n, rhs, cls_, part_rank_ == 0 ? 7 : 3, bvec, stream_);
        for (int lv = 0; lv < L1; ++lv)
            launch_fwd_group(lv, bvec, yvec, stream_);
        launch_vec_select(n, bvec, cls_, 4, exch_, stream_);
    } else if (phase == 1) {
        launch_vec_merge(n, exch_, cls_, 4, bvec, stream_);
        for (int lv = L1; lv < n_levels_; ++lv)
            launch_fwd_group(lv, bvec, yvec, stream_);
        for (int s = 0; s < n_levels_; ++s)  // top groups first, then this rank's
            launch_tri_step(true, tri_bwd_ + bwd_step_[s], bwd_step_[s + 1] - bwd_step_[s], yvec, x, stream_);
        launch_vec_select(n, x, cls_, part_rank_ == 0 ? 6 : 2, exch_, stream_);
    } else {
        (void)hipMemcpyAsync(x, exch_, n_pad() * sizeof(double), hipMemcpyDeviceToDevice, stream_);
    }
}

// kGraphFactor: factorisation of the local level groups (all of them in a plan that is not distributed), kGraphSweeps: both
// sweeps, kGraphFactorTop: factorisation of the top level groups, kGraphDistSolve0 / 1: phases 0 / 1 of the distributed solve
bool TilePlan::run_graph(int which, const double* rhs, double* x, double* work) {
    if (!use_graphs_) return false;
    if (graph_exec_[which] && (rhs != graph_rhs_[which] || x != graph_x_[which] || work != graph_work_[which])) {
        (void)hipGraphExecDestroy(graph_exec_[which]);  // the captured pointers changed
        graph_exec_[which] = nullptr;
    }
    if (!graph_exec_[which]) {
        if (graph_failed_[which]) return false;
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal) != hipSuccess) { graph_failed_[which] = true; return false; }
        if (which == kGraphFactor) enqueue_factor(0, n_local_groups_);
        else if (which == kGraphFactorTop) enqueue_factor(n_local_groups_, n_levels_);
        else if (which == kGraphDistSolve0 || which == kGraphDistSolve1) enqueue_dist_solve(which - kGraphDistSolve0, rhs, x, work);
        else enqueue_solve(rhs, x, work);
        if (hipStreamEndCapture(stream_, &g) != hipSuccess || !g) { graph_failed_[which] = true; (void)hipGetLastError(); return false; }
        hipGraphExec_t ex = nullptr;
        if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) { (void)hipGraphDestroy(g); graph_failed_[which] = true; (void)hipGetLastError(); return false; }
        (void)hipGraphDestroy(g);
        graph_exec_[which] = ex;
        graph_rhs_[which] = rhs; graph_x_[which] = x; graph_work_[which] = work;
    }
    return hipGraphLaunch(graph_exec_[which], stream_) == hipSuccess;
}

void TilePlan::enable_tri_flow(bool on) {
    if (on == tri_flow_) return;
    tri_flow_ = on;
    for (int which : {kGraphSweeps, kGraphDistSolve0, kGraphDistSolve1})   // the captured sweeps change
        if (graph_exec_[which]) { (void)hipGraphExecDestroy(graph_exec_[which]); graph_exec_[which] = nullptr; }
}

hipError_t TilePlan::enable_flow_trace() {
    if (flow_trace_) return hipSuccess;
    const size_t n = 3 * (size_t)std::max(flow_n_[0] + flow_n_[1], 1);
    hipError_t e = flow_trace_.alloc(n);
    if (e != hipSuccess) return e;
    for (int which : {kGraphFactor, kGraphFactorTop})   // the captured launches hold the old (null) pointer
        if (graph_exec_[which]) { (void)hipGraphExecDestroy(graph_exec_[which]); graph_exec_[which] = nullptr; }
    return hipMemset(flow_trace_, 0, n * sizeof(unsigned long long));
}

hipError_t TilePlan::read_flow_trace(std::vector<FactorUnit>* units, std::vector<unsigned long long>* stamps) {
    const size_t n = (size_t)(flow_n_[0] + flow_n_[1]);
    units->resize(n); stamps->resize(3 * n);
    if (n == 0 || !flow_trace_) return hipErrorNotInitialized;
    hipError_t e = hipMemcpy(units->data(), flow_units_, n * sizeof(FactorUnit), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    return hipMemcpy(stamps->data(), flow_trace_, 3 * n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
}

std::vector<SchedOp> TilePlan::schedule_trace(int phase) const {
    return phase == 0 ? factor_schedule(input(), 0, n_local_groups_) : factor_schedule(input(), n_local_groups_, n_levels_);
}

void TilePlan::top_slot_ranges(std::pair<int64_t, int64_t> out[2]) const {
    out[0] = {n_t_nt_, n_touched_ - n_t_nt_};
    out[1] = {n_f_nt_, n_slots_ - n_f_nt_};
}

void TilePlan::factor_phase(int phase) {
    tiles_written();
    if (phase == 0) { if (!run_graph(kGraphFactor, nullptr, nullptr, nullptr)) enqueue_factor(0, n_local_groups_); }
    else if (!run_graph(kGraphFactorTop, nullptr, nullptr, nullptr)) enqueue_factor(n_local_groups_, n_levels_);
}

void TilePlan::solve_phase(int phase, const double* rhs, double* x, double* work) {
    if (phase == 2 || !run_graph(kGraphDistSolve0 + phase, rhs, x, work)) enqueue_dist_solve(phase, rhs, x, work);
}

hipError_t TilePlan::factor(int* failed_at, bool defer_flags) {
    tiles_written();
    if (distributed()) {
        if (!comm_.sum || !comm_.max_int) return hipErrorNotInitialized;  // a distributed plan needs its communicator
        factor_phase(0);
        std::pair<int64_t, int64_t> rg[2];
        top_slot_ranges(rg);
        const size_t te = (size_t)kNB * kNB;
        for (int i = 0; i < 2; ++i)
            if (rg[i].second > 0 && !comm_.sum(tiles_ + (size_t)rg[i].first * te, (size_t)rg[i].second * te, stream_)) return hipErrorUnknown;
        factor_phase(1);
        if (!comm_.max_int(flag_, 2, stream_)) return hipErrorUnknown;  // a failed pivot (or a dataflow time-out) anywhere fails the factorisation everywhere
        return read_flags(failed_at);
    }
    if (poison_factor_) {   // (tests: the poisoned launch is not part of the captured graphs)
        enqueue_factor(0, n_levels_);
        poison_factor_ = false;
    } else if (!run_graph(kGraphFactor, nullptr, nullptr, nullptr)) enqueue_factor(0, n_levels_);
    if (defer_flags) { *failed_at = 0; return hipGetLastError(); }
    return read_flags(failed_at);
}

// The pivot flag of this factorisation.  (The error word of the dataflow sweeps belongs to the SOLVE that ran them:
// post_sweep_status / sweep_timed_out.)
hipError_t TilePlan::read_flags(int* failed_at) {
    int f[2] = {0, 0};   // [0] first failed tile column + 1, [1] error word of the dataflow factorisation (k_factor_flow)
    hipError_t e = hipMemcpyAsync(f, flag_, sizeof f, hipMemcpyDeviceToHost, stream_);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream_);
    *failed_at = f[0];
    if (e == hipSuccess && f[1] != 0) {
        // a unit gave up waiting (flow_wait's spin limit): the tiles are half updated.  Back to the level launches for the
        // rest of the plan's life; the caller re-assembles and factorises again (factor_flow_gave_up()).
        flow_gave_up_ = true;
        flow_on_ = false;
        for (int which : {kGraphFactor, kGraphFactorTop})
            if (graph_exec_[which]) { (void)hipGraphExecDestroy(graph_exec_[which]); graph_exec_[which] = nullptr; }
        (void)hipMemsetAsync(flag_ + 1, 0, sizeof(int), stream_);
    }
    return e;
}

// Behind the sweeps of a solve: the error word goes to pinned host memory (no synchronisation here: the caller's next
// one covers it) and is cleared for the next solve.  Distributed plans take the max over the ranks first -- a rank whose
// sweep gave up must not be the only one that repeats the solve, the others would be waiting in its collectives.
bool TilePlan::post_sweep_status(bool reduce) {
    if (!flow_flags_ || !flow_err_host_) return true;
    int* err = flow_flags_ + 2 * (size_t)nt_;
    if (reduce && comm_.max_int && !comm_.max_int(err, 1, stream_)) return false;   // (the communicator keeps its message)
    if (!reduce && flow_err_host_dev_) { launch_post_word(err, flow_err_host_dev_, stream_); return true; }   // (one launch, no copy engine)
    (void)hipMemcpyAsync(flow_err_host_, err, sizeof(int), hipMemcpyDeviceToHost, stream_);
    (void)hipMemsetAsync(err, 0, sizeof(int), stream_);
    return true;
}

bool TilePlan::sweep_timed_out() {
    if (!flow_err_host_ || flow_err_host_[0] == 0) return false;
    flow_err_host_[0] = 0;
    ++n_sweep_timeouts_;
    return true;
}

hipError_t TilePlan::debug_occupy_cus(int n_cus, int micros) {
    if (!flow_err_host_) return hipErrorNotInitialized;
    if (!occ_stream_) { const hipError_t e = hipStreamCreateWithFlags(&occ_stream_, hipStreamNonBlocking); if (e != hipSuccess) return e; }
    volatile int* started = flow_err_host_ + 1;
    started[0] = 0; started[1] = 0;
    launch_occupy_cus(n_cus, micros, flow_err_host_ + 1, occ_stream_);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (int spin = 0; spin < 2000 && started[0] < n_cus; ++spin) std::this_thread::sleep_for(std::chrono::microseconds(100));
    return started[0] >= n_cus ? hipSuccess : hipErrorNotReady;
}

hipError_t TilePlan::solve(const double* rhs, double* x, double* work) {
    if (distributed()) {
        if (!comm_.sum) return hipErrorNotInitialized;
        solve_phase(0, rhs, x, work);
        if (!comm_.sum(exch_, (size_t)n_pad(), stream_)) return hipErrorUnknown;
        solve_phase(1, rhs, x, work);
        if (!comm_.sum(exch_, (size_t)n_pad(), stream_)) return hipErrorUnknown;
        solve_phase(2, rhs, x, work);
        // (the collective is entered by every rank or by none: tri_flow_ is a plan-wide setting, and a distributed plan has
        // dataflow tasks on every rank -- at least the fold tasks of the shared top columns)
        if (tri_flow_ && !post_sweep_status(true)) return hipErrorUnknown;
        return hipGetLastError();
    }
    if (poison_ != 0) {   // (tests: the poisoned launch is not part of the captured graphs)
        enqueue_solve(rhs, x, work);
        poison_ = 0;
    } else if (!run_graph(kGraphSweeps, rhs, x, work)) enqueue_solve(rhs, x, work);
    if (tri_flow_ && n_flow_tasks_ > 0) (void)post_sweep_status(false);
    return hipGetLastError();
}

void TilePlan::sym_matvec(const double* x, double* y) {
    launch_sym_tile_products(sym_tiles_, n_sym_tiles_, tiles_, x, sym_part_, stream_);
    launch_sym_tile_gather(nt_, sym_row_ptr_, sym_entries_, sym_part_, x, y, row_dot_, stream_);
}

// solve_with_pcg (explicit_schur.rs:639-756).  Per iteration: one pass over the non-zero tiles
// (k_sym_tile_products + k_sym_tile_gather, which also yields p.Ap), two fused vector kernels that keep
// alpha/beta on the device, and ONE host read-back of {p.Ap, r.r, r.z} for the reference's three
// termination tests -- read ONE ITERATION BEHIND (round 5): iteration k + 1 is enqueued before the host waits for the
// scalars of iteration k, so the device never idles through a host round trip (25 us of a 185-us iteration).  The tests are
// also made on the device (k_pcg_close_iteration): the speculative iteration behind a met test changes nothing, and x, the
// iteration count and every scalar are those of the loop that waited every time.
hipError_t TilePlan::pcg(const double* rhs, double* x, double* work, int max_iter, double tol, int* iters) {
    tiles_written();
    const int n = (int)n_pad();
    double *dg = work, *pre = work + n, *r = work + 2 * (size_t)n, *z = work + 3 * (size_t)n, *p = work + 4 * (size_t)n,
           *ap = work + 5 * (size_t)n;
    double* sc = scal_;  // [0] rz_old  [1] p.Ap  [2] r.r  [3] r.z  [4] frozen
    hipError_t e;
    if (!pcg_host_) {
        if ((e = pcg_host_.alloc(16)) != hipSuccess) return e;
        for (hipEvent_t& ev : pcg_ev_) if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
    }
    launch_tile_diag(tiles_, diag_slot_, nt_, dg, stream_);
    launch_pcg_init(n, dg, rhs, pre, x, r, z, p, stream_);
    if ((e = hipMemsetAsync(sc, 0, 8 * sizeof(double), stream_)) != hipSuccess) return e;
    launch_dot(n, r, z, sc, stream_);
    launch_dot(n, r, r, sc + 2, stream_);
    double* h = pcg_host_;
    if ((e = hipMemcpyAsync(h, sc, 4 * sizeof(double), hipMemcpyDeviceToHost, stream_)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream_)) != hipSuccess) return e;
    const double abs_tol = tol * std::max(sqrt(h[2]), 1.0);
    auto enqueue_iteration = [&](int slot) -> hipError_t {
        launch_sym_tile_products(sym_tiles_, n_sym_tiles_, tiles_, p, sym_part_, stream_);
        launch_sym_tile_gather(nt_, sym_row_ptr_, sym_entries_, sym_part_, p, ap, row_dot_, stream_);
        launch_pcg_step1(n, nt_, sc, row_dot_, p, ap, pre, x, r, blk_part_, sc + 1, stream_);
        launch_pcg_step2(n, sc, blk_part_, pre, r, p, sc + 2, abs_tol, stream_);
        const hipError_t ce = hipMemcpyAsync(pcg_host_ + 8 * slot, sc, 5 * sizeof(double), hipMemcpyDeviceToHost, stream_);
        return ce != hipSuccess ? ce : hipEventRecord(pcg_ev_[slot], stream_);
    };
    int it = 0;
    if (max_iter > 0 && (e = enqueue_iteration(0)) != hipSuccess) return e;
    for (; it < max_iter; ++it) {
        if (it + 1 < max_iter && (e = enqueue_iteration((it + 1) & 1)) != hipSuccess) return e;   // on speculation
        if ((e = hipEventSynchronize(pcg_ev_[it & 1])) != hipSuccess) return e;
        h = pcg_host_ + 8 * (it & 1);
        // the device's verdict (h[4], k_pcg_close_iteration) decides -- the speculative iteration obeys the same word
        if (fabs(h[1]) < 1e-30) break;                       // p.Ap (:703-705); x was left untouched
        if (h[4] != 0.0) { ++it; break; }                    // |r| < tol (:726-728) or rz_old ~ 0 (:741-743)
    }
    *iters = it;
    return hipStreamSynchronize(stream_);   // (the speculative iteration, if any, has drained: x is final)
}

SelectedInverse& TilePlan::inverse() {
    SinvPlanView v;
    v.tiles = tiles_; v.linv = linv_; v.slot = slot_; v.diag_slot = diag_slot_;
    v.nt = nt_; v.n_slots = n_slots_; v.stream = stream_;
    v.slot_host = slot_h_.data(); v.group_cols = &group_cols_;
    v.distributed = distributed() || part_world_ > 1;
    v.factor_valid = factor_valid_; v.factor_epoch = factor_epoch_;
    inverse_.bind(v);
    return inverse_;
}

}  // namespace apex
