// capi_debug.cpp -- extern "C" surface declared in include/apexgpu.h: the host-arithmetic apexgpu_debug_* entries (partition,
// schedule, plan tables, selected-inversion lists, pair lists, host structure), apexgpu_shard_range, apexgpu_debug_invert_blocks
// and the lockstep solve.  None of them takes one handle; those that allocate run under guarded() (capi_guard.h).
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ba_structure.h"
#include "capi_handles.h"
#include "sinv_lists.h"

// Test entry: the `n` handles are the ranks 0..n-1 of one sharded problem (apexgpu_set_shard(r, n) before
// set_structure, same parameters), all on this process's GPU.  Runs ONE distributed Cholesky solve in lockstep --
// every rank executes phase p, then this function plays the communicator for the exchange that follows it (sums in
// rank order, max for the failure flag) -- and leaves the step on every handle (apexgpu_export_step).
static int lockstep_solve_impl(apexgpu_solver** hs, int n, double lambda) {
    if (!hs || n < 2) return APEXGPU_ERR_INVALID_INPUT;
    auto solver = [&](int r) { return apex::HandleOwner::solver(hs[r]); };   // (the communicator owns all ranks at once)
    for (int r = 0; r < n; ++r) if (!hs[r] || !solver(r)) return APEXGPU_ERR_INVALID_INPUT;
    for (int phase = 0; phase <= 5; ++phase) {
        for (int r = 0; r < n; ++r) {
            const int rc = solver(r)->dist_phase(phase, lambda);
            if (rc != 0) return rc;
            // one rank at a time: the ranks share this GPU, and their stage timers then show what each would take alone
            if (hipDeviceSynchronize() != hipSuccess) return APEXGPU_ERR_DEVICE;
        }
        if (phase == 5) break;
        std::vector<apex::ExchangeList> lists(n);   // the lists production issues behind this phase (Solver::exchange)
        for (int r = 0; r < n; ++r) lists[r] = solver(r)->exchange(phase, true);
        for (size_t b = 0; b < lists[0].size(); ++b) {
            const size_t len = lists[0][b].n;
            const int root = lists[0][b].root, op = lists[0][b].op;
            for (int r = 1; r < n; ++r)
                if (lists[r].size() != lists[0].size() || lists[r][b].op != op || lists[r][b].n != len || lists[r][b].root != root) return APEXGPU_ERR_INVALID_STATE;
            if (len == 0) continue;
            if (op == apex::ExchangeItem::kMaxInt) {   // the failure flags: max over the ranks, on the host
                std::vector<int> mx(len, 0), f(len);
                for (int r = 0; r < n; ++r) {
                    if (hipMemcpy(f.data(), lists[r][b].dev, len * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return APEXGPU_ERR_DEVICE;
                    for (size_t i = 0; i < len; ++i) mx[i] = std::max(mx[i], f[i]);
                }
                for (int r = 0; r < n; ++r) if (hipMemcpy(lists[r][b].dev, mx.data(), len * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return APEXGPU_ERR_DEVICE;
                continue;
            }
            auto buf = [&](int r) { return static_cast<double*>(lists[r][b].dev); };
            const int dst = root >= 0 ? root : 0;   // ncclReduce(root) / ncclAllReduce: ranks summed in rank order
            for (int r = 0; r < n; ++r)
                if (r != dst) apex::launch_vec_add((int64_t)len, buf(dst), buf(r), buf(dst), nullptr);
            if (root < 0)
                for (int r = 1; r < n; ++r)
                    if (hipMemcpyAsync(buf(r), buf(0), len * sizeof(double), hipMemcpyDeviceToDevice, nullptr) != hipSuccess) return APEXGPU_ERR_DEVICE;
        }
        if (hipDeviceSynchronize() != hipSuccess) return APEXGPU_ERR_DEVICE;
    }
    return APEXGPU_OK;
}

// The host-only plan of the apexgpu_debug_* calls that take opts[8]: structure and lists on the stand-in bases, the schedule
// switches; err = why it was refused.
struct HostPlan {
    apex::PlanStructure s; apex::PlanLists l; apex::ScheduleSwitches w; std::string err;
    std::vector<apex::SchedOp> schedule(int phase) const {
        const int cut = s.n_local_groups;
        return phase == 0 ? apex::factor_schedule(apex::schedule_input(s, l, w), 0, cut) : apex::factor_schedule(apex::schedule_input(s, l, w), cut, s.n_levels());
    }
};
static HostPlan host_plan(int nt, const uint8_t* present, int world, int rank, const int opts[8]) {
    HostPlan h;
    apex::PlanOptions o;
    if (world > 1) { o.rank = rank; o.world = world; }
    o.two_side = opts[0];
    h.w.overlap = opts[1] != 0; if (opts[1] > 1) h.w.overlap_min = opts[1];
    h.w.split_u1 = opts[2] > 0; if (opts[2] > 0) h.w.split_u1_min = opts[2];
    h.w.gate_min = opts[3];
    o.flow_cols = opts[4]; if (opts[5] > 0) o.flow_rows = opts[5];
    h.w.skip_idle_wait = opts[6] != 0;
    const std::vector<uint8_t> pr(present, present + (size_t)nt * nt);
    h.s = apex::plan_structure(nt, pr, o);
    h.err = apex::build_plan_lists(h.s, pr, o, reinterpret_cast<double*>(apex::kStandInTiles), reinterpret_cast<double*>(apex::kStandInLinv), &h.l);
    return h;
}

// One table of apexgpu_debug_plan_lists (include/apexgpu.h) as rows of `*width` integers.  Tiles by name: (array, index) with
// array 0 the tiles (index = slot), 1 linv (index = tile column), (-1, -1) null.
static int plan_table(const apex::PlanStructure& s, const apex::PlanLists& l, const double* tiles, const double* linv, int which, std::vector<int64_t>* out, int* width) {
    constexpr ptrdiff_t kTile = (ptrdiff_t)apex::kNB * apex::kNB;
    auto clean = [](const double* p) { return reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(p) & ~uintptr_t(7)); };
    auto in_linv = [&](const double* p) { return p >= linv && p < linv + s.nt * kTile; };
    auto arr = [&](const double* p) -> int64_t { p = clean(p); return !p ? -1 : in_linv(p) ? 1 : 0; };
    auto idx = [&](const double* p) -> int64_t { p = clean(p); return !p ? -1 : in_linv(p) ? (p - linv) / kTile : (p - tiles) / kTile; };
    auto bits = [](double v) { int64_t b; memcpy(&b, &v, sizeof b); return b; };
    auto row = [&](std::initializer_list<int64_t> v) { *width = (int)v.size(); out->insert(out->end(), v); };
    auto gemm = [&](const std::vector<apex::GemmTask>& v) {
        *width = 7;
        for (const apex::GemmTask& t : v) row({arr(t.C), idx(t.C), (int64_t)(reinterpret_cast<uintptr_t>(t.C) & 1), arr(t.A), idx(t.A), arr(t.B), idx(t.B)});
    };
    auto tri = [&](const std::vector<apex::TriTask>& v) {
        *width = 6;
        for (const apex::TriTask& t : v) row({arr(t.Mdiag), idx(t.Mdiag), arr(t.Moff), idx(t.Moff), t.k, t.other});
    };
    auto flow = [&](const std::vector<apex::FlowTask>& v) {
        *width = 10;
        for (const apex::FlowTask& t : v) row({arr(t.mat), idx(t.mat), t.src, t.dst, t.part, t.count, arr(t.mat2), idx(t.mat2), t.src2, t.slot2});
    };
    const int nt = s.nt;
    switch (which) {
        case 0: {
            const apex::PlanLists::Flow* f = l.flow;
            row({s.n_levels(), s.n_local_groups, s.n_top_cols, s.n_slots, s.n_touched, (int64_t)l.potrf.size(), (int64_t)l.panel.size(), (int64_t)l.upd.size(),
                 l.two_side_plan, l.first_ok, f[0].g0, f[0].g1, f[0].first, f[0].n, f[1].g0, f[1].g1, f[1].first, f[1].n, l.n_flow_local, l.n_flow_parts,
                 bits(s.predicted_ms), bits(f[0].sim_us), bits(f[1].sim_us)});
            break;
        }
        case 1: *width = 3; for (int I = 0; I < nt; ++I) for (int J = 0; J < nt; ++J) if (s.slot_of(I, J) >= 0) row({I, J, s.slot_of(I, J)}); break;
        case 2: *width = 4; for (int K = 0; K < nt; ++K) row({K, s.cls[K], s.owner[K], s.diag_slot[K]}); break;
        case 3:   // per owner: its touched and fill slot ranges; last the ranges of the shared top
            for (size_t o = 0; o < s.own_range.size(); ++o) row({(int64_t)o, s.own_range[o].first, s.own_range[o].second, s.own_fill[o].first, s.own_fill[o].second});
            row({-1, s.n_t_nt, s.n_touched - s.n_t_nt, s.n_f_nt, s.n_slots - s.n_f_nt});
            break;
        case 4: *width = 9; for (const apex::Level& v : l.lv) row({v.potrf, v.panel, v.fwd, v.upd, v.u1o, v.u2a, v.u2b1, v.u2b2, (int64_t)v.fwd_cut.size()}); break;
        case 5: *width = 2; for (size_t g = 0; g < l.lv.size(); ++g) for (int c : l.lv[g].fwd_cut) row({(int64_t)g, c}); break;
        case 6: *width = 2; for (const auto& r : l.upd_rounds) row({r.first, r.second}); break;
        case 7: *width = 1; for (int b : l.bwd_step) row({b}); break;
        case 8: *width = 5; for (const apex::PotrfTask& t : l.potrf) row({arr(t.A), idx(t.A), arr(t.Linv), idx(t.Linv), t.K}); break;
        case 9: gemm(l.panel); break;
        case 10: gemm(l.upd); break;
        case 11: tri(l.fwd); break;
        case 12: tri(l.bwd); break;
        case 13: flow(l.flow_fwd); break;
        case 14: flow(l.flow_bwd); break;
        case 15:
            *width = 16;
            for (const apex::FactorUnit& u : l.units)
                row({arr(u.C), idx(u.C), arr(u.A), idx(u.A), arr(u.B), idx(u.B), u.wait_flag[0], u.wait_flag[1], u.wait_flag[2], u.wait_val[0], u.wait_val[1], u.wait_val[2],
                     u.pub, u.kind, u.strip, u.pad});
            break;
        case 16: *width = 1; for (int v : l.sym_row_ptr) row({v}); break;
        case 17: *width = 3; for (const apex::SymEntry& e : l.sym_entries) row({e.slot, e.other, e.kind}); break;
        case 18: *width = 3; for (const apex::SymTile& t : l.sym_tiles) row({t.slot, t.I, t.J}); break;
        case 19: *width = 2; for (size_t g = 0; g < s.group_cols.size(); ++g) for (int K : s.group_cols[g]) row({(int64_t)g, K}); break;
        default: return APEXGPU_ERR_INVALID_INPUT;
    }
    return APEXGPU_OK;
}

// rows of apexgpu_debug_sinv_lists / _direct (include/apexgpu.h)
static int sinv_rows(const apex::SinvLists& l, int64_t* rows, int max_rows, int64_t counts[4]) {
    const size_t n = l.tasks.size() + l.prods.size();
    size_t i = 0;
    for (size_t g = 0; g < l.groups.size(); ++g)
        for (int k = 0; k < 3; ++k)
            for (int t = l.groups[g][k]; t < l.groups[g][k + 1] && i < (size_t)max_rows; ++t, ++i) {
                const apex::SinvTaskH& tk = l.tasks[t];
                int64_t* r = rows + 6 * i;
                r[0] = k; r[1] = (int64_t)g; r[2] = tk.C.array; r[3] = tk.C.tile; r[4] = tk.first; r[5] = tk.count;
            }
    for (size_t p = 0; p < l.prods.size() && l.tasks.size() + p < (size_t)max_rows; ++p) {
        const apex::SinvProdH& pr = l.prods[p];
        int64_t* r = rows + 6 * (l.tasks.size() + p);
        r[0] = 3; r[1] = pr.A.array; r[2] = pr.A.tile; r[3] = pr.B.array; r[4] = pr.B.tile; r[5] = pr.op;
    }
    if (counts) { counts[0] = l.n[0]; counts[1] = l.n[1]; counts[2] = l.n[2]; counts[3] = l.y_max; }
    return (int)n;
}

// Host arithmetic only (no device is touched): the sorted camera-pair lists k_schur_pairs consumes (csrc/schur_pairs.h)
// for the observation list (cam_idx, pt_idx), with the caller's camera order and a dense tile map (slot of tile (I, J),
// I >= J, = I (I + 1) / 2 + J).  Two-call pattern: with every output NULL the sizes come back in counts[4] = {slots,
// chunks, blocks, tasks}; o_index_out[n_obs] receives the landmark-major position -> caller's observation index map that
// the records' i / j refer to.  Lets CPU tests replay the kernel's bookkeeping (block boundaries, padding, flush points).
static int debug_pair_lists_impl(int64_t n_cam, int64_t n_pt, int64_t n_obs, int dc, const uint32_t* cam_idx, const uint32_t* pt_idx,
                                 int64_t counts[4], uint32_t* recs4_out, int32_t* chunks2_out, int64_t* blocks4_out,
                                 int32_t* tasks2_out, int32_t* o_index_out, bool queued, int64_t* qdesc3_out) {
    if (n_cam <= 0 || n_pt <= 0 || n_obs < 0 || (dc != 6 && dc != 9) || !cam_idx || !pt_idx || !counts) return APEXGPU_ERR_INVALID_INPUT;
    return guarded([&]() -> int {
        for (int64_t i = 0; i < n_obs; ++i)
            if (cam_idx[i] >= (uint64_t)n_cam || pt_idx[i] >= (uint64_t)n_pt) return APEXGPU_ERR_INVALID_INPUT;
        std::vector<int> pt_ptr(n_pt + 1, 0), order(n_obs);
        for (int64_t i = 0; i < n_obs; ++i) pt_ptr[pt_idx[i] + 1]++;
        for (int64_t l = 0; l < n_pt; ++l) pt_ptr[l + 1] += pt_ptr[l];
        { std::vector<int> fill(pt_ptr.begin(), pt_ptr.end() - 1); for (int64_t i = 0; i < n_obs; ++i) order[fill[pt_idx[i]]++] = (int)i; }
        for (int64_t l = 0; l < n_pt; ++l)
            std::stable_sort(order.begin() + pt_ptr[l], order.begin() + pt_ptr[l + 1], [&](int a, int b) { return cam_idx[a] < cam_idx[b]; });
        std::vector<uint32_t> o_cam(n_obs), o_pt(n_obs);
        for (int64_t k = 0; k < n_obs; ++k) { o_cam[k] = cam_idx[order[k]]; o_pt[k] = pt_idx[order[k]]; }
        std::vector<int> cam_ptr(n_cam + 1, 0), cam_obs(n_obs);
        for (int64_t k = 0; k < n_obs; ++k) cam_ptr[o_cam[k] + 1]++;
        for (int64_t c = 0; c < n_cam; ++c) cam_ptr[c + 1] += cam_ptr[c];
        { std::vector<int> fill(cam_ptr.begin(), cam_ptr.end() - 1); for (int64_t k = 0; k < n_obs; ++k) cam_obs[fill[o_cam[k]]++] = (int)k; }
        const int nt = (int)((n_cam * dc + apex::kNB - 1) / apex::kNB);
        std::vector<int> slot((size_t)nt * nt, -1);
        for (int I = 0; I < nt; ++I) for (int J = 0; J <= I; ++J) slot[(size_t)I * nt + J] = I * (I + 1) / 2 + J;
        std::vector<int> ext(n_cam);
        for (int64_t c = 0; c < n_cam; ++c) ext[c] = (int)c;
        apex::PairLists pl;
        apex::build_pair_lists(dc, nt, slot.data(), n_cam, ext.data(), o_cam.data(), o_pt.data(), pt_ptr.data(), cam_ptr.data(), cam_obs.data(), &pl, 0, queued);
        counts[0] = (int64_t)pl.recs.size(); counts[1] = (int64_t)pl.chunks.size(); counts[2] = (int64_t)pl.blocks.size(); counts[3] = (int64_t)pl.tasks.size();
        if (recs4_out) memcpy(recs4_out, pl.recs.data(), pl.recs.size() * sizeof(apex::PairRec));
        if (chunks2_out) memcpy(chunks2_out, pl.chunks.data(), pl.chunks.size() * sizeof(apex::PairChunk));
        if (blocks4_out)
            for (size_t b = 0; b < pl.blocks.size(); ++b) {
                blocks4_out[4 * b] = pl.blocks[b].dst; blocks4_out[4 * b + 1] = pl.blocks[b].ci; blocks4_out[4 * b + 2] = pl.blocks[b].cj;
                blocks4_out[4 * b + 3] = pl.blocks[b].flags;
            }
        if (tasks2_out) memcpy(tasks2_out, pl.tasks.data(), pl.tasks.size() * sizeof(apex::PairTask));
        if (o_index_out) for (int64_t k = 0; k < n_obs; ++k) o_index_out[k] = order[k];
        if (qdesc3_out)
            for (size_t q = 0; q < pl.qdesc.size(); ++q) { qdesc3_out[3 * q] = pl.qdesc[q].dst; qdesc3_out[3 * q + 1] = pl.qdesc[q].cj; qdesc3_out[3 * q + 2] = pl.qdesc[q].flags; }
        return APEXGPU_OK;
    });
}

extern "C" {

int apexgpu_debug_lockstep_solve(apexgpu_solver** hs, int n, double lambda) {
    return guarded([&] { return lockstep_solve_impl(hs, n, lambda); });
}

// Host arithmetic only (no device is touched): the cut of the tile elimination tree that a distributed plan of `world`
// ranks makes for the lower-triangular tile structure `present` (nt x nt, row-major, I >= J).  owner_out[nt]: owning
// rank of every tile column, -1 for the shared top; returns the number of top columns (0: the plan stays replicated).
int apexgpu_debug_partition(int nt, const uint8_t* present, int world, int* owner_out) {
    if (nt <= 0 || !present || !owner_out || world < 1) return APEXGPU_ERR_INVALID_INPUT;
    return guarded([&]() -> int {
    const std::vector<int> owner = apex::plan_owners(nt, std::vector<uint8_t>(present, present + (size_t)nt * nt), world);
    if (owner.empty()) { for (int i = 0; i < nt; ++i) owner_out[i] = 0; return 0; }
    int n_top = 0;
    for (int i = 0; i < nt; ++i) { owner_out[i] = owner[i]; n_top += owner[i] < 0; }
    return n_top;
    });
}

int apexgpu_debug_check_schedule(int nt, const uint8_t* present, int world, int rank, const int opts[8], int64_t out[8], char* msg, int msg_len) {
    if (nt <= 0 || !present || !opts || !out || world < 1 || rank < 0 || rank >= world) return APEXGPU_ERR_INVALID_INPUT;
    return guarded([&]() -> int {
    const HostPlan hp = host_plan(nt, present, world, rank, opts);
    const std::string& e = hp.err;
    std::string first;
    if (!e.empty()) { if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", e.c_str()); return APEXGPU_ERR_INVALID_STATE; }
    for (int k = 0; k < 8; ++k) out[k] = 0;
    for (int ph = 0; ph < 2; ++ph) {
        std::vector<apex::SchedOp> ops = hp.schedule(ph);
        if (opts[7] >= 0 && ph == 0) {   // drop the opts[7]-th stream wait of the sequence: the checker must notice when it mattered
            int seen = 0;
            for (size_t i = 0; i < ops.size(); ++i)
                if (ops[i].op == apex::kOpWait && seen++ == opts[7]) { ops.erase(ops.begin() + (long)i); out[7] = 1; break; }
        }
        std::string why;
        const int bad = apex::check_schedule(ops, hp.l.potrf, hp.l.panel, hp.l.upd, hp.l.units, &why);
        for (const apex::SchedOp& o : ops) { out[0] += o.op <= apex::kOpWait; out[1] += o.op == apex::kOpLaunch; out[6] += o.op == apex::kOpWait; }
        out[2 + ph] = bad;
        if (bad && first.empty()) first = why;
    }
    const apex::PlanLists::Flow* f = hp.l.flow;
    out[4] = f[0].n + f[1].n; out[5] = (f[0].g1 - f[0].g0) + (f[1].g1 - f[1].g0);
    if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", first.c_str());
    return hp.s.n_levels();
    });
}

int apexgpu_debug_schedule_ops(int nt, const uint8_t* present, int world, int rank, const int opts[8], int phase, int64_t* rows, int max_rows) {
    if (nt <= 0 || !present || !opts || world < 1 || rank < 0 || rank >= world || phase < 0 || phase > 1 || max_rows < 0 || (max_rows > 0 && !rows)) return APEXGPU_ERR_INVALID_INPUT;
    return guarded([&]() -> int {
    const HostPlan hp = host_plan(nt, present, world, rank, opts);
    if (!hp.err.empty()) return APEXGPU_ERR_INVALID_STATE;
    const std::vector<apex::SchedOp> ops = hp.schedule(phase);
    for (size_t i = 0; i < ops.size() && i < (size_t)max_rows; ++i) {
        const apex::SchedOp& o = ops[i];
        int64_t* r = rows + 6 * i;
        r[0] = o.op; r[1] = (int64_t)o.stream; r[2] = (int64_t)o.event; r[3] = o.list; r[4] = o.first; r[5] = o.count;
    }
    return (int)ops.size();
    });
}

int apexgpu_debug_plan_lists(int nt, const uint8_t* present, int world, int rank, const int opts[8], int which, int64_t* rows, int max_rows) {
    if (nt <= 0 || !present || !opts || world < 1 || rank < 0 || rank >= world || max_rows < 0 || (max_rows > 0 && !rows)) return APEXGPU_ERR_INVALID_INPUT;
    return guarded([&]() -> int {
    const HostPlan hp = host_plan(nt, present, world, rank, opts);
    if (!hp.err.empty()) return APEXGPU_ERR_INVALID_STATE;
    std::vector<int64_t> out;
    int width = 1;
    const int rc = plan_table(hp.s, hp.l, reinterpret_cast<const double*>(apex::kStandInTiles), reinterpret_cast<const double*>(apex::kStandInLinv), which, &out, &width);
    if (rc != APEXGPU_OK) return rc;
    const size_t n = out.size() / (size_t)width;
    if (max_rows > 0) memcpy(rows, out.data(), std::min(n, (size_t)max_rows) * (size_t)width * sizeof(int64_t));
    return (int)n;
    });
}

int apexgpu_debug_sinv_lists(int nt, const uint8_t* present, int64_t* rows, int max_rows, int64_t counts[4], int32_t* slot_out) {
    if (nt <= 0 || !present || max_rows < 0 || (max_rows > 0 && !rows)) return APEXGPU_ERR_INVALID_INPUT;
    return guarded([&]() -> int {
    const apex::PlanStructure s = apex::plan_structure(nt, std::vector<uint8_t>(present, present + (size_t)nt * nt), apex::PlanOptions());
    if (s.refused) return APEXGPU_ERR_INVALID_STATE;
    if (slot_out) memcpy(slot_out, s.slot.data(), (size_t)nt * nt * sizeof(int32_t));
    apex::SinvLists lists;
    if (!apex::build_sinv_lists(nt, s.slot.data(), s.group_cols, &lists).empty()) return APEXGPU_ERR_INVALID_STATE;
    return sinv_rows(lists, rows, max_rows, counts);
    });
}

int apexgpu_debug_sinv_lists_direct(int nt, const int32_t* slot, int n_groups, const int32_t* group_ptr, const int32_t* group_cols,
                                    int64_t* rows, int max_rows, int64_t counts[4], char* msg, int msg_len) {
    if (nt <= 0 || !slot || n_groups < 0 || !group_ptr || !group_cols || max_rows < 0 || (max_rows > 0 && !rows)) return APEXGPU_ERR_INVALID_INPUT;
    return guarded([&]() -> int {
    std::vector<std::vector<int>> groups(n_groups);
    for (int g = 0; g < n_groups; ++g) {
        if (group_ptr[g] < 0 || group_ptr[g + 1] < group_ptr[g]) return APEXGPU_ERR_INVALID_INPUT;
        for (int i = group_ptr[g]; i < group_ptr[g + 1]; ++i) {
            if (group_cols[i] < 0 || group_cols[i] >= nt || slot[(size_t)group_cols[i] * nt + group_cols[i]] < 0) return APEXGPU_ERR_INVALID_INPUT;
            groups[g].push_back(group_cols[i]);
        }
    }
    apex::SinvLists lists;
    const std::string e = apex::build_sinv_lists(nt, slot, groups, &lists);
    if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", e.c_str());
    if (!e.empty()) return APEXGPU_ERR_INVALID_STATE;
    return sinv_rows(lists, rows, max_rows, counts);
    });
}

int apexgpu_shard_range(int64_t n_pt, int64_t n_obs, const uint32_t* pt_idx, int rank, int world, int64_t* lo, int64_t* hi) {
    if (!pt_idx || !lo || !hi || world < 1 || rank < 0 || rank >= world || n_pt <= 0) return APEXGPU_ERR_INVALID_INPUT;
    return guarded([&]() -> int {
        std::vector<int64_t> ptr(n_pt + 1, 0);
        for (int64_t i = 0; i < n_obs; ++i) {
            if (pt_idx[i] >= (uint64_t)n_pt) return APEXGPU_ERR_INVALID_INPUT;
            ptr[pt_idx[i] + 1]++;
        }
        for (int64_t l = 0; l < n_pt; ++l) ptr[l + 1] += ptr[l];
        apex::shard_range(n_pt, ptr.data(), rank, world, lo, hi);
        return APEXGPU_OK;
    });
}

int apexgpu_debug_pair_lists(int64_t n_cam, int64_t n_pt, int64_t n_obs, int dc, const uint32_t* cam_idx, const uint32_t* pt_idx,
                             int64_t counts[4], uint32_t* recs4_out, int32_t* chunks2_out, int64_t* blocks4_out,
                             int32_t* tasks2_out, int32_t* o_index_out) {
    return debug_pair_lists_impl(n_cam, n_pt, n_obs, dc, cam_idx, pt_idx, counts, recs4_out, chunks2_out, blocks4_out, tasks2_out, o_index_out, false, nullptr);
}
// The same in the QUEUED layout ("schur_form" 4, d_c = 9; csrc/schur_pairs.h): qdesc3_out[8 * chunks][3] = {dst, cj, flags} of
// every (chunk, queue) -- entry 7 of a chunk: cj = the row's camera --, chunks2_out[.][0] = the chunk's flush bits.
int apexgpu_debug_pair_lists_queued(int64_t n_cam, int64_t n_pt, int64_t n_obs, const uint32_t* cam_idx, const uint32_t* pt_idx,
                                    int64_t counts[4], uint32_t* recs4_out, int32_t* chunks2_out, int64_t* blocks4_out,
                                    int32_t* tasks2_out, int32_t* o_index_out, int64_t* qdesc3_out) {
    return debug_pair_lists_impl(n_cam, n_pt, n_obs, 9, cam_idx, pt_idx, counts, recs4_out, chunks2_out, blocks4_out, tasks2_out, o_index_out, true, qdesc3_out);
}
// ... and for either camera width (round 5): dc = 9 as above; dc = 6: sixteen queues of four pairs per chunk, qdesc3_out[17 * chunks][3],
// entry 16 of a chunk = the row's camera
int apexgpu_debug_pair_lists_queued_dc(int64_t n_cam, int64_t n_pt, int64_t n_obs, int dc, const uint32_t* cam_idx, const uint32_t* pt_idx,
                                       int64_t counts[4], uint32_t* recs4_out, int32_t* chunks2_out, int64_t* blocks4_out,
                                       int32_t* tasks2_out, int32_t* o_index_out, int64_t* qdesc3_out) {
    return debug_pair_lists_impl(n_cam, n_pt, n_obs, dc, cam_idx, pt_idx, counts, recs4_out, chunks2_out, blocks4_out, tasks2_out, o_index_out, true, qdesc3_out);
}

// Host arithmetic only: everything apexgpu_set_structure derives from the observation list before it touches the device
// (csrc/ba_structure.h) -- camera order with hub cameras last and nested dissection of the tile graph, symbolic fill,
// partition of the elimination tree, landmark sharding, the lists of the Schur reduction -- for rank `rank` of `world`.
// opts[5] = {nested_dissection (0 off, 1 on, > 1 leaf size), hubs_last, dist_factor, tree_sharding, schur_form}.
// stats_out[16] = {tile rows, hub cameras, border tiles, tiles S touches, tiles after fill, elimination-tree levels,
// shared top columns, tree sharded, seconds: order+structure, sharding+lists, (unused), Schur lists, (unused), total,
// pair contributions incl. self pairs, camera-pair blocks}.  cmap_out[n_cam] (caller's camera -> internal), owned_out[n_pt]
// (1: this rank assembles the landmark), tile_owner_out[tile rows] (-1: shared top / not distributed) may be NULL.
int apexgpu_debug_host_structure(int64_t n_cam, int64_t n_pt, int64_t n_obs, int mode, const uint32_t* cam_idx,
                                 const uint32_t* pt_idx, int rank, int world, const int opts[5], double stats_out[16],
                                 int32_t* cmap_out, uint8_t* owned_out, int32_t* tile_owner_out) {
    if (n_cam <= 0 || n_pt <= 0 || n_obs < 0 || !cam_idx || !pt_idx || !opts || !stats_out || world < 1 || rank < 0 || rank >= world)
        return APEXGPU_ERR_INVALID_INPUT;
    if (mode < APEXGPU_MODE_BUNDLE_ADJUSTMENT || mode > APEXGPU_MODE_LANDMARKS_AND_INTRINSICS) return APEXGPU_ERR_INVALID_INPUT;
    return guarded([&]() -> int {
        for (int64_t i = 0; i < n_obs; ++i)
            if (cam_idx[i] >= (uint64_t)n_cam || pt_idx[i] >= (uint64_t)n_pt) return APEXGPU_ERR_INVALID_INPUT;
        apex::BaStructOptions so;
        so.dc = (apex::mode_mask(mode) & 1) ? 9 : 6;
        so.use_nd = opts[0] != 0; if (opts[0] > 1) so.nd_leaf = opts[0];
        so.hubs_last = opts[1] != 0; so.dist_factor = opts[2] != 0; so.tree_sharding = opts[3] != 0; so.schur_form = opts[4];
        so.rank = rank; so.world = world;
        apex::BaHostStructure hs;
        std::vector<double> uv(2 * (size_t)n_obs, 0.0);
        const std::string e = hs.build_lists(n_cam, n_pt, n_obs, cam_idx, pt_idx, uv.data(), so);
        if (!e.empty()) return APEXGPU_ERR_INVALID_INPUT;
        apex::PlanOptions po;
        po.rank = hs.part_rank; po.world = hs.part_world; po.own_all = hs.part_own_all;
        const apex::PlanStructure ps = apex::plan_structure(hs.nt, hs.present, po);
        hs.build_schur_lists(so, ps.slot.data());
        const double t_all = hs.seconds[0] + hs.seconds[1] + hs.seconds[3];
        const double st[16] = {(double)hs.nt, (double)hs.n_hubs, (double)hs.n_border_tiles, (double)hs.n_present, (double)ps.n_slots,
                               (double)ps.n_true_levels, (double)ps.n_top_cols, hs.tree_shard ? 1.0 : 0.0, hs.seconds[0], hs.seconds[1],
                               0.0, hs.seconds[3], 0.0, t_all, (double)hs.n_pairs, (double)hs.pl.n_blocks};
        for (int k = 0; k < 16; ++k) stats_out[k] = st[k];
        if (cmap_out) for (int64_t c = 0; c < n_cam; ++c) cmap_out[c] = hs.cmap[c];
        if (owned_out) for (int64_t l = 0; l < n_pt; ++l) owned_out[l] = (hs.lmap[l] >= hs.lm_lo && hs.lmap[l] < hs.lm_hi) ? 1 : 0;
        if (tile_owner_out) {
            for (int t = 0; t < hs.nt; ++t) tile_owner_out[t] = ps.n_top_cols > 0 ? ps.owner[t] : -1;
        }
        return APEXGPU_OK;
    });
}

// Parity probe: the device's eigenvalue-gated 3x3 inverse (invert_landmark_blocks_with_lambda with lambda = 0,
// explicit_schur.rs:365-442) applied to n caller-supplied symmetric blocks on GPU `device`.
int apexgpu_debug_invert_blocks(int device, int64_t n, const double* blocks9, double* inv9_out, int32_t* ok_out) {
    if (n < 0 || (n > 0 && (!blocks9 || !inv9_out || !ok_out))) return APEXGPU_ERR_INVALID_INPUT;
    if (n == 0) return APEXGPU_OK;
    if (hipSetDevice(device) != hipSuccess) return APEXGPU_ERR_DEVICE;
    apex::DeviceBuffer<double> din, dout;
    apex::DeviceBuffer<int> dok;
    int rc = APEXGPU_ERR_DEVICE;
    if (din.alloc(9 * n) == hipSuccess && dout.alloc(9 * n) == hipSuccess && dok.alloc(n) == hipSuccess &&
        hipMemcpy(din, blocks9, 9 * n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess) {
        apex::launch_debug_invert_blocks(n, din, dout, dok, nullptr);
        if (hipMemcpy(inv9_out, dout, 9 * n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(ok_out, dok, n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
            rc = APEXGPU_OK;
    }
    return rc;
}

}  // extern "C"
