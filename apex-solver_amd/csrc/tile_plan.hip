// tile_plan.hip -- see tile_plan.h
#include "tile_plan.h"
#include "host_parallel.h"

#include <chrono>
#include <thread>

#include <stdlib.h>

#include <algorithm>

namespace apex {

void TilePlan::release() {
    for (int i = 0; i < kGraphs; ++i) {   // the graph execs first: their nodes point into the buffers freed below
        if (graph_exec_[i]) { (void)hipGraphExecDestroy(graph_exec_[i]); graph_exec_[i] = nullptr; }
        graph_failed_[i] = false;
    }
    inverse_.release();
    pcg_.release();
    tiles_written();
    static_cast<TilePlanMemory&>(*this) = TilePlanMemory();   // frees every device and pinned block of the plan
    lists_ = PlanLists(); sw_.flow_on = true; flow_gave_up_ = false;
    flow_err_host_dev_ = nullptr;
    if (occ_stream_) { (void)hipStreamSynchronize(occ_stream_); (void)hipStreamDestroy(occ_stream_); occ_stream_ = nullptr; }
    for (const auto& evs : ev_) for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    ev_.clear();
}

TilePlan::~TilePlan() {
    release();
    for (hipStream_t s : {side_, side2_, so_})
        if (s) (void)hipStreamDestroy(s);
}

// the one refusal that asks the device
std::string TilePlan::refuse_by_memory() {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const double need = (double)(structure_.n_slots + structure_.nt) * kNB * kNB * 8.0;
    if (need <= 0.9 * (double)free_b) return "";
    refused_ = 2;
    return "the tile matrix needs " + std::to_string(need / 1e9) + " GB; only " + std::to_string(free_b / 1e9) + " GB free";
}

#define TP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return std::string("HIP error in " #expr ": ") + hipGetErrorString(_e); } while (0)

std::string TilePlan::build(int nt, const std::vector<uint8_t>& present, hipStream_t stream) {
    release();
    stream_ = stream;
    SetupTrace ptr_trace;
    structure_ = plan_structure(nt, present, opts_);
    refused_ = structure_.refused;
    if (refused_) return structure_.message;
    std::string e = refuse_by_memory();
    if (!e.empty()) return e;
    ptr_trace.mark("plan: symbolic fill, slots");
    TP_TRY(tiles_.alloc_zero((size_t)structure_.n_slots * kNB * kNB));
    TP_TRY(linv_.alloc_zero((size_t)structure_.nt * kNB * kNB));
    ptr_trace.mark("plan: tiles allocated, cleared");
    e = build_plan_lists(structure_, present, opts_, tiles_, linv_, &lists_);
    if (!e.empty()) return e;
    ptr_trace.mark("plan: task lists, dataflow units");
    e = upload();
    if (e.empty()) ptr_trace.mark("plan: uploads, streams, events");
    return e;
}

// The device step of build(): the lists and maps to the device, the work arrays, the streams and events.
std::string TilePlan::upload() {
    TP_TRY(slot_.upload(structure_.slot));
    TP_TRY(diag_slot_.upload(structure_.diag_slot));
    TP_TRY(flag_.alloc_zero(4));
    TP_TRY(flow_units_.upload(lists_.units));
    TP_TRY(flow_ver_.alloc_zero((size_t)structure_.n_slots));
    TP_TRY(sym_tiles_.upload(lists_.sym_tiles));
    TP_TRY(pcg_.setup(PcgPlanView{tiles_, diag_slot_, sym_tiles_, n_sym_tiles(), structure_.nt, n_pad(), stream_}, lists_, structure_.n_slots));
    TP_TRY(tri_fwd_.upload(lists_.fwd));
    TP_TRY(tri_bwd_.upload(lists_.bwd));
    TP_TRY(flow_fwd_.upload(lists_.flow_fwd));
    TP_TRY(flow_bwd_.upload(lists_.flow_bwd));
    TP_TRY(flow_part_.alloc_zero((size_t)std::max(lists_.n_flow_parts, 1) * kNB));
    TP_TRY(flow_flags_.alloc_zero((size_t)2 * structure_.nt + 1));   // cnt[nt] | done[nt] | error word of the dataflow sweeps
    if (!flow_err_host_) {
        TP_TRY(flow_err_host_.alloc(4));
        flow_err_host_[0] = flow_err_host_[1] = flow_err_host_[2] = flow_err_host_[3] = 0;
        void* dp = nullptr;   // (pinned host memory is mapped: the kernels that post a word write it through this address)
        flow_err_host_dev_ = hipHostGetDevicePointer(&dp, flow_err_host_, 0) == hipSuccess ? static_cast<int*>(dp) : nullptr;
        (void)hipGetLastError();
    }
    TP_TRY(potrf_tasks_.upload(lists_.potrf));
    TP_TRY(trsm_tasks_.upload(lists_.panel));
    TP_TRY(upd_tasks_.upload(lists_.upd));
    TP_TRY(cls_.upload(structure_.cls));
    TP_TRY(exch_.alloc_zero((size_t)n_pad()));
    // (a lowest-priority side stream was tried: no gain without graphs, +2.7 ms with them)
    // (and so was a CU-masked one that leaves 1 CU in 8 / 4 / 2 to the critical path: the same, either way)
    for (hipStream_t* s : {&side_, &so_, &side2_})
        if (!*s) TP_TRY(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    ev_.assign(structure_.n_levels(), {});
    for (auto& evs : ev_)
        for (hipEvent_t& ev : evs) TP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    TP_TRY(gate_cnt_.alloc((size_t)(structure_.n_levels() + 1)));
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
    if (distributed() && !opts_.own_all && opts_.rank < (int)structure_.own_range.size()) {
        // a rank of a distributed plan factorises its own columns and the shared top: the fill tiles of the other ranks'
        // columns are never touched; their touched tiles only when this rank's landmarks may add to them (range sharding)
        if (own_touched_only) { clear(structure_.own_range[opts_.rank].first, structure_.own_range[opts_.rank].second); clear(structure_.n_t_nt, structure_.n_touched - structure_.n_t_nt); }
        else clear(0, structure_.n_touched);
        clear(structure_.own_fill[opts_.rank].first, structure_.own_fill[opts_.rank].second);
        clear(structure_.n_f_nt, structure_.n_slots - structure_.n_f_nt);
    } else {
        clear(0, (skip_fill && lists_.first_ok) ? structure_.n_touched : structure_.n_slots);
    }
    if (e != hipSuccess) return e;
    launch_clear_i32(flag_, 4, stream_);
    return hipGetLastError();
}

void TilePlan::add_diag(int n_valid, double add_valid, double pad_value) {
    tiles_written();
    launch_tile_add_diag(tiles_, diag_slot_, n_valid, (int)n_pad(), add_valid, pad_value, stream_);
}

void TilePlan::scale_sym(const double* scale) { tiles_written(); launch_tile_scale_sym(sym_tiles_, n_sym_tiles(), tiles_, scale, stream_); }

void TilePlan::diag(double* out) const { launch_tile_diag(tiles_, diag_slot_, structure_.nt, out, stream_); }

// forward step of level group lv: one launch, or one per column where the plan asks for it (Level::fwd_cut)
void TilePlan::launch_fwd_group(int lv, double* bvec, double* yvec, hipStream_t s) {
    const std::vector<int>& cut = lists_.lv[lv].fwd_cut;
    if (cut.size() < 2) {
        launch_tri_step(false, tri_fwd_ + lists_.lv[lv].fwd, lists_.lv[lv + 1].fwd - lists_.lv[lv].fwd, bvec, yvec, s);
        return;
    }
    for (size_t i = 0; i < cut.size(); ++i) {
        const int b = cut[i], e = i + 1 < cut.size() ? cut[i + 1] : lists_.lv[lv + 1].fwd;
        launch_tri_step(false, tri_fwd_ + b, e - b, bvec, yvec, s);
    }
}

// The factorisation and the triangular solves are static launch sequences for a given structure:
// they are captured once into hipGraphs (a few hundred dependent launches would otherwise be paced by
// host launch overhead) and replayed every iteration.
ScheduleInput TilePlan::input() const { return schedule_input(structure_, lists_, sw_); }

// The factorisation's launch sequence (factor_schedule), call by call: the list check_schedule proves is the list issued.
void TilePlan::issue(const std::vector<SchedOp>& ops) {
    for (const SchedOp& o : ops) {
        const hipStream_t s = stream_of(o.stream);
        switch (o.op) {
            case kOpLaunch:
                if (o.list == 0) launch_potrf_inv(potrf_tasks_ + o.first, o.count, flag_, s, o.arrive >= 0 ? gate_cnt_ + o.arrive : nullptr);
                else if (o.list == 1) launch_tile_gemm_nt(trsm_tasks_ + o.first, o.count, 1.0, 0.0, s, /*tri_b=*/true);
                else if (o.list == 2) launch_tile_gemm_nt(upd_tasks_ + o.first, o.count, -1.0, 1.0, s, /*tri_b=*/false, diag_lower());
                else launch_factor_flow(flow_units_ + o.first, o.count, flow_ver_, flag_, flag_ + 1, s, flow_trace_ ? flow_trace_ + 3 * (size_t)o.first : nullptr, diag_lower());
                break;
            case kOpRecord: (void)hipEventRecord(ev_[o.event / kLevelEvents][o.event % kLevelEvents], s); break;
            case kOpWait: (void)hipStreamWaitEvent(s, ev_[o.event / kLevelEvents][o.event % kLevelEvents], 0); break;
            case kOpGate: launch_gate(gate_cnt_ + o.first, o.count, 150, s); break;
            case kOpClearGates: launch_clear_i32(gate_cnt_, o.count, s); break;
            case kOpClearVersions:
                launch_clear_i32(flow_ver_, structure_.n_slots, s);
                if (poison_factor_)   // (tests: the version of the first unit's tile starts hugely negative and is never reached)
                    (void)hipMemsetAsync(flow_ver_ + lists_.units[(size_t)o.first].pub, 0x80, sizeof(int), s);
                break;
        }
    }
}

void TilePlan::enqueue_solve(const double* rhs, double* x, double* work) {
    // L y = rhs (work vector bvec), then L^T x = y (work vector yvec); level by level
    double* bvec = work;
    double* yvec = work + n_pad();
    const bool flow = tri_flow_ && n_flow_fwd() > 0;
    if (flow) {
        launch_tri_flow(false, flow_fwd_, n_flow_fwd(), rhs, yvec, flow_part_, flow_flags_, structure_.nt, stream_, nullptr, nullptr,
                        poison_ == 1 ? structure_.nt - 1 : -1);
    } else {
        (void)hipMemcpyAsync(bvec, rhs, n_pad() * sizeof(double), hipMemcpyDeviceToDevice, stream_);
        for (int lv = 0; lv < structure_.n_levels(); ++lv)
            launch_fwd_group(lv, bvec, yvec, stream_);
    }
    if (flow) {
        launch_tri_flow(true, flow_bwd_, n_flow_bwd(), yvec, x, flow_part_, flow_flags_, structure_.nt, stream_, nullptr, nullptr,
                        poison_ == 2 ? structure_.nt - 1 : -1);
        return;
    }
    for (int s = 0; s < structure_.n_levels(); ++s)
        launch_tri_step(true, tri_bwd_ + lists_.bwd_step[s], lists_.bwd_step[s + 1] - lists_.bwd_step[s], yvec, x, stream_);
}

// The distributed triangular solves (see tile_plan.h).  bvec/yvec as in enqueue_solve; masks: bit (1 << class).
void TilePlan::enqueue_dist_solve(int phase, const double* rhs, double* x, double* work) {
    double* bvec = work;
    double* yvec = work + n_pad();
    const int n = (int)n_pad();
    const int L1 = structure_.n_local_groups;
    const bool flow = tri_flow_ && lists_.n_flow_local > 0;
    if (phase == 0 && flow) {
        // dataflow form: this rank's columns in one launch; its contributions to the shared top blocks are folded
        // straight into the exchange vector (the top blocks of the right-hand side enter the sum once, on rank 0)
        (void)hipMemsetAsync(exch_, 0, n_pad() * sizeof(double), stream_);
        launch_tri_flow(false, flow_fwd_, lists_.n_flow_local, rhs, yvec, flow_part_, flow_flags_, structure_.nt, stream_,
                        opts_.rank == 0 ? rhs : nullptr, exch_);
    } else if (phase == 1 && flow) {
        // the top columns forward (right-hand side = the summed exchange vector), then everything backward, top first.
        // Pull form, fixed fold order: the ranks' copies of the top solution are bitwise equal by construction.
        launch_tri_flow(false, flow_fwd_ + lists_.n_flow_local, n_flow_fwd() - lists_.n_flow_local, exch_, yvec, flow_part_, flow_flags_, structure_.nt,
                        stream_, nullptr, nullptr);
        launch_tri_flow(true, flow_bwd_, n_flow_bwd(), yvec, x, flow_part_, flow_flags_, structure_.nt, stream_, nullptr, nullptr);
        launch_vec_select(n, x, cls_, opts_.rank == 0 ? 6 : 2, exch_, stream_);
    } else if (phase == 0) {
        // the top blocks of the right-hand side enter the sum once (rank 0); every rank adds its columns' updates
        launch_vec_select(n, rhs, cls_, opts_.rank == 0 ? 7 : 3, bvec, stream_);
        for (int lv = 0; lv < L1; ++lv)
            launch_fwd_group(lv, bvec, yvec, stream_);
        launch_vec_select(n, bvec, cls_, 4, exch_, stream_);
    } else if (phase == 1) {
        launch_vec_merge(n, exch_, cls_, 4, bvec, stream_);
        for (int lv = L1; lv < structure_.n_levels(); ++lv)
            launch_fwd_group(lv, bvec, yvec, stream_);
        for (int s = 0; s < structure_.n_levels(); ++s)  // top groups first, then this rank's
            launch_tri_step(true, tri_bwd_ + lists_.bwd_step[s], lists_.bwd_step[s + 1] - lists_.bwd_step[s], yvec, x, stream_);
        launch_vec_select(n, x, cls_, opts_.rank == 0 ? 6 : 2, exch_, stream_);
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
        if (which == kGraphFactor) enqueue_factor(0, structure_.n_local_groups);
        else if (which == kGraphFactorTop) enqueue_factor(structure_.n_local_groups, structure_.n_levels());
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

void TilePlan::set_diag_lower(bool on) {
    if (on == diag_lower()) return;
    opts_.diag_lower = on ? 1 : 0;
    for (int which : {kGraphFactor, kGraphFactorTop})   // the captured launches hold the old value
        if (graph_exec_[which]) { (void)hipGraphExecDestroy(graph_exec_[which]); graph_exec_[which] = nullptr; }
}

hipError_t TilePlan::enable_flow_trace() {
    if (flow_trace_) return hipSuccess;
    const size_t n = 3 * (size_t)std::max(lists_.flow[0].n + lists_.flow[1].n, 1);
    hipError_t e = flow_trace_.alloc(n);
    if (e != hipSuccess) return e;
    for (int which : {kGraphFactor, kGraphFactorTop})   // the captured launches hold the old (null) pointer
        if (graph_exec_[which]) { (void)hipGraphExecDestroy(graph_exec_[which]); graph_exec_[which] = nullptr; }
    return hipMemset(flow_trace_, 0, n * sizeof(unsigned long long));
}

hipError_t TilePlan::read_flow_trace(std::vector<FactorUnit>* units, std::vector<unsigned long long>* stamps) {
    const size_t n = (size_t)(lists_.flow[0].n + lists_.flow[1].n);
    units->resize(n); stamps->resize(3 * n);
    if (n == 0 || !flow_trace_) return hipErrorNotInitialized;
    hipError_t e = hipMemcpy(units->data(), flow_units_, n * sizeof(FactorUnit), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    return hipMemcpy(stamps->data(), flow_trace_, 3 * n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
}

ExchangeList TilePlan::exchange(int point) const {
    const size_t te = (size_t)kNB * kNB;
    const auto tiles = [&](int64_t first, int64_t end) { return ExchangeItem{ExchangeItem::kSum, tiles_ + (size_t)first * te, (size_t)(end - first) * te, -1}; };
    switch (point) {
        case 1: return {tiles(structure_.n_t_nt, structure_.n_touched), tiles(structure_.n_f_nt, structure_.n_slots)};
        case 2: return {{ExchangeItem::kMaxInt, flag_.get(), 2, -1}};  // a failed pivot (or a dataflow time-out) anywhere fails the factorisation everywhere
        case 3: case 4: return {{ExchangeItem::kSum, exch_.get(), (size_t)n_pad(), -1}};
        default: return {};
    }
}

void TilePlan::factor_phase(int phase) {
    tiles_written();
    if (phase == 0) { if (!run_graph(kGraphFactor, nullptr, nullptr, nullptr)) enqueue_factor(0, structure_.n_local_groups); }
    else if (!run_graph(kGraphFactorTop, nullptr, nullptr, nullptr)) enqueue_factor(structure_.n_local_groups, structure_.n_levels());
}

void TilePlan::solve_phase(int phase, const double* rhs, double* x, double* work) {
    if (phase == 2 || !run_graph(kGraphDistSolve0 + phase, rhs, x, work)) enqueue_dist_solve(phase, rhs, x, work);
}

hipError_t TilePlan::factor(int* failed_at, bool defer_flags) {
    tiles_written();
    if (distributed()) {
        if (!comm_) return hipErrorNotInitialized;  // a distributed plan needs its communicator
        factor_phase(0);
        if (!comm_(exchange(1), stream_)) return hipErrorUnknown;
        factor_phase(1);
        if (!comm_(exchange(2), stream_)) return hipErrorUnknown;
        return read_flags(failed_at);
    }
    if (poison_factor_) {   // (tests: the poisoned launch is not part of the captured graphs)
        enqueue_factor(0, structure_.n_levels());
        poison_factor_ = false;
    } else if (!run_graph(kGraphFactor, nullptr, nullptr, nullptr)) enqueue_factor(0, structure_.n_levels());
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
        sw_.flow_on = false;
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
    int* err = flow_flags_ + 2 * (size_t)structure_.nt;
    if (reduce && comm_ && !comm_({{ExchangeItem::kMaxInt, err, 1, -1}}, stream_)) return false;   // (the hook's owner keeps the message)
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
        if (!comm_) return hipErrorNotInitialized;
        solve_phase(0, rhs, x, work);
        if (!comm_(exchange(3), stream_)) return hipErrorUnknown;
        solve_phase(1, rhs, x, work);
        if (!comm_(exchange(4), stream_)) return hipErrorUnknown;
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
    if (tri_flow_ && n_flow_fwd() > 0) (void)post_sweep_status(false);
    return hipGetLastError();
}

SelectedInverse& TilePlan::inverse() {
    SinvPlanView v;
    v.tiles = tiles_; v.linv = linv_; v.slot = slot_; v.diag_slot = diag_slot_;
    v.nt = structure_.nt; v.n_slots = structure_.n_slots; v.stream = stream_;
    v.slot_host = structure_.slot.data(); v.group_cols = &structure_.group_cols;
    v.distributed = distributed() || opts_.world > 1;
    v.factor_valid = factor_valid_; v.factor_epoch = factor_epoch_;
    inverse_.bind(v);
    return inverse_;
}

}  // namespace apex
