// solver.hip -- host orchestration of the MI355X bundle-adjustment backend (see solver.h).
#include "solver.h"
#include "ba_device.hpp"
#include "ba_structure.h"
#include "hessian_csc.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <future>

namespace apex {

void warm_ba_kernels(hipStream_t s);
void warm_schur_pairs(hipStream_t s);
void warm_chol_kernels(hipStream_t s);
void warm_pcg_kernels(hipStream_t s);

// a collective that failed is surfaced as APEXGPU_ERR_DEVICE with the transport's own text (rank_exchange.h)
#define RANK_TRY(expr) do { const int _rc = (expr); if (_rc != kOk) return fail(_rc, ranks_.error()); } while (0)

// OptimizeParams<POSE, LANDMARK, INTRINSIC> of every mode as 4 POSE + 2 LANDMARK + INTRINSIC (src/factors/mod.rs:82-101)
int mode_mask(int mode) {
    static const int m[7] = {6 /* BundleAdjustment */, 7 /* SelfCalibration */, 4 /* OnlyPose */, 2 /* OnlyLandmarks */,
                             1 /* OnlyIntrinsics */, 5 /* PoseAndIntrinsics */, 3 /* LandmarksAndIntrinsics */};
    return (mode >= 0 && mode < 7) ? m[mode] : 7;
}

Solver::Solver(int64_t n_cam, int64_t n_pt, int64_t n_obs, int mode, int device)
    : TileBackend(device, kNumStages, /*nd_leaf=*/16, kStStats, /*n_partial=*/1024), n_cam_(n_cam), n_pt_(n_pt), n_obs_(n_obs), mode_(mode), dc_(mode_mask(mode) & 1 ? 9 : 6) {
    lm_lo_ = 0; lm_hi_ = n_pt;
    HostBlockCache::get().retain();   // (the set-up's host blocks are cached only while a handle is alive: host_parallel.h)
}

Solver::~Solver() {
    if (free_thread_.joinable()) free_thread_.join();
    HostBlockCache::get().release();   // the last handle returns the cached blocks to the system
    hipSetDevice(device_);
    if (stream_) hipStreamSynchronize(stream_);   // (and the join above) before any buffer is freed; stream_last_ destroys the stream after them
    ranks_.close();
    for (hipEvent_t e : pin_ev_) if (e) (void)hipEventDestroy(e);
}

// A hipMemcpy from pageable memory is staged by the runtime in small pieces (0.19 s for the 107 MB of final-13682's points:
// 0.56 GB/s); through two pinned 16 MB chunks the copy runs at memcpy speed with the DMA of one chunk under the memcpy of the
// next.  Asynchronous on stream_ like the copies it replaces (the caller synchronises).
int Solver::upload_staged(void* dst_dev, const void* src_host, size_t bytes) {
    constexpr size_t kChunk = (size_t)16 << 20;
    if (bytes <= ((size_t)1 << 20)) return check_hip(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, stream_), "upload");
    for (int b = 0; b < 2; ++b) {
        if (!pin_[b]) HIP_TRY(pin_[b].alloc(kChunk));
        if (!pin_ev_[b]) HIP_TRY(hipEventCreateWithFlags(&pin_ev_[b], hipEventDisableTiming));
    }
    size_t i = 0;
    for (size_t off = 0; off < bytes; off += kChunk, ++i) {
        const int b = (int)(i & 1);
        const size_t n = std::min(kChunk, bytes - off);
        // a pinned chunk is rewritten only when the DMA that last read it has finished -- also the one a PREVIOUS call (or a
        // call that returned early on an error) left in flight
        if (pin_busy_[b]) { HIP_TRY(hipEventSynchronize(pin_ev_[b])); pin_busy_[b] = false; }
        memcpy(pin_[b], static_cast<const char*>(src_host) + off, n);
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst_dev) + off, pin_[b], n, hipMemcpyHostToDevice, stream_));
        HIP_TRY(hipEventRecord(pin_ev_[b], stream_));
        pin_busy_[b] = true;
    }
    return kOk;
}

BAView Solver::view(int which) const {
    BAView v;
    v.n_cam = n_cam_; v.n_pt = n_pt_; v.n_obs = (int64_t)o_orig_h_.size();
    v.camp = camp_[which]; v.camq = camp_[which] + (size_t)kCamStride * n_cam_; v.pts = pts_[which];
    v.o_cam = o_cam_; v.o_pt = o_pt_; v.o_uv = reinterpret_cast<const double2*>(o_uv_.get()); v.pt_ptr = pt_ptr_;
    // set_loss: no loss, L2 and Huber are what the huber_delta kernels compute, so they run there (the same bits as a delta given
    // to set_structure); every other kind runs the general instantiations, which take general_loss() and do not read this
    v.huber_delta = !loss_set_ ? huber_delta_ : (loss_.kind == kLossHuber ? loss_.p0 : -1.0);
    v.mask_code = mode_mask(mode_);
    v.co_pt = co_pt_; v.co_uv = reinterpret_cast<const double2*>(co_uv_.get()); v.co_rank = co_rank_;
    v.cam_scale = scaled_ ? cam_scale_.dev.get() : nullptr;
    v.pt_scale = scaled_ ? pt_scale_.dev.get() : nullptr;
    v.lam_mask = tree_shard_ ? lam_mask_ : nullptr;
    v.o_slot = o_slot_; v.wg_cam_n = wg_cam_n_; v.wg_cam_list = wg_cam_list_;
    if (ranks_.world() > 1 && lm_hi_ > lm_lo_) {   // the rank's own landmark range, in whole workgroups of kLmWg
        v.lm_wg0 = (int)(lm_lo_ / kLmWg);
        v.lm_wgn = (int)((lm_hi_ + kLmWg - 1) / kLmWg) - v.lm_wg0;
    }
    return v;
}

TileMap Solver::tilemap() const { return tp_.tilemap(); }

void Solver::stage_begin(int st) { timer_.begin(st, stream_); }
void Solver::stage_end(int st) { timer_.end(st, stream_); }

int Solver::set_shard(int rank, int world) {
    if (have_priors()) return fail(kInvalidState, "set_shard: the handle holds camera priors, which are single-rank only");
    if (have_structure_) return fail(kInvalidState, "set_shard must precede set_structure");
    RANK_TRY(ranks_.set_shard(rank, world));
    return kOk;
}

int Solver::adopt_comm(int world, int rank, const MakeComm& make) {
    const int rc = set_shard(rank, world);
    if (rc != kOk) return rc;
    HIP_TRY(hipSetDevice(device_));
    std::string err;
    std::unique_ptr<Communicator> c = make(&err);
    RANK_TRY(ranks_.adopt(std::move(c), err));
    tp_.set_comm([this](const ExchangeList& l, hipStream_t st) { return ranks_.issue(l, st) == kOk; });
    HIP_TRY(ranks_.lm_ranges.alloc(2 * (size_t)world));
    return kOk;
}

int Solver::comm_init(int world, int rank, const void* unique_id128) {
    return adopt_comm(world, rank, [&](std::string* err) { return make_rccl_comm(world, rank, unique_id128, err); });
}

// The same multi-rank schedule over the host shared-memory transport (comm.h): ranks = processes of one node.
int Solver::comm_init_shm(int world, int rank, const char* name) {
    return adopt_comm(world, rank, [&](std::string* err) { return make_shm_comm(world, rank, name, err); });
}

// Landmark range [lo,hi) of `rank`: contiguous, balanced by observation count.  ptr[l] = number of
// observations of landmarks < l (n_pt+1 entries).  Pure host arithmetic, identical on every rank.
void shard_range(int64_t n_pt, const int64_t* ptr, int rank, int world, int64_t* lo, int64_t* hi) {
    const int64_t n_obs = ptr[n_pt];
    auto cut = [&](int r) -> int64_t {
        if (r <= 0) return 0;
        if (r >= world) return n_pt;
        const int64_t target = (n_obs * r) / world;
        return std::min<int64_t>(std::lower_bound(ptr, ptr + n_pt + 1, target) - ptr, n_pt);
    };
    *lo = cut(rank);
    *hi = cut(rank + 1);
}

// ---------------------------------------------------------------------------------------------
// structure
// ---------------------------------------------------------------------------------------------
static double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The state of ONE set_structure call, shared by the calling thread and its three helpers: the device thread (device,
// stream, the caller's measurements, code objects), the planner (tile plan, variant selection) and the uploader (everything
// that does not depend on the plan).  Every field names the one thread that writes it and the point after which the
// others may read it.
struct Solver::Setup {
    // the caller's arguments: set before any thread starts, read-only afterwards
    const uint32_t *cam_idx = nullptr, *pt_idx = nullptr;
    const double* obs_uv = nullptr;
    const int64_t *intr_col = nullptr, *pose_col = nullptr, *pt_col = nullptr;
    const uint8_t *fix_pose = nullptr, *fix_intr = nullptr, *fix_pt = nullptr;
    bool raw_uv_wanted = false;   // single rank: the device thread copies the measurements as they are
    // calling thread, before the planner and the uploader start; schur_form alone is rewritten later (after the planner is
    // joined), and neither helper reads that field
    BaStructOptions so;
    // calling thread.  The planner reads nothing of it (present_plan is its copy); the uploader reads the lists
    // build_obs_lists left, complete before it starts, while the calling thread adds the Schur lists (hs->pl)
    std::unique_ptr<BaHostStructure> hs{new BaHostStructure};
    // planner (or the calling thread where the plan is built in line): read after planner.join()
    std::vector<uint8_t> present_plan;   // the plan's own copy of hs->present: a matrix-free handle keeps the diagonal only
    std::string plan_err;
    double plan_seconds = 0.0;
    // uploader, which keeps its own error text (err_ belongs to the calling thread): read after uploader.join().  The
    // calling thread then adds the pair lists' copy time to up_seconds.  (The uploader also writes the solver's two column
    // maps, from the caller's column lists above and cmap_ / lmap_: nothing reads them before set_structure has returned)
    std::string up_err;
    int up_rc = kOk;
    double up_seconds = 0.0;
    // device thread; the uploader takes it over (and frees it) after joining the device thread
    DeviceBuffer<double> raw_uv;
    // set by the device thread once the device and stream_ are there: device_ready() waits for it on any thread
    std::promise<hipError_t> init_p;
    std::shared_future<hipError_t> init_f = init_p.get_future().share();
    // set by the calling thread (release_device_thread): the 0.5 GB copy of the measurements does not start for a call
    // that is about to be refused.  The device thread waits for it
    std::promise<bool> validated_p;
    std::shared_future<bool> validated_f = validated_p.get_future().share();
    bool validated_set = false;   // calling thread
    SetupTrace tr;                // calling thread
    std::chrono::steady_clock::time_point t_begin;   // calling thread
    // started and joined by the calling thread; the device thread alone is joined by the uploader where it takes raw_uv over
    std::thread device_thread, planner, uploader;

    void release_device_thread(bool valid) {
        if (!validated_set) { validated_set = true; validated_p.set_value(valid); }
    }
    // Every way out of set_structure, early returns and exceptions included: the device thread is released before anything
    // is joined (it may still wait for the verdict on the index lists); the uploader is joined first because it may itself
    // be joining the device thread; the planner waits for nothing but the device thread's first step.
    ~Setup() {
        release_device_thread(false);
        if (uploader.joinable()) uploader.join();
        if (planner.joinable()) planner.join();
        if (device_thread.joinable()) device_thread.join();
    }
};

// The first stream this process creates costs 0.1-0.16 s (the runtime brings up its hardware queues; measured with
// APEX_SETUP_TRACE in bench.py, torch's context already there), the code objects of the three kernel files a few ms more:
// both on a thread, beside the argument checks and the camera order (host only), joined in front of the first device call
// (device_ready) -- round 5.
void Solver::device_thread_body(Setup& su) {
    SetupTrace wt;
    hipError_t e = hipSetDevice(device_);
    if (e == hipSuccess && !stream_) e = hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking);
    su.init_p.set_value(e);
    wt.mark("device thread: device, stream");
    if (e != hipSuccess) return;
    if (su.raw_uv_wanted && su.validated_f.get()) {   // the caller's measurements as they are, beside the host's list building -- once the lists are valid
        if (su.raw_uv.alloc(std::max<size_t>(2 * (size_t)n_obs_, 2)) != hipSuccess ||
            hipMemcpy(su.raw_uv, su.obs_uv, 2 * (size_t)n_obs_ * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            su.raw_uv.reset();
            (void)hipGetLastError();
        }
        wt.mark("device thread: measurements up");
    }
    hipStream_t ws = nullptr;
    if (hipStreamCreateWithFlags(&ws, hipStreamNonBlocking) != hipSuccess) return;
    warm_ba_kernels(ws); warm_schur_pairs(ws); warm_chol_kernels(ws); warm_pcg_kernels(ws);
    (void)hipStreamSynchronize(ws);
    (void)hipStreamDestroy(ws);
    wt.mark("device thread: code objects");
}

hipError_t Solver::device_ready(const Setup& su) {   // (any thread: the calling thread's device is set as well)
    const hipError_t e = su.init_f.get();
    return e != hipSuccess ? e : hipSetDevice(device_);
}

int Solver::validate_indices(Setup& su) {
    std::atomic<int64_t> bad(n_obs_);   // first observation that references a missing variable
    const uint32_t *cam_idx = su.cam_idx, *pt_idx = su.pt_idx;
    const uint64_t n_cam = (uint64_t)n_cam_, n_pt = (uint64_t)n_pt_;
    parallel_ranges(n_obs_, 1 << 18, [&bad, cam_idx, pt_idx, n_cam, n_pt](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i)
            if (cam_idx[i] >= n_cam || pt_idx[i] >= n_pt) {
                int64_t cur = bad.load();
                while (i < cur && !bad.compare_exchange_weak(cur, i)) {}
                return;
            }
    });
    if (bad.load() < n_obs_) return fail(kInvalidInput, "observation " + std::to_string(bad.load()) + " references a missing variable");
    return kOk;
}

// The tile plan and with it the variant this structure runs: the decision is made afresh for every structure (an automatic
// selection of an earlier set_structure on this handle does not stick), on whichever thread builds the plan.
void Solver::choose_and_build_plan(Setup& su) {
    const auto t_plan = std::chrono::steady_clock::now();
    (void)hipSetDevice(device_);
    matrix_free_only_ = matrix_free_only_opt_;
    auto_fallback_ = false; fallback_reason_.clear();
    std::vector<uint8_t>& present_plan = su.present_plan;
    if (matrix_free_only_) {   // S is never formed: keep the diagonal tiles (Schur-Jacobi blocks are read from them), nothing else
        std::fill(present_plan.begin(), present_plan.end(), (uint8_t)0);
        for (int I = 0; I < nt_; ++I) present_plan[(size_t)I * nt_ + I] = 1;
    }
    tp_.enable_graphs(use_graphs_);
    // Variant selection by predicted cost (round 6; the reference's dispatch never fails on the fill of S and a drop-in backend
    // should not spend 10 s where it owns a 0.5 s way to the same step: levenberg_marquardt.rs:1039-1082).  The matrix-free
    // PCG costs at most its cap times one S p -- two passes over the observations, 160 bytes each at the 4.5 TB/s the two
    // kernels sustain (1.01 ms on final-13682, 0.45 ms on synthetic-10k: DESIGN section 5) -- whatever the structure; the tile
    // plan refuses to be built when its own prediction (predict_solve_ms, plan_lists.h) is above that.  Both numbers are host
    // arithmetic on the replicated structure: every rank decides alike.  "variant_cost_permille" scales the matrix-free side
    // (tests move the crossover onto small problems; 0: the rule is off).
    pred_mf_ms_ = 500.0 * (160.0 * (double)n_obs_ / 4.5e12 * 1e3 + 0.02) * (double)variant_cost_permille_ / 1000.0;
    pred_direct_ms_ = 0.0; variant_choice_ = matrix_free_only_ ? 3 : 0;
    tp_.set_cost_limit_ms((auto_variant_ && !matrix_free_only_ && variant_cost_permille_ > 0) ? pred_mf_ms_ : 0.0);
    std::string e = tp_.build(nt_, present_plan, stream_);
    if (!matrix_free_only_) pred_direct_ms_ = tp_.predicted_ms();
    // A structure whose direct factorisation is out of reach (a photo collection: S dense at tile granularity) is not an
    // error of the caller's: the reference's LM never fails on the fill of S.  The handle becomes matrix-free only by itself
    // and answers every variant with the matrix-free PCG (set_auto_variant).  The update-list rule is pure host arithmetic
    // on the replicated structure (every rank decides alike); the memory rule depends on the device and is single-rank only.
    const bool refused_size = tp_.refused_too_large(), refused_mem = tp_.refused_no_memory() && ranks_.world() == 1, refused_cost = tp_.refused_by_cost();
    if (!e.empty() && auto_variant_ && !matrix_free_only_ && (refused_size || refused_mem || refused_cost)) {
        auto_fallback_ = true; matrix_free_only_ = true;
        variant_choice_ = refused_cost ? 1 : 2;
        fallback_reason_ = (refused_cost ? "matrix-free PCG (IterativeSchurSolver semantics) selected by predicted cost (" : "the direct factorisation of S was refused (") + e +
                           (refused_cost ? ")" : "): matrix-free PCG (IterativeSchurSolver semantics) selected");
        tp_.set_cost_limit_ms(0.0);
        std::fill(present_plan.begin(), present_plan.end(), (uint8_t)0);
        for (int I = 0; I < nt_; ++I) present_plan[(size_t)I * nt_ + I] = 1;
        e = tp_.build(nt_, present_plan, stream_);
    }
    su.plan_err = e;
    su.plan_seconds = seconds_since(t_plan);
}

void Solver::planner_body(Setup& su) {   // (nothing may escape a thread)
    try {
        if (device_ready(su) != hipSuccess) { su.plan_err = "the device could not be initialised"; return; }
        choose_and_build_plan(su);
    } catch (const std::exception& ex) { su.plan_err = std::string("tile plan: ") + ex.what(); }
}

int Solver::adopt_host_structure(Setup& su) {
    const BaHostStructure& hs = *su.hs;
    n_c_ = hs.n_c; nt_ = hs.nt; n_c_pad_ = hs.n_c_pad;
    cmap_ = hs.cmap; cinv_ = hs.cinv; lmap_ = hs.lmap;
    lm_lo_ = hs.lm_lo; lm_hi_ = hs.lm_hi; tree_shard_ = hs.tree_shard; pad_rank_ = hs.pad_rank;
    n_hubs_ = hs.n_hubs; n_border_tiles_ = hs.n_border_tiles;
    cam_scale_.set_size(n_c_, n_c_pad_);
    pt_scale_.set_size(3 * n_pt_, 3 * n_pt_);
    o_orig_h_.assign(hs.o_orig.begin(), hs.o_orig.end());
    n_pairs_ = hs.n_pairs; n_present_ = hs.n_present;
    lam_mask_.reset();
    if (tree_shard_) HIP_TRY(lam_mask_.upload(hs.lam_mask));
    return kOk;
}

// Uploads of everything that does not depend on the tile plan, on a thread of their own: the observation lists (1.7 GB on
// final-13682), the camera staging lists, the masks and the work arrays go to the device while the calling thread builds
// the tile plan and the pair list (round 5: 0.09 s of copies under 0.27 s of host work).
void Solver::uploader_body(Setup& su) {   // (nothing may escape a thread: an allocation failure becomes this call's status)
    try {
        const auto t0 = std::chrono::steady_clock::now();
        int rc = upload_observation_lists(su, &su.up_err);
        build_column_maps(su);   // (host only; on this thread because it has the slack: 3 n_pt columns)
        if (rc == kOk) rc = upload_fixed_masks(su, &su.up_err);
        if (rc == kOk) rc = alloc_work_arrays(&su.up_err);
        if (rc == kOk) su.up_seconds = seconds_since(t0);
        su.up_rc = rc;
    } catch (const std::exception& ex) { su.up_rc = kDeviceError; su.up_err = std::string("set_structure uploads: ") + ex.what(); }
}

int Solver::upload_observation_lists(Setup& su, std::string* err) {
    const BaHostStructure& hs = *su.hs;
    HIP_TRY(hipSetDevice(device_), err);   // (the first step on its thread)
    {
        const BaHostStructure::CamStaging st = hs.build_cam_staging();   // (host work hidden on this thread)
        HIP_TRY(o_slot_.upload(st.slot), err);
        HIP_TRY(wg_cam_n_.upload(st.wg_n), err);
        HIP_TRY(wg_cam_list_.upload(st.wg_list), err);
    }
    HIP_TRY(o_cam_.upload(hs.o_cam), err);
    HIP_TRY(o_pt_.upload(hs.o_pt), err);
    HIP_TRY(o_orig_.upload(o_orig_h_), err);
    HIP_TRY(pt_ptr_.upload(hs.pt_ptr), err);
    HIP_TRY(cam_ptr_.upload(hs.cam_ptr), err);
    HIP_TRY(cam_obs_.upload(hs.cam_obs), err);
    HIP_TRY(co_rank_.upload(hs.co_rank), err);
    if (!su.so.device_gathers) {
        HIP_TRY(o_uv_.upload(hs.o_uv), err);
        HIP_TRY(co_pt_.upload(hs.co_pt), err);
        HIP_TRY(co_uv_.upload(hs.co_uv), err);
        return kOk;
    }
    // the caller's measurements go up as they are (one contiguous copy, no host gather), the three lists that are
    // permutations of what is on the device already are made there
    const size_t n_loc = hs.o_cam.size();
    if (su.device_thread.joinable()) su.device_thread.join();   // (the measurements went up on the device thread, beside the list building)
    hipError_t ge = hipSuccess;
    if (!su.raw_uv) {
        HIP_TRY(su.raw_uv.alloc(std::max<size_t>(2 * (size_t)n_obs_, 2)), err);
        ge = hipMemcpy(su.raw_uv, su.obs_uv, 2 * (size_t)n_obs_ * sizeof(double), hipMemcpyHostToDevice);
    }
    // (plain allocations: every element is written by the gathers.  NOT alloc_zero -- its hipMemset runs on the
    // null stream, which stream_ (non-blocking) does not follow: the clear could land AFTER the gather had written the
    // array; seen once in 36 problems of the population test as a step of garbage)
    if (ge == hipSuccess) ge = o_uv_.alloc(2 * n_loc);
    if (ge == hipSuccess) ge = co_uv_.alloc(2 * n_loc);
    if (ge == hipSuccess) ge = co_pt_.alloc(n_loc);
    if (ge == hipSuccess) {
        launch_gather_uv((int64_t)n_loc, o_orig_, su.raw_uv, o_uv_, stream_);
        launch_gather_uv((int64_t)n_loc, cam_obs_, o_uv_, co_uv_, stream_);
        launch_gather_u32((int64_t)n_loc, cam_obs_, o_pt_, co_pt_, stream_);
        ge = hipStreamSynchronize(stream_);
    }
    su.raw_uv.reset();
    HIP_TRY(ge, err);
    return kOk;
}

// The caller's columns against the internal order (column_map.h): cmap_ and lmap_ are known, every export from here on goes
// through these two
void Solver::build_column_maps(const Setup& su) {
    cam_map_ = camera_column_map(std::vector<int64_t>(su.pose_col, su.pose_col + n_cam_), std::vector<int64_t>(su.intr_col, su.intr_col + n_cam_), cmap_, dc_);
    pt_map_ = block_column_map(std::vector<int64_t>(su.pt_col, su.pt_col + n_pt_), lmap_, 3);
}

int Solver::upload_fixed_masks(const Setup& su, std::string* err) {
    std::vector<uint8_t> fp(6 * n_cam_, 0), fi(3 * n_cam_, 0), fl(3 * n_pt_, 0);
    if (su.fix_pose) blocks_to_internal(cmap_, 6, su.fix_pose, fp.data());
    if (su.fix_intr) blocks_to_internal(cmap_, 3, su.fix_intr, fi.data());
    if (su.fix_pt) blocks_to_internal(lmap_, 3, su.fix_pt, fl.data());
    HIP_TRY(fix_pose_.upload(fp), err);
    HIP_TRY(fix_intr_.upload(fi), err);
    HIP_TRY(fix_pt_.upload(fl), err);
    return kOk;
}

int Solver::alloc_work_arrays(std::string* err) {
    for (int w = 0; w < 2; ++w) {
        HIP_TRY(poses_[w].alloc_zero(7 * n_cam_), err);
        HIP_TRY(intr_[w].alloc_zero(3 * n_cam_), err);
        HIP_TRY(pts_[w].alloc_zero(3 * n_pt_), err);
        HIP_TRY(camp_[w].alloc_zero((size_t)(kCamStride + kCamQStride) * n_cam_), err);   // [n_cam][16] records | [n_cam][10] compact form
    }
    HIP_TRY(g_c_.alloc_zero(n_c_pad_), err);
    HIP_TRY(g_red_.alloc_zero(n_c_pad_), err);
    HIP_TRY(dcam_.alloc_zero(n_c_pad_), err);
    HIP_TRY(hinv_.alloc_zero((size_t)kLmStride * n_pt_), err);  // landmark records: Hll^-1 | g_l | point
    // projection records of the local observations (xn, yn, p_w.z, sqrt(rho')): the record form of the pair kernel
    HIP_TRY(orec_.alloc_zero(4 * o_orig_h_.size()), err);
    HIP_TRY(g_l_.alloc_zero(3 * n_pt_), err);
    HIP_TRY(dl_.alloc_zero(3 * n_pt_), err);
    HIP_TRY(partial_.alloc_zero(3 * (size_t)n_partial_), err);
    HIP_TRY(scal_.alloc_zero(1), err);
    HIP_TRY(tile_work_.alloc_zero(6 * (size_t)n_c_pad_), err);   // tp_.pcg: "work: 6*n_pad doubles" (tile_plan.h), the largest of its users
    HIP_TRY(lmu_.alloc_zero((size_t)kLmuStride * n_pt_), err);
    HIP_TRY(mf_xs_.alloc_zero(n_c_pad_), err);
    HIP_TRY(sj_pcg_.setup(n_cam_, dc_, n_c_, n_c_pad_, stream_, partial_, n_partial_), err);
    HIP_TRY(flags_.alloc_zero(4), err);
    for (int b = 0; b < 2; ++b) {   // the pinned chunks of upload_staged: mapped here, not in the caller's first set_params
        if (!pin_[b]) HIP_TRY(pin_[b].alloc((size_t)16 << 20), err);
        if (!pin_ev_[b]) HIP_TRY(hipEventCreateWithFlags(&pin_ev_[b], hipEventDisableTiming), err);
    }
    return kOk;
}

// The task lists of the Schur reduction, after the uploader is joined (the device builds the records from its lists).
int Solver::upload_pair_lists(Setup& su, const PairDeviceTables& dtab, bool recs_on_device) {
    const auto t0 = std::chrono::steady_clock::now();
    const PairLists& pl = su.hs->pl;
    HIP_TRY(ptasks_.upload(pl.tasks));
    HIP_TRY(pchunks_.upload(pl.chunks));
    HIP_TRY(pblocks_.upload(pl.blocks));
    if (recs_on_device && pl.queued) {
        // the records of the queued layout are written by the device from the observation lists the uploader put there
        // (schur_pairs.h, PairDeviceTables): 17 MB of tables up instead of 1.56 GB of records built and copied
        DeviceBuffer<int> d_rows, d_run_ptr, d_run_piece0;   // (tables of this call only: freed on every way out of the block)
        DeviceBuffer<uint32_t> d_run_cj;
        DeviceBuffer<int2> d_piece, d_task;
        hipError_t e = precs_.alloc((size_t)dtab.n_slots);
        if (e == hipSuccess) e = d_rows.upload(dtab.rows);
        if (e == hipSuccess) e = d_run_ptr.upload(dtab.run_ptr);
        if (e == hipSuccess) e = d_run_cj.upload(dtab.run_cj);
        if (e == hipSuccess) e = d_run_piece0.upload(dtab.run_piece0);
        if (e == hipSuccess) e = d_piece.upload(dtab.piece);
        if (e == hipSuccess) e = d_task.upload(dtab.task);
        if (e == hipSuccess)
            e = launch_build_pair_recs_q(n_cam_, d_rows, d_run_ptr, d_run_cj, d_run_piece0, d_piece, d_task, cam_ptr_, cam_obs_, o_pt_, pt_ptr_, o_cam_,
                                         precs_, dtab.n_slots, stream_);
        HIP_TRY(e);
    } else {
        HIP_TRY(precs_.upload(pl.recs));
    }
    pqdesc_.reset();
    if (pl.queued) HIP_TRY(pqdesc_.upload(pl.qdesc));
    su.up_seconds += seconds_since(t0);
    return kOk;
}

// the host lists (3.7 GB on final-13682) are unmapped off the caller's path: 0.2 s
void Solver::hand_lists_to_free_thread(Setup& su) {
    if (free_thread_.joinable()) free_thread_.join();
    const char* fm = getenv("APEX_SETUP_FREE");   // experiment switch: "sync" frees on the caller's path, "leak" never
    if (fm && !strcmp(fm, "sync")) su.hs.reset();
    else if (fm && !strcmp(fm, "leak")) (void)su.hs.release();
    else free_thread_ = std::thread([p = su.hs.release()] { delete p; (void)HostBlockCache::get().end_setup(); });   // (what only an older, larger structure used goes back to the system)
}

int Solver::set_structure(const uint32_t* cam_idx, const uint32_t* pt_idx, const double* obs_uv,
                          const int64_t* intr_col, const int64_t* pose_col, const int64_t* pt_col,
                          const uint8_t* fix_pose, const uint8_t* fix_intr, const uint8_t* fix_pt,
                          double huber_delta) {
    if (n_cam_ <= 0 || n_pt_ <= 0) return fail(kInvalidInput, n_cam_ <= 0 ? "No camera variables found" : "No landmark variables found");
    if (n_obs_ < 0 || n_obs_ > 2000000000LL) return fail(kInvalidInput, "observation count out of range");
    lc_.release();   // (the landmark covariance lists belong to the old structure)
    pose_pri_ = PriorSet{}; intr_pri_ = PriorSet{};   // (and so do the priors: camera indices of the old problem)
    pri_diag_.reset(); pri_g_.reset(); pri_cost_.reset(); pri_res_.reset();
    Setup su;   // (its destructor releases and joins whatever thread is still out, on every return below)
    su.cam_idx = cam_idx; su.pt_idx = pt_idx; su.obs_uv = obs_uv;
    su.intr_col = intr_col; su.pose_col = pose_col; su.pt_col = pt_col;
    su.fix_pose = fix_pose; su.fix_intr = fix_intr; su.fix_pt = fix_pt;
    su.raw_uv_wanted = ranks_.world() == 1;
    su.device_thread = std::thread(&Solver::device_thread_body, this, std::ref(su));
    { const int rc = validate_indices(su); if (rc != kOk) return rc; }
    su.release_device_thread(true);
    huber_delta_ = huber_delta;
    loss_set_ = false;
    loss_ = PgLoss{};
    // (the caller's factor list is NOT kept: get_hessian_csc, the one reader, rebuilds it from the device's observation
    // lists on demand -- 0.1 s of set-up on final-13682 for an export the LM loop never calls)
    su.tr.mark("validate the index lists");

    // ---- everything derived from the observation list on the host (ba_structure.h): internal camera order (hub
    // cameras last, nested dissection of the tile graph), tile structure, landmark sharding, observation lists ------
    su.t_begin = std::chrono::steady_clock::now();
    HostBlockCache::get().begin_setup();
    BaStructOptions& so = su.so;
    so.dc = dc_; so.use_nd = use_nd_; so.nd_leaf = nd_leaf_; so.hubs_last = hubs_last_;
    so.rank = ranks_.rank(); so.world = ranks_.world(); so.dist_factor = dist_factor_; so.tree_sharding = tree_sharding_;
    so.dist_selftest = dist_selftest_; so.schur_form = rows_form_;
    so.device_gathers = ranks_.world() == 1;
    BaHostStructure& hs = *su.hs;
    // Camera order and tile structure first; then the tile plan (symbolic fill, task lists, 1.4 GB of device allocations: 0.06-
    // 0.1 s, mostly serial) is built on a thread of its own BESIDE the observation lists (0.1 s), which do not need it (round 5).
    // A distributed plan with tree sharding previews the partition inside the list phase (plan_owners): no overlap then.
    hs.build_order(n_cam_, n_pt_, n_obs_, cam_idx, pt_idx, so);
    tp_.set_partition(hs.part_rank, hs.part_world);
    tp_.set_own_all(hs.part_own_all);
    if (hs.part_own_all) {   // (self-test: one rank plays every owner, the exchanges are no-ops)
        tp_.set_comm([](const ExchangeList&, hipStream_t) { return true; });
    }
    nt_ = hs.nt;
    su.present_plan = hs.present;
    su.tr.mark("camera order, tile structure");
    const bool plan_beside_lists = !BaHostStructure::needs_owner_preview(so);
    if (plan_beside_lists) su.planner = std::thread(&Solver::planner_body, this, std::ref(su));
    {
        const std::string e = hs.build_obs_lists(cam_idx, pt_idx, obs_uv, so);
        if (!e.empty()) return fail(kInvalidInput, e);
    }
    su.tr.mark("observation lists");
    HIP_TRY(device_ready(su));
    su.tr.mark("waited for the device thread");
    { const int rc = adopt_host_structure(su); if (rc != kOk) return rc; }
    su.uploader = std::thread(&Solver::uploader_body, this, std::ref(su));

    // ---- the tile plan: built beside the lists above, or here (distributed plans with tree sharding) -------------
    if (plan_beside_lists) su.planner.join(); else choose_and_build_plan(su);
    if (matrix_free_only_) so.schur_form = -1;
    if (!su.plan_err.empty()) return fail(kInvalidInput, "reduced camera matrix: " + su.plan_err);
    hs.seconds[2] = su.plan_seconds;
    // ---- task lists of the selected form of the Schur reduction (they need the slot map) ------------------------------
    // (tried in round 5: the pair list built from a host-only twin's slot map BEFORE the planner thread is done -- the host pool
    // is shared, the three threads then slow one another down: set-up 0.26-0.28 s against 0.24)
    PairDeviceTables dtab;
    const bool recs_on_device = device_pair_recs_ && so.schur_form == 4 && dc_ == 9;
    hs.build_schur_lists(so, tp_.slot_host(), recs_on_device ? &dtab : nullptr);
    n_ptasks_ = (int)hs.pl.tasks.size();
    n_pair_blocks_ = hs.pl.n_blocks; pair_queued_ = hs.pl.queued;
    n_pair_slots_ = (recs_on_device && hs.pl.queued) ? dtab.n_slots : (int64_t)hs.pl.recs.size();
    su.uploader.join();
    if (su.up_rc != kOk) return fail(su.up_rc, su.up_err);
    hs.release_scratch();
    su.tr.mark("plan + Schur lists (observation lists uploading beside them)");
    { const int rc = upload_pair_lists(su, dtab, recs_on_device); if (rc != kOk) return rc; }

    HIP_TRY(hipDeviceSynchronize());  // the null-stream memsets of the work arrays precede any work on stream_
    hs.seconds[4] = su.up_seconds;   // (copy time; the first part of it ran beside the plan and the pair list)
    hs.seconds[5] = seconds_since(su.t_begin);
    for (int k = 0; k < 6; ++k) setup_s_[k] = hs.seconds[k];
    su.tr.mark("set_structure body");
    hand_lists_to_free_thread(su);
    su.tr.mark("host lists handed to the free thread");

    have_structure_ = true;
    have_params_ = false;
    voided_by(Change::kStructure);
    release_dogleg_buffers();
    st_.cur = 0;
    return kOk;
}

// What a change voids ("What a change voids"): the one place outside the solve path that touches the pending step,
// the Dog-Leg cache, the projection records, the factor's linearisation point and the factor's validity.
void Solver::voided_by(Change why) {
    switch (why) {
        case Change::kStructure:   // (the new plan holds no valid factor; set_params, which must follow, voids the rest)
            st_.invalidate();
            drop_dogleg_cache();
            break;
        case Change::kParams:      // the current set is overwritten: the factor's linearisation is no longer known
        case Change::kLoss:        // the factor was linearised, and the records written, under the old loss
            st_.invalidate();
            orec_fresh_ = false;
            drop_dogleg_cache();
            factor_lin_ = -1;
            break;
        case Change::kPriors:      // (the projection records do not see the priors: they stay)
            st_.invalidate();
            drop_dogleg_cache();
            tp_.set_factor_valid(false);   // the factor is of a system without these rows
            factor_lin_ = -1;
            break;
        case Change::kInformation:   // (pose graphs only)
            break;
        case Change::kScalingVectors:
            if (factor_scaled_) factor_lin_ = -1;   // the factor's scale vectors are overwritten
            [[fallthrough]];
        case Change::kScalingOff:    // the step is of the system under the old scaling; a trial point already written stays committable
            st_.invalidate_step();
            drop_dogleg_cache();
            break;
    }
}

int Solver::set_params(const double* poses, const double* intr, const double* points) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    HIP_TRY(hipSetDevice(device_));
    std::vector<double> hp(7 * n_cam_), hi(3 * n_cam_);
    blocks_to_internal(cmap_, 7, poses, hp.data());
    blocks_to_internal(cmap_, 3, intr, hi.data());
    HIP_TRY(hipMemcpyAsync(poses_[st_.cur], hp.data(), 7 * n_cam_ * sizeof(double), hipMemcpyHostToDevice, stream_));
    HIP_TRY(hipMemcpyAsync(intr_[st_.cur], hi.data(), 3 * n_cam_ * sizeof(double), hipMemcpyHostToDevice, stream_));
    std::vector<double> hpt;
    const double* src_pts = points;
    if (tree_shard_) {  // landmarks are renumbered so that every rank's set is one internal range
        hpt.resize(3 * n_pt_);
        blocks_to_internal(lmap_, 3, points, hpt.data());
        src_pts = hpt.data();
    }
    { const int rc = upload_staged(pts_[st_.cur], src_pts, 3 * (size_t)n_pt_ * sizeof(double)); if (rc != kOk) return rc; }
    launch_prepare_cams(n_cam_, poses_[st_.cur], intr_[st_.cur], camp_[st_.cur], mode_mask(mode_), stream_);
    HIP_TRY(hipStreamSynchronize(stream_));
    have_params_ = true;
    voided_by(Change::kParams);
    return kOk;
}

int Solver::set_loss(int kind, double p0, double p1) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    PgLoss l;
    if (!pg_loss_make(kind, p0, p1, &l)) return fail(kInvalidInput, "set_loss: unknown loss kind or a parameter its constructor refuses");
    if (!pg_loss_first_arm_only(l)) {
        const char* name = kind == kLossAndrews ? "Andrews" : kind == kLossLpNorm ? "LpNorm with p > 2" : "Barron with alpha > 2";
        return fail(kInvalidInput, std::string("set_loss: ") + name + " has rho'' > 0 for some residuals; the corrector's rank-one "
                    "Jacobian term does not fit the one weight per observation of the bundle-adjustment kernels");
    }
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipStreamSynchronize(stream_));
    loss_ = l;
    loss_set_ = true;
    voided_by(Change::kLoss);
    return kOk;
}

// what the observations carry: the loss of set_loss, else set_structure's Huber delta (or none)
void Solver::get_loss(int* kind, double out2[2]) const {
    out2[0] = out2[1] = 0.0;
    if (loss_set_) { *kind = loss_.kind; out2[0] = loss_.p0; out2[1] = loss_.p1; }
    else if (huber_delta_ > 0.0) { *kind = kLossHuber; out2[0] = huber_delta_; }
    else *kind = kLossNone;
}

// ---------------------------------------------------------------------------------------------
// PriorFactor blocks on the cameras
// ---------------------------------------------------------------------------------------------
int Solver::set_priors(bool intr, int64_t n, const uint32_t* cam, const double* data, const double* huber_delta, const double* weight) {
    const std::string what = intr ? "set_intrinsic_priors" : "set_pose_priors";
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    if (ranks_.world() > 1 || tp_.distributed()) return fail(kInvalidState, what + ": camera priors are single-rank only (this handle is sharded)");
    if (!prior_count_in_range(n)) return fail(kInvalidInput, what + ": prior count out of range");
    if (n > 0 && (!cam || !data)) return fail(kInvalidInput, what + ": cam / data are NULL");
    if (intr && n > 0 && dc_ != 9)
        return fail(kInvalidInput, "set_intrinsic_priors: this handle optimises six columns per camera; the intrinsics have no columns on the device");
    const PriorLayout lay = intr ? PriorLayout{3, kIntrPriorStride, true} : PriorLayout{7, kPosePriorStride, true};
    { const std::string why = ba_prior_refusal(what, n, cam, n_cam_, lay.amb, data, huber_delta, weight); if (!why.empty()) return fail(kInvalidInput, why); }
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipStreamSynchronize(stream_));
    // The new set goes up into a local and replaces the member only when every upload has succeeded (as PoseGraphSolver::set_priors)
    PriorSet ns;
    if (n > 0) {
        // sorted by internal camera (stable): one lane sums a camera's run in the caller's order; slot keeps the caller's index
        const PriorLists pl = build_prior_lists(n, cam, cmap_, lay, data, huber_delta, weight, true, n_cam_);
        HIP_TRY(ns.ptr.upload(pl.ptr));
        HIP_TRY(ns.slot.upload(pl.slot));
        HIP_TRY(ns.cam.upload(pl.owner));
        HIP_TRY(ns.data.upload(pl.data));
        ns.n = (int)n;
        if (!pri_diag_) {
            HIP_TRY(pri_diag_.alloc_zero(n_c_pad_));
            HIP_TRY(pri_g_.alloc_zero(n_c_pad_));
            HIP_TRY(pri_cost_.alloc_zero(n_cam_));
            HIP_TRY(hipDeviceSynchronize());   // (null-stream memsets ahead of the work on stream_)
        }
    }
    (intr ? intr_pri_ : pose_pri_) = std::move(ns);
    pri_res_.reset();   // (sized by the old counts)
    voided_by(Change::kPriors);
    return kOk;
}

BaPriorView Solver::prior_view() const {
    BaPriorView pv;
    pv.n_pose = pose_pri_.n; pv.pose_ptr = pose_pri_.ptr; pv.pose_data = pose_pri_.data; pv.pose_slot = pose_pri_.slot; pv.pose_cam = pose_pri_.cam;
    pv.n_intr = intr_pri_.n; pv.intr_ptr = intr_pri_.ptr; pv.intr_data = intr_pri_.data; pv.intr_slot = intr_pri_.slot; pv.intr_cam = intr_pri_.cam;
    return pv;
}

void Solver::enqueue_prior_eval(int which, bool cost_only) {
    launch_ba_prior_eval(dc_, n_cam_, camp_[which] + (size_t)kCamStride * n_cam_, prior_view(), cost_only ? nullptr : pri_diag_.get(),
                         cost_only ? nullptr : pri_g_.get(), pri_cost_, stream_);
}

void Solver::enqueue_prior_cost(int which, double* sumsq) {
    enqueue_prior_eval(which, true);
    launch_ba_prior_cost_add(n_cam_, pri_cost_, sumsq, stream_);
}

int Solver::get_prior_residual(double* pose_r7_out, double* intr_r3_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    if (!have_priors()) return kOk;
    HIP_TRY(hipSetDevice(device_));
    const size_t np = 7 * (size_t)pose_pri_.n, ni = 3 * (size_t)intr_pri_.n;
    if (!pri_res_) HIP_TRY(pri_res_.alloc(std::max<size_t>(np + ni, 1)));   // kept with the priors (set_priors frees it)
    launch_ba_prior_export(camp_[st_.cur] + (size_t)kCamStride * n_cam_, prior_view(), pri_res_, pri_res_ + np, stream_);
    HIP_TRY(hipGetLastError());
    if (pose_r7_out && np) HIP_TRY(hipMemcpyAsync(pose_r7_out, pri_res_, np * sizeof(double), hipMemcpyDeviceToHost, stream_));
    if (intr_r3_out && ni) HIP_TRY(hipMemcpyAsync(intr_r3_out, pri_res_ + np, ni * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    return kOk;
}

int Solver::get_params(double* poses, double* intr, double* points) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    if (ranks_.active()) {
        // every rank owns a contiguous landmark range: gather the owners' points everywhere
        // (ranges differ in size, so one broadcast per owner)
        // all ranks compute identical cuts from the replicated structure: re-derive from pt_ptr is not
        // possible without the full lists, so exchange the range starts.
        int64_t mine[2] = {lm_lo_, lm_hi_};
        int64_t* d_rng = ranks_.lm_ranges;
        HIP_TRY(hipMemcpyAsync(d_rng + 2 * ranks_.rank(), mine, sizeof mine, hipMemcpyHostToDevice, stream_));
        RANK_TRY(ranks_.all_gather(d_rng + 2 * ranks_.rank(), d_rng, 2 * sizeof(int64_t), stream_));
        std::vector<int64_t> rng(2 * ranks_.world());
        HIP_TRY(hipMemcpyAsync(rng.data(), d_rng, rng.size() * 8, hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
        for (int r = 0; r < ranks_.world(); ++r) {
            const int64_t a = rng[2 * r], b = rng[2 * r + 1];
            if (b > a) RANK_TRY(ranks_.broadcast(pts_[st_.cur] + 3 * a, 3 * (b - a), r, stream_));
        }
    }
    std::vector<double> hp(7 * n_cam_), hi(3 * n_cam_);
    HIP_TRY(hipMemcpyAsync(hp.data(), poses_[st_.cur], 7 * n_cam_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipMemcpyAsync(hi.data(), intr_[st_.cur], 3 * n_cam_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    std::vector<double> hpt(tree_shard_ ? 3 * n_pt_ : 0);
    HIP_TRY(hipMemcpyAsync(tree_shard_ ? hpt.data() : points, pts_[st_.cur], 3 * n_pt_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    if (tree_shard_) blocks_to_caller(lmap_, 3, hpt.data(), points);
    blocks_to_caller(cmap_, 7, hp.data(), poses);
    blocks_to_caller(cmap_, 3, hi.data(), intr);
    return kOk;
}

// ---------------------------------------------------------------------------------------------
// cost (A16)
// ---------------------------------------------------------------------------------------------
int Solver::cost(double* out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    stage_begin(kStCost);
    double* sumsq = &scal_.get()->cost_sumsq;
    launch_cost(view(st_.cur), partial_, n_partial_, sumsq, stream_, general_loss());
    RANK_TRY(ranks_.sum(sumsq, 1, stream_));
    if (have_priors()) enqueue_prior_cost(st_.cur, sumsq);
    stage_end(kStCost);
    HIP_TRY(hipGetLastError());
    double ss = 0.0;
    HIP_TRY(hipMemcpyAsync(&ss, sumsq, sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    *out = cost_from_sumsq(ss);
    return kOk;
}

// ---------------------------------------------------------------------------------------------
// assembly of S, g_red, Hll^-1, g (A6-A11) at the current parameters
// ---------------------------------------------------------------------------------------------
int Solver::assemble(double lambda, double diag_extra, bool for_factor) {
    if (matrix_free_only_) return fail(kInvalidState, "this handle was built matrix-free only (\"matrix_free_only\"): the explicit S does not exist");
    int rc = assemble_local(lambda, diag_extra, for_factor);
    if (rc != kOk) return rc;
    if (ranks_.active()) {
        stage_begin(kStAllReduce);
        RANK_TRY(ranks_.issue(exchange(0, for_factor), stream_));
        stage_end(kStAllReduce);
    }
    return assemble_finish();
}

ExchangeList Solver::exchange(int point, bool for_factor) const {
    if (point != 0) return tp_.exchange(point);
    const size_t te = (size_t)kNB * kNB;
    ExchangeList l;
    if (for_factor && tp_.distributed()) {
        // A distributed factorisation sums the shared top tiles itself, after the local levels, and a rank's local
        // levels read its own columns only: every column's tiles are reduced to their owner (tile_plan.h).
        // (tree sharding: a rank's landmarks are exactly those that touch its columns -- its tiles are complete)
        for (int o = 0; o < tp_.part_world() && !tree_shard_; ++o) {
            const std::pair<int64_t, int64_t> rg = tp_.owner_slot_range(o);
            l.push_back({ExchangeItem::kSum, tp_.tiles() + (size_t)rg.first * te, (size_t)rg.second * te, o});
        }
    } else l.push_back({ExchangeItem::kSum, tp_.tiles(), (size_t)tp_.n_touched_slots() * te, -1});
    l.push_back({ExchangeItem::kSum, g_red_.get(), (size_t)n_c_pad_, -1});
    l.push_back({ExchangeItem::kSum, g_c_.get(), (size_t)n_c_pad_, -1});
    l.push_back({ExchangeItem::kMaxInt, flags_.get(), 1, -1});  // a singular landmark block anywhere fails the solve on every rank
    return l;
}

// this rank's part of S, g_red, g_c (its landmarks), before any exchange
int Solver::assemble_local(double lambda, double diag_extra, bool for_factor) {
    drop_dogleg_cache();   // (g_c_ / g_l_ are overwritten)
    const BAView v = view(st_.cur);
    const TileMap tm = tilemap();
    stage_begin(kStAssembleCam);
    // (a tree-sharded rank that assembles for its distributed factorisation adds to its own and the top tiles only; every
    // other use of S -- PCG, exports, the ladder's diagonal -- all-reduces every touched tile and needs them all cleared)
    HIP_TRY(tp_.zero_tiles(tree_shard_ && for_factor, for_factor && ranks_.world() == 1));   // (the fill tiles stay as they are: tile_plan.h, first_ok_)
    launch_clear3(g_red_, g_c_, n_c_pad_, flags_, 4, stream_);   // (one launch instead of three fills)
    // identity on the padding rows of the last tile (rank 0 only: the all-reduce sums the ranks)
    // (tree sharding: by the owner of the last tile column, whose tiles are never summed -- pad_rank_)
    tp_.add_diag((int)n_c_, 0.0, ranks_.rank() == pad_rank_ ? 1.0 : 0.0);
    stage_end(kStAssembleCam);
    stage_begin(kStAssembleLm);
    launch_landmark_reduce(dc_, v, lambda, hinv_, g_l_, flags_, nullptr, stream_, orec_, general_loss());   // (the pair kernel and the back-substitution read the projection records)
    orec_fresh_ = true;
    stage_end(kStAssembleLm);
    stage_begin(kStAssembleCam);
    launch_cam_reduce(dc_, v, tm, cam_ptr_, cam_obs_, lambda + diag_extra, ranks_.rank() == 0 ? 1 : 0, hinv_, g_l_, 1,
                      g_c_, g_red_, stream_, general_loss());
    if (have_priors()) {   // the prior rows of the Jacobian: block-diagonal in H_cc, so S and g_red take them as they are (before any rescaling)
        enqueue_prior_eval(st_.cur, false);
        launch_ba_prior_add_system(n_c_, pri_diag_, pri_g_, tm, g_c_, g_red_, stream_);
    }
    stage_end(kStAssembleCam);
    stage_begin(kStScatter);
    launch_schur_pairs(dc_, v, tp_.tiles(), ptasks_, n_ptasks_, pchunks_, pblocks_, precs_, hinv_, stream_, orec_, pqdesc_);
    stage_end(kStScatter);
    return check_hip(hipGetLastError(), "assembly kernels");
}

// after the exchange: the reduced system in the scaled variables when Jacobi scaling is on (linear, so it also
// commutes with the later sum of the top tiles of a distributed factorisation)
int Solver::assemble_finish() {
    if (scaled_) {  // the reduced system in the scaled variables: S := D_c S D_c, g_red := D_c g_red
        stage_begin(kStAssembleCam);
        tp_.scale_sym(cam_scale_.dev);
        launch_vec_mul(n_c_pad_, g_red_, cam_scale_.dev, g_red_, stream_);
        stage_end(kStAssembleCam);
    }
    return kOk;
}

int Solver::factor_now(int* failed_at, bool defer_flags) {
    stage_begin(kStFactor);
    const hipError_t fe = tp_.factor(failed_at, defer_flags);
    if (fe == hipErrorUnknown && ranks_.active()) return fail(kDeviceError, ranks_.error());   // (a collective of the plan's: tile_plan.h)
    HIP_TRY(fe);
    stage_end(kStFactor);
    return kOk;
}

int Solver::enqueue_sweeps() {
    stage_begin(kStTriSolve);
    const hipError_t se = tp_.solve(g_red_, dcam_, tile_work_);
    if (se == hipErrorUnknown && ranks_.active()) return fail(kDeviceError, ranks_.error());
    HIP_TRY(se);
    stage_end(kStTriSolve);
    return kOk;
}

// solve_with_cholesky (explicit_schur.rs:539-634) incl. the regularisation ladder, up to the factor (direct_solve runs the sweeps)
int Solver::factor_with_ladder(double lambda) {
    int failed = 0;
    last_reg_ = 0.0;
    const int rc = factor_fresh(lambda, 0.0, &failed);
    return (rc != kOk || !failed) ? rc : ladder(lambda);
}

// A speculative factorisation went wrong: what was enqueued behind it is void.  A failed pivot takes the waited-for path from
// the top (S again, the factorisation, the ladder); after a give-up the repaired factorisation stands in for that path's first.
int Solver::recover_factor(double lambda, int failed, bool gave_up) {
    if (dl_mode_) {   // Dog-Leg: no ladder -- a regularised h would not solve the system whose products are priced; the loop raises mu
        if (gave_up) { const int rc = factor_again(lambda, 0.0, &failed); if (rc != kOk) return rc; }
        return failed ? fail(kFactorizationFailed, "non-positive pivot in tile column " + std::to_string(failed - 1) + " of S") : kOk;
    }
    if (!gave_up) {
        const int rc = assemble(lambda, 0.0, true);
        return rc != kOk ? rc : factor_with_ladder(lambda);
    }
    const int rc = factor_again(lambda, 0.0, &failed);
    return (rc != kOk || !failed) ? rc : ladder(lambda);
}

int Solver::ladder(double lambda) {
    // the factorisation overwrote S: re-assemble it to read trace and max |diag| (:563-579)
    int failed = 0;
    int rc = assemble(lambda, 0.0);
    if (rc != kOk) return rc;
    double* diag = tile_work_;
    tp_.diag(diag);
    std::vector<double> hd(n_c_);
    HIP_TRY(hipMemcpyAsync(hd.data(), diag, n_c_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    // the reference's S also holds the 3 n_cam intrinsic rows when the factors do not touch them
    // (BundleAdjustment mode): their diagonal is lambda.
    double trace = 0.0, max_diag = 0.0;
    for (double d : hd) { trace += d; max_diag = std::max(max_diag, fabs(d)); }
    int64_t n_ref = n_c_;
    if (dc_ == 6) { trace += 3.0 * n_cam_ * lambda; max_diag = std::max(max_diag, fabs(lambda)); n_ref = 9 * n_cam_; }
    const double base = std::max(std::max(trace / (double)n_ref, max_diag), 1.0);
    for (int attempt = 0; attempt < 5; ++attempt) {
        const double reg = base * pow(10.0, (double)(attempt - 4));
        rc = assemble(lambda, reg, true);
        if (rc != kOk) return rc;
        rc = factor_fresh(lambda, reg, &failed);
        if (rc != kOk) return rc;
        if (!failed) { last_reg_ = reg; return kOk; }
    }
    return fail(kSingularMatrix, "Schur complement singular after 5 regularization attempts (max reg = " + std::to_string(base) + ")");
}

// solve_with_pcg (explicit_schur.rs:639-756): Jacobi-preconditioned CG on the explicit S.
int Solver::pcg_solve() {
    stage_begin(kStFactor);
    HIP_TRY(tp_.pcg(g_red_, dcam_, tile_work_, cg_max_iter_, cg_tol_, &last_pcg_iters_));
    stage_end(kStFactor);
    return kOk;
}

// ---------------------------------------------------------------------------------------------
// A18: IterativeSchurSolver (src/linalg/sparse/implicit_schur.rs) -- S is never formed.
//   assemble_implicit : Hll^-1 / g_l (k_landmark_reduce), g_c and g_red plus the DIAGONAL blocks of S
//                       (k_cam_reduce with its self terms), Schur-Jacobi blocks inverted per variable
//   implicit_pcg_solve: solve_pcg_block (:577-679), the loop SchurJacobiPcg's (schur_jacobi_pcg.h); every S p (implicit_matvec) is two
//                       passes over the observations (landmark-major, then camera-major), nothing but 64 bytes per landmark in between
// Sharded: g_red, g_c and the diagonal blocks are all-reduced once, every S p once per iteration.
// ---------------------------------------------------------------------------------------------
int Solver::assemble_implicit(double lambda) {
    drop_dogleg_cache();   // (g_c_ / g_l_ are overwritten)
    tp_.set_factor_valid(false);   // (the camera reduction adds to the diagonal tiles)
    const BAView v = view(st_.cur);
    stage_begin(kStAssembleLm);
    HIP_TRY(hipMemsetAsync(flags_, 0, 4 * sizeof(int), stream_));
    launch_landmark_reduce(dc_, v, lambda, hinv_, g_l_, flags_, lmu_, stream_, orec_, general_loss());
    orec_fresh_ = orec_ != nullptr;
    stage_end(kStAssembleLm);
    stage_begin(kStAssembleCam);
    launch_cam_reduce(dc_, v, tilemap(), cam_ptr_, cam_obs_, lambda, ranks_.rank() == 0 ? 1 : 0, hinv_, g_l_, 1, g_c_, g_red_, stream_, general_loss());
    launch_extract_diag_blocks(dc_, n_cam_, tilemap(), sj_pcg_.diag_blocks(), stream_);
    if (have_priors()) {   // (single rank: nothing below sums these twice)
        enqueue_prior_eval(st_.cur, false);
        launch_ba_prior_add_blocks(dc_, n_cam_, pri_diag_, pri_g_, sj_pcg_.diag_blocks(), g_c_, g_red_, stream_);
    }
    stage_end(kStAssembleCam);
    if (ranks_.active()) {
        stage_begin(kStAllReduce);
        RANK_TRY(ranks_.issue({{ExchangeItem::kSum, sj_pcg_.diag_blocks(), (size_t)n_cam_ * dc_ * dc_, -1},
                               {ExchangeItem::kSum, g_red_.get(), (size_t)n_c_pad_, -1},
                               {ExchangeItem::kSum, g_c_.get(), (size_t)n_c_pad_, -1},
                               {ExchangeItem::kMaxInt, flags_.get(), 1, -1}},   // a singular landmark block anywhere fails the solve on every rank
                              stream_));
        stage_end(kStAllReduce);
    }
    stage_begin(kStAssembleCam);
    if (scaled_) launch_vec_mul(n_c_pad_, g_red_, cam_scale_.dev, g_red_, stream_);
    sj_pcg_.build_preconditioner(scaled_ ? cam_scale_.dev.get() : nullptr);
    stage_end(kStAssembleCam);
    return kOk;
}

// y = S x of the matrix-free operator (in the scaled variables when a scaling is set: D_c S0 D_c x, where S0 carries
// lambda / s^2 on its diagonal).  lam_local: lambda on rank 0, 0 elsewhere (the all-reduce sums the ranks' partial products).
int Solver::implicit_matvec(const double* x, double lam_local, double* y, bool reduce) {
    const double* xin = x;
    if (scaled_) {
        launch_vec_mul(n_c_, x, cam_scale_.dev, mf_xs_, stream_);
        xin = mf_xs_;
    }
    launch_implicit_matvec(dc_, view(st_.cur), cam_ptr_, hinv_, lmu_, xin, lam_local, y, stream_, backsub_records(), general_loss());
    if (have_priors()) launch_ba_prior_matvec(n_c_, pri_diag_, xin, y, stream_);   // (diag(P) of assemble_implicit's evaluation, in the unscaled variables)
    if (reduce) RANK_TRY(ranks_.sum(y, (size_t)n_c_, stream_));
    if (scaled_) launch_vec_mul(n_c_, y, cam_scale_.dev, y, stream_);
    return check_hip(hipGetLastError(), "implicit_matvec");
}

int Solver::implicit_pcg_solve(double lambda, int max_iter, double tol) {
    stage_begin(kStFactor);
    const double lam_local = (ranks_.rank() == 0) ? lambda : 0.0;  // the all-reduce sums the ranks' partial S p
    // (a failed collective of the matvec ends the loop with its status, its text in err_)
    const int rc = sj_pcg_.solve(g_red_, dcam_, max_iter, tol, [&](const double* p, double* ap) { return implicit_matvec(p, lam_local, ap, true); },
                                 &last_pcg_iters_, &err_);
    if (rc != kOk) return rc;
    stage_end(kStFactor);
    return kOk;
}

int Solver::solve_augmented(double lambda, int variant, double* step_out, double* grad_out) {
    if (!have_params_) return fail(kInvalidState, "Block structure not built or parameters not set");
    HIP_TRY(hipSetDevice(device_));
    begin_solve(lambda);
    drop_dogleg_cache();
    last_pcg_iters_ = 0;   // (the PCG variants set it: apexgpu_info[5] is about THIS solve)
    tp_.set_factor_valid(false);   // (every variant writes the tiles or leaves them stale for this point)
    int pcg_max = cg_max_iter_;
    double pcg_tol = cg_tol_;
    if (auto_fallback_ && variant != 2) {   // set_structure selected the matrix-free variant for this handle (set_auto_variant)
        if (variant == 0) { pcg_max = 500; pcg_tol = 1e-9; }   // IterativeSchurSolver::new (implicit_schur.rs:94-95)
        variant = 2;
    }
    int rc = (variant == 2) ? assemble_implicit(lambda) : assemble(lambda, 0.0, variant == 0);
    if (rc != kOk) return rc;
    // ONE host wait per Cholesky solve (TileBackend::direct_solve) on a single rank.  Otherwise the host waits three times inside
    // this call -- for the landmark-inversion flag behind the assembly, for the pivot flag behind the factorisation, for the step
    // at the end -- and the GPU idles through a synchronisation plus a graph launch each time.
    const bool speculative = one_wait_ && variant == 0 && !ranks_.active() && !tp_.distributed();
    if (speculative) {
        last_reg_ = 0.0;
    } else {
        int lm_err = 0;
        HIP_TRY(hipMemcpyAsync(&lm_err, flags_, sizeof(int), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
        if (lm_err) return own_flag_raised();
        rc = (variant == 2) ? implicit_pcg_solve(lambda, pcg_max, pcg_tol) : (variant == 1) ? pcg_solve() : factor_with_ladder(lambda);
        if (rc != kOk) return rc;
    }
    // (the PCG variants have the camera step in dcam_: no sweeps, no sweep time-out to look for, no factor to keep)
    return variant == 0 ? direct_solve(speculative, lambda, step_out, grad_out) : finish_step(step_out, grad_out);
}

// the camera step is in dcam_: scaling back, back-substitution, the eager evaluation, the export and its wait
int Solver::finish_step(double* step_out, double* grad_out) {
    stage_begin(kStBackSub);
    if (scaled_) launch_vec_mul(n_c_, dcam_, cam_scale_.dev, dcam_, stream_);  // apply_inverse_scaling: dc = D_c y
    // what the LM loop asks next (step statistics, trial cost) rides on this solve's wait (tile_backend.h, eager_eval_; single
    // rank); the trial POINTS are written by the back-substitution itself
    // (a Dog-Leg solve evaluates the BLENDED step behind its tail, not the Gauss-Newton step these sweeps left)
    const bool eager = eager_eval_ && !ranks_.active() && !dl_mode_;
    trial_pts_written_ = eager && fix_pt_ != nullptr;
    launch_back_substitute(dc_, view(st_.cur), hinv_, g_l_, dcam_, dl_, stream_, backsub_records(), trial_pts_written_ ? fix_pt_ : nullptr,
                           trial_pts_written_ ? pts_[st_.cur ^ 1] : nullptr, general_loss());
    stage_end(kStBackSub);
    HIP_TRY(hipGetLastError());
    st_.step_computed();
    if (dl_mode_) {
        const int rc = enqueue_dogleg_tail(true);
        if (rc != kOk) return rc;
        HIP_TRY(hipStreamSynchronize(stream_));
        return kOk;
    }
    if (eager) { const int rc = enqueue_eager_eval(); if (rc != kOk) return rc; }
    const int rc = export_step(step_out, grad_out);   // (synchronises)
    if (rc == kOk && eager) post_eager_answers();
    return rc;
}

// camera_covariance() may invert this factor -- single rank only
void Solver::keep_factor() {
    if (ranks_.world() != 1 || tp_.distributed()) return;
    tp_.set_factor_valid(true);
    factor_lin_ = st_.cur;   // (commit_step flips st_.cur: the factorised cameras are then in the other set)
    factor_scaled_ = scaled_;
}

// the last step / gradient in the reference's global column order (syncs)
int Solver::export_step(double* step_out, double* grad_out) {
    if (step_out) { const int rc = export_columns({{dcam_, &cam_map_, &cam_scale_}, {dl_, &pt_map_, &pt_scale_}}, ExportAs::kStep, step_out); if (rc != kOk) return rc; }
    if (grad_out) { const int rc = export_columns({{g_c_, &cam_map_, &cam_scale_}, {g_l_, &pt_map_, &pt_scale_}}, ExportAs::kGradient, grad_out); if (rc != kOk) return rc; }
    if (!step_out && !grad_out) HIP_TRY(hipStreamSynchronize(stream_));
    return kOk;
}

// ---------------------------------------------------------------------------------------------
// The distributed Cholesky solve cut into its phases, so that a test can drive the `world` instances of a
// sharded problem in lockstep inside ONE process and play the communicator itself (capi: apexgpu_debug_lockstep_solve).
// The production path (solve_augmented with a communicator) runs these pieces and issues, in between, the very lists the
// test plays: exchange(p, true) follows phase p, and it is what assemble(), TilePlan::factor and TilePlan::solve issue.
//   0: each rank's column tiles (reduce to the owner), g_red, g_c, the landmark flag (max)   1: the top tile ranges
//   2: the two failure words of the factorisation (max)   3, 4: TilePlan's exchange vector
// ---------------------------------------------------------------------------------------------
int Solver::dist_phase(int phase, double lambda) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    if (!tp_.distributed()) return fail(kInvalidState, "the plan is not distributed (set_shard with world > 1, dist_factor on)");
    if (matrix_free_only_) return fail(kInvalidState, "this handle was built matrix-free only (\"matrix_free_only\"): the explicit S does not exist");
    HIP_TRY(hipSetDevice(device_));
    switch (phase) {
        case 0: st_.invalidate_step(); last_lambda_ = lambda; return assemble_local(lambda, 0.0, true);
        case 1: {
            int rc = assemble_finish();
            if (rc != kOk) return rc;
            stage_begin(kStFactor);
            tp_.factor_phase(0);
            stage_end(kStFactor);
            return kOk;
        }
        case 2:
            stage_begin(kStAllReduce);   // lockstep runs only: the replicated top levels are booked under this stage's
            tp_.factor_phase(1);         // name so that they can be told apart from the local levels
            stage_end(kStAllReduce);
            return kOk;
        case 3: {
            int f[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(&f[0], tp_.flag_dev(), sizeof(int), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(hipMemcpyAsync(&f[1], flags_, sizeof(int), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(hipStreamSynchronize(stream_));
            if (f[1]) return fail(kSingularMatrix, "Landmark block is singular");
            if (f[0]) return fail(kFactorizationFailed, "non-positive pivot in tile column " + std::to_string(f[0] - 1));
            stage_begin(kStTriSolve);
            tp_.solve_phase(0, g_red_, dcam_, tile_work_);
            stage_end(kStTriSolve);
            return kOk;
        }
        case 4:
            stage_begin(kStTriSolve);
            tp_.solve_phase(1, g_red_, dcam_, tile_work_);
            stage_end(kStTriSolve);
            return kOk;
        case 5:
            tp_.solve_phase(2, g_red_, dcam_, tile_work_);
            if (scaled_) launch_vec_mul(n_c_, dcam_, cam_scale_.dev, dcam_, stream_);
            launch_back_substitute(dc_, view(st_.cur), hinv_, g_l_, dcam_, dl_, stream_, backsub_records(), nullptr, nullptr, general_loss());
            HIP_TRY(hipStreamSynchronize(stream_));
            st_.step_computed();
            return kOk;
        default: return fail(kInvalidInput, "phase out of range");
    }
}

int Solver::assemble_only(double lambda) {
    if (!have_params_) return fail(kInvalidState, "Block structure not built or parameters not set");
    HIP_TRY(hipSetDevice(device_));
    st_.invalidate_step();
    drop_dogleg_cache();
    last_lambda_ = lambda;
    int rc = assemble(lambda, 0.0);
    if (rc != kOk) return rc;
    int lm_err = 0;
    HIP_TRY(hipMemcpyAsync(&lm_err, flags_, sizeof(int), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    if (lm_err) return fail(kSingularMatrix, "Landmark block is singular");
    return kOk;
}

int Solver::enqueue_step_stats() {
    stage_begin(kStStats);
    double* step = scal_.get()->step;   // [0..2] the camera half, [3..5] the landmark half
    launch_step_stats(n_c_, g_c_, dcam_, last_lambda_, scaled_ ? cam_scale_.dev.get() : nullptr, partial_, n_partial_, step, stream_);
    launch_step_stats(3 * n_pt_, g_l_, dl_, last_lambda_, scaled_ ? pt_scale_.dev.get() : nullptr, partial_, n_partial_, &step[3], stream_);
    RANK_TRY(ranks_.sum(&step[3], 3, stream_));   // landmark part is sharded, camera part replicated
    stage_end(kStStats);
    return kOk;
}
// set `to` = set `from` (+) sign * step over the cameras and n_pt of the points, and the prepared cameras of the result
void Solver::retract_sets(int from, double sign, int to, int64_t n_pt) {
    stage_begin(kStRetract);
    launch_retract(dc_, n_cam_, n_pt, poses_[from], intr_[from], pts_[from], dcam_, dl_, sign, fix_pose_, fix_intr_, fix_pt_,
                   poses_[to], intr_[to], pts_[to], stream_);
    launch_prepare_cams(n_cam_, poses_[to], intr_[to], camp_[to], mode_mask(mode_), stream_);
    stage_end(kStRetract);
}
// the trial point x (+) step in the other parameter set and the sum of squared corrected residuals there (device scalar)
int Solver::enqueue_trial_point(double* sumsq_out) {
    const int t = st_.cur ^ 1;
    retract_sets(st_.cur, 1.0, t, trial_pts_written_ ? 0 : n_pt_);   // (the points: by k_back_substitute when trial_pts_written_)
    trial_pts_written_ = false;
    stage_begin(kStCost);
    launch_cost(view(t), partial_, n_partial_, sumsq_out, stream_, general_loss());
    RANK_TRY(ranks_.sum(sumsq_out, 1, stream_));
    if (have_priors()) enqueue_prior_cost(t, sumsq_out);
    stage_end(kStCost);
    return kOk;
}

int Solver::parameter_norm(double* out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    double* sumsq = scal_.get()->param_sumsq;
    launch_sumsq(7 * n_cam_, poses_[st_.cur], partial_, n_partial_, &sumsq[0], stream_);
    launch_sumsq(3 * n_cam_, intr_[st_.cur], partial_, n_partial_, &sumsq[1], stream_);
    // points: in a sharded run only the owned range is current on this rank
    launch_sumsq(3 * (lm_hi_ - lm_lo_), pts_[st_.cur] + 3 * lm_lo_, partial_, n_partial_, &sumsq[2], stream_);
    RANK_TRY(ranks_.sum(&sumsq[2], 1, stream_));
    double h[3];
    HIP_TRY(hipMemcpyAsync(h, sumsq, sizeof h, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    *out = sqrt(h[0] + h[1] + h[2]);
    return kOk;
}

// ---------------------------------------------------------------------------------------------
// Jacobi column scaling (process_jacobian_generic, optimizer/mod.rs:749-763)
// ---------------------------------------------------------------------------------------------
// squared column norms of the corrected Jacobian at the current parameters, left in the two holders' device vectors
int Solver::column_norms_sq_device() {
    HIP_TRY(cam_scale_.ensure());
    HIP_TRY(pt_scale_.ensure());
    const bool was = scaled_;
    scaled_ = false;
    const BAView v = view(st_.cur);
    scaled_ = was;
    HIP_TRY(hipMemsetAsync(cam_scale_.dev, 0, n_c_pad_ * sizeof(double), stream_));
    HIP_TRY(hipMemsetAsync(pt_scale_.dev, 0, std::max<int64_t>(3 * n_pt_, 1) * sizeof(double), stream_));
    launch_column_norms_sq(dc_, v, cam_scale_.dev, pt_scale_.dev, stream_, general_loss());
    if (have_priors()) {   // a prior row has one entry per column: its square is diag(P)
        enqueue_prior_eval(st_.cur, false);
        launch_vec_add(n_c_, cam_scale_.dev, pri_diag_, cam_scale_.dev, stream_);
    }
    RANK_TRY(ranks_.sum(cam_scale_.dev, (size_t)n_c_, stream_));   // every rank sees all cameras but only its own landmarks
    return kOk;
}

int Solver::column_norms(double* norms_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    drop_dogleg_cache();
    int rc = column_norms_sq_device();
    if (rc != kOk) return rc;
    std::vector<double> hc(n_c_), hl(3 * n_pt_);
    HIP_TRY(hipMemcpyAsync(hc.data(), cam_scale_.dev, n_c_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipMemcpyAsync(hl.data(), pt_scale_.dev, 3 * n_pt_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    const auto root = [](double n2, int64_t) { return sqrt(n2); };
    cam_map_.scatter(hc.data(), norms_out, 0.0, root);
    pt_map_.scatter(hl.data(), norms_out, 0.0, root);
    if (scaled_) {  // the device vectors held the active scaling: put it back
        HIP_TRY(cam_scale_.reupload(stream_));
        HIP_TRY(pt_scale_.reupload(stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
    }
    return kOk;
}

int Solver::set_column_scaling(const double* scaling) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built");
    HIP_TRY(hipSetDevice(device_));
    if (!scaling) { scaled_ = false; voided_by(Change::kScalingOff); return kOk; }
    voided_by(Change::kScalingVectors);   // (ahead of the checks: a refused vector has voided the step all the same)
    HIP_TRY(cam_scale_.ensure());
    HIP_TRY(pt_scale_.ensure());
    std::vector<double> hc, hl;
    if (!cam_scale_.accepts(cam_map_, scaling, &hc) || !pt_scale_.accepts(pt_map_, scaling, &hl)) return fail(kInvalidInput, JacobiScaling::kRefused);
    HIP_TRY(cam_scale_.set_from_caller(std::move(hc), stream_));
    HIP_TRY(pt_scale_.set_from_caller(std::move(hl), stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    scaled_ = true;
    return kOk;
}

// iteration 0 of the reference's loop: norms of the current Jacobian -> s = 1 / (1 + norm), kept for the whole optimize
int Solver::set_jacobi_scaling(bool on) {
    if (!on) { scaled_ = false; voided_by(Change::kScalingOff); return kOk; }
    if (!have_params_) return fail(kInvalidState, "no parameters set");   // (no parameters: no step and no Dog-Leg cache to void)
    HIP_TRY(hipSetDevice(device_));
    voided_by(Change::kScalingVectors);   // (ahead of the norms, which overwrite the vectors)
    int rc = column_norms_sq_device();
    if (rc != kOk) return rc;
    HIP_TRY(cam_scale_.from_norms_sq(cam_scale_.dev, n_c_pad_, stream_));  // padding: n2 = 0 -> 1
    HIP_TRY(pt_scale_.from_norms_sq(pt_scale_.dev, 3 * n_pt_, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    scaled_ = true;
    return kOk;
}

// ---------------------------------------------------------------------------------------------
// The LM loop (optimize_with_mode, levenberg_marquardt.rs:823-1031) with the state on the device.
// ---------------------------------------------------------------------------------------------
int Solver::lm_optimize(LmConfig* cfg, LmResult* res, LmIterRecord* hist, int hist_cap) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    return run_lm(*this, cfg, res, hist, hist_cap);
}

// ---------------------------------------------------------------------------------------------
// Dog-Leg (tr_loop.h): what this solver puts into TileBackend::dogleg_step.  d is the unscaled step the
// back-substitution left; the Gram kernel is handed D^2 g and d and never sees D (tile_backend.hip).
// ---------------------------------------------------------------------------------------------
int Solver::dogleg_refusal() {
    if (!have_params_) return fail(kInvalidState, "Block structure not built or parameters not set");
    if (matrix_free_only_ || auto_fallback_)
        return fail(kInvalidState, "Dog-Leg needs the direct solve: this handle is matrix-free only (the PCG step is inexact and S is never factorised)");
    if (ranks_.world() > 1 || tp_.distributed()) return fail(kInvalidState, "Dog-Leg: single rank only");
    return kOk;
}

int Solver::dogleg_segments(DlSegment out[2]) {
    out[0] = DlSegment{n_c_, g_c_, dcam_, scaled_ ? cam_scale_.dev.get() : nullptr, nullptr, nullptr, n_c_pad_, &cam_map_};
    out[1] = DlSegment{3 * n_pt_, g_l_, dl_, scaled_ ? pt_scale_.dev.get() : nullptr, nullptr, nullptr, 3 * n_pt_, &pt_map_};
    return 2;
}

void Solver::enqueue_jv_gram(const double* const a[2], const double* const b[2], double* out3) {
    static_assert(sizeof(PgLoss) % sizeof(double) == 0, "k_ba_jv_gram keeps the loss in doubles of LDS");
    launch_ba_jv_gram(dc_, view(st_.cur), a[0], a[1], b[0], b[1], partial_, n_partial_, out3, stream_, general_loss());
    if (have_priors()) {
        enqueue_prior_eval(st_.cur, false);
        launch_ba_prior_gram_add(n_c_, pri_diag_, a[0], b[0], out3, stream_);
    }
}

// solve_augmented(mu, 0) on a single rank, with dl_mode_ on: finish_step runs the tail, recover_factor leaves the ladder out
int Solver::solve_for_dogleg(double mu) {
    begin_solve(mu);
    last_pcg_iters_ = 0;
    last_reg_ = 0.0;
    tp_.set_factor_valid(false);
    int rc = assemble(mu, 0.0, true);   // (drops the Dog-Leg cache)
    if (rc != kOk) return rc;
    if (!one_wait_) {   // the flags are waited for where they are raised
        int lm_err = 0, failed = 0;
        HIP_TRY(hipMemcpyAsync(&lm_err, flags_, sizeof(int), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
        if (lm_err) return own_flag_raised();
        rc = factor_fresh(mu, 0.0, &failed);
        if (rc == kOk) rc = recover_factor(mu, failed, false);   // (a failed pivot: the error)
        if (rc != kOk) return rc;
    }
    return direct_solve(one_wait_, mu, nullptr, nullptr);
}

int Solver::dogleg_optimize(DlConfig* cfg, LmResult* res, DlIterRecord* hist, int hist_cap) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    if (cfg->variant != 0) return fail(kInvalidInput, "Dog-Leg runs on the sparse Cholesky variant (0) only");
    { const int rc = dogleg_refusal(); if (rc != kOk) return rc; }
    if (!(cfg->trust_region_radius > 0.0) || !(cfg->mu >= 0.0)) return fail(kInvalidInput, "Dog-Leg: the radius must be positive and mu non-negative");
    return run_dogleg(*this, cfg, res, hist, hist_cap);
}

int Solver::jv_gram(const double* a, const double* b, double out3[3]) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    if (ranks_.world() > 1) return fail(kInvalidState, "jv_gram: single rank only");
    return jv_gram_columns(a, b, out3);
}

// ---------------------------------------------------------------------------------------------
// parity / debug exports
// ---------------------------------------------------------------------------------------------
int Solver::get_residual(double* r_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    DeviceBuffer<double> d;
    HIP_TRY(d.alloc(2 * n_obs_));
    hipMemsetAsync(d, 0, 2 * n_obs_ * sizeof(double), stream_);
    launch_export_linearization(dc_, view(st_.cur), o_orig_, d, nullptr, nullptr, stream_, general_loss());
    hipError_t e = hipMemcpyAsync(r_out, d, 2 * n_obs_ * sizeof(double), hipMemcpyDeviceToHost, stream_);
    hipStreamSynchronize(stream_);
    return check_hip(e, "get_residual");
}

int Solver::get_jacobian_blocks(double* jc_out, double* jl_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    DeviceBuffer<double> dj, dl;
    HIP_TRY(dj.alloc(2 * dc_ * n_obs_));
    HIP_TRY(dl.alloc(6 * n_obs_));
    hipMemsetAsync(dj, 0, 2 * dc_ * n_obs_ * sizeof(double), stream_);
    hipMemsetAsync(dl, 0, 6 * n_obs_ * sizeof(double), stream_);
    launch_export_linearization(dc_, view(st_.cur), o_orig_, nullptr, dj, dl, stream_, general_loss());
    hipError_t e1 = hipMemcpyAsync(jc_out, dj, 2 * dc_ * n_obs_ * sizeof(double), hipMemcpyDeviceToHost, stream_);
    hipError_t e2 = hipMemcpyAsync(jl_out, dl, 6 * n_obs_ * sizeof(double), hipMemcpyDeviceToHost, stream_);
    hipStreamSynchronize(stream_);
    int rc = check_hip(e1, "get_jacobian_blocks");
    return rc != kOk ? rc : check_hip(e2, "get_jacobian_blocks");
}

// Dense S (9 n_cam square, row-major) and g_red in the reference's camera-side column order,
// re-assembled at the current parameters with the last lambda (the factorisation works in place).
int Solver::get_schur(double* S_out, double* gred_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    int rc = assemble(last_lambda_, 0.0);
    if (rc != kOk) return rc;
    const int64_t nref = 9 * n_cam_;
    if (gred_out) {   // (g_red as the solver sees it: of the scaled system when scaling is on)
        std::fill(gred_out, gred_out + nref, 0.0);
        rc = export_columns({{g_red_, &cam_map_, &cam_scale_}}, ExportAs::kPlain, gred_out);
        if (rc != kOk) return rc;
    }
    if (S_out) {
        std::fill(S_out, S_out + nref * nref, 0.0);
        // intrinsic variables exist but no factor touches them: S_ii = lambda.  A shard without a communicator exports its
        // partial S, and the partials sum to the whole: rank 0 alone carries these entries, as in schur_matvec
        if (ranks_.rank() == 0 || ranks_.has_comm())
            for (int64_t u : cam_map_.untouched) S_out[u * nref + u] = last_lambda_;
        return export_tiles_dense(cam_map_, nref, tp_.n_slots(), S_out);
    }
    return kOk;
}

// Parity export: y = S x through BOTH implementations of the reduced camera matrix -- the explicit tiles
// (k_cam_reduce + k_schur_rows, multiplied by the symmetric tile product) and the matrix-free operator of
// the implicit variant -- for the same lambda.  x and the outputs are in the reference's camera-side column
// order (9 n_cam entries).  Two independent code paths that must agree at any problem size.
int Solver::schur_matvec(double lambda, const double* x_in, double* y_explicit, double* y_implicit) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    st_.invalidate_step();
    const int64_t nref = 9 * n_cam_;
    std::vector<double> h(n_c_pad_, 0.0);
    cam_map_.gather(x_in, h.data());
    DeviceBuffer<double> xd, yd;   // (a parity export: allocated in the call)
    HIP_TRY(xd.alloc(n_c_pad_));
    HIP_TRY(yd.alloc(n_c_pad_));
    HIP_TRY(hipMemcpyAsync(xd, h.data(), n_c_pad_ * sizeof(double), hipMemcpyHostToDevice, stream_));
    for (int pass = 0; pass < 2; ++pass) {
        double* out = pass == 0 ? y_explicit : y_implicit;
        if (!out) continue;
        int rc = pass == 0 ? assemble(lambda, 0.0) : assemble_implicit(lambda);
        if (rc != kOk) return rc;
        if (pass == 0) tp_.sym_matvec(xd, yd);
        else implicit_matvec(xd, ranks_.rank() == 0 ? lambda : 0.0, yd, false);  // a shard's partial
        HIP_TRY(hipMemcpyAsync(h.data(), yd, n_c_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
        std::fill(out, out + nref, 0.0);
        cam_map_.scatter(h.data(), out, 0.0);
        if (ranks_.rank() == 0)  // intrinsic variables exist but no factor touches them: S_ii = lambda
            for (int64_t u : cam_map_.untouched) out[u] = lambda * x_in[u];
    }
    return kOk;
}

// get_hessian (explicit_schur.rs:1236-1238): H = J^T J, undamped, full symmetric, CSC in the global column order.  The
// device never forms it; this export rebuilds it on the host from the per-factor blocks the device linearises (an
// observer / DogLeg path, not the hot path): structural entries of every factor are kept even when a block is zero
// (a point behind its camera), as the reference's sparse product keeps them.  The device work is here -- the two copies that
// rebuild the caller's factor list, the priors' diagonal, the blocks --, the assembly is the host function hessian_csc.
int Solver::get_hessian_csc(int64_t* nnz_out, int64_t* colptr, int64_t* rowidx, double* values) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    if (ranks_.world() > 1) return fail(kInvalidState, "the Hessian export is single-rank");
    if (!nnz_out) return fail(kInvalidInput, "nnz_out is NULL");
    // the caller's factor list, rebuilt from the device's landmark-major lists (single rank: they hold every observation):
    // observation k of the device is the caller's o_orig[k], its camera / landmark the internal ones mapped back
    std::vector<uint32_t> cam_idx_h_(n_obs_), pt_idx_h_(n_obs_);
    {
        HIP_TRY(hipSetDevice(device_));
        if ((int64_t)o_orig_h_.size() != n_obs_) return fail(kInvalidState, "the Hessian export needs every observation on this rank");
        std::vector<uint32_t> oc(n_obs_), op(n_obs_);
        HIP_TRY(hipMemcpyAsync(oc.data(), o_cam_, n_obs_ * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipMemcpyAsync(op.data(), o_pt_, n_obs_ * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
        std::vector<int> linv(n_pt_);
        for (int64_t l = 0; l < n_pt_; ++l) linv[lmap_[l]] = (int)l;
        for (int64_t k = 0; k < n_obs_; ++k) {
            const int64_t i = o_orig_h_[k];
            cam_idx_h_[i] = (uint32_t)cinv_[oc[k]];
            pt_idx_h_[i] = (uint32_t)linv[op[k]];
        }
    }
    HessianCscInput in;
    in.n_cam = n_cam_; in.n_pt = n_pt_; in.n_obs = n_obs_; in.dc = dc_;
    in.cam_idx = cam_idx_h_.data(); in.pt_idx = pt_idx_h_.data();
    in.cmap = &cmap_; in.cam_map = &cam_map_; in.pt_map = &pt_map_;
    std::vector<double> pd;   // diag(P) of the camera priors, internal order: their cameras carry a diagonal block even when unobserved
    if (have_priors()) {
        enqueue_prior_eval(st_.cur, false);
        pd.resize(n_c_);
        HIP_TRY(hipMemcpyAsync(pd.data(), pri_diag_, n_c_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
        in.prior_diag = &pd;
    }
    *nnz_out = hessian_csc(in, nullptr, nullptr, nullptr);   // (no blocks: the count alone)
    if (!colptr) return kOk;
    if (!rowidx || !values) return fail(kInvalidInput, "rowidx / values are NULL");
    std::vector<double> jc((size_t)2 * dc_ * n_obs_), jl((size_t)6 * n_obs_);
    int rc = get_jacobian_blocks(jc.data(), jl.data());
    if (rc != kOk) return rc;
    in.jc = jc.data(); in.jl = jl.data();
    if (hessian_csc(in, colptr, rowidx, values) != *nnz_out) return fail(kInvalidState, "Hessian export: entry count mismatch");
    return kOk;
}

// tests: the pair records of the default Schur form as they sit on the device (host-built and copied, or written by the device)
int Solver::get_pair_records(uint32_t* recs4_out, int64_t cap_slots) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built");
    if (!precs_ || cap_slots < n_pair_slots_) return fail(kInvalidInput, "pair records: none on this handle, or the buffer is too small");
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipMemcpy(recs4_out, precs_, (size_t)n_pair_slots_ * sizeof(PairRec), hipMemcpyDeviceToHost));
    return kOk;
}

// mask[l] = 1 for the landmarks this rank assembles and back-substitutes (the caller's landmark numbering)
int Solver::owned_landmarks(uint8_t* mask) const {
    for (int64_t l = 0; l < n_pt_; ++l) mask[l] = (lmap_[l] >= lm_lo_ && lmap_[l] < lm_hi_) ? 1 : 0;
    return kOk;
}

int Solver::get_landmark_blocks(double* hinv_out, double* gl_out) {
    if (!have_params_) return fail(kInvalidState, "no parameters set");
    HIP_TRY(hipSetDevice(device_));
    if (hinv_out)   // the record's first six doubles: Hll^-1 as (00, 01, 02, 11, 12, 22) (ba_kernels.h); expanded below
        HIP_TRY(hipMemcpy2DAsync(hinv_out, 9 * sizeof(double), hinv_, kLmStride * sizeof(double), 6 * sizeof(double), (size_t)n_pt_,
                                 hipMemcpyDeviceToHost, stream_));
    if (gl_out) HIP_TRY(hipMemcpyAsync(gl_out, g_l_, 3 * n_pt_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    if (hinv_out)
        for (int64_t l = 0; l < n_pt_; ++l) {
            double* h = hinv_out + 9 * l;
            const double s[6] = {h[0], h[1], h[2], h[3], h[4], h[5]};
            h[0] = s[0]; h[1] = s[1]; h[2] = s[2]; h[3] = s[1]; h[4] = s[3]; h[5] = s[4]; h[6] = s[2]; h[7] = s[4]; h[8] = s[5];
        }
    if (tree_shard_) {  // back to the caller's landmark order
        std::vector<double> t;
        if (hinv_out) { t.assign(hinv_out, hinv_out + 9 * n_pt_); blocks_to_caller(lmap_, 9, t.data(), hinv_out); }
        if (gl_out) { t.assign(gl_out, gl_out + 3 * n_pt_); blocks_to_caller(lmap_, 3, t.data(), gl_out); }
    }
    return kOk;
}


int Solver::camera_covariance(double* out) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    if (!out) return fail(kInvalidInput, "cov_out is NULL");
    if (ranks_.world() > 1 || tp_.distributed()) return fail(kInvalidState, "covariance: multi-rank handles are not supported (single rank only)");
    if (matrix_free_only_)
        return fail(kInvalidState, auto_fallback_ ? "covariance: the automatic variant selection chose the matrix-free PCG for this handle: there is no factor to invert"
                                                  : "covariance: this handle was built matrix-free only: there is no factor to invert");
    HIP_TRY(hipSetDevice(device_));
    std::vector<double> blk((size_t)n_cam_ * dc_ * dc_);
    std::string err;
    const int rc = tp_.inverse().blocks(cam_map_.pos.data(), n_cam_, dc_, blk.data(), &err);
    if (rc == 1) return fail(kInvalidState, "covariance: " + err + " (the Iterative and matrix-free variants have no factor)");
    if (rc != 0) return fail(kDeviceError, "covariance: " + err);
    for (int64_t c = 0; c < n_cam_; ++c) {
        double* o = out + (size_t)c * 81;
        std::fill(o, o + 81, 0.0);
        for (int a = 0; a < dc_; ++a)
            for (int b = 0; b < dc_; ++b) o[a * 9 + b] = blk[((size_t)c * dc_ + a) * dc_ + b];
        if (dc_ == 6)   // get_schur's intrinsics rows: lambda on the diagonal, no cross terms
            for (int a = 6; a < 9; ++a) o[a * 9 + a] = 1.0 / last_lambda_;
    }
    return kOk;
}

void Solver::LandmarkCov::release() {
    lists.reset(); err.reset(); out.reset();   // (null out: landmark_covariance sets up again)
    n_small = n_large = 0;
    pairs = 0; bytes = 0;
}

// The landmark lists of the covariance pass from the observation pointers (landmark_cov_lists.h), and the pass's buffers
int Solver::lc_setup() {
    std::vector<int> ptr(n_pt_ + 1);
    HIP_TRY(hipMemcpy(ptr.data(), pt_ptr_, (n_pt_ + 1) * sizeof(int), hipMemcpyDeviceToHost));
    const LandmarkCovLists ll = build_landmark_cov_lists(n_pt_, ptr.data(), kLcSmallK);
    const size_t b_lists = std::max<size_t>(ll.lists.size(), 1) * sizeof(int), b_out = 9 * (size_t)n_pt_ * sizeof(double);
    hipError_t e = lc_.lists.upload(ll.lists);
    if (e == hipSuccess) e = lc_.err.alloc(1);
    if (e == hipSuccess) e = lc_.out.alloc(9 * (size_t)n_pt_);
    if (e != hipSuccess) { lc_.release(); return check_hip(e, "landmark covariance set-up"); }
    lc_.n_large = ll.n_large;
    lc_.n_small = ll.n_small;
    lc_.pairs = ll.pairs;
    lc_.bytes = b_lists + sizeof(int) + b_out;
    return kOk;
}

int Solver::landmark_covariance(double* out) {
    if (!have_structure_) return fail(kInvalidState, "Block structure not built. Call set_structure() first.");
    if (!out) return fail(kInvalidInput, "cov_out is NULL");
    if (ranks_.world() > 1 || tp_.distributed()) return fail(kInvalidState, "landmark covariance: multi-rank handles are not supported (single rank only)");
    if (matrix_free_only_)
        return fail(kInvalidState, auto_fallback_ ? "landmark covariance: the automatic variant selection chose the matrix-free PCG for this handle: there is no factor to invert"
                                                  : "landmark covariance: this handle was built matrix-free only: there is no factor to invert");
    if (tp_.factor_valid() && (factor_lin_ < 0 || !have_params_))
        return fail(kInvalidState, "landmark covariance: the linearisation point of the factor is gone (parameters or column scaling were set after the solve)");
    HIP_TRY(hipSetDevice(device_));
    std::string err;
    bool recomputed = false;
    int rc = tp_.inverse().ensure(&recomputed, &err);
    if (rc == 1) return fail(kInvalidState, "landmark covariance: " + err + " (the Iterative and matrix-free variants have no factor)");
    if (rc != 0) return fail(kDeviceError, "landmark covariance: " + err);
    if (!lc_.out && (rc = lc_setup()) != kOk) return rc;
    lc_.recomputed = recomputed;
    lc_.ms = 0.0;
    BAView v = view(factor_lin_);   // the cameras the factor was linearised at; the points come from the landmark records
    v.cam_scale = factor_scaled_ ? cam_scale_.dev.get() : nullptr;
    v.pt_scale = factor_scaled_ ? pt_scale_.dev.get() : nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    const bool timed = tp_.inverse().timing();
    if (timed) {
        HIP_TRY(hipEventCreate(&ev[0]));
        HIP_TRY(hipEventCreate(&ev[1]));
    }
    HIP_TRY(hipMemsetAsync(lc_.err, 0, sizeof(int), stream_));
    if (timed) HIP_TRY(hipEventRecord(ev[0], stream_));
    launch_landmark_cov(dc_, v, hinv_, tp_.inverse().map(), lc_.lists, lc_.n_small, lc_.lists + lc_.n_small, lc_.n_large, lc_.out, lc_.err, stream_, general_loss());
    if (timed) HIP_TRY(hipEventRecord(ev[1], stream_));
    hipError_t e = hipGetLastError();
    std::vector<double> blk(9 * (size_t)n_pt_);
    int kerr = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(blk.data(), lc_.out, blk.size() * sizeof(double), hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess) e = hipMemcpyAsync(&kerr, lc_.err, sizeof(int), hipMemcpyDeviceToHost, stream_);
    const hipError_t se = hipStreamSynchronize(stream_);
    if (e == hipSuccess) e = se;
    if (timed) {
        float ms = 0.0f;
        if (e == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) lc_.ms = ms;
        (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
    }
    if (e != hipSuccess) return check_hip(e, "landmark covariance");
    if (kerr) return fail(kDeviceError, "landmark covariance: a covisible camera pair is not in the factor's tile pattern");
    blocks_to_caller(lmap_, 9, blk.data(), out);
    return kOk;
}

}  // namespace apex
