// tile_sinv.h -- marginal covariances: selected inversion of a TilePlan's factor (the lists: sinv_lists.h; the kernels:
// sinv_kernels.hip).  SelectedInverse owns everything that is selected inversion -- Z, the Y tiles of the largest level group,
// the device lists, the timing -- and reads the plan through a view the plan fills in.  It writes nothing of the plan: L is
// left as it is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <string>
#include <vector>

#include "ba_kernels.h"
#include "device_buffer.h"
#include "tile_tasks.h"

namespace apex {

// one launch: nine workgroups per task (one per 48 x 48 block of C); no atomics, a fixed summation order
void launch_sinv_gemm(const SinvTask* tasks, int n_tasks, const SinvProd* prods, hipStream_t s);
// out[v][a][b] = (Z[p + a][p + b] + Z[p + b][p + a]) / 2, p = pos[v] (a d x d block inside one diagonal tile of Z)
void launch_sinv_diag_blocks(const double* z, const int* diag_slot, const int64_t* pos, int64_t n_var, int d, double* out, hipStream_t s);

// What the selected inversion reads of its plan, as of the call (TilePlan::inverse() fills it in).
struct SinvPlanView {
    const double* tiles = nullptr;   // L (device), by slot
    const double* linv = nullptr;    // [nt] inverses of the diagonal tiles of L (device)
    const int* slot = nullptr;       // device: slot[I * nt + J]
    const int* diag_slot = nullptr;  // device
    int nt = 0;
    int64_t n_slots = 0;
    hipStream_t stream = nullptr;
    const int* slot_host = nullptr;
    const std::vector<std::vector<int>>* group_cols = nullptr;   // the level groups' columns in execution order
    bool distributed = false;        // the plan is cut for several ranks
    bool factor_valid = false;       // the tiles hold a factor ...
    uint64_t factor_epoch = 0;       // ... and this counts the writes of the tiles and the factors declared valid
};

class SelectedInverse {
   public:
    void bind(const SinvPlanView& v) { v_ = v; }
    // out[v] = the d x d diagonal block of Z at n_pad position pos[v] (symmetrised), after the recurrence.  The Z tiles (as many as
    // L's), the Y tiles of the largest level group and the lists are allocated on the first call only and live until
    // release().  Returns 0, 1 (refused: distributed plan or no valid factor; *err says why) or 2 (HIP error).  Syncs.
    int blocks(const int64_t* pos, int64_t n_var, int d, double* out, std::string* err);
    // Z of the held factor for a caller that reads Z itself (the landmark covariances): reuses Z when blocks() or ensure() has
    // computed it for this factor (*recomputed = false), else runs the recurrence without the diagonal gather.  Z is current
    // exactly while the factor is valid and the plan's epoch is the one Z was computed at.  Returns as blocks().
    int ensure(bool* recomputed, std::string* err);
    TileMap map() const { return TileMap{z_, v_.slot, v_.nt}; }   // Z, addressed as TilePlan::tilemap() addresses S (valid after ensure)
    void release();
    size_t bytes() const { return bytes_; }   // device memory the first call added (0 before)
    // per level group (execution order, root group first): milliseconds of its three launches in the last call -- recorded
    // only while enabled (events between the groups)
    void enable_timing(bool on) { timing_ = on; }
    bool timing() const { return timing_; }
    const std::vector<double>& group_ms() const { return group_ms_; }
    // tile products of one selected inversion: Y, off-diagonal Z, diagonal Z (each 2*144^3 flop)
    void op_counts(int64_t* y, int64_t* zoff, int64_t* zdiag) const { *y = n_[0]; *zoff = n_[1]; *zdiag = n_[2]; }

   private:
    std::string setup();
    int check(std::string* err) const;   // 0, or 1 with the refusal
    // the recurrence (set-up on the first call) enqueued, with timing events when enabled (0 or 2); after the caller's
    // synchronisation collect reads and destroys them
    int enqueue(std::vector<hipEvent_t>* ev, std::string* err);
    void collect(std::vector<hipEvent_t>& ev, bool ok);
    bool current() const { return v_.factor_valid && z_epoch_ == v_.factor_epoch; }

    SinvPlanView v_;
    DeviceBuffer<double> z_, y_;
    DeviceBuffer<SinvTask> tasks_;
    DeviceBuffer<SinvProd> prods_;
    std::vector<std::array<int, 4>> groups_;   // root group first (SinvLists::groups)
    int64_t n_[3] = {0, 0, 0};
    size_t bytes_ = 0;
    bool timing_ = false;
    std::vector<double> group_ms_;
    uint64_t z_epoch_ = 0;   // the plan's epoch whose factor z_ holds the selected inverse of (0: none; a valid factor's is >= 1)
};

}  // namespace apex
