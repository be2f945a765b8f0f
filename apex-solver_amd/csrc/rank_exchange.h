// rank_exchange.h -- what one rank of a sharded solve exchanges with the others, and through what.
//
// An exchange is a value: the list of device buffers that are combined over the ranks at one point of the solve.  The
// solver and the tile plan state each point once (Solver::exchange, TilePlan::exchange); production issues the list through
// the communicator (issue), the single-process lockstep test plays the same list by hand (capi_debug.cpp).
// RankExchange owns the rank's place (rank, world), the communicator and the text of the last call that failed.  Every
// collective returns a Status the caller hands on, and returns kOk at once, touching nothing, unless active().
#pragma once
#include <vector>

#include "comm.h"
#include "lm_loop.h"   // Status
#ifndef APEX_COMM_HOST_ONLY
#include "device_buffer.h"
#endif

namespace apex {

// kSum: doubles summed, the result needed on rank `root` only or, root -1, on every rank; kMaxInt: ints maximised, on every rank
struct ExchangeItem { enum Op { kSum, kMaxInt } op; void* dev; size_t n; int root; };
using ExchangeList = std::vector<ExchangeItem>;

class RankExchange {
   public:
    int set_shard(int rank, int world) { if (world < 1 || rank < 0 || rank >= world) return refuse(kInvalidInput, "bad rank/world"); rank_ = rank; world_ = world; return kOk; }
    // the communicator of set_shard's world; nullptr: kDeviceError with `err` as the text
    int adopt(std::unique_ptr<Communicator> c, const std::string& err) { if (!c) return refuse(kDeviceError, err); comm_ = std::move(c); return kOk; }
    void close() { comm_.reset(); }
    int rank() const { return rank_; }
    int world() const { return world_; }
    bool has_comm() const { return comm_ != nullptr; }
    // (a handle may be sharded, world > 1, with no communicator: it computes its partial system and exchanges nothing)
    bool active() const { return has_comm() && world_ > 1; }
    const std::string& error() const { return err_; }   // of the last call that did not return kOk

    int sum(double* dev, size_t n, hipStream_t s) { return active() ? done(comm_->all_reduce_sum(dev, n, s)) : kOk; }
    int max_int(int* dev, size_t n, hipStream_t s) { return active() ? done(comm_->all_reduce_max(dev, n, s)) : kOk; }
    int reduce(double* dev, size_t n, int root, hipStream_t s) { return active() ? done(comm_->reduce_sum(dev, n, root, s)) : kOk; }
    int all_gather(const void* send, void* recv, size_t bytes_per_rank, hipStream_t s) { return active() ? done(comm_->all_gather(send, recv, bytes_per_rank, s)) : kOk; }
    int broadcast(double* dev, size_t n, int root, hipStream_t s) { return active() ? done(comm_->broadcast(dev, n, root, s)) : kOk; }
    // one list as one group of collectives, in the list's order; an item of no elements is passed over
    int issue(const ExchangeList& list, hipStream_t s);
#ifndef APEX_COMM_HOST_ONLY
    DeviceBuffer<int64_t> lm_ranges;   // [world][2] staging of every rank's landmark range: Solver::get_params, sized with the communicator
#endif

   private:
    int refuse(int code, const std::string& why) { err_ = why; return code; }
    int done(bool ok) { return ok ? kOk : refuse(kDeviceError, comm_->error()); }
    int rank_ = 0, world_ = 1;
    std::unique_ptr<Communicator> comm_;
    std::string err_;
};

}  // namespace apex
