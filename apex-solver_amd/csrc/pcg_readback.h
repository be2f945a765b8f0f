// pcg_readback.h -- where the host reads a PCG loop's device scalars (pcg_loop.h): two pinned slots of eight doubles, laid out as
// Scalars (pcg_kernels.h), and an event behind the copy into each.  Created on the first ensure(), gone with the owner.
#pragma once
#include <hip/hip_runtime.h>

#include "device_buffer.h"

namespace apex {

template <typename Scalars>
class PcgReadback {
    static_assert(sizeof(Scalars) == 8 * sizeof(double), "a slot is eight doubles");

   public:
    PcgReadback() = default;
    PcgReadback(const PcgReadback&) = delete;
    PcgReadback& operator=(const PcgReadback&) = delete;
    ~PcgReadback() { release(); }
    hipError_t ensure() {
        if (host_) return hipSuccess;
        hipError_t e = host_.alloc(2);
        for (hipEvent_t& ev : ev_) if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) release();
        return e;
    }
    void release() {
        host_.reset();
        for (hipEvent_t& ev : ev_) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
    }
    // the first n_doubles of the device scalars to `slot`, and the event wait(slot) waits for
    hipError_t post(int slot, const double* dev_scalars, int n_doubles, hipStream_t stream) {
        const hipError_t e = hipMemcpyAsync(&host_[slot], dev_scalars, n_doubles * sizeof(double), hipMemcpyDeviceToHost, stream);
        return e != hipSuccess ? e : hipEventRecord(ev_[slot], stream);
    }
    hipError_t wait(int slot) { return hipEventSynchronize(ev_[slot]); }
    Scalars& host(int slot) { return host_[slot]; }

   private:
    PinnedBuffer<Scalars> host_;
    hipEvent_t ev_[2] = {nullptr, nullptr};
};

}  // namespace apex
