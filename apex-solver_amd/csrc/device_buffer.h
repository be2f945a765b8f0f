// device_buffer.h -- the two owners of memory the library allocates through HIP: DeviceBuffer<T> (one hipMalloc block) and
// PinnedBuffer<T> (one hipHostMalloc block).  Move-only; the destructor frees; alloc / alloc_zero / upload free what was held
// first and return the HIP status.  Both convert to T*, so a buffer is passed, indexed, offset and null-tested as the
// pointer it owns.  Every allocation holds at least kMinBytes: an empty list still gets an address, and upload() of an empty
// list clears it -- the kernels issue their first loads unconditionally on a clamped index (ba_kernels.hip), so entry 0 of a
// list must exist and be a valid index even on a rank that holds no observation at all.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <algorithm>

namespace apex {

constexpr size_t kMinBytes = 64;   // (the widest unconditional first load is 32 bytes: two double2 of a projection record)

template <typename T>
class DeviceBuffer {
   public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { reset(); }

    hipError_t alloc(size_t n) {   // contents undefined
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), std::max<size_t>(n * sizeof(T), kMinBytes));
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    hipError_t alloc_zero(size_t n) {   // cleared on the NULL stream: the caller synchronises the device before a non-blocking stream reads it
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemset(p_, 0, std::max<size_t>(n * sizeof(T), kMinBytes));
    }
    template <typename C>
    hipError_t upload(const C& hv) {   // synchronous copy of anything with data() / size() and T's element size
        static_assert(sizeof(*hv.data()) == sizeof(T), "upload: element size differs");
        const hipError_t e = alloc(hv.size());
        if (e != hipSuccess) return e;
        if (hv.size() == 0) return hipMemset(p_, 0, kMinBytes);
        return hipMemcpy(p_, hv.data(), hv.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    void reset() {
        if (p_) { (void)hipFree(p_); p_ = nullptr; }
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }

   private:
    T* p_ = nullptr;
};

template <typename T>
class PinnedBuffer {
   public:
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    PinnedBuffer& operator=(PinnedBuffer&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { reset(); }

    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), std::max<size_t>(n, 1) * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() {
        if (p_) { (void)hipHostFree(p_); p_ = nullptr; }
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }

   private:
    T* p_ = nullptr;
};

}  // namespace apex
