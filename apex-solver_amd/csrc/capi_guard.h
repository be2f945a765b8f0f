// capi_guard.h -- the one rule of the C boundary (include/apexgpu.h), in one place.  Plain C++17, no HIP.
//
// No C++ exception may cross the C boundary (a caller in Rust / C / ctypes cannot unwind it), so every entry point that
// touches a handle runs its body through with_handle(): a null handle, or one without a solver, is
// APEXGPU_ERR_INVALID_STATE and the body does not run; otherwise the body runs under guarded() with a reference to the
// solver.  What is thrown becomes a status code and nothing else: no error text is written into the handle.
//   std::bad_alloc, any std::exception (length_error from a size taken from an untrusted header, ...)  APEXGPU_ERR_INVALID_INPUT
//   anything else                                                                                      APEXGPU_ERR_INVALID_STATE
// Which solver methods allocate is then nobody's business at the boundary.  The solver pointer of a handle is private:
// with_handle() is the way to it, and HandleOwner is the way around the guard for the few places that own the pointer
// itself (create, destroy, the lockstep communicator) -- an entry point cannot skip the guard without naming it.
#pragma once
#include <exception>
#include <memory>
#include <new>

#include "../../include/apexgpu.h"

namespace apex {

template <typename F>
int guarded(F&& f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return APEXGPU_ERR_INVALID_INPUT;
    } catch (const std::exception&) {
        return APEXGPU_ERR_INVALID_INPUT;
    } catch (...) {
        return APEXGPU_ERR_INVALID_STATE;
    }
}

// Base of the opaque handle structs: `struct apexgpu_solver : apex::Handle<apex::Solver> {};`
template <typename S>
class Handle {
  public:
    using solver_type = S;

  private:
    S* s = nullptr;
    template <typename H, typename F>
    friend int with_handle(H* h, F&& f) noexcept;
    friend struct HandleOwner;
};

template <typename H, typename F>
int with_handle(H* h, F&& f) noexcept {
    if (!h || !h->s) return APEXGPU_ERR_INVALID_STATE;
    return guarded([&] { return f(*h->s); });
}

struct HandleOwner {
    template <typename H>
    static auto& solver(H* h) { return h->s; }
    // *out = a handle of type H with a solver built from `args`; a failed allocation is APEXGPU_ERR_INVALID_STATE, what the
    // solver's constructor throws goes through the guard; nothing is left behind either way
    template <typename H, typename... A>
    static int create(H** out, A... args) noexcept {
        return guarded([&]() -> int {
            std::unique_ptr<H> h(new (std::nothrow) H());
            if (!h) return APEXGPU_ERR_INVALID_STATE;
            h->s = new (std::nothrow) typename H::solver_type(args...);
            if (!h->s) return APEXGPU_ERR_INVALID_STATE;
            *out = h.release();
            return APEXGPU_OK;
        });
    }
    template <typename H>
    static void destroy(H* h) {
        if (!h) return;
        delete h->s;
        delete h;
    }
};

}  // namespace apex
