// host_harness_capi_guard.cpp -- the one guarded entry path of the C ABI (csrc/capi_guard.h) over a fake handle type: g++, no GPU,
// no HIP.  with_handle() refuses a null handle and a handle without a solver without running the body, passes every status code
// through, and turns what the body throws into the status code of the rule; HandleOwner::create does the same for a throwing
// constructor and leaves nothing behind.  Prints "ok <n checks>" and returns 0, or names the first check that failed
// (tests/test_capi_guard_host.py).
#include <stdio.h>

#include <new>
#include <stdexcept>
#include <string>

#include "capi_guard.h"

static int n_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++n_checks;                                                      \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static int n_alive = 0;   // FakeSolver objects constructed and not yet destroyed
struct FakeSolver {
    int value;
    FakeSolver(int v, int mode) : value(v) {   // mode 1, 2, 3: the constructor throws
        if (mode == 1) throw std::runtime_error("refused");
        if (mode == 2) throw std::bad_alloc();
        if (mode == 3) throw 7;
        ++n_alive;
    }
    ~FakeSolver() { --n_alive; }
    std::string text;   // (something a body can grow)
};
struct fake_handle : apex::Handle<FakeSolver> {};

int main() {
    using apex::HandleOwner;
    using apex::with_handle;
    int ran = 0;
    auto body_ok = [&](FakeSolver&) { ++ran; return APEXGPU_OK; };

    // a null handle, a handle with a null solver: APEXGPU_ERR_INVALID_STATE, and the body does not run
    CHECK(with_handle((fake_handle*)nullptr, body_ok) == APEXGPU_ERR_INVALID_STATE);
    CHECK(with_handle((const fake_handle*)nullptr, body_ok) == APEXGPU_ERR_INVALID_STATE);
    fake_handle empty;
    CHECK(with_handle(&empty, body_ok) == APEXGPU_ERR_INVALID_STATE);
    CHECK(ran == 0);

    fake_handle* h = nullptr;
    CHECK(HandleOwner::create(&h, 41, 0) == APEXGPU_OK && h && n_alive == 1);
    CHECK(HandleOwner::solver(h) && HandleOwner::solver(h)->value == 41);

    // the body runs once per call with the handle's own solver, and every status code comes back as it is
    const int codes[] = {APEXGPU_OK, APEXGPU_ERR_FACTORIZATION_FAILED, APEXGPU_ERR_SINGULAR_MATRIX, APEXGPU_ERR_SPARSE_MATRIX_CREATION,
                         APEXGPU_ERR_MATRIX_CONVERSION, APEXGPU_ERR_INVALID_INPUT, APEXGPU_ERR_INVALID_STATE, APEXGPU_ERR_DEVICE, 17};
    for (int code : codes) {
        const int before = ran;
        CHECK(with_handle(h, [&](FakeSolver& s) { ++ran; s.value += 1; return code; }) == code);
        CHECK(ran == before + 1);
    }
    CHECK(HandleOwner::solver(h)->value == 41 + (int)(sizeof codes / sizeof codes[0]));
    CHECK(with_handle(h, [&](FakeSolver& s) { return &s == HandleOwner::solver(h) ? APEXGPU_OK : 1; }) == APEXGPU_OK);

    // what the body throws: bad_alloc and every std::exception are INVALID_INPUT, anything else is INVALID_STATE
    ran = 0;
    CHECK(with_handle(h, [&](FakeSolver&) -> int { ++ran; throw std::bad_alloc(); }) == APEXGPU_ERR_INVALID_INPUT);
    CHECK(with_handle(h, [&](FakeSolver&) -> int { ++ran; throw std::length_error("too long"); }) == APEXGPU_ERR_INVALID_INPUT);
    CHECK(with_handle(h, [&](FakeSolver&) -> int { ++ran; throw std::runtime_error("no"); }) == APEXGPU_ERR_INVALID_INPUT);
    CHECK(with_handle(h, [&](FakeSolver&) -> int { ++ran; throw 3; }) == APEXGPU_ERR_INVALID_STATE);
    CHECK(ran == 4);
    // ... thrown by the library, with a body's own objects alive: a string that cannot be that long, after one that grew
    CHECK(with_handle(h, [&](FakeSolver& s) -> int {
              s.text.assign(1000, 'x');
              std::string t(s.text);
              t.resize(t.max_size() + 1);
              return APEXGPU_OK;
          }) == APEXGPU_ERR_INVALID_INPUT);
    CHECK(with_handle(h, [&](FakeSolver& s) { return s.text.size() == 1000 ? APEXGPU_OK : 1; }) == APEXGPU_OK);   // the handle is still good

    // a const handle: the same path
    const fake_handle* ch = h;
    CHECK(with_handle(ch, [&](const FakeSolver& s) { return s.value; }) == HandleOwner::solver(h)->value);
    CHECK(with_handle(ch, [&](FakeSolver&) -> int { throw 3; }) == APEXGPU_ERR_INVALID_STATE);

    // guarded() by itself, as the entry points without a handle use it
    CHECK(apex::guarded([] { return 5; }) == 5);
    CHECK(apex::guarded([]() -> int { throw std::out_of_range("x"); }) == APEXGPU_ERR_INVALID_INPUT);
    CHECK(apex::guarded([]() -> int { throw "text"; }) == APEXGPU_ERR_INVALID_STATE);

    // create with a constructor that throws: the guard's code, no handle, nothing left alive; destroy ends the solver
    for (int mode = 1; mode <= 3; ++mode) {
        fake_handle* bad = nullptr;
        CHECK(HandleOwner::create(&bad, 1, mode) == (mode == 3 ? APEXGPU_ERR_INVALID_STATE : APEXGPU_ERR_INVALID_INPUT));
        CHECK(bad == nullptr && n_alive == 1);
    }
    HandleOwner::destroy(h);
    CHECK(n_alive == 0);
    HandleOwner::destroy((fake_handle*)nullptr);

    printf("ok %d\n", n_checks);
    return 0;
}
