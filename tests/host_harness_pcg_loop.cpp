// host_harness_pcg_loop.cpp -- drives pcg_loop_one_behind (csrc/pcg_loop.h), the host loop of both device PCG variants, with
// scripted callables that record every call: g++, no GPU, no HIP.  Prints "ok <n checks>" and returns 0, or names the first
// check that failed (tests/test_pcg_loop_host.py).
#include <stdio.h>

#include <string>

#include "pcg_loop.h"

using namespace apex;

static int n_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++n_checks;                                                      \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

// One run of the loop.  The log holds every call in order: e<slot> enqueue, w<slot> wait, v<slot> verdict.
struct Script {
    int stop_at = -1;                               // the iteration whose verdict is `stop` (-1: none)
    PcgVerdict stop = PcgVerdict::kStopCounted;
    int fail_enqueue = -1, fail_wait = -1;          // the enqueue / wait call (0-based, in call order) that returns `status`
    int status = 7;
};
struct Run {
    std::string log;
    int n_enqueue = 0, n_wait = 0, n_verdict = 0;
    PcgLoopResult res{0, 0};
};
static Run run(int max_iter, const Script& sc) {
    Run r;
    auto note = [&](char what, int slot) { if (!r.log.empty()) r.log += ' '; r.log += what; r.log += std::to_string(slot); };
    r.res = pcg_loop_one_behind(
        max_iter, [&](int slot) { note('e', slot); return r.n_enqueue++ == sc.fail_enqueue ? sc.status : 0; },
        [&](int slot) { note('w', slot); return r.n_wait++ == sc.fail_wait ? sc.status : 0; },
        [&](int slot) { note('v', slot); return r.n_verdict++ == sc.stop_at ? sc.stop : PcgVerdict::kGoOn; });
    return r;
}
static int min_i(int a, int b) { return a < b ? a : b; }

int main() {
    {   // no exit: the exact sequence, no speculative enqueue behind the last iteration, the count is the cap
        const char* want[6] = {"", "e0 w0 v0", "e0 e1 w0 v0 w1 v1", nullptr, nullptr, "e0 e1 w0 v0 e0 w1 v1 e1 w0 v0 e0 w1 v1 w0 v0"};
        for (int m : {0, 1, 2, 5}) {
            const Run r = run(m, Script());
            CHECK(r.log == want[m]);
            CHECK(r.res.iterations == m && r.res.status == 0 && r.n_enqueue == m && r.n_wait == m && r.n_verdict == m);
        }
        CHECK(run(-3, Script()).log.empty());   // (a negative cap is no iteration)
    }
    {   // "stop, counted" at iteration k: k + 1 iterations, ONE speculative enqueue beyond it when k + 1 < cap, else none
        Script sc; sc.stop_at = 2;
        Run r = run(5, sc);
        CHECK(r.log == "e0 e1 w0 v0 e0 w1 v1 e1 w0 v0" && r.res.iterations == 3 && r.res.status == 0);
        sc.stop_at = 4;
        r = run(5, sc);
        CHECK(r.log == "e0 e1 w0 v0 e0 w1 v1 e1 w0 v0 e0 w1 v1 w0 v0" && r.res.iterations == 5);
        sc.stop_at = 0;
        CHECK(run(1, sc).log == "e0 w0 v0" && run(1, sc).res.iterations == 1);
        CHECK(run(2, sc).log == "e0 e1 w0 v0" && run(2, sc).res.iterations == 1);
        for (int m = 1; m <= 6; ++m)
            for (int k = 0; k < m; ++k) {
                sc.stop_at = k;
                r = run(m, sc);
                CHECK(r.res.iterations == k + 1 && r.res.status == 0);
                CHECK(r.n_enqueue == min_i(k + 2, m) && r.n_wait == k + 1 && r.n_verdict == k + 1);
            }
    }
    {   // "stop, not counted" at iteration k: k iterations; the calls are those of the counted stop
        Script sc; sc.stop = PcgVerdict::kStopUncounted; sc.stop_at = 2;
        Run r = run(5, sc);
        CHECK(r.log == "e0 e1 w0 v0 e0 w1 v1 e1 w0 v0" && r.res.iterations == 2 && r.res.status == 0);
        sc.stop_at = 0;
        CHECK(run(1, sc).log == "e0 w0 v0" && run(1, sc).res.iterations == 0);
        for (int m = 1; m <= 6; ++m)
            for (int k = 0; k < m; ++k) {
                sc.stop_at = k;
                r = run(m, sc);
                CHECK(r.res.iterations == k && r.res.status == 0);
                CHECK(r.n_enqueue == min_i(k + 2, m) && r.n_wait == k + 1 && r.n_verdict == k + 1);
            }
        // the cap does not show in the count: k, k + 1 or 5000 stop at the same iteration, counted or not
        for (PcgVerdict v : {PcgVerdict::kStopCounted, PcgVerdict::kStopUncounted}) {
            sc.stop = v; sc.stop_at = 3;
            const int want = v == PcgVerdict::kStopCounted ? 4 : 3;
            CHECK(run(4, sc).res.iterations == want && run(5, sc).res.iterations == want && run(5000, sc).res.iterations == want);
        }
    }
    {   // a status from enqueue ends the loop with it, nothing is called behind it: the first enqueue, one in the middle, and the
        // speculative one behind an iteration whose verdict would have stopped the loop
        Script sc; sc.status = 11; sc.fail_enqueue = 0;
        Run r = run(5, sc);
        CHECK(r.log == "e0" && r.res.status == 11);
        sc.fail_enqueue = 3;
        r = run(5, sc);
        CHECK(r.log == "e0 e1 w0 v0 e0 w1 v1 e1" && r.res.status == 11);
        sc.fail_enqueue = 2; sc.stop_at = 1;
        r = run(5, sc);
        CHECK(r.log == "e0 e1 w0 v0 e0" && r.res.status == 11);
        sc.fail_enqueue = 1; sc.stop_at = -1;   // (the first speculative one: no wait has been made yet)
        r = run(2, sc);
        CHECK(r.log == "e0 e1" && r.res.status == 11);
    }
    {   // ... and so does a status from wait: the first wait, one in the middle, the last iteration's (no speculative enqueue
        // before it), and the wait of an iteration whose verdict is never asked
        Script sc; sc.status = -4; sc.fail_wait = 0;
        Run r = run(5, sc);
        CHECK(r.log == "e0 e1 w0" && r.res.status == -4);
        sc.fail_wait = 2;
        r = run(5, sc);
        CHECK(r.log == "e0 e1 w0 v0 e0 w1 v1 e1 w0" && r.res.status == -4);
        r = run(3, sc);
        CHECK(r.log == "e0 e1 w0 v0 e0 w1 v1 w0" && r.res.status == -4);
        sc.fail_wait = 1; sc.stop_at = 1;
        r = run(5, sc);
        CHECK(r.log == "e0 e1 w0 v0 e0 w1" && r.res.status == -4 && r.n_verdict == 1);
    }
    printf("ok %d\n", n_checks);
    return 0;
}
