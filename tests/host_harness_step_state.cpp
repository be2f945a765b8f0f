// host_harness_step_state.cpp -- walks the transitions of StepState (csrc/step_state.h) on the host: g++, no GPU, no HIP.
// Prints "ok <n checks>" and returns 0, or names the first check that failed (tests/test_step_state_host.py).
#include <stdio.h>
#include <string.h>

#include "step_state.h"

using namespace apex;

static int n_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++n_checks;                                                      \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static bool refused(Status rc, const StepState& s, const char* text) { return rc == kInvalidState && strcmp(s.refusal, text) == 0; }

static const StepAnswers kA{3.0, 4.0, 5.0, 18.0}, kB{6.0, 7.0, 8.0, 50.0};

// a solve that posts its answers at its own wait (the eager evaluation, a Dog-Leg step)
static void solve_posting(StepState& s, const StepAnswers& a) { s.begin_solve(); s.step_computed(); s.post_answers(a); }
// ... and one that does not: the caller computes what is asked
static void solve_plain(StepState& s) { s.begin_solve(); s.step_computed(); }

int main() {
    const StepAnswers* a = nullptr;
    {   // before any solve: every call is refused with its own text, nothing moves
        StepState s;
        CHECK(refused(s.ask_stats(&a), s, "no step computed"));
        CHECK(refused(s.ask_trial(&a), s, "no step computed"));
        CHECK(refused(s.commit(), s, "no trial point"));
        CHECK(refused(s.begin_discard(), s, "no trial point"));
        CHECK(refused(s.finish_discard(), s, "no trial point"));
        CHECK(s.cur == 0 && !s.have_step && !s.have_trial && !s.answered());
    }
    {   // solve -> stats -> eval -> commit, answers served
        StepState s;
        solve_posting(s, kA);
        CHECK(s.ask_stats(&a) == kOk && a && a->gradient_norm == 3.0 && a->step_norm == 4.0 && a->predicted_reduction == 5.0);
        CHECK(!s.have_trial);   // (asking for the statistics does not make a trial point)
        CHECK(refused(s.commit(), s, "no trial point"));
        CHECK(s.ask_trial(&a) == kOk && a && a->trial_sumsq == 18.0 && s.have_trial);
        CHECK(cost_from_sumsq(a->trial_sumsq) == 0.5 * sqrt(18.0) * sqrt(18.0));
        CHECK(s.commit() == kOk && s.cur == 1 && !s.have_step && !s.have_trial);
        // commit twice; and the step is gone with it
        CHECK(refused(s.commit(), s, "no trial point") && s.cur == 1);
        CHECK(refused(s.ask_stats(&a), s, "no step computed"));
        CHECK(refused(s.ask_trial(&a), s, "no step computed"));
    }
    {   // the same without posted answers: the caller computes, then says the trial point is written
        StepState s;
        solve_plain(s);
        CHECK(s.ask_stats(&a) == kOk && a == nullptr);
        CHECK(s.ask_trial(&a) == kOk && a == nullptr && !s.have_trial);
        s.trial_written();
        CHECK(s.commit() == kOk && s.cur == 1);
        solve_plain(s);
        CHECK(s.ask_trial(&a) == kOk && a == nullptr);
        s.trial_written();
        CHECK(s.commit() == kOk && s.cur == 0);   // (and back)
    }
    {   // solve -> eval -> discard: the current set stays, step and trial point are gone
        StepState s;
        solve_posting(s, kA);
        CHECK(refused(s.begin_discard(), s, "no trial point"));   // (not evaluated yet)
        CHECK(s.ask_trial(&a) == kOk && a);
        CHECK(s.begin_discard() == kOk && s.have_trial);
        CHECK(s.finish_discard() == kOk && s.cur == 0 && !s.have_step && !s.have_trial);
        CHECK(refused(s.begin_discard(), s, "no trial point"));
        CHECK(refused(s.ask_stats(&a), s, "no step computed"));
    }
    {   // a second solve voids the first solve's trial point and its answers
        StepState s;
        solve_posting(s, kA);
        CHECK(s.ask_trial(&a) == kOk && a && s.have_trial);
        solve_plain(s);   // solve k + 1 posts nothing
        CHECK(!s.have_trial && !s.answered());
        CHECK(refused(s.commit(), s, "no trial point") && s.cur == 0);
        CHECK(s.ask_stats(&a) == kOk && a == nullptr);   // answers posted for solve k are not served for solve k + 1
        CHECK(s.ask_trial(&a) == kOk && a == nullptr && !s.have_trial);
        s.trial_written();
        CHECK(s.commit() == kOk && s.cur == 1);
        // ... and when solve k + 1 posts its own, those are served
        solve_posting(s, kA);
        solve_posting(s, kB);
        CHECK(s.ask_stats(&a) == kOk && a && a->gradient_norm == 6.0);
        CHECK(s.ask_trial(&a) == kOk && a && a->trial_sumsq == 50.0);
    }
    {   // answers posted, then a solve that fails behind them (begin_solve, no step): nothing is served
        StepState s;
        solve_posting(s, kA);
        s.begin_solve();
        CHECK(refused(s.ask_stats(&a), s, "no step computed"));
        s.step_computed();
        CHECK(s.ask_stats(&a) == kOk && a == nullptr);
    }
    {   // invalidate after eval refuses commit and discard
        StepState s;
        solve_posting(s, kA);
        CHECK(s.ask_trial(&a) == kOk && s.have_trial);
        s.invalidate();
        CHECK(refused(s.commit(), s, "no trial point") && s.cur == 0);
        CHECK(refused(s.begin_discard(), s, "no trial point"));
        CHECK(refused(s.ask_stats(&a), s, "no step computed"));
        CHECK(refused(s.ask_trial(&a), s, "no step computed"));
    }
    {   // invalidate_step drops the step alone: a trial point already written can still be committed
        StepState s;
        solve_posting(s, kA);
        CHECK(s.ask_trial(&a) == kOk);
        s.invalidate_step();
        CHECK(refused(s.ask_stats(&a), s, "no step computed") && s.have_trial);
        CHECK(s.commit() == kOk && s.cur == 1);
    }
    printf("ok %d\n", n_checks);
    return 0;
}
