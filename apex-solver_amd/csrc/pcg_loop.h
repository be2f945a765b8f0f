// pcg_loop.h -- the host loop of both device PCG variants, once: the scalars of an iteration are read ONE ITERATION BEHIND.
// Iteration k + 1 is enqueued on speculation before the host waits for the scalars of iteration k, so the device never idles
// through a host round trip; the termination tests are also made on the device, so an iteration enqueued behind a met test
// changes nothing, and x, the iteration count and every scalar are those of the loop that waited every time -- whatever the cap.
// No HIP here: TilePcg::solve (tile_pcg.hip) and SchurJacobiPcg::solve (schur_jacobi_pcg.h) give the device work as callables over
// a PcgReadback (pcg_readback.h), tests/host_harness_pcg_loop.cpp walks the loop on the host.
#pragma once

namespace apex {

// what the scalars of an iteration say.  kStopUncounted: the reference breaks before the iteration's update (p.Ap ~ 0: x was left
// untouched); kStopCounted: it breaks behind it (converged, or rz_old ~ 0)
enum class PcgVerdict { kGoOn, kStopCounted, kStopUncounted };

struct PcgLoopResult {
    int iterations;   // as the reference counts them
    int status;       // the first non-zero status of enqueue or wait (the loop ended there), else 0
};

// enqueue(slot) -> status: one iteration on the stream, its scalars posted to `slot` (0 / 1); wait(slot) -> status: until that
// post has arrived; verdict(slot): of the scalars in it.  The caller synchronises its stream afterwards (a speculative iteration
// may still be running).
template <typename Enqueue, typename Wait, typename Verdict>
PcgLoopResult pcg_loop_one_behind(int max_iter, Enqueue&& enqueue, Wait&& wait, Verdict&& verdict) {
    int it = 0, rc = 0;
    if (max_iter > 0 && (rc = enqueue(0)) != 0) return {it, rc};
    for (; it < max_iter; ++it) {
        if (it + 1 < max_iter && (rc = enqueue((it + 1) & 1)) != 0) return {it, rc};   // on speculation
        if ((rc = wait(it & 1)) != 0) return {it, rc};
        const PcgVerdict v = verdict(it & 1);
        if (v == PcgVerdict::kStopUncounted) break;
        if (v == PcgVerdict::kStopCounted) { ++it; break; }
    }
    return {it, 0};
}

}  // namespace apex
