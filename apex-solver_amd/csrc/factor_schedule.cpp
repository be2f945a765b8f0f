// factor_schedule.cpp -- see factor_schedule.h.  Plain C++: compiles without a HIP include path.
#include "factor_schedule.h"

#include <algorithm>

namespace apex {

// The factorisation is a static launch sequence for a given structure: it is captured once into a hipGraph (a few hundred
// dependent launches would otherwise be paced by host launch overhead) and replayed every iteration.
std::vector<SchedOp> factor_schedule(const ScheduleInput& in, int g0, int g1) {
    // Three streams.  Main: potrf(lv), panel solves(lv), U1d(lv) = the updates of the next level's DIAGONAL tiles (all
    // its potrf needs).  Third: U1o(lv) = the updates of the other tiles of the next level's columns, beside that
    // potrf; the next panel solves wait for them.  Side: U2(lv) = every other update of level lv, overlapped with
    // potrf / panel solves of level lv+1 (one workgroup resp. a few dozen: they leave the chip nearly empty).
    // Ordering that keeps every tile's read-modify-write sequence race free:
    //   U2(lv) after the panel solves of lv;  U1d(lv), U1o(lv) after U2a(lv-1) -- the part of U2(lv-1) whose targets lie in
    //   the columns of level lv+1, and with it (side-stream order) every older side-stream update; U2b(lv-1), targets in
    //   level lv+2 and above, runs on beside them (round 3: the wait for the whole of U2(lv-1) had become the critical chain
    //   once the flood gate let the potrf start on time);
    //   potrf(lv) after U1d(lv-1) [stream order] and whatever U1d(lv-1) waited for;
    //   panel(lv) after U1o(lv-1) [event];  U1o(lv) and U2(lv) hit different columns (level lv+1 / above);
    //   a U2 too small for the side stream runs on the main stream after the side stream's last U2b [kEvB].
    const std::vector<Level>& lv_ = in.lv;
    std::vector<SchedOp> ops;
    auto launch = [&](StreamId s, int list, int64_t first, int64_t n, int arrive = -1) {
        if (n > 0) ops.push_back({kOpLaunch, (uintptr_t)s, 0, list, first, (int)n, arrive});
    };
    auto wait = [&](StreamId s, int lv, LevelEvent k) { ops.push_back({kOpWait, (uintptr_t)s, (uintptr_t)lv * kLevelEvents + k, -1, 0, 0, -1}); };
    auto record = [&](int lv, LevelEvent k, StreamId s) { ops.push_back({kOpRecord, (uintptr_t)s, (uintptr_t)lv * kLevelEvents + k, -1, 0, 0, -1}); };
    auto potrf = [&](int lv) { launch(kMain, 0, lv_[lv].potrf, lv_[lv + 1].potrf - lv_[lv].potrf, in.gate_min > 0 ? lv : -1); };
    auto panel = [&](int lv) { launch(kMain, 1, lv_[lv].panel, lv_[lv + 1].panel - lv_[lv].panel); };   // (the panel solves multiply by Linv)
    auto updates = [&](int r0, int r1, StreamId s) {   // update rounds [r0, r1), one launch each
        for (int r = r0; r < r1; ++r) launch(s, 2, in.upd_rounds[r].first, in.upd_rounds[r].second);
    };
    // the stream stalls until the potrf workgroups of level lv+1 have announced themselves
    auto gate = [&](int lv, StreamId s) { ops.push_back({kOpGate, (uintptr_t)s, 0, -1, lv + 1, lv_[lv + 2].potrf - lv_[lv + 1].potrf, -1}); };
    const bool two = in.overlap && in.n_levels > 2;
    // the trailing groups [gf, g1) of this phase run as one dataflow launch behind the level launches (build())
    const int ph = (g0 == in.n_local_groups && g1 == in.n_levels && in.n_local_groups < in.n_levels) ? 1 : 0;
    const ScheduleInput::Flow& flow = in.flow[ph];
    const int g_end = g1;
    if (in.flow_on && flow.n > 0 && flow.g0 >= g0 && flow.g1 == g1) g1 = flow.g0;
    if (in.gate_min > 0) ops.push_back({kOpClearGates, kMain, 0, -1, 0, in.n_levels + 1, -1});
    int last_a = -1, last_b = -1;   // last levels with work on the side streams A / B that the main stream has not waited for
    std::vector<int> lastb((size_t)std::max(g1 - g0, 1), -1);   // lastb[lv - g0]: the last level <= lv with U2b2 work on stream B
    bool u2_pending = false, o_pending = false;   // the previous level group put its U2a / U1o on a side stream (recorded kEvU2 / kEvO)
    int b2_pending = -1, a_waited = -1;
    auto a_wait_upto = [&](int lvb) {   // stream A waits for stream B up to level lvb's U2b2 (B runs in order)
        if (lvb > a_waited) { wait(kSide, lvb, kEvB2); a_waited = lvb; }
    };
    for (int lv = g0; lv < g1; ++lv) {
        potrf(lv);
        // the panel solves work on the off-diagonal tiles of this level's columns: U1o of the level below must be in
        if (lv > g0 && o_pending) wait(kMain, lv - 1, kEvO);
        const int r0 = lv_[lv].upd, rd = lv_[lv].u1o, rs = lv_[lv].u2a, r1 = lv_[lv + 1].upd;
        int64_t n_u2 = 0, n_o = 0;
        for (int r = rs; r < r1; ++r) n_u2 += in.upd_rounds[r].second;
        for (int r = rd; r < rs; ++r) n_o += in.upd_rounds[r].second;
        // a cross-stream edge costs a few microseconds in the graph: only worth it when the batch is a real one
        const bool has_u2 = two && n_u2 >= in.overlap_min;
        const bool has_o = two && in.split_u1 && n_o >= in.split_u1_min;
        panel(lv);
        if (has_u2 || has_o) record(lv, kEvT, kMain);
        if (has_u2) wait(kSide, lv, kEvT);
        if (has_o) wait(kSo, lv, kEvT);
        if (two && lv > g0 && u2_pending) {
            wait(kMain, lv - 1, kEvU2);
            if (has_o) wait(kSo, lv - 1, kEvU2);
        } else if (two && lv > g0 && !in.skip_idle_wait) {
            // Level lv-1 put nothing on the side streams, so there is no kEvU2 of lv-1 to carry "every older side-stream update
            // precedes U1(lv)": U2b1(lv-2) [targets in level lv+1, stream A] and the U2b2 of levels <= lv-3 [stream B] may
            // still be at work on the tiles U1(lv) is about to update (and that potrf(lv+1) then reads).  Levels are assigned
            // by height, so a chain can pass through such a level.  Wait for both side streams outright.
            if (last_a >= 0) {
                wait(kMain, last_a, kEvB);
                if (has_o) wait(kSo, last_a, kEvB);
                last_a = -1;
            }
            if (last_b >= 0) {
                wait(kMain, last_b, kEvB2);
                if (has_o) wait(kSo, last_b, kEvB2);
                last_b = -1;
            }
        }
        updates(r0, rd, kMain);   // U1d: what the next potrf needs
        updates(rd, rs, has_o ? kSo : kMain);   // U1o: what the next panel solves need, beside the next potrf
        o_pending = has_o;
        if (has_o) record(lv, kEvO, kSo);
        // U2 on two streams of its own.  A (side): U2a(lv) [targets in level lv+2: what U1(lv+1) waits for], then U2b1(lv)
        // [level lv+3].  B (second side): U2b2(lv) [level lv+4 and above: the bulk].  Writers of one target level t, in time:
        // U2b2(<= t-4) -> U2b1(t-3) -> U2a(t-2) -> U1(t-1); B orders the first among themselves, U2b1(lv) waits for
        // U2b2(lv-1) [kEvB2], the rest is stream order on A and kEvU2.  U2a(lv+1) thus waits for U2b1(lv) only, not for the
        // bulk of level lv (on one stream it did, and through it U1d(lv+2) and the potrf behind it).
        // (only when there is such work: a stream that joins the capture must come back to it with an event)
        const bool b2_side = has_u2 && in.two_side_plan && r1 > lv_[lv].u2b2;
        // flood gate: the bulk updates of a big level start when the next level's potrf workgroups sit on their CUs (they
        // follow U1d on the main stream) -- otherwise the update's grid takes every CU first and the potrf, 124 KB of LDS per
        // workgroup, waits for it to drain
        const bool gated = has_u2 && in.gate_min > 0 && n_u2 >= in.gate_min && lv + 1 < g1;
        if (gated) gate(lv, kSide);
        // a small U2 stays on the main stream: earlier levels' U2b may still be at work on the same targets over there
        if (!has_u2 && r1 > rs) {
            if (last_a >= 0) { wait(kMain, last_a, kEvB); last_a = -1; }
            if (last_b >= 0) { wait(kMain, last_b, kEvB2); last_b = -1; }
        }
        const int ra = lv_[lv].u2b1, rb = lv_[lv].u2b2;
        const StreamId sa = has_u2 ? kSide : kMain, sb = b2_side ? kSide2 : sa;
        // U2a(lv) [level lv+2] follows every U2b2 of levels <= lv-2 [their targets start at level lv+2] ...
        if (has_u2 && lv - 2 >= g0) a_wait_upto(lastb[lv - 2 - g0]);
        updates(rs, ra, sa);   // U2a
        u2_pending = has_u2;
        if (has_u2) record(lv, kEvU2, kSide);   // ... and, in stream order, every earlier update on A
        if (b2_side) {
            wait(kSide2, lv, kEvT);
            if (gated) gate(lv, kSide2);
        }
        if (has_u2 && lv - 1 >= g0) a_wait_upto(lastb[lv - 1 - g0]);   // ... and U2b1(lv) [level lv+3] every U2b2 of levels <= lv-1
        updates(ra, rb, sa);   // U2b1
        updates(rb, r1, sb);   // U2b2
        if (has_u2) { record(lv, kEvB, kSide); last_a = lv; }
        if (b2_side) { record(lv, kEvB2, kSide2); last_b = lv; }
        lastb[lv - g0] = b2_pending = b2_side ? lv : b2_pending;
    }
    if (g1 > g0 && o_pending) wait(kMain, g1 - 1, kEvO);
    // join: the last side-stream work precedes whatever follows on the main stream
    if (last_a >= 0) wait(kMain, last_a, kEvB);
    if (last_b >= 0) wait(kMain, last_b, kEvB2);
    if (g1 < g_end) {   // every update the level launches add to the region's tiles is in: the joins above
        ops.push_back({kOpClearVersions, kMain, 0, -1, flow.first, flow.n, -1});
        launch(kMain, 3, flow.first, flow.n);
    }
    return ops;
}

int check_schedule(const std::vector<SchedOp>& ops, const std::vector<PotrfTask>& potrf, const std::vector<GemmTask>& panel,
                   const std::vector<GemmTask>& upd, const std::vector<FactorUnit>& units, std::string* first_violation) {
    // vector clocks over the streams that appear: clock[s] = how many launches of stream s happen before this point
    std::vector<uintptr_t> streams;
    auto sid = [&](uintptr_t s) { for (size_t i = 0; i < streams.size(); ++i) if (streams[i] == s) return (int)i; streams.push_back(s); return (int)streams.size() - 1; };
    auto orders = [](const SchedOp& o) { return o.op == kOpLaunch || o.op == kOpRecord || o.op == kOpWait; };   // (the rest touches no tile)
    for (const SchedOp& o : ops) if (orders(o)) (void)sid(o.stream);
    const int S = (int)streams.size();
    typedef std::vector<int> Clock;
    std::vector<Clock> now((size_t)S, Clock((size_t)S, 0));     // per stream: what precedes its next call
    std::vector<std::pair<uintptr_t, Clock>> events;             // last record of each event
    struct Access { int launch; bool write; };
    struct Launch { int stream, pos; Clock before; const SchedOp* op; };
    std::vector<Launch> launches;
    std::vector<std::pair<const double*, Access>> acc;
    int bad = 0;
    auto complain = [&](const std::string& m) { if (bad++ == 0 && first_violation) *first_violation = m; };
    auto describe = [&](const Launch& l) {
        static const char* const names[] = {"potrf", "panel solves", "updates", "dataflow launch"};
        return std::string(names[l.op->list]) + " [" + std::to_string(l.op->first) + ", +" + std::to_string(l.op->count) + ") on stream " + std::to_string(l.stream);
    };
    for (const SchedOp& o : ops) {
        if (!orders(o)) continue;
        const int s = sid(o.stream);
        if (o.op == kOpRecord) {
            bool found = false;
            for (auto& e : events) if (e.first == o.event) { e.second = now[(size_t)s]; found = true; }
            if (!found) events.push_back({o.event, now[(size_t)s]});
        } else if (o.op == kOpWait) {
            bool found = false;
            for (const auto& e : events)
                if (e.first == o.event) { for (int k = 0; k < S; ++k) now[(size_t)s][(size_t)k] = std::max(now[(size_t)s][(size_t)k], e.second[(size_t)k]); found = true; }
            if (!found) complain("a stream waits for an event that was never recorded");
        } else {
            const int li = (int)launches.size();
            launches.push_back({s, now[(size_t)s][(size_t)s] + 1, now[(size_t)s], &o});
            now[(size_t)s][(size_t)s] += 1;
            // the tiles the launch touches; inside one launch no tile may be written twice or read and written by two tasks
            std::vector<std::pair<const double*, int>> local;   // (tile, +1 write / 0 read) of this launch
            auto touch = [&](const double* t, bool w) { acc.push_back({t, {li, w}}); local.push_back({t, w ? 1 : 0}); };
            for (int64_t q = o.first; q < o.first + o.count; ++q) {
                if (o.list == 0) { touch(potrf[(size_t)q].A, true); touch(potrf[(size_t)q].Linv, true); }
                else if (o.list == 1) { touch(panel[(size_t)q].C, true); touch(panel[(size_t)q].B, false); }
                else if (o.list == 2) { touch(reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(upd[(size_t)q].C) & ~uintptr_t(7)), true); touch(upd[(size_t)q].A, false); touch(upd[(size_t)q].B, false); }
                else {   // the dataflow launch orders its own units (version counters): one writer of everything it touches
                    const FactorUnit& u = units[(size_t)q];
                    touch(u.C, true);
                    if ((u.kind & 15) == 0) touch(u.A, true);
                }
            }
            if (o.list != 3) {
                std::sort(local.begin(), local.end());
                for (size_t i = 0; i < local.size();) {
                    size_t j = i; int writes = 0;
                    while (j < local.size() && local[j].first == local[i].first) writes += local[j++].second;
                    if (writes >= 1 && j - i >= 2) { complain("two tasks of one launch touch a tile that one of them writes: " + describe(launches.back())); break; }
                    i = j;
                }
            }
        }
    }
    // every pair of launches on one tile with a writer among them must be ordered
    std::sort(acc.begin(), acc.end(), [](const std::pair<const double*, Access>& a, const std::pair<const double*, Access>& b) {
        return a.first != b.first ? a.first < b.first : a.second.launch < b.second.launch; });
    for (size_t i = 0; i < acc.size();) {
        size_t j = i;
        while (j < acc.size() && acc[j].first == acc[i].first) ++j;
        for (size_t a = i; a < j; ++a)
            for (size_t b = a + 1; b < j; ++b) {
                const Access &x = acc[a].second, &y = acc[b].second;
                if (x.launch == y.launch || (!x.write && !y.write)) continue;
                const Launch &lx = launches[(size_t)x.launch], &ly = launches[(size_t)y.launch];   // lx was issued first
                if (ly.before[(size_t)lx.stream] < lx.pos)
                    complain("unordered accesses to one tile: " + describe(lx) + " and " + describe(ly));
            }
        i = j;
    }
    return bad;
}

}  // namespace apex
