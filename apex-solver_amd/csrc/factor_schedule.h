// factor_schedule.h -- the launch sequence of one phase of the tile Cholesky as a value: built on the host from the plan's
// level table (factor_schedule), proven race free (check_schedule), then issued call by call (TilePlan::issue).  What is
// proven is what runs.  Host only: no HIP type here or in anything this file includes.
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "tile_tasks.h"

namespace apex {

// The schedule names its streams and events by id; only TilePlan::issue maps them to handles.  Events per level group:
// after its panel solves, its U2a, its U1o, its U2b (all of the side stream), its U2b2 (second side stream)
enum StreamId { kMain, kSide, kSide2, kSo };   // TilePlan's stream_, side_, side2_, so_
enum LevelEvent { kEvT, kEvU2, kEvO, kEvB, kEvB2, kLevelEvents };

// SchedOp::op.  The three calls that order tile accesses keep the values the schedule tests know; the rest is what the
// device needs beside them (check_schedule passes over it).
enum SchedKind {
    kOpLaunch = 0,          // a batch of tile tasks: `list`, [first, first + count)
    kOpRecord = 1,          // event record
    kOpWait = 2,            // stream waits for event
    kOpGate = 3,            // flood gate: the stream stalls until arrival counter `first` has reached `count` (or a time-out)
    kOpClearGates = 4,      // the arrival counters [0, count) := 0
    kOpClearVersions = 5,   // the version counters of the dataflow launch := 0 ([first, +count): the units of that launch)
};

// One call of the factorisation's launch sequence.
struct SchedOp {
    int op;             // SchedKind
    uintptr_t stream;   // the stream the call goes to (StreamId)
    uintptr_t event;    // record / wait: the event (level group * kLevelEvents + LevelEvent)
    int list;           // launch: 0 potrf, 1 panel solves, 2 updates, 3 the dataflow launch
    int64_t first;      // launch: first task (unit) of its list
    int count;          // ... and how many
    int arrive;         // potrf launch: the arrival counter its workgroups announce themselves on (-1: none)
};

// per level group: its first task in each list, the update rounds U1d [upd, u1o) | U1o | U2a | U2b1 | U2b2 [u2b2, next upd),
// the first forward task of each column that gets a launch of its own
struct Level { int potrf = 0, panel = 0, fwd = 0, upd = 0, u1o = 0, u2a = 0, u2b1 = 0, u2b2 = 0; std::vector<int> fwd_cut; };

// The read-only facts of a plan that decide its launch sequence.
struct ScheduleInput {
    const std::vector<Level>& lv;                                  // [n_levels + 1]
    const std::vector<std::pair<int64_t, int64_t>>& upd_rounds;    // per update round: first task, count
    int n_levels, n_local_groups;
    bool overlap; int overlap_min;
    bool split_u1; int split_u1_min;
    bool two_side_plan;
    int gate_min;
    bool skip_idle_wait;   // tests only: the round-3 schedule bug (no wait after a level without side-stream work)
    bool flow_on;          // the dataflow launches run (none once one has timed out)
    struct Flow { int g0, g1, first, n; } flow[2];   // per phase: the level groups inside its dataflow launch, its units
};

// The calls of the level groups [g0, g1), in issue order.  No empty launch is listed (the launchers skip them).
std::vector<SchedOp> factor_schedule(const ScheduleInput& in, int g0, int g1);

// Proves a sequence race free: stream order + event edges give a happens-before relation; every two launches that touch one
// tile, at least one of them writing it, must be ordered by it, and no two tasks of one launch may write one tile (or one
// read what another writes).  The task lists are the host copies the launches index.  Returns the number of violations
// (0 = proven) and describes the first.
int check_schedule(const std::vector<SchedOp>& ops, const std::vector<PotrfTask>& potrf, const std::vector<GemmTask>& panel,
                   const std::vector<GemmTask>& upd, const std::vector<FactorUnit>& units, std::string* first_violation);

}  // namespace apex
