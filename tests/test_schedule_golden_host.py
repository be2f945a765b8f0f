"""The factorisation's launch sequence pinned call by call (no GPU).  tests/golden/factor_schedule.json holds, per tile
structure and option set, the SHA-256 of the launch / event-record / stream-wait rows of apexgpu_debug_schedule_ops, recorded
by tools/record_factor_schedule.py with the library of the commit BEFORE the schedule became a value (factor_schedule.cpp):
the list that TilePlan::issue plays back is the sequence that enqueue_factor used to issue.  A change of the chain shows here
as a schedule diff; re-record only from a commit whose sequence is the wanted one."""
import importlib.util
import json
import os

import numpy as np

import apex_solver_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_factor_schedule", os.path.join(ROOT, "tools", "record_factor_schedule.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

LAUNCH, RECORD, WAIT, GATE, CLEAR_GATES, CLEAR_VERSIONS = range(6)
MAIN, SIDE, SIDE2 = 0, 1, 2
N_EVENTS, EV_T = 5, 0


def test_every_recorded_sequence_is_reproduced():
    with open(os.path.join(ROOT, "tests", "golden", "factor_schedule.json")) as f:
        golden = json.load(f)
    seen = []
    for cid, name, p, kw in rec.cases():
        phases = rec.ordering_rows(p, **kw)
        g = golden[cid]
        for ph, want in enumerate(g.get("rows", [])):   # name the first differing call where the rows are kept
            got = phases[ph].tolist()
            for i, (a, b) in enumerate(zip(got, want)):
                assert a == b, f"{cid} phase {ph}: call {i} is {a}, recorded {b} (op, stream, event, list, first, count)"
            assert len(got) == len(want), f"{cid} phase {ph}: {len(got)} calls, recorded {len(want)}"
        assert [len(r) for r in phases] == g["calls"], (cid, [len(r) for r in phases], g["calls"])
        assert rec.digest(phases) == g["sha256"], cid
        seen.append(cid)
    assert sorted(seen) == sorted(golden) and len(seen) == 4 * len(rec.tsh.structures()) + 6


def test_gates_and_counter_clears_are_in_the_list_exactly_where_the_device_needs_them():
    """What the race check passes over but the device needs.  flood_gate = 2 (every U2 batch of two tasks or more that goes to
    a side stream is gated): the arrival counters are cleared first; a level group that hands U2 to the side stream (that
    stream waits for the group's panel solves) gates that stream, and the second side stream where it takes the bulk, on the
    NEXT group's potrf -- counter = that group, expected arrivals = its diagonal tiles -- unless it is the last group with
    level launches.  A dataflow launch has the clear of its version counters directly in front of it.  flood_gate = 0: no gate,
    no clear of arrival counters."""
    n_gates = 0
    for name, p in rec.tsh.structures():
        for oname in ("all_on", "all_on_flow"):
            rows = pkg.capi.schedule_ops(p, **rec.OPTION_SETS[oname])
            potrf = rows[(rows[:, 0] == LAUNCH) & (rows[:, 3] == 0)]   # one per level group with level launches, in order
            n_groups = len(potrf)
            levels = pkg.capi.check_schedule(p, **rec.OPTION_SETS[oname])["levels"]
            assert rows[0].tolist() == [CLEAR_GATES, MAIN, 0, -1, 0, levels + 1], (name, oname, rows[0])
            assert (rows[:, 0] == CLEAR_GATES).sum() == 1
            want = []
            for r in rows[(rows[:, 0] == WAIT) & (rows[:, 2] % N_EVENTS == EV_T) & np.isin(rows[:, 1], (SIDE, SIDE2))]:
                lv = int(r[2]) // N_EVENTS
                if lv + 1 < n_groups:
                    want.append([GATE, int(r[1]), 0, -1, lv + 1, int(potrf[lv + 1, 5])])
            got = rows[rows[:, 0] == GATE].tolist()
            assert sorted(got) == sorted(want), (name, oname, got, want)
            n_gates += len(got)
            for i in np.nonzero(rows[:, 0] == GATE)[0]:   # the stream's previous call is its wait for the group's panel solves
                prev = rows[:i][rows[:i, 1] == rows[i, 1]][-1]
                assert prev.tolist() == [WAIT, rows[i, 1], (int(rows[i, 4]) - 1) * N_EVENTS + EV_T, -1, 0, 0], (name, oname, int(i), prev)
            flow = np.nonzero((rows[:, 0] == LAUNCH) & (rows[:, 3] == 3))[0]
            clears = np.nonzero(rows[:, 0] == CLEAR_VERSIONS)[0]
            assert len(flow) == len(clears) <= 1 and (oname == "all_on_flow" or len(flow) == 0)
            for i in flow:
                assert rows[i - 1].tolist() == [CLEAR_VERSIONS, MAIN, 0, -1, int(rows[i, 4]), int(rows[i, 5])] and i == len(rows) - 1
        rows = pkg.capi.schedule_ops(p, **rec.OPTION_SETS["all_off"])
        assert (rows[:, 0] <= WAIT).all(), (name, rows[rows[:, 0] > WAIT])
    assert n_gates >= 20, n_gates
