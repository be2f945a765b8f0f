"""The tile plan's structure and task lists pinned record by record (no GPU).  tests/golden/plan_lists.json holds, per tile
structure, option set and table of apexgpu_debug_plan_lists (slot map, partition, level table, update rounds, every task
list, the dataflow units, the first-writer flags, the scalars), the SHA-256 of the rows.  It was recorded by
tools/record_plan_lists.py with the library of the commit BEFORE the lists became a value (plan_lists.cpp) plus the export
function alone, written there against TilePlan's fields: the lists build_plan_lists returns are the lists TilePlan's member
functions used to leave in them.  A reordering inside an update round changes the bits of every factorisation and shows here.
Never re-record with the code under test; only from a commit whose lists are the wanted ones."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_plan_lists", os.path.join(ROOT, "tools", "record_plan_lists.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


def test_every_recorded_table_is_reproduced():
    with open(os.path.join(ROOT, "tests", "golden", "plan_lists.json")) as f:
        golden = json.load(f)
    seen = []
    for cid, name, p, kw in rec.cases():
        tabs = rec.tables(p, **kw)
        g = golden[cid]
        assert sorted(g["sha256"]) == sorted(rec.TABLES), cid
        for t, want in g.get("kept", {}).items():   # name the first differing record where the rows are kept
            got = tabs[t].tolist()
            for i, (a, b) in enumerate(zip(got, want)):
                assert a == b, f"{cid} table {t}: record {i} is {a}, recorded {b}"
            assert len(got) == len(want), f"{cid} table {t}: {len(got)} records, recorded {len(want)}"
        for t in rec.TABLES:
            assert len(tabs[t]) == g["rows"][t], (cid, t, len(tabs[t]), g["rows"][t])
            assert rec.digest(tabs[t]) == g["sha256"][t], (cid, t)
        seen.append(cid)
    assert sorted(seen) == sorted(golden) and len(seen) == 4 * len(rec.tsh.structures()) + 6 + 5


def test_the_tables_are_not_trivially_empty():
    """What the digests cover: across the cases there are update rounds with conflicts, flagged first writers, dataflow units
    of both kinds, a cut forward sweep and fill tiles -- an export that returned nothing would pass no digest, but it should
    also not be possible to record one."""
    flagged = units = cuts = rounds = 0
    for cid, name, p, kw in rec.cases():
        if name not in ("advisor", "random0", "ndband60"):
            continue
        flagged += int(rec.capi.plan_lists(p, "upd", **kw)[:, 2].sum())
        units += len(rec.capi.plan_lists(p, "units", **kw))
        cuts += len(rec.capi.plan_lists(p, "fwd_cut", **kw))
        rounds += len(rec.capi.plan_lists(p, "upd_rounds", **kw))
    assert flagged > 0 and units > 0 and cuts > 0 and rounds > 0, (flagged, units, cuts, rounds)
