"""Writes tests/golden/factor_schedule.json: the factorisation's launch sequence (apexgpu_debug_schedule_ops, host only) of
the structures of tests/test_schedule_host.py under four option sets, and of the banded 48-tile structure cut for 2 and 4
ranks.  Per case the SHA-256 of the launch / event-record / stream-wait rows of both phases; for three small structures the
rows themselves, so that a mismatch can name its first differing call.

The file pins the sequence ACROSS a change: record it with the library built from the commit BEFORE the change
(APEXGPU_LIB=<that build's libapexgpu.so> python tools/record_factor_schedule.py), never with the changed code.
tests/test_schedule_golden_host.py compares.  Usage: python tools/record_factor_schedule.py [output path]"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from apex_solver_amd import capi  # noqa: E402
import test_schedule_host as tsh  # noqa: E402

OPTION_SETS = {
    "defaults": {},
    "all_on": dict(two_side=2, overlap=1, split_u1=1, flood_gate=2, factor_flow=0),
    "all_on_flow": dict(two_side=2, overlap=1, split_u1=1, flood_gate=2, factor_flow=3, factor_flow_rows=64),
    "all_off": dict(two_side=0, overlap=0, split_u1=0, flood_gate=0, factor_flow=0),
}
ROWS_KEPT = ("advisor", "dense12", "chain+leaves")
ORDERING_OPS = (0, 1, 2)   # launch, event record, stream wait


def cases():
    """(id, structure name, present, keyword arguments of capi.schedule_ops)"""
    for name, p in tsh.structures():
        for oname, o in OPTION_SETS.items():
            yield f"{name}/{oname}", name, p, dict(o)
    nt = 48
    band = tsh.lower(nt, [(i, j) for i in range(nt) for j in range(max(0, i - 3), i)])
    for world in (2, 4):
        for rank in range(world):
            yield f"band48/world{world}/rank{rank}", "band48", band, dict(world=world, rank=rank)


def ordering_rows(present, **kw):
    """Per phase: the rows of the calls that order tile accesses (every other kind of call filtered out)."""
    out = []
    for phase in (0, 1):
        rows = capi.schedule_ops(present, phase=phase, **kw)
        out.append(rows[np.isin(rows[:, 0], ORDERING_OPS)])
    return out


def digest(phases):
    h = hashlib.sha256()
    for rows in phases:
        h.update(np.int64(len(rows)).tobytes())
        h.update(np.ascontiguousarray(rows, dtype="<i8").tobytes())
    return h.hexdigest()


def record():
    out = {}
    for cid, name, p, kw in cases():
        phases = ordering_rows(p, **kw)
        entry = {"sha256": digest(phases), "calls": [int(len(r)) for r in phases]}
        if name in ROWS_KEPT:
            entry["rows"] = [r.tolist() for r in phases]
        out[cid] = entry
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "factor_schedule.json")
    rec = record()
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in rec.items()) + "\n}\n")
    print(f"{len(rec)} cases -> {path} (library {capi.LIB_PATH})")
