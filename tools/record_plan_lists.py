"""Writes tests/golden/plan_lists.json: the tile plan's structure and task lists (apexgpu_debug_plan_lists, host only) of the
cases of tools/record_factor_schedule.py -- the structures of tests/test_schedule_host.py under four option sets, and the
banded 48-tile structure for 2 and 4 ranks, every rank -- and of a dissected band that those rank counts do cut.  Per case and table the SHA-256 of its rows; for the advisor's
structure the rows themselves, so that a mismatch can name its first differing record.

The file pins the lists ACROSS a change: record it with the library built from the commit BEFORE the change
(APEXGPU_LIB=<that build's libapexgpu.so> python tools/record_plan_lists.py), never with the changed code.
tests/test_plan_lists_golden_host.py compares.  Usage: python tools/record_plan_lists.py [output path]"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from apex_solver_amd import capi  # noqa: E402
import record_factor_schedule as rfs  # noqa: E402

ROWS_KEPT = ("advisor",)
TABLES = tuple(name for name, _ in capi.PLAN_TABLES)
tsh = rfs.tsh


def nd_band(nt, bw, leaf):
    """A banded structure in a nested-dissection order (separators of bw tiles last): a tree that a distributed plan cuts."""
    order = []

    def dissect(lo, hi):
        if hi - lo <= leaf:
            order.extend(range(lo, hi)); return
        mid = lo + (hi - lo - bw) // 2
        dissect(lo, mid); dissect(mid + bw, hi)
        order.extend(range(mid, mid + bw))

    dissect(0, nt)
    perm = np.empty(nt, dtype=int); perm[order] = np.arange(nt)
    return tsh.lower(nt, [(perm[i], perm[j]) for i in range(nt) for j in range(max(0, i - bw), i)])


def cases():
    """The cases of record_factor_schedule.py (the banded 48 is a chain: no rank count cuts it), and a dissected band of 60
    tiles that IS cut -- local groups, shared top groups, one forward launch per top column -- for 2 and 3 ranks, every rank."""
    yield from rfs.cases()
    p = nd_band(60, 3, 8)
    for world in (2, 3):
        for rank in range(world):
            yield f"ndband60/world{world}/rank{rank}", "ndband60", p, dict(world=world, rank=rank)


def tables(present, **kw):
    """Every table of one case, by name."""
    return {t: capi.plan_lists(present, t, **kw) for t in TABLES}


def digest(rows):
    h = hashlib.sha256()
    h.update(np.array(rows.shape, dtype="<i8").tobytes())
    h.update(np.ascontiguousarray(rows, dtype="<i8").tobytes())
    return h.hexdigest()


def record():
    out = {}
    for cid, name, p, kw in cases():
        tabs = tables(p, **kw)
        entry = {"sha256": {t: digest(r) for t, r in tabs.items()}, "rows": {t: int(len(r)) for t, r in tabs.items()}}
        if name in ROWS_KEPT:
            entry["kept"] = {t: r.tolist() for t, r in tabs.items()}
        out[cid] = entry
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "plan_lists.json")
    rec = record()
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in rec.items()) + "\n}\n")
    print(f"{len(rec)} cases -> {path} (library {capi.LIB_PATH})")
