"""Writes tests/golden/sinv_lists.json: per tile structure of tests/test_schedule_host.py (single rank, each once) the SHA-256
of the selected inversion's task and product rows (apexgpu_debug_sinv_lists, host only) and the three product counts.

The file pins the lists ACROSS a change: record it with a library built from the commit BEFORE the change
(APEXGPU_LIB=<that build's libapexgpu.so> python tools/record_sinv_lists.py), never with the changed code.  The commit
before the lists became a value (sinv_lists.cpp) had no host entry for them: the recording build was that commit plus a
scratch patch that ran its list builder on a host-only plan with stand-in addresses and dumped the same rows.
tests/test_sinv_lists_host.py compares.  Usage: python tools/record_sinv_lists.py [output path]"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from apex_solver_amd import capi  # noqa: E402
import test_schedule_host as tsh  # noqa: E402


def cases():
    return tsh.structures()


def entry(present):
    rows, counts = capi.sinv_lists(present)
    h = hashlib.sha256()
    h.update(np.int64(len(rows)).tobytes())
    h.update(np.ascontiguousarray(rows, dtype="<i8").tobytes())
    return {"sha256": h.hexdigest(), "rows": int(len(rows)), "products": [int(c) for c in counts[:3]]}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sinv_lists.json")
    rec = {name: entry(p) for name, p in cases()}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in rec.items()) + "\n}\n")
    print(f"{len(rec)} cases -> {path} (library {capi.LIB_PATH})")
