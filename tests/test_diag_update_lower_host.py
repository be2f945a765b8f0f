"""The option "diag_update_lower" on the host (csrc/plan_lists.h, PlanOptions::diag_lower): it changes what the update kernels
compute inside a diagonal tile and nothing else -- the structure, the task lists, the dataflow units with their waits and
publishes, and the launch sequence of a plan are byte for byte the same with it on and off (tests/host_harness_diag_lower.cpp),
so the proof of factor_schedule.cpp covers both.  Also the count of diagonal-target updates against its closed form."""
import os
import subprocess

import numpy as np
import pytest

import tile_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("diag_lower") / "host_harness_diag_lower")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, os.path.join(ROOT, "tests", "host_harness_diag_lower.cpp"),
                         os.path.join(CSRC, "plan_lists.cpp"), os.path.join(CSRC, "factor_schedule.cpp"), "-pthread", "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]

    def run(pat, factor_flow):
        nt = pat.shape[0]
        pairs = [(I, J) for I in range(nt) for J in range(I) if pat[I, J]]
        p = subprocess.run([exe, str(nt), str(factor_flow)], input="".join(f"{a} {b}\n" for a, b in pairs), capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-500:], p.stderr[-500:])
        return [int(x) for x in p.stdout.split()[1:]]
    return run


CASES = {"dense6": lambda: tr.dense(6), "arrow4": lambda: tr.arrow(4), "band12": lambda: tr.band(12), "grid4x4": lambda: tr.grid(4, 4)}


@pytest.mark.parametrize("factor_flow", [0, 64, -1])
@pytest.mark.parametrize("name", list(CASES))
def test_lists_units_and_schedule_do_not_see_the_option(name, factor_flow, harness):
    pat = CASES[name]()
    units, upd, diag_level, diag_flow, ops = harness(pat, factor_flow)
    # a column with h tiles below its diagonal tile sends h updates into diagonal tiles (and h (h - 1) / 2 elsewhere)
    h = [len(rows) for rows in tr.symbolic_cols(pat)]
    assert upd == sum(x * (x + 1) // 2 for x in h)
    assert diag_level + diag_flow == sum(h), (diag_level, diag_flow, h)
    if factor_flow == 0:
        assert units == 0 and diag_flow == 0
    if factor_flow == 64 and pat.shape[0] > 2:
        assert units > 0 and diag_level == 0   # (every group fits: the whole factorisation is one dataflow launch)
    assert ops > 0
