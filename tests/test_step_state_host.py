"""StepState (csrc/step_state.h), the state of the trial-step protocol both solvers run through TileBackend, as a host program
(tests/host_harness_step_state.cpp, g++, no GPU): wrong-state calls and their texts, solve -> stats -> eval -> commit,
solve -> eval -> discard, commit twice, a second solve voiding the first one's trial point and answers, invalidate."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")


def test_step_state_transitions(tmp_path):
    exe = str(tmp_path / "host_harness_step_state")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CSRC,
                         os.path.join(ROOT, "tests", "host_harness_step_state.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
