"""pcg_loop_one_behind (csrc/pcg_loop.h), the host loop both device PCG variants run -- scalars read one iteration behind, the next
iteration enqueued on speculation -- as a host program (tests/host_harness_pcg_loop.cpp, g++, no GPU, no HIP) over scripted
callables that record every call: the exact call sequence for caps 0, 1, 2, 5; a counted and an uncounted stop at every
iteration of caps 1..6 (count, and exactly one speculative enqueue beyond the stop when the cap allows one); a status from
enqueue or from wait at the first, a middle and a speculative position ends the loop with it and nothing is called behind it.
Once as it is and once under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O1", "-Werror"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_pcg_loop_call_sequence(flags, tmp_path):
    exe = str(tmp_path / "host_harness_pcg_loop")
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", CSRC,
                         os.path.join(ROOT, "tests", "host_harness_pcg_loop.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
