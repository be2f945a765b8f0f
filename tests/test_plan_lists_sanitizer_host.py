"""The host-only planning code (plan_lists.cpp, factor_schedule.cpp, sinv_lists.cpp) as a plain program under the host
compilers' AddressSanitizer + UndefinedBehaviorSanitizer (no GPU): tools/plan_lists_check.cpp builds structures, lists, the
selected inversion's lists and both phases' schedules for a dense, a tree-shaped, a banded (1, 2, 4 ranks), a distributed and
a refused structure and proves every schedule race free.  All of it is index arithmetic into nt x nt maps.  The include path
holds csrc alone: that the program compiles is the proof that these files need no device header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]


@pytest.mark.parametrize("compiler", ["g++", "/opt/rocm/llvm/bin/clang++"])
def test_plan_lists_check_is_clean_under_asan_and_ubsan(compiler, tmp_path):
    cxx = shutil.which(compiler)
    if cxx is None:
        pytest.skip(f"no {compiler} on this machine")
    exe = str(tmp_path / "plan_lists_check")
    srcs = [os.path.join(ROOT, "tools", "plan_lists_check.cpp")] + [os.path.join(CSRC, f + ".cpp") for f in ("plan_lists", "factor_schedule", "sinv_lists")]
    cc = subprocess.run([cxx, *FLAGS, "-I", CSRC, *srcs, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all clean" in run.stdout and "FAIL" not in run.stdout, (run.stdout[-3000:], run.stderr[-3000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
