"""The one guarded entry path of the C ABI (csrc/capi_guard.h: guarded(), with_handle(), HandleOwner) as a host program
(tests/host_harness_capi_guard.cpp, g++, no GPU, no HIP) over a fake handle type.  Exactly: a null handle and a handle with a null
solver answer APEXGPU_ERR_INVALID_STATE and the body does not run (a counter); a body's status code comes back as it is, for
every code of include/apexgpu.h; a body that throws std::bad_alloc, std::length_error or std::runtime_error answers
APEXGPU_ERR_INVALID_INPUT and one that throws an int APEXGPU_ERR_INVALID_STATE; a const handle takes the same path; a solver
constructor that throws inside create gives the same codes, no handle and no leak.  Once as it is and once under
AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O1", "-Werror"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_guard_and_handle_helper_on_a_fake_handle(flags, tmp_path):
    exe = str(tmp_path / "host_harness_capi_guard")
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", CSRC,
                         os.path.join(ROOT, "tests", "host_harness_capi_guard.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
