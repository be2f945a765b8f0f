"""ColumnMap (csrc/column_map.h), the permutation between the caller's global column order and the device's internal order, as a
host program (tests/host_harness_column_map.cpp, g++, no GPU, no HIP) against loops written out naively: 4 cameras in a
non-identity internal order with nine and with six columns and intrinsics-first caller columns, 5 landmarks with a non-identity
map, a pose graph of 4 vertices with six and three columns.  Exactly: scatter then gather is the identity on the internal vector;
the untouched columns of six-column cameras receive the given value and nothing else is written; col is injective and covers the
camera-side columns together with untouched; the block permutes of widths 3, 7, 9 and of byte masks round-trip; the host half of
the scaling holder permutes, writes 1.0 on the padding and refuses a zero, a negative, an infinite and a NaN entry without a
trace.  Once as it is and once under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O1", "-Werror"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_column_map_against_naive_loops(flags, tmp_path):
    exe = str(tmp_path / "host_harness_column_map")
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", CSRC,
                         os.path.join(ROOT, "tests", "host_harness_column_map.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
