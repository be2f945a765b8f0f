"""The host lists behind the setters and exports of the two solvers, as host programs (g++, no GPU, no HIP) against loops written
out naively in each harness; once as it is and once under AddressSanitizer + UndefinedBehaviorSanitizer.

prior_lists (csrc/prior_lists.h, tests/host_harness_prior_lists.cpp): 4 owners with a non-identity map, 7 blocks -- three on one
owner in non-sorted caller order, two of them in a row, one owner with none -- at the widths and strides of every use (BA pose and
intrinsics, SE3 / SE2 / SO3 vertices): the stable order and the caller's slots, the CSR, the defaults -1 and 1, zero padding, the
caller's order kept when not sorted, n = 0, and the text of every refusal.
info_pack (csrc/info_pack.h, tests/host_harness_info_pack.cpp): D = 3 and 6, 3 edges: expand(pack(W)) == W, the packed row is the
upper triangle in row order at the shared stride; an infinity, a NaN, asymmetry at, just below and just above 1e-12 max|W| with
max|W| a power of two, a pivot that is exactly 0 and a negative one, each naming its edge and pivot.
hessian_csc (csrc/hessian_csc.cpp, tests/host_harness_hessian_csc.cpp): 3 cameras, 4 landmarks, 7 factors, nine and six columns,
intrinsics-first caller columns: a repeated factor, a camera seen only through a prior, a landmark never observed, an all-zero
factor; == against a dense J^T J + prior diagonal of small integers, the count-only call, sorted rows, colptr[total] == nnz.
landmark_cov_lists (csrc/landmark_cov_lists.h, tests/host_harness_landmark_cov_lists.cpp): counts 0, 1, small_k, small_k + 1, two
large landmarks of equal count in a stable order, the pair sum."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")

HARNESSES = {"prior_lists": [], "info_pack": [], "hessian_csc": [os.path.join(CSRC, "hessian_csc.cpp")], "landmark_cov_lists": []}


@pytest.mark.parametrize("flags", [["-O1", "-Werror"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
@pytest.mark.parametrize("name", sorted(HARNESSES))
def test_host_lists_against_naive_loops(name, flags, tmp_path):
    exe = str(tmp_path / ("host_harness_" + name))
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", CSRC,
                         os.path.join(ROOT, "tests", "host_harness_" + name + ".cpp"), *HARNESSES[name], "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
