"""RankExchange (apex-solver_amd/csrc/rank_exchange.cpp) WITHOUT a GPU: a host build over the shared-memory transport
(tests/rank_exchange_host_harness.cpp, g++, -DAPEX_COMM_HOST_ONLY), like tests/test_comm_host.py for the transport itself.
  * a RankExchange with no communicator, a sharded one with none, and one at world 1 return kOk from every call and leave
    the buffers' bytes untouched;
  * worlds of 2 and 3 real processes issue ONE ExchangeList of four items -- a sum of 5 doubles to every rank, a sum of 3
    doubles to root 1, a sum of 0 doubles, a max over 2 ints --, rank r contributing r + 1 in every slot: the sums are 3 and
    6, the rooted sum is checked on its root, the max is the world.
Not tested: a call made after the peers have gone.  The transport's only bounded wait is the barrier's 120 s, so the case
would hold the suite for two minutes."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")


@pytest.fixture(scope="module")
def lib_path():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "librank_exchange_host.so")
    src = os.path.join(ROOT, "tests", "rank_exchange_host_harness.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("rank_exchange.cpp", "rank_exchange.h", "comm.cpp", "comm.h", "lm_loop.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-DAPEX_COMM_HOST_ONLY", "-shared", "-fPIC", "-pthread", src, "-o", so, "-lrt"], check=True)
    return so


def test_inactive_exchange_touches_nothing(lib_path):
    L = C.CDLL(lib_path)
    L.rank_exchange_idle_selftest.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    msg = C.create_string_buffer(512)
    rc = L.rank_exchange_idle_selftest(f"pytest-{os.getpid()}-rx-solo".encode(), msg, 512)
    assert rc == 0 and msg.value == b"idle ok", msg.value.decode()


WORKER = """
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
L.rank_exchange_list_selftest.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
msg = C.create_string_buffer(512)
rc = L.rank_exchange_list_selftest(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4].encode(), msg, 512)
print(msg.value.decode())
sys.exit(rc)
"""


@pytest.mark.parametrize("world, total", [(2, 3), (3, 6)])
def test_one_list_between_processes(lib_path, world, total):
    name = f"pytest-{os.getpid()}-rx-w{world}"
    procs = [subprocess.Popen([sys.executable, "-c", WORKER, lib_path, str(world), str(r), name],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for r, p in enumerate(procs):
        o, _ = p.communicate(timeout=180)
        outs.append((r, p.returncode, o.strip()))
    assert all(rc == 0 for _, rc, _ in outs), outs
    assert [o for _, _, o in outs] == [f"rank {r} of {world} ok: sum {total} max {world}" for r in range(world)], outs
