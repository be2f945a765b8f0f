"""The incident-edge lists of the row-owned SE2 assembly (apex-solver_amd/csrc/pg2_lists.h) and a host replay of the
kernel's loop over them (pg2_assemble_row, the body of k_pg2_assemble) against the dense J^T J.  No GPU needed."""
import numpy as np
import pytest

import apex_solver_amd as pkg
import np_ref_se2 as ref
from test_se2_device_math_host import load_harness


@pytest.fixture(scope="module")
def hh():
    return load_harness()


def lists(hh, n_v, ef, et):
    ef = np.ascontiguousarray(ef, dtype=np.uint32); et = np.ascontiguousarray(et, dtype=np.uint32)
    ptr = np.zeros(n_v + 1, np.int32); edge = np.zeros(max(2 * len(ef), 1), np.uint32)
    n = hh.hh2_lists(n_v, len(ef), ef, et, ptr, edge)
    return n, ptr, edge[:max(n, 0)]


def odd_graph():
    """duplicates (0-1 three times, both directions), a self-loop on 2, vertex 5 without edges, a hub"""
    ef = [0, 1, 0, 2, 3, 4, 4, 4, 6, 1]
    et = [1, 0, 1, 2, 4, 3, 0, 6, 4, 6]
    return 7, np.array(ef, np.uint32), np.array(et, np.uint32)


def test_lists_hold_every_edge_once_per_endpoint(hh):
    for n_v, ef, et in (odd_graph(), (lambda d: (d.n_v, d.e_from, d.e_to))(pkg.synthetic.make_manhattan(300))):
        n, ptr, edge = lists(hh, n_v, ef, et)
        loops = int((ef == et).sum())
        assert n == 2 * len(ef) - loops and ptr[0] == 0 and ptr[-1] == n and (np.diff(ptr) >= 0).all()
        for v in range(n_v):
            mine = edge[ptr[v]:ptr[v + 1]]
            want = np.nonzero((ef == v) | (et == v))[0]
            assert np.array_equal(mine, want)                 # ascending edge index, a self-loop once
    n_v, ef, et = odd_graph()
    n, ptr, edge = lists(hh, n_v, ef, et)
    assert ptr[6] - ptr[5] == 0                               # the vertex without edges
    assert hh.hh2_lists(3, 1, np.array([0], np.uint32), np.array([3], np.uint32), np.zeros(4, np.int32), np.zeros(2, np.uint32)) == -1
    assert lists(hh, 4, np.zeros(0, np.uint32), np.zeros(0, np.uint32))[0] == 0


@pytest.mark.parametrize("delta", [-1.0, 0.3])
def test_replay_of_the_kernel_loop_equals_dense_normal_equations(hh, delta):
    rng = np.random.default_rng(5)
    graphs = []
    n_v, ef, et = odd_graph()
    poses = rng.uniform(-2, 2, size=(n_v, 3)); meas = rng.uniform(-1, 1, size=(len(ef), 3))
    graphs.append((poses, ef, et, meas))
    d = pkg.synthetic.make_manhattan(120)
    graphs.append((d.poses, d.e_from, d.e_to, d.meas))
    for poses, ef, et, meas in graphs:
        n_v = len(poses); n = 3 * n_v
        H = np.zeros((n, n)); g = np.zeros(n); writes = np.zeros((n_v, n_v), np.int32); writer = np.full((n_v, n_v), -1, np.int32)
        ef = np.ascontiguousarray(ef, np.uint32); et = np.ascontiguousarray(et, np.uint32)
        assert hh.hh2_assemble_dense(n_v, len(ef), np.ascontiguousarray(poses), ef, et, np.ascontiguousarray(meas), delta, H, g, writes, writer) == 0
        p = ref.Problem(poses, ef, et, meas, 3 * np.arange(n_v), np.zeros((n_v, 3), np.uint8), delta if delta > 0 else None)
        Hd, gd = p.normal_equations()
        sc = max(1.0, np.abs(Hd).max())
        assert np.abs(np.tril(H) - np.tril(Hd)).max() < 1e-12 * sc and np.abs(g - gd).max() < 1e-12 * sc
        assert np.array_equal(np.triu(H, 1), np.zeros_like(H))            # nothing above the diagonal
        # the owner of every off-diagonal block is its larger vertex, one read-add-write per edge of the pair
        for v in range(n_v):
            for u in range(n_v):
                k = int((((ef == v) & (et == u)) | ((ef == u) & (et == v))).sum()) if u < v else 0
                assert writes[v, u] == k and (k == 0 or writer[v, u] == v)
