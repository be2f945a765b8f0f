"""Edge information matrices through the host-only layers: write_g2o -> G2oLoader -> to_problem_data(use_information=True)
(apexgpu_g2o_problem_information), the Python defaults, and the symbol list.  No GPU needed."""
import numpy as np
import pytest

import apex_solver_amd as pkg
import info_graphs as ig
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import G2oLoader, PoseGraphProblem, write_g2o
from test_capi_symbols import header_symbols


@pytest.mark.parametrize("man", ["se3", "se2"])
def test_g2o_round_trip_keeps_the_information(man, tmp_path):
    d = ig.graph(man, 40)
    W = ig.information(d)
    path = tmp_path / "w.g2o"
    write_g2o(path, d, information=W)
    g = G2oLoader.load(path)
    raw = g.edge_info_se2 if man == "se2" else g.edge_information
    assert np.array_equal(raw, W)                       # {:.17e} round-trips every double
    p = g.to_problem_data(use_information=True)
    assert p.manifold == man and np.array_equal(p.information, W)
    assert np.array_equal(p.e_from, d.e_from) and np.array_equal(p.e_to, d.e_to)
    assert g.to_problem_data().information is None and g.to_problem_data(use_information=False).information is None
    prob = PoseGraphProblem.pose_graph(p)
    assert np.array_equal(prob.information, W)          # falls back to data.information
    other = 2.0 * W
    assert np.array_equal(PoseGraphProblem.pose_graph(p, information=other).information, other)
    assert PoseGraphProblem.pose_graph(d).information is None
    with pytest.raises(ValueError):
        PoseGraphProblem.pose_graph(d, information=W[:-1])


def test_unsorted_file_gives_the_matrices_in_problem_edge_order(tmp_path):
    """vertices out of id order, edges in an order of their own, SE3 and SE2 lines interleaved: the problem's edges are the
    file's edges in file order with endpoints as indices into the sorted ids, and the information follows the edges"""
    def up6(k):
        A = np.arange(36, dtype=np.float64).reshape(6, 6) * 0.01 * (k + 1)
        return A @ A.T + (k + 1) * np.eye(6)

    def up3(k):
        A = np.arange(9, dtype=np.float64).reshape(3, 3) * 0.1 * (k + 1)
        return A @ A.T + (k + 1) * np.eye(3)

    ids3, ids2 = [7, 2, 9, 4], [30, 10, 20]
    e3, e2 = [(9, 2), (2, 7), (4, 9), (7, 7)], [(20, 30), (10, 20), (30, 10)]
    lines = []
    for k in range(4):
        lines.append(f"VERTEX_SE3:QUAT {ids3[k]} {k} 0 0 0 0 0 1")
        if k < 3:
            lines.append(f"VERTEX_SE2 {ids2[k]} {k} 0 0.1")
    for k in range(4):
        W = up6(k)
        lines.append(f"EDGE_SE3:QUAT {e3[k][0]} {e3[k][1]} 1 0 0 0 0 0 1 " + " ".join(f"{W[i, j]:.17e}" for i in range(6) for j in range(i, 6)))
        if k < 3:
            W = up3(k)
            lines.append(f"EDGE_SE2 {e2[k][0]} {e2[k][1]} 1 0 0 " + " ".join(f"{W[i, j]:.17e}" for i in range(3) for j in range(i, 3)))
    path = tmp_path / "mixed.g2o"
    path.write_text("\n".join(lines) + "\n")
    g = G2oLoader.load(path)
    p3 = g.to_problem_data(manifold="se3", use_information=True)
    assert list(p3.ids) == sorted(ids3)
    assert [(int(p3.ids[a]), int(p3.ids[b])) for a, b in zip(p3.e_from, p3.e_to)] == e3
    assert p3.information.shape == (4, 6, 6)
    for k in range(4):
        assert np.array_equal(p3.information[k], up6(k))
    p2 = g.to_problem_data(manifold="se2", use_information=True)
    assert list(p2.ids) == sorted(ids2)
    assert [(int(p2.ids[a]), int(p2.ids[b])) for a, b in zip(p2.e_from, p2.e_to)] == e2
    for k in range(3):
        assert np.array_equal(p2.information[k], up3(k))
    L = capi.load()
    assert L.apexgpu_g2o_problem_information(None, 0, None) != 0


def test_symbols_cover_the_header():
    assert sorted(capi.SYMBOLS) == header_symbols()
    for name in ("apexgpu_pg_set_information", "apexgpu_pg_get_information", "apexgpu_g2o_problem_information"):
        assert name in capi.SYMBOLS and hasattr(capi.load(), name)


def test_pose_graph_data_defaults_to_no_information():
    d = pkg.synthetic.make_manhattan(30)
    assert d.information is None and PoseGraphProblem.pose_graph(d).information is None
