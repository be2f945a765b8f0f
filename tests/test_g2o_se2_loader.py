"""SE2 content of G2O files through the library's reader (apexgpu_g2o_raw_se2 / apexgpu_g2o_problem_se2).  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import apex_solver_amd as pkg
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import G2oError, G2oLoader, write_g2o

MIXED = """# a comment
VERTEX_SE2 10 1.0 2.0 0.5
VERTEX_SE3:QUAT 3 0 0 0 0 0 0 1
VERTEX_SE2 2 -1.5 0.25 -3.0

VERTEX_SE2 100 4 5 3.5
EDGE_SE2 10 2 0.1 0.2 0.3 1 2 3 4 5 6
# another
EDGE_SE2 2 100 -0.1 -0.2 -0.3 10 0 0 20 0 30
EDGE_SE3:QUAT 3 3 0 0 0 0 0 0 1 1 0 0 0 0 0 1 0 0 0 0 1 0 0 0 1 0 0 1 0 1
FIX 2
"""


def test_mixed_file_keeps_the_se2_values(tmp_path):
    p = tmp_path / "mixed.g2o"; p.write_text(MIXED)
    g = G2oLoader.load(p)
    assert g.n_vertices_se2 == 3 and g.n_edges_se2 == 2 and g.vertex_count() == 4 and g.edge_count() == 3
    assert g.vertex_ids_se2.tolist() == [10, 2, 100]                                  # file order
    assert np.array_equal(g.poses_se2, [[1, 2, 0.5], [-1.5, 0.25, -3.0], [4, 5, 3.5]])
    assert g.edge_from_se2.tolist() == [10, 2] and g.edge_to_se2.tolist() == [2, 100]
    assert np.array_equal(g.edge_meas_se2, [[0.1, 0.2, 0.3], [-0.1, -0.2, -0.3]])
    assert np.array_equal(g.edge_info_se2[0], [[1, 2, 3], [2, 4, 5], [3, 5, 6]]) and np.array_equal(g.edge_info_se2[1], np.diag([10.0, 20, 30]))
    assert g.vertex_ids.tolist() == [3]                                               # the SE3 side answers as before
    d = g.to_problem_data(manifold="se2")
    assert d.ids.tolist() == [2, 10, 100] and np.array_equal(d.poses[0], [-1.5, 0.25, -3.0])
    assert d.e_from.tolist() == [1, 0] and d.e_to.tolist() == [0, 2]
    assert g.to_problem_data().manifold == "se3"                                      # mixed: SE3 stays the default
    # the C entry with every output: sorted-name columns x10 < x100 < x2, the first (sorted) vertex fixed
    L = capi.load(); h = C.c_void_p()
    assert L.apexgpu_g2o_open(str(p).encode(), C.byref(h)) == 0
    sid = np.zeros(3, np.int64); sp = np.zeros((3, 3)); ef = np.zeros(2, np.uint32); et = np.zeros(2, np.uint32); pm = np.zeros((2, 3))
    col = np.zeros(3, np.int64); fix = np.zeros((3, 3), np.uint8)
    assert L.apexgpu_g2o_problem_se2(h, capi.ptr(sid), capi.ptr(sp), capi.ptr(ef), capi.ptr(et), capi.ptr(pm), capi.ptr(col), capi.ptr(fix)) == 0
    L.apexgpu_g2o_close(h)
    assert sid.tolist() == [2, 10, 100] and col.tolist() == [6, 0, 3] and fix.tolist() == [[1, 1, 1], [0, 0, 0], [0, 0, 0]]
    out = np.zeros(3, np.int64)
    assert L.apexgpu_pose_graph_columns_se2(3, capi.ptr(np.array([2, 10, 100], np.int64)), capi.ptr(out)) == 0 and out.tolist() == [6, 0, 3]


def test_write_read_round_trip_is_exact(tmp_path):
    d = pkg.synthetic.make_manhattan(60, id_stride=3)
    p = tmp_path / "m60.g2o"
    write_g2o(p, d)
    txt = p.read_text()
    assert f"# SE2 vertices: 60, SE3 vertices: 0, SE2 edges: {d.n_e}, SE3 edges: 0" in txt and "VERTEX_SE2 3 " in txt
    g = G2oLoader.load(p)
    assert g.vertex_ids.size == 0 and g.n_vertices_se2 == 60 and g.n_edges_se2 == d.n_e
    q = g.to_problem_data()                                                           # SE2 only: the default is "se2"
    assert q.manifold == "se2"
    for k in ("ids", "poses", "e_from", "e_to", "meas"):
        assert np.array_equal(getattr(q, k), getattr(d, k)), k                        # 17 significant digits round-trip fp64
    assert np.array_equal(g.edge_info_se2, np.broadcast_to(np.eye(3), (d.n_e, 3, 3)))


def test_se3_only_file_has_empty_se2_arrays(tmp_path):
    d = pkg.synthetic.make_sphere(3, 4)
    p = tmp_path / "s.g2o"; write_g2o(p, d)
    g = G2oLoader.load(p)
    assert g.n_vertices_se2 == 0 and g.vertex_ids_se2.size == 0 and g.poses_se2.shape == (0, 3) and g.edge_meas_se2.shape == (0, 3)
    assert g.to_problem_data().manifold == "se3" and np.allclose(g.to_problem_data().poses, d.poses, rtol=0, atol=1e-15 * 50)   # (the reader renormalises quaternions)


@pytest.mark.parametrize("text,kind", [
    ("VERTEX_SE2 1 0 0\n", "MissingFields"), ("VERTEX_SE2 x 0 0 0\n", "InvalidNumber"), ("VERTEX_SE2 1 0 zz 0\n", "InvalidNumber"),
    ("VERTEX_SE2 1 0 0 0\nVERTEX_SE2 1 0 0 0\n", "DuplicateVertex"), ("EDGE_SE2 0 1 0 0 0 1 0 0 1 0\n", "MissingFields"),
    ("EDGE_SE2 0 1 0 0 q 1 0 0 1 0 1\n", "InvalidNumber"), ("EDGE_SE2 0 1 0 0 0 1 0 0 1 0 q\n", "Parse"),
])
def test_se2_error_cases(tmp_path, text, kind):
    p = tmp_path / "bad.g2o"; p.write_text(text)
    with pytest.raises(G2oError) as e:
        G2oLoader.load(p)
    assert e.value.kind == kind


def test_dangling_se2_edge_loads_and_fails_only_when_the_se2_problem_is_asked_for(tmp_path):
    """A file whose EDGE_SE2 names a vertex it does not hold loaded before SE2 values were kept (the lines were counted);
    it still does, SE3 content included, and the Parse error comes from to_problem_data(manifold="se2")."""
    p = tmp_path / "dangling.g2o"
    p.write_text("VERTEX_SE3:QUAT 3 0 0 0 0 0 0 1\nVERTEX_SE2 0 0 0 0\nEDGE_SE2 0 9 0 0 0 1 0 0 1 0 1\n")
    g = G2oLoader.load(p)
    assert g.n_vertices_se2 == 1 and g.n_edges_se2 == 1 and g.edge_to_se2.tolist() == [9]
    assert g.to_problem_data().ids.tolist() == [3]
    with pytest.raises(G2oError) as e:
        g.to_problem_data(manifold="se2")
    assert e.value.kind == "Parse"
