"""The SO3 surface that needs no device: the C entry's argument checks, the rotation-graph generator, the rotation part of a
G2O file.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import apex_solver_amd as pkg
import so3_ref as sr
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import G2oLoader, PoseGraphProblem, so3_as_vector, write_g2o


def test_create_so3_refuses_bad_arguments():
    L = capi.load()
    assert capi.MANIFOLD_SO3 == 2 and capi.MANIFOLD_SIZES[capi.MANIFOLD_SO3] == (4, 3)
    # out == NULL is refused before any device is asked for: INVALID_INPUT (-1 in include/apexgpu.h's numbering), not the
    # DEVICE error a machine without a GPU gives every other call
    invalid_input = L.apexgpu_pg_create_so3(4, 3, 0, None)
    assert invalid_input != 0 and invalid_input == L.apexgpu_pg_create_se2(4, 3, 0, None) == L.apexgpu_pg_create(4, 3, 0, None)
    h = C.c_void_p(1)
    rc = L.apexgpu_pg_create_so3(4, 3, -1, C.byref(h))                 # no such device
    assert rc != 0 and not h.value                                     # *out is cleared on failure
    rc = L.apexgpu_pg_create_so3(4, 3, 1 << 20, C.byref(h))
    assert rc != 0 and not h.value
    import torch
    if not torch.cuda.is_available():                                  # without a device the refusal is the device's, not the argument's
        assert rc != invalid_input
    with pytest.raises(ValueError):
        capi.PgHandle(4, 3, 0, manifold=7)


def test_problem_sizes_and_prior_data():
    d = pkg.synthetic.make_rotation_graph(30, 4, 0.05, 1)
    assert d.manifold == "so3"
    p = PoseGraphProblem(d, manifold="so3")
    assert (p.dof, p.ambient, p.total_dof) == (3, 4, 90) and p.fix.shape == (30, 3)
    assert np.array_equal(PoseGraphProblem(d).pose_col, p.pose_col)    # picked from the width as well
    p.add_prior("x3", huber_delta=1.0).add_prior("x4", data=[1.0, 0, 0, 0])
    assert p.priors[0][0] == 3 and np.array_equal(p.priors[0][1], so3_as_vector(d.poses[3])) and p.priors[1][1].shape == (4,)
    q = so3_as_vector(np.array([2.0, 0, 0, 0.5]))
    assert abs(q @ q - 1.0) < 4e-16
    with pytest.raises(ValueError):
        PoseGraphProblem(d, manifold="se2")
    with pytest.raises(ValueError):
        PoseGraphProblem(pkg.synthetic.make_manhattan(10), manifold="so3")
    g = PoseGraphProblem.pose_graph(d)
    assert g.fix[0].all() and not g.fix[1:].any()


@pytest.mark.parametrize("n_v,degree,window", [(200, 6, None), (500, 30, 40), (50, 4, None), (3, 2, None), (1, 4, None)])
def test_rotation_graph_properties(n_v, degree, window):
    d = pkg.synthetic.make_rotation_graph(n_v, degree, 0.05, 3, window=window)
    assert d.poses.shape == (n_v, 4) and d.meas.shape == (d.n_e, 4) and d.truth.shape == (n_v, 4)
    assert d.n_e == max(n_v - 1, int(round(n_v * degree / 2.0))) or n_v < 3
    for q in (d.poses, d.meas, d.truth):
        assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() < 4e-16 if len(q) else True
    assert (d.e_from != d.e_to).all() and (d.e_from < n_v).all() and (d.e_to < n_v).all()
    if window:
        assert (np.abs(d.e_to.astype(int) - d.e_from.astype(int)) <= window).all()
    # connected: the chain is there
    seen = np.zeros(n_v, bool); seen[0] = True
    for a, b in zip(d.e_from[:n_v - 1], d.e_to[:n_v - 1]):
        assert b == a + 1
        seen[b] = seen[a]
    assert seen.all()
    d2 = pkg.synthetic.make_rotation_graph(n_v, degree, 0.05, 3, window=window)
    assert np.array_equal(d.meas, d2.meas) and np.array_equal(d.poses, d2.poses)      # a pure function of its arguments


def test_rotation_graph_has_zero_cost_at_its_truth_without_noise():
    d = pkg.synthetic.make_rotation_graph(120, 6, 0.0, 5)
    assert np.array_equal(d.poses, d.truth)
    r, _ = sr.so3_between(d.truth[d.e_from], d.truth[d.e_to], d.meas)
    assert float(np.abs(r).max()) < 1e-15                              # (the measurements are rounded to fp64)
    n = pkg.synthetic.make_rotation_graph(120, 6, 0.05, 5)
    rn, _ = sr.so3_between(n.truth[n.e_from], n.truth[n.e_to], n.meas)
    s = float(np.sqrt((rn * rn).mean()))
    assert 0.04 < s < 0.06                                             # Exp(N(0, sigma^2 I)) on the measurements


def test_g2o_rotation_part(tmp_path):
    d = pkg.synthetic.make_sphere(4, 5, id_stride=3)
    rng = np.random.default_rng(0)
    info = np.zeros((d.n_e, 6, 6))
    for e in range(d.n_e):
        A = rng.standard_normal((6, 6)); info[e] = A @ A.T + 6 * np.eye(6)
    path = tmp_path / "s.g2o"
    write_g2o(path, d, information=info)
    g = G2oLoader.load(path)
    se3 = g.to_problem_data(use_information=True)
    so3 = g.to_problem_data(manifold="so3", use_information=True)
    assert so3.manifold == "so3" and np.array_equal(so3.ids, se3.ids)
    assert np.array_equal(so3.poses, se3.poses[:, 3:7]) and np.array_equal(so3.meas, se3.meas[:, 3:7])     # [qw, qx, qy, qz]
    assert np.array_equal(so3.e_from, se3.e_from) and np.array_equal(so3.e_to, se3.e_to)
    assert np.array_equal(so3.information, se3.information[:, 3:, 3:]) and so3.information.flags["C_CONTIGUOUS"]
    assert g.to_problem_data(manifold="so3").information is None
    p = PoseGraphProblem.pose_graph(so3)
    assert p.manifold == "so3" and p.information.shape == (d.n_e, 3, 3)
    with pytest.raises(ValueError):
        g.to_problem_data(manifold="so2")


def test_rotation_part_of_a_file_without_se3_content_is_refused(tmp_path):
    path = tmp_path / "m.g2o"
    write_g2o(path, pkg.synthetic.make_manhattan(12))
    g = G2oLoader.load(path)
    assert g.to_problem_data().manifold == "se2"
    with pytest.raises(ValueError, match="no SE3 content"):
        g.to_problem_data(manifold="so3")
