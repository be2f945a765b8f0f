"""SE2 through the Python mirror without a GPU: the seeded Manhattan generator, the dataset registry, and no CPU fallback."""
import numpy as np
import pytest

import apex_solver_amd as pkg
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem


def test_make_manhattan_is_seeded_and_connected():
    a = pkg.synthetic.make_manhattan(3500); b = pkg.synthetic.make_manhattan(3500)
    for k in ("ids", "poses", "e_from", "e_to", "meas", "truth"):
        assert np.array_equal(getattr(a, k), getattr(b, k))
    assert (a.n_v, a.n_e) == (3500, 9378) and a.poses.shape == (3500, 3) and a.meas.shape == (9378, 3)   # the docstring's count
    assert a.manifold == "se2"
    assert np.array_equal(a.e_from[:3499], np.arange(3499)) and np.array_equal(a.e_to[:3499], np.arange(1, 3500))   # connected
    lc = a.e_to[3499:].astype(int) - a.e_from[3499:].astype(int)
    assert lc.size == 5879 and (lc >= 12).all()                                                            # loop closures
    assert np.bincount(a.e_to[3499:], minlength=3500).max() <= 2
    assert not np.array_equal(pkg.synthetic.make_manhattan(200, config_id=2).meas, pkg.synthetic.make_manhattan(200).meas)
    d = pkg.synthetic.make_manhattan(10000)
    assert (d.n_v, d.n_e) == (10000, 27281)
    # measurements are the true relative poses up to the noise
    import np_ref_se2 as ref
    r = ref.minus(ref.vec(ref.inv(ref.mat(a.truth[a.e_from])) @ ref.mat(a.truth[a.e_to])), a.meas)
    assert np.abs(r[:, :2]).max() < 0.15 and np.abs(r[:, 2]).max() < 0.08 and r.std() > 0.005


def test_datasets_fall_back_to_the_generator():
    for name in ("M3500", "intel", "mit", "ring"):
        assert pkg.datasets.G2O_FILES[name] == ("2d", name + ".g2o")
    d, kind, path = pkg.datasets.load_pose_graph("M3500")
    assert kind == "synthetic" and path is None and d.poses.shape == (3500, 3) and d.meas.shape[1] == 3
    d, kind, _ = pkg.datasets.load_pose_graph("intel")
    assert kind == "synthetic" and d.n_v == 1228


def test_problem_picks_the_manifold_from_the_width():
    d = pkg.synthetic.make_manhattan(30, id_stride=7)
    p = PoseGraphProblem.pose_graph(d)
    assert p.manifold == "se2" and p.total_dof == 90 and p.fix.shape == (30, 3) and p.fix[0].all() and p.fix[1:].sum() == 0
    assert sorted(p.pose_col.tolist()) == list(range(0, 90, 3))
    names = sorted(f"x{i}" for i in d.ids)
    assert [int(c) for c in p.pose_col] == [3 * names.index(f"x{i}") for i in d.ids]
    p.add_prior("x7", huber_delta=1.0)
    assert p.priors[0][0] == 1 and p.priors[0][1].shape == (3,)
    s = pkg.synthetic.make_sphere(3, 4)
    assert PoseGraphProblem.pose_graph(s).manifold == "se3" and PoseGraphProblem.pose_graph(s).total_dof == 72


def test_no_cpu_fallback_for_se2():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    d = pkg.synthetic.make_manhattan(30)
    with pytest.raises(pkg.capi.LinAlgError) as e:
        GpuSparseCholeskySolver(0).initialize_structure(PoseGraphProblem.pose_graph(d))
    assert e.value.kind == "DeviceError"
