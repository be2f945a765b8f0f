"""apexgpu_pg_covariance on an SE2 handle (needs a real MI355X: `pytest -m gpu`): the 3 x 3 diagonal blocks of the dense
inverse of apexgpu_pg_get_hessian(lambda), at the tolerance tests/test_gpu_covariance.py uses for SE3."""
import numpy as np
import pytest

import apex_solver_amd as pkg
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem

pytestmark = pytest.mark.gpu
TOL = {1e4: 1e-10, 1e-3: 1e-7}       # tests/test_gpu_covariance.py


def block_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("lam", [1e4, 1e-3])
def test_se2_marginal_covariances(lam, scaled):
    d = pkg.synthetic.make_manhattan(600, id_stride=3)
    prob = PoseGraphProblem.pose_graph(d)
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    s.set_parameters(d.poses)
    if scaled:
        s.apply_column_scaling(1.0 / (1.0 + s.compute_column_norms()))
    H, _ = s.get_hessian(lam)
    with pytest.raises(capi.LinAlgError) as e:      # an export since the last solve: no valid factor
        s.pose_covariance_blocks()
    assert e.value.kind == "InvalidState"
    s.solve_augmented_equation(lam)
    cov = s.pose_covariance_blocks()
    assert cov.shape == (d.n_v, 3, 3)
    Z = np.linalg.inv(H)
    errs = [block_err(cov[v], Z[prob.pose_col[v]:prob.pose_col[v] + 3, prob.pose_col[v]:prob.pose_col[v] + 3]) for v in range(d.n_v)]
    print(lam, scaled, "worst block error", max(errs))
    assert max(errs) <= TOL[lam]
    named = s.compute_covariances()
    assert named[f"x{int(d.ids[7])}"].shape == (3, 3) and np.array_equal(named[f"x{int(d.ids[7])}"], cov[7])
    s.get_hessian(lam)
    with pytest.raises(capi.LinAlgError) as e:
        s.pose_covariance_blocks()
    assert e.value.kind == "InvalidState"
    s.close()
