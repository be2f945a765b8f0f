"""The covariance surface that needs no GPU: the LM option, the result field, the per-camera split of the blocks."""
import numpy as np

from apex_solver_amd.solver import LevenbergMarquardtConfig, SolverResult, camera_covariance_dict


def test_config_flag_defaults_off_and_builder_sets_it():
    c = LevenbergMarquardtConfig.new()
    assert c.compute_covariances is False
    on = c.with_compute_covariances(True)
    assert on.compute_covariances is True and c.compute_covariances is False
    # the flag is a Python-side switch: the C config the loop receives is unchanged
    assert bytes(on.to_c()) == bytes(c.to_c())


def test_result_field_is_last_and_defaults_to_none():
    names = list(SolverResult.__dataclass_fields__)
    assert names[-1] == "covariances"
    assert SolverResult.__dataclass_fields__["covariances"].default is None


def test_camera_covariance_dict_split():
    b = np.arange(2 * 81, dtype=np.float64).reshape(2, 9, 9)
    d = camera_covariance_dict(b)
    assert set(d) == {"pose_0000", "intr_0000", "pose_0001", "intr_0001"}
    assert np.array_equal(d["pose_0001"], b[1, :6, :6]) and np.array_equal(d["intr_0000"], b[0, 6:, 6:])
