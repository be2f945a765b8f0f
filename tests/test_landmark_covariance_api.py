"""The landmark covariance surface that needs no GPU: the LM option, the landmark naming, the C declarations."""
import os
import re

import numpy as np

from apex_solver_amd import capi
from apex_solver_amd.solver import LevenbergMarquardtConfig, landmark_covariance_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("apexgpu_landmark_covariance", "apexgpu_landmark_covariance_stats")


def test_config_flag_defaults_off_and_leaves_the_c_config_alone():
    c = LevenbergMarquardtConfig.new()
    assert c.compute_landmark_covariances is False
    on = c.with_compute_covariances(True).with_compute_landmark_covariances(True)
    assert on.compute_landmark_covariances is True and c.compute_landmark_covariances is False
    assert bytes(on.to_c()) == bytes(c.to_c())
    assert bytes(c.with_compute_landmark_covariances(True).to_c()) == bytes(c.to_c())


def test_landmark_covariance_dict_names_and_copies():
    b = np.arange(3 * 9, dtype=np.float64).reshape(3, 3, 3)
    d = landmark_covariance_dict(b)
    assert list(d) == ["pt_00000", "pt_00001", "pt_00002"]
    assert np.array_equal(d["pt_00002"], b[2])
    d["pt_00000"][0, 0] = -1.0
    assert b[0, 0, 0] == 0.0


def test_symbols_declared_and_loaded():
    with open(os.path.join(ROOT, "include", "apexgpu.h")) as f:
        hdr = f.read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in capi.SYMBOLS
    # the camera entry points at the landmark one instead of "not computed"
    cam = hdr[hdr.index("Marginal camera covariances"):hdr.index("int apexgpu_camera_covariance(")]
    assert "not\n * computed" not in cam and "apexgpu_landmark_covariance" in cam
