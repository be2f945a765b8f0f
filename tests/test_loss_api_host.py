"""The robust-loss entries of the C ABI and of apex_solver_amd.pose_graph that need no device: apexgpu_loss_evaluate against
tests/np_ref_loss.py, parameter validation, create_loss_function's names / aliases / defaults / error, and the
loss | huber_delta exclusion of PoseGraphProblem."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import apex_solver_amd as pkg
import np_ref_loss as nl
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import Loss, PoseGraphProblem, create_loss_function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_INPUT = -5


def evaluate(kind, p0, p1, s):
    out = (C.c_double * 6)()
    rc = capi.load().apexgpu_loss_evaluate(kind, p0, p1, s, C.byref(out))
    return rc, np.array(out[:])


DEFAULTS = [("l2", capi.LOSS_L2, 0.0, 0.0), ("l1", capi.LOSS_L1, 0.0, 0.0), ("huber", capi.LOSS_HUBER, 1.345, 0.0),
            ("cauchy", capi.LOSS_CAUCHY, 2.3849, 0.0), ("fair", capi.LOSS_FAIR, 1.3999, 0.0), ("welsch", capi.LOSS_WELSCH, 2.9846, 0.0),
            ("tukey", capi.LOSS_TUKEY, 4.6851, 0.0), ("geman", capi.LOSS_GEMAN_MCCLURE, 1.0, 0.0),
            ("gemanmcclure", capi.LOSS_GEMAN_MCCLURE, 1.0, 0.0), ("andrews", capi.LOSS_ANDREWS, 1.339, 0.0),
            ("ramsay", capi.LOSS_RAMSAY, 0.3, 0.0), ("trimmed", capi.LOSS_TRIMMED_MEAN, 2.0, 0.0),
            ("trimmedmean", capi.LOSS_TRIMMED_MEAN, 2.0, 0.0), ("lp", capi.LOSS_LP_NORM, 1.5, 0.0),
            ("barron0", capi.LOSS_BARRON, 0.0, 1.0), ("barron1", capi.LOSS_BARRON, 1.0, 1.0), ("barron-2", capi.LOSS_BARRON, -2.0, 1.0),
            ("t-distribution", capi.LOSS_T_DISTRIBUTION, 5.0, 0.0), ("tdistribution", capi.LOSS_T_DISTRIBUTION, 5.0, 0.0),
            ("adaptive-barron", capi.LOSS_BARRON, 0.0, 1.0), ("adaptivebarron", capi.LOSS_BARRON, 0.0, 1.0)]


@pytest.mark.parametrize("name,kind,p0,p1", DEFAULTS)
def test_create_loss_function_defaults_and_library_values(name, kind, p0, p1):
    loss = create_loss_function(name)
    assert (loss.kind, loss.p0, loss.p1) == (kind, p0, p1)
    assert create_loss_function(name.upper()) == loss   # to_lowercase (pose_graph_g2o.rs:260)
    for s in (0.0, 1e-20, 0.37, 4.0, 30.0, 1e4):
        rc, out = evaluate(loss.kind, loss.p0, loss.p1, s)
        ref = nl.six(loss, s)
        assert rc == 0 and np.all(np.abs(out.astype(nl.LD) - ref) <= 1e-13 * np.maximum(1.0, np.abs(ref))), (name, s, out, ref)
        assert np.array_equal(loss.evaluate(s), out)


def test_create_loss_function_scale_goes_where_the_reference_puts_it():
    assert create_loss_function("cauchy", 0.7) == Loss(capi.LOSS_CAUCHY, 0.7, 0.0)
    assert create_loss_function("lp", 3.0) == Loss(capi.LOSS_LP_NORM, 3.0, 0.0)                     # the scale is p
    assert create_loss_function("t-distribution", 4.0) == Loss(capi.LOSS_T_DISTRIBUTION, 4.0, 0.0)   # the scale is nu
    assert create_loss_function("barron-2", 0.5) == Loss(capi.LOSS_BARRON, -2.0, 0.5)
    assert create_loss_function("adaptive-barron", 2.0) == Loss(capi.LOSS_BARRON, 0.0, 2.0)
    assert create_loss_function("l1", 9.0) == Loss(capi.LOSS_L1)                                     # l2 / l1 ignore it
    with pytest.raises(capi.LinAlgError) as e:
        create_loss_function("tukey", -1.0)
    assert e.value.code == INVALID_INPUT


def test_create_loss_function_unknown_name_has_the_reference_message():
    with pytest.raises(ValueError) as e:
        create_loss_function("Hubber")
    assert str(e.value) == ("Unknown loss function: Hubber. Valid options: l2, l1, huber, cauchy, fair, welsch, tukey, geman, andrews, "
                            "ramsay, trimmed, lp, barron0, barron1, barron-2, t-distribution, adaptive-barron")


def test_invalid_parameters_and_unknown_kinds():
    for kind in range(capi.LOSS_HUBER, capi.LOSS_T_DISTRIBUTION + 1):
        if kind == capi.LOSS_BARRON:
            continue
        for bad in (0.0, -1.0):
            assert evaluate(kind, bad, 1.0, 1.0)[0] == INVALID_INPUT, kind
    assert evaluate(capi.LOSS_BARRON, 1.0, 0.0, 1.0)[0] == INVALID_INPUT and evaluate(capi.LOSS_BARRON, 1.0, -1.0, 1.0)[0] == INVALID_INPUT
    assert evaluate(capi.LOSS_BARRON, -50.0, 1.0, 1.0)[0] == 0    # alpha is unrestricted
    assert evaluate(15, 1.0, 1.0, 1.0)[0] == INVALID_INPUT and evaluate(-1, 1.0, 1.0, 1.0)[0] == INVALID_INPUT
    assert capi.load().apexgpu_loss_evaluate(capi.LOSS_L2, 0.0, 0.0, 1.0, None) == INVALID_INPUT
    rc, out = evaluate(capi.LOSS_NONE, 0.0, 0.0, 3.0)
    assert rc == 0 and list(out) == [3.0, 1.0, 0.0, 1.0, 1.0, 0.0]


def test_problem_takes_a_loss_or_a_huber_delta_not_both():
    d = pkg.synthetic.make_sphere(3, 4)
    with pytest.raises(ValueError):
        PoseGraphProblem(d, loss=create_loss_function("cauchy"), huber_delta=1.0)
    with pytest.raises(ValueError):
        PoseGraphProblem.pose_graph(d, 1.0, create_loss_function("cauchy"))
    assert PoseGraphProblem.pose_graph(d, loss=create_loss_function("cauchy")).loss.kind == capi.LOSS_CAUCHY
    assert PoseGraphProblem.pose_graph(d, 1.0).loss is None


def test_header_symbols_and_constants_agree():
    with open(os.path.join(ROOT, "include", "apexgpu.h")) as f:
        h = f.read()
    for sym in ("apexgpu_pg_set_loss", "apexgpu_pg_get_loss", "apexgpu_loss_evaluate"):
        assert sym in capi.SYMBOLS and re.search(r"\b%s\(" % sym, h) and hasattr(capi.load(), sym)
    for value, name in enumerate(capi.LOSS_KINDS):
        assert re.search(r"#define APEXGPU_LOSS_%s %d\b" % (name, value), h), name
        assert getattr(capi, "LOSS_" + name) == value
