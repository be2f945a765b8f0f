"""tests/np_ref_loss.py pinned by the assertions of the reference's own unit tests (src/core/loss_functions.rs:1606-2020,
src/core/corrector.rs:308-404), restated as data rows in tests/golden/loss_kat.json.  No GPU, no library."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import np_ref_loss as nl
from apex_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "loss_kat.json")) as f:
    KAT = json.load(f)["rows"]
OUT = {"rho": 0, "rho1": 1, "rho2": 2, "sqrt_rho1": 3, "residual_scaling": 4, "alpha_sq_norm": 5}


def make(name, p):
    p = list(p) + [0.0, 0.0]
    return SimpleNamespace(kind=capi.LOSS_KINDS.index(name), p0=p[0], p1=p[1])


def value(loss, s, out):
    return float(nl.six(loss, s)[OUT[out]])


@pytest.mark.parametrize("k", range(len(KAT)), ids=lambda k: f"{KAT[k]['test']}-{k}")
def test_reference_assertion(k):
    row = KAT[k]
    loss, s, op = make(row["loss"], row["p"]), row["s"], row["op"]
    if op in ("err", "ok"):
        assert nl.valid(loss) == (op == "ok")
        return
    assert nl.valid(loss)
    x = value(loss, s, row["out"])
    if op == "eq": assert x == row["v"]
    elif op == "near": assert abs(x - row["v"]) < row["tol"]
    elif op == "abslt": assert abs(x) < row["v"]
    elif op == "gt": assert x > row["v"]
    elif op == "lt": assert x < row["v"]
    elif op == "in": assert row["v"][0] < x < row["v"][1]
    elif op == "finite": assert np.isfinite(x)
    elif op == "lt_at": assert x < value(loss, row["s2"], row["out"])
    elif op == "lt_loss": assert x < value(make(*row["other"]), s, row["out"])
    elif op in ("num_d1", "num_d2"):
        h = row["h"]
        rp, r0, rm = (float(nl.evaluate(loss, t)[0]) for t in (s + h, s, s - h))
        num = (rp - rm) / (2 * h) if op == "num_d1" else (rp - 2 * r0 + rm) / (h * h)
        assert abs(x - num) < row["tol"]
    else:
        raise AssertionError(f"unknown op {op}")


def test_every_reference_test_is_covered():
    names = {r["test"] for r in KAT}
    assert len(names) >= 22 and {"test_corrector_cauchy", "test_lp_norm_loss", "test_new_loss_constructor_validation"} <= names


def test_correct_second_arm_is_the_literal_formula():
    """corrector.rs:241-253 on the reference's own example shape (2 x 3), with Lp(3) so that rho'' > 0."""
    loss = make("LP_NORM", [3.0])
    r = np.array([2.0, 1.0]); J = np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    rt, Jt, arm, s = nl.correct(r, J, loss)
    assert arm == 2 and s == 5.0
    rho1, rho2 = 1.5 * np.sqrt(5.0), 0.75 / np.sqrt(5.0)
    alpha = 1 - np.sqrt(1 + 2 * 5.0 * rho2 / rho1)
    assert np.allclose(np.asarray(rt, float), np.sqrt(rho1) / (1 - alpha) * r, rtol=1e-15)
    assert np.allclose(np.asarray(Jt, float), np.sqrt(rho1) * (J - (alpha / 5.0) * np.outer(r, r) @ J), rtol=1e-14)
    # the identity behind the device's normal-equation form: J~^T J~ = rho' (J^T J - a (2 - a s) w w^T), w = J^T r
    a = alpha / 5.0
    w = J.T @ r
    assert np.allclose(np.asarray(Jt.T @ Jt, float), rho1 * (J.T @ J - a * (2 - a * 5.0) * np.outer(w, w)), rtol=1e-13)
    assert np.allclose(np.asarray(Jt.T @ rt, float), np.sqrt(rho1) * (np.sqrt(rho1) / (1 - alpha)) * (1 - a * 5.0) * w, rtol=1e-13)
