"""The InternalModel estimator behind BatchLinMPC on the MI355X: the checks of tests/test_im.py (runners and NumPy restatement:
tests/im_util.py) on the product library, with every shape of the estimator and of the controller parity.

Estimator quantities: δ = the largest difference between the two NumPy formulations (tables Ks, Ps against the recurrence) on
the test's own inputs; the bar is 32 δ floored at 1e-13 max|quantity|.  ŷs, x̂s and x̂d are the same expression in both
formulations (δ = 0: the floor decides), Ŷs is where they differ.  Every test prints error, δ and bar.  Measured on the
MI355X, Ŷs error / δ / bar, then the worst of ŷs, x̂s, x̂d against its bar:
    a  1.8e-15 / 0       / 8.3e-13;  1.8e-15 (bar 7.7e-13)      d  4.3e-14 / 1.4e-14 / 7.8e-12;  2.8e-14 (bar 9.5e-12)
    b  1.8e-14 / 5.3e-15 / 3.1e-12;  8.9e-15 (bar 1.6e-12)      e  2.2e-15 / 2.0e-15 / 4.4e-13;  2.7e-15 (bar 6.5e-13)
    c  8.0e-15 / 7.1e-15 / 1.7e-12;  2.0e-14 (bar 1.7e-12)      f  1.3e-15 / 8.9e-16 / 2.8e-13;  2.2e-15 (bar 8.4e-13)
(DESIGN.md 4.13 has the table.)"""
import numpy as np
import pytest

import mpcqp
from mpcqp import api
from tests import im_util as iu

pytestmark = pytest.mark.gpu


def test_known_answers_default_model(hiplib):
    iu.check_known_answers_default(iu.known_answers_default(None))


def test_known_answers_tustin_model(hiplib):
    iu.check_known_answers_tustin(iu.known_answers_tustin(None))


def test_known_answer_setmodel(hiplib):
    iu.check_known_answer_setmodel(iu.known_answer_setmodel(None))


def test_disturbance_rejection_through_sim(hiplib):
    iu.check_disturbance_rejection(*iu.disturbance_rejection(None))


@pytest.mark.parametrize("name", list(iu.SHAPES))
def test_estimator_quantities(hiplib, name):
    iu.check_estimator(name, iu.estimator_periods(name, None))


def test_controller_parity_four_per_wavefront(hiplib, monkeypatch):
    """nZ̃ = 7 with output bounds on k_step_small_y (MPCQP_SMALL_Y=1: at this batch size the handle's own specialisation would
    take the steps).  u and Z̃; F and Ŷ are outputs that move a step off this kernel (next test)."""
    monkeypatch.setenv("MPCQP_SMALL_Y", "1")
    iu.check_parity("four_per_wavefront", *iu.controller_parity("four_per_wavefront", None, B=9, info=False), small=True)


@pytest.mark.parametrize("name", ["c2_dims_c3_rows", "manifest_3_2_7"])
def test_controller_parity(hiplib, name):
    """The shapes of spec_manifest.txt that the build compiles ahead of time: u, Z̃, F and Ŷ against the oracle with
    B + Ŷs, and the same QPs through a plain handle with Ŷs as a measured-disturbance preview."""
    worst, share, kind = iu.controller_parity(name, None, B=6)
    iu.check_parity(name, worst, share, kind)
    assert kind == api.KERNEL_ONDEMAND, kind


def test_zero_mismatch_is_bit_identical(hiplib):
    iu.check_zero_mismatch(iu.zero_mismatch(None))


def test_loop_device_against_methods(hiplib):
    assert all(iu.loop_against_methods(None, "cuda"))


def test_sim_against_methods(hiplib):
    iu.check_sim(*iu.sim_against_methods(None))


def test_isolation(hiplib):
    iu.check_isolation(iu.isolation(None))


def test_stale_model(hiplib):
    iu.check_stale(*iu.stale_model(None))


def test_refusals(hiplib):
    iu.check_refusals(*iu.refusals(None))
    assert iu.multi_refusal(None) == -4


def test_python_validation(hiplib):
    iu.check_validation(iu.python_validation(None))
