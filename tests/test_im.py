"""The InternalModel estimator behind BatchLinMPC on the CPU wave emulator (tests/emu/libmpcqp_emu_im.so: csrc/im_bodies.h under
the launcher of tests/emu/emu_im.cpp, next to the emulated controller kernels).  The runners and the NumPy restatement are
tests/im_util.py; tests/test_gpu_im.py runs the same checks on the MI355X.

Estimator quantities: δ = the largest difference between the two NumPy formulations (tables Ks, Ps against the
recurrence) on the test's own inputs, the bar 32 δ floored at 1e-13 max|quantity|.  Measured on the emulator, Ŷs error / δ /
bar per shape: a 1.8e-15 / 0 / 8.3e-13, b 2.0e-14 / 5.3e-15 / 3.1e-12, c 1.0e-14 / 7.1e-15 / 1.7e-12, d 5.7e-14 / 1.4e-14 /
7.8e-12, e 1.8e-15 / 2.0e-15 / 4.4e-13, f 1.6e-15 / 8.9e-16 / 2.8e-13; ŷs, x̂s, x̂d (δ = 0) at most 4.3e-14 against 9.5e-12
(DESIGN.md 4.13 has the MI355X table)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mpcqp
from mpcqp import api
from tests import emu_util, im_util as iu

pytestmark = pytest.mark.slow
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return mpcqp.api.load_library(iu.build())


def test_stock_emulator_refuses(tmp_path):
    """A library without the launcher (the stock emulator) answers MPCQP_ERR_UNSUPPORTED: no fallback."""
    code = ("import numpy as np, mpcqp\nfrom tests import emu_util\nlib = mpcqp.api.load_library(emu_util.build())\n"
            "m = mpcqp.BatchLinMPC(np.full((2,1,1),.5), np.ones((2,1,1)), np.ones((2,1,1)), Hp=3, Hc=1, lib=lib)\n"
            "try:\n    m.setinternalmodel()\nexcept mpcqp.MpcqpError as e:\n    print('refused', e)\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert "refused mpcqp error -4" in out.stdout, out.stdout + out.stderr


def test_known_answers_default_model(lib):
    iu.check_known_answers_default(iu.known_answers_default(lib))


def test_known_answers_tustin_model(lib):
    iu.check_known_answers_tustin(iu.known_answers_tustin(lib))


def test_known_answer_setmodel(lib):
    iu.check_known_answer_setmodel(iu.known_answer_setmodel(lib))


def test_disturbance_rejection_through_sim(lib):
    iu.check_disturbance_rejection(*iu.disturbance_rejection(lib))


@pytest.mark.parametrize("name", list(iu.SHAPES))
def test_estimator_quantities(lib, name):
    iu.check_estimator(name, iu.estimator_periods(name, lib))


def test_controller_parity_four_per_wavefront(lib, monkeypatch):
    """(the emulator runs the smallest shape, on both kernels that take it; the GPU twin all three shapes)"""
    monkeypatch.setenv("MPCQP_SMALL_Y", "1")
    iu.check_parity("four_per_wavefront", *iu.controller_parity("four_per_wavefront", lib, B=4, info=False), small=True)


def test_controller_parity_with_F_and_Yhat(lib):
    iu.check_parity("four_per_wavefront", *iu.controller_parity("four_per_wavefront", lib, B=4))


def test_zero_mismatch_is_bit_identical(lib):
    iu.check_zero_mismatch(iu.zero_mismatch(lib))


def test_loop_device_against_methods(lib):
    assert all(iu.loop_against_methods(lib, None))


def test_sim_against_methods(lib):
    iu.check_sim(*iu.sim_against_methods(lib))


def test_isolation(lib):
    iu.check_isolation(iu.isolation(lib))


def test_stale_model(lib):
    iu.check_stale(*iu.stale_model(lib))


def test_refusals(lib):
    iu.check_refusals(*iu.refusals(lib))
    assert iu.multi_refusal(lib) == -4


def test_python_validation(lib):
    iu.check_validation(iu.python_validation(lib))
