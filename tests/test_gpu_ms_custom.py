"""Custom linear constraints on the stage-structured MultipleShooting kernel on the GPU (k_ms_step_w / k_ms_step_gw):
T9 at the reference's horizon, randomised families, a SingleShooting problem beyond the LDS of a CU, unstable plants and
the fused Kalman loop.  The emulator runs of the same code are in tests/test_ms_custom.py."""
import numpy as np
import pytest

from mpcqp import api
from tests import ms_custom_util as mcu

pytestmark = pytest.mark.gpu
TOL = 1e-5


def test_t9_at_the_reference_horizon_under_multiple_shooting(hiplib):
    """T9 at Hp = Hc = 50 with transcription=MultipleShooting: the reference's expected values
    (test/3_test_predictive_control.jl:466-495) and the condensed oracle; the returned X̂0 is the model rolled out from ΔU."""
    r = mcu.run_t9(B=2, Hp=50)
    assert all(w == 0 for w in r["whys"]) and all(k == api.KERNEL_MS for k in r["kinds"]), r
    assert r["worst"] <= TOL, r
    assert r["defect"] <= 1e-9 and r["xroll"] <= 1e-9, r


@pytest.mark.parametrize("seed", list(range(8)))
def test_random_custom_families_on_gpu(hiplib, seed):
    """Randomised families with custom rows under MultipleShooting (nd > 0 with a varying preview, ±Inf holes in Wmin /
    Wmax, soft / hard rows, move blocking): every member within TOL of the condensed oracle's certified optimum."""
    r = mcu.random_custom_family(seed, B=4)
    assert r["kind"] == api.KERNEL_MS and r["why"] == 0 and np.all(r["status"] == 0), r
    assert r["worst"] <= TOL, r
    assert r["defect"] <= 1e-9, r


def test_condensed_problem_beyond_the_lds_with_custom_rows(hiplib):
    """SingleShooting 12,4,4,46,46 (nZ̃ = 185, beyond the LDS of a CU) plus two soft custom rows, 256 controllers: the steps
    run on the stage-structured kernel (MPCQP_ERR_UNSUPPORTED before), all OPTIMAL, a subset held to the oracle."""
    r = mcu.beyond_lds_with_custom_rows(B=256, check=range(0, 256, 32))
    assert r["kind"] == api.KERNEL_MS and r["why"] == 0, r
    assert np.all(r["status"] == 0), r["status"]
    assert r["worst"] <= TOL, r


def test_unstable_plant_with_custom_rows_on_gpu(hiplib):
    """The unstable plants of test_multiple_shooting_unstable_plant_on_gpu (eigenvalues 1.12, 1.05, Hp = Hc = 50) with a
    hard and a soft custom row: the stage-structured kernel keeps its accuracy and its model defects at rounding."""
    r = mcu.unstable_plant_with_custom_rows(B=16, check=range(0, 16, 4))
    assert r["kind"] == api.KERNEL_MS and np.all(r["status"] == 0), r
    assert r["worst"] <= 1e-7, r
    assert r["defect"] <= 1e-11, r


def test_fused_loop_with_custom_rows_on_gpu(hiplib):
    """mpcqp_loop_device equals the three separate entry points bit for bit on a custom-row MultipleShooting handle."""
    assert mcu.fused_loop_custom(torch_device="cuda:0") == 0.0
