"""Stage-separable weight blocks, MPCQP_FLAG_WARM_DUAL and MPCQP_FLAG_KEEP_QP on the stage-structured MultipleShooting
kernel on the GPU (k_ms_step / _w: everything in LDS; k_ms_step_g / _gw: horizon-long data in HBM, products on the matrix
cores).  The shapes are chosen for the code path, not for the workload.  The emulator runs of the same code are in
tests/test_ms_options.py."""
import numpy as np
import pytest

from mpcqp import synth
from tests import ms_options_util as mou
from tests.parity_util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
KEEP_TOL = mou.KEEP_TOL
# Mean iterations per period from the second period on, C3 shapes under MultipleShooting: measured on the CPU emulator
# (the same algorithm, deterministic) on the first 48 members of this batch: plain start 10.86, MPCQP_FLAG_WARM_DUAL 9.70
# -- a gain of 1.16 (period by period +0.83, -1.75, -1.48, -2.23).  Half of it is asserted.  The figure of the 512
# controllers on the GPU has not been measured yet.
WARM_GAIN = 0.58


@pytest.mark.parametrize("custom", [False, True])
def test_weight_blocks_closed_loop_in_lds(hiplib, custom):
    """The block-weight closed loop of the emulator test at B = 64: the LDS placement, k_ms_step / k_ms_step_w."""
    r = mou.blocks_closed_loop(B=64, which="MNL", custom=custom)
    assert r["worst"] <= TOL, r
    assert r["defect"] <= 1e-9, r


def test_beyond_the_lds_with_every_option_on_gpu(hiplib):
    """SingleShooting 12,4,4,46,46 with M / N / L blocks, warm_dual, keep_qp and two soft custom rows at B = 64: the HBM
    placement (k_ms_step_gw), the matrix-core products with a dense R_t; every eighth member held to the oracle, the kept
    q~ / F of member 0."""
    r = mou.beyond_lds_with_everything(B=64, check=tuple(range(0, 64, 8)), periods=2)
    print(f"kept F / q~ error {r['keep']}")
    assert r["worst"] <= TOL, r
    assert max(r["keep"]) <= KEEP_TOL, r


def test_kept_qp_on_gpu(hiplib):
    """Kept q~ / F of the stage kernel on the GPU: SingleShooting beyond the LDS (k_ms_step_g) and the block-weight
    controller under MultipleShooting, without and with a measured disturbance (k_ms_step)."""
    a, b = mou.kept_qp_beyond_lds(), mou.kept_qp_with_blocks()
    c, moved, worst = mou.kept_qp_with_disturbance()
    print(f"kept F / q~ error beyond the LDS {a}, with blocks {b}, with a measured disturbance {c}")
    assert moved > 1e-2 and worst <= TOL, (moved, worst)
    assert max(a + b + c) <= KEEP_TOL, (a, b, c)


def test_unstable_plants_with_dual_warm_start_and_move_blocks(hiplib):
    """The unstable plants (eigenvalues 1.12, 1.05, Hp = Hc = 50, cond(H~) >= 1e8) under MultipleShooting with warm_dual and
    an N_Hc of SPD 2 x 2 blocks: three closed-loop periods, every member OPTIMAL, members 0, 4, 8, 12 against the oracle."""
    r = mou.unstable_plant_warm_blocks(B=16, check=(0, 4, 8, 12), periods=3)
    assert r["worst"] <= TOL, r
    assert r["defect"] <= 1e-9, r


def test_dual_warm_start_saves_iterations_on_the_stage_kernel(hiplib):
    """MPCQP_FLAG_WARM_DUAL in a noisy closed loop under MultipleShooting (C3, 512 controllers, 5 periods): the same optimum
    as the plain start at every period, in fewer iterations from the second period on."""
    cfg = synth.C3
    bt = synth.make_batch(cfg, 512, seed=6)
    res = mou.closed_loop_pair_ms(cfg, bt, 5, warm_dual=True)
    nDU = cfg.nu * cfg.Hc
    for Za, Zb, ita, itb, defect in res:
        assert rel_err(Zb, Za, nDU).max() <= TOL
    plain = np.mean([r[2].mean() for r in res[1:]])
    warm = np.mean([r[3].mean() for r in res[1:]])
    print(f"mean iterations from period 2 on: plain {plain:.3f}, warm {warm:.3f}")
    assert warm <= plain - WARM_GAIN, (plain, warm)


def test_fused_loop_with_dual_warm_start_on_gpu(hiplib):
    """mpcqp_loop_device equals the three separate entry points bit for bit with MPCQP_FLAG_WARM_DUAL on the stage kernel."""
    diff, used = mou.fused_loop_warm_dual(torch_device="cuda:0")
    assert diff == 0.0
    assert used
