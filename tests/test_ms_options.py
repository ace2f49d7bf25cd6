"""Options of the condensed kernels on the stage-structured MultipleShooting kernel (csrc/ms_bodies.h), without a GPU:
stage-separable Hermitian weight blocks (M_Hp, N_Hc, L_Hp), MPCQP_FLAG_WARM_DUAL and MPCQP_FLAG_KEEP_QP -- the kernel body
on the CPU wave emulator against the condensed oracle (both transcriptions solve the same QP).  The GPU runs are in
tests/test_gpu_ms_options.py."""

import numpy as np
import pytest

from mpcqp import api, synth
from tests import emu_util
from tests import ms_options_util as mou
from tests.parity_util import rel_err

TOL = 1e-5
KEEP_TOL = mou.KEEP_TOL


@pytest.fixture(scope="module")
def emulib():
    return api.load_library(emu_util.build())


def test_the_blocks_move_the_optimum_on_the_oracle():
    """The block-weight case cannot pass on ignored off-diagonal entries: on the oracle the optimum with the blocks differs
    from the optimum with their diagonals alone by more than 1e-2 in every period, and the slack is in play."""
    assert min(mou.blocks_matter_on_the_oracle()) > 1e-2
    ref, _ = mou.blocks_oracle_loop("MNL")
    assert all(r["status"] == 0 for r in ref) and min(r["Z"][-1] for r in ref) > 1e-6


@pytest.mark.parametrize("which,custom", [("MNL", False), ("N", False), ("L", False), ("M", False), ("MNL", True)])
def test_weight_blocks_closed_loop_on_the_stage_kernel(emulib, which, custom):
    """M_Hp = kron(I, M), N_Hc = kron(I, N), L_Hp = kron(I, L) with full 2 x 2 blocks under MultipleShooting, move blocking
    [1, 2, 2] over Hp = 8, u / y bounds with the slack in play: three closed-loop periods on the stage kernel (no reason
    mask, no fallback warning) against the condensed oracle; each matrix alone (the host's classification); with a custom
    row on top (the kernels with custom rows)."""
    r = mou.blocks_closed_loop(lib=emulib, B=2, which=which, custom=custom)
    assert r["worst"] <= TOL, r
    assert r["defect"] <= 1e-9, r
    if which == "MNL" and not custom:
        assert min(r["eps"]) > 1e-6, r


def test_separable_output_weight_through_the_dense_setter(emulib):
    """A stage-separable M_Hp sent through mpcqp_set_dense_weights (a caller of the C-ABI may do that) takes the block path."""
    r = mou.blocks_closed_loop(lib=emulib, B=2, which="MNL", raw_M=True)
    assert r["worst"] <= TOL and r["defect"] <= 1e-9, r


@pytest.mark.parametrize("which", ["N", "L"])
def test_weights_that_couple_stages_stay_refused(emulib, which):
    """An N_Hc entry linking two moves, an L_Hp entry linking two steps of one move-blocking interval: reason mask 1, the
    fallback warning, and the condensed kernels' answer is the oracle's."""
    why, msg, worst = mou.coupled_weight_case(emulib, which)
    assert why == 1, why
    assert "reason mask 1:" in msg, msg
    assert worst <= TOL, worst


@pytest.mark.parametrize("which", ["N", "L"])
def test_a_block_that_is_not_symmetric_stays_refused(emulib, which):
    """A block-diagonal N_Hc / L_Hp with one block that is not symmetric in one member of the batch: reason mask 1 (the
    stage kernel reads the blocks as symmetric matrices); symmetric again, the handle is taken."""
    assert mou.asymmetric_block_mask(emulib, which) == (1, 0)


def test_dual_warm_start_on_the_stage_kernel(emulib):
    """MPCQP_FLAG_WARM_DUAL under MultipleShooting (the set-up of test_dual_warm_start_on_cpu_emulator): the next period
    starts around the previous row multipliers; same optimum as the plain start."""
    cfg = mou.WARM_CFG
    bt = synth.make_batch(cfg, 1, seed=2)
    for Za, Zb, ita, itb, defect in mou.closed_loop_pair_ms(cfg, bt, 3, lib=emulib, warm_dual=True):
        assert rel_err(Zb, Za, cfg.nu * cfg.Hc).max() <= 1e-6
        assert defect <= 1e-9


def test_fused_loop_with_dual_warm_start_on_the_emulator(emulib):
    """mpcqp_loop_device equals the three separate entry points bit for bit with MPCQP_FLAG_WARM_DUAL on the stage kernel."""
    diff, used = mou.fused_loop_warm_dual(lib=emulib)
    assert diff == 0.0
    assert used


@pytest.mark.parametrize("change", ["set_transcription", "row_group", "cold_start"])
def test_stored_multipliers_are_dropped_when_they_no_longer_apply(emulib, change):
    """After mpcqp_set_transcription, after a set_bounds that adds a row group, and on a handle that switches
    MPCQP_FLAG_COLD_START on, the next step is the plain start: bit for bit the step of a fresh handle."""
    fn = {"set_transcription": lambda g: g.hd.set_transcription(api.MULTIPLE_SHOOTING),
          "row_group": mou.add_output_lower_bounds,
          "cold_start": lambda g: g.hd.set_flags(g.hd.flags | api.FLAG_COLD_START)}[change]
    diff, same_iters, used = mou.warm_dual_validity(emulib, fn)
    assert diff == 0.0 and same_iters
    if change == "set_transcription":
        assert used         # (left alone, the stored multipliers do change the next step)


def test_kept_qp_on_the_stage_kernel_beyond_the_lds(emulib):
    """MPCQP_FLAG_KEEP_QP on a SingleShooting controller beyond the LDS (3,4,2,46,46: the stage kernel): F and q~ in the
    condensed layout against the oracle's."""
    eF, eq = mou.kept_qp_beyond_lds(lib=emulib)
    print(f"kept F error {eF:.3e}, q~ error {eq:.3e}")
    assert eF <= KEEP_TOL and eq <= KEEP_TOL, (eF, eq)


def test_kept_qp_with_weight_blocks_under_multiple_shooting(emulib):
    """The same under MultipleShooting with the M / N / L blocks and a non-zero R^u: the dense-L term of q~."""
    eF, eq = mou.kept_qp_with_blocks(lib=emulib)
    print(f"kept F error {eF:.3e}, q~ error {eq:.3e}")
    assert eF <= KEEP_TOL and eq <= KEEP_TOL, (eF, eq)


def test_kept_qp_with_a_measured_disturbance(emulib):
    """The same with a measured disturbance (nd = 1, D^ varying over the horizon): the D^d D^0 term of F and of the
    gradient, which moves both by far more than the bound on the oracle."""
    (eF, eq), moved, worst = mou.kept_qp_with_disturbance(lib=emulib)
    print(f"kept F error {eF:.3e}, q~ error {eq:.3e}; the disturbance moves F / q~ by at least {moved:.3e}")
    assert moved > 1e-2, moved
    assert eF <= KEEP_TOL and eq <= KEEP_TOL, (eF, eq)
    assert worst <= TOL, worst


def test_beyond_the_lds_with_every_option(emulib):
    """SingleShooting 12,4,4,46,46 (nZ~ = 185) with M / N / L blocks, warm_dual, keep_qp and two soft custom rows: two
    closed-loop periods on the stage kernel against the oracle."""
    r = mou.beyond_lds_with_everything(lib=emulib, B=2, check=(0, 1), periods=2)
    assert r["worst"] <= TOL, r
    assert max(r["keep"]) <= KEEP_TOL, r
