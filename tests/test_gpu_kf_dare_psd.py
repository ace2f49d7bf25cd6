"""GPU tests of the SteadyKalmanFilter built from a positive SEMIdefinite Q̂ (csrc/kf_kernels.hip: k_kf_dare_psd<NX> with four
estimators per wavefront, k_kf_dare_psd_wide<NX> with one and the products on the matrix cores: the second pass behind
mpcqp_kf_set_steady) through the C-ABI and the BatchLinMPC mirror.  Inputs and runners: tests/kf_dare_psd_util.py, shared with
the emulator tests of tests/test_kf_dare_psd.py.

K̂ and P̂∞ are compared with SciPy's solve_discrete_are at tests/kf_util.BAR, 1e-11 relative to max(1, max|.|): a NumPy
restatement of the scheme sits within 1.7e-13 / 3.8e-13 of SciPy on these generators and the emulator within 5.6e-13 /
1.6e-12.  Measured on the MI355X over the eighteen cases of the first test: K̂ within 3.1e-13 (C2, lowrank) and P̂∞ within
4.3e-13 (nx̂ = 32, lowrank), 4 - 11 iterations; the silent integrator ends at the cap with status 1; the 42 rank-one
blocks within 1.6e-12 (emulator 5.3e-14)."""
import pytest

from tests import kf_dare_psd_util as pu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gen", list(pu.GENERATORS))
@pytest.mark.parametrize("shape", list(pu.SHAPES))
def test_semidefinite_gain_against_scipy(hiplib, shape, gen):
    """One shape per compiled NX (each is a kernel of its own), three kinds of semidefinite Q̂: status 0, path 1, within the bar."""
    pu.check_against_scipy(shape, gen)


@pytest.mark.parametrize("shape,members", [("NX8-C2-B6", [1, 4]), ("NX32-B3", [1])], ids=["C2-B6", "nx32-B3"])
def test_mixed_wavefront(hiplib, shape, members):
    """Semidefinite and definite members side by side: each keeps, bit for bit, what it has among its own kind."""
    pu.check_mixed_wavefront(shape, members)


def test_still_refused(hiplib):
    """An indefinite Q̂ and a silent integrator inside a diag0 batch: a status each, zero K̂ and P̂∞, untouched neighbours, one
    warning with the count."""
    pu.check_still_refused()


def test_rank_one_blocks_take_the_square_root_pass(hiplib):
    """Numerically singular Q̂ that the definite body may get through: path 1 and the bar for all 42 members."""
    pu.check_rank_one_blocks()


def test_refused_after_the_first_pass_served(hiplib):
    """A pole at 1 that a rank-one Q̂ never reaches: a status and zeros, also where the definite body had written a gain."""
    pu.check_refused_after_first_pass()


def test_small_definite_stays_with_the_definite_body(hiplib):
    pu.check_small_definite()


def test_resolve_after_set_model(hiplib):
    pu.check_resolve()


def test_controller(hiplib):
    """BatchLinMPC with steady=dict(Q̂ = diag0, R̂) against its twin given steady_kalman_gain: no warning, path all 1."""
    pu.closed_loop()


def test_contract(hiplib):
    pu.check_contract()
