"""`LinMPC(MovingHorizonEstimator)` on the CPU wave emulator (tests/emu/libmpcqp_emu_mheloop.so: the emulated controller, plant
and estimator kernels + csrc/est_init_bodies.h under the launcher of tests/emu/emu_est_init.cpp): the attachment, the public
methods, `sim` and mpcqp_loop_device with the estimator on the device, `initstate`.  The checks are tests/mhe_loop_util.py's;
tests/test_gpu_mhe_loop.py runs the same ones on the HIP library."""
import os
import subprocess

import numpy as np
import pytest

import mpcqp
from tests import mhe_loop_util as mu
from tests import sim_util as su

pytestmark = pytest.mark.slow


@pytest.fixture(scope="module")
def lib():
    return mpcqp.api.load_library(mu.build())


def test_attach_and_refusals(lib):
    mu.check_attach_and_refusals(lib)


@pytest.mark.parametrize("direct", [True, False])
def test_public_methods_forward_to_the_estimator(lib, direct):
    mu.check_public_methods(lib, direct)


@pytest.mark.parametrize("name", list(mu.TWIN_CASES))
def test_sim_against_the_per_period_twin(lib, name):
    mu.check_sim_against_twin(lib, name)


@pytest.mark.parametrize("bounded", [False, True])
def test_recorded_run_replayed_through_the_oracle(lib, bounded):
    mu.check_oracle_replay(lib, bounded)


@pytest.mark.parametrize("kw", [dict(), dict(direct=False), dict(kind="linmpc_umax")])
def test_two_runs_of_three_equal_one_of_six(lib, kw):
    mu.check_continuation(lib, **kw)


@pytest.mark.parametrize("wide", [False, True])
def test_member_equals_itself_alone(lib, wide):
    mu.check_member_alone(lib, wide)


def test_a_member_whose_estimator_fails(lib):
    mu.check_failing_member(lib)


@pytest.mark.parametrize("kind,direct", [("linmpc_umax", True), ("explicit_step", False)])
def test_loop_device_equals_prepare_step_update(lib, kind, direct):
    mu.check_loop_device(lib, kind, direct)


@pytest.mark.parametrize("name", list(mu.INIT_SHAPES))
def test_initstate_against_lstsq(lib, name):
    mu.check_initstate_lstsq(lib, name)


def test_initstate_doctest_of_the_reference(lib):
    mu.check_initstate_doctest(lib)


def test_initstate_reproduces_the_measurement_of_a_consistent_system(lib):
    mu.check_initstate_consistent(lib)


@pytest.mark.parametrize("name", ["nx16_nym4", "nx17_nym4"])
def test_initstate_member_alone(lib, name):
    mu.check_initstate_member_alone(lib, name)


def test_initstate_rank_deficient_member(lib):
    mu.check_initstate_rank_deficient(lib)


def test_initstate_covariance_half(lib):
    mu.check_initstate_covariances(lib)


@pytest.mark.parametrize("xhat_given", [False, True])
def test_sim_initstate_equals_the_calls_made_by_hand(lib, xhat_given):
    mu.check_sim_initstate(lib, xhat_given)


def test_other_emulator_libraries_have_no_initstate_kernel():
    """A library without the launcher of csrc/est_init_launch.h refuses: no quiet fall-back."""
    sim = mpcqp.api.load_library(su.build())
    c = su.Case("explicit_law")
    mpc = c.controller(sim)
    with pytest.raises(mpcqp.MpcqpError, match="error -4:"):
        mpc.initstate(c.lastu, c.bt["ops"]["yop"], c.d)


def test_host_code_under_sanitizers(tmp_path):
    """Attach, loop, a simulation with a moving window, detaching a borrowed estimator and initstate in a stand-alone program
    under the address and undefined-behaviour sanitizers, linked against the emulator objects like tests/sim_asan_main.cpp;
    nothing is loaded into python."""
    mu.build()
    exe = str(tmp_path / "mhe_loop_asan")
    subprocess.check_call(su.SANITIZER_CXX + ["-x", "c++", os.path.join(su.CSRC, "mpcqp_host.hip"), os.path.join(su.CSRC, "mhe_host.hip"),
                                              os.path.join(su.ROOT, "tests", "mhe_loop_asan_main.cpp"), "-x", "none"]
                          + [o for o in mu.SANITIZER_OBJS if not o.endswith("mhe_host.o")] + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "mhe loop sanitizer run: ok" in out.stdout, out.stdout + out.stderr
