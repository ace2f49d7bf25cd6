"""CPU tests of the SteadyKalmanFilter built from Q̂ and R̂ for 32 < max(nx̂, nym) <= 64 (mpcqp_kf_set_steady on the LDS-resident
Riccati kernels): the body of csrc/kf_dare_lds_bodies.h on the CPU wave emulator (tests/emu/emu_kf_dare_lds.cpp: one emulated
wavefront per estimator, T = 1) through the C-ABI and the BatchLinMPC mirror, against SciPy's solve_discrete_are, and the host code
under the address and undefined-behaviour sanitizers in a stand-alone program.  The GPU tests are in
tests/test_gpu_kf_dare_lds.py.

The bar of K̂ and P̂∞ is tests/kf_util.BAR (1e-11 relative to max(1, max|.|)): a NumPy restatement of the same doubling iteration
with unpivoted Gauss-Jordan inverses sits at 4.4e-15 (K̂) and 3.5e-14 (P̂∞) against SciPy on these generators."""
import os
import subprocess

import numpy as np
import pytest

import mpcqp
from tests import emu_util
from tests import kf_dare_lds_util as lu
from tests import kf_dare_util as du
from tests import kf_util as ku

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ldslib():
    lib = mpcqp.api.load_library(lu.build_emulator())
    yield lib
    mpcqp.api._lib = None


@pytest.mark.slow
@pytest.mark.parametrize("shape_id", list(lu.SHAPES))
def test_emulator_gain_against_scipy(ldslib, shape_id):
    """K̂ and P̂∞ of every member against SciPy, one shape per padded order and per edge; 64 lanes per estimator on the emulator.
    Without the LDS-resident kernels mpcqp_kf_set_steady answers -4 for every one of these shapes."""
    lu.check_against_scipy(shape_id, 64, lib=ldslib)


@pytest.mark.slow
def test_emulator_small_process_noise(ldslib):
    """nx̂ = 40 with Q̂ = 1e-6 I, R̂ = I: status 0, within the bar, within the cap."""
    lu.check_small_q(lib=ldslib)


@pytest.mark.slow
def test_emulator_members_are_independent(ldslib):
    """nx̂ = 33, B = 6: an undetectable member, one with Q̂ = -I and one with a rank-5 Q̂ get a status and zeros, their neighbours
    the bits of the healthy batch, the mirror one warning with the count."""
    lu.check_independence(lib=ldslib)


@pytest.mark.slow
def test_emulator_resolve_after_set_model(ldslib):
    lu.check_resolve(lib=ldslib)


@pytest.mark.slow
def test_emulator_controller(ldslib):
    """BatchLinMPC at nx̂ = 40 with steady=dict(Q̂, R̂) against the same controller given steady_kalman_gain; setmodel re-solves."""
    lu.closed_loop(lib=ldslib)


@pytest.mark.slow
def test_emulator_what_stays_refused(ldslib):
    """kf_set_covariances and est_initstate answer -4 on the wide handle, which keeps its solved gain."""
    lu.check_still_refused(lib=ldslib)


def test_library_without_the_launcher_still_refuses():
    """libmpcqp_emu_est.so has the row-lane Riccati launcher and not the LDS-resident one: -4 at nx̂ = 33, as before."""
    lib = mpcqp.api.load_library(emu_util.build(emu_util.EST))
    try:
        sh = lu.reference("nx33-nym3")[0]
        h = du.make_handle(sh, lib=lib, steady=False)
        with pytest.raises(mpcqp.MpcqpError, match="-4"):
            h.kf_set_steady(sh["Qhat"], sh["Rhat"], sh["i_ym"])
        assert h.kf_lanes_per_estimator() == 0
    finally:
        mpcqp.api._lib = None


def test_host_code_under_sanitizers(tmp_path):
    """csrc/mpcqp_host.hip compiled for the host with -fsanitize=address,undefined into tests/kf_dare_lds_asan_main.cpp (its own
    main), with the emulator launchers compiled the same way: set at nx̂ = 33, solve again after a model swap, the read-backs,
    the refusals that stay, handle destroyed.  No sanitizer goes into Python."""
    emu_util.build(emu_util.EST)
    exe = str(tmp_path / "kf_dare_lds_asan")
    subprocess.check_call(emu_util.SANITIZER_CXX + ["-x", "c++", os.path.join(emu_util.CSRC, "mpcqp_host.hip"),
                                                    os.path.join(emu_util.EMU, "emu_kf_dare.cpp"),
                                                    os.path.join(emu_util.EMU, "emu_kf_dare_lds.cpp"),
                                                    os.path.join(ROOT, "tests", "kf_dare_lds_asan_main.cpp"), "-x", "none"]
                          + emu_util.SANITIZER_OBJS + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "kf dare lds asan ok" in out.stdout, out.stdout + out.stderr
