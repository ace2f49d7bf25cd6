"""CPU tests of the SteadyKalmanFilter built from a positive SEMIdefinite Q̂: the second pass of the Riccati solve
(csrc/kf_dare_bodies.h, square-root form: H(k) = L L' without pivoting, S = L (I + L'GL)⁻¹ L') on the CPU wave emulator
(tests/emu/emu_kf_dare_psd.cpp in tests/emu/libmpcqp_emu_est_psd.so) through the C-ABI and the BatchLinMPC mirror, against
SciPy's solve_discrete_are, and the host code under the address and undefined-behaviour sanitizers in a stand-alone program.
The GPU tests are in tests/test_gpu_kf_dare_psd.py; inputs and runners in tests/kf_dare_psd_util.py.

The bar of K̂ and P̂∞ is tests/kf_util.BAR (1e-11 relative to max(1, max|.|)).  A NumPy restatement of the scheme sits within
1.7e-13 (K̂) and 3.8e-13 (P̂∞) of SciPy on these generators; measured on the emulator over the eighteen cases of the first
test: K̂ within 5.6e-13 and P̂∞ within 1.6e-12 (both at nx̂ = 32, lowrank; every other case below 5e-13), 4 - 11 iterations."""
import os
import subprocess

import pytest

import mpcqp
from tests import emu_util
from tests import kf_dare_psd_util as pu
from tests import kf_util as ku

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def psdlib():
    lib = mpcqp.api.load_library(pu.build_emulator())
    yield lib
    mpcqp.api._lib = None


@pytest.mark.slow
@pytest.mark.parametrize("gen", list(pu.GENERATORS))
@pytest.mark.parametrize("shape", list(pu.SHAPES))
def test_emulator_semidefinite_gain_against_scipy(psdlib, shape, gen):
    """One shape per compiled NX, three kinds of semidefinite Q̂: status 0, path 1, K̂ and P̂∞ within the bar.  (Without the
    second pass every member has status 2.)"""
    pu.check_against_scipy(shape, gen, lib=psdlib)


@pytest.mark.slow
@pytest.mark.parametrize("shape,members", [("NX8-C2-B6", [1, 4]), ("NX32-B3", [1])], ids=["C2-B6", "nx32-B3"])
def test_emulator_mixed_wavefront(psdlib, shape, members):
    """Semidefinite and definite members side by side: each keeps, bit for bit, what it has among its own kind."""
    pu.check_mixed_wavefront(shape, members, lib=psdlib)


@pytest.mark.slow
def test_emulator_still_refused(psdlib):
    """An indefinite Q̂ and a silent integrator inside a diag0 batch: a status each, zero K̂ and P̂∞, untouched neighbours, one
    warning with the count."""
    pu.check_still_refused(lib=psdlib)


@pytest.mark.slow
def test_emulator_rank_one_blocks_take_the_square_root_pass(psdlib):
    """Numerically singular Q̂ that the definite body may get through: path 1 and the bar for all 42 members."""
    pu.check_rank_one_blocks(lib=psdlib)


@pytest.mark.slow
def test_emulator_refused_after_the_first_pass_served(psdlib):
    """A pole at 1 that a rank-one Q̂ never reaches: a status and zeros, also where the definite body had written a gain."""
    pu.check_refused_after_first_pass(lib=psdlib)


@pytest.mark.slow
def test_emulator_small_definite_stays_with_the_definite_body(psdlib):
    pu.check_small_definite(lib=psdlib)


@pytest.mark.slow
def test_emulator_resolve_after_set_model(psdlib):
    pu.check_resolve(lib=psdlib)


@pytest.mark.slow
def test_emulator_controller(psdlib):
    """BatchLinMPC with steady=dict(Q̂ = diag0, R̂) against its twin given steady_kalman_gain: no warning, path all 1."""
    pu.closed_loop(lib=psdlib)


@pytest.mark.slow
def test_emulator_contract(psdlib):
    pu.check_contract(lib=psdlib)


@pytest.mark.slow
def test_library_without_the_second_pass_keeps_status_2():
    """tests/emu/libmpcqp_emu_est.so exports mpcqp_kf_steady_path but links no launcher of the second pass (weak declaration):
    a diag0 batch gets status 2, a zero gain and path 0, as before."""
    lib = mpcqp.api.load_library(emu_util.build(emu_util.EST))
    try:
        from tests import kf_dare_util as du
        h = du.make_handle(pu.diag0(ku.shape_c2(B=6)), lib=lib)
        assert h.kf_status().tolist() == [2] * 6 and h.kf_steady_path().tolist() == [0] * 6
        assert not h.kf_gain().any() and not h.kf_covariance().any()
    finally:
        mpcqp.api._lib = None


def test_mirror_without_the_entry_point_keeps_todays_getinfo():
    """A library without mpcqp_kf_steady_path (an older build): the Handle methods raise NotImplementedError naming the entry
    point, like every other optional one."""
    h = mpcqp.api.Handle.__new__(mpcqp.api.Handle)
    h.lib = object()
    for call, name in ((h.kf_steady_path, "mpcqp_kf_steady_path"), (lambda: h.kf_set_steady(None, None, [0]), "mpcqp_kf_set_steady")):
        with pytest.raises(NotImplementedError, match="this library has no " + name):
            call()


def test_host_code_under_sanitizers(tmp_path):
    """csrc/mpcqp_host.hip compiled for the host with -fsanitize=address,undefined into tests/kf_dare_psd_asan_main.cpp (its
    own main), with both emulator launchers of the Riccati solve compiled the same way: set with a diag0 batch, solve again
    after a model swap, the read-backs including mpcqp_kf_steady_path, handle destroyed.  No sanitizer goes into Python."""
    emu_util.build(emu_util.EST)
    exe = str(tmp_path / "kf_dare_psd_asan")
    subprocess.check_call(emu_util.SANITIZER_CXX + ["-x", "c++", os.path.join(emu_util.CSRC, "mpcqp_host.hip"),
                                                    os.path.join(emu_util.EMU, "emu_kf_dare.cpp"),
                                                    os.path.join(emu_util.EMU, "emu_kf_dare_psd.cpp"),
                                                    os.path.join(ROOT, "tests", "kf_dare_psd_asan_main.cpp"), "-x", "none"]
                          + emu_util.SANITIZER_OBJS + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "kf dare psd asan ok" in out.stdout, out.stdout + out.stderr
