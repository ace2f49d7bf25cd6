"""CPU tests of the SteadyKalmanFilter built from Q̂ and R̂ (mpcqp_kf_set_steady): the Riccati kernel body of
csrc/kf_dare_bodies.h on the CPU wave emulator (tests/emu/emu_kf_dare.cpp) through the C-ABI and the BatchLinMPC mirror, against
SciPy's solve_discrete_are, and the host code under the address and undefined-behaviour sanitizers in a stand-alone program.
The GPU tests are in tests/test_gpu_kf_dare.py.

The bar of K̂ and P̂∞ is tests/kf_util.BAR (1e-11 relative to max(1, max|.|)): a NumPy restatement of the same doubling
iteration with unpivoted Gauss-Jordan inverses sits at 1e-14 (K̂) and 5.3e-14 (P̂) against SciPy on these generators."""
import os
import subprocess

import numpy as np
import pytest

import mpcqp
from tests import emu_util
from tests import kf_dare_util as du
from tests import kf_util as ku

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def darelib():
    lib = mpcqp.api.load_library(emu_util.build(emu_util.EST))
    yield lib
    mpcqp.api._lib = None


@pytest.mark.slow
@pytest.mark.parametrize("shape,lanes", [(ku.shape_c2, 16), (ku.shape_c3, 16), (ku.shape_17, 64), (ku.shape_32, 64)],
                         ids=["C2-B6", "C3-B7", "nx17-B3", "nx32-B3"])
def test_emulator_gain_against_scipy(darelib, shape, lanes):
    """K̂ and P̂∞ of every member against SciPy; C3 at B = 7 has a partly filled group of three and two emulated wavefronts."""
    du.check_against_scipy(shape, lanes, lib=darelib)


@pytest.mark.slow
def test_emulator_small_process_noise(darelib):
    """C3 with Q̂ = 1e-6 I, R̂ = I, B = 5: status 0, within the bar, within the cap."""
    du.check_small_q(lib=darelib)


@pytest.mark.slow
def test_emulator_members_are_independent(darelib):
    """An undetectable member and a member with Q̂ = -I: a status, a zero gain, and neighbours that keep their bits."""
    du.check_independence(lib=darelib)


@pytest.mark.slow
def test_emulator_resolve_after_set_model(darelib):
    du.check_resolve(lib=darelib)


@pytest.mark.slow
def test_emulator_controller(darelib):
    """BatchLinMPC with steady=dict(Q̂, R̂) against the same controller given steady_kalman_gain; setmodel re-solves; the warning."""
    du.closed_loop(lib=darelib)
    du.check_warning(lib=darelib)


@pytest.mark.slow
def test_emulator_contract(darelib):
    """Return codes, read-backs and leaving the mode."""
    sh = ku.shape_c2(B=5)
    B, nxh = 5, sh["nxh"]
    # before a model
    h = mpcqp.api.Handle(B, nxh, sh["nu"], sh["ny"], 0, 2, 1, lib=darelib)
    with pytest.raises(mpcqp.MpcqpError, match="-5"):
        h.kf_set_steady(sh["Qhat"], sh["Rhat"], sh["i_ym"])
    du.set_model(h, sh)
    bad = sh["Qhat"].copy(); bad[0, 0, 1] += 1e-6
    with pytest.raises(mpcqp.MpcqpError, match="-3"):
        h.kf_set_steady(bad, sh["Rhat"], sh["i_ym"])
    with pytest.raises(mpcqp.MpcqpError, match="-3"):
        h.kf_set_steady(sh["Qhat"], sh["Rhat"], [0, 0])
    # a handle given its gain by kf_set: no solve, no iteration counts, the read-backs of today
    h.kf_set(np.full((B, 2, nxh), 0.1), [0, 1])
    for call in (h.kf_solve_steady, h.kf_solve_steady_device, h.kf_steady_iters, h.kf_status, h.kf_covariance):
        with pytest.raises(mpcqp.MpcqpError, match="-5"):
            call()
    assert h.kf_lanes_per_estimator() == 0
    # steady mode: P̂∞ through MPCQP_GET_KF_COV, lanes, and the estimator steps of a steady gain
    h.kf_set_steady(sh["Qhat"], sh["Rhat"], sh["i_ym"])
    K, P = du.scipy_dare(sh)
    assert h.kf_lanes_per_estimator() == 16 and not h.kf_status().any()
    assert ku.rel(h.get(mpcqp.api.GET_KF_COV).transpose(0, 2, 1), P) <= ku.BAR
    x = np.zeros((B, nxh))
    h.kf_correct(x, np.ones((B, 2)))
    assert ku.rel(x, K.sum(axis=2)) <= ku.BAR
    h.kf_solve_steady_device()
    assert ku.rel(h.kf_gain(), K) <= ku.BAR
    # kf_set leaves the mode
    h.kf_set(np.full((B, 2, nxh), 0.1), [0, 1])
    with pytest.raises(mpcqp.MpcqpError, match="-5"):
        h.kf_solve_steady()
    # and so does kf_set_covariances: the time-varying recursion as before
    h.kf_set_steady(sh["Qhat"], sh["Rhat"], sh["i_ym"])
    h.kf_set_covariances(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
    with pytest.raises(mpcqp.MpcqpError, match="-5"):
        h.kf_steady_iters()
    ref = ku.NumpyKalmanCov(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
    for _ in range(2):
        h.kf_correct(x, np.ones((B, 2))); h.kf_predict(x, np.ones((B, sh["nu"])))
        ref.correct(sh["Chat"]); ref.predict(sh["Ahat"])
    assert not h.kf_status().any() and ku.rel(h.kf_covariance(), ref.P) <= ku.BAR and ku.rel(h.kf_gain(), ref.K) <= ku.BAR


def _refused_then_kf_set(h, B, nxh, nym, Q, R, i_ym):
    with pytest.raises(mpcqp.MpcqpError, match="-4"):
        h.kf_set_steady(Q, R, i_ym)
    assert h.kf_lanes_per_estimator() == 0
    h.kf_set(np.full((B, nym, nxh), 0.1), i_ym)
    x = np.zeros((B, nxh))
    h.kf_correct(x, np.ones((B, nym)))
    assert np.allclose(x, 0.1 * nym)
    with pytest.raises(mpcqp.MpcqpError, match="-5"):
        h.kf_solve_steady()


def test_refused_beyond_32_states(darelib):
    B, nxh = 2, 33
    h = mpcqp.api.Handle(B, nxh, 1, 1, 0, 2, 1, lib=darelib)
    rng = np.random.default_rng(1)
    A = 0.5 * np.broadcast_to(np.eye(nxh), (B, nxh, nxh))
    h.set_model(mpcqp.colmajor(A), mpcqp.colmajor(rng.standard_normal((B, nxh, 1))), mpcqp.colmajor(rng.standard_normal((B, 1, nxh))))
    eye = lambda n: np.broadcast_to(np.eye(n), (B, n, n))
    _refused_then_kf_set(h, B, nxh, 1, eye(nxh), eye(1), [0])


def test_stock_emulator_refuses_the_steady_solve():
    """A library without the launcher links (weak declaration) and answers MPCQP_ERR_UNSUPPORTED; a kf_set gain still works."""
    lib = mpcqp.api.load_library(emu_util.build())
    try:
        sh = ku.shape_c2(B=2)
        h = du.make_handle(sh, lib=lib, steady=False)
        _refused_then_kf_set(h, 2, sh["nxh"], 2, sh["Qhat"], sh["Rhat"], sh["i_ym"])
    finally:
        mpcqp.api._lib = None


def test_mirror_validates_before_any_device_call():
    """BatchLinMPC.setestimator(steady=...): exclusive with Khat and covariances, Hermitian and size checks, and a handle
    without mpcqp_kf_set_steady -- all before anything is sent to the device."""
    class Recorder:
        calls = []
        def kf_set_steady(self, *a): self.calls.append(a)
        def kf_status(self): return np.zeros(2, np.int32)
    mpc = mpcqp.BatchLinMPC.__new__(mpcqp.BatchLinMPC)
    mpc.B, mpc.nxh, mpc.ny, mpc.nu, mpc.nd = 2, 3, 2, 1, 0
    mpc.xhop = np.zeros((2, 3))
    mpc.hd = Recorder()
    steady = dict(Qhat=np.eye(3), Rhat=np.eye(1))
    with pytest.raises(ValueError):
        mpc.setestimator(np.zeros((2, 3, 1)), steady=steady)
    with pytest.raises(ValueError):
        mpc.setestimator(steady=steady, covariances=dict(Qhat=np.eye(3), Rhat=np.eye(1), P0=np.eye(3)))
    with pytest.raises(ValueError, match="Hermitian"):
        mpc.setestimator(steady=dict(Qhat=np.array([[1, 0.1, 0], [0, 1, 0], [0, 0, 1.0]]), Rhat=np.eye(1)), i_ym=[1])
    with pytest.raises(ValueError, match="size"):
        mpc.setestimator(steady=dict(Qhat=np.eye(3), Rhat=np.eye(2)), i_ym=[1])
    assert not Recorder.calls
    mpc.setestimator(steady=steady, i_ym=[1], xhat0=[1.0, 2.0, 3.0])
    assert mpc.kf_steady and not mpc.kf_timevarying and Recorder.calls[0][0].shape == (2, 3, 3) and mpc.xhat0.shape == (2, 3)
    mpc.hd = object()
    with pytest.raises(NotImplementedError):
        mpc.setestimator(steady=steady, i_ym=[1])


def test_host_code_under_sanitizers(tmp_path):
    """csrc/mpcqp_host.hip compiled for the host with -fsanitize=address,undefined into tests/kf_dare_asan_main.cpp (its own
    main), with the emulator launcher compiled the same way: set, solve again after a model swap, read-backs, the refusals,
    handle destroyed.  No sanitizer goes into Python."""
    emu_util.build(emu_util.EST)
    exe = str(tmp_path / "kf_dare_asan")
    subprocess.check_call(emu_util.SANITIZER_CXX + ["-x", "c++", os.path.join(emu_util.CSRC, "mpcqp_host.hip"),
                                                    os.path.join(emu_util.EMU, "emu_kf_dare.cpp"),
                                                    os.path.join(ROOT, "tests", "kf_dare_asan_main.cpp"), "-x", "none"]
                          + emu_util.SANITIZER_OBJS + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "kf dare asan ok" in out.stdout, out.stdout + out.stderr
