"""CPU checks of the time-varying KalmanFilter of the LinMPC loop (csrc/kf_cov_bodies.h, include/mpcqp.h): the NumPy batch
recursion of tests/kf_util.py against oracle/mhe.py, the kernel body on the CPU wave emulator (tests/emu/emu_kf_cov.cpp) for
the 16-lane shapes, the refusal of a library without the kernel, the host mirror, and the host code under the address and
undefined-behaviour sanitizers in a stand-alone program.  The GPU tests are in tests/test_gpu_kf_cov.py."""
import os
import subprocess

import numpy as np
import pytest

import mpcqp
from mpcqp import synth
from oracle import estim as es
from oracle import mhe as om
from tests import emu_util
from tests import kf_util as ku

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_numpy_recursion_is_the_oracle_kalman_filter():
    """NumpyKalmanCov against oracle.mhe.make_kalman_filter (pinned on the reference's "MHE v.s. Kalman filters" test): a
    model with one integrator per measured output, 10 periods, P̂ after every correction and prediction at 1e-13."""
    rng = np.random.default_rng(4)
    A = np.array([[0.8, 0.1, 0.0], [0.0, 0.7, 0.2], [0.1, 0.0, 0.9]])
    model = es.LinModelOracle(A, rng.standard_normal((3, 2)), rng.standard_normal((2, 3)))
    kf = om.make_kalman_filter(model, direct=True, sigmaQ=[0.1, 0.2, 0.3], sigmaR=[0.5, 0.4], sigmaQint_ym=[0.2, 0.1],
                               sigmaP_0=[1.0, 2.0, 0.5], sigmaPint_ym_0=[1.0, 1.5], nint_ym=[1, 1])
    assert kf.nxh == 5
    ref = ku.NumpyKalmanCov(kf.Q[None], kf.R[None], kf.P0[None], np.arange(2))
    Ah, Ch = kf.Ah[None], np.zeros((1, 2, 5))
    Ch[0] = kf.Chm
    worst = 0.0
    for _ in range(10):
        kf.preparestate(rng.standard_normal(2))
        ref.correct(Ch)
        worst = max(worst, ku.rel(ref.P[0], kf.P))
        kf.updatestate(rng.standard_normal(2), None)
        ref.predict(Ah)
        worst = max(worst, ku.rel(ref.P[0], kf.P))
    assert worst <= 1e-13, worst
    assert np.abs(ref.K[0]).max() > 1e-2


def test_numpy_recursion_drops_an_indefinite_update():
    sh = ku.shape_c2(B=3)
    R = sh["Rhat"].copy()
    R[1] = -10.0 * np.eye(2)
    ref = ku.NumpyKalmanCov(sh["Qhat"], R, sh["P0"], sh["i_ym"])
    for _ in range(2):
        ref.correct(sh["Chat"]); ref.predict(sh["Ahat"])
    assert ref.status.tolist() == [0, 2, 0] and np.array_equal(ref.P[1], sh["P0"][1]) and not ref.K[1].any() and ref.K[0].any()


@pytest.fixture(scope="module")
def kflib():
    lib = mpcqp.api.load_library(emu_util.build(emu_util.EST))
    yield lib
    mpcqp.api._lib = None


@pytest.mark.slow
@pytest.mark.parametrize("shape,NXlanes", [(ku.shape_c2, 16), (ku.shape_c3, 16), (ku.shape_ym, 16)], ids=["C2-nx6", "C3-nx16", "iym20-nd1"])
def test_emulator_recursion(kflib, shape, NXlanes):
    """The kernel body on the CPU wave emulator, B = 7 (a tail group of three, two emulated wavefronts): K̂, P̂ and x̂ of
    four periods against NumPy at the bar of the GPU test."""
    res, h = ku.run_recursion(shape(B=7), 4, lib=kflib)
    assert h.kf_lanes_per_estimator() == NXlanes
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR and res["ex"] <= 1e-10, res


@pytest.mark.slow
def test_emulator_fused_modes_and_dropped_update(kflib):
    """Host-side plumbing on the emulator: Q̂ / R̂ replaced with P̂ kept, setstate's P̂, the refusals, the return to the steady
    gain, and one estimator whose R̂ makes M̂ indefinite (status 2, P̂ = P̂_0, K̂ = 0, neighbours untouched)."""
    sh = ku.shape_c2(B=5)
    sh["Rhat"] = sh["Rhat"].copy()
    sh["Rhat"][3] = -10.0 * np.eye(2)
    h = ku.make_handle(sh, lib=kflib)
    ref = ku.NumpyKalmanCov(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
    x = np.zeros((5, sh["nxh"]))
    for _ in range(2):
        h.kf_correct(x, np.ones((5, 2))); h.kf_predict(x, np.ones((5, sh["nu"])))
        ref.correct(sh["Chat"]); ref.predict(sh["Ahat"])
    assert h.kf_status().tolist() == [0, 0, 0, 2, 0]
    P, K = h.kf_covariance(), h.kf_gain()
    assert np.array_equal(P[3], sh["P0"][3]) and not K[3].any()
    keep = [0, 1, 2, 4]
    assert ku.rel(P[keep], ref.P[keep]) <= ku.BAR and ku.rel(K[keep], ref.K[keep]) <= ku.BAR
    # a valid R̂ with P̂ kept: the estimator recovers
    Rnew = sh["Rhat"].copy()
    Rnew[3] = 10.0 * np.eye(2)
    h.kf_set_covariances(sh["Qhat"], Rnew, None, sh["i_ym"])
    ref.R = Rnew
    h.kf_correct(x, np.ones((5, 2))); ref.correct(sh["Chat"])
    assert not h.kf_status().any() and ku.rel(h.kf_covariance(), ref.P) <= ku.BAR
    # setstate!(estim, x̂, P̂)
    h.kf_set_state_covariance(2.0 * sh["P0"])
    assert np.array_equal(h.kf_covariance(), 2.0 * sh["P0"])
    bad = sh["P0"].copy(); bad[0, 0, 1] += 1e-6
    with pytest.raises(mpcqp.MpcqpError, match="-3"):
        h.kf_set_state_covariance(bad)
    with pytest.raises(mpcqp.MpcqpError, match="-3"):
        h.kf_set_covariances(bad, sh["Rhat"], sh["P0"], sh["i_ym"])
    with pytest.raises(mpcqp.MpcqpError, match="-2"):           # Q̂, R̂ alone: nym must be the handle's
        h.kf_set_covariances(sh["Qhat"], sh["Rhat"][:, :1, :1], None, [0])
    # back to the steady gain
    h.kf_set(np.zeros((5, 2, sh["nxh"])), [0, 1])
    assert h.kf_lanes_per_estimator() == 0
    with pytest.raises(mpcqp.MpcqpError, match="-5"):
        h.kf_status()


def test_stock_emulator_refuses_the_time_varying_filter():
    """A library without the kernel unit links (weak launcher) and answers MPCQP_ERR_UNSUPPORTED; the steady gain still works."""
    lib = mpcqp.api.load_library(emu_util.build())
    try:
        sh = ku.shape_c2(B=2)
        h = mpcqp.api.Handle(2, sh["nxh"], sh["nu"], sh["ny"], 0, 2, 1, lib=lib)
        cm = mpcqp.api.colmajor
        h.set_model(cm(sh["Ahat"]), cm(sh["Bhu"]), cm(sh["Chat"]))
        with pytest.raises(mpcqp.MpcqpError, match="-4"):
            h.kf_set_covariances(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
        assert h.kf_lanes_per_estimator() == 0
        K = np.full((2, 2, sh["nxh"]), 0.1)
        h.kf_set(K, [0, 1])
        x = np.zeros((2, sh["nxh"]))
        h.kf_correct(x, np.ones((2, 2)))
        assert np.allclose(x, 0.2)
    finally:
        mpcqp.api._lib = None


def test_mirror_validates_like_the_reference():
    """BatchLinMPC.setestimator(covariances=...): keyword names, Hermitian check, direct=False refused -- before any device call."""
    class Recorder:
        calls = []
        def kf_set_covariances(self, *a): self.calls.append(a)
        def kf_set_state_covariance(self, P): self.calls.append(("P", P))
    mpc = mpcqp.BatchLinMPC.__new__(mpcqp.BatchLinMPC)
    mpc.B, mpc.nxh, mpc.ny, mpc.nu, mpc.nd = 2, 3, 2, 1, 0
    mpc.xhop = np.zeros((2, 3))
    mpc.hd = Recorder()
    with pytest.raises(NotImplementedError):
        mpc.setestimator(covariances=dict(Qhat=np.eye(3), Rhat=np.eye(1), P0=np.eye(3)), i_ym=[1], direct=False)
    with pytest.raises(ValueError, match="Hermitian"):
        mpc.setestimator(covariances=dict(Qhat=np.array([[1, 0.1, 0], [0, 1, 0], [0, 0, 1.0]]), Rhat=np.eye(1), P0=np.eye(3)), i_ym=[1])
    with pytest.raises(ValueError, match="size"):
        mpc.setestimator(covariances=dict(Qhat=np.eye(3), Rhat=np.eye(2), P0=np.eye(3)), i_ym=[1])
    with pytest.raises(ValueError):
        mpc.setestimator(np.zeros((2, 3, 1)), covariances=dict(Qhat=np.eye(3), Rhat=np.eye(1), P0=np.eye(3)))
    assert not Recorder.calls
    mpc.setestimator(covariances=dict(Qhat=np.eye(3), Rhat=np.eye(1), P0=2 * np.eye(3)), i_ym=[1], xhat0=[1.0, 2.0, 3.0])
    assert mpc.kf_timevarying and mpc.xhat0.shape == (2, 3) and Recorder.calls[0][0].shape == (2, 3, 3)
    mpc.setstate([0.0, 1.0, 2.0], Phat=np.eye(3))
    assert Recorder.calls[-1][0] == "P" and mpc.xhat0[1].tolist() == [0.0, 1.0, 2.0]
    mpc.est_kind = mpcqp.controller.EST_STEADY
    with pytest.raises(ValueError, match="no covariance"):
        mpc.setstate([0.0, 1.0, 2.0], Phat=np.eye(3))


def test_host_code_under_sanitizers(tmp_path):
    """csrc/mpcqp_host.hip compiled for the host with -fsanitize=address,undefined into tests/kf_asan_main.cpp (its own main):
    covariances set, three periods on the emulator objects, read-backs, handle destroyed.  No sanitizer goes into Python."""
    emu_util.build(emu_util.EST)
    exe = str(tmp_path / "kf_asan")
    subprocess.check_call(emu_util.SANITIZER_CXX + ["-x", "c++", os.path.join(emu_util.CSRC, "mpcqp_host.hip"),
                                                    os.path.join(ROOT, "tests", "kf_asan_main.cpp"), "-x", "none"]
                          + emu_util.SANITIZER_OBJS + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "kf asan ok" in out.stdout, out.stdout + out.stderr
