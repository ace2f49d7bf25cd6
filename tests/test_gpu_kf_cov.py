"""GPU tests of the time-varying KalmanFilter of the LinMPC loop (csrc/kf_kernels.hip: k_kf_cov<NX> with four estimators per
wavefront, k_kf_cov_wide<NX> with one and the products on the matrix cores) through the C-ABI and the BatchLinMPC mirror.

The bar of K̂ and P̂ against the NumPy recursion of tests/kf_util.py is 1e-11 relative to max(1, max|.|): two operation
orders of this recursion on the CPU differ by 1e-15 on these inputs, which leaves four decades for the Gauss-Jordan inverse
and the summation order of the matrix cores and still catches any wrong entry."""
import numpy as np
import pytest

import mpcqp
from mpcqp import synth
from tests import kf_util as ku

pytestmark = pytest.mark.gpu
TOL = 1e-5          # tests/test_gpu_parity.py: the interior-point optimum against the oracle controller


@pytest.mark.parametrize("shape,lanes", [(ku.shape_c2, 16), (ku.shape_c3, 16), (ku.shape_ym, 16), (ku.shape_17, 64), (ku.shape_32, 64)],
                         ids=["C2-B6", "C3-B7", "iym20-nd1-B5", "nx17-B3", "nx32-B3"])
def test_recursion_against_numpy(hiplib, shape, lanes):
    """K̂ and P̂ after each of 12 periods (correction and prediction) against NumPy, x̂ along with them."""
    res, h = ku.run_recursion(shape(), 12)
    print(res)
    assert h.kf_lanes_per_estimator() == lanes
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR and res["ex"] <= 1e-10, res


def test_closed_loop_with_the_time_varying_filter(hiplib):
    """C2, B = 6, 15 periods of preparestate / moveinput / updatestate: u within TOL of the oracle controller fed by the NumPy
    filter, x̂ within 1e-5 max(1, |x̂|)."""
    res, ref, _, gpu, st = ku.closed_loop(synth.C2, 6, 21, 15)
    print(res)
    assert np.all(st == 0) and not gpu.hd.kf_status().any()
    assert res["eu"] <= TOL and res["ex"] <= 1e-5 and res["eK"] <= ku.BAR and res["eP"] <= ku.BAR, res
    info = gpu.getinfo()
    assert ku.rel(info["P̂"], ref.P) <= ku.BAR and ku.rel(info["K̂"], ref.K) <= ku.BAR and not info["kf_status"].any()


def test_model_swap_is_picked_up(hiplib):
    """The same loop with setmodel after periods 5 and 9 (Â scaled by 0.9, B̂u perturbed): K̂ and P̂ stay with a NumPy filter
    given the same swaps, and differ visibly from one that never saw them (a kernel reading a stale copy of the model)."""
    res, ref, stale, gpu, st = ku.closed_loop(synth.C2, 6, 21, 15, swaps=(5, 9))
    print(res, ku.rel(stale.P, ref.P), ku.rel(stale.K, ref.K))
    assert np.all(st != mpcqp.STATUS_ERROR)
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR and res["ex"] <= 1e-5, res
    P, K = gpu.hd.kf_covariance(), gpu.hd.kf_gain()
    assert ku.rel(P, stale.P) > 1e-6 and ku.rel(K, stale.K) > 1e-6


def test_fused_loop_equals_separate_calls(hiplib):
    """mpcqp_loop_device against kf_correct_device + step_device + kf_predict_device on a time-varying handle, B = 64, five
    periods, condensed kernel and MultipleShooting: x̂, u0, Z̃, P̂ and K̂ differ by exactly 0.0."""
    import torch
    for ms in (False, True):
        diff, kmax = ku.fused_vs_separate(B=64, periods=5, torch_device=torch.device("cuda", 0), multiple_shooting=ms)
        assert diff == 0.0 and kmax > 1e-2, (ms, diff, kmax)


def test_dropped_update_is_a_status_not_a_fault(hiplib):
    """B = 5, estimator 3 with R̂ = -10 I: after two periods its status is 2, its P̂ is P̂_0 and its K̂ zero; the other four match
    NumPy; the LinMPC step statuses are untouched."""
    cfg, B = synth.C2, 5
    sh = ku.shape_linmpc(cfg, B, 21)
    R = sh["Rhat"].copy()
    R[3] = -10.0 * np.eye(cfg.ny)
    from tests.parity_util import make_controller
    gpu = make_controller(cfg, sh["bt"])
    gpu.setestimator(covariances=dict(Qhat=sh["Qhat"], Rhat=R, P0=sh["P0"]), xhat0=sh["bt"]["xhat0"])
    gpu.lastu0 = sh["bt"]["lastu0"].copy()
    ref = ku.NumpyKalmanCov(sh["Qhat"], R, sh["P0"], sh["i_ym"])
    rng = np.random.default_rng(2)
    for _ in range(2):
        y = 0.3 * rng.standard_normal((B, cfg.ny))
        gpu.preparestate(y); ref.correct(sh["Chat"])
        u = gpu.moveinput(None, sh["bt"]["ry"])
        assert np.all(gpu.status == 0)
        gpu.updatestate(u, y); ref.predict(sh["Ahat"])
    assert gpu.hd.kf_status().tolist() == [0, 0, 0, 2, 0] and ref.status.tolist() == [0, 0, 0, 2, 0]
    P, K = gpu.hd.kf_covariance(), gpu.hd.kf_gain()
    assert np.array_equal(P[3], sh["P0"][3]) and not K[3].any()
    keep = [0, 1, 2, 4]
    assert ku.rel(P[keep], ref.P[keep]) <= ku.BAR and ku.rel(K[keep], ref.K[keep]) <= ku.BAR


def test_limits_and_modes(hiplib):
    """nx̂ = 33 is refused and the handle still takes a steady gain; lanes per estimator 0 / 16 / 64; a 16-lane and a wide
    handle stepped alternately in one process."""
    B, nxh = 2, 33
    h = mpcqp.api.Handle(B, nxh, 1, 1, 0, 2, 1)
    rng = np.random.default_rng(1)
    A = 0.5 * np.broadcast_to(np.eye(nxh), (B, nxh, nxh))
    h.set_model(mpcqp.colmajor(A), mpcqp.colmajor(rng.standard_normal((B, nxh, 1))), mpcqp.colmajor(rng.standard_normal((B, 1, nxh))))
    eye = lambda n: np.broadcast_to(np.eye(n), (B, n, n))
    with pytest.raises(mpcqp.MpcqpError, match="-4"):
        h.kf_set_covariances(eye(nxh), eye(1), eye(nxh), [0])
    h.kf_set(np.full((B, 1, nxh), 0.1), [0])
    x = np.zeros((B, nxh))
    h.kf_correct(x, np.ones((B, 1)))
    assert np.allclose(x, 0.1) and h.kf_lanes_per_estimator() == 0
    # alternately
    s16, s64 = ku.shape_c2(), ku.shape_17()
    h16, h64 = ku.make_handle(s16), ku.make_handle(s64)
    assert (h16.kf_lanes_per_estimator(), h64.kf_lanes_per_estimator()) == (16, 64)
    r16 = ku.NumpyKalmanCov(s16["Qhat"], s16["Rhat"], s16["P0"], s16["i_ym"])
    r64 = ku.NumpyKalmanCov(s64["Qhat"], s64["Rhat"], s64["P0"], s64["i_ym"])
    x16, x64 = np.zeros((6, s16["nxh"])), np.zeros((3, s64["nxh"]))
    for _ in range(3):
        h16.kf_correct(x16, np.ones((6, 2))); h64.kf_correct(x64, np.ones((3, 3)))
        h16.kf_predict(x16, np.ones((6, 2))); h64.kf_predict(x64, np.ones((3, 2)))
        r16.correct(s16["Chat"]); r16.predict(s16["Ahat"]); r64.correct(s64["Chat"]); r64.predict(s64["Ahat"])
    assert ku.rel(h16.kf_covariance(), r16.P) <= ku.BAR and ku.rel(h64.kf_covariance(), r64.P) <= ku.BAR
    assert ku.rel(h16.kf_gain(), r16.K) <= ku.BAR and ku.rel(h64.kf_gain(), r64.K) <= ku.BAR
