"""CPU checks of the predictor form (direct=False) and of missing measurements in the Kalman filters of the LinMPC loop, on the
CPU wave emulator (tests/emu): the reference's doctest of preparestate!, the predictor form as the filter form re-ordered,
per-member misses against the NumPy reference of tests/kf_direct_util.py, a miss next to a dropped update, the fused period
against the separate entry points with NaN in the data, and the new ABI entry points.  GPU: tests/test_gpu_kf_direct.py.

Bars: K̂ and P̂ against NumPy at tests/kf_util.BAR (1e-11), x̂ at 1e-10 (tests/test_gpu_kf_cov.py); exact equality wherever
the same kernels see the same inputs."""
import warnings

import numpy as np
import pytest

import mpcqp
from tests import emu_util
from tests import kf_direct_util as kd
from tests import kf_util as ku


@pytest.fixture(scope="module")
def kflib():
    lib = mpcqp.api.load_library(emu_util.build(emu_util.EST))
    yield lib
    mpcqp.api._lib = None


@pytest.mark.parametrize("shape", [ku.shape_c2, ku.shape_ym, ku.shape_17, ku.shape_32], ids=["C2-B6", "iym20-nd1-B5", "nx17-B3", "nx32-B3"])
def test_numpy_reference_alone_is_finite_on_the_seeds(shape):
    """The data of test_misses_per_member through the NumPy reference alone: finite, no Cholesky failure, and misses do occur."""
    ok, nmiss = kd.reference_alone(shape())
    assert ok and nmiss > shape()["Ahat"].shape[0]


@pytest.mark.slow
def test_reference_doctest_of_preparestate(kflib):
    """estimator/execute.jl:321-331: SteadyKalmanFilter(LinModel(ss(0.1, 0.5, 1, 0, 4)), nint_ym=0): preparestate!(estim, [1])
    is 0.5 (two digits) with direct=true and exactly 0.0 with direct=false."""
    A, Bu, Cm = np.full((1, 1, 1), 0.1), np.full((1, 1, 1), 0.5), np.ones((1, 1, 1))
    K = mpcqp.steady_kalman_gain(A, Cm, np.eye(1), np.eye(1))
    got = {}
    for direct in (True, False):
        mpc = mpcqp.BatchLinMPC(A, Bu, Cm, Hp=2, Hc=1, lib=kflib)
        mpc.setestimator(K, direct=direct)
        got[direct] = mpc.preparestate([1.0])
    assert np.round(got[True], 2).tolist() == [[0.5]] and got[False].tolist() == [[0.0]]


@pytest.mark.slow
@pytest.mark.parametrize("steady", [True, False], ids=["steady", "time-varying"])
def test_predictor_form_is_the_filter_form_reordered(kflib, steady):
    assert kd.run_forms(steady, lib=kflib) > 1e-2


@pytest.mark.slow
@pytest.mark.parametrize("shape,lanes", [(ku.shape_c2, 16), (ku.shape_ym, 16), (ku.shape_17, 64), (ku.shape_32, 64)],
                         ids=["C2-B6", "iym20-nd1-B5", "nx17-B3", "nx32-B3"])
def test_misses_per_member(kflib, shape, lanes):
    """12 periods, each estimator missing about one in four (one NaN channel or all), one period with ym=None: a missed
    correction keeps x̂0, P̂, K̂ bit for bit with status 1 (asserted inside), everything follows NumPy at the bars."""
    res = kd.run_misses(shape(), lib=kflib)
    assert res["lanes"] == lanes and res["nmiss"] > 0
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR and res["ex"] <= kd.XBAR, res


@pytest.mark.slow
@pytest.mark.parametrize("shape", [ku.shape_c2, ku.shape_17], ids=["C2-B6", "nx17-B3"])
def test_misses_per_member_predictor_form(kflib, shape):
    res = kd.run_misses(shape(), lib=kflib, direct=False)
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR and res["ex"] <= kd.XBAR, res


def check_miss_and_drop(lib):
    sts, P, K, ref, sh, mpc = kd.run_miss_and_drop(lib)
    want = [[0, 0, 0, 2, 0], [0, 1, 0, 2, 0], [0, 0, 0, 1, 0]]
    assert [s[0] for s in sts] == want and [s[1] for s in sts] == want, sts
    # estimator 3 never had a correction (K̂ = 0), but its miss let the prediction run: P̂ is no longer P̂_0
    assert not K[3].any() and not np.array_equal(P[3], sh["P0"][3])
    assert ku.rel(P[3], sh["Ahat"][3] @ sh["P0"][3] @ sh["Ahat"][3].T + sh["Qhat"][3]) <= ku.BAR
    assert ku.rel(P, ref.cov.P) <= ku.BAR and ku.rel(K, ref.K) <= ku.BAR and ku.rel(mpc.xhat0, ref.x) <= kd.XBAR


@pytest.mark.slow
def test_miss_and_drop_together(kflib):
    check_miss_and_drop(kflib)


@pytest.mark.slow
@pytest.mark.parametrize("ms", [False, True], ids=["condensed", "MultipleShooting"])
@pytest.mark.parametrize("tv", [True, False], ids=["time-varying", "steady"])
@pytest.mark.parametrize("direct", [1, 0], ids=["direct1", "direct0"])
def test_fused_equals_separate_with_misses(kflib, direct, tv, ms):
    """mpcqp_loop_device against the separate entry points, B = 64, five periods, NaN in a tenth of the (estimator, period)
    pairs: x̂0, u0, Z̃, K̂ and P̂ differ by exactly 0.0; the missed estimators' step statuses are 0 (asserted inside)."""
    diff, kmax, nmiss = kd.fused_variants(direct, tv, ms, lib=kflib)
    assert diff == 0.0 and kmax > 1e-2 and nmiss > 10, (diff, kmax, nmiss)


@pytest.mark.slow
def test_abi_of_the_new_entry_points(kflib):
    sh = ku.shape_c2(B=5)
    B, nxh = 5, sh["nxh"]
    cm = mpcqp.api.colmajor
    h0 = mpcqp.api.Handle(B, nxh, sh["nu"], sh["ny"], 0, 2, 1, lib=kflib)
    h0.set_model(cm(sh["Ahat"]), cm(sh["Bhu"]), cm(sh["Chat"]))
    x = np.ones((B, nxh))
    with pytest.raises(mpcqp.MpcqpError, match="-5"):          # MPCQP_ERR_ORDER: no estimator attached
        h0.kf_update(x, np.zeros((B, sh["nu"])), np.zeros((B, 2)))
    with pytest.raises(mpcqp.MpcqpError, match="-3"):          # MPCQP_ERR_ARG
        _chk_direct(h0, 2)
    # y0m == NULL: prediction only, every status 1, K̂ untouched, P̂ predicted once
    h = ku.make_handle(sh, lib=kflib)
    u = np.full((B, sh["nu"]), 0.1)
    x1 = x.copy()
    h.kf_update(x1, u, None)
    assert h.kf_status().tolist() == [1] * B and not h.kf_gain().any()
    xp = np.einsum("bij,bj->bi", sh["Ahat"], x) + np.einsum("bij,bj->bi", sh["Bhu"], u)
    Pp = sh["Ahat"] @ sh["P0"] @ sh["Ahat"].transpose(0, 2, 1) + sh["Qhat"]
    assert ku.rel(x1, xp) <= kd.XBAR and ku.rel(h.kf_covariance(), Pp) <= ku.BAR
    # kf_correct with y0m == NULL: nothing moves, every status 1
    h3 = ku.make_handle(sh, lib=kflib)
    h3.kf_correct(x1, np.full((B, 2), 0.3))
    assert not h3.kf_status().any()
    xk, Pk, Kk = x1.copy(), h3.kf_covariance(), h3.kf_gain()
    h3.kf_correct(x1, None)
    assert h3.kf_status().tolist() == [1] * B and np.array_equal(x1, xk)
    assert np.array_equal(h3.kf_covariance(), Pk) and np.array_equal(h3.kf_gain(), Kk) and Kk.any()
    # kf_update equals kf_correct followed by kf_predict bit for bit, P̂ moving once
    y = np.full((B, 2), 0.3); y[2, 1] = np.nan
    h2 = ku.make_handle(sh, lib=kflib)
    xa, xb = x.copy(), x.copy()
    h.kf_set_state_covariance(sh["P0"])
    h.kf_update(xa, u, y)
    h2.kf_correct(xb, y); h2.kf_predict(xb, u)
    assert np.array_equal(xa, xb) and np.array_equal(h.kf_covariance(), h2.kf_covariance()) and np.array_equal(h.kf_gain(), h2.kf_gain())
    assert h.kf_status().tolist() == [0, 0, 1, 0, 0] == h2.kf_status().tolist()


def _chk_direct(h, v):
    mpcqp.api._chk(h.lib, h.lib.mpcqp_kf_set_direct(h.h, v))


@pytest.mark.slow
@pytest.mark.parametrize("tv", [True, False], ids=["kf_set-then-covariances", "covariances-then-kf_set"])
def test_direct_flag_survives_the_setters(kflib, tv):
    """kf_set_direct(0), then both setters in turn: mpcqp_loop_device still runs step -> correction -> prediction (equal to
    step_device + kf_update_device, whose step sees the uncorrected x̂0)."""
    diff, _, _ = kd.fused_variants(0, tv, False, B=3, periods=2, lib=kflib, churn=True)
    assert diff == 0.0
