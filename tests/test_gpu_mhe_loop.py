"""`LinMPC(MovingHorizonEstimator)` on the MI355X: the checks of tests/test_mhe_loop.py on the HIP library, at the same bars
(csrc/est_kernels.hip for `initstate`, the estimator's launches on the stream of the controller's loop), and the device entry
points on torch buffers on a side stream."""
import numpy as np
import pytest

import mpcqp
from mpcqp import mhe as pm
from tests import mhe_loop_util as mu
from tests import sim_util as su

pytestmark = pytest.mark.gpu


def test_attach_and_refusals(hiplib):
    mu.check_attach_and_refusals(None)


@pytest.mark.parametrize("direct", [True, False])
def test_public_methods_forward_to_the_estimator(hiplib, direct):
    mu.check_public_methods(None, direct)


@pytest.mark.parametrize("name", list(mu.TWIN_CASES))
def test_sim_against_the_per_period_twin(hiplib, name):
    mu.check_sim_against_twin(None, name)


@pytest.mark.parametrize("bounded", [False, True])
def test_recorded_run_replayed_through_the_oracle(hiplib, bounded):
    mu.check_oracle_replay(None, bounded)


@pytest.mark.parametrize("kw", [dict(), dict(direct=False), dict(kind="linmpc_umax")])
def test_two_runs_of_three_equal_one_of_six(hiplib, kw):
    mu.check_continuation(None, **kw)


@pytest.mark.parametrize("wide", [False, True])
def test_member_equals_itself_alone(hiplib, wide):
    mu.check_member_alone(None, wide)


def test_a_member_whose_estimator_fails(hiplib):
    mu.check_failing_member(None)


@pytest.mark.parametrize("kind,direct", [("linmpc_umax", True), ("explicit_step", False)])
def test_loop_device_equals_prepare_step_update(hiplib, kind, direct):
    mu.check_loop_device(None, kind, direct)


@pytest.mark.parametrize("name", list(mu.INIT_SHAPES))
def test_initstate_against_lstsq(hiplib, name):
    mu.check_initstate_lstsq(None, name)


def test_initstate_doctest_of_the_reference(hiplib):
    mu.check_initstate_doctest(None)


def test_initstate_reproduces_the_measurement_of_a_consistent_system(hiplib):
    mu.check_initstate_consistent(None)


@pytest.mark.parametrize("name", ["nx16_nym4", "nx17_nym4"])
def test_initstate_member_alone(hiplib, name):
    mu.check_initstate_member_alone(None, name)


def test_initstate_rank_deficient_member(hiplib):
    mu.check_initstate_rank_deficient(None)


def test_initstate_covariance_half(hiplib):
    mu.check_initstate_covariances(None)


@pytest.mark.parametrize("xhat_given", [False, True])
def test_sim_initstate_equals_the_calls_made_by_hand(hiplib, xhat_given):
    mu.check_sim_initstate(None, xhat_given)


def test_device_entry_points_on_torch_buffers_on_a_side_stream(hiplib):
    """mpcqp_sim_device with a MovingHorizonEstimator attached and mpcqp_est_initstate_device on torch buffers, enqueued on a
    side stream of torch's, B = 67 (C3 plant dimensions); against the host-pointer calls, bit for bit.  The estimator's
    set-up ran on its own stream and the controller's on the handle's: this is the test that sees the cross-stream ordering."""
    import torch
    mc = mu.MheCase("explicit_law", dims=dict(nx=12, nu=4, ny=4, Hp=6, Hc=2), B=67, N=4, seed=5)
    case = mc.case
    host_mpc = mc.controller()
    host = mu.run(host_mpc, **mc.args())
    mpc = mc.controller()
    mpc._sim_plant(case.plant)
    B, N, nxp = case.B, case.N, case.nxp
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()
    o = case.bt["ops"]
    with torch.cuda.stream(side):
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        abi = lambda w: t(w.transpose(0, 2, 1))
        inp = dict(ry=t(case.ry - o["yop"]), d=t(case.d - o["dop"]), u_step=t(case.kw["u_step"]), y_step=t(case.kw["y_step"]),
                   d_step=t(case.kw["d_step"]), sigma_u=t(case.kw["u_noise"]), sigma_y=t(case.kw["y_noise"]), sigma_d=t(case.kw["d_noise"]),
                   sigma_x=t(case.kw["x_noise"]), w_u=abi(case.draws["w_u"]), w_y=abi(case.draws["w_y"]), w_d=abi(case.draws["w_d"]),
                   w_x=abi(case.draws["w_x"]), x0=t(case.x_0 - case.plant["xop"]), xhat0=t(case.xhat_0 - o["xhop"]), lastu0=t(case.lastu - o["uop"]))
        new = lambda n, dt=torch.float64: torch.full((B, N, n), -7, dtype=dt, device=dev)
        rec = dict(Y=new(4), X=new(nxp), D=new(1), Xhat=new(16), Yhat=new(4), U=new(4), Ud=new(4))
        st = torch.full((B, N), -7, dtype=torch.int32, device=dev)
        mpc.hd.sim_device(N, stream=side.cuda_stream, status=st.data_ptr(), **{k: v.data_ptr() for k, v in {**inp, **rec}.items()})
    side.synchronize()
    g = lambda a: a.cpu().numpy().transpose(0, 2, 1)
    assert np.all(st.cpu().numpy() == 0)
    for k, name, op in (("Y", "Y_data", o["yop"]), ("X", "X_data", case.plant["xop"]), ("D", "D_data", o["dop"]), ("Xhat", "X̂_data", o["xhop"]),
                        ("Yhat", "Ŷ_data", o["yop"]), ("U", "U_data", o["uop"]), ("Ud", "Ud_data", o["uop"])):
        op = np.broadcast_to(op, (B, rec[k].shape[2]))
        assert np.array_equal(g(rec[k]) + op[:, :, None], getattr(host, name)), k
    assert np.array_equal(mpc.hd.sim_est_status(N).T, host.est_status)
    # the estimator's own stream goes on behind the run: its x̂0 is the caller's, and the host run's
    assert np.array_equal(mpc.mhe.handle.get(pm.GET_XHAT0), inp["xhat0"].cpu().numpy())
    assert np.array_equal(mpc.mhe.handle.get(pm.GET_XHAT0), host_mpc.xhat0)

    # mpcqp_est_initstate_device on the side stream against the host-pointer call
    u0, y0m, d0 = case.lastu - o["uop"], 0.5 + 0.1 * case.draws["w_y"][:, :, 0], case.d - o["dop"]
    xh = np.full((B, 16), 3.0)
    sth = mpc.hd.est_initstate(xh, u0, y0m, d0)
    with torch.cuda.stream(side):
        xd, ud, yd, dd = t(np.full((B, 16), 3.0)), t(u0), t(y0m), t(d0)
        sd = torch.full((B,), -7, dtype=torch.int32, device=dev)
        mpc.hd.est_initstate_device(xd.data_ptr(), ud.data_ptr(), yd.data_ptr(), sd.data_ptr(), d0=dd.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert np.all(sth == 0) and np.array_equal(sd.cpu().numpy(), sth) and np.array_equal(xd.cpu().numpy(), xh)
    assert not np.any(xh == 3.0)
