"""`BatchLinMPC.sim` / mpcqp_sim on the MI355X (csrc/sim_kernels.hip between the device entry points of the estimator and the
controller): the checks of tests/test_sim.py on the HIP library, at the same bars, and the device entry point on torch buffers."""
import numpy as np
import pytest

import mpcqp
from tests import sim_util as su
from tests import test_sim as ts

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", list(ts.VARIANTS))
@pytest.mark.parametrize("kind", su.KINDS)
def test_per_period_path_against_reference(hiplib, kind, variant):
    ts.check_against_reference(None, kind, variant)


@pytest.mark.parametrize("name", list(ts.FUSED_CASES))
def test_fused_path_against_per_period_path(hiplib, name):
    ts.check_fused_against_per_period(None, name)


@pytest.mark.parametrize("name", list(ts.FALLBACKS))
def test_not_eligible_takes_the_per_period_path(hiplib, name):
    ts.check_fallback(None, name)


@pytest.mark.parametrize("kind", ["explicit_law", "explicit_law_per_period", "explicit_step", "linmpc", "linmpc_umax"])
def test_member_equals_itself_alone(hiplib, kind):
    if kind == "explicit_law_per_period":
        return ts.check_member_alone(None, "explicit_law", fuse=False)
    ts.check_member_alone(None, kind)


@pytest.mark.parametrize("kind,kw", [("explicit_law", dict()), ("explicit_law", dict(direct=False)), ("explicit_law", dict(fuse=False)),
                                     ("explicit_law", dict(ry_per_period=True)), ("explicit_step", dict(estimator="tv")),
                                     ("linmpc_umax", dict(warm_dual=True)), ("linmpc", dict(direct=False))])
def test_two_runs_of_three_equal_one_of_six(hiplib, kind, kw):
    ts.check_two_halves(None, kind, **kw)


@pytest.mark.parametrize("kind,kw", [("explicit_law", dict()), ("explicit_law", dict(fuse=False)), ("linmpc", dict())])
def test_nan_measurement_skips_one_members_correction(hiplib, kind, kw):
    ts.check_nan(None, kind, **kw)


@pytest.mark.parametrize("kind,kw", [("explicit_law", dict()), ("explicit_law", dict(fuse=False)), ("explicit_step", dict())])
def test_explicit_status_2_member(hiplib, kind, kw):
    ts.check_status_policy(None, kind, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(fuse=False)])
def test_results_do_not_depend_on_explicit_waves(hiplib, monkeypatch, kw):
    ts.check_waves(None, monkeypatch, **kw)


def test_refusals_and_seeded_draws(hiplib):
    ts.check_refusals(None)


def test_device_entry_point_on_torch_buffers(hiplib):
    """mpcqp_sim_device on torch buffers, B = 67 (C3 plant dimensions: groups of 16 lanes, 17 wavefronts, the last one with
    three of its four groups in use), asynchronous on torch's stream; against the host-pointer call, bit for bit, on the
    single-launch path and with MPCQP_SIM_FLAG_NO_FUSE."""
    import torch
    case = su.Case("explicit_law", dims=dict(nx=12, nu=4, ny=4, Hp=6, Hc=2), B=67, N=3, seed=5)
    for fuse in (True, False):
        _device_against_host(case, fuse)


def _device_against_host(case, fuse):
    import torch
    host = su.run(case.controller(), **{**case.args(), "fuse": fuse})
    assert host.path == (mpcqp.api.SIM_PATH_FUSED if fuse else mpcqp.api.SIM_PATH_PERIOD)
    mpc = case.controller()
    mpc._sim_plant(case.plant)
    B, N, nxp = case.B, case.N, case.nxp
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    abi = lambda w: t(w.transpose(0, 2, 1))
    o = case.bt["ops"]
    inp = dict(ry=t(case.ry - o["yop"]), d=t(case.d - o["dop"]), u_step=t(case.kw["u_step"]), y_step=t(case.kw["y_step"]),
               d_step=t(case.kw["d_step"]), sigma_u=t(case.kw["u_noise"]), sigma_y=t(case.kw["y_noise"]), sigma_d=t(case.kw["d_noise"]),
               sigma_x=t(case.kw["x_noise"]), w_u=abi(case.draws["w_u"]), w_y=abi(case.draws["w_y"]), w_d=abi(case.draws["w_d"]),
               w_x=abi(case.draws["w_x"]), x0=t(case.x_0 - case.plant["xop"]), xhat0=t(case.xhat_0 - o["xhop"]), lastu0=t(case.lastu - o["uop"]))
    new = lambda n, dt=torch.float64: torch.full((B, N, n), -7, dtype=dt, device=dev)
    rec = dict(Y=new(4), X=new(nxp), D=new(1), Xhat=new(16), Yhat=new(4), U=new(4), Ud=new(4))
    st = torch.full((B, N), -7, dtype=torch.int32, device=dev)
    mpc.hd.sim_device(N, flags=0 if fuse else mpcqp.api.SIM_FLAG_NO_FUSE, stream=torch.cuda.current_stream().cuda_stream, status=st.data_ptr(),
                      **{k: v.data_ptr() for k, v in {**inp, **rec}.items()})
    torch.cuda.synchronize()
    g = lambda a: a.cpu().numpy().transpose(0, 2, 1)
    assert np.all(st.cpu().numpy() == 0)
    for k, name, op in (("Y", "Y_data", o["yop"]), ("X", "X_data", case.plant["xop"]), ("D", "D_data", o["dop"]), ("Xhat", "X̂_data", o["xhop"]),
                        ("Yhat", "Ŷ_data", o["yop"]), ("U", "U_data", o["uop"]), ("Ud", "Ud_data", o["uop"])):
        op = np.broadcast_to(op, (B, rec[k].shape[2]))
        assert np.array_equal(g(rec[k]) + op[:, :, None], getattr(host, name)), k
