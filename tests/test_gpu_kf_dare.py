"""GPU tests of the SteadyKalmanFilter built from Q̂ and R̂ (csrc/kf_kernels.hip: k_kf_dare<NX> with four estimators per
wavefront, k_kf_dare_wide<NX> with one and the products on the matrix cores) through the C-ABI and the BatchLinMPC mirror.

K̂ and P̂∞ are compared with SciPy's solve_discrete_are (what mpcqp.steady_kalman_gain uses) at tests/kf_util.BAR, 1e-11
relative to max(1, max|.|): a NumPy restatement of the same iteration sits at 1e-14 / 5.3e-14 on these generators, which
leaves two decades for the operation order and the summation of the matrix cores."""
import numpy as np
import pytest

import mpcqp
from mpcqp import synth
from tests import kf_dare_util as du
from tests import kf_util as ku

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,lanes", [(ku.shape_c2, 16), (ku.shape_c3, 16), (ku.shape_17, 64), (ku.shape_32, 64)],
                         ids=["C2-B6", "C3-B7", "nx17-B3", "nx32-B3"])
def test_gain_against_scipy(hiplib, shape, lanes):
    du.check_against_scipy(shape, lanes)


def test_small_process_noise(hiplib):
    """C3 with Q̂ = 1e-6 I, R̂ = I, B = 5: status 0, within the bar, within the cap."""
    du.check_small_q()


def test_members_are_independent(hiplib):
    """An undetectable member and a member with Q̂ = -I: a status, a zero gain, and neighbours that keep their bits."""
    du.check_independence()


def test_resolve_after_set_model(hiplib):
    du.check_resolve()


def test_controller(hiplib):
    """BatchLinMPC with steady=dict(Q̂, R̂) against the same controller given steady_kalman_gain; setmodel re-solves; the warning."""
    du.closed_loop()
    du.check_warning()


def test_tiled_batch_equals_its_twin(hiplib):
    """The seven models of C3 tiled to B = 1027 (257 groups: several wavefronts, the grid-stride loop where the grid is
    capped, a last group of three): every member bit-equal to its twin of the B = 7 batch."""
    sh = ku.shape_c3(B=7)
    h7 = du.make_handle(sh)
    B = 1027
    idx = np.arange(B) % 7
    big = dict(sh, **{k: np.ascontiguousarray(sh[k][idx]) for k in ("Ahat", "Bhu", "Chat", "Qhat", "Rhat")})
    hb = du.make_handle(big)
    assert not h7.kf_status().any() and not hb.kf_status().any()
    assert np.array_equal(hb.kf_steady_iters(), h7.kf_steady_iters()[idx])
    assert hb.kf_gain().tobytes() == h7.kf_gain()[idx].tobytes()
    assert hb.kf_covariance().tobytes() == h7.kf_covariance()[idx].tobytes()


def test_fused_loop_equals_separate_calls(hiplib):
    """mpcqp_loop_device on a handle whose gain was solved for on the device, B = 64, five periods, device buffers: the fused
    period against kf_correct_device + step_device + kf_predict_device, exactly 0.0 apart; no launch touches K̂ on the way."""
    import torch
    dev = torch.device("cuda", 0)
    B, periods = 64, 5
    cfg = synth.Config("loop", nx=3, nu=2, ny=2, Hp=8, Hc=3, umin=-0.6, umax=0.7, ymax=0.9)
    sh = ku.shape_linmpc(cfg, B, 12)
    bt = sh["bt"]
    K_ref, _ = du.scipy_dare(sh)

    def make():
        hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, cfg.Hc, neps=1, flags=mpcqp.FLAG_RY_CONSTANT | mpcqp.FLAG_KEEP_QP)
        hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
        hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt), np.full(B, cfg.Cwt))
        hd.set_bounds(U0min=np.full((B, hd.nU), cfg.umin), U0max=np.full((B, hd.nU), cfg.umax), Y0max=np.full((B, hd.nY), cfg.ymax))
        hd.kf_set_steady(sh["Qhat"], sh["Rhat"], sh["i_ym"])
        hd.prepare()
        return hd

    new = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr, host = (lambda a: a.data_ptr()), (lambda a: a.cpu().numpy())
    runs = []
    for fused in (False, True):
        hd = make()
        assert not hd.kf_status().any() and ku.rel(hd.kf_gain(), K_ref) <= ku.BAR
        K0 = hd.kf_gain()
        x, lu, ry = new(bt["xhat0"]), new(bt["lastu0"]), new(bt["ry"])
        Z, u0 = new(np.zeros((B, hd.nZ))), new(np.zeros((B, cfg.nu)))
        st, it = new(np.zeros(B, np.int32)), new(np.zeros(B, np.int32))
        rg = np.random.default_rng(7)
        out = []
        for _ in range(periods):
            y = new(0.3 * rg.standard_normal((B, cfg.ny)))
            if fused:
                hd.loop_device(ptr(x), ptr(y), ptr(lu), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
            else:
                hd.kf_correct_device(ptr(x), ptr(y))
                hd.step_device(ptr(x), ptr(lu), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
                hd.kf_predict_device(ptr(x), ptr(u0))
            torch.cuda.synchronize()
            assert np.all(host(st) == 0)
            out.append((host(x).copy(), host(u0).copy(), host(Z).copy()))
            lu, u0 = u0, lu                      # u0 of this period is lastu0 of the next
        assert hd.kf_gain().tobytes() == K0.tobytes() and not hd.kf_status().any()
        runs.append(out)
    diff = max(float(np.abs(a - b).max()) for pa, pb in zip(*runs) for a, b in zip(pa, pb))
    assert diff == 0.0, diff
    assert max(float(np.abs(p[0]).max()) for p in runs[0]) > 1e-2
