"""GPU tests of the SteadyKalmanFilter built from Q̂ and R̂ for 32 < max(nx̂, nym) <= 64 (csrc/kf_dare_lds_kernels.hip:
k_kf_dare_lds<N, T>, operands in LDS, one estimator per workgroup of T wavefronts, the products on the matrix cores) through the
C-ABI and the BatchLinMPC mirror.  The CPU twins of the first six cases are in tests/test_kf_dare_lds.py.

K̂ and P̂∞ are compared with SciPy's solve_discrete_are at tests/kf_util.BAR, 1e-11 relative to max(1, max|.|): a NumPy
restatement of the same iteration sits at 4.4e-15 / 3.5e-14 on these generators, which leaves two decades for the operation
order and the summation of the matrix cores."""
import numpy as np
import pytest

import mpcqp
from tests import kf_dare_lds_util as lu
from tests import kf_dare_util as du
from tests import kf_util as ku

pytestmark = pytest.mark.gpu

TEAMS = ("1", "2", "4")


@pytest.mark.parametrize("shape_id", list(lu.SHAPES))
def test_gain_against_scipy(hiplib, shape_id):
    """One shape per padded order and per edge; a workgroup of four wavefronts per estimator (256 lanes).  The library before
    these kernels answers -4 for every one of these shapes."""
    lu.check_against_scipy(shape_id, 256)


def test_small_process_noise(hiplib):
    """nx̂ = 40 with Q̂ = 1e-6 I, R̂ = I: status 0, within the bar, within the cap."""
    lu.check_small_q()


def test_members_are_independent(hiplib):
    """nx̂ = 33, B = 6: an undetectable member, one with Q̂ = -I and one with a rank-5 Q̂ get a status and zeros, their neighbours
    the bits of the healthy batch, the mirror one warning with the count."""
    lu.check_independence()


def test_resolve_after_set_model(hiplib):
    lu.check_resolve()


def test_controller(hiplib):
    """BatchLinMPC at nx̂ = 40 with steady=dict(Q̂, R̂) against the same controller given steady_kalman_gain; setmodel re-solves."""
    lu.closed_loop()


def test_what_stays_refused(hiplib):
    """kf_set_covariances and est_initstate answer -4 on the wide handle, which keeps its solved gain."""
    lu.check_still_refused()


def test_tiled_batch_equals_its_twin(hiplib):
    """The three models of the nx̂ = 64 shape tiled to B = 3 x (workgroups of the persistent grid) + 2: the grid-stride loop with a
    last round that is partly filled.  Every member's K̂, P̂∞ and iteration count bit-equal to its twin of the B = 3 batch."""
    import torch
    sh, _, _ = lu.reference("nx64-nym8-nd1")
    _, g3 = lu.solved(sh)
    grid = torch.cuda.get_device_properties(0).multi_processor_count       # (kf_dare_lds_waves_for: one workgroup per CU)
    B = 3 * grid + 2
    idx = np.arange(B) % 3
    big = dict(sh, **{k: np.ascontiguousarray(sh[k][idx]) for k in ("Ahat", "Bhu", "Chat", "Bhd", "Dhd", "Qhat", "Rhat")})
    _, gb = lu.solved(big)
    assert not g3["status"].any() and not gb["status"].any()
    assert np.array_equal(gb["iters"], g3["iters"][idx])
    assert gb["K"].tobytes() == g3["K"][idx].tobytes()
    assert gb["P"].tobytes() == g3["P"][idx].tobytes()


@pytest.mark.parametrize("shape_id", ["nx33-nym3", "nx64-nym8-nd1"])
def test_team_size_invariance(hiplib, monkeypatch, shape_id):
    """K̂, P̂∞, status and iterations at MPCQP_KF_DARE_TEAM = 1, 2, 4 and at the default are bit-identical: one wavefront has no
    cross-wave hazard, so a barrier that is missing between the wavefronts of a team shows here.  An unknown value is ignored."""
    sh, K, P = lu.reference(shape_id)
    monkeypatch.delenv("MPCQP_KF_DARE_TEAM", raising=False)
    h0, g0 = lu.solved(sh)
    assert h0.kf_lanes_per_estimator() == 256 and not g0["status"].any()
    assert ku.rel(g0["K"], K) <= ku.BAR and ku.rel(g0["P"], P) <= ku.BAR
    for team in TEAMS + ("3",):
        monkeypatch.setenv("MPCQP_KF_DARE_TEAM", team)
        h, g = lu.solved(sh)
        assert h.kf_lanes_per_estimator() == 64 * (int(team) if team in TEAMS else 4)
        for k in ("K", "P", "status", "iters"):
            assert g[k].tobytes() == g0[k].tobytes(), (team, k)
    # read at every solve: the same handle, another team
    monkeypatch.setenv("MPCQP_KF_DARE_TEAM", "1")
    h0.kf_solve_steady()
    assert h0.kf_lanes_per_estimator() == 64 and h0.kf_gain().tobytes() == g0["K"].tobytes()


def test_fused_loop_equals_separate_calls(hiplib):
    """mpcqp_loop_device on the nx̂ = 40 handle whose gain was solved for on the device, B = 16, three periods, device buffers:
    the fused period against kf_correct_device + step_device + kf_predict_device, exactly 0.0 apart; no launch touches K̂ on
    the way."""
    import torch
    dev = torch.device("cuda", 0)
    B, periods = 16, 3
    cfg = lu.CFG40
    sh = ku.shape_linmpc(cfg, B, 12)
    bt = sh["bt"]
    K_ref, _ = du.scipy_dare(sh)

    def make():
        hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, cfg.Hc, neps=1, flags=mpcqp.FLAG_RY_CONSTANT | mpcqp.FLAG_KEEP_QP)
        hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
        hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt), np.full(B, cfg.Cwt))
        hd.set_bounds(U0min=np.full((B, hd.nU), -0.6), U0max=np.full((B, hd.nU), 0.7), Y0max=np.full((B, hd.nY), 0.9))
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
        x, lu0, ry = new(bt["xhat0"]), new(bt["lastu0"]), new(bt["ry"])
        Z, u0 = new(np.zeros((B, hd.nZ))), new(np.zeros((B, cfg.nu)))
        st, it = new(np.zeros(B, np.int32)), new(np.zeros(B, np.int32))
        rg = np.random.default_rng(7)
        out = []
        for _ in range(periods):
            y = new(0.3 * rg.standard_normal((B, cfg.ny)))
            if fused:
                hd.loop_device(ptr(x), ptr(y), ptr(lu0), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
            else:
                hd.kf_correct_device(ptr(x), ptr(y))
                hd.step_device(ptr(x), ptr(lu0), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
                hd.kf_predict_device(ptr(x), ptr(u0))
            torch.cuda.synchronize()
            assert np.all(host(st) == 0)
            out.append((host(x).copy(), host(u0).copy(), host(Z).copy()))
            lu0, u0 = u0, lu0                    # u0 of this period is lastu0 of the next
        assert hd.kf_gain().tobytes() == K0.tobytes() and not hd.kf_status().any()
        runs.append(out)
    diff = max(float(np.abs(a - b).max()) for pa, pb in zip(*runs) for a, b in zip(pa, pb))
    assert diff == 0.0, diff
    assert max(float(np.abs(p[0]).max()) for p in runs[0]) > 1e-2
