"""Helpers of the steady-state Riccati solve tests (csrc/kf_dare_bodies.h behind mpcqp_kf_set_steady): SciPy's
solution of the predictor DARE as the reference, and the case runners that tests/test_kf_dare.py (emulator: the launcher of
tests/emu/emu_kf_dare.cpp in tests/emu/libmpcqp_emu_est.so, tests/emu_util.py) and tests/test_gpu_kf_dare.py (HIP library)
share."""
import warnings

import numpy as np

import mpcqp
from mpcqp import synth
from tests import kf_util as ku

MAX_ITER = 40           # DARE_MAX_ITER of csrc/kf_dare_launch.h


def scipy_dare(sh):
    """(K̂, P̂∞) of every member from scipy.linalg.solve_discrete_are: what mpcqp.steady_kalman_gain computes, with P̂ kept."""
    from scipy.linalg import solve_discrete_are
    B = sh["Ahat"].shape[0]
    i_ym = np.asarray(sh["i_ym"], int)
    K, P = np.empty((B, sh["nxh"], len(i_ym))), np.empty((B, sh["nxh"], sh["nxh"]))
    for b in range(B):
        Cm = sh["Chat"][b][i_ym]
        P[b] = solve_discrete_are(sh["Ahat"][b].T, Cm.T, sh["Qhat"][b], sh["Rhat"][b])
        K[b] = P[b] @ Cm.T @ np.linalg.inv(Cm @ P[b] @ Cm.T + sh["Rhat"][b])
    return K, P


def make_handle(sh, lib=None, Hp=2, Hc=1, steady=True):
    """A raw C-ABI handle with the shape's model and (steady=True) the gain solved for from the shape's Q̂ and R̂."""
    B = sh["Ahat"].shape[0]
    h = mpcqp.api.Handle(B, sh["nxh"], sh["nu"], sh["ny"], sh["nd"], Hp, Hc, lib=lib)
    set_model(h, sh)
    if steady:
        h.kf_set_steady(sh["Qhat"], sh["Rhat"], sh["i_ym"])
    return h


def set_model(h, sh, Ahat=None):
    cm = mpcqp.api.colmajor
    h.set_model(cm(sh["Ahat"] if Ahat is None else Ahat), cm(sh["Bhu"]), cm(sh["Chat"]), None if not sh["nd"] else cm(sh["Bhd"]),
                None if not sh["nd"] else cm(sh["Dhd"]))


def solve_case(sh, lib=None):
    """Solve on a handle of the shape; returns the handle and the errors of K̂ and P̂∞ against SciPy (ku.rel)."""
    h = make_handle(sh, lib=lib)
    K, P = scipy_dare(sh)
    assert mpcqp.api.steady_kalman_gain(sh["Ahat"], sh["Chat"], sh["Qhat"], sh["Rhat"], sh["i_ym"]).tobytes() == K.tobytes()
    res = dict(eK=ku.rel(h.kf_gain(), K), eP=ku.rel(h.kf_covariance(), P), iters=h.kf_steady_iters().tolist())
    print(res)
    return h, res


def check_against_scipy(shape, lanes, lib=None):
    """Case 1: K̂, P̂∞ within ku.BAR of SciPy, every status 0, iterations within the cap, lanes per estimator."""
    h, res = solve_case(shape(), lib=lib)
    assert not h.kf_status().any(), h.kf_status()
    assert 1 <= min(res["iters"]) and max(res["iters"]) <= MAX_ITER, res
    assert h.kf_lanes_per_estimator() == lanes
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR, res


def small_q_shape(B=5):
    """Case 2: C3 with Q̂ = 1e-6 I, R̂ = I -- slow estimator poles, where a cap or tolerance that only suits benign inputs shows."""
    sh = ku.shape_c3(B=B)
    sh["Qhat"] = np.broadcast_to(1e-6 * np.eye(sh["nxh"]), (B, sh["nxh"], sh["nxh"])).copy()
    sh["Rhat"] = np.broadcast_to(np.eye(len(sh["i_ym"])), (B, len(sh["i_ym"]), len(sh["i_ym"]))).copy()
    return sh


def check_small_q(lib=None):
    h, res = solve_case(small_q_shape(), lib=lib)
    assert not h.kf_status().any() and max(res["iters"]) <= MAX_ITER, (h.kf_status(), res)
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR, res


def undetectable_shape(B=6, member=2):
    """shape_c2 with one member made undetectable: one integrator column of its Ĉ zeroed (the integrator has a pole at 1
    that no measurement sees)."""
    sh = ku.shape_c2(B=B)
    cfg = sh["cfg"]
    sh["Chat"] = sh["Chat"].copy()
    sh["Chat"][member][:, cfg.nx] = 0.0            # the first of the output integrators that follow the plant states
    return sh


def check_independence(lib=None, member=2):
    """Case 3: an undetectable member, then one with Q̂ = -I: its status, its K̂ = 0, the other five bit-equal to the healthy
    batch."""
    healthy = ku.shape_c2(B=6)
    h0 = make_handle(healthy, lib=lib)
    assert not h0.kf_status().any()
    K0, P0 = h0.kf_gain(), h0.kf_covariance()
    others = [i for i in range(6) if i != member]
    bad = undetectable_shape(6, member)
    assert np.abs(np.linalg.eigvals(bad["Ahat"][member])).max() >= 1.0 - 1e-12       # (the integrators)
    h1 = make_handle(bad, lib=lib)
    st = h1.kf_status()
    print("undetectable:", st.tolist(), h1.kf_steady_iters().tolist())
    assert st[member] != 0 and not st[others].any()
    K1, P1 = h1.kf_gain(), h1.kf_covariance()
    assert not K1[member].any() and not P1[member].any()
    assert K1[others].tobytes() == K0[others].tobytes() and P1[others].tobytes() == P0[others].tobytes()
    neg = ku.shape_c2(B=6)
    neg["Qhat"] = neg["Qhat"].copy()
    neg["Qhat"][member] = -np.eye(neg["nxh"])
    h2 = make_handle(neg, lib=lib)
    st = h2.kf_status()
    assert st[member] == 2 and not st[others].any(), st
    K2, P2 = h2.kf_gain(), h2.kf_covariance()
    assert not K2[member].any()
    assert K2[others].tobytes() == K0[others].tobytes() and P2[others].tobytes() == P0[others].tobytes()
    return bad


def check_resolve(lib=None):
    """Case 4: set_model with 0.9 Â leaves the old gain in place; kf_solve_steady then meets SciPy on the new model."""
    sh = ku.shape_c2(B=6)
    h = make_handle(sh, lib=lib)
    K_old = h.kf_gain()
    new = dict(sh, Ahat=0.9 * sh["Ahat"])
    set_model(h, new)
    assert h.kf_gain().tobytes() == K_old.tobytes()
    h.kf_solve_steady()
    K, P = scipy_dare(new)
    assert not h.kf_status().any()
    assert ku.rel(h.kf_gain(), K) <= ku.BAR and ku.rel(h.kf_covariance(), P) <= ku.BAR
    assert ku.rel(h.kf_gain(), K_old) > 1e-6


def closed_loop(lib=None, B=6, nper=5, swap_after=3):
    """Case 5: C2, B = 6, five periods of preparestate / moveinput / updatestate on a controller given steady=dict(Q̂, R̂) against
    the same controller given steady_kalman_gain(...): x̂ within 1e-10, equal step statuses.  Then setmodel on the first
    (0.9 Â) re-solves: K̂ meets SciPy on the new model."""
    from tests.parity_util import make_controller
    cfg = synth.C2
    sh = ku.shape_linmpc(cfg, B, 21)
    bt = sh["bt"]
    a, b = make_controller(cfg, bt, lib=lib), make_controller(cfg, bt, lib=lib)
    a.setestimator(steady=dict(Qhat=sh["Qhat"], Rhat=sh["Rhat"]), xhat0=bt["xhat0"])
    b.setestimator(mpcqp.api.steady_kalman_gain(sh["Ahat"], sh["Chat"], sh["Qhat"], sh["Rhat"]), xhat0=bt["xhat0"])
    a.lastu0, b.lastu0 = bt["lastu0"].copy(), bt["lastu0"].copy()
    xp = bt["xhat0"].copy()
    rng = np.random.default_rng(0)
    ex = 0.0
    for k in range(nper):
        y = np.einsum("bij,bj->bi", bt["Chat"], xp) + 0.02 * rng.standard_normal((B, cfg.ny))
        a.preparestate(y); b.preparestate(y)
        ua, ub = a.moveinput(None, bt["ry"]), b.moveinput(None, bt["ry"])
        assert np.array_equal(a.status, b.status) and np.all(a.status != mpcqp.STATUS_ERROR)
        a.updatestate(ub, y); b.updatestate(ub, y)
        ex = max(ex, float(np.abs(a.xhat0 - b.xhat0).max()))
        xp = np.einsum("bij,bj->bi", bt["Ahat"], xp) + np.einsum("bij,bj->bi", bt["Bhu"], ub)
    print("closed loop: max |x̂ - x̂ref| =", ex)
    assert ex <= 1e-10, ex
    info = a.getinfo()
    K, P = scipy_dare(sh)
    assert ku.rel(info["K̂"], K) <= ku.BAR and ku.rel(info["P̂"], P) <= ku.BAR and not info["kf_status"].any()
    new = dict(sh, Ahat=0.9 * sh["Ahat"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                 # (every member solvable: no warning)
        a.setmodel(new["Ahat"], bt["Bhu"], bt["Chat"])
    Kn, _ = scipy_dare(new)
    assert ku.rel(a.hd.kf_gain(), Kn) <= ku.BAR and ku.rel(a.hd.kf_gain(), K) > 1e-6
    return a


def check_warning(lib=None):
    """Case 5, last part: the batch of case 3 produces one RuntimeWarning with the count of members without a gain."""
    import pytest
    from tests.parity_util import make_controller
    sh = undetectable_shape(6, 2)
    bt = dict(sh["bt"], Chat=sh["Chat"])
    c = make_controller(sh["cfg"], bt, lib=lib)
    with pytest.warns(RuntimeWarning, match=r"\(1 of 6 estimators\)") as rec:
        c.setestimator(steady=dict(Qhat=sh["Qhat"], Rhat=sh["Rhat"]))
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert c.hd.kf_status()[2] != 0
