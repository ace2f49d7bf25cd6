"""Helpers of the tests of the steady-state Riccati solve for 32 < max(nx̂, nym) <= 64 (csrc/kf_dare_lds_bodies.h behind
mpcqp_kf_set_steady: operands in LDS, one estimator per workgroup): the shapes -- one per padded order and per edge -- and the
case runners that tests/test_kf_dare_lds.py (emulator: the launcher of tests/emu/emu_kf_dare_lds.cpp in
tests/emu/libmpcqp_emu_est_lds.so, built by tests/emu/dare_lds.mk) and tests/test_gpu_kf_dare_lds.py (HIP library) share.
The reference is SciPy's solve_discrete_are (kf_dare_util.scipy_dare) at tests/kf_util.BAR."""
import os
import subprocess
import warnings

import numpy as np

import mpcqp
from mpcqp import synth
from tests import emu_util
from tests import kf_dare_util as du
from tests import kf_util as ku

EST_LDS = "libmpcqp_emu_est_lds.so"
MAX_ITER = du.MAX_ITER


def build_emulator():
    """tests/emu/libmpcqp_emu_est_lds.so: libmpcqp_emu_est.so + the launcher of the LDS-resident solve; returns its path."""
    subprocess.check_call(["make", "-s", "-j8", "-C", emu_util.EMU, "-f", "dare_lds.mk", EST_LDS])
    return os.path.join(emu_util.EMU, EST_LDS)


# ---------------------------------------------------------------------------------------------
# shapes (B = 3, dense symmetric positive definite Q̂ and R̂): nx̂, nym -> padded order N
MHE33 = synth.MheConfig("kf nx̂=33", nx=30, nu=2, nym=3, nd=0, He=1)       # first size past 32; N = 48 with 15 padded rows
MHE48 = synth.MheConfig("kf nx̂=48", nx=42, nu=2, nym=6, nd=0, He=1)       # N = 48 without padding
MHE49 = synth.MheConfig("kf nx̂=49", nx=43, nu=2, nym=6, nd=0, He=1)       # N = 64 with 15 padded rows
MHE64 = synth.MheConfig("kf nx̂=64", nx=56, nu=2, nym=8, nd=1, He=1)       # N = 64 full
MHE40 = synth.MheConfig("kf nx̂=40 nym=20", nx=20, nu=2, nym=20, nd=0, He=1)   # the nym x nym inverse of the gain spans two tiles
CFG40 = synth.Config("nx̂=40", nx=36, nu=3, ny=4, Hp=6, Hc=2)               # the controller path
CFG33 = synth.Config("nx̂=33", nx=30, nu=2, ny=3, Hp=6, Hc=2)               # refusals, with a controller for the warning

SHAPES = {
    "nx33-nym3": lambda B=3: ku.shape_mhe(MHE33, B, 5),
    "nx48-nym6": lambda B=3: ku.shape_mhe(MHE48, B, 5),
    "nx49-nym6": lambda B=3: ku.shape_mhe(MHE49, B, 5),
    "nx64-nym8-nd1": lambda B=3: ku.shape_mhe(MHE64, B, 5),
    "nx40-nym20": lambda B=3: ku.shape_mhe(MHE40, B, 5),
    "nx40-linmpc": lambda B=3: ku.shape_linmpc(CFG40, B, 21),
}

_REF = {}


def _freeze(sh):
    for v in sh.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sh


def reference(shape_id):
    """(shape, K̂, P̂∞ of SciPy): computed once per shape, shared by the tests, never modified."""
    if shape_id not in _REF:
        sh = _freeze(SHAPES[shape_id]())
        K, P = du.scipy_dare(sh)
        K.setflags(write=False); P.setflags(write=False)
        _REF[shape_id] = (sh, K, P)
    return _REF[shape_id]


def solved(sh, lib=None):
    """A handle of the shape with its gain solved for, and the read-backs of the solve."""
    h = du.make_handle(sh, lib=lib)
    return h, dict(K=h.kf_gain(), P=h.kf_covariance(), status=h.kf_status(), iters=h.kf_steady_iters(), path=h.kf_steady_path())


def check_against_scipy(shape_id, lanes, lib=None):
    """Case 1: status 0, 1 <= iters <= 40, K̂ and P̂∞ within ku.BAR of SciPy, lanes per estimator, path 0."""
    sh, K, P = reference(shape_id)
    h, got = solved(sh, lib=lib)
    eK, eP = ku.rel(got["K"], K), ku.rel(got["P"], P)
    print(shape_id, dict(eK=eK, eP=eP, iters=got["iters"].tolist(), status=got["status"].tolist()))
    assert not got["status"].any(), got["status"]
    assert 1 <= got["iters"].min() and got["iters"].max() <= MAX_ITER, got["iters"]
    assert not got["path"].any()
    assert h.kf_lanes_per_estimator() == lanes
    assert eK <= ku.BAR and eP <= ku.BAR, (eK, eP)


def small_q_shape():
    """Case 2: the nx̂ = 40 controller shape with Q̂ = 1e-6 I, R̂ = I -- slow estimator poles."""
    sh = dict(reference("nx40-linmpc")[0])
    B, n, m = sh["Ahat"].shape[0], sh["nxh"], len(sh["i_ym"])
    sh["Qhat"] = np.broadcast_to(1e-6 * np.eye(n), (B, n, n)).copy()
    sh["Rhat"] = np.broadcast_to(np.eye(m), (B, m, m)).copy()
    return sh


def check_small_q(lib=None):
    sh = small_q_shape()
    K, P = du.scipy_dare(sh)
    h, got = solved(sh, lib=lib)
    eK, eP = ku.rel(got["K"], K), ku.rel(got["P"], P)
    print("small Q̂:", dict(eK=eK, eP=eP, iters=got["iters"].tolist()))
    assert not got["status"].any() and got["iters"].max() <= MAX_ITER, got
    assert eK <= ku.BAR and eP <= ku.BAR, (eK, eP)


UNDETECTABLE, NEGATIVE, LOWRANK = 1, 3, 4          # the members of case 3 that must be refused (B = 6)


def refused_shapes():
    """Case 3, nx̂ = 33, B = 6: the healthy batch and the one in which member 1 is undetectable (the first output integrator's
    column of its Ĉ zeroed, as kf_dare_util.undetectable_shape does), member 3 has Q̂ = -I and member 4 Q̂ = B_w B_w' of rank 5."""
    healthy = ku.shape_linmpc(CFG33, 6, 21)
    bad = dict(healthy, Chat=healthy["Chat"].copy(), Qhat=healthy["Qhat"].copy())
    bad["Chat"][UNDETECTABLE][:, CFG33.nx] = 0.0
    bad["Qhat"][NEGATIVE] = -np.eye(bad["nxh"])
    Bw = np.random.default_rng(5).standard_normal((bad["nxh"], 5))
    bad["Qhat"][LOWRANK] = Bw @ Bw.T
    bad["bt"] = dict(healthy["bt"], Chat=bad["Chat"])
    return healthy, bad


def check_independence(lib=None):
    """Case 3: each refused member has a status (2 for the two Q̂ cases), a zero K̂ and a zero P̂∞; the other three are bit-equal
    to the healthy batch; BatchLinMPC warns once, with the count."""
    import pytest
    from tests.parity_util import make_controller
    healthy, bad = refused_shapes()
    assert np.abs(np.linalg.eigvals(bad["Ahat"][UNDETECTABLE])).max() >= 1.0 - 1e-12       # (the integrators)
    _, g0 = solved(healthy, lib=lib)
    h1, g1 = solved(bad, lib=lib)
    refused = [UNDETECTABLE, NEGATIVE, LOWRANK]
    others = [i for i in range(6) if i not in refused]
    print("refused:", g1["status"].tolist(), g1["iters"].tolist())
    assert not g0["status"].any()
    assert g1["status"][UNDETECTABLE] != 0 and g1["status"][NEGATIVE] == 2 and g1["status"][LOWRANK] == 2, g1["status"]
    assert not g1["status"][others].any() and not g1["path"].any()
    for m in refused:
        assert not g1["K"][m].any() and not g1["P"][m].any()
    assert g1["K"][others].tobytes() == g0["K"][others].tobytes() and g1["P"][others].tobytes() == g0["P"][others].tobytes()
    assert np.array_equal(g1["iters"][others], g0["iters"][others])
    c = make_controller(CFG33, bad["bt"], lib=lib)
    with pytest.warns(RuntimeWarning, match=r"\(3 of 6 estimators\)") as rec:
        c.setestimator(steady=dict(Qhat=bad["Qhat"], Rhat=bad["Rhat"]))
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert np.array_equal(c.hd.kf_status(), g1["status"])


def check_resolve(lib=None):
    """Case 4, first part: set_model with 0.9 Â leaves the old gain in place; kf_solve_steady then meets SciPy on the new model."""
    sh, K0, _ = reference("nx33-nym3")
    h, got = solved(sh, lib=lib)
    assert ku.rel(got["K"], K0) <= ku.BAR
    new = dict(sh, Ahat=0.9 * sh["Ahat"])
    du.set_model(h, new)
    assert h.kf_gain().tobytes() == got["K"].tobytes()
    h.kf_solve_steady()
    K, P = du.scipy_dare(new)
    assert not h.kf_status().any()
    assert ku.rel(h.kf_gain(), K) <= ku.BAR and ku.rel(h.kf_covariance(), P) <= ku.BAR
    assert ku.rel(h.kf_gain(), got["K"]) > 1e-6


def closed_loop(lib=None, B=6, nper=5):
    """Cases 5 and 4 (second part), the protocol of kf_dare_util.closed_loop on the nx̂ = 40 Config: five periods of preparestate /
    moveinput / updatestate on a controller given steady=dict(Q̂, R̂) against the same controller given steady_kalman_gain(...):
    x̂ within 1e-10, equal step statuses.  Then setmodel (0.9 Â) solves again, without a warning: K̂ meets SciPy on the new model."""
    from tests.parity_util import make_controller
    cfg = CFG40
    sh = ku.shape_linmpc(cfg, B, 21)
    bt = sh["bt"]
    a, b = make_controller(cfg, bt, lib=lib), make_controller(cfg, bt, lib=lib)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a.setestimator(steady=dict(Qhat=sh["Qhat"], Rhat=sh["Rhat"]), xhat0=bt["xhat0"])
    b.setestimator(mpcqp.api.steady_kalman_gain(sh["Ahat"], sh["Chat"], sh["Qhat"], sh["Rhat"]), xhat0=bt["xhat0"])
    a.lastu0, b.lastu0 = bt["lastu0"].copy(), bt["lastu0"].copy()
    xp = bt["xhat0"].copy()
    rng = np.random.default_rng(0)
    ex = 0.0
    for _ in range(nper):
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
    K, P = du.scipy_dare(sh)
    assert ku.rel(info["K̂"], K) <= ku.BAR and ku.rel(info["P̂"], P) <= ku.BAR and not info["kf_status"].any()
    new = dict(sh, Ahat=0.9 * sh["Ahat"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                 # (every member solvable: no warning)
        a.setmodel(new["Ahat"], bt["Bhu"], bt["Chat"])
    Kn, _ = du.scipy_dare(new)
    assert ku.rel(a.hd.kf_gain(), Kn) <= ku.BAR and ku.rel(a.hd.kf_gain(), K) > 1e-6
    return a


def check_still_refused(lib=None):
    """Case 6: on the solved nx̂ = 33 handle the time-varying KalmanFilter and initstate keep their limit of 32 (-4), and the
    handle keeps its solved gain, bit for bit."""
    import pytest
    sh, _, _ = reference("nx33-nym3")
    h, got = solved(sh, lib=lib)
    B = sh["Ahat"].shape[0]
    with pytest.raises(mpcqp.MpcqpError, match="-4"):
        h.kf_set_covariances(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
    x = np.zeros((B, sh["nxh"]))
    with pytest.raises(mpcqp.MpcqpError, match="-4"):
        h.est_initstate(x, np.zeros((B, sh["nu"])), np.zeros((B, len(sh["i_ym"]))))
    assert not x.any()
    assert h.kf_gain().tobytes() == got["K"].tobytes() and h.kf_covariance().tobytes() == got["P"].tobytes()
    assert not h.kf_status().any() and np.array_equal(h.kf_steady_iters(), got["iters"])
    h.kf_solve_steady()                                # (still a steady handle)
    assert h.kf_gain().tobytes() == got["K"].tobytes()
