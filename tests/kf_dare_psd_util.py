"""Helpers of the tests of the steady-state Riccati solve with a positive SEMIdefinite Q̂ (csrc/kf_dare_bodies.h in its square-root form: the
second pass behind mpcqp_kf_set_steady): the generators of such Q̂ on the shapes of tests/kf_util.py, and the case runners that
tests/test_kf_dare_psd.py (emulator: the launcher of tests/emu/emu_kf_dare_psd.cpp in tests/emu/libmpcqp_emu_est_psd.so, built
by tests/emu/psd.mk) and tests/test_gpu_kf_dare_psd.py (HIP library) share.  The reference is SciPy's solve_discrete_are
(kf_dare_util.scipy_dare) at tests/kf_util.BAR; R̂ is the shape's own."""
import os
import subprocess
import warnings

import numpy as np

import mpcqp
from mpcqp import synth
from tests import emu_util
from tests import kf_dare_util as du
from tests import kf_util as ku

EST_PSD = "libmpcqp_emu_est_psd.so"
MAX_ITER = du.MAX_ITER


def build_emulator():
    """tests/emu/libmpcqp_emu_est_psd.so: libmpcqp_emu_est.so + the launcher of the second pass; returns its path."""
    subprocess.check_call(["make", "-s", "-j8", "-C", emu_util.EMU, "-f", "psd.mk", EST_PSD])
    return os.path.join(emu_util.EMU, EST_PSD)


# ---------------------------------------------------------------------------------------------
# shapes: one per compiled NX (every instantiation is a kernel of its own, with its own spills)
CFG4 = synth.Config("psd nx̂=4", nx=2, nu=1, ny=2, Hp=4, Hc=2)           # NX = 4
CFG12 = synth.Config("psd nx̂=11", nx=8, nu=2, ny=3, Hp=4, Hc=2)         # NX = 12, nx̂ = 11: a padded row and column


def shape_4(B=5, seed=21): return ku.shape_linmpc(CFG4, B, seed)         # a full group and a group of one
def shape_12(B=5, seed=21): return ku.shape_linmpc(CFG12, B, seed)


SHAPES = {"NX4-B5": (shape_4, 16), "NX8-C2-B6": (ku.shape_c2, 16), "NX12-B5": (shape_12, 16), "NX16-C3-B7": (ku.shape_c3, 16),
          "NX24-nx17-B3": (ku.shape_17, 64), "NX32-B3": (ku.shape_32, 64)}


# ---------------------------------------------------------------------------------------------
# generators: sh -> sh with a semidefinite Q̂ (and, for `decoupled`, another Â).  npl plant states precede the integrators.
def _npl(sh):
    return sh["nxh"] - sh["ny"]


def _diag0_q(sh, rng):
    B, nxh, npl = sh["Ahat"].shape[0], sh["nxh"], _npl(sh)
    q = rng.uniform(0.1, 1.0, (B, nxh))
    q[:, 1:npl:2] = 0.0                                  # the odd plant states carry no noise
    return q


def diag0(sh):
    """Q̂ = diag(q): q ~ U(0.1, 1) on the even plant states and on every integrator, 0 on the odd plant states."""
    q = _diag0_q(sh, np.random.default_rng(5))
    return dict(sh, Qhat=np.einsum("bi,ij->bij", q, np.eye(sh["nxh"])))


def lowrank(sh, seed=5):
    """Q̂ = B_w B_w': max(1, npl // 3) standard-normal columns into the plant states, diag(U(0.3, 1)) on the integrators."""
    rng = np.random.default_rng(seed)
    B, nxh, npl = sh["Ahat"].shape[0], sh["nxh"], _npl(sh)
    Bw = rng.standard_normal((B, npl, max(1, npl // 3)))
    Q = np.zeros((B, nxh, nxh))
    Q[:, :npl, :npl] = Bw @ Bw.transpose(0, 2, 1)
    qi = rng.uniform(0.3, 1.0, (B, nxh - npl))
    Q[:, range(npl, nxh), range(npl, nxh)] = qi
    return dict(sh, Qhat=0.5 * (Q + Q.transpose(0, 2, 1)))


def decoupled(sh):
    """States 0 and 1 cut loose from the rest (Â₀₀ = 0.7, Â₁₁ = -0.4) and without noise: Q̂ = diag(0, 0, 1, ..., 1).  P̂∞ is
    singular -- its rows and columns 0, 1 are zero -- so the factorisation drops a column in every iteration."""
    B, nxh = sh["Ahat"].shape[0], sh["nxh"]
    A = sh["Ahat"].copy()
    A[:, :2, :] = 0.0
    A[:, :, :2] = 0.0
    A[:, 0, 0], A[:, 1, 1] = 0.7, -0.4
    q = np.ones(nxh); q[:2] = 0.0
    bt = dict(sh["bt"], Ahat=A) if "bt" in sh else None
    return dict(sh, Ahat=A, Qhat=np.broadcast_to(np.diag(q), (B, nxh, nxh)).copy(), **({"bt": bt} if bt else {}))


def with_indef(sh, member):
    """Member `member` gets Q̂ = diag(1, -1e-3, 1, ...): indefinite beyond any rounding, it must stay status 2."""
    Q = sh["Qhat"].copy()
    q = np.ones(sh["nxh"]); q[1] = -1e-3
    Q[member] = np.diag(q)
    return dict(sh, Qhat=Q)


def with_silent_integrator(sh, member):
    """Member `member` (of a diag0 batch) loses the noise of its first output integrator: an unreachable pole at 1, for which no
    stabilising solution exists (SciPy raises on some such members and returns a P̂ that keeps the pole on others)."""
    Q = sh["Qhat"].copy()
    Q[member, _npl(sh), _npl(sh)] = 0.0
    return dict(sh, Qhat=Q)


GENERATORS = {"diag0": diag0, "lowrank": lowrank, "decoupled": decoupled}


# ---------------------------------------------------------------------------------------------
_REF = {}


def reference(shape_id, gen_id):
    """(shape with the generator's Q̂, K̂, P̂∞ of SciPy): computed once per case, shared, never modified."""
    key = (shape_id, gen_id)
    if key not in _REF:
        sh = GENERATORS[gen_id](SHAPES[shape_id][0]())
        K, P = du.scipy_dare(sh)
        for a in (K, P, sh["Qhat"], sh["Ahat"]):
            a.setflags(write=False)
        _REF[key] = (sh, K, P)
    return _REF[key]


def check_against_scipy(shape_id, gen_id, lib=None):
    """Case 1: status 0, path 1, iterations within the cap, K̂ and P̂∞ within ku.BAR of SciPy; returns the errors."""
    sh, K, P = reference(shape_id, gen_id)
    h = du.make_handle(sh, lib=lib)
    res = dict(eK=ku.rel(h.kf_gain(), K), eP=ku.rel(h.kf_covariance(), P), iters=h.kf_steady_iters().tolist(),
               status=h.kf_status().tolist(), path=h.kf_steady_path().tolist())
    print(shape_id, gen_id, res)
    assert not any(res["status"]), res
    assert all(p == 1 for p in res["path"]), res
    assert 1 <= min(res["iters"]) and max(res["iters"]) <= MAX_ITER, res
    assert h.kf_lanes_per_estimator() == SHAPES[shape_id][1]
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR, res
    return res


def check_rank_one_blocks(lib=None, seeds=range(6)):
    """A rank-one 2 x 2 plant block in Q̂ (nx̂ = 4, B = 7, several seeds: 42 members).  In exact arithmetic the second pivot of Q̂
    is zero; rounding leaves it with either sign, and a positive one gets through the pivot test of the definite body, which
    then answers status 0 with a wrong P̂∞.  Every member has to come from the square-root body (path 1), within the bar."""
    worst = 0.0
    for seed in seeds:
        sh = lowrank(shape_4(B=7, seed=30 + seed), seed=seed)
        K, P = du.scipy_dare(sh)
        h = du.make_handle(sh, lib=lib)
        assert not h.kf_status().any(), (seed, h.kf_status())
        assert h.kf_steady_path().tolist() == [1] * 7, (seed, h.kf_steady_path())
        eK, eP = ku.rel(h.kf_gain(), K), ku.rel(h.kf_covariance(), P)
        worst = max(worst, eK, eP)
        assert eK <= ku.BAR and eP <= ku.BAR, (seed, eK, eP)
    print("rank-one blocks: worst error", worst)


def unreachable_pole_shape(seed, B=7):
    """nx̂ = 4: every plant block is T diag(1, 0.5) T⁻¹ and Q̂'s plant block is v v' with v = T[:, 1] -- a rank-one Q̂ without a
    zero on its diagonal whose noise never reaches the pole at 1.  No stabilising solution exists.  The definite body gets
    through Q̂ for some of these members (a rounding-sized positive pivot) and writes a gain for them."""
    sh = shape_4(B=B, seed=40 + seed)
    rng = np.random.default_rng([seed, 3])
    A, Q = sh["Ahat"].copy(), sh["Qhat"].copy()
    for b in range(B):
        T = rng.standard_normal((2, 2)) + 2.0 * np.eye(2)
        A[b, :2, :2] = T @ np.diag([1.0, 0.5]) @ np.linalg.inv(T)
        Q[b] = np.diag(np.diag(Q[b]))
        Q[b, :2, :2] = np.outer(T[:, 1], T[:, 1])
    return dict(sh, Ahat=A, Qhat=Q, bt=dict(sh["bt"], Ahat=A))


def check_refused_after_first_pass(lib=None, seeds=range(6)):
    """A non-zero status never comes with a gain of that solve: the members of unreachable_pole_shape are refused by the
    square-root body, and those the definite body had served before (status 0, K̂ and P̂∞ written) get zeros back."""
    statuses = []
    for seed in seeds:
        h = du.make_handle(unreachable_pole_shape(seed), lib=lib)
        st = h.kf_status()
        statuses += st.tolist()
        assert st.all() and h.kf_steady_path().all(), (seed, st, h.kf_steady_path())
        assert not h.kf_gain().any() and not h.kf_covariance().any(), seed
    print("unreachable pole at 1:", statuses)


def check_small_definite(lib=None):
    """Q̂ = 1e-11 I at C2 is definite, however small: it stays with the definite body (path 0), within the bar."""
    sh = ku.shape_c2(B=6)
    sh = dict(sh, Qhat=np.broadcast_to(1e-11 * np.eye(sh["nxh"]), sh["Qhat"].shape).copy())
    h = du.make_handle(sh, lib=lib)
    K, P = du.scipy_dare(sh)
    assert not h.kf_status().any() and not h.kf_steady_path().any(), (h.kf_status(), h.kf_steady_path())
    assert ku.rel(h.kf_gain(), K) <= ku.BAR and ku.rel(h.kf_covariance(), P) <= ku.BAR


def check_mixed_wavefront(shape_id, members, lib=None):
    """Case 2: `members` carry their diag0 Q̂, the rest the shape's definite one.  The definite members: path 0 and the bits of
    the all-definite batch; `members`: path 1 and the bits they have in the batch where everyone carries diag0."""
    base = SHAPES[shape_id][0]()
    B = base["Ahat"].shape[0]
    rest = [i for i in range(B) if i not in members]
    semi = diag0(base)
    Q = base["Qhat"].copy()
    Q[members] = semi["Qhat"][members]
    hd, hs, hm = du.make_handle(base, lib=lib), du.make_handle(semi, lib=lib), du.make_handle(dict(base, Qhat=Q), lib=lib)
    assert not hd.kf_status().any() and not hs.kf_status().any() and not hm.kf_status().any()
    assert not hd.kf_steady_path().any() and hs.kf_steady_path().all()
    path = hm.kf_steady_path()
    assert not path[rest].any() and path[members].all(), path
    Kd, Pd, Ks, Ps, Km, Pm = hd.kf_gain(), hd.kf_covariance(), hs.kf_gain(), hs.kf_covariance(), hm.kf_gain(), hm.kf_covariance()
    assert Km[rest].tobytes() == Kd[rest].tobytes() and Pm[rest].tobytes() == Pd[rest].tobytes()
    assert Km[members].tobytes() == Ks[members].tobytes() and Pm[members].tobytes() == Ps[members].tobytes()
    assert np.array_equal(hm.kf_steady_iters()[rest], hd.kf_steady_iters()[rest])
    assert np.array_equal(hm.kf_steady_iters()[members], hs.kf_steady_iters()[members])


def refused_shape(indef=2, silent=4):
    """C2, B = 6, every member with its diag0 Q̂; member `indef` indefinite, member `silent` with the silent integrator."""
    healthy = diag0(ku.shape_c2(B=6))
    return healthy, with_silent_integrator(with_indef(healthy, indef), silent)


def check_still_refused(lib=None, indef=2, silent=4):
    """Case 3: the indefinite member keeps status 2, the silent integrator gets a status too (no stabilising solution
    exists; SciPy raises on some such members and returns a P̂ that keeps the pole on others); both keep zero K̂ and P̂∞, the
    neighbours the bits of the healthy diag0 batch; BatchLinMPC warns once, with the count."""
    import pytest
    from tests.parity_util import make_controller
    healthy, bad = refused_shape(indef, silent)
    h0, h1 = du.make_handle(healthy, lib=lib), du.make_handle(bad, lib=lib)
    assert not h0.kf_status().any()
    st = h1.kf_status()
    print("still refused:", st.tolist(), h1.kf_steady_iters().tolist(), h1.kf_steady_path().tolist())
    others = [i for i in range(6) if i not in (indef, silent)]
    assert st[indef] == 2 and st[silent] != 0 and not st[others].any(), st
    K0, P0, K1, P1 = h0.kf_gain(), h0.kf_covariance(), h1.kf_gain(), h1.kf_covariance()
    for m in (indef, silent):
        assert not K1[m].any() and not P1[m].any()
    assert K1[others].tobytes() == K0[others].tobytes() and P1[others].tobytes() == P0[others].tobytes()
    c = make_controller(bad["cfg"], bad["bt"], lib=lib)
    with pytest.warns(RuntimeWarning, match=r"\(2 of 6 estimators\)") as rec:
        c.setestimator(steady=dict(Qhat=bad["Qhat"], Rhat=bad["Rhat"]))
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert np.array_equal(c.hd.kf_status(), st)


def check_resolve(lib=None):
    """Case 4: set_model(0.9 Â), then kf_solve_steady on a diag0 handle meets SciPy on the new model; so does
    kf_solve_steady_device after one more swap."""
    sh = diag0(ku.shape_c2(B=6))
    h = du.make_handle(sh, lib=lib)
    K_old = h.kf_gain()
    for k, solve in ((1, h.kf_solve_steady), (2, h.kf_solve_steady_device)):
        new = dict(sh, Ahat=0.9 ** k * sh["Ahat"])
        du.set_model(h, new)
        assert h.kf_gain().tobytes() == K_old.tobytes()
        solve()
        K, P = du.scipy_dare(new)
        assert not h.kf_status().any() and h.kf_steady_path().all()
        assert ku.rel(h.kf_gain(), K) <= ku.BAR and ku.rel(h.kf_covariance(), P) <= ku.BAR
        assert ku.rel(h.kf_gain(), K_old) > 1e-6
        K_old = h.kf_gain()


def closed_loop(lib=None, B=6, nper=5):
    """Case 5 (the protocol of kf_dare_util.closed_loop): C2, five periods of preparestate / moveinput / updatestate on a
    controller given steady=dict(Q̂ = diag0, R̂) against its twin given steady_kalman_gain(...): x̂ within 1e-10, equal step
    statuses, no warning, and getinfo()["kf_steady_path"] all 1."""
    from tests.parity_util import make_controller
    cfg = synth.C2
    sh = diag0(ku.shape_linmpc(cfg, B, 21))
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
    assert not info["kf_status"].any() and info["kf_steady_path"].tolist() == [1] * B
    return a


def check_contract(lib=None):
    """Case 6, first part: the return codes of mpcqp_kf_steady_path."""
    import ctypes
    import pytest
    lib = lib or mpcqp.load_library()
    sh = diag0(ku.shape_c2(B=5))
    h = du.make_handle(sh, lib=lib, steady=False)
    out = np.empty(5, np.int32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.mpcqp_kf_steady_path(None, p) == -1 and lib.mpcqp_kf_steady_path(h.h, None) == -1       # MPCQP_ERR_NULL
    assert lib.mpcqp_kf_steady_path(h.h, p) == -5                                                       # no estimator yet
    h.kf_set(np.full((5, 2, sh["nxh"]), 0.1), [0, 1])
    with pytest.raises(mpcqp.MpcqpError, match="-5"):
        h.kf_steady_path()
    h.kf_set_steady(sh["Qhat"], sh["Rhat"], sh["i_ym"])
    assert h.kf_steady_path().tolist() == [1] * 5 and not h.kf_status().any()
    definite = ku.shape_c2(B=5)
    h.kf_set_steady(definite["Qhat"], definite["Rhat"], definite["i_ym"])                               # (zeroed before every solve)
    assert h.kf_steady_path().tolist() == [0] * 5 and not h.kf_status().any()
    h.kf_set_covariances(definite["Qhat"], definite["Rhat"], definite["P0"], definite["i_ym"])           # leaves the mode
    with pytest.raises(mpcqp.MpcqpError, match="-5"):
        h.kf_steady_path()
