"""Shared by tests/test_kf_place.py (CPU wave emulator: the launcher of tests/emu/emu_kf_place.cpp in
tests/emu/libmpcqp_emu_kf_place.so) and tests/test_gpu_kf_place.py (MI355X): a NumPy restatement of the pole placement of the
Luenberger observer (csrc/kf_place_bodies.h behind mpcqp_kf_set_poles), the generators, and the checks both twins run.

The restatement (`place_ref`) follows the kernel step by step -- Householder QR without pivoting with the same sign rule, the
projector as "reflect, zero, reflect back", the same start, sweep, stop rule and rank test -- with NumPy's dot products in
place of the wave reductions, so the two differ in rounding only.

The bar of a placement (`pole_check`) is Bauer-Fike: with M = Â (I - K̂ Ĉm) from the returned gain and V its unit-column
eigenvectors,
    max |sort(eig M) - sort(p)| <= TAU cond2(V) eps (|F|2 + |G|2 |K̂|2),     F = Â', G = (Ĉm Â)'.
TAU is 8 times the largest ratio  lhs / (cond2(V) eps (|F|2 + |G|2 |K̂|2))  that the RESTATEMENT shows on the inputs of the
tests themselves (`CASES`, `DEFAULT_POLE_CASES`, `REPEATED`); the factor 8 is for a reduction order that differs from
NumPy's, the conditioning is in the bound already.  Measured (tests/test_kf_place.py::test_restatement_sets_tau prints and
pins them): largest ratio 0.269, at (n, m) = (4, 2); 0.241 at (3, 1), 0.25 at (3, 4), at most 0.02 from n = 9 on.  TAU = 8 x 0.269
rounded up.

The seeds of the sweep test (`SWEEP_CASES`) are such that the restatement's cond2(X) at cap 0 is at least 4 times its
cond2(X) at cap 30 for every member (test_kf_place.py::test_restatement_sweeps_improve_conditioning pins that); the ratios are
written next to them."""
import os
import subprocess
import warnings

import numpy as np

import mpcqp
from mpcqp import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
LIB = "libmpcqp_emu_kf_place.so"
EPS = np.finfo(float).eps
TAU = 2.2               # 8 x 0.269 (see above)
CAP = 30                # PLACE_CAP_DEFAULT of csrc/kf_place_launch.h
DET_RTOL, VEC_TOL = 1e-3, 1e-8
# (n, m, B) of "the poles are placed"
CASES = [(3, 1, 5), (4, 2, 6), (9, 3, 5), (16, 4, 7), (17, 5, 3), (32, 8, 3), (5, 5, 3), (3, 4, 3)]
DEFAULT_POLE_CASES = [(4, 2, 4), (16, 4, 3)]
# (n, m, B, seed): per-member ratios cond X(cap 0) / cond X(cap 30) of the restatement: 5.24 ... 218 and 15.6 ... 144.  The
# eigenvectors V of Â (I - K̂ Ĉm) are the columns of X'^-1 scaled to unit length, so cond2(V) follows cond2(X) without being
# equal to it; with these seeds the restatement's own cond2(V) is at most 0.65 c* at cap 30 and at least 2.3 c* at cap 0.
SWEEP_CASES = [(9, 3, 6, 298), (12, 4, 6, 140)]


def build():
    """make tests/emu/libmpcqp_emu_kf_place.so (tests/emu/kf_place.mk); returns its path."""
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "kf_place.mk", LIB])
    return os.path.join(EMU, LIB)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _hqr(M):
    """Householder QR without pivoting of the columns of M (n x k, k <= n): normalised reflectors V (H_p = I - v_p v_p'), the
    triangle R (k x k) and |R_pp|."""
    M = np.array(M, float)
    n, k = M.shape
    V, d = np.zeros((n, k)), np.zeros(k)
    for p in range(k):
        x = M[p:, p].copy()
        sigma = float(x @ x)
        akk = x[0]
        nrm = np.sqrt(sigma)
        alpha = -nrm if akk >= 0.0 else nrm
        v = np.zeros(n)
        v[p:] = x
        v[p] = akk - alpha
        den = sigma - alpha * akk
        vs = v / np.sqrt(den) if den > 0.0 else np.zeros(n)
        M[:, p + 1:] -= np.outer(vs, vs @ M[:, p + 1:])
        M[p, p] = alpha
        M[p + 1:, p] = 0.0
        V[:, p], d[p] = vs, nrm
    return V, M[:k], d


def _singular(d):
    return bool(np.isnan(d).any() or not d.min() > 64.0 * EPS * d.max())


def _fwd(V, y):
    for k in range(V.shape[1]):
        y = y - V[:, k] * (V[:, k] @ y)
    return y


def _rev(V, y):
    for k in range(V.shape[1] - 1, -1, -1):
        y = y - V[:, k] * (V[:, k] @ y)
    return y


def place_one(A, Cm, lam, cap=CAP):
    """One member: dict(status, K (n, m) or None, sweeps, X)."""
    n, m = A.shape[0], Cm.shape[0]
    mm, q = min(n, m), n - min(n, m)
    out = dict(status=2, K=None, sweeps=0, X=None)
    with np.errstate(all="ignore"):
        G = (Cm @ A).T[:, :mm]
        VG, Z, d = _hqr(G)
        if _singular(d):
            return out
        Q = np.stack([_rev(VG, e) for e in np.eye(n)], axis=1)
        X = np.eye(n)
        detp = 0.0
        if q > 0:
            U1 = Q[:, mm:]
            AU = A @ U1
            W = []
            for j in range(n):
                Vt, _, d = _hqr(AU - lam[j] * U1)
                if _singular(d):
                    return out
                W.append(Vt)
            proj = lambda j, y: _rev(W[j], np.where(np.arange(n) < q, 0.0, _fwd(W[j], y)))
            for j in range(n):
                X[:, j] = 0.0
                for t in range(n):
                    v = proj(j, np.eye(n)[(j + t) % n])
                    nv = np.sqrt(v @ v)
                    if nv >= VEC_TOL:
                        X[:, j] = v / nv
                        break
            detp = float(np.prod(_hqr(X)[2]))
            for s in range(1, cap + 1):
                for j in range(n):
                    Vx = _hqr(np.delete(X, j, axis=1))[0]
                    y = _rev(Vx, np.eye(n)[n - 1])
                    v = proj(j, y)
                    nv = np.sqrt(v @ v)
                    if nv >= VEC_TOL:
                        X[:, j] = v / nv
                det = float(np.prod(_hqr(X)[2]))
                out["sweeps"] = s
                if abs(det - detp) <= DET_RTOL * det:
                    break
                detp = det
        out["X"] = X
        Vx, R, d = _hqr(X)
        if _singular(d):
            return out
        S = np.linalg.solve(R.T, lam[:, None] * X.T)
        Mt = np.stack([_rev(Vx, S[:, c]) for c in range(n)], axis=1)
        Wt = (A - Mt) @ Q[:, :mm]
        K = np.zeros((n, m))
        K[:, :mm] = np.linalg.solve(Z, Wt.T).T
        if not np.isfinite(K).all():
            return out
    out.update(status=0, K=K)
    return out


def place_ref(case, cap=CAP):
    """The whole batch: dict(K (B,n,m) zeros where refused, status, sweeps, condX)."""
    A, Cm, P = case["Ahat"], case["Chat"][:, case["i_ym"]], case["poles"]
    res = [place_one(A[b], Cm[b], P[b], cap) for b in range(A.shape[0])]
    n, m = A.shape[1], Cm.shape[1]
    return dict(K=np.stack([r["K"] if r["status"] == 0 else np.zeros((n, m)) for r in res]),
                status=np.array([r["status"] for r in res], np.int32), sweeps=np.array([r["sweeps"] for r in res], np.int32),
                condX=np.array([np.linalg.cond(r["X"]) if r["X"] is not None else np.nan for r in res]))


# ---- generators ----------------------------------------------------------------------------------------------------------
def make_case(n, m, B, seed=None, poles=None, ny=None, i_ym=None):
    """Â random with spectral radius 0.9, Ĉ Gaussian, poles linspace(0.05, 0.85, n) unless given ((n,) or (B,n))."""
    rng = np.random.default_rng([1000 * n + m, B] if seed is None else seed)
    A = rng.standard_normal((B, n, n))
    A *= (0.9 / np.abs(np.linalg.eigvals(A)).max(axis=1))[:, None, None]
    ny = m if ny is None else ny
    C = rng.standard_normal((B, ny, n))
    p = np.linspace(0.05, 0.85, n) if poles is None else np.asarray(poles, float)
    return dict(n=n, m=m, B=B, ny=ny, nu=1, Ahat=A, Chat=C, Bhu=rng.standard_normal((B, n, 1)), i_ym=list(range(m)) if i_ym is None else list(i_ym),
                poles=np.broadcast_to(p, (B, n)).copy())


def default_poles(n):
    return 1e-3 * np.arange(1, n + 1) + 0.5       # the reference's 1e-3*(1:nx̂) .+ 0.5


REPEATED = dict(n=4, m=2, B=4, poles=[0.3, 0.3, 0.6, 0.6])


def all_pole_cases():
    return ([make_case(*c) for c in CASES] + [make_case(n, m, B, poles=default_poles(n)) for n, m, B in DEFAULT_POLE_CASES]
            + [make_case(**REPEATED)])


# ---- handles and the check ---------------------------------------------------------------------------------------------
def set_model(h, case, Ahat=None, Chat=None):
    cm = mpcqp.api.colmajor
    h.set_model(cm(case["Ahat"] if Ahat is None else Ahat), cm(case["Bhu"]), cm(case["Chat"] if Chat is None else Chat))


def make_handle(case, lib=None, place=True, cap=None):
    """A raw C-ABI handle with the case's model and (place=True) the poles placed; cap: placed again with that cap."""
    h = mpcqp.api.Handle(case["B"], case["n"], case["nu"], case["ny"], 0, 2, 1, lib=lib)
    set_model(h, case)
    if place:
        h.kf_set_poles(case["poles"], case["i_ym"])
        if cap is not None:
            h.kf_set_place_cap(cap)
            h.kf_place()
    return h


def closed_loop_matrix(A, Cm, K):
    return A @ (np.eye(A.shape[0]) - K @ Cm)


def pole_ratio(A, Cm, K, p):
    """(lhs, ratio, cond2(V)) of the bar above for one member."""
    w, V = np.linalg.eig(closed_loop_matrix(A, Cm, K))
    V = V / np.linalg.norm(V, axis=0)
    lhs = float(np.abs(np.sort_complex(w) - np.sort(p)).max())
    cV = float(np.linalg.cond(V))
    scale = cV * EPS * (np.linalg.norm(A, 2) + np.linalg.norm(Cm @ A, 2) * np.linalg.norm(K, 2))
    return lhs, lhs / scale, cV


def worst_ratio(case, K):
    Cm = case["Chat"][:, case["i_ym"]]
    rows = [pole_ratio(case["Ahat"][b], Cm[b], K[b], case["poles"][b]) for b in range(case["B"])]
    return max(r[1] for r in rows), max(r[0] for r in rows), [r[2] for r in rows]


def check_placed(case, lib=None):
    """Status 0 for every member and the Bauer-Fike bar with TAU."""
    h = make_handle(case, lib=lib)
    st, K, sw = h.kf_status(), h.kf_gain(), h.kf_place_sweeps()
    assert K.shape == (case["B"], case["n"], case["m"])
    ratio, lhs, conds = worst_ratio(case, K)
    print(f"(n, m, B) = {(case['n'], case['m'], case['B'])}: status {st.tolist()} sweeps {sw.tolist()} max |eig - p| = {lhs:.3e} "
          f"ratio {ratio:.3g} (TAU {TAU}) cond V {min(conds):.3g} .. {max(conds):.3g}")
    assert not st.any(), st
    assert h.kf_lanes_per_estimator() == 64
    assert (sw >= (1 if case["m"] < case["n"] else 0)).all() and (sw <= CAP).all()
    assert ratio <= TAU, (ratio, lhs)
    return h


def check_closed_form(lib=None):
    """n = 1: K̂ = (1 - p / a) / c within 16 eps relative."""
    a = np.array([0.8, -0.7, 0.3, 1.4, -1.2])
    c = np.array([1.0, 2.5, -0.4, 3.0, -0.9])
    p = np.array([0.5, 0.2, -0.6, 0.0, 0.9])
    B = len(a)
    case = dict(n=1, m=1, B=B, ny=1, nu=1, Ahat=a.reshape(B, 1, 1), Chat=c.reshape(B, 1, 1), Bhu=np.ones((B, 1, 1)), i_ym=[0],
                poles=p.reshape(B, 1))
    h = make_handle(case, lib=lib)
    K, want = h.kf_gain().reshape(B), (1.0 - p / a) / c
    err = np.abs(K - want) / np.abs(want)
    print("closed form: relative errors / eps", (err / EPS).tolist())
    assert not h.kf_status().any() and not h.kf_place_sweeps().any()
    assert (err <= 16 * EPS).all(), err


_sweep_refs = {}


def sweep_refs(spec):
    """The case of SWEEP_CASES entry `spec` and the restatement's results at cap 0 and at cap 30 (computed once)."""
    if spec not in _sweep_refs:
        n, m, B, seed = spec
        case = make_case(n, m, B, seed=seed)
        _sweep_refs[spec] = (case, place_ref(case, 0), place_ref(case, CAP))
    case, r0, r30 = _sweep_refs[spec]
    return case, r0["condX"], r30["condX"]


def condV(case, K):
    Cm = case["Chat"][:, case["i_ym"]]
    return np.array([pole_ratio(case["Ahat"][b], Cm[b], K[b], case["poles"][b])[2] for b in range(case["B"])])


def device_condV(case, h):
    return condV(case, h.kf_gain())


def check_sweeps(spec, lib=None):
    """Default cap: cond2(V) below the geometric mean c* of the restatement's two condition numbers, sweeps >= 1; cap 0: above
    it, sweeps 0."""
    case, c0, c30 = sweep_refs(spec)
    cstar = np.sqrt(c0 * c30)
    h = make_handle(case, lib=lib)
    cv, sw = device_condV(case, h), h.kf_place_sweeps()
    print("default cap: cond V", cv.tolist(), "c*", cstar.tolist(), "sweeps", sw.tolist())
    assert not h.kf_status().any() and (sw >= 1).all() and (cv < cstar).all()
    h.kf_set_place_cap(0)
    h.kf_place()
    cv0, sw0 = device_condV(case, h), h.kf_place_sweeps()
    print("cap 0: cond V", cv0.tolist(), "sweeps", sw0.tolist())
    assert not h.kf_status().any() and not sw0.any() and (cv0 > cstar).all()


def refusal_cases():
    """n = 2, m = 1, B = 6: members 1 (the reference's unobservable model), 3 (double pole) and 4 (NaN in Â) broken; and the
    same batch with healthy members in their places."""
    good = make_case(2, 1, 6, poles=[0.3, 0.6])
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
    bad["Ahat"][1], bad["Chat"][1] = np.diag([1.0, 1.5]), np.array([[1.0, 0.0]])
    bad["poles"][3] = [0.5, 0.5]
    bad["Ahat"][4][0, 1] = np.nan
    return good, bad, [1, 3, 4], [0, 2, 5]


def check_refusals(lib=None):
    good, bad, broken, healthy = refusal_cases()
    hg, hb = make_handle(good, lib=lib), make_handle(bad, lib=lib)
    assert not hg.kf_status().any()
    st, Kg, Kb = hb.kf_status(), hg.kf_gain(), hb.kf_gain()
    print("refusals:", st.tolist())
    assert (st[broken] == 2).all() and not st[healthy].any()
    assert not Kb[broken].any()
    assert Kb[healthy].tobytes() == Kg[healthy].tobytes()
    # a model swap that breaks member 1 of the healthy handle: it keeps its old gain, the others are placed on their models
    swapped = good["Ahat"].copy()
    swapped[1] = bad["Ahat"][1]
    set_model(hg, good, Ahat=swapped, Chat=bad["Chat"])
    assert hg.kf_gain().tobytes() == Kg.tobytes()
    hg.kf_place()
    st = hg.kf_status()
    assert st[1] == 2 and not st[[0, 2, 3, 4, 5]].any(), st
    assert hg.kf_gain()[1].tobytes() == Kg[1].tobytes() and hg.kf_gain()[[0, 2, 5]].tobytes() == Kg[[0, 2, 5]].tobytes()


def check_contract(lib=None, torch_stream=False):
    """Return codes, read-backs, _device against the host call, placing again against a fresh handle, leaving the mode."""
    import pytest
    case = make_case(4, 2, 5)
    B, n, m = 5, 4, 2
    err = lambda code: pytest.raises(mpcqp.MpcqpError, match=str(code))
    h = mpcqp.api.Handle(B, n, 1, m, 0, 2, 1, lib=lib)
    with err(-5):                                   # MPCQP_ERR_ORDER: no model yet
        h.kf_set_poles(case["poles"], case["i_ym"])
    set_model(h, case)
    for bad in (1.0, -1.0, 1.5, np.nan, np.inf):    # MPCQP_ERR_ARG
        p = case["poles"].copy(); p[2, 1] = bad
        with err(-3):
            h.kf_set_poles(p, case["i_ym"])
    for iy in ([0, 0], [0, 2], [-1, 0]):
        with err(-3):
            h.kf_set_poles(case["poles"], iy)
    for call in (h.kf_place, h.kf_place_device, h.kf_place_sweeps, lambda: h.kf_set_place_cap(3)):
        with err(-5):                               # not in the mode yet
            call()
    h.kf_set_poles(case["poles"], case["i_ym"])
    for cap in (101, -1):
        with err(-3):
            h.kf_set_place_cap(cap)
    K = h.kf_gain()
    assert not h.kf_status().any() and K.any() and h.kf_lanes_per_estimator() == 64
    with err(-5):
        h.get(mpcqp.api.GET_KF_COV)                 # an observer has no covariance
    for call in (h.kf_solve_steady, h.kf_steady_iters, h.kf_steady_path):
        with err(-5):
            call()
    # the estimator steps are those of a gain from kf_set
    x, h2 = np.zeros((B, n)), mpcqp.api.Handle(B, n, 1, m, 0, 2, 1, lib=lib)
    set_model(h2, case)
    h2.kf_set(mpcqp.api.colmajor(K), case["i_ym"])
    x2 = x.copy()
    h.kf_correct(x, np.ones((B, m))); h2.kf_correct(x2, np.ones((B, m)))
    h.kf_predict(x, np.ones((B, 1))); h2.kf_predict(x2, np.ones((B, 1)))
    assert x.any() and x.tobytes() == x2.tobytes()
    # _device equals the host call
    stream = 0
    if torch_stream:
        import torch
        s = torch.cuda.Stream()
        stream = s.cuda_stream
    h.kf_place_device(stream)
    if torch_stream:
        s.synchronize()
    assert h.kf_gain().tobytes() == K.tobytes()
    # placing again after set_model equals a fresh handle on the new model; until then the old gain stays
    new = dict(case, Ahat=0.9 * case["Ahat"])
    set_model(h, new)
    assert h.kf_gain().tobytes() == K.tobytes()
    h.kf_place()
    fresh = make_handle(new, lib=lib)
    assert h.kf_gain().tobytes() == fresh.kf_gain().tobytes() and h.kf_gain().tobytes() != K.tobytes()
    assert h.kf_place_sweeps().tobytes() == fresh.kf_place_sweeps().tobytes()
    # leaving the mode
    eye = lambda k: np.broadcast_to(np.eye(k), (B, k, k)).copy()
    leavers = [lambda: h.kf_set(mpcqp.api.colmajor(K), case["i_ym"]),
               lambda: h.kf_set_covariances(eye(n), eye(m), eye(n), case["i_ym"])]
    leavers.append(lambda: h.kf_set_steady(eye(n), eye(m), case["i_ym"]))
    for leave in leavers:
        h.kf_set_poles(case["poles"], case["i_ym"])
        leave()
        for call in (h.kf_place, h.kf_place_device, h.kf_place_sweeps, lambda: h.kf_set_place_cap(3)):
            with err(-5):
                call()


def refused_then_kf_set(h, case):
    """MPCQP_ERR_UNSUPPORTED, the handle keeps what it had, and a kf_set gain still works afterwards."""
    import pytest
    B, n, m = case["B"], case["n"], case["m"]
    with pytest.raises(mpcqp.MpcqpError, match="-4"):
        h.kf_set_poles(case["poles"], case["i_ym"])
    assert h.kf_lanes_per_estimator() == 0
    h.kf_set(np.full((B, m, n), 0.1), case["i_ym"])
    x = np.zeros((B, n))
    h.kf_correct(x, np.ones((B, m)))
    assert np.allclose(x, 0.1 * m)
    with pytest.raises(mpcqp.MpcqpError, match="-5"):
        h.kf_place()


# ---- the controller ------------------------------------------------------------------------------------------------------
CFG = synth.C2


def controller_pair(direct, lib=None, B=4, seed=31):
    """Two BatchLinMPCs on a C2 batch: one with luenberger=dict(poles), one given the gain read back from it."""
    from tests.parity_util import make_controller
    bt = synth.make_batch(CFG, B, seed=seed)
    poles = np.linspace(0.2, 0.7, CFG.nxh)
    a, b = make_controller(CFG, bt, lib=lib), make_controller(CFG, bt, lib=lib)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                 # (every member placeable: no warning)
        a.setestimator(luenberger=dict(poles=poles), xhat0=bt["xhat0"], direct=direct)
    K = a.hd.kf_gain()
    assert not a.hd.kf_status().any() and K.any()
    b.setestimator(K, xhat0=bt["xhat0"], direct=direct)
    a.lastu0, b.lastu0 = bt["lastu0"].copy(), bt["lastu0"].copy()
    return a, b, bt, poles


def check_controller(direct, lib=None, nper=5, torch_device=None):
    """u, x̂0 and status bit for bit over five periods: the methods, sim, and hd.loop_device (whose buffers are the device's:
    torch tensors on `torch_device`, NumPy arrays on the emulator)."""
    a, b, bt, _ = controller_pair(direct, lib=lib)
    B = bt["xhat0"].shape[0]
    xp = bt["xhat0"].copy()
    rng = np.random.default_rng(0)
    for k in range(nper):
        y = np.einsum("bij,bj->bi", bt["Chat"], xp) + 0.02 * rng.standard_normal((B, CFG.ny))
        a.preparestate(y); b.preparestate(y)
        ua, ub = a.moveinput(None, bt["ry"]), b.moveinput(None, bt["ry"])
        assert ua.tobytes() == ub.tobytes() and np.array_equal(a.status, b.status) and np.all(a.status != mpcqp.STATUS_ERROR)
        a.updatestate(ua, y); b.updatestate(ub, y)
        assert a.xhat0.tobytes() == b.xhat0.tobytes() and a.xhat0.any()
        xp = np.einsum("bij,bj->bi", bt["Ahat"], xp) + np.einsum("bij,bj->bi", bt["Bhu"], ua)
    info = a.getinfo()
    assert info["K̂"].tobytes() == a.hd.kf_gain().tobytes() and not info["kf_status"].any() and (info["place_sweeps"] >= 1).all()
    with np.testing.assert_raises(ValueError):
        a.setstate(np.zeros(CFG.nxh), np.eye(CFG.nxh))
    # sim
    a, b, bt, _ = controller_pair(direct, lib=lib)
    plant = dict(A=bt["Ahat"], Bu=bt["Bhu"], C=bt["Chat"])
    ra, rb = (c.sim(nper, bt["ry"], plant=plant, y_noise=np.full(CFG.ny, 0.02), seed=3, x_0=bt["xhat0"]) for c in (a, b))
    assert ra.U_data.tobytes() == rb.U_data.tobytes() and ra.Xhat_data.tobytes() == rb.Xhat_data.tobytes()
    assert np.array_equal(ra.status, rb.status) and ra.path == rb.path and ra.U_data.any()
    # hd.loop_device
    a, b, bt, _ = controller_pair(direct, lib=lib)
    if torch_device is None:
        new, ptr, host, sync = (lambda v: np.ascontiguousarray(v).copy()), (lambda v: v.ctypes.data), (lambda v: v), (lambda: None)
    else:
        import torch
        new = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(torch_device)
        ptr, host, sync = (lambda v: v.data_ptr()), (lambda v: v.cpu().numpy()), torch.cuda.synchronize
    outs = []
    for c in (a, b):
        c._sim_prepare()
        hd = c.hd
        x, lu, ry = new(bt["xhat0"]), new(bt["lastu0"]), new(np.tile(bt["ry"] - c.yop, CFG.Hp))     # (R̂y over the horizon: nY values)
        Z, u0 = new(np.zeros((B, hd.nZ))), new(np.zeros((B, CFG.nu)))
        st, it = new(np.zeros(B, np.int32)), new(np.zeros(B, np.int32))
        rg = np.random.default_rng(7)
        rows = []
        for k in range(nper):
            y = new(0.3 * rg.standard_normal((B, CFG.ny)))
            hd.loop_device(ptr(x), ptr(y), ptr(lu), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
            sync()
            rows.append((host(x).copy(), host(u0).copy(), host(st).copy()))
            lu, u0 = u0, lu
        outs.append(rows)
    for ra_, rb_ in zip(*outs):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(ra_, rb_)) and ra_[0].any() and ra_[1].any()


def check_observer_error(lib=None, N=40):
    """Constant input and measurement, x̂ off by e0: after N periods the error is at most cond2(V) rho^N |e0| + 1e-12 (the
    error obeys e <- Â (I - K̂ Ĉm) e = V Λ V⁻¹ e)."""
    a, _, bt, poles = controller_pair(True, lib=lib)
    B, n = bt["xhat0"].shape[0], CFG.nxh
    K, A, C = a.hd.kf_gain(), bt["Ahat"], bt["Chat"]
    # the steady state of every linear model: input, state and measurement at the operating point (the augmented model has
    # integrators, so I - Â cannot be solved for another one)
    u, xs, y = np.zeros((B, CFG.nu)), np.zeros((B, n)), np.zeros((B, CFG.ny))
    e0 = np.random.default_rng(5).standard_normal((B, n))
    a.setstate(xs + e0 + a.xhop)
    for _ in range(N):
        a.preparestate(y + a.yop)
        a.updatestate(u + a.uop, y + a.yop)
    err = np.linalg.norm(a.xhat0 - xs, axis=1)
    cV = np.array([np.linalg.cond(np.linalg.eig(closed_loop_matrix(A[b], C[b], K[b]))[1]) for b in range(B)])
    bound = cV * np.abs(poles).max() ** N * np.linalg.norm(e0, axis=1) + 1e-12
    print("observer error after", N, "periods:", err.tolist(), "bound", bound.tolist())
    assert (err <= bound).all() and (np.linalg.norm(e0, axis=1) > 1e3 * err).all()


def check_setmodel_and_warning(lib=None):
    """setmodel places again (equal to a fresh controller on the new model); one RuntimeWarning with the count."""
    import pytest
    from tests.parity_util import make_controller
    a, _, bt, poles = controller_pair(True, lib=lib)
    K = a.hd.kf_gain()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a.setmodel(0.9 * bt["Ahat"], bt["Bhu"], bt["Chat"])
    c = make_controller(CFG, dict(bt, Ahat=0.9 * bt["Ahat"]), lib=lib)
    c.setestimator(luenberger=dict(poles=poles))
    assert a.hd.kf_gain().tobytes() == c.hd.kf_gain().tobytes() and a.hd.kf_gain().tobytes() != K.tobytes()
    # two members made unobservable: a zero column of Ĉ for a mode of a diagonalised member
    B, n = bt["xhat0"].shape[0], CFG.nxh
    Cb = bt["Chat"].copy()
    Ab = bt["Ahat"].copy()
    for i in (1, 2):
        Ab[i] = np.diag(np.linspace(0.2, 0.9, n))
        Cb[i][:, 0] = 0.0
    d = make_controller(CFG, dict(bt, Ahat=Ab, Chat=Cb), lib=lib)
    with pytest.warns(RuntimeWarning, match=r"Cannot compute the Luenberger gain K̂ with specified poles\. \(2 of 4 estimators\)") as rec:
        d.setestimator(luenberger=dict(poles=poles))
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    st = d.hd.kf_status()
    assert st.tolist() == [0, 2, 2, 0] and not d.hd.kf_gain()[[1, 2]].any()
    # the default poles are the reference's
    e = make_controller(CFG, bt, lib=lib)
    e.setestimator(luenberger=dict())
    f = make_controller(CFG, bt, lib=lib)
    f.setestimator(luenberger=dict(poles=np.broadcast_to(default_poles(n), (B, n))))
    assert e.hd.kf_gain().tobytes() == f.hd.kf_gain().tobytes() and not e.hd.kf_status().any()
