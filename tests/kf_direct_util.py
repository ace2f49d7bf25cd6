"""Helpers of the tests of the predictor form (direct=False) and of missing measurements in the Kalman filters of the LinMPC
loop (include/mpcqp.h: mpcqp_kf_set_direct, mpcqp_kf_update, the NaN rule; csrc/kf_cov_bodies.h, kf_correct_lds of
csrc/mpcqp_bodies.h).  The NumPy reference is tests/kf_util.NumpyKalmanCov with a per-estimator miss mask, written from the
reference (src/estimator/kalman.jl:245-251 / 478-484: any(isnan, y0m) skips the correction step; execute.jl:335: `nothing`
is a row of NaN).  Every runner takes `lib`: None for the HIP library, the CPU emulator library otherwise."""
import warnings

import numpy as np

import mpcqp
from mpcqp import synth
from tests import kf_util as ku

WARNING = "NaN values in the Kalman filter measurements ym: skipping correction step"
XBAR = 1e-10        # x̂ against NumPy, as in tests/test_gpu_kf_cov.py


class MissKalmanCov(ku.NumpyKalmanCov):
    """NumpyKalmanCov whose correction skips the estimators of `miss` (bool (B,)): P̂ and K̂ stay, status 1; unlike a dropped
    update (status 2) the prediction of that period runs."""

    def correct(self, Chat, miss=None):
        P, K = self.P.copy(), self.K.copy()
        super().correct(Chat)
        if miss is not None:
            m = np.asarray(miss, bool)
            self.P[m], self.K[m], self.status[m] = P[m], K[m], 1


class NumpyFilter:
    """B Kalman filters in NumPy on a shape of tests/kf_util.py: the covariance part is MissKalmanCov (or a fixed gain), the
    state part the reference's correct_estimate_obsv! / predict_estimate_obsv!."""

    def __init__(self, sh, x0, Khat=None):
        self.sh, self.x = sh, np.array(x0, float)
        self.cov = MissKalmanCov(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"]) if Khat is None else None
        self.Khat = Khat

    @property
    def K(self):
        return self.cov.K if self.cov is not None else self.Khat

    def correct(self, y, d=None):
        """y (B,nym) with NaN where missing, or None (everybody misses)."""
        sh, B = self.sh, len(self.x)
        miss = np.ones(B, bool) if y is None else np.isnan(y).any(axis=1)
        if self.cov is not None:
            self.cov.correct(sh["Chat"], miss)
        for b in np.flatnonzero(~miss):
            iy = sh["i_ym"]
            v = y[b] - sh["Chat"][b][iy] @ self.x[b] - (sh["Dhd"][b][iy] @ d[b] if sh["nd"] else 0.0)
            self.x[b] = self.x[b] + self.K[b] @ v
        return miss

    def predict(self, u, d=None):
        sh = self.sh
        if self.cov is not None:
            self.cov.predict(sh["Ahat"])
        for b in range(len(self.x)):
            self.x[b] = sh["Ahat"][b] @ self.x[b] + sh["Bhu"][b] @ u[b] + (sh["Bhd"][b] @ d[b] if sh["nd"] else 0.0)


def make_mirror(sh, lib=None, direct=True, Rhat=None, steady=False, x0=None):
    """A BatchLinMPC on the shape's model (Hp = 2, Hc = 1, no constraints: estimator calls only) with the time-varying filter,
    or the steady gain of the shape's covariances."""
    mpc = mpcqp.BatchLinMPC(sh["Ahat"], sh["Bhu"], sh["Chat"], sh["Bhd"], sh["Dhd"], Hp=2, Hc=1, lib=lib)
    R = sh["Rhat"] if Rhat is None else Rhat
    if steady:
        K = mpcqp.steady_kalman_gain(sh["Ahat"], sh["Chat"], sh["Qhat"], R, sh["i_ym"])
        mpc.setestimator(K, sh["i_ym"], xhat0=x0, direct=direct)
        return mpc, K
    mpc.setestimator(covariances=dict(Qhat=sh["Qhat"], Rhat=R, P0=sh["P0"]), i_ym=sh["i_ym"], xhat0=x0, direct=direct)
    return mpc, None


def miss_plan(B, nym, nper, seed, none_at):
    """Per period the (B,nym) bool mask of the NaN entries, or None at period `none_at` (ym = nothing): each estimator misses
    about one period in four, half of the misses with one NaN channel and half with all channels NaN."""
    rng = np.random.default_rng([seed, 31])
    plan = []
    for k in range(nper):
        if k == none_at:
            plan.append(None)
            continue
        mask = np.zeros((B, nym), bool)
        for b in np.flatnonzero(rng.random(B) < 0.25):
            if rng.random() < 0.5:
                mask[b, rng.integers(nym)] = True
            else:
                mask[b] = True
        plan.append(mask)
    return plan


def _call(fn, *a, **kw):
    """fn(*a) with its warnings recorded: (result, counts n of the '(n of B estimators)' warnings)."""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*a, **kw)
    ns = [int(str(w.message).split("(")[1].split(" of ")[0]) for w in rec
          if issubclass(w.category, RuntimeWarning) and str(w.message).startswith(WARNING)]
    return out, ns


def run_misses(sh, nper=12, lib=None, direct=True, seed=3, none_at=5):
    """nper periods of preparestate / updatestate on the mirror with the misses of miss_plan, against NumpyFilter.  Asserts
    what a missed correction must keep bit for bit; returns the worst errors of K̂, P̂, x̂ against NumPy, the lanes per
    estimator and the number of missed corrections."""
    B, nxh, nd, nym = sh["Ahat"].shape[0], sh["nxh"], sh["nd"], len(sh["i_ym"])
    rng = np.random.default_rng([seed, 9])
    x0 = rng.standard_normal((B, nxh))
    mpc, _ = make_mirror(sh, lib=lib, direct=direct, x0=x0)
    ref = NumpyFilter(sh, x0)
    plan = miss_plan(B, nym, nper, seed, none_at)
    eK = eP = ex = 0.0
    nmiss = 0
    hd = mpc.hd
    for k in range(nper):
        y, u = rng.standard_normal((B, nym)), rng.standard_normal((B, sh["nu"]))
        d = rng.standard_normal((B, nd)) if nd else None
        ym = None if plan[k] is None else np.where(plan[k], np.nan, y)
        miss = np.ones(B, bool) if ym is None else plan[k].any(axis=1)
        nmiss += int(miss.sum())
        x_in, P_in, K_in = mpc.xhat0.copy(), hd.kf_covariance(), hd.kf_gain()
        if direct:
            _, ns = _call(mpc.preparestate, ym, d)
            assert ns == ([int(miss.sum())] if miss.any() else []), (k, ns, miss)
            ref.correct(ym, d)
            P, K, st = hd.kf_covariance(), hd.kf_gain(), hd.kf_status()
            # a missed correction keeps x̂0, P̂ and K̂ bit for bit and says so; the others moved
            assert np.array_equal(mpc.xhat0[miss], x_in[miss]) and np.array_equal(P[miss], P_in[miss]) and np.array_equal(K[miss], K_in[miss])
            assert np.array_equal(st, np.where(miss, 1, 0)) and np.array_equal(st, ref.cov.status), (k, st, ref.cov.status)
            assert all(not np.array_equal(mpc.xhat0[b], x_in[b]) for b in np.flatnonzero(~miss))
            eK, eP, ex = max(eK, ku.rel(K, ref.K)), max(eP, ku.rel(P, ref.cov.P)), max(ex, ku.rel(mpc.xhat0, ref.x))
            _, ns = _call(mpc.updatestate, u, None, d)
            assert ns == []
        else:
            xp, ns = _call(mpc.preparestate, ym, d)
            assert ns == [] and np.array_equal(xp, x_in) and np.array_equal(mpc.xhat0, x_in)     # (x̂op = 0)
            _, ns = _call(mpc.updatestate, u, ym, d)
            assert ns == ([int(miss.sum())] if miss.any() else []), (k, ns, miss)
            ref.correct(ym, d)
            K, st = hd.kf_gain(), hd.kf_status()
            assert np.array_equal(K[miss], K_in[miss]) and np.array_equal(st, np.where(miss, 1, 0)), (k, st)
            eK = max(eK, ku.rel(K, ref.K))
        ref.predict(u, d)
        assert not (ref.cov.status == 2).any()          # (the seeds were checked: NumPy's Cholesky succeeds throughout)
        eP, ex = max(eP, ku.rel(hd.kf_covariance(), ref.cov.P)), max(ex, ku.rel(mpc.xhat0, ref.x))
    st = hd.kf_status()
    assert np.isfinite(mpc.xhat0).all() and np.isfinite(hd.kf_covariance()).all() and np.isfinite(hd.kf_gain()).all()
    assert np.isin(st, (0, 1)).all()
    return dict(eK=eK, eP=eP, ex=ex, lanes=hd.kf_lanes_per_estimator(), nmiss=nmiss)


def reference_alone(sh, nper=12, seed=3, none_at=5):
    """The NumPy reference alone on the data of run_misses: True when it stays finite and no correction is dropped."""
    B, nxh, nd, nym = sh["Ahat"].shape[0], sh["nxh"], sh["nd"], len(sh["i_ym"])
    rng = np.random.default_rng([seed, 9])
    ref = NumpyFilter(sh, rng.standard_normal((B, nxh)))
    plan = miss_plan(B, nym, nper, seed, none_at)
    ok, nmiss = True, 0
    for k in range(nper):
        y, u = rng.standard_normal((B, nym)), rng.standard_normal((B, sh["nu"]))
        d = rng.standard_normal((B, nd)) if nd else None
        ym = None if plan[k] is None else np.where(plan[k], np.nan, y)
        nmiss += int(ref.correct(ym, d).sum())
        ok = ok and not (ref.cov.status == 2).any()
        ref.predict(u, d)
        ok = ok and not (ref.cov.status == 2).any() and bool(np.isfinite(ref.x).all() and np.isfinite(ref.cov.P).all())
    return ok, nmiss


def run_forms(steady, lib=None, B=6, nper=8, seed=21):
    """Test 2: the same ym, u sequence through a direct=True controller (preparestate; updatestate) and a direct=False one
    (updatestate(u, ym)) on the C2 shape.  Asserts bit-equality of x̂0, P̂, K̂ after every period, that preparestate of the
    predictor form does nothing, and that its moveinput is that of a plain controller given x̂ₖ₋₁(k).  Returns max |K̂|."""
    from tests.parity_util import make_controller
    cfg = synth.C2
    sh = ku.shape_linmpc(cfg, B, seed)
    bt = sh["bt"]
    ctrl = []
    for direct in (True, False):
        c = make_controller(cfg, bt, lib=lib)
        if steady:
            c.setestimator(mpcqp.steady_kalman_gain(bt["Ahat"], bt["Chat"], sh["Qhat"], sh["Rhat"]), xhat0=bt["xhat0"], direct=direct)
        else:
            c.setestimator(covariances=dict(Qhat=sh["Qhat"], Rhat=sh["Rhat"], P0=sh["P0"]), xhat0=bt["xhat0"], direct=direct)
        c.lastu0 = bt["lastu0"].copy()
        ctrl.append(c)
    filt, pred = ctrl
    plain = make_controller(cfg, bt, lib=lib)
    plain.lastu0 = bt["lastu0"].copy()
    rng = np.random.default_rng(11)
    kmax = 0.0
    for k in range(nper):
        y, u = 0.3 * rng.standard_normal((B, cfg.ny)), 0.2 * rng.standard_normal((B, cfg.nu))
        x_in = pred.xhat0.copy()
        xp = pred.preparestate(y)
        assert np.array_equal(pred.xhat0, x_in) and np.array_equal(xp, x_in + pred.xhop)
        up, uq = pred.moveinput(None, bt["ry"]), plain.moveinput(x_in, bt["ry"])
        assert np.array_equal(up, uq) and np.array_equal(pred.Z, plain.Z) and np.all(pred.status == 0), k
        filt.preparestate(y)
        filt.updatestate(u)
        pred.updatestate(u, y)
        assert np.array_equal(filt.xhat0, pred.xhat0), k
        assert np.array_equal(filt.hd.kf_gain(), pred.hd.kf_gain()), k
        if not steady:
            assert np.array_equal(filt.hd.kf_covariance(), pred.hd.kf_covariance()), k
            assert not filt.hd.kf_status().any() and not pred.hd.kf_status().any()
        kmax = max(kmax, float(np.abs(pred.hd.kf_gain()).max()))
    assert np.isfinite(pred.xhat0).all() and np.abs(pred.xhat0 - bt["xhat0"]).max() > 1e-3
    return kmax


def run_miss_and_drop(lib=None):
    """Test 4: B = 5, estimator 3 with R̂ = -10 I (every correction dropped), NaN for estimator 1 in period 1 and for estimator
    3 in period 2.  Returns the statuses after each of the three periods, P̂, K̂, the NumPy reference and the shape."""
    sh = ku.shape_c2(B=5)
    R = sh["Rhat"].copy()
    R[3] = -10.0 * np.eye(2)
    sh = dict(sh, Rhat=R)
    mpc, _ = make_mirror(sh, lib=lib)
    ref = NumpyFilter(sh, np.zeros((5, sh["nxh"])))
    rng = np.random.default_rng(2)
    sts = []
    for k in range(3):
        y, u = 0.3 * rng.standard_normal((5, 2)), 0.2 * rng.standard_normal((5, sh["nu"]))
        if k == 1:
            y[1, 0] = np.nan
        if k == 2:
            y[3] = np.nan
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            mpc.preparestate(y)
        ref.correct(y)
        mpc.updatestate(u)
        ref.predict(u)
        sts.append((mpc.hd.kf_status().tolist(), ref.cov.status.tolist()))
    return sts, mpc.hd.kf_covariance(), mpc.hd.kf_gain(), ref, sh, mpc


def fused_variants(direct, timevarying, multiple_shooting, B=64, periods=5, torch_device=None, lib=None, seed=7, churn=False):
    """Test 5, after tests/kf_util.fused_vs_separate: mpcqp_loop_device against the separate entry points on the same resident
    data, with NaN in a seeded tenth of the (estimator, period) pairs.  direct=1: against kf_correct_device + step_device +
    kf_predict_device; direct=0: against step_device + kf_update_device and against step_device + kf_correct_device +
    kf_predict_device.  Returns the largest |difference| of x̂0, u0, Z̃, K̂ (and P̂) between the fused run and every other,
    the largest |K̂| and the number of missed corrections; asserts step statuses 0 and (time-varying) filter statuses 1 on
    exactly the missed estimators.  The form is set BEFORE the estimator is attached (the flag survives the setters); with
    `churn` the handle first gets the other kind of estimator, then the one asked for."""
    cfg = synth.Config("loop", nx=3, nu=2, ny=2, Hp=8, Hc=3, umin=-0.6, umax=0.7, ymax=0.9)
    sh = ku.shape_linmpc(cfg, B, 12)
    bt = sh["bt"]
    Ksteady = None if timevarying and not churn else mpcqp.steady_kalman_gain(bt["Ahat"], bt["Chat"], sh["Qhat"], sh["Rhat"])

    def make():
        hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, cfg.Hc, neps=1,
                          flags=mpcqp.FLAG_RY_CONSTANT | (0 if multiple_shooting else mpcqp.FLAG_KEEP_QP), lib=lib)
        if multiple_shooting:
            hd.set_transcription(mpcqp.api.MULTIPLE_SHOOTING)
        hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
        hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt), np.full(B, cfg.Cwt))
        hd.set_bounds(U0min=np.full((B, hd.nU), cfg.umin), U0max=np.full((B, hd.nU), cfg.umax), Y0max=np.full((B, hd.nY), cfg.ymax))
        hd.kf_set_direct(direct)
        if churn and timevarying:
            hd.kf_set(mpcqp.colmajor(Ksteady), np.arange(cfg.ny))
        elif churn:
            hd.kf_set_covariances(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
        if timevarying:
            hd.kf_set_covariances(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
        else:
            hd.kf_set(mpcqp.colmajor(Ksteady), np.arange(cfg.ny))
        hd.prepare()
        return hd

    if torch_device is None:
        new, ptr, host, sync = (lambda a: np.ascontiguousarray(a).copy()), (lambda a: a.ctypes.data), (lambda a: a), (lambda: None)
    else:
        import torch
        new = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch_device)
        ptr, host, sync = (lambda a: a.data_ptr()), (lambda a: a.cpu().numpy()), torch.cuda.synchronize
    variants = ["loop", "correct+step+predict"] if direct else ["loop", "step+update", "step+correct+predict"]
    runs, kmax, nmiss = [], 0.0, 0
    for var in variants:
        hd = make()
        x = new(bt["xhat0"]); lu = new(bt["lastu0"]); ry = new(bt["ry"])
        Z = new(np.zeros((B, hd.nZ))); u0 = new(np.zeros((B, cfg.nu)))
        st = new(np.zeros(B, np.int32)); it = new(np.zeros(B, np.int32))
        rg = np.random.default_rng(seed)
        out = []
        nmiss = 0
        for k in range(periods):
            yh = 0.3 * rg.standard_normal((B, cfg.ny))
            for b in np.flatnonzero(rg.random(B) < 0.1):
                if rg.random() < 0.5:
                    yh[b, rg.integers(cfg.ny)] = np.nan
                else:
                    yh[b] = np.nan
            miss = np.isnan(yh).any(axis=1)
            nmiss += int(miss.sum())
            y = new(yh)
            step = lambda: hd.step_device(ptr(x), ptr(lu), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
            if var == "loop":
                hd.loop_device(ptr(x), ptr(y), ptr(lu), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
            elif var == "correct+step+predict":
                hd.kf_correct_device(ptr(x), ptr(y)); step(); hd.kf_predict_device(ptr(x), ptr(u0))
            elif var == "step+update":
                step(); hd.kf_update_device(ptr(x), ptr(u0), ptr(y))
            else:
                step(); hd.kf_correct_device(ptr(x), ptr(y)); hd.kf_predict_device(ptr(x), ptr(u0))
            sync()
            assert np.all(host(st) == 0), (var, k, host(st))                  # (the missed estimators' steps included)
            if timevarying:
                assert np.array_equal(hd.kf_status(), np.where(miss, 1, 0)), (var, k)
            out.append((host(x).copy(), host(u0).copy(), host(Z).copy(), hd.kf_gain()) + ((hd.kf_covariance(),) if timevarying else ()))
            assert all(np.isfinite(a).all() for a in out[-1]), (var, k)
            kmax = max(kmax, float(np.abs(out[-1][3]).max()))
            lu, u0 = u0, lu                      # u0 of this period is lastu0 of the next
        runs.append(out)
    diff = max(float(np.abs(a - b).max()) for other in runs[1:] for pa, pb in zip(runs[0], other) for a, b in zip(pa, pb))
    return diff, kmax, nmiss
