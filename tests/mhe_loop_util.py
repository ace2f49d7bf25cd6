"""Case builders and checks of `LinMPC(MovingHorizonEstimator)` -- `BatchLinMPC.setestimator(mhe=…)`, mpcqp_loop_device and
`sim` with the estimator on the device, `initstate` -- shared by tests/test_mhe_loop.py (CPU emulator, libmpcqp_emu_mheloop.so)
and tests/test_gpu_mhe_loop.py (the HIP library): every check takes the library (`lib=None`: the product library).

Cases are `sim_util.Case` data (plant, draws, steps, noise, Q̂, R̂, P̂_0) with a BatchMHE on the controller's augmented model
behind the controller.  The reference of every comparison with a bar is the same run one period at a time through the public
methods of a twin controller (`sim_util.reference`); bars: `sim_util.BAR` (explicit law, unconstrained estimator),
`sim_util.BAR_QP` (interior-point controller and bounded estimator)."""
import os
import subprocess
import warnings

import numpy as np

import mpcqp
from mpcqp import mhe as pm
from oracle import estim as es
from oracle import mhe as om
from tests import explicit_util as xu
from tests import sim_util as su

EMU = su.EMU
LIBNAME = "libmpcqp_emu_mheloop.so"
SANITIZER_OBJS = su.SANITIZER_OBJS + [os.path.join(EMU, "emu_est_init.o")]
WIDE = dict(nx=13, nu=4, ny=4, Hp=6, Hc=2)          # nx̂ = 17: the wide estimator kernels
ROW16 = dict(nx=12, nu=4, ny=4, Hp=6, Hc=2)         # nx̂ = 16: the last size of the 16-lane family
NY2 = dict(nx=4, nu=2, ny=2, Hp=5, Hc=2)


def build():
    """make tests/emu/libmpcqp_emu_mheloop.so (tests/emu/mheloop.mk); returns its path."""
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "mheloop.mk", LIBNAME])
    return os.path.join(EMU, LIBNAME)


class MheCase:
    """A `sim_util.Case` whose controllers carry a BatchMHE (horizon `He`, measured outputs `i_ym`, the case's Q̂, R̂, P̂_0 and
    form).  `bounds`: keywords of `BatchMHE.setconstraint`, each (n,) or (B,n); `infeasible`: a member that gets
    x̂min > x̂max through the handle (the Python setter refuses such bounds)."""

    def __init__(self, kind, *, He=3, i_ym=None, bounds=None, infeasible=None, **kw):
        self.case = su.Case(kind, fuse=False, **kw)
        c = self.case
        self.kind, self.B, self.N, self.He, self.direct = kind, c.B, c.N, He, c.direct
        self.ny = c.cfg.ny
        self.i_ym = np.arange(self.ny) if i_ym is None else np.asarray(i_ym, int)
        self.bounds, self.infeasible = bounds, infeasible

    def estimator(self, lib=None, members=None, He=None):
        c, bt, o = self.case, self.case.bt, self.case.bt["ops"]
        m = slice(None) if members is None else list(members)
        iy = self.i_ym
        nd = c.nd
        est = pm.BatchMHE(bt["Ahat"][m], bt["Bhu"][m], bt["Chat"][m][:, iy], bt["Bhd"][m] if nd else None,
                          bt["Dhd"][m][:, iy] if nd else None, He=He or self.He, Q̂=c.Qhat[m], R̂=c.Rhat[m][:, iy][:, :, iy], P̂_0=c.P0[m],
                          direct=c.direct, uop=o["uop"], yop_m=o["yop"][iy], dop=o["dop"], x̂op=o["xhop"], f̂op=o["fhop"], lib=lib)
        if self.bounds:
            g = lambda v: (np.asarray(v, float)[m] if np.ndim(v) == 2 else v)
            est.setconstraint(**{k: g(v) for k, v in self.bounds.items()})
        if self.infeasible is not None:
            idx = list(range(self.B)) if members is None else list(members)
            if self.infeasible in idx:
                nB, nx = est.B, est.nx̂
                lo, hi = np.full((nB, nx), -np.inf), np.full((nB, nx), np.inf)
                j = idx.index(self.infeasible)
                lo[j], hi[j] = 1.0, -1.0
                est.handle.set_bounds(xmin=lo, xmax=hi)
        return est

    def controller(self, lib=None, members=None, He=None):
        mpc = self.case.controller(lib, members)          # (with the case's Kalman filter: the attachment replaces it)
        mpc.setestimator(mhe=self.estimator(lib, members, He), i_ym=self.i_ym)
        return mpc

    def args(self, *a, **k):
        return self.case.args(*a, **k)


def run(mpc, **kw):
    return su.run(mpc, **kw)


def reference(twin, **kw):
    """`sim_util.reference` on a twin with a MovingHorizonEstimator behind it, and the estimator's status of every period."""
    est, rec = twin.mhe, []
    orig = twin.updatestate

    def updatestate(*a, **k):
        out = orig(*a, **k)
        rec.append(est.handle.get(pm.GET_STATUS))
        return out
    twin.updatestate = updatestate
    try:
        ref = su.reference(twin, **kw)
    finally:
        del twin.updatestate
    ref["est_status"] = np.stack(rec, axis=-1)
    return ref


# -- 1. attachment and refusals -----------------------------------------------------------------------------------------------
def check_attach_and_refusals(lib=None):
    import pytest
    mc = MheCase("explicit_law")
    c, bt, o = mc.case, mc.case.bt, mc.case.bt["ops"]
    B = c.B
    code = lambda n: pytest.raises(mpcqp.MpcqpError, match=f"error {n}:")
    mpc = mpcqp.BatchExplicitMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], bt["Bhd"], bt["Dhd"], Hp=5, Hc=2, law=True, lib=lib, **o)
    mpc._sim_plant(c.plant)
    nxh, nZ = mpc.nxh, mpc.nZ
    io = dict(ry=np.zeros((B, 1)), d=np.zeros((B, 1)), x0=np.zeros((B, c.nxp)), xhat0=np.zeros((B, nxh)), lastu0=np.zeros((B, 1)),
              Ztilde=np.zeros((B, nZ)))
    dbuf = {k: np.zeros(s) for k, s in (("x", (B, nxh)), ("y", (B, 1)), ("lu", (B, 1)), ("ry", (B, 1)), ("Z", (B, nZ)), ("u", (B, 1)),
                                        ("d", (B, 1)), ("D", (B, 5)))}
    st = np.zeros(B, np.int32)
    ad = lambda a: a.ctypes.data
    loop = lambda hd: hd.loop_device(ad(dbuf["x"]), ad(dbuf["y"]), ad(dbuf["lu"]), ad(dbuf["ry"]), ad(dbuf["Z"]), ad(dbuf["u"]), ad(st),
                                     d0=ad(dbuf["d"]), Dhat0=ad(dbuf["D"]))
    with code(-5):                      # before the attachment: no estimator
        mpc.hd.sim(2, **io)
    if lib is not None:                 # (the emulator's "device" is the host: NumPy buffers serve as device pointers)
        with code(-5):
            loop(mpc.hd)
    with code(-5):
        mpc.hd.est_initstate(np.zeros((B, nxh)), np.zeros((B, 1)), np.zeros((B, 1)), np.zeros((B, 1)))
    est = mc.estimator(lib)
    # every mismatch
    other = lambda **kw: MheCase("explicit_law", **kw).estimator(lib)
    for bad in (other(B=4), other(nd=0), other(dims=dict(su.SMALL, nx=3)), other(dims=dict(su.SMALL, nu=2)), other(dims=NY2)):
        with pytest.raises(ValueError):
            mpc.setestimator(mhe=bad)
    with pytest.raises(ValueError):                         # nym = 1 but two measured rows asked for
        mpc.setestimator(mhe=est, i_ym=[0, 0])
    with pytest.raises(ValueError, match="direct"):
        mpc.setestimator(mhe=est, direct=False)
    if lib is not None:                 # (an estimator of another library: the stock emulator next to this one)
        from tests import emu_util
        stock = mpcqp.api.load_library(emu_util.build())
        with pytest.raises(ValueError, match="libraries"):
            mpc.setestimator(mhe=MheCase("explicit_law").estimator(stock))
    for k, v in (("uop", o["uop"] + 1.0), ("yop_m", o["yop"] + 1.0), ("dop", o["dop"] + 1.0), ("x̂op", o["xhop"] + 1.0)):
        e2 = mc.estimator(lib)
        setattr(e2, k, np.broadcast_to(v, getattr(e2, k).shape).copy())
        with pytest.raises(ValueError, match="must be the controller's"):
            mpc.setestimator(mhe=e2)
    with pytest.raises(ValueError):
        mpc.setestimator(mhe=est, Khat=c.Khat)
    # the C-ABI's own refusals
    h4 = MheCase("explicit_law", B=4).estimator(lib).handle
    with code(-2):
        mpc.hd.mhe_attach(h4, [0])
    with code(-2):
        mpc.hd.mhe_attach(est.handle, [0, 0])               # nym disagrees
    with code(-3):
        mpc.hd.mhe_attach(est.handle, [1])                  # outside 0 .. ny-1
    # attached: the explicit-law handle stays on the per-period path
    mpc.setestimator(c.Khat)
    assert mpc.hd.sim_path() == mpcqp.api.SIM_PATH_FUSED
    mpc.setestimator(mhe=est)
    assert mpc.hd.sim_path() == mpcqp.api.SIM_PATH_PERIOD and mpc.mhe is est and mpc.xhat0 is est.x̂0
    mpc.hd.sim(2, **io)
    assert mpc.hd.sim_est_status(2).shape == (2, B)
    with code(-3):
        mpc.hd.sim_est_status(3)
    with pytest.raises(mpcqp.MpcqpError):                   # a covariance passed to setstate raises, as in the reference
        mpc.setstate(np.zeros(nxh), np.eye(nxh))
    assert "estim" in _moved(mpc, c).getinfo() and "Nk" in mpc.getinfo()["estim"]
    # attach, then kf_set: a Kalman handle again
    with code(-5):
        mpc.hd.kf_correct(np.zeros((B, nxh)), np.zeros((B, 1)), np.zeros((B, 1)))
    mpc.setestimator(c.Khat)
    assert getattr(mpc, "mhe", None) is None and mpc.hd.sim_path() == mpcqp.api.SIM_PATH_FUSED
    mpc.hd.kf_correct(np.zeros((B, nxh)), np.zeros((B, 1)), np.zeros((B, 1)))
    # detach by NULL
    mpc.setestimator(mhe=est)
    mpc.hd.mhe_attach(None)
    with code(-5):
        mpc.hd.sim(2, **io)


def _moved(mpc, c):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mpc.preparestate(c.bt["ops"]["yop"], c.d)
        mpc.moveinput(None, c.ry, c.d)
    return mpc


# -- 2. the public methods --------------------------------------------------------------------------------------------------
def check_public_methods(lib=None, direct=True, periods=5):
    """`mpc.preparestate / moveinput / updatestate` with the estimator attached against the stand-alone `est.preparestate`,
    `mpc.moveinput(est.x̂0, …)`, `est.updatestate` on twins, bit for bit."""
    mc = MheCase("explicit_law", direct=direct)
    c = mc.case
    a, est_b, b = mc.controller(lib), mc.estimator(lib), mc.case.controller(lib)
    rng = np.random.default_rng(3)
    o = c.bt["ops"]
    for k in range(periods):
        ym = o["yop"] + rng.standard_normal((c.B, mc.ny))
        d = o["dop"] + 0.3 * rng.standard_normal((c.B, c.nd))
        xa = a.preparestate(ym, d)
        xb = est_b.preparestate(ym, d)
        ua = a.moveinput(None, c.ry, d)
        ub = b.moveinput(est_b.x̂0, c.ry, d)
        xa2 = a.updatestate(ua, ym, d)
        xb2 = est_b.updatestate(ub, ym, d)
        assert np.array_equal(xa, xb) and np.array_equal(ua, ub) and np.array_equal(xa2, xb2), k
        assert np.array_equal(a.xhat0, est_b.x̂0) and a.xhat0 is a.mhe.x̂0
    assert a.mhe.handle.Nk == mc.He and np.any(ua != o["uop"])
    # setmodel forwards the measured rows of Ĉ and D̂d; setstate sets x̂0 and nothing else
    bt = c.bt
    A2, iy = 0.9 * bt["Ahat"], mc.i_ym
    a.setmodel(A2, bt["Bhu"], bt["Chat"], bt["Bhd"], bt["Dhd"])
    b.setmodel(A2, bt["Bhu"], bt["Chat"], bt["Bhd"], bt["Dhd"])
    est_b.setmodel(A2, bt["Bhu"], bt["Chat"][:, iy], bt["Bhd"], None if bt["Dhd"] is None else bt["Dhd"][:, iy])
    xs = o["xhop"] + rng.standard_normal((c.B, a.nxh))
    a.setstate(xs)
    est_b.setstate(xs)
    assert np.array_equal(a.xhat0, est_b.x̂0) and a.mhe.handle.Nk == mc.He
    xa, xb = a.preparestate(ym, d), est_b.preparestate(ym, d)
    ua, ub = a.moveinput(None, c.ry, d), b.moveinput(est_b.x̂0, c.ry, d)
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub)
    assert np.array_equal(a.updatestate(ua, ym, d), est_b.updatestate(ub, ym, d))


# -- 3. sim against the per-period twin ---------------------------------------------------------------------------------------
# v̂ and x̂ bounds of the bounded case, chosen on the CPU so that oracle.mhe.MHEOracle, replaying the bounded run's records, has
# an active bound in at least two periods of at least two members with every status 0 (periods with an active bound per
# member on the emulator: 1, 3, 5, 0, 6); check_sim_against_twin asserts that condition on every run
BOUNDED = dict(v̂min=np.full(2, -0.12), v̂max=np.full(2, 0.12), x̂min=np.full(6, -2.5), x̂max=np.full(6, 2.5))
TWIN_CASES = {
    "law": ("explicit_law", dict()), "law_predictor": ("explicit_law", dict(direct=False)), "law_nd0": ("explicit_law", dict(nd=0)),
    "law_nd0_predictor": ("explicit_law", dict(nd=0, direct=False)),
    "linmpc_umax_bounded": ("linmpc_umax", dict(bounds=BOUNDED)),
    "ny2_iym1": ("explicit_law", dict(dims=NY2, i_ym=[1])),
    "wide": ("explicit_law", dict(dims=WIDE)),
}


def bound_activity(mc, res):
    """The bounded run's records replayed through MHEOracle, member by member: statuses, and per member the number of periods
    in which a bound of the oracle's solution is active to 1e-6 (as tests/mhe_util.py counts them)."""
    B, N = mc.B, mc.N
    active, statuses = np.zeros(B, int), []
    for b in range(B):
        e = oracle_of(mc, b)
        for k in range(N):
            _oracle_period(e, mc, res, b, k)
            statuses.append(e.status)
            Nk, nx, nym = e.Nk, e.nxh, e.nym
            hit = False
            for val, lo, hi, n in ((e.X0[:Nk * nx], e.con["X0min"], e.con["X0max"], nx), (e.Vhat[:Nk * nym], e.con["Vmin"], e.con["Vmax"], nym)):
                lo, hi = lo[len(lo) - n * Nk:], hi[len(hi) - n * Nk:]
                hit = hit or bool(np.any(np.abs(val - lo) <= 1e-6) or np.any(np.abs(val - hi) <= 1e-6))
            active[b] += hit
    return active, statuses


def check_sim_against_twin(lib=None, name="law"):
    kind, kw = TWIN_CASES[name]
    mc = MheCase(kind, **kw)
    mpc, twin = mc.controller(lib), mc.controller(lib)
    if name == "wide":
        assert mpc.mhe.handle.lanes_per_estimator() == 64
    res = run(mpc, **mc.args())
    ref = reference(twin, **mc.args())
    errs, same = su.compare(res, ref)
    errs["x̂0"], errs["lastu0"] = su.err(mpc.xhat0, twin.xhat0), su.err(mpc.lastu0, twin.lastu0)
    if not kind.startswith("explicit"):
        errs["Z̃"] = su.err(mpc.Z, twin.Z)
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    bar = su.BAR_QP if kind == "linmpc_umax" else su.BAR
    assert res.path == mpcqp.api.SIM_PATH_PERIOD and same, (res.status, ref["status"])
    assert np.array_equal(res.est_status, ref["est_status"]) and res.est_status.shape == (mc.B, mc.N), (res.est_status, ref["est_status"])
    for k, v in errs.items():
        assert v <= bar, (k, v)
    assert np.array_equal(mpc.mhe.x̂0, mpc.xhat0) and mpc.mhe.handle.Nk == twin.mhe.handle.Nk == min(mc.He, mc.N)
    if name == "linmpc_umax_bounded":
        # from the oracle alone: an active estimator bound in at least two periods of at least two members, every status 0
        active, statuses = bound_activity(mc, res)
        print("periods with an active estimator bound per member:", active)
        assert all(s == 0 for s in statuses) and np.all(res.est_status == 0), (statuses, res.est_status)
        assert np.sum(active >= 2) >= 2, active
    return errs


# -- 4. the independent oracle ------------------------------------------------------------------------------------------------
def oracle_of(mc, b):
    """MHEOracle of member b on the case's augmented model, covariances, operating points and bounds."""
    c, bt, o = mc.case, mc.case.bt, mc.case.bt["ops"]
    nx, ny, nd = c.cfg.nx, c.cfg.ny, c.nd
    Ah, Bh, Ch = bt["Ahat"][b], bt["Bhu"][b], bt["Chat"][b]
    model = es.LinModelOracle(Ah[:nx, :nx], Bh[:nx], Ch[:, :nx], bt["Bhd"][b][:nx] if nd else None, bt["Dhd"][b] if nd else None)
    model.setop(uop=o["uop"], yop=o["yop"], dop=o["dop"])
    e = om.MHEOracle(model, He=mc.He, direct=mc.direct, nint_ym=[1] * ny, P_0=c.P0[b])
    assert np.allclose(e.Ah, Ah) and np.allclose(e.Bhu, Bh) and np.allclose(e.Chm, Ch[mc.i_ym]) and (not nd or np.allclose(e.Bhd, bt["Bhd"][b]))
    # the case's covariances (full Q̂) and operating points of the augmented state
    e.Q = e.cov.Q = c.Qhat[b].copy()
    e.R = e.cov.R = c.Rhat[b].copy()
    e.invQ, e.invR = np.linalg.inv(e.Q), np.linalg.inv(e.R)
    e.xhop = e.cov.xhop = np.asarray(o["xhop"], float).copy()
    e.fhop = e.cov.fhop = np.asarray(o["fhop"], float).copy()
    (e.E, e.G, e.J, e.B, e.exbar, e.EX, e.GX, e.JX, e.BX) = om.init_predmat_mhe(e.Ah, e.Bhu, e.Chm, e.Bhd, e.Dhdm, e.xhop, e.fhop, e.He, e.direct)
    e.reset()
    if mc.bounds:
        e.setconstraint(**{k2: mc.bounds[k1] for k1, k2 in (("x̂min", "xhatmin"), ("x̂max", "xhatmax"), ("v̂min", "vhatmin"), ("v̂max", "vhatmax"))
                           if k1 in mc.bounds})
    e.setstate(c.xhat_0[b])         # (`sim` seeds x̂0 alone: the estimator's own lastu0 stays zero, as after its construction)
    return e


def _oracle_period(e, mc, res, b, k):
    """Period k of the recorded run on the oracle; returns x̂ as X̂_data records it (after preparestate!)."""
    d = res.D_data[b, :, k] if mc.case.nd else ()
    ym = res.Y_data[b, mc.i_ym, k]
    x = e.preparestate(ym, d)
    e.updatestate(res.U_data[b, :, k], ym, d)
    return x


def check_oracle_replay(lib=None, bounded=False):
    """The recorded U, Y[i_ym], D of one run replayed through MHEOracle, member by member (B = 3): X̂_data per period at the
    bars of tests/test_mhe.py against the same oracle -- 1e-12 without bounds (test_mhe.py:99, `ex`: |x̂ - x̂_oracle| /
    max(1, max|x̂_oracle|)), 2e-6 with bounds (test_mhe.py:114).  Direct form: X̂_data is the estimate after preparestate!."""
    kind, kw = ("linmpc_umax", dict(bounds=BOUNDED)) if bounded else ("explicit_law", dict())
    mc = MheCase(kind, B=3, **kw)
    res = run(mc.controller(lib), **mc.args())
    assert np.all(res.est_status == 0)
    worst = 0.0
    for b in range(mc.B):
        e = oracle_of(mc, b)
        for k in range(mc.N):
            xo = _oracle_period(e, mc, res, b, k)
            assert e.status == 0
            worst = max(worst, float(np.abs(res.X̂_data[b, :, k] - xo).max() / max(1.0, np.abs(xo).max())))
    print("oracle replay", "bounded" if bounded else "unconstrained", f"{worst:.2e}")
    assert worst <= (2e-6 if bounded else 1e-12), worst
    return worst


# -- 5. continuation, 6. batch independence, 7. a failing member -----------------------------------------------------------------
def check_continuation(lib=None, kind="explicit_law", **kw):
    """Two runs of three periods equal one run of six, bit for bit, He = 2: windows, P̄, Nk and the ring indices go on."""
    mc = MheCase(kind, He=2, **kw)
    one, two = mc.controller(lib), mc.controller(lib)
    whole = run(one, **mc.args())
    h = mc.N // 2
    a = run(two, **mc.args(periods=(0, h)))
    b = run(two, **mc.args(periods=(h, mc.N), first=False))
    for k in su.RECORDS:
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)], axis=2), getattr(whole, k)), k
    assert np.array_equal(np.concatenate([a.status, b.status], axis=1), whole.status)
    assert np.array_equal(np.concatenate([a.est_status, b.est_status], axis=1), whole.est_status)
    for k in ("xhat0", "lastu0", "Z", "sim_x0"):
        assert np.array_equal(getattr(one, k), getattr(two, k), equal_nan=True), k
    i1, i2 = one.mhe.getinfo(), two.mhe.getinfo()
    assert i1["Nk"] == i2["Nk"] == 2 and np.array_equal(i1["P̄"], i2["P̄"]) and np.array_equal(i1["Ŵ"], i2["Ŵ"])


def check_member_alone(lib=None, wide=False, member=3):
    mc = MheCase("explicit_law", dims=WIDE if wide else ROW16)
    mpc = mc.controller(lib)
    assert mpc.mhe.handle.lanes_per_estimator() == (64 if wide else 16)
    whole = run(mpc, **mc.args())
    alone = run(mc.controller(lib, [member]), **mc.args([member]))
    assert su.same_records(whole, alone, [member], [0]) == []
    assert np.array_equal(whole.est_status[member], alone.est_status[0])


def check_failing_member(lib=None, bad=2):
    """Member `bad` with x̂min > x̂max: estimator status 2 in every period (the open-loop estimate is kept), counted in the
    warning; every other member bit-identical to the run in which that member is feasible."""
    import pytest
    mc, ok = MheCase("explicit_law", infeasible=bad), MheCase("explicit_law")
    with pytest.warns(RuntimeWarning, match=r"MHE terminated without solution: estimation in open-loop \(6 of 30 estimator periods\)"):
        res = mc.controller(lib).sim(**mc.args())
    good = run(ok.controller(lib), **ok.args())
    others = [b for b in range(mc.B) if b != bad]
    assert np.all(res.est_status[bad] == 2) and np.all(res.est_status[others] == 0) and np.all(good.est_status == 0)
    assert su.same_records(res, good, others) == []
    assert np.all(np.isfinite(res.X̂_data[bad])) and not np.array_equal(res.X̂_data[bad], good.X̂_data[bad])


# -- 8. mpcqp_loop_device ---------------------------------------------------------------------------------------------------------
class Dev:
    """Device buffers: torch tensors on the GPU, NumPy arrays on the emulator (whose device memory is the host's)."""

    def __init__(self, lib):
        self.gpu = lib is None
        if self.gpu:
            import torch
            self.torch = torch

    def put(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.tensor(a, device="cuda:0") if self.gpu else a.copy()

    def ptr(self, t):
        return t.data_ptr() if self.gpu else t.ctypes.data

    def get(self, t):
        return t.cpu().numpy() if self.gpu else t.copy()

    def sync(self):
        if self.gpu:
            self.torch.cuda.synchronize()


def check_loop_device(lib=None, kind="linmpc_umax", direct=True, periods=5):
    """mpcqp_loop_device on a handle with a MovingHorizonEstimator against prepare + step + update issued separately (the
    estimator's calls on its own stream, the step on the default stream, a synchronisation between them), bit for bit, He = 2."""
    mc = MheCase(kind, He=2, direct=direct)
    c, o = mc.case, mc.case.bt["ops"]
    B, nd = c.B, c.nd
    dv = Dev(lib)
    rng = np.random.default_rng(8)
    out = []
    for fused in (True, False):
        mpc = mc.controller(lib)
        mpc._prepare_kernel()
        hd, eh = mpc.hd, mpc.mhe.handle
        hd.set_flags(hd.flags | mpcqp.api.FLAG_RY_CONSTANT)
        eh.set_state(c.xhat_0 - o["xhop"])
        xe = eh.device_ptr(pm.GET_XHAT0)
        x = dv.put(np.full((B, mpc.nxh), -7.0))
        lu, ry = dv.put(c.lastu - o["uop"]), dv.put(c.ry - o["yop"])
        Z, u0 = dv.put(np.zeros((B, mpc.nZ))), dv.put(np.zeros((B, mpc.nu)))
        st, it = dv.put(np.zeros(B, np.int32)), dv.put(np.zeros(B, np.int32))
        rec = []
        r2 = np.random.default_rng(8)
        for k in range(periods):
            y0m = dv.put(r2.standard_normal((B, mc.ny)))
            d0h = 0.3 * r2.standard_normal((B, nd))
            d0, Dh = dv.put(d0h), dv.put(np.tile(d0h, mpc.Hp))
            if fused:
                hd.loop_device(dv.ptr(x), dv.ptr(y0m), dv.ptr(lu), dv.ptr(ry), dv.ptr(Z), dv.ptr(u0), dv.ptr(st), iters=dv.ptr(it),
                               d0=dv.ptr(d0), Dhat0=dv.ptr(Dh))
                dv.sync()
                xs = dv.get(x)
            else:
                eh.prepare_device(dv.ptr(y0m), dv.ptr(d0))
                eh.sync()
                xs = eh.get(pm.GET_XHAT0)
                hd.step_device(xe, dv.ptr(lu), dv.ptr(ry), dv.ptr(Z), dv.ptr(u0), dv.ptr(st), iters=dv.ptr(it), d0=dv.ptr(d0), Dhat0=dv.ptr(Dh))
                dv.sync()
                eh.update_device(dv.ptr(u0), dv.ptr(y0m), dv.ptr(d0))
                eh.sync()
            lu = dv.put(dv.get(u0))
            rec.append((xs, dv.get(u0), dv.get(Z), dv.get(st), eh.get(pm.GET_XHAT0), eh.get(pm.GET_STATUS), eh.get(pm.GET_PBAR), eh.Nk))
        out.append(rec)
    for k, (a, b) in enumerate(zip(*out)):
        for i, (p, q) in enumerate(zip(a, b)):
            assert np.array_equal(p, q), (k, i)
    assert out[0][-1][-1] == 2 and not np.array_equal(out[0][0][1], out[0][-1][1])
    assert not np.any(out[0][-1][0] == -7.0)


# -- 9. initstate -------------------------------------------------------------------------------------------------------------------
INIT_SHAPES = {"nx3_nym1": dict(nx=2, nu=1, ny=1), "nx16_nym4": dict(nx=12, nu=4, ny=4), "nx17_nym4": dict(nx=13, nu=4, ny=4),
               "nx32_nym16": dict(nx=16, nu=3, ny=16), "nx32_nym32": dict(nx=16, nu=3, ny=16, extra=16)}


def init_controller(lib, name, B=5, nd=1, seed=7, members=None, singular=None, ops=True):
    """A controller on an `explicit_util.random_batch` model with a steady gain of zeros attached (the gain plays no part in
    initstate); `extra` further random output rows (ny + extra measured outputs: nym = 32 on nx̂ = 32, the 64-row case);
    `singular`: a member whose Ĉ loses the column of its first integrator (no full column rank)."""
    sh = dict(INIT_SHAPES[name])
    extra = sh.pop("extra", 0)
    cfg, bt = xu.random_batch(sh["nx"], sh["nu"], sh["ny"], 2, 1, B, nd=nd, seed=seed, ops=ops)
    rng = np.random.default_rng([seed, 5])
    Chat, Dhd = bt["Chat"], bt["Dhd"]
    o = dict(bt["ops"])
    if extra:
        Chat = np.concatenate([Chat, rng.standard_normal((B, extra, bt["nxh"])) / np.sqrt(bt["nxh"])], axis=1)
        Dhd = np.concatenate([Dhd, 0.3 * rng.standard_normal((B, extra, nd))], axis=1)
        o["yop"] = np.concatenate([o["yop"], rng.standard_normal(extra)])
    if singular is not None:
        Chat = Chat.copy()
        Chat[singular, :, sh["nx"]] = 0.0
    m = slice(None) if members is None else list(members)
    mpc = mpcqp.BatchExplicitMPC(bt["Ahat"][m], bt["Bhu"][m], Chat[m], bt["Bhd"][m], Dhd[m], Hp=2, Hc=1, lib=lib, **o)
    nB, ny = mpc.B, mpc.ny
    mpc.setestimator(np.zeros((nB, mpc.nxh, ny)))
    u = o["uop"] + rng.standard_normal((B, sh["nu"]))
    ym = o["yop"] + rng.standard_normal((B, ny))
    d = o["dop"] + rng.standard_normal((B, nd))
    return mpc, u[m], ym[m], d[m]


def init_system(mpc, u, ym, d):
    """M = [I - Â; Ĉm] and the right-hand side of every member (src/estimator/execute.jl:246-259)."""
    iy = mpc.i_ym
    M = np.concatenate([np.eye(mpc.nxh) - mpc._Ahat, mpc._Chat[:, iy]], axis=1)
    top = np.einsum("bij,bj->bi", mpc._Bhu, u - mpc.uop) + np.einsum("bij,bj->bi", mpc._Bhd, d - mpc.dop) + mpc.fhop - mpc.xhop
    bot = ym - mpc.yop[:, iy] - np.einsum("bij,bj->bi", mpc._Dhd[:, iy], d - mpc.dop)
    return M, np.concatenate([top, bot], axis=1)


def check_initstate_lstsq(lib=None, name="nx3_nym1"):
    """Against np.linalg.lstsq per member, bar explicit_util.BAR; the inputs have cond(M) <= 1e3, so cond² eps <= 2.3e-10."""
    mpc, u, ym, d = init_controller(lib, name)
    M, rhs = init_system(mpc, u, ym, d)
    conds = np.array([np.linalg.cond(Mb) for Mb in M])
    assert M.shape[1:] == (mpc.nxh + len(mpc.i_ym), mpc.nxh) and conds.max() <= 1e3, conds
    before = mpc.xhat0.copy()
    x = mpc.initstate(u, ym, d)
    ref = np.array([np.linalg.lstsq(Mb, rb, rcond=None)[0] for Mb, rb in zip(M, rhs)])
    e = xu.err(mpc.xhat0, ref)
    print(name, "cond", f"{conds.max():.1f}", "err", f"{e:.2e}")
    assert np.all(mpc.init_status == 0) and e <= xu.BAR, e
    assert np.array_equal(x, mpc.xhat0 + mpc.xhop) and not np.array_equal(mpc.xhat0, before)
    assert np.all(mpc.Z == 0.0) and np.array_equal(mpc.lastu0, u - mpc.uop)
    return e


def check_initstate_doctest(lib=None, B=2):
    """The doctest of initstate! (src/estimator/execute.jl:193-199): SteadyKalmanFilter(LinModel(tf(3, [10, 1]), 0.5),
    nint_ym=[2]), u = [1], y = [3 - 0.1]: x̂ = [10, 0, -0.1]; against oracle.estim's initstate, and ŷm = ym afterwards."""
    A, Bm, Cm = es.tf1_zoh(3.0, 10.0, 0.5)
    sc = Cm[0, 0] / 0.3            # the realisation of the reference's ss(tf(3, [10, 1])): C = 0.3, so x = 10 at y = 3
    kf = es.SteadyKalmanFilterOracle(es.LinModelOracle(A, Bm * sc, Cm / sc, Ts=0.5), nint_ym=[2])
    xo = kf.initstate([1.0], [2.9])
    rep = lambda a: np.broadcast_to(a, (B,) + a.shape).copy()
    mpc = mpcqp.BatchExplicitMPC(rep(kf.Ah), rep(kf.Bhu), rep(kf.Ch), Hp=3, Hc=1, lib=lib)
    mpc.setestimator(rep(kf.Khat))
    x = mpc.initstate([1.0], [2.9])
    yhat = np.einsum("bij,bj->bi", mpc._Chat, mpc.xhat0)
    print("doctest x̂", x[0], "oracle", xo)
    assert xu.err(x, rep(xo)) <= xu.BAR and np.allclose(yhat, 2.9, rtol=0.0, atol=1e-9)
    assert np.allclose(x, [10.0, 0.0, -0.1], rtol=0.0, atol=1e-9)
    return x


def check_initstate_consistent(lib=None, name="nx16_nym4"):
    """ŷm = ym afterwards when the system is consistent (atol 1e-9): ym is the model's output at a steady state x* of (u, d)
    -- plant states from (I - A) x = Bu u0 + Bd d0, integrator states drawn -- on a model without operating points (f̂op - x̂op
    on an integrator row has no steady state).  Returns max |ŷm - ym| and max |x̂0 - x*|."""
    mpc, u, ym, d = init_controller(lib, name, ops=False)
    M, rhs = init_system(mpc, u, ym, d)
    n, nxp = mpc.nxh, mpc.nxh - mpc.ny
    assert np.all(rhs[:, nxp:n] == 0.0)
    xs = np.random.default_rng(1).standard_normal((mpc.B, n))
    for b in range(mpc.B):
        xs[b, :nxp] = np.linalg.solve(M[b, :nxp, :nxp], rhs[b, :nxp])
    ymc = np.einsum("bij,bj->bi", mpc._Chat, xs) + np.einsum("bij,bj->bi", mpc._Dhd, d)
    mpc.initstate(u, ymc, d)
    yhat = np.einsum("bij,bj->bi", mpc._Chat, mpc.xhat0) + np.einsum("bij,bj->bi", mpc._Dhd, d)
    ey, ex = float(np.abs(yhat - ymc).max()), float(np.abs(mpc.xhat0 - xs).max())
    print(name, "consistent system: |ŷm - ym|", f"{ey:.2e}", "|x̂0 - x*|", f"{ex:.2e}")
    assert np.all(mpc.init_status == 0) and ey <= 1e-9, (ey, ex)
    return ey, ex


def check_initstate_member_alone(lib=None, name="nx17_nym4", member=3):
    whole, u, ym, d = init_controller(lib, name)
    alone, u1, ym1, d1 = init_controller(lib, name, members=[member])
    whole.initstate(u, ym, d)
    alone.initstate(u1, ym1, d1)
    assert np.array_equal(whole.xhat0[member], alone.xhat0[0])


def check_initstate_rank_deficient(lib=None, name="nx16_nym4", bad=1):
    import pytest
    sick, u, ym, d = init_controller(lib, name, singular=bad)
    well, *_ = init_controller(lib, name)
    seed = np.random.default_rng(2).standard_normal((sick.B, sick.nxh))
    sick.xhat0, well.xhat0 = seed.copy(), seed.copy()
    M, _ = init_system(sick, u, ym, d)
    assert np.linalg.matrix_rank(M[bad]) == sick.nxh - 1
    with pytest.warns(RuntimeWarning, match=r"no full column rank.*\(1 of 5 estimators\)") as rec:
        sick.initstate(u, ym, d)
    assert len([w for w in rec if "full column rank" in str(w.message)]) == 1
    well.initstate(u, ym, d)
    others = [b for b in range(sick.B) if b != bad]
    assert sick.init_status[bad] == 1 and np.all(sick.init_status[others] == 0)
    assert np.array_equal(sick.xhat0[bad], seed[bad]) and np.array_equal(sick.xhat0[others], well.xhat0[others])


def check_initstate_covariances(lib=None):
    """init_estimate_cov!: a time-varying filter has P̂ = P̂_0 afterwards, a MovingHorizonEstimator Nk = 0 and P̄ = P̂_0."""
    c = su.Case("explicit_law", estimator="tv")
    mpc = c.controller(lib)
    su.run(mpc, **c.args())
    assert not np.array_equal(mpc.hd.kf_covariance(), c.P0)
    mpc.initstate(c.lastu, c.bt["ops"]["yop"] + 0.5, c.d)
    assert np.array_equal(mpc.hd.kf_covariance(), c.P0)
    mc = MheCase("explicit_law")
    mpc = mc.controller(lib)
    run(mpc, **mc.args())
    assert mpc.mhe.handle.Nk == mc.He and not np.allclose(mpc.mhe.getinfo()["P̄"], mc.case.P0)
    x = mpc.initstate(mc.case.lastu, mc.case.bt["ops"]["yop"] + 0.5, mc.case.d)
    info = mpc.mhe.getinfo()
    assert info["Nk"] == 0 and np.allclose(info["P̄"], mc.case.P0, rtol=0.0, atol=1e-14)
    assert np.array_equal(x, mpc.mhe.x̂0 + mpc.xhop) and np.array_equal(mpc.mhe.handle.get(pm.GET_XHAT0), mpc.mhe.x̂0)
    # the same estimate as behind a Kalman filter on the same model
    kf = mc.case.controller(lib)
    assert np.array_equal(kf.initstate(mc.case.lastu, mc.case.bt["ops"]["yop"] + 0.5, mc.case.d), x)


def check_sim_initstate(lib=None, xhat_given=False):
    """`sim(initstate=True)` equals the three calls made by hand: initstate(lastu, lasty[i_ym], lastd), setstate, sim."""
    mc = MheCase("explicit_law")
    c, o = mc.case, mc.case.bt["ops"]
    a, b = mc.controller(lib), mc.controller(lib)
    kw = mc.args()
    if not xhat_given:
        kw.pop("xhat_0")
    ra = run(a, initstate=True, **kw)
    p = c.plant
    lasty = np.einsum("bij,bj->bi", p["C"], c.x_0 - p["xop"]) + np.einsum("bij,bj->bi", p["Dd"], c.d - o["dop"]) + o["yop"]
    b.initstate(c.lastu, lasty[:, mc.i_ym], c.d)
    if xhat_given:
        b.setstate(c.xhat_0)
    kw2 = mc.args()
    kw2.pop("xhat_0")
    rb = run(b, **kw2)
    assert su.same_records(ra, rb) == [] and np.array_equal(ra.est_status, rb.est_status)
    plain = run(mc.controller(lib), **kw)
    assert xhat_given or su.same_records(ra, plain) != []
