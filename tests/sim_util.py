"""Case builders and runners of `BatchLinMPC.sim` / mpcqp_sim shared by tests/test_sim.py (CPU emulator) and
tests/test_gpu_sim.py (the HIP library): every runner takes the library (`lib=None`: the product library).

The reference of every comparison with a bar is the same run driven one period at a time through the public methods
`preparestate`, `moveinput` and `updatestate` of a twin controller, around `oracle.estim.LinModelOracle` plants in NumPy, with
the same draws (`reference`).  BAR = 1e-9 * max(1, max|reference|) is `explicit_util.BAR`, the bar of the closed form; BAR_QP =
1e-5 is the project's bar against the certified optimum, for the LinMPC whose inputs saturate (an interior-point solve may
amplify a last-bit difference in ym)."""
import os
import subprocess
import warnings

import numpy as np

import mpcqp
from mpcqp import synth
from oracle import estim as es
from tests import explicit_util as xu

ROOT, EMU, CSRC = xu.ROOT, xu.EMU, xu.CSRC
SIM = "libmpcqp_emu_sim.so"
BAR, BAR_QP = xu.BAR, 1e-5
SANITIZER_OBJS = xu.SANITIZER_OBJS + [os.path.join(EMU, "emu_sim.o")]
SANITIZER_CXX = xu.SANITIZER_CXX
RECORDS = ("Y_data", "Ry_data", "Ŷ_data", "U_data", "Ud_data", "Ru_data", "D_data", "X_data", "X̂_data")
SMALL = dict(nx=2, nu=1, ny=1, Hp=5, Hc=2)
C2 = dict(nx=4, nu=2, ny=2, Hp=20, Hc=5)
KINDS = ("linmpc", "linmpc_umax", "explicit_step", "explicit_law")


def build():
    """make tests/emu/libmpcqp_emu_sim.so (tests/emu/sim.mk); returns its path."""
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "sim.mk", SIM])
    return os.path.join(EMU, SIM)


def err(got, ref):
    return xu.err(got, ref)


class Case:
    """A seeded closed loop: the controllers' augmented models with operating points on every signal (explicit_util.random_batch),
    a plant of its own order -- the controller's plant with every input gain times 1.2 and `nxp - nx` further states --, the
    estimator's covariances and the arguments of a run with steps and noise on all four channels.  `members` selects a
    sub-batch: the same members, whatever the batch they sit in."""

    def __init__(self, kind, *, dims=None, B=5, N=6, nd=1, nxp=None, seed=0, estimator="steady", direct=True, ry_per_period=False,
                 noise=True, ru=False, warm_dual=False, bad=None, policy_weights=False, umax=0.25, fuse=True):
        assert kind in KINDS
        self.kind, self.B, self.N, self.nd, self.seed = kind, B, N, nd, seed
        self.estimator, self.direct, self.warm_dual, self.bad, self.umax = estimator, direct, warm_dual, bad, umax
        self.policy_weights = policy_weights or bad is not None
        self.fuse = fuse
        dims = dict(dims or (C2 if kind == "linmpc_umax" else SMALL))
        nx, nu, ny = dims["nx"], dims["nu"], dims["ny"]
        self.cfg, self.bt = xu.random_batch(nx, nu, ny, dims["Hp"], dims["Hc"], B, nd=nd, seed=seed, ops=True)
        bt, nxh = self.bt, self.bt["nxh"]
        nxp = nx + 1 if nxp is None else nxp
        self.nxp = nxp
        rng = np.random.default_rng([seed, 41])
        n0 = min(nx, nxp)
        A = 0.5 * synth._stable_A(rng, nxp, B)
        A[:, :n0, :n0], A[:, :n0, n0:], A[:, n0:, :n0] = bt["Ahat"][:, :n0, :n0], 0.0, 0.1 * rng.standard_normal((B, nxp - n0, n0))
        Bu = 0.3 * rng.standard_normal((B, nxp, nu))
        Bu[:, :n0] = 1.2 * bt["Bhu"][:, :n0]
        Cm = 0.1 * rng.standard_normal((B, ny, nxp))
        Cm[:, :, :n0] = bt["Chat"][:, :, :n0]
        self.plant = dict(A=A, Bu=Bu, C=Cm, xop=0.1 * rng.standard_normal((B, nxp)), fop=0.1 * rng.standard_normal((B, nxp)))
        if nd:
            self.plant.update(Bd=0.5 * rng.standard_normal((B, nxp, nd)), Dd=0.3 * rng.standard_normal((B, ny, nd)))
        G = rng.standard_normal((B, nxh, nxh)) / np.sqrt(nxh)
        self.Qhat = 0.05 * np.eye(nxh) + 0.05 * G @ G.transpose(0, 2, 1)
        self.Rhat = np.broadcast_to(0.2 * np.eye(ny), (B, ny, ny)).copy()
        self.P0 = np.broadcast_to(0.5 * np.eye(nxh), (B, nxh, nxh)).copy()
        self.Khat = mpcqp.steady_kalman_gain(bt["Ahat"], bt["Chat"], self.Qhat, self.Rhat)
        o = bt["ops"]
        self.xhat_0 = 0.3 * rng.standard_normal((B, nxh)) + o["xhop"]
        self.x_0 = 0.3 * rng.standard_normal((B, nxp)) + self.plant["xop"]
        self.lastu = 0.1 * rng.standard_normal((B, nu)) + o["uop"]
        ry = o["yop"] + 0.5 + 0.3 * rng.standard_normal((B, ny))
        self.ry = ry[:, :, None] + 0.2 * rng.standard_normal((B, ny, N)) if ry_per_period else ry
        self.d = (o["dop"] + 0.3 * rng.standard_normal((B, nd))) if nd else None
        self.ru = (o["uop"] + 0.1 * rng.standard_normal((B, nu))) if ru else None
        z = lambda *s: rng.standard_normal(s)
        self.kw = {}
        if noise:
            self.kw = dict(u_step=0.1 * z(B, nu), y_step=0.2 * z(B, ny), u_noise=0.05 * np.abs(z(B, nu)) + 0.01,
                           y_noise=0.05 * np.abs(z(B, ny)) + 0.01, x_noise=0.02 * np.abs(z(B, nxp)) + 0.01)
            if nd:
                self.kw.update(d_step=0.1 * z(B, nd), d_noise=0.05 * np.abs(z(B, nd)) + 0.01)
        self.draws = dict(w_d=z(B, nd, N), w_y=z(B, ny, N), w_u=z(B, nu, N), w_x=z(B, nxp, N))

    # -- the controller -------------------------------------------------------------------------------------------------
    def controller(self, lib=None, members=None):
        """A fresh controller with its estimator attached, on the members `members` (default: all)."""
        m = slice(None) if members is None else list(members)
        bt, o = self.bt, self.bt["ops"]
        g = lambda a: None if a is None else a[m]
        args = (g(bt["Ahat"]), g(bt["Bhu"]), g(bt["Chat"]), g(bt["Bhd"]), g(bt["Dhd"]))
        kw = dict(Hp=self.cfg.Hp, Hc=self.cfg.Hc, lib=lib, **o)
        nB = args[0].shape[0]
        if self.policy_weights:         # explicit_util.run_status_policy: per-member weights, H̃ = 0 for the member `bad`
            M, Nw, L = np.ones((self.B, self.cfg.ny)), np.full((self.B, self.cfg.nu), 0.1), np.full((self.B, self.cfg.nu), 0.05)
            if self.bad is not None:
                M[self.bad] = Nw[self.bad] = L[self.bad] = 0.0
            kw.update(Mwt=M[m], Nwt=Nw[m], Lwt=L[m])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)         # (the factor warning of a member with H̃ = 0)
            if self.kind.startswith("explicit"):
                mpc = mpcqp.BatchExplicitMPC(*args, law=self.kind == "explicit_law", **kw)
            elif self.kind == "linmpc":
                mpc = mpcqp.BatchLinMPC(*args, Cwt=np.inf, warm_dual=self.warm_dual, **kw)
            else:       # C2's pattern of row groups (its specialisation is in the library); only umax is ever active
                mpc = mpcqp.BatchLinMPC(*args, warm_dual=self.warm_dual, **kw)
                mpc.setconstraint(umin=o["uop"] - 50.0, umax=o["uop"] + self.umax, Δumin=np.full(self.cfg.nu, -50.0),
                                  Δumax=np.full(self.cfg.nu, 50.0))
        if self.estimator == "steady":
            mpc.setestimator(self.Khat[m], direct=self.direct)
        elif self.estimator == "steady_qr":     # the gain solved for on the device
            mpc.setestimator(steady=dict(Qhat=self.Qhat[m], Rhat=self.Rhat[m]), direct=self.direct)
        else:
            mpc.setestimator(covariances=dict(Qhat=self.Qhat[m], Rhat=self.Rhat[m], P0=self.P0[m]), direct=self.direct)
        assert mpc.B == nB
        return mpc

    def args(self, members=None, periods=None, first=True, draws=None):
        """Keyword arguments of `sim` for the members and the periods [lo, hi) asked for; `first=False`: a continuation (no
        x_0, x̂_0, lastu)."""
        m = slice(None) if members is None else list(members)
        lo, hi = periods or (0, self.N)
        g = lambda a: None if a is None else a[m]
        ry = self.ry[m][:, :, lo:hi] if self.ry.ndim == 3 else self.ry[m]
        dr = {k: v[m][:, :, lo:hi] for k, v in (draws or self.draws).items()}
        kw = dict(N=hi - lo, ry=ry, d=g(self.d), ru=g(self.ru), plant={k: v[m] for k, v in self.plant.items()}, draws=dr, fuse=self.fuse,
                  **{k: v[m] for k, v in self.kw.items()})
        if first:
            kw.update(x_0=self.x_0[m], xhat_0=self.xhat_0[m], lastu=self.lastu[m])
        return kw


def run(mpc, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)             # (status and NaN warnings are the business of their own tests)
        return mpc.sim(kw.pop("N"), kw.pop("ry"), kw.pop("d"), kw.pop("ru"), **kw)


def reference(mpc, *, N, ry, d, ru, plant, draws, x_0, xhat_0, lastu, fuse=True, u_step=0.0, y_step=0.0, d_step=0.0, u_noise=0.0,
              y_noise=0.0, d_noise=0.0, x_noise=0.0):
    """The periods of sim_closedloop! (src/plot_sim.jl:291-311) one by one through preparestate / moveinput / updatestate of
    `mpc`, the plants in NumPy.  Returns the records as a dict, (B,n,N) each, and the controller's status (B,N)."""
    B, nd = mpc.B, mpc.nd
    models = []
    for b in range(B):
        model = es.LinModelOracle(plant["A"][b], plant["Bu"][b], plant["C"][b], plant["Bd"][b] if nd else None, plant["Dd"][b] if nd else None)
        model.setop(uop=mpc.uop[b], yop=mpc.yop[b], dop=mpc.dop[b], xop=plant["xop"][b], fop=plant["fop"][b])
        model.x0 = x_0[b] - plant["xop"][b]
        models.append(model)
    mpc.xhat0 = (xhat_0 - mpc.xhop).copy()
    mpc.lastu0 = (lastu - mpc.uop).copy()
    out = {k: [] for k in RECORDS + ("status",)}
    i_ym = mpc.i_ym
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for i in range(N):
            di = None
            if nd:
                di = d + d_step + d_noise * draws["w_d"][:, :, i]
            y = np.array([m.evaloutput(di[b] if nd else ()) for b, m in enumerate(models)]) + y_step + y_noise * draws["w_y"][:, :, i]
            ym = y[:, i_ym]
            x = np.array([m.x0 + m.xop for m in models])
            xhat = mpc.preparestate(ym, di)
            ry_i = ry[:, :, i] if ry.ndim == 3 else ry
            u = mpc.moveinput(None, ry_i, di, Rhatu=None if ru is None else np.tile(ru, mpc.Hp))
            ud = u + u_step + u_noise * draws["w_u"][:, :, i]
            yhat = np.einsum("bij,bj->bi", mpc._Chat, xhat - mpc.xhop) + mpc.yop
            if nd:
                yhat = yhat + np.einsum("bij,bj->bi", mpc._Dhd, di - mpc.dop)
            for k, v in (("Y_data", y), ("Ry_data", ry_i), ("Ŷ_data", yhat), ("U_data", u), ("Ud_data", ud),
                         ("Ru_data", mpc.uop if ru is None else ru), ("D_data", di if nd else np.zeros((B, 0))), ("X_data", x),
                         ("X̂_data", xhat), ("status", mpc.status)):
                out[k].append(np.array(v, copy=True))
            for b, m in enumerate(models):
                m.updatestate(ud[b], di[b] if nd else ())
                m.x0 = m.x0 + x_noise[b] * draws["w_x"][b, :, i] if np.ndim(x_noise) else m.x0
            mpc.updatestate(u, ym, di)
    return {k: np.stack(v, axis=-1) for k, v in out.items()}


def compare(res, ref):
    """Relative error of every record, and whether the statuses agree."""
    errs = {k: err(getattr(res, k), ref[k]) for k in RECORDS}
    return errs, bool(np.array_equal(res.status, ref["status"]))


def run_against_reference(case, lib=None):
    """`sim` on one fresh controller, the reference on its twin; returns (errors per record, result, reference, controller)."""
    mpc, twin = case.controller(lib), case.controller(lib)
    res = run(mpc, **case.args())
    kw = case.args()
    ref = reference(twin, **kw)
    errs, same = compare(res, ref)
    assert same, (res.status, ref["status"])
    # the controller goes on from period N like its twin
    errs["x̂0"], errs["lastu0"] = err(mpc.xhat0, twin.xhat0), err(mpc.lastu0, twin.lastu0)
    if not (case.kind.startswith("explicit")):
        errs["Z̃"] = err(mpc.Z, twin.Z)
    return errs, res, ref, mpc


def same_records(a, b, members=None, other=None):
    """Names of the records in which result `a` (its members `members`) differs from `b` (its members `other`) in any bit."""
    m = slice(None) if members is None else list(members)
    o = m if other is None else list(other)
    bad = [k for k in RECORDS if not np.array_equal(getattr(a, k)[m], getattr(b, k)[o], equal_nan=True)]
    if not np.array_equal(a.status[m], b.status[o]):
        bad.append("status")
    return bad
