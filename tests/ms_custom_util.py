"""Helpers of the custom-linear-constraint tests of the stage-structured (MultipleShooting) kernel: custom rows
wmin <= Wy ŷ + Wu u + Wd d̂ + Wr r̂ <= wmax (construct.jl:1138-1160, execute.jl:337-364) under MultipleShooting, and on
SingleShooting problems beyond the LDS, against the condensed oracle (both transcriptions solve the same QP).  Written
after tests/parity_util.py (custom_constraint_cases, run_soft_custom_constraints), which is left as it is."""
import warnings

import numpy as np

import mpcqp
from mpcqp import api
from oracle import condense as cd
from tests.parity_util import custom_constraint_cases

TOL = 1e-5


def rep(a, B):
    a = np.asarray(a, dtype=float)
    return np.broadcast_to(a, (B,) + a.shape).copy()


def no_fallback_step(g, *args, **kw):
    """moveinput with every warning turned into an error: a MultipleShooting controller that falls back to the condensed
    kernels (RuntimeWarning of api.py) fails here."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return g.moveinput(*args, **kw)


def block_starts(Hp, Hc):
    """First step of every move-blocking interval (construct.jl:597-660; the oracle's move_blocking)."""
    nb = cd.move_blocking(Hp, Hc)
    return [int(v) for v in np.cumsum([0] + list(nb)[:-1])]


def rollout_defect(g, i, x0dev, lastu0dev, Hc, d0dev=None, Dhat0dev=None, ops=None):
    """max |X̂0 returned by the kernel - X̂0 rolled out from the returned ΔU| of member i (deviation variables, the model
    equations of transcription.jl:386-389), relative to 1 + max |X̂0|.  ops: (Ah, Bhu, Bhd, fhop - xhop) of that member."""
    Ah, Bhu, Bhd, f = ops
    nu, Hp = Bhu.shape[1], g.Hp
    starts = block_starts(Hp, Hc)
    DU = g.Z[i, :nu * len(starts)].reshape(-1, nu)
    X = g.hd.get(api.GET_XHAT_MS)[i]
    x, u = np.array(x0dev, float), np.array(lastu0dev, float)
    worst, scale = 0.0, 1.0 + np.abs(X).max()
    for t in range(Hp):
        if t in starts:
            u = u + DU[starts.index(t)]
        dd = 0.0
        if Bhd is not None and Bhd.shape[1]:
            dd = Bhd @ (d0dev if t == 0 else Dhat0dev[(t - 1) * Bhd.shape[1]:t * Bhd.shape[1]])
        x = Ah @ x + Bhu @ u + dd + f
        worst = max(worst, np.abs(X[t] - x).max() / scale)
    return worst


def run_t9(lib=None, B=2, Hp=12, which=(0, 1, 2, 3), transcription="MultipleShooting"):
    """T9 (test/3_test_predictive_control.jl:466-495) with the given transcription: returns the worst relative difference
    of Z̃[:nDU] / W to the condensed oracle, the reason masks, the kernel kinds, the worst defect of the returned X̂0 and
    the worst X̂0 rollout difference.  At Hp = 50 the reference's expected values are asserted too."""
    model, kf, cases = custom_constraint_cases()
    worst, whys, kinds, defect, xroll = 0.0, [], [], 0.0, 0.0
    for kwW, wmin, wmax, checks in [cases[i] for i in which]:
        kw = dict(Hp=Hp, Hc=Hp, Nwt=[0], Cwt=np.inf, uop=model.uop, yop=model.yop, dop=model.dop,
                  xhop=kf.xhop, fhop=kf.fhop)
        orc = cd.LinMPCOracle(kf.Ah, kf.Bhu, kf.Ch, kf.Bhd, kf.Dhd, **kw, **kwW)
        orc.setconstraint(wmin=wmin, wmax=wmax)
        g = mpcqp.BatchLinMPC(rep(kf.Ah, B), rep(kf.Bhu, B), rep(kf.Ch, B), rep(kf.Bhd, B), rep(kf.Dhd, B), lib=lib,
                              transcription=transcription, **kw, **kwW)
        g.setconstraint(wmin=wmin, wmax=wmax)
        x0 = np.zeros(kf.nxh)
        g.initstate([25.0]); orc.lastu0 = np.zeros(1)
        ops = (kf.Ah, kf.Bhu, kf.Bhd, kf.fhop - kf.xhop)
        for ry, key, want in checks:
            lastu0 = orc.lastu0.copy()
            ug = no_fallback_step(g, np.tile(x0, (B, 1)), [ry], [30.0], want_info=True)
            orc.moveinput(x0, [ry], [30.0])
            assert np.all(g.status == 0), g.status
            whys.append(g.hd.transcription_supported())
            kinds.append(g.kernel)
            ig, io = g.getinfo(), orc.getinfo()
            if Hp == 50:
                assert np.all(np.abs(ig[key][B - 1] - want) < 1e-1), (kwW, ry, ig[key][B - 1], want)
            nDU = g.nDU
            worst = max(worst, np.abs(g.Z[:, :nDU] - orc.Zt[:nDU]).max() / max(1.0, np.abs(orc.Zt[:nDU]).max()),
                        np.abs(ig["W"] - io["W"]).max() / max(1.0, np.abs(io["W"]).max()))
            if g.kernel == api.KERNEL_MS:
                defect = max(defect, float(g.hd.get(api.GET_MS_DEFECT).max()))
                d0 = np.array([30.0]) - model.dop
                xroll = max(xroll, rollout_defect(g, B - 1, x0, lastu0, Hp, d0, np.tile(d0, Hp), ops))
            del ug
    return dict(worst=worst, whys=whys, kinds=kinds, defect=defect, xroll=xroll)


def run_soft_custom(lib=None, B=2, seed=4, Hp=8, Hc=(1, 2, 2), Cwt=1e5, periods=3, no_polish=False):
    """Closed loop of `periods` control periods of the soft custom-row case under MultipleShooting against the condensed
    oracle.  Returns dict(worst difference, kinds, masks, max active custom-row slack |W - bound| at the optimum, defects,
    X̂0 rollout difference)."""
    from oracle import estim as es
    rng = np.random.default_rng(seed)
    A = np.diag([0.85, 0.6, 0.3]); Bu = rng.standard_normal((3, 2)); C = rng.standard_normal((2, 3))
    Bd = rng.standard_normal((3, 1)); Dd = rng.standard_normal((2, 1))
    model = es.LinModelOracle(A, Bu, C, Bd, Dd).setop(uop=[0.5, -0.2], yop=[2.0, 1.0], dop=[0.3])
    kf = es.SteadyKalmanFilterOracle(model)
    Wy, Wu = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
    Wd, Wr = rng.standard_normal((2, 1)), 0.3 * rng.standard_normal((2, 2))
    kw = dict(Hp=Hp, Hc=list(Hc) if not np.isscalar(Hc) else int(Hc), Lwt=[0.05, 0.02], Cwt=Cwt, uop=model.uop,
              yop=model.yop, dop=model.dop, xhop=kf.xhop, fhop=kf.fhop, Wy=Wy, Wu=Wu, Wd=Wd, Wr=Wr)
    orc = cd.LinMPCOracle(kf.Ah, kf.Bhu, kf.Ch, kf.Bhd, kf.Dhd, **kw)
    g = mpcqp.BatchLinMPC(rep(kf.Ah, B), rep(kf.Bhu, B), rep(kf.Ch, B), rep(kf.Bhd, B), rep(kf.Dhd, B), lib=lib,
                          transcription="MultipleShooting", **kw)
    if no_polish:
        g.hd.set_flags(g.hd.flags | api.FLAG_NO_POLISH)
    wmin, wmax = np.array([0.2, -np.inf]), np.array([1.5, 0.9])
    con = dict(umin=[-0.6, -1.0], umax=[1.4, 0.9], ymax=[2.6, 1.8], wmin=wmin, wmax=wmax)
    if np.isfinite(Cwt):
        con.update(c_wmin=[0.7, 1.0], c_wmax=[1.3, 0.4])
    orc.setconstraint(**con); g.setconstraint(**con)
    x0 = 0.3 * rng.standard_normal(kf.nxh)
    g.initstate([0.6, 0.0]); orc.lastu0 = np.array([0.6, 0.0]) - model.uop
    out = dict(worst=0.0, kinds=[], whys=[], active=np.inf, defect=0.0, xroll=0.0, eps=[])
    ops = (kf.Ah, kf.Bhu, kf.Bhd, kf.fhop - kf.xhop)
    for k in range(periods):
        ry, d = [2.5 + 0.2 * k, 0.4], [0.5 - 0.1 * k]
        lastu0 = orc.lastu0.copy()
        ug = no_fallback_step(g, np.tile(x0, (B, 1)), ry, d, want_info=True)
        uo = orc.moveinput(x0, ry, d)
        assert np.all(g.status == 0), g.status
        assert orc.status == 0
        out["kinds"].append(g.kernel); out["whys"].append(g.hd.transcription_supported())
        ig, io = g.getinfo(), orc.getinfo()
        out["worst"] = max(out["worst"], np.abs(g.Z - orc.Zt).max() / max(1.0, np.abs(orc.Zt).max()),
                           np.abs(ug - uo).max(), np.abs(ig["W"] - io["W"]).max() / max(1.0, np.abs(io["W"]).max()))
        W = io["W"].reshape(Hp + 1, 2)
        eps = orc.Zt[-1] if np.isfinite(Cwt) else 0.0
        out["eps"].append(eps)
        gap = np.concatenate([np.abs(W[:, 0] - (wmin[0] - 0.7 * eps)), np.abs(W - (wmax + np.array([1.3, 0.4]) * eps)).ravel()])
        out["active"] = min(out["active"], gap.min())
        out["defect"] = max(out["defect"], float(g.hd.get(api.GET_MS_DEFECT).max()))
        d0 = np.array(d) - model.dop
        out["xroll"] = max(out["xroll"], rollout_defect(g, B - 1, x0, lastu0, kw["Hc"], d0, np.tile(d0, Hp), ops))
        x0 = kf.Ah @ x0 + kf.Bhu @ (uo - model.uop) * 0.5
    return out


def custom_oracle_check(g, orcs, x0s, lus, rys, members, d=None):
    """Worst relative ΔU / ϵ difference of the members `members` of g (after its step) to their condensed oracles."""
    worst = 0.0
    nDU = g.nDU
    for i in members:
        o = orcs[i]
        o.lastu0 = np.array(lus[i], float)
        if d is None:
            o.moveinput(x0s[i], rys[i])
        else:
            o.moveinput(x0s[i], rys[i], d[0], Dhat=d[1])
        assert o.status == 0, (i, o.status)
        worst = max(worst, np.abs(g.Z[i, :nDU] - o.Zt[:nDU]).max() / max(1.0, np.abs(o.Zt[:nDU]).max()))
        if g.Z.shape[1] > nDU:
            worst = max(worst, abs(g.Z[i, -1] - o.Zt[-1]) / max(1.0, abs(o.Zt[-1])))
    return worst


def random_custom_family(seed, lib=None, B=4, transcription="MultipleShooting"):
    """A randomised controller family with custom rows: plant dimensions, move blocking, nd > 0 with a varying D̂ preview,
    soft or hard custom rows (finite Cwt or Inf) with ±Inf holes in Wmin / Wmax, on top of random u / Δu / y bounds.  B
    members share the weights and constraints and differ in x̂0, u(k-1), ry.  Returns dict(worst difference to the
    condensed oracle, statuses, kernel kind, reason mask, defect of X̂0)."""
    rng = np.random.default_rng([31, seed])
    nx, nu, ny = int(rng.integers(2, 5)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
    nd = int(rng.integers(0, 2)) if seed % 2 else 1
    nw = int(rng.integers(1, 3))
    Hp = int(rng.integers(6, 15))
    Hc = [int(v) for v in rng.integers(1, 4, size=3)] if seed % 3 == 0 else int(rng.integers(2, Hp))
    A = rng.standard_normal((nx, nx)); A *= rng.uniform(0.6, 0.98) / max(abs(np.linalg.eigvals(A)))
    Bu, C = rng.standard_normal((nx, nu)), rng.standard_normal((ny, nx))
    Bd, Dd = rng.standard_normal((nx, nd)), 0.5 * rng.standard_normal((ny, nd))
    Cwt = np.inf if seed % 4 == 1 else 1e5
    kw = dict(Hp=Hp, Hc=Hc, Mwt=rng.uniform(0.5, 2.0, ny), Nwt=rng.uniform(0.05, 0.3, nu), Lwt=rng.uniform(0.0, 0.05, nu),
              Cwt=Cwt, Wy=rng.standard_normal((nw, ny)), Wu=rng.standard_normal((nw, nu)))
    if nd:
        kw["Wd"] = 0.5 * rng.standard_normal((nw, nd))
    if seed % 2 == 0:
        kw["Wr"] = 0.3 * rng.standard_normal((nw, ny))
    wmin, wmax = -rng.uniform(0.3, 1.0, nw), rng.uniform(0.3, 1.0, nw)
    wmin[rng.random(nw) < 0.3] = -np.inf
    wmax[rng.random(nw) < 0.3] = np.inf
    if not np.isfinite(wmin).any() and not np.isfinite(wmax).any():
        wmax[0] = 0.5
    if not np.isfinite(Cwt):                 # (hard rows: wide enough to keep every member feasible)
        wmin, wmax = wmin - 2.0, wmax + 2.0
    con = dict(umin=np.full(nu, -1.5), umax=np.full(nu, 1.5), wmin=wmin, wmax=wmax)
    if seed % 2 and np.isfinite(Cwt):
        con.update(dumin=np.full(nu, -0.5), dumax=np.full(nu, 0.5))
    if np.isfinite(Cwt):
        con["ymax"] = np.full(ny, 1.2)
        con.update(c_wmin=rng.uniform(0.5, 1.5, nw), c_wmax=rng.uniform(0.5, 1.5, nw))
    gcon = {{"dumin": "Δumin", "dumax": "Δumax"}.get(k, k): v for k, v in con.items()}
    args = (A, Bu, C) + ((Bd, Dd) if nd else ())
    g = mpcqp.BatchLinMPC(*[rep(a, B) for a in args], lib=lib, transcription=transcription, **kw)
    g.setconstraint(**gcon)
    orcs = []
    for _ in range(B):
        o = cd.LinMPCOracle(*args, **kw)
        o.setconstraint(**con)
        orcs.append(o)
    x0s = 0.3 * rng.standard_normal((B, nx))
    lus = 0.3 * rng.standard_normal((B, nu))
    rys = 0.5 * rng.standard_normal((B, ny))
    g.lastu0 = lus.copy()
    dargs = None
    if nd:
        dk = rng.standard_normal(nd)
        Dh = dk + 0.2 * np.cumsum(rng.standard_normal((Hp, nd)), axis=0).ravel()     # a preview that varies over the horizon
        dargs = (dk, Dh)
        no_fallback_step(g, x0s, rys, dk, Dhat=Dh)
    else:
        no_fallback_step(g, x0s, rys)
    out = dict(status=g.status.copy(), kind=g.kernel, why=g.hd.transcription_supported(),
               defect=float(g.hd.get(api.GET_MS_DEFECT).max()) if g.kernel == api.KERNEL_MS else 0.0)
    out["worst"] = custom_oracle_check(g, orcs, x0s, lus, rys, range(B), dargs)
    return out


def beyond_lds_with_custom_rows(lib=None, B=256, check=range(0, 256, 32)):
    """SingleShooting 12,4,4,46,46 (nZ̃ = 185: the condensed problem does not fit the LDS of a CU) plus two soft custom
    rows on ŷ and u: runs on the stage-structured kernel.  Returns dict(kind, why, status, worst of the checked members)."""
    from mpcqp import synth
    from tests.parity_util import constraint_kwargs
    cfg = synth.get_config("12,4,4,46,46")
    bt = synth.make_batch(cfg, B, seed=11)
    rng = np.random.default_rng(3)
    Wy, Wu = 0.5 * rng.standard_normal((2, cfg.ny)), 0.5 * rng.standard_normal((2, cfg.nu))
    kw = dict(Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt, Mwt=np.full(cfg.ny, cfg.Mwt), Nwt=np.full(cfg.nu, cfg.Nwt),
              Lwt=np.full(cfg.nu, cfg.Lwt), Wy=Wy, Wu=Wu)
    wcon = dict(wmin=[-0.8, -np.inf], wmax=[0.8, 0.6])
    if np.isfinite(cfg.Cwt):
        wcon.update(c_wmin=[1.0, 0.5], c_wmax=[1.0, 0.5])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")               # (the reroute to the stage kernel is announced: expected here)
        g = mpcqp.BatchLinMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], lib=lib, **kw)
        g.setconstraint(**constraint_kwargs(cfg), **wcon)
        g.lastu0 = bt["lastu0"].copy()
        g.moveinput(bt["xhat0"], bt["ry"])
    orcs = {}
    for i in check:
        o = cd.LinMPCOracle(bt["Ahat"][i], bt["Bhu"][i], bt["Chat"][i], **kw)
        o.setconstraint(**constraint_kwargs(cfg, oracle=True), **wcon)
        orcs[i] = o
    worst = custom_oracle_check(g, orcs, bt["xhat0"], bt["lastu0"], bt["ry"], check)
    return dict(kind=g.kernel, why=g.hd.transcription_supported(), status=g.status.copy(), worst=worst)


def unstable_plant_with_custom_rows(lib=None, B=16, check=range(0, 16, 4), rho=(1.12, 1.05)):
    """The unstable plants of parity_util.unstable_plant_members (Hp = Hc = 50) plus one hard and one soft custom row
    mixing ŷ and u, under MultipleShooting, against the condensed oracle.  Returns dict(kind, status, worst, defect)."""
    from tests.parity_util import unstable_plant_members
    mem = unstable_plant_members(B, rho=rho)
    st = lambda f: np.stack([f(m) for m in mem])
    ny, nu = mem[0]["Ch"].shape[0], mem[0]["Bhu"].shape[1]
    Wy = np.array([[0.5, -0.3] + [0.0] * (ny - 2), [0.2, 0.4] + [0.0] * (ny - 2)])
    Wu = np.array([[0.3, 0.1] + [0.0] * (nu - 2), [-0.2, 0.5] + [0.0] * (nu - 2)])
    kw = dict(mem[0]["kw"], Wy=Wy, Wu=Wu)
    c = mem[0]["con"]
    wcon = dict(wmin=[-1.0, -np.inf], wmax=[1.0, 0.4], c_wmin=[0.0, 1.0], c_wmax=[0.0, 1.0])
    g = mpcqp.BatchLinMPC(st(lambda m: m["Ah"]), st(lambda m: m["Bhu"]), st(lambda m: m["Ch"]), lib=lib,
                          transcription="MultipleShooting", **kw)
    g.setconstraint(umin=c["umin"], umax=c["umax"], Δumin=c["dumin"], Δumax=c["dumax"], ymax=c["ymax"], **wcon)
    no_fallback_step(g, st(lambda m: m["x0"]), st(lambda m: m["ry"]))
    orcs = {}
    for i in check:
        m = mem[i]
        o = cd.LinMPCOracle(m["Ah"], m["Bhu"], m["Ch"], **kw)
        o.setconstraint(**c, **wcon)
        orcs[i] = o
    worst = custom_oracle_check(g, orcs, st(lambda m: m["x0"]), np.zeros((B, nu)), st(lambda m: m["ry"]), check)
    return dict(kind=g.kernel, status=g.status.copy(), worst=worst, defect=float(g.hd.get(api.GET_MS_DEFECT).max()))


def fused_loop_custom(lib=None, B=3, periods=4, torch_device=None):
    """mpcqp_loop_device against the three separate entry points on a MultipleShooting handle with custom rows (after
    parity_util.fused_loop_vs_separate_steps): max |difference| of x̂0, u0, Z̃ over the periods (expected 0)."""
    from mpcqp import synth
    cfg = synth.Config("loopw", nx=3, nu=2, ny=2, Hp=8, Hc=3, umin=-0.6, umax=0.7, ymax=0.9)
    bt = synth.make_batch(cfg, B, seed=12)
    K = mpcqp.steady_kalman_gain(bt["Ahat"], bt["Chat"], np.eye(cfg.nxh), np.eye(cfg.ny))
    nw = 2
    Wy = np.array([[1.0, -0.5], [0.3, 0.8]]); Wu = np.array([[0.4, 0.0], [-0.6, 1.0]])

    def make():
        hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, cfg.Hc, neps=1, flags=mpcqp.FLAG_RY_CONSTANT, lib=lib)
        hd.set_transcription(api.MULTIPLE_SHOOTING)
        hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
        hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt), np.full(B, cfg.Cwt))
        hd.set_bounds(U0min=np.full((B, hd.nU), cfg.umin), U0max=np.full((B, hd.nU), cfg.umax), Y0max=np.full((B, hd.nY), cfg.ymax))
        hd.set_custom_constraints(nw, mpcqp.colmajor(rep(Wy, B)), mpcqp.colmajor(rep(Wu, B)))
        nW = nw * (cfg.Hp + 1)
        hd.set_custom_bounds(np.tile([-0.5, -np.inf], (B, cfg.Hp + 1)), np.tile([0.5, 0.4], (B, cfg.Hp + 1)),
                             np.ones((B, nW)), np.full((B, nW), 0.5))
        hd.kf_set(mpcqp.colmajor(K), np.arange(cfg.ny))
        assert hd.transcription_supported() == 0
        assert hd.prepare() == api.KERNEL_MS
        return hd

    if torch_device is None:
        new = lambda a: np.ascontiguousarray(a).copy()
        ptr = lambda a: a.ctypes.data
        host = lambda a: a
        sync = lambda: None
    else:
        import torch
        new = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch_device)
        ptr = lambda a: a.data_ptr()
        host = lambda a: a.cpu().numpy()
        sync = torch.cuda.synchronize
    runs = []
    for fused in (False, True):
        hd = make()
        x = new(bt["xhat0"]); lu = new(bt["lastu0"]); ry = new(bt["ry"])
        Z = new(np.zeros((B, hd.nZ))); u0 = new(np.zeros((B, cfg.nu)))
        st = new(np.zeros(B, np.int32)); it = new(np.zeros(B, np.int32))
        rg = np.random.default_rng(7)
        out = []
        for k in range(periods):
            y = new(0.3 * rg.standard_normal((B, cfg.ny)))
            if fused:
                hd.loop_device(ptr(x), ptr(y), ptr(lu), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
            else:
                hd.kf_correct_device(ptr(x), ptr(y))
                hd.step_device(ptr(x), ptr(lu), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
                hd.kf_predict_device(ptr(x), ptr(u0))
            sync()
            assert np.all(host(st) == 0)
            out.append((host(x).copy(), host(u0).copy(), host(Z).copy()))
            lu, u0 = u0, lu
        runs.append(out)
    return max(float(np.abs(a - b).max()) for pa, pb in zip(*runs) for a, b in zip(pa, pb))
