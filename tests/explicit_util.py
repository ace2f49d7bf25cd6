"""Case runners of the batched ExplicitMPC shared by tests/test_explicit.py (CPU emulator) and tests/test_gpu_explicit.py
(the HIP library): every runner takes the library (`lib=None`: the product library) and returns the figures the tests bound.

The reference of every comparison is the oracle's closed form, -H̃⁻¹ q̃ by a NumPy solve on `orc.Ht`, `orc.qt`
(oracle/condense.py), at BAR = 1e-9 * max(1, max|reference|) -- the bar tests/test_gpu_parity.py uses for this closed form."""
import os
import subprocess

import numpy as np

import mpcqp
from mpcqp import synth
from oracle import condense as cd, estim as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "modelpredictivecontrol.jl_amd", "csrc")
EXPLICIT = "libmpcqp_emu_explicit.so"
BAR = 1e-9
# objects a stand-alone sanitizer program links next to its own compilation of csrc/mpcqp_host.hip
SANITIZER_OBJS = [os.path.join(EMU, o) for o in ("emu_launch.o", "emu_mhe.o", "emu_ms.o", "mhe_host.o", "emu_kf_cov.o",
                                                  "emu_mhe_wide.o", "emu_kf_dare.o", "emu_explicit.o")]
SANITIZER_CXX = ["g++", "-std=c++20", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                 "-I" + os.path.join(EMU, "fakehip"), "-I" + CSRC]


def build():
    """make tests/emu/libmpcqp_emu_explicit.so (tests/emu/explicit.mk); returns its path."""
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "explicit.mk", EXPLICIT])
    return os.path.join(EMU, EXPLICIT)


def err(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    return float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref))))) if ref.size else 0.0


def random_batch(nx, nu, ny, Hp, Hc, B, nd=0, seed=0, ops=False):
    """A seeded batch of stable plants with one output integrator each (synth.make_batch), optional measured disturbances and
    operating points on every signal."""
    cfg = synth.Config("explicit", nx=nx, nu=nu, ny=ny, Hp=Hp, Hc=Hc, Cwt=np.inf)
    bt = synth.make_batch(cfg, B, seed=seed)
    rng = np.random.default_rng([seed, 99])
    nxh = cfg.nxh
    bt["Bhd"] = bt["Dhd"] = None
    if nd:
        bt["Bhd"] = np.concatenate([rng.standard_normal((B, nx, nd)) / np.sqrt(nx), np.zeros((B, ny, nd))], axis=1)
        bt["Dhd"] = 0.3 * rng.standard_normal((B, ny, nd))
    z = lambda n: np.zeros(n)
    bt["ops"] = dict(uop=rng.standard_normal(nu) if ops else z(nu), yop=rng.standard_normal(ny) if ops else z(ny),
                     dop=rng.standard_normal(nd) if ops else z(nd), xhop=0.2 * rng.standard_normal(nxh) if ops else z(nxh),
                     fhop=0.2 * rng.standard_normal(nxh) if ops else z(nxh))
    bt["nd"], bt["nxh"] = nd, nxh
    return cfg, bt


def weight_matrix(kind, n, blk, B, seed):
    """A symmetric positive definite (B,n,n) weight: 'block' couples the `blk` channels of one step, 'dense' everything."""
    rng = np.random.default_rng([seed, n])
    if kind == "block":
        M = np.zeros((B, n, n))
        for t in range(n // blk):
            G = rng.standard_normal((B, blk, blk))
            M[:, t * blk:(t + 1) * blk, t * blk:(t + 1) * blk] = np.eye(blk) + 0.3 * G @ G.transpose(0, 2, 1)
        return M
    G = rng.standard_normal((B, n, n)) / np.sqrt(n)
    return np.eye(n) + 0.5 * G @ G.transpose(0, 2, 1)


def make_pair(cfg, bt, lib=None, law=False, weights=None, cls=None):
    """The batch controller and one oracle LinMPC (Cwt = Inf) per member."""
    w = dict(weights or {})
    B = bt["Ahat"].shape[0]
    cls = cls or mpcqp.BatchExplicitMPC
    kw = dict(law=law) if cls is mpcqp.BatchExplicitMPC else dict(Cwt=np.inf)
    mpc = cls(bt["Ahat"], bt["Bhu"], bt["Chat"], bt["Bhd"], bt["Dhd"], Hp=cfg.Hp, Hc=cfg.Hc, lib=lib, **bt["ops"], **w, **kw)
    orcs = []
    for b in range(B):
        wb = {k: (v[b] if (np.ndim(v) == 3 or (np.ndim(v) == 2 and k in ("Mwt", "Nwt", "Lwt"))) else v) for k, v in w.items()}
        orcs.append(cd.LinMPCOracle(bt["Ahat"][b], bt["Bhu"][b], bt["Chat"][b], None if bt["Bhd"] is None else bt["Bhd"][b],
                                    None if bt["Dhd"] is None else bt["Dhd"][b], Hp=cfg.Hp, Hc=cfg.Hc, Cwt=np.inf, **bt["ops"], **wb))
    return mpc, orcs


def period_inputs(cfg, bt, seed=1, full_ry=False, full_ru=False, preview=False):
    """Engineering-value inputs of one period: ry, d, lastu and the optional horizon-long R̂y, R̂u, D̂."""
    B, nd = bt["Ahat"].shape[0], bt["nd"]
    rng = np.random.default_rng([seed, 7])
    o = bt["ops"]
    inp = dict(x=bt["xhat0"], ry=bt["ry"] + o["yop"], lastu=bt["lastu0"] + o["uop"], d=None, Dhat=None, Rhaty=None, Rhatu=None)
    if nd:
        inp["d"] = rng.standard_normal((B, nd)) + o["dop"]
        if preview:
            inp["Dhat"] = rng.standard_normal((B, nd * cfg.Hp)) + np.tile(o["dop"], cfg.Hp)
    if full_ry:
        inp["Rhaty"] = 2.0 * rng.standard_normal((B, cfg.ny * cfg.Hp))
    if full_ru:
        inp["Rhatu"] = rng.standard_normal((B, cfg.nu * cfg.Hp))
    return inp


def oracle_period(orcs, inp):
    """Closed form of every member: Z̃ = -H̃⁻¹ q̃ (NumPy solve), u, Ŷ."""
    Z, U, Y = [], [], []
    g = lambda k, b: None if inp[k] is None else inp[k][b]
    for b, orc in enumerate(orcs):
        orc.initpred(inp["x"][b], inp["lastu"][b], inp["ry"][b], g("d", b), g("Dhat", b), g("Rhaty", b), g("Rhatu", b))
        z = -np.linalg.solve(orc.Ht, orc.qt)
        Z.append(z)
        U.append(z[:orc.nu] + orc.lastu0 + orc.uop)
        Y.append(orc.Et @ z + orc.F + orc.Yop)
    return np.array(Z), np.array(U), np.array(Y)


def step_call(mpc, inp, want_info=True):
    u = mpc.moveinput(inp["x"], inp["ry"], inp["d"], lastu=inp["lastu"], Dhat=inp["Dhat"], Rhaty=inp["Rhaty"], Rhatu=inp["Rhatu"],
                      want_info=want_info)
    return mpc.Z.copy(), u, (mpc.getinfo()["Ŷ"] if want_info else None), mpc.status.copy()


def run_shape(lib=None, *, nx, nu, ny, Hp, Hc, B, nd=0, ops=False, weights=None, Mkind=None, Lkind=None, Nkind=None,
              full_ry=False, full_ru=False, preview=False, law=False, seed=0):
    """One period of a random batch on the explicit step, against the oracle closed form and against mpcqp_step's no-row
    path on the same handle; with `law` also the law call and the law tables.  Returns a dict of relative errors."""
    cfg, bt = random_batch(nx, nu, ny, Hp, Hc, B, nd=nd, seed=seed, ops=ops)
    w = dict(weights or {})
    if Mkind:
        w["M_Hp"] = weight_matrix(Mkind, ny * Hp, ny, B, seed + 1)
    if Lkind:
        w["L_Hp"] = weight_matrix(Lkind, nu * Hp, nu, B, seed + 2) * 0.2
    if Nkind:
        w["N_Hc"] = weight_matrix(Nkind, nu * cfg.Hc, nu, B, seed + 3) * 0.1
    mpc, orcs = make_pair(cfg, bt, lib=lib, law=law, weights=w)
    inp = period_inputs(cfg, bt, seed=seed, full_ry=full_ry, full_ru=full_ru, preview=preview)
    Zo, Uo, Yo = oracle_period(orcs, inp)
    Z, u, Y, st = step_call(mpc, inp)
    out = dict(status=st, factor_status=mpc.hd.explicit_status(), Z=err(Z, Zo), u=err(u, Uo), Y=err(Y, Yo), cond=float(np.linalg.cond(orcs[0].Ht)))
    # mpcqp_step on the same handle: no finite row, the closed form inside the interior-point kernel
    # (called on the handle, which never compiles: the runtime-dimension kernel unless the shape has a kernel in the library)
    o = bt["ops"]
    held = inp["Rhaty"] is None
    Ry0 = (inp["ry"] - o["yop"]) if held else inp["Rhaty"] - np.tile(o["yop"], Hp)
    Ru0 = None if inp["Rhatu"] is None else inp["Rhatu"] - np.tile(o["uop"], Hp)
    d0 = None if not nd else inp["d"] - o["dop"]
    Dh0 = None if not nd else (np.tile(d0, Hp) if inp["Dhat"] is None else inp["Dhat"] - np.tile(o["dop"], Hp))
    Zs = np.zeros((B, mpc.nZ))
    mpc.hd.step(inp["x"], inp["lastu"] - o["uop"], Ry0, Zs, Ru=Ru0, d0=d0, Dhat0=Dh0)
    out["step_vs_mpcqp_step"] = err(Z, Zs)
    if law:
        held = not (full_ry or full_ru or preview)
        if held:
            Zl, ul, stl = mpc.hd.explicit_law(inp["x"], inp["lastu"] - o["uop"], inp["ry"] - o["yop"], d0)
            _, ul2, _ = mpc.hd.explicit_law(inp["x"], inp["lastu"] - o["uop"], inp["ry"] - o["yop"], d0, want_Z=False)
            out.update(law_Z=err(Zl, Zo), law_vs_step=err(Zl, Z), law_u=err(ul + o["uop"], Uo), law_u_only=err(ul2, ul), law_status=stl)
        out["law_tables"] = err(mpc.hd.get(mpcqp.api.GET_EXPLICIT_LAW), oracle_law(orcs))
    out["mpc"], out["orcs"], out["inp"], out["bt"], out["cfg"] = mpc, orcs, inp, bt, cfg
    return out


def oracle_law(orcs):
    """(B, 1+nx̂+nu+ny+nd, nZ): gains [g0 Gx Gu Gr Gd] of Z̃ = g0 + Gx x̂0 + Gu lastu0 + Gr ry0 + Gd d0 in deviation variables,
    from the oracle's dense matrices: q̃ = 2 [Ẽ'M (B + K x̂0 + V lastu0 + (G + J 1) d0 - 1 ry0) + P̃u'L Tu lastu0]."""
    out = []
    for o in orcs:
        Hi = np.linalg.inv(o.Ht)
        EM, PL = 2.0 * o.Et.T @ o.M_Hp, 2.0 * o.Put.T @ o.L_Hp
        rep_y = np.tile(np.eye(o.ny), (o.Hp, 1))
        cols = [EM @ o.B, EM @ o.K, EM @ o.V + PL @ o.Tu, -EM @ rep_y]
        if o.nd:
            cols.append(EM @ (o.G + o.J @ np.tile(np.eye(o.nd), (o.Hp, 1))))
        Q = np.column_stack([c.reshape(o.nZt, -1) for c in cols])
        out.append((-Hi @ Q).T)
    return np.array(out)


def run_refresh(lib=None, B=3, law=True, seed=3):
    """set_model with Â scaled by 0.9: step and law against a rebuilt oracle, and their distance from the stale answer."""
    cfg, bt = random_batch(4, 2, 2, 12, 3, B, seed=seed)
    mpc, _ = make_pair(cfg, bt, lib=lib, law=law)
    inp = period_inputs(cfg, bt, seed=seed)
    Zstale, *_ = step_call(mpc, inp, want_info=False)
    bt2 = dict(bt, Ahat=0.9 * bt["Ahat"])
    mpc.setmodel(bt2["Ahat"], bt2["Bhu"], bt2["Chat"])
    _, orcs = make_pair(cfg, bt2, lib=lib, cls=_NoController)
    Zo, Uo, _ = oracle_period(orcs, inp)
    Z, u, _, _ = step_call(mpc, inp, want_info=False)
    out = dict(step=err(Z, Zo), moved=float(np.max(np.abs(Z - Zstale))))
    if law:
        Zl, _, _ = mpc.hd.explicit_law(inp["x"], inp["lastu"], inp["ry"])
        out.update(law=err(Zl, Zo), law_moved=float(np.max(np.abs(Zl - Zstale))), law_tables=err(mpc.hd.get(mpcqp.api.GET_EXPLICIT_LAW), oracle_law(orcs)))
    return out


class _NoController:
    """make_pair(cls=_NoController): the oracles alone."""
    def __init__(self, *a, **k):
        pass


def run_status_policy(lib=None, B=5, bad=2, seed=4):
    """Member `bad` with Mwt = Nwt = Lwt = 0 (H̃ = 0): status 2, Z̃ = 0, u0 = lastu0 from step and law; every other member
    bit for bit what it is in a run in which that member is regular."""
    cfg, bt = random_batch(4, 2, 2, 10, 3, B, seed=seed)
    inp = period_inputs(cfg, bt, seed=seed)
    res = {}
    for name, zero in (("regular", False), ("failed", True)):
        M, N, L = np.ones((B, 2)), np.full((B, 2), 0.1), np.full((B, 2), 0.05)
        if zero:
            M[bad] = N[bad] = L[bad] = 0.0
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            mpc = mpcqp.BatchExplicitMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], Hp=cfg.Hp, Hc=cfg.Hc, Mwt=M, Nwt=N, Lwt=L, law=True, lib=lib)
        Z, u, Y, st = step_call(mpc, inp)
        Zl, ul, stl = mpc.hd.explicit_law(inp["x"], inp["lastu"], inp["ry"])
        res[name] = dict(Z=Z, u=u, Y=Y, st=st, Zl=Zl, ul=ul, stl=stl, fst=mpc.hd.explicit_status(), tab=mpc.hd.get(mpcqp.api.GET_EXPLICIT_LAW))
    res["bad"], res["lastu"] = bad, inp["lastu"]
    return res


def tf_pair(gain, tau, Ts, B=3, lib=None, law=False, cls=None, **kw):
    """B identical controllers on the first-order plant gain / (tau s + 1) with the default estimator's augmentation, and the
    oracle estimator that carries x̂0."""
    op = {k: kw.pop(k) for k in ("uop", "yop") if k in kw}
    A, Bm, C = es.tf1_zoh(gain, tau, Ts)
    model = es.LinModelOracle(A, Bm, C, Ts=Ts).setop(**op)
    kf = es.SteadyKalmanFilterOracle(model)
    rep = lambda a: np.broadcast_to(a, (B,) + a.shape).copy()
    cls = cls or mpcqp.BatchExplicitMPC
    extra = dict(law=law) if cls is mpcqp.BatchExplicitMPC else dict(Cwt=np.inf)
    mpc = cls(rep(kf.Ah), rep(kf.Bhu), rep(kf.Ch), uop=model.uop, yop=model.yop, xhop=kf.xhop, fhop=kf.fhop, lib=lib, **kw, **extra)
    return model, kf, mpc


def run_T7_closed_loop(lib=None, B=3, N=25, law=False):
    """test/3_test_predictive_control.jl:1593-1630: 25 closed-loop periods on tf(10, [400, 1]), Ts = 100, Hp = 30,
    Hc = [2, 3, 4, 21], Mwt = 1, Nwt = 0, r = 5: the ExplicitMPC against the unconstrained LinMPC (Cwt = Inf).  Returns both
    input series, (N, B)."""
    kw = dict(Mwt=[1], Nwt=[0], Hp=30, Hc=[2, 3, 4, 21])
    model, kf, mpc0 = tf_pair(10.0, 400.0, 100.0, B=B, lib=lib, law=law, **kw)
    _, _, mpc1 = tf_pair(10.0, 400.0, 100.0, B=B, lib=lib, cls=mpcqp.BatchLinMPC, **kw)
    Kh = np.broadcast_to(kf.Khat, (B,) + kf.Khat.shape).copy()
    for m in (mpc0, mpc1):
        m.setestimator(Kh)
    U0, U1 = np.zeros((N, B)), np.zeros((N, B))
    for i in range(N):
        y = np.tile(model.evaloutput(), (B, 1))
        for m in (mpc0, mpc1):
            m.preparestate(y)
        u0, u1 = mpc0.moveinput(None, [5.0]), mpc1.moveinput(None, [5.0])
        U0[i], U1[i] = u0[:, 0], u1[:, 0]
        mpc0.updatestate(u0, y)
        mpc1.updatestate(u1, y)
        model.updatestate(u1[0])
    return U0, U1
