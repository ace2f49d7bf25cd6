"""Shared by tests/test_im.py (CPU wave emulator) and tests/test_gpu_im.py (MI355X): a NumPy restatement of the InternalModel
estimator (src/estimator/internal_model.jl) and the runners of both twins.

The restatement forms the stochastic prediction from the TABLES Ks, Ps of init_stochpred (construct.jl:1254-1267), Ŷs =
Ks x̂s + Ps ŷs -- the device runs the recurrence Ŷs_t = Cs As^(t-1) (Âs x̂s + B̂s ŷs) -- and can also run the recurrence itself
(`tables=False`): the largest difference between the two on a test's own inputs is δ, the rounding level of that problem.
The bar of the estimator quantities is 32 δ, floored at 1e-13 times the largest magnitude of the quantity (`bar`).

The controller oracle is oracle.condense.LinMPCOracle with `orc.B = B_model + Ŷs` assigned before each period."""
import os
import subprocess
import warnings

import numpy as np

import mpcqp
from mpcqp import api, synth
from oracle import condense as cd, qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
IM = "libmpcqp_emu_im.so"
TOL = 1e-5              # tests/test_gpu_parity.py: relative ΔU error of a solve against the oracle
FBAR = 1e-11            # ... and of F (there: 1e-11 max(1, max|F|))
QUANTITIES = ("ys", "xs", "xd", "Yhs")


def build():
    """make tests/emu/libmpcqp_emu_im.so (tests/emu/im.mk); returns its path."""
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "im.mk", IM])
    return os.path.join(EMU, IM)


def mv(M, v):
    return np.einsum("bij,bj->bi", M, v)


class ImRef:
    """The estimator of every member in NumPy: arrays carry a leading batch axis; stoch = (As, Bs, Cs, Ds) on the measured
    outputs.  Members whose Ds is singular (`off`) have no stochastic part, like status 2 of the library."""

    def __init__(self, A, Bu, C, Bd, Dd, fx, stoch, i_ym, Hp, tables=True, off=None):
        self.A, self.Bu, self.C, self.fx = A, Bu, C, fx
        B, self.ny = A.shape[0], C.shape[1]
        self.nd = 0 if Bd is None else Bd.shape[2]
        self.Bd = np.zeros(A.shape[:2] + (0,)) if Bd is None else Bd
        self.Dd = np.zeros((B, self.ny, 0)) if Dd is None else Dd
        self.i_ym, self.Hp, self.tables = np.asarray(i_ym), Hp, tables
        As, Bs, Cs, Ds = (np.array(m, float) for m in stoch)
        off = np.zeros(B, bool) if off is None else np.asarray(off)
        Ds = np.where(off[:, None, None], np.eye(Ds.shape[1]), Ds)
        self.As, self.Cs = As, Cs
        self.Bhs = np.linalg.solve(Ds.transpose(0, 2, 1), Bs.transpose(0, 2, 1)).transpose(0, 2, 1)      # Bs / Ds
        self.Ahs = As - self.Bhs @ Cs
        self.Bhs[off], self.Ahs[off] = 0.0, 0.0
        self.off = off
        nxs, nym = As.shape[1], len(self.i_ym)
        self.Ks, self.Ps = np.zeros((B, Hp, nym, nxs)), np.zeros((B, Hp, nym, nym))
        P = np.broadcast_to(np.eye(nxs), As.shape).copy()      # As^(i-1)
        for i in range(Hp):
            Ms = Cs @ P @ self.Bhs
            P = P @ As
            self.Ks[:, i] = Cs @ P - Ms @ Cs
            self.Ps[:, i] = Ms
        self.xs, self.ysm = np.zeros((B, nxs)), np.zeros((B, nym))
        self.Yhs = np.zeros((B, Hp * self.ny))

    def full(self, vm):
        out = np.zeros(vm.shape[:-1] + (self.ny,))
        out[..., self.i_ym] = vm
        return out

    @property
    def ys(self):
        return self.full(self.ysm)

    def stoch_output(self, xd, y0m, d0):
        yd = mv(self.C, xd) + (mv(self.Dd, d0) if self.nd else 0.0)
        ysm = np.where(np.isfinite(y0m), y0m - yd[:, self.i_ym], 0.0)
        ysm[self.off] = 0.0
        return ysm

    def correct(self, xd, y0m, d0=None):
        self.ysm = self.stoch_output(xd, y0m, d0)
        if self.tables:
            Ym = np.einsum("btij,bj->bti", self.Ks, self.xs) + np.einsum("btij,bj->bti", self.Ps, self.ysm)
        else:
            z = mv(self.Ahs, self.xs) + mv(self.Bhs, self.ysm)
            Ym = np.empty((len(z), self.Hp, len(self.i_ym)))
            for t in range(self.Hp):
                Ym[:, t] = mv(self.Cs, z)
                z = mv(self.As, z)
        self.Yhs = self.full(Ym).reshape(len(Ym), -1)
        return self.Yhs

    def update(self, xd, u0, d0=None):
        xn = mv(self.A, xd) + mv(self.Bu, u0) + (mv(self.Bd, d0) if self.nd else 0.0) + self.fx
        self.xs = mv(self.Ahs, self.xs) + mv(self.Bhs, self.ysm)
        return xn

    def initstate(self, u0, y0m, d0=None):
        B, nx = self.A.shape[:2]
        rhs = mv(self.Bu, u0) + (mv(self.Bd, d0) if self.nd else 0.0) + self.fx
        xd = np.linalg.solve(np.eye(nx) - self.A, rhs[:, :, None])[:, :, 0]
        self.ysm = self.stoch_output(xd, y0m, d0)
        self.xs = np.linalg.solve(np.eye(self.As.shape[1]) - self.Ahs, mv(self.Bhs, self.ysm)[:, :, None])[:, :, 0]
        return xd


# ---- estimator quantities on randomised heterogeneous batches ---------------------------------------------------------------------
# name: nx, nu, ny, i_ym (None: all), nxs (None: the default stochastic model), Hp, nd
SHAPES = {
    "a": (3, 2, 2, None, None, 5, 0),
    "b_not_a_prefix": (5, 2, 3, [0, 2], 4, 6, 1),
    "c_row_boundary": (16, 1, 16, None, 16, 3, 0),
    "d_wide_by_nx": (17, 1, 2, None, 2, 4, 0),
    "e_wide_by_nxs": (8, 2, 2, None, 20, 4, 0),
    "f_wavefront_boundary": (32, 2, 3, None, 32, 3, 0),
}
B_EST = 67              # not a multiple of the members per wavefront (4), and the wide shapes run 67 wavefronts


def random_stoch(rng, B, nxs, nym):
    """Spectral radius <= 1; member 0 has an integrator (an eigenvalue of exactly 1); Ds = I + a small perturbation."""
    As = synth._stable_A(rng, nxs, B)
    As[0, 0, :], As[0, :, 0] = 0.0, 0.0
    As[0, 0, 0] = 1.0
    Bs = rng.standard_normal((B, nxs, nym)) / np.sqrt(nxs)
    Cs = rng.standard_normal((B, nym, nxs)) / np.sqrt(nxs)
    Ds = np.eye(nym) + 0.3 * rng.standard_normal((B, nym, nym)) / np.sqrt(nym)
    return As, Bs, Cs, Ds


def default_stoch(B, nym):
    eye = np.broadcast_to(np.eye(nym), (B, nym, nym)).copy()
    return eye, eye.copy(), eye.copy(), eye.copy()


def random_batch(name, B=B_EST, seed=5):
    nx, nu, ny, i_ym, nxs, Hp, nd = SHAPES[name]
    rng = np.random.default_rng([seed, nx, ny])
    i_ym = np.arange(ny) if i_ym is None else np.asarray(i_ym)
    nym = len(i_ym)
    m = dict(A=0.9 * synth._stable_A(rng, nx, B), Bu=rng.standard_normal((B, nx, nu)) / np.sqrt(nx),
             C=rng.standard_normal((B, ny, nx)) / np.sqrt(nx), Bd=None, Dd=None)
    if nd:
        m["Bd"], m["Dd"] = rng.standard_normal((B, nx, nd)) / np.sqrt(nx), rng.standard_normal((B, ny, nd))
    ops = dict(uop=rng.standard_normal((B, nu)), yop=5.0 * rng.standard_normal((B, ny)), dop=rng.standard_normal((B, nd)),
               xhop=rng.standard_normal((B, nx)), fhop=rng.standard_normal((B, nx)))
    stoch = None if nxs is None else random_stoch(rng, B, nxs, nym)
    return dict(name=name, m=m, ops=ops, stoch=stoch, i_ym=i_ym, Hp=Hp, nd=nd, B=B, nx=nx, nu=nu, ny=ny, nym=nym, rng=rng)


def controller(c, lib, Hc=2, **kw):
    m = c["m"]
    mpc = mpcqp.BatchLinMPC(m["A"], m["Bu"], m["C"], m["Bd"], m["Dd"], Hp=c["Hp"], Hc=Hc, lib=lib, **c["ops"], **kw)
    mpc.setestimator(internal=dict(stoch_ym=c["stoch"]), i_ym=c["i_ym"])
    return mpc


def reference_of(c, tables=True, off=None):
    m, ops = c["m"], c["ops"]
    stoch = default_stoch(c["B"], c["nym"]) if c["stoch"] is None else c["stoch"]
    return ImRef(m["A"], m["Bu"], m["C"], m["Bd"], m["Dd"], ops["fhop"] - ops["xhop"], stoch, c["i_ym"], c["Hp"], tables=tables, off=off)


def bar(delta, ref):
    return max(32.0 * delta, 1e-13 * float(np.abs(ref).max()))


def estimator_periods(name, lib, periods=3):
    """Three periods of preparestate / updatestate (no controller step: u is drawn) on the device and in both NumPy
    formulations.  Returns {quantity: (device error, δ, bar)} over all periods."""
    c = random_batch(name)
    B, rng = c["B"], c["rng"]
    mpc = controller(c, lib)
    refs = [reference_of(c, tables=True), reference_of(c, tables=False)]
    ops = c["ops"]
    xd = [np.zeros((B, c["nx"])) for _ in refs]
    out = {k: [0.0, 0.0, 0.0] for k in QUANTITIES}

    def note(k, dev, a, b):
        out[k][0] = max(out[k][0], float(np.abs(dev - a).max()))
        out[k][1] = max(out[k][1], float(np.abs(a - b).max()))
        out[k][2] = max(out[k][2], float(np.abs(a).max()))
    for _ in range(periods):
        ym = ops["yop"][:, c["i_ym"]] + rng.standard_normal((B, c["nym"]))
        u = ops["uop"] + rng.standard_normal((B, c["nu"]))
        d = ops["dop"] + rng.standard_normal((B, c["nd"])) if c["nd"] else None
        d0 = None if d is None else d - ops["dop"]
        mpc.preparestate(ym, d)
        for r, x in zip(refs, xd):
            r.correct(x, ym - ops["yop"][:, c["i_ym"]], d0)
        xs, ys, Yhs = mpc.hd.im_state()
        note("ys", ys, refs[0].ys, refs[1].ys)
        note("xs", xs, refs[0].xs, refs[1].xs)
        note("Yhs", Yhs, refs[0].Yhs, refs[1].Yhs)
        mpc.updatestate(u, ym, d)
        xd = [r.update(x, u - ops["uop"], d0) for r, x in zip(refs, xd)]
        note("xd", mpc.xhat0, xd[0], xd[1])
    xs = mpc.hd.get(api.GET_IM_XS)
    note("xs", xs, refs[0].xs, refs[1].xs)
    assert np.abs(refs[0].xs).max() > 1e-3          # (three periods: x̂s is not zero)
    return {k: (e, dl, bar(dl, mag)) for k, (e, dl, mag) in out.items()}


# ---- known answers of the reference's tests ------------------------------------------------------------------------------------

def zoh_first_order(gains, taus, Ts):
    """diag_i gain_i / (tau_i s + 1) sampled with a zero-order hold: A, Bu, C (C = I)."""
    a = np.exp(-Ts / np.asarray(taus, float))
    return np.diag(a), np.diag((1.0 - a) * np.asarray(gains, float)), np.eye(len(a))


def setup_model():
    """The plant of the reference's estimator tests (test/0_test_module.jl, inputs 1 and 2), Ts = 400 s, in a diagonal
    realisation: y1 = 1.90 / (1800 s + 1) (u1 + u2), y2 = 0.74 / (800 s + 1) (u2 - u1)."""
    a = np.exp(-400.0 / np.array([1800.0, 800.0]))
    return np.diag(a), (1.0 - a)[:, None] * np.array([[1.90, 1.90], [-0.74, 0.74]]), np.eye(2)


def neighbour(rng, nx, nu, ny):
    """A member with another model, to stand next to a known-answer member."""
    return 0.9 * synth._stable_A(rng, nx, 1)[0], rng.standard_normal((nx, nu)), rng.standard_normal((ny, nx))


def batch_of(members, **kw):
    """BatchLinMPC arguments of a list of (A, Bu, C) members."""
    return tuple(np.stack([m[k] for m in members]) for k in range(3))


def tustin_stoch():
    """diag((2.5 s + 1) / (1.2 s² + s), (1.5 s + 1) / (1.3 s² + s)) discretised with Tustin at Ts = 1 (nxs = 4)."""
    from scipy import signal
    from scipy.linalg import block_diag
    parts = []
    for num, den in (([2.5, 1.0], [1.2, 1.0, 0.0]), ([1.5, 1.0], [1.3, 1.0, 0.0])):
        A, Bm, Cm, D = signal.tf2ss(num, den)
        parts.append(signal.cont2discrete((A, Bm, Cm, D), 1.0, method="bilinear")[:4])
    return tuple(block_diag(*(p[k] for p in parts)) for k in range(4))


def quiet(f, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return f(*a, **kw)


# ---- controller parity --------------------------------------------------------------------------------------------------------
# name: nx, nu, ny, Hp, Hc, constraints, kernel kinds the shape may run on
PARITY = {
    "c2_dims_c3_rows": (6, 2, 2, 20, 5, dict(umin=[-1.0, -1.0], umax=[1.0, 1.0], ymax=[0.4, 0.4])),
    "four_per_wavefront": (3, 2, 2, 6, 3, dict(umin=[-1.0, -1.0], umax=[1.0, 1.0], ymax=[0.3, 0.3])),
    "manifest_3_2_7": (7, 3, 2, 12, 4, dict(umin=[-1.0] * 3, umax=[1.0] * 3, Δumin=[-0.5] * 3, Δumax=[0.5] * 3, ymin=[-2.0, -2.0],
                                            ymax=[0.4, 0.4])),
}


def parity_batch(name, B, seed=9):
    nx, nu, ny, Hp, Hc, con = PARITY[name]
    rng = np.random.default_rng([seed, nx, nu])
    m = dict(A=0.9 * synth._stable_A(rng, nx, B), Bu=rng.standard_normal((B, nx, nu)) / np.sqrt(nx),
             C=rng.standard_normal((B, ny, nx)) / np.sqrt(nx), Bd=None, Dd=None)
    ops = dict(uop=np.zeros((B, nu)), yop=np.zeros((B, ny)), dop=np.zeros((B, 0)), xhop=0.1 * rng.standard_normal((B, nx)),
               fhop=0.1 * rng.standard_normal((B, nx)))
    return dict(name=name, m=m, ops=ops, stoch=random_stoch(rng, B, 3, ny), i_ym=np.arange(ny), Hp=Hp, Hc=Hc, con=con, nd=0, B=B,
                nx=nx, nu=nu, ny=ny, nym=ny, rng=rng)


def oracle_of(c, i, extra_nd=0):
    m, ops = c["m"], c["ops"]
    orc = cd.LinMPCOracle(m["A"][i], m["Bu"][i], m["C"][i], Hp=c["Hp"], Hc=c["Hc"], xhop=ops["xhop"][i], fhop=ops["fhop"][i])
    orc.setconstraint(**{k.replace("Δ", "d"): v for k, v in c["con"].items()})
    return orc


def controller_parity(name, lib, B=6, periods=2, info=True):
    """`periods` periods of preparestate / moveinput / updatestate on the device against the NumPy estimator driving one
    LinMPCOracle per member with orc.B = B_model + Ŷs.  Returns the worst relative ΔU / ϵ error, the worst F and Ŷ errors
    (relative to max(1, max|.|)), the share of members with an active ymax row and Ŷs != 0 on the oracle, the kernel kind,
    and the same QPs solved by a plain handle that gets Ŷs as the preview of ny extra measured disturbances.  `info=False`
    asks for neither F (MPCQP_FLAG_KEEP_QP) nor Ŷ: either moves a step off the four-per-wavefront kernel."""
    c = parity_batch(name, B)
    rng, ops, ny, nu, Hp = c["rng"], c["ops"], c["ny"], c["nu"], c["Hp"]
    mpc = controller(c, lib, Hc=c["Hc"], keep_qp=info)
    mpc.setconstraint(**c["con"])
    # the cross-check handle: the same model with B̂d = 0, D̂d = I on ny extra channels
    m = c["m"]
    twin = mpcqp.BatchLinMPC(m["A"], m["Bu"], m["C"], np.zeros((B, c["nx"], ny)), np.broadcast_to(np.eye(ny), (B, ny, ny)).copy(),
                             Hp=Hp, Hc=c["Hc"], lib=lib, **{**ops, "dop": np.zeros((B, ny))})
    twin.setconstraint(**c["con"])
    ref = reference_of(c)
    orcs = [oracle_of(c, i) for i in range(B)]
    Bmodel = [o.B.copy() for o in orcs]
    xd = np.zeros((B, c["nx"]))
    worst = dict(Z=0.0, u=0.0, F=0.0, Yhat=0.0, twin=0.0)
    active = np.zeros(B, bool)
    ry = 0.6 + 0.2 * rng.standard_normal((B, ny))
    nDU = mpc.nDU
    for _ in range(periods):
        ym = mv(m["C"], xd) + 0.3 * rng.standard_normal((B, ny)) + 0.15
        quiet(mpc.preparestate, ym)
        Yhs = ref.correct(xd, ym)
        Zprev = mpc.Z.copy()
        u = quiet(mpc.moveinput, None, ry, want_info=info)
        Yhat = mpc.getinfo()["Ŷ"] if info else None
        F = mpc.hd.get(api.GET_FVEC) if info else None
        # the plain handle: d0 = ŷs is not what the InternalModel adds at k, but row k is not part of the QP; the preview is Ŷs
        twin.Z, twin.lastu0 = Zprev, mpc._lastu0_prev.copy()
        ut = quiet(twin.moveinput, mpc.xhat0, ry, np.zeros((B, ny)), Dhat=Yhs)
        worst["twin"] = max(worst["twin"], float(rel(mpc.Z, twin.Z, nDU).max()), float(np.abs(u - ut).max()))
        for i, o in enumerate(orcs):
            o.B = Bmodel[i] + Yhs[i]
            o.initpred(xd[i], mpc._lastu0_prev[i], ry[i])
            o.linconstraint()
            z, st, _ = qp.solve_qp(*o.qp_data(), o.warmstart(), return_info=True)
            assert st == 0
            o.Zt = z
            Y0 = o.Et @ z + o.F
            hi = np.isfinite(o.Y0max) & (np.abs(Y0 - (o.Y0max + o.C_ymax * z[-1])) <= 1e-7)
            active[i] |= bool(hi.any()) and bool(np.abs(Yhs[i]).max() > 1e-3)
            worst["Z"] = max(worst["Z"], float(rel(mpc.Z[i:i + 1], z[None], nDU).max()),
                             abs(mpc.Z[i, -1] - z[-1]) / max(1.0, abs(z[-1])))
            worst["u"] = max(worst["u"], float(np.abs(u[i] - (z[:nu] + mpc._lastu0_prev[i])).max()) / max(1.0, np.abs(z[:nu]).max()))
            if info:
                worst["F"] = max(worst["F"], float(np.abs(F[i] - o.F).max()) / max(1.0, np.abs(o.F).max()))
                worst["Yhat"] = max(worst["Yhat"], float(np.abs(Yhat[i] - Y0).max()) / max(1.0, np.abs(Y0).max()))
        quiet(mpc.updatestate, u, ym)
        xd = ref.update(xd, u)
        assert np.abs(mpc.xhat0 - xd).max() <= 1e-12 * max(1.0, np.abs(xd).max())
    return worst, float(active.mean()), mpc.hd.kernel_kind()


def rel(Zg, Zo, nDU):
    return np.max(np.abs(Zg[:, :nDU] - Zo[:, :nDU]), axis=1) / np.maximum(1.0, np.max(np.abs(Zo[:, :nDU]), axis=1))


# ---- exactness ---------------------------------------------------------------------------------------------------------------

def exact_batch(B=7, seed=3, Hp=20, Hc=5, zero_uy=False):
    """A small heterogeneous batch whose model entries and states are multiples of 1/8, so that Ĉ x̂0 is exact in every
    summation order and with or without fused multiply-adds; f̂op != x̂op, so the model's B is not zero.  The dimensions
    and the constraint pattern are a line of spec_manifest.txt (2 2 6 20 5 1 8c): no compilation at first use."""
    rng = np.random.default_rng(seed)
    nx, nu, ny = 6, 2, 2
    q = lambda *s: rng.integers(-4, 5, s) / 8.0
    A = np.zeros((B, nx, nx))
    A[:, range(nx), range(nx)] = rng.integers(1, 7, (B, nx)) / 8.0
    A[:, 0, 1] = q(B)
    m = dict(A=A, Bu=q(B, nx, nu), C=q(B, ny, nx), Bd=None, Dd=None)
    ops = dict(uop=q(B, nu), yop=q(B, ny), dop=np.zeros((B, 0)), xhop=q(B, nx), fhop=q(B, nx) + 0.125)
    if zero_uy:         # (records in engineering units then are the device's values: (v + op) - op is not v bit for bit)
        ops["uop"], ops["yop"] = np.zeros((B, nu)), np.zeros((B, ny))
    return dict(name="exact", m=m, ops=ops, stoch=random_stoch(rng, B, 3, ny), i_ym=np.arange(ny), Hp=Hp, Hc=Hc, nd=0, B=B, nx=nx,
                nu=nu, ny=ny, nym=ny, rng=rng, con=dict(umin=[-0.5, -0.5], umax=[0.5, 0.5], ymax=[0.3, 0.3]))


def plain_controller(c, lib, **kw):
    m = c["m"]
    mpc = mpcqp.BatchLinMPC(m["A"], m["Bu"], m["C"], m["Bd"], m["Dd"], Hp=c["Hp"], Hc=c["Hc"], lib=lib, **c["ops"], **kw)
    mpc.setconstraint(**c["con"])
    return mpc


def zero_mismatch(lib):
    """ym = the model's own output: ŷs = x̂s = Ŷs = 0 exactly, and the step is bit for bit the step of the same handle
    without an estimator at the same x̂0."""
    c = exact_batch()
    B, ops = c["B"], c["ops"]
    ry = ops["yop"] + 0.25
    im = plain_controller(c, lib)
    im.setestimator(internal=dict(stoch_ym=c["stoch"]))
    plain = plain_controller(c, lib)
    assert np.abs(plain.hd.get(api.GET_BVEC)).max() > 0.0
    out = []
    for _ in range(2):
        im.xhat0 = c["rng"].integers(-8, 9, (B, c["nx"])) / 8.0       # (setstate: an x̂0 whose Ĉ x̂0 is exact)
        ym = mv(c["m"]["C"], im.xhat0) + ops["yop"]
        im.preparestate(ym)
        xs, ys, Yhs = im.hd.im_state()
        assert not xs.any() and not ys.any() and not Yhs.any()
        xk = im.xhat0.copy()
        ua, ub = quiet(im.moveinput, None, ry), quiet(plain.moveinput, xk, ry)
        out.append((same(im.Z, plain.Z) and same(ua, ub) and same(im.status, plain.status), int(np.sum(im.status == 0))))
        im.updatestate(ua, ym)
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def methods_run(c, lib, periods, y_all, ry, members=None, stoch=None, reps=1):
    """preparestate / moveinput / updatestate for `periods` periods on measurements y_all (periods,B,nym); returns the records."""
    sel = slice(None) if members is None else members
    sub = dict(c, m={k: (None if v is None else v[sel]) for k, v in c["m"].items()}, ops={k: v[sel] for k, v in c["ops"].items()})
    st = c["stoch"] if stoch is None else stoch
    mpc = plain_controller(sub, lib)
    quiet(mpc.setestimator, internal=dict(stoch_ym=tuple(a[sel] for a in st)))
    rec = []
    for k in range(periods):
        quiet(mpc.preparestate, y_all[k][sel])
        xs, ys, Yhs = mpc.hd.im_state()
        u = quiet(mpc.moveinput, None, ry[sel])
        mpc.hd.im_update(mpc.xhat0, mpc.lastu0)         # (updatestate(u) would take u0 = (u0 + uop) - uop, which is not u0 bit for bit)
        rec.append(dict(xs=xs, ys=ys, Yhs=Yhs, u=u, Z=mpc.Z.copy(), status=mpc.status.copy(), xd=mpc.xhat0.copy()))
    return rec, mpc


def isolation(lib):
    """A member with a NaN measurement, a member whose Ds is singular (status 2) and -- in initstate -- a member whose
    I - Âs is singular (status 1): every other member bit for bit what it is in a batch without them."""
    c = exact_batch(B=9, seed=4)
    B, rng, ops = c["B"], c["rng"], c["ops"]
    periods = 3
    y_all = ops["yop"] + 0.3 * rng.standard_normal((periods, B, c["ny"]))
    ry = ops["yop"] + 0.25
    bad = np.array(c["stoch"][3])
    bad[5] = [[1.0, 2.0], [2.0, 4.0]]            # singular: the elimination meets an exact zero pivot
    y_nan = y_all.copy()
    y_nan[1, 2, 0] = np.nan
    keep = np.array([0, 1, 3, 4, 6, 7, 8])
    full, mpc = methods_run(c, lib, periods, y_nan, ry, stoch=c["stoch"][:3] + (bad,))
    part, _ = methods_run(c, lib, periods, y_all, ry, members=keep)
    st = mpc.hd.im_status()
    ok = all(same(f[k][keep], p[k]) for f, p in zip(full, part) for k in f)
    nan_ys = full[1]["ys"][2]
    off_zero = all(not f["ys"][5].any() and not f["Yhs"][5].any() and not f["xs"][5].any() for f in full)
    # initstate with a member whose stochastic model has Âs = I (Bs = 0, As = I): I - Âs is singular
    As, Bs, Cs, Ds = (np.array(a) for a in c["stoch"])
    As[4], Bs[4] = np.eye(As.shape[1]), 0.0
    def init(members):
        sub = dict(c, m={k: (None if v is None else v[members]) for k, v in c["m"].items()}, ops={k: v[members] for k, v in c["ops"].items()})
        m2 = plain_controller(sub, lib)
        m2.setestimator(internal=dict(stoch_ym=(As[members], Bs[members], Cs[members], Ds[members])), xhat0=np.full((len(members), c["nx"]), 0.5))
        x = quiet(m2.initstate, (ops["uop"] + 0.25)[members], y_all[0][members])
        return x, m2.hd.get(api.GET_IM_XS), m2.init_status.copy(), m2
    allm, rest = np.arange(B), np.array([0, 1, 2, 3, 5, 6, 7, 8])
    xa, xsa, sta, m_all = init(allm)
    xr, xsr, str_, _ = init(rest)
    init_ok = same(xa[rest], xr) and same(xsa[rest], xsr) and not str_.any()
    kept = same(m_all.xhat0[4], np.full(c["nx"], 0.5)) and not xsa[4].any()
    return dict(neighbours=ok, status=st, nan_ys=nan_ys, off_zero=off_zero, init_neighbours=init_ok, init_status=sta, init_kept=kept)


def stale_model(lib):
    """setmodel keeps x̂s, ŷs and Ŷs: the step after it runs on the new B with the old Ŷs (F = B_new + K x̂0 + V lastu0 + Ŷs)."""
    c = exact_batch(B=5, seed=6)
    B, ops, rng = c["B"], c["ops"], c["rng"]
    mpc = plain_controller(c, lib, keep_qp=True)
    mpc.setestimator(internal=dict(stoch_ym=c["stoch"]))
    ym = ops["yop"] + 0.3 * rng.standard_normal((B, c["ny"]))
    for _ in range(2):
        mpc.preparestate(ym)
        u = quiet(mpc.moveinput, None, ops["yop"] + 0.25)
        mpc.updatestate(u, ym)
    mpc.preparestate(ym)
    before = mpc.hd.im_state()
    A2 = c["m"]["A"] * 0.5
    mpc.setmodel(A2, c["m"]["Bu"], c["m"]["C"])
    after = mpc.hd.im_state()
    lu = mpc.lastu0.copy()
    quiet(mpc.moveinput, None, ops["yop"] + 0.25)
    F = mpc.hd.get(api.GET_FVEC)
    worst = 0.0
    for i in range(B):
        o = cd.LinMPCOracle(A2[i], c["m"]["Bu"][i], c["m"]["C"][i], Hp=c["Hp"], Hc=c["Hc"], xhop=ops["xhop"][i], fhop=ops["fhop"][i])
        o.B = o.B + before[2][i]
        o.initpred(mpc.xhat0[i], lu[i], 0.25 * np.ones(c["ny"]))
        worst = max(worst, float(np.abs(F[i] - o.F).max()) / max(1.0, np.abs(o.F).max()))
    return all(same(a, b) for a, b in zip(before, after)), worst, float(np.abs(before[2]).max())


# ---- the loop and sim against the methods -------------------------------------------------------------------------------------

def loop_against_methods(lib, torch_device, periods=6):
    """mpcqp_loop_device on device arrays for `periods` periods against preparestate / moveinput / updatestate: u0, Z̃, status,
    x̂0 and the estimator's x̂s, ŷs, Ŷs after every period, bit for bit.  `torch_device`: "cuda" on the GPU; None on the
    emulator, where "device" pointers are host pointers."""
    c = exact_batch(B=6, seed=8)
    B, ops, rng = c["B"], c["ops"], c["rng"]
    y_all = ops["yop"] + 0.3 * rng.standard_normal((periods, B, c["ny"]))
    ry = ops["yop"] + 0.25
    rec, _ = methods_run(c, lib, periods, y_all, ry)
    mpc = plain_controller(c, lib)
    quiet(mpc.setestimator, internal=dict(stoch_ym=c["stoch"]))
    mpc._prepare_kernel()
    mpc.hd.set_flags(mpc.hd.flags | api.FLAG_RY_CONSTANT)
    if torch_device is None:
        mk = lambda a: np.ascontiguousarray(a)
        ptr, host = (lambda a: a.ctypes.data), (lambda a: a.copy())
        sync = lambda: None
    else:
        import torch
        mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch_device)
        ptr, host = (lambda a: a.data_ptr()), (lambda a: a.cpu().numpy())
        sync = torch.cuda.synchronize
    xh, lu, Z = mk(np.zeros((B, c["nx"]))), mk(np.zeros((B, c["nu"]))), mk(np.zeros((B, mpc.nZ)))
    u0, st, ryd = mk(np.zeros((B, c["nu"]))), mk(np.zeros(B, np.int32)), mk(ry - ops["yop"])
    ok = []
    for k in range(periods):
        y = mk(y_all[k] - ops["yop"])
        sync()
        mpc.hd.loop_device(ptr(xh), ptr(y), ptr(lu), ptr(ryd), ptr(Z), ptr(u0), ptr(st))
        sync()
        xs, ys, Yhs = mpc.hd.im_state()
        r = rec[k]
        ok.append(same(host(u0) + ops["uop"], r["u"]) and same(host(Z), r["Z"]) and same(host(st), r["status"]) and same(host(xh), r["xd"])
                  and same(ys, r["ys"]) and same(Yhs, r["Yhs"]))
        if k + 1 < periods:
            ok[-1] = ok[-1] and same(xs, rec[k + 1]["xs"])
        if torch_device is None:
            lu[:] = u0
        else:
            lu.copy_(u0)
    return ok


def sim_against_methods(lib, N=8):
    """`sim` (the plant on the device) against the same loop one period at a time through the correct / step / update methods,
    fed the measurements the run recorded (uop = yop = 0: the records are the device's values): every record of the
    estimator and the controller bit for bit, but Ŷ, which the methods compute on the host (evaloutput): 1e-13 max(1, max|Ŷ|)."""
    c = exact_batch(B=5, seed=10, zero_uy=True)
    B, ops, m = c["B"], c["ops"], c["m"]
    ry = ops["yop"] + 0.25
    ystep = np.full((B, c["ny"]), 0.125)
    mpc = plain_controller(c, lib)
    quiet(mpc.setestimator, internal=dict(stoch_ym=c["stoch"]))
    res = quiet(mpc.sim, N, ry, plant=dict(A=m["A"], Bu=1.25 * m["Bu"], C=m["C"]), y_step=ystep, x_0=np.zeros((B, c["nx"])), lastu=ops["uop"])
    twin = plain_controller(c, lib)
    quiet(twin.setestimator, internal=dict(stoch_ym=c["stoch"]))
    twin.lastu0 = np.zeros((B, c["nu"]))
    ok = []
    for k in range(N):
        ym = res.Y_data[:, :, k]
        quiet(twin.preparestate, ym)
        yhat = twin.evaloutput()
        xk = twin.xhat0.copy()
        u = quiet(twin.moveinput, None, ry)
        twin.hd.im_update(twin.xhat0, twin.lastu0)      # (see methods_run)
        ok.append(dict(U=same(res.U_data[:, :, k], u), Xhat=same(res.X̂_data[:, :, k], xk + ops["xhop"]), status=same(res.status[:, k], twin.status),
                       Yhat=float(np.abs(res.Ŷ_data[:, :, k] - yhat).max()) / max(1.0, float(np.abs(yhat).max()))))
    assert np.abs(res.Y_data[:, :, -1] - res.Y_data[:, :, 0]).max() > 1e-3          # (the loop moved)
    final = same(mpc.xhat0, twin.xhat0) and same(mpc.Z, twin.Z) and all(same(a, b) for a, b in zip(mpc.hd.im_state(), twin.hd.im_state()))
    return ok, final, res.path


# ---- known answers of the reference's tests, through the whole controller ----------------------------------------------------

def known_answers_default(lib):
    """test/2_test_state_estim.jl:478-490, 514-520 (two members each, next to a neighbour with another model)."""
    rng = np.random.default_rng(1)
    kn = setup_model()
    A, Bu, C = batch_of([kn, neighbour(rng, 2, 2, 2), kn])
    uop, yop = np.array([10.0, 50.0]), np.array([50.0, 30.0])
    mpc = mpcqp.BatchLinMPC(A, Bu, C, Hp=5, Hc=2, uop=uop, yop=yop, lib=lib)
    mpc.setinternalmodel()
    out = {}
    y = yop + 1.0
    for _ in range(2):
        mpc.preparestate(y)
        x = mpc.updatestate(uop, y)
    out["x0_after_two"] = x[[0, 2]]
    out["xs_after_two"] = mpc.hd.get(api.GET_IM_XS)[[0, 2]]
    mpc.preparestate(y)
    out["evaloutput"] = mpc.evaloutput()[[0, 2]]
    out["init_x"] = mpc.initstate(uop, yop)[[0, 2]]
    out["init_xs"] = mpc.hd.get(api.GET_IM_XS)[[0, 2]]
    # :514-520: ŷs preset to 7 by a period with ym = yop + 7, then a NaN measurement
    mpc.preparestate(yop + 7.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        mpc.preparestate(np.array([57.0, np.nan]))
    out["nan_ys"] = mpc.hd.get(api.GET_IM_YS)[[0, 2]]
    out["nan_warnings"] = [str(x.message) for x in w]
    return out


def known_answers_tustin(lib):
    """:493-506: diag(3/(5s+1), 2/(10s+1)), Ts = 1, a second-order stochastic model per output with an integrator."""
    rng = np.random.default_rng(2)
    kn = zoh_first_order([3.0, 2.0], [5.0, 10.0], 1.0)
    A, Bu, C = batch_of([kn, kn, neighbour(rng, 2, 2, 2)])
    mpc = mpcqp.BatchLinMPC(A, Bu, C, Hp=5, Hc=2, lib=lib)
    st = tustin_stoch()
    mpc.setinternalmodel(stoch_ym=st)
    ref = ImRef(A, Bu, C, None, None, np.zeros((3, 2)), tuple(np.broadcast_to(a, (3,) + a.shape) for a in st), np.arange(2), 5)
    out = {}
    u, ym = np.array([1.0, 2.0]), np.array([3.1, 4.5])
    x = mpc.initstate(u, ym)
    out["fixed_point_xd"] = np.abs(x - (mv(A, x) + mv(Bu, np.broadcast_to(u, (3, 2)))))[:2]
    mpc.preparestate(ym)
    out["yhat"] = mpc.evaloutput()[:2]
    xs, ys, _ = mpc.hd.im_state()
    out["fixed_point_xs"] = np.abs(xs - (mv(ref.Ahs, xs) + mv(ref.Bhs, ys)))[:2]
    out["xs_mag"] = float(np.abs(xs[:2]).max())
    mpc.updatestate(u, np.array([-13.0, -14.0]))
    mpc.preparestate(np.array([13.0, 14.0]))
    out["yhat2"] = mpc.evaloutput()[:2]
    return out


def known_answer_setmodel(lib):
    """:525-545: setmodel with changed operating points; x̂0 = x̂ - x̂op follows."""
    one = lambda v: np.full((2, 1, 1), v)
    mpc = mpcqp.BatchLinMPC(one(0.5), one(0.3), one(1.0), Hp=4, Hc=2, uop=[2.0], yop=[50.0], xhop=[3.0], fhop=[3.0], lib=lib)
    mpc.setinternalmodel()
    out = {}
    mpc.preparestate([50.0])
    out["y1"] = mpc.evaloutput()
    mpc.preparestate([50.0])
    out["x1"] = mpc.updatestate([2.0], [50.0])
    mpc.uop[:], mpc.yop[:] = 3.0, 55.0          # (setop! of the new model; BatchLinMPC.setmodel takes x̂op and f̂op)
    mpc.Uop, mpc.Yop = np.tile(mpc.uop, mpc.Hp), np.tile(mpc.yop, mpc.Hp)
    mpc.setmodel(one(0.2), one(0.3), one(1.0))
    mpc.preparestate([55.0])
    out["y2"] = mpc.evaloutput()
    mpc.preparestate([55.0])
    out["x2"] = mpc.updatestate([3.0], [55.0])
    mpc.setmodel(one(0.2), one(0.3), one(1.0), xhop=[8.0], fhop=[8.0])
    out["x0"] = mpc.xhat0.copy()
    return out


def disturbance_rejection(lib, N=25):
    """test/3_test_predictive_control.jl:159-178 through `sim`: 5/(2s+1), Ts = 3, yop = 10, r = 15, an output disturbance of
    -5; two members of it next to a neighbour with another gain.  Returns u and ym of the last period and the same loop by
    the NumPy estimator and the oracle controller."""
    a = np.exp(-1.5)
    gains = np.array([5.0, 5.0, 3.0])
    A, Bu, C = np.full((3, 1, 1), a), (gains * (1.0 - a)).reshape(3, 1, 1), np.ones((3, 1, 1))
    mpc = mpcqp.BatchLinMPC(A, Bu, C, Hp=10, Hc=2, yop=[10.0], lib=lib)
    mpc.setinternalmodel()
    res = quiet(mpc.sim, N, [15.0], plant=dict(A=A, Bu=Bu, C=C), y_step=[-5.0], x_0=np.zeros((3, 1)), lastu=[0.0])
    ref = ImRef(A, Bu, C, None, None, np.zeros((3, 1)), default_stoch(3, 1), [0], 10)
    orcs = [cd.LinMPCOracle(A[i], Bu[i], C[i], Hp=10, Hc=2, yop=[10.0]) for i in range(3)]
    B0 = [o.B.copy() for o in orcs]
    x, xd, U, Y = np.zeros((3, 1)), np.zeros((3, 1)), np.zeros((3, N)), np.zeros((3, N))
    for k in range(N):
        ym = mv(C, x) + 10.0 - 5.0
        Yhs = ref.correct(xd, ym - 10.0)
        u = np.empty((3, 1))
        for i, o in enumerate(orcs):
            o.B = B0[i] + Yhs[i]
            u[i] = o.moveinput(xd[i], [15.0])
        xd = ref.update(xd, u)
        x = mv(A, x) + mv(Bu, u)
        U[:, k], Y[:, k] = u[:, 0], ym[:, 0]
    return res.U_data[:, 0, :], res.Y_data[:, 0, :], U, Y


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def refusals(lib):
    """Every refusal of include/mpcqp.h: {name: (returned code or exception name, expected)}; and the estimator state before and
    after the refused calls."""
    c = exact_batch(B=4, seed=12)
    mpc = plain_controller(c, lib)
    mpc.setestimator(internal=dict(stoch_ym=c["stoch"]))
    ym = c["ops"]["yop"] + 0.25
    mpc.preparestate(ym)
    u = quiet(mpc.moveinput, None, ym)
    mpc.updatestate(u, ym)
    mpc.preparestate(ym)
    before = mpc.hd.im_state()
    L, h = mpc.hd.lib, mpc.hd.h
    iy = np.arange(2, dtype=np.int32)
    p = lambda a: a.ctypes.data
    got = {}
    bad = lambda iyv, nym, nxs=0: L.mpcqp_im_set(h, nxs, None, None, None, None, p(np.asarray(iyv, np.int32)), nym)
    got["nym_gt_ny"] = (bad([0, 1, 1], 3), -2)
    got["repeated_i_ym"] = (bad([1, 1], 2), -3)
    got["i_ym_out_of_range"] = (bad([0, 2], 2), -3)
    As = np.zeros((4, 1))
    got["nxs_lt_1"] = (L.mpcqp_im_set(h, 0, p(As), p(As), p(As), p(As), p(iy), 2), -3)
    got["kf_set_direct_0"] = (L.mpcqp_kf_set_direct(h, 0), -3)
    got["explicit_prepare"] = (L.mpcqp_explicit_prepare(h, 0), -4)
    z = np.zeros(64)
    got["explicit_step"] = (L.mpcqp_explicit_step(h, p(z), p(z), p(z), None, None, None, p(z), p(z), p(z), None), -4)
    got["explicit_law"] = (L.mpcqp_explicit_law(h, p(z), p(z), p(z), None, p(z), p(z), p(z)), -4)
    st = np.zeros(4, np.int32)
    got["explicit_status"] = (L.mpcqp_explicit_status(h, p(st)), -4)
    Wy = np.ones((4, 1, 2))
    got["custom_constraints"] = (L.mpcqp_set_custom_constraints(h, 1, p(Wy), p(Wy), None, None, None), -4)
    after = mpc.hd.im_state()
    # a handle on the stage kernel, one with custom constraints, one prepared as ExplicitMPC, a shard of a multi handle
    ms = plain_controller(c, lib, transcription="MultipleShooting")
    ms._prepare_kernel()
    got["multiple_shooting"] = (L.mpcqp_im_set(ms.hd.h, 0, None, None, None, None, p(iy), 2), -4)
    cw = plain_controller(c, lib, Wy=np.ones((1, 2)))
    got["nw_gt_0"] = (L.mpcqp_im_set(cw.hd.h, 0, None, None, None, None, p(iy), 2), -4)
    m = c["m"]
    ex = mpcqp.BatchExplicitMPC(m["A"], m["Bu"], m["C"], Hp=c["Hp"], Hc=c["Hc"], lib=lib)
    got["explicit_handle"] = (L.mpcqp_im_set(ex.hd.h, 0, None, None, None, None, p(iy), 2), -4)
    # switching the transcription after the estimator was set: the step refuses, the estimator state stays
    mpc.hd.set_transcription(api.MULTIPLE_SHOOTING)
    try:
        quiet(mpc.hd.step, mpc.xhat0, mpc.lastu0, ym - c["ops"]["yop"], mpc.Z.copy())
        got["step_on_stage_kernel"] = (0, -4)
    except mpcqp.MpcqpError as e:
        got["step_on_stage_kernel"] = (int(str(e).split()[2].rstrip(":")), -4)
    mpc.hd.set_transcription(api.SINGLE_SHOOTING)
    after2 = mpc.hd.im_state()
    unchanged = all(same(a, b) for a, b in zip(before, after)) and all(same(a, b) for a, b in zip(before, after2))
    return got, unchanged


def multi_refusal(lib, devices=(0, 0)):
    c = exact_batch(B=4, seed=12)
    mh = api.MultiHandle(4, c["nx"], c["nu"], c["ny"], 0, c["Hp"], c["Hc"], list(devices), lib=lib)
    iy = np.arange(2, dtype=np.int32)
    hg = mh.lib.mpcqp_multi_handle(mh.h, 0)
    rc = mh.lib.mpcqp_im_set(hg, 0, None, None, None, None, iy.ctypes.data, 2)
    mh.close()
    return rc


def python_validation(lib):
    """The reference's constructor checks, on the host at set-up: ValueError."""
    c = exact_batch(B=3, seed=13)
    As, Bs, Cs, Ds = c["stoch"]
    out = {}
    def raises(f):
        try:
            f()
        except ValueError as e:
            return str(e)
        return None
    mpc = plain_controller(c, lib)
    out["Ds_zero"] = raises(lambda: mpc.setinternalmodel(stoch_ym=(As, Bs, Cs, np.zeros_like(Ds))))
    out["Cs_rows"] = raises(lambda: mpc.setinternalmodel(stoch_ym=(As, Bs[:, :, :1], Cs[:, :1], Ds[:, :1, :1])))
    m = dict(c["m"])
    A = m["A"].copy()
    A[1, 0, 0] = 1.0
    uns = mpcqp.BatchLinMPC(A, m["Bu"], m["C"], Hp=c["Hp"], Hc=c["Hc"], lib=lib)
    out["integrating"] = raises(lambda: uns.setinternalmodel())
    out["direct_false"] = raises(lambda: mpc.setestimator(internal=dict(), direct=False))
    return out


# ---- what the twins assert -----------------------------------------------------------------------------------------------------

def check_estimator(name, res):
    for k, (e, delta, b) in res.items():
        print(f"{name:22s} {k:4s} error {e:.2e}  delta {delta:.2e}  bar {b:.2e}")
    for k, (e, delta, b) in res.items():
        assert e <= b, (name, k, e, delta, b)


def near(a, b, tol):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) <= tol


EBAR = 1e-12            # known answers: 1e-13 max|quantity| (the floor of `bar`) at magnitudes up to 57, rounded up


def check_known_answers_default(o):
    assert near(o["x0_after_two"], 0.0, EBAR) and near(o["xs_after_two"], 1.0, EBAR), o
    assert near(o["evaloutput"], [51.0, 31.0], 1e-13 * 51) and near(o["init_x"], [0.0, 0.0], EBAR) and near(o["init_xs"], 0.0, EBAR), o
    assert near(o["nan_ys"], [7.0, 0.0], EBAR), o
    assert len(o["nan_warnings"]) == 1 and "NaN values in the internal model measurements ym: assigning them ŷs=0" in o["nan_warnings"][0], o


def check_known_answers_tustin(o):
    assert o["xs_mag"] > 1e-2, o
    assert near(o["fixed_point_xd"], 0.0, 1e-13 * 10) and near(o["fixed_point_xs"], 0.0, 1e-13 * max(1.0, o["xs_mag"]) * 10), o
    assert near(o["yhat"], [3.1, 4.5], 1e-13 * 45) and near(o["yhat2"], [13.0, 14.0], 1e-13 * 140), o


def check_known_answer_setmodel(o):
    assert near(o["y1"], 50.0, 1e-13 * 50) and near(o["x1"], 3.0, EBAR) and near(o["y2"], 55.0, 1e-13 * 55) and near(o["x2"], 3.0, EBAR), o
    assert near(o["x0"], 3.0 - 8.0, EBAR), o


def check_disturbance_rejection(U, Y, Uo, Yo):
    print("u", U[:, -1], "ym", Y[:, -1])
    assert near(U[:2, -1], 2.0, 1e-2) and near(Y[:2, -1], 15.0, 1e-2), (U[:, -1], Y[:, -1])       # the reference's atol
    assert not near(U[2, -1], 2.0, 1e-2)                                                          # (the neighbour is another plant)
    eu, ey = np.abs(U - Uo).max() / max(1.0, np.abs(Uo).max()), np.abs(Y - Yo).max() / max(1.0, np.abs(Yo).max())
    print("against the oracle loop", eu, ey)
    assert eu <= TOL and ey <= TOL, (eu, ey)


def check_parity(name, worst, share, kind, small=False):
    print(name, worst, "share of members with an active ymax row and Ŷs != 0:", share, "kernel kind", kind)
    assert share > 0.0
    assert worst["Z"] <= TOL and worst["u"] <= TOL and worst["Yhat"] <= TOL and worst["F"] <= FBAR and worst["twin"] <= TOL, worst
    if small:
        assert kind == api.KERNEL_SMALL, kind


def check_zero_mismatch(out):
    assert all(ok for ok, _ in out) and all(n > 0 for _, n in out), out


def check_sim(ok, final, path):
    assert path == api.SIM_PATH_PERIOD
    for k, r in enumerate(ok):
        assert r["U"] and r["Xhat"] and r["status"] and r["Yhat"] <= 1e-13, (k, r)
    assert final


def check_isolation(o):
    assert o["neighbours"] and o["off_zero"] and o["init_neighbours"] and o["init_kept"], o
    assert o["status"].tolist() == [0, 0, 0, 0, 0, 2, 0, 0, 0] and o["init_status"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0], o
    assert o["nan_ys"][0] == 0.0 and o["nan_ys"][1] != 0.0, o


def check_stale(kept, worst, mag):
    assert kept and mag > 1e-3 and worst <= FBAR, (kept, worst, mag)


def check_refusals(got, unchanged):
    for k, (rc, want) in got.items():
        assert rc == want, (k, rc, want)
    assert unchanged


def check_validation(o):
    assert o["Ds_zero"] and "nonzero direct transmission" in o["Ds_zero"], o
    assert o["Cs_rows"] and "different from measured output quantity" in o["Cs_rows"], o
    assert o["integrating"] and "integrating or unstable" in o["integrating"], o
    assert o["direct_false"], o
