"""Shared checks of the discretisation of continuous-time models (mpcqp_c2d, mpcqp_set_model_continuous; csrc/c2d_bodies.h):
tests/test_c2d.py runs them on the CPU wave emulator (tests/emu/c2d.mk), tests/test_gpu_c2d.py on the MI355X, with the same bars.

Accuracy of the exponential.  Truth: mpmath.expm at 60 digits, stored with the inputs under tests/golden/c2d/ as hi + lo pairs
of doubles (scripts/make_c2d_golden.py).  Bar, per member: the relative Frobenius error of [Φ Γ] is at most
8 e_scipy + N 2^-53, e_scipy the error of scipy.linalg.expm on the same member against the same truth, N the block order:
each squaring at most doubles a relative error, so 8 allows three squarings more than SciPy chooses; the floor is one
length-N accumulation of unit roundoffs.  e_scipy <= 1e-11 is asserted for every stored member, so the bar can never be loose.

Tustin block.  The Markov parameters D, CB, CAB, ... (2 nx of them) of the d-channel do not depend on the realisation; truth: an
mpmath bilinear transform of the same data; bar: 8 times the error of scipy.signal.cont2discrete(method="bilinear"), plus
nx 2^-53.  The parameters of both models are accumulated in extended precision, so the bar compares the models, not the
test's own products."""
import functools
import os
import warnings

import numpy as np
import scipy.linalg
import scipy.signal

import mpcqp
from oracle import condense as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "c2d")
EMU = os.path.join(ROOT, "tests", "emu")
LIB = "libmpcqp_emu_c2d.so"
# (nx, nu, nd, B): a scalar member; a small block; C3 dimensions; both d_methods; block order 32 exactly; nx = 16 (with four
# integrators in the augmentation tests: the boundary of the 16-lane row family of the estimator kernels)
SHAPES = [(1, 1, 0, 3), (2, 1, 0, 12), (12, 4, 0, 12), (12, 4, 2, 6), (28, 4, 0, 4), (16, 4, 0, 4)]
UNSUPPORTED = (29, 4, 0, 2)
ACCURACY_CASES = [(s, "tustin") for s in SHAPES] + [((12, 4, 2, 6), "zoh")]
U = 2.0 ** -53
LD = np.longdouble


def build():
    """make tests/emu/libmpcqp_emu_c2d.so (tests/emu/c2d.mk); returns its path."""
    import subprocess
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "c2d.mk", LIB])
    return os.path.join(EMU, LIB)


@functools.lru_cache(maxsize=None)
def golden(shape):
    g = dict(np.load(os.path.join(GOLDEN, "%d_%d_%d_%d.npz" % shape)))
    for v in g.values():
        v.setflags(write=False)
    return g


def rel_err(got, hi, lo):
    d = (np.asarray(got, LD) - np.asarray(hi, LD)) - np.asarray(lo, LD)
    return float(np.sqrt((d * d).sum()) / np.sqrt((np.asarray(hi, LD) ** 2).sum()))


def block(g, b, N):
    nx = g["A"].shape[1]
    M = np.zeros((N, N))
    M[:nx] = np.hstack([g["A"][b], g["Bu"][b], g["Bd"][b]])[:, :N]
    return M


def run(g, method="tustin", lib=None, **kw):
    nd = g["Bd"].shape[2]
    return mpcqp.c2d(g["A"], g["Bu"], g["C"], g["Ts"], g["Bd"] if nd else None, g["Dd"] if nd else None, d_method=method,
                     lib=lib, **kw)


def check_accuracy(shape, method, lib=None):
    """[Φ Γu (Γd)] of every member of the shape against the stored truth, with the bar above; returns the ratios to SciPy."""
    nx, nu, nd, B = shape
    g = golden(shape)
    N = nx + nu + (nd if method == "zoh" else 0)
    Ah, Bh, _, Bdh, _, st = run(g, method, lib=lib)
    assert not st.any(), st
    ratios = []
    for b in range(B):
        got = np.hstack([Ah[b, :nx, :nx], Bh[b, :nx]] + ([Bdh[b, :nx]] if method == "zoh" and nd else []))
        hi, lo = g["hi"][b][:, :N], g["lo"][b][:, :N]
        e_scipy = rel_err(scipy.linalg.expm(block(g, b, N) * g["Ts"][b])[:nx], hi, lo)
        e = rel_err(got, hi, lo)
        bar = 8.0 * e_scipy + N * U
        ratios.append(e / max(e_scipy, U))
        print("shape", shape, method, "member", b, "family", int(g["family"][b]), "norm index", int(g["norm"][b]),
              "e %.3g e_scipy %.3g bar %.3g" % (e, e_scipy, bar))
        assert e_scipy <= 1e-11
        assert e <= bar, (b, e, e_scipy, bar)
    return ratios


def check_closed_forms(lib=None):
    # A = 0: Φ = I and Γ = Ts B, to 1 ulp
    rng = np.random.default_rng(3)
    B, nx, nu = 4, 5, 2
    Bu, Ts = rng.standard_normal((B, nx, nu)), np.array([0.01, 0.3, 2.0, 40.0])
    Ah, Bh, Ch, _, _, st = mpcqp.c2d(np.zeros((B, nx, nx)), Bu, np.ones((B, 1, nx)), Ts, lib=lib)
    want = Bu * Ts[:, None, None]
    assert not st.any() and np.array_equal(Ah, np.broadcast_to(np.eye(nx), (B, nx, nx)))
    assert (np.abs(Bh - want) <= np.spacing(np.abs(want))).all()
    # the double integrator: Φ = [[1, Ts], [0, 1]], Γ = [Ts^2/2; Ts]
    Ts = np.array([0.1, 1.0, 7.0])
    A = np.broadcast_to(np.array([[0.0, 1.0], [0.0, 0.0]]), (3, 2, 2))
    Ah, Bh, _, _, _, st = mpcqp.c2d(A, np.broadcast_to(np.array([[0.0], [1.0]]), (3, 2, 1)), np.ones((3, 1, 2)), Ts, lib=lib)
    assert not st.any()
    for b, t in enumerate(Ts):
        assert np.allclose(Ah[b], [[1.0, t], [0.0, 1.0]], rtol=4 * U * 2, atol=0) and Ah[b, 1, 0] == 0.0
        assert np.allclose(Bh[b, :, 0], [t * t / 2, t], rtol=8 * U, atol=0)
    # T1's model 5 / (2s + 1) at Ts = 3: Φ = exp(-1.5), DC gain 5
    Ah, Bh, Ch, _, _, st = mpcqp.c2d(-0.5, 1.0, 2.5, 3.0, lib=lib)
    assert not st.any() and abs(Ah[0, 0, 0] - np.exp(-1.5)) <= 4 * U
    assert abs(Ch[0, 0, 0] * Bh[0, 0, 0] / (1.0 - Ah[0, 0, 0]) - 5.0) <= 5.0 * 16 * U


def _markov_ld(A, Bm, Cm, D, n):
    A, Bm, Cm, D = (np.asarray(M, LD) for M in (A, Bm, Cm, D))
    out, X = [D], Bm
    for _ in range(n - 1):
        out.append(Cm @ X)
        X = A @ X
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def tustin_truth(shape):
    """Markov parameters of the bilinear transform of every member's d-channel, by mpmath at 60 digits (hi, lo)."""
    import mpmath as mp
    mp.mp.dps = 60
    g = golden(shape)
    nx, nd = g["A"].shape[1], g["Bd"].shape[2]
    his, los = [], []
    for b in range(g["A"].shape[0]):
        A, Bd, Cm, Dd = (mp.matrix(g[k][b].tolist()) for k in ("A", "Bd", "C", "Dd"))
        a = mp.mpf(float(g["Ts"][b])) / 2
        W = mp.inverse(mp.eye(nx) - a * A)
        At, Bt, Ct, Dt = W * (mp.eye(nx) + a * A), W * Bd * (2 * a), Cm * W, Dd + a * (Cm * W * Bd)
        par, X = [Dt], Bt
        for _ in range(2 * nx - 1):
            par.append(Ct * X)
            X = At * X
        hi = np.array([[[float(P[i, j]) for j in range(nd)] for i in range(P.rows)] for P in par])
        lo = np.array([[[float(P[i, j] - mp.mpf(hi[k][i][j])) for j in range(nd)] for i in range(P.rows)] for k, P in enumerate(par)])
        his.append(hi)
        los.append(lo)
    return np.array(his), np.array(los)


def check_tustin(lib=None, shape=(12, 4, 2, 6)):
    nx, nu, nd, B = shape
    g = golden(shape)
    Ah, Bh, Ch, Bdh, Ddh, st = run(g, "tustin", lib=lib)
    assert not st.any() and Ah.shape == (B, 2 * nx, 2 * nx)
    # the stacking [sysu_dis sysd_dis]: blkdiag(Φ, At), Bu = [Γu; 0], Bd = [0; Bt], C = [C, Ct]
    assert not Ah[:, :nx, nx:].any() and not Ah[:, nx:, :nx].any() and not Bh[:, nx:].any() and not Bdh[:, :nx].any()
    assert np.array_equal(Ch[:, :, :nx], g["C"])
    hi, lo = tustin_truth(shape)
    ratios = []
    for b in range(B):
        got = _markov_ld(Ah[b], Bdh[b], Ch[b], Ddh[b], 2 * nx)
        sd = scipy.signal.cont2discrete((g["A"][b], g["Bd"][b], g["C"][b], g["Dd"][b]), g["Ts"][b], method="bilinear")
        ref = _markov_ld(sd[0], sd[1], sd[2], sd[3], 2 * nx)
        e, e_scipy = rel_err(got, hi[b], lo[b]), rel_err(ref, hi[b], lo[b])
        bar = 8.0 * e_scipy + nx * U
        ratios.append(e / max(e_scipy, U))
        print("tustin member", b, "family", int(g["family"][b]), "e %.3g e_scipy %.3g bar %.3g" % (e, e_scipy, bar))
        assert e <= bar, (b, e, e_scipy, bar)
    # I - aA exactly singular: A = diag(2 / Ts, -1)
    Ts = 0.5
    A = np.stack([np.diag([2.0 / Ts, -1.0]), np.diag([-3.0, -1.0])])
    one = np.ones((2, 2, 1))
    res = mpcqp.c2d(A, one, np.ones((2, 1, 2)), Ts, one, np.ones((2, 1, 1)), lib=lib)
    assert res[5].tolist() == [2, 0] and not res[0][0].any() and res[0][1].any()
    return ratios


NINTS_U = [0, 1, [2, 0, 1, 0]]
NINTS_YM = [0, 1, [2, 0, 1]]
I_YM = [0, 2, 3]            # (partial: output 1 is not measured)


def check_augmentation(shape, method, lib=None):
    """Against oracle.condense.init_estimstoch / augment_model fed with the device's own discrete plant: bit for bit."""
    nx, nu, nd, B = shape
    g = golden(shape)
    ny = g["C"].shape[1]
    A, Bu, Cm, Bd, Dd, st0 = run(g, method, lib=lib)
    assert not st0.any()
    nxd = A.shape[1]
    dop = np.random.default_rng(9).standard_normal((B, nxd))
    for nint_u in NINTS_U:
        for nint_ym in NINTS_YM:
            got = run(g, method, lib=lib, nint_u=nint_u, nint_ym=nint_ym, i_ym=I_YM, dop=dop)
            assert not got[5].any()
            each = lambda v, n: [v] * n if np.isscalar(v) and v != 0 else v      # (the oracle takes 0 or one count per channel)
            As, Cs_u, Cs_y, _, _ = cd.init_estimstoch(nu, ny, I_YM, each(nint_u, nu), each(nint_ym, len(I_YM)))
            for b in range(B):
                want = cd.augment_model(A[b], Bu[b], Cm[b], Bd[b] if nd else np.zeros((nxd, 0)), Dd[b] if nd else np.zeros((ny, 0)),
                                        np.zeros(nxd), dop[b], As, Cs_u, Cs_y)
                assert got[0][b].shape == want[0].shape, (nint_u, nint_ym)
                for k, (x, w) in enumerate(zip((got[0], got[1], got[2]) + ((got[3], got[4]) if nd else ()),
                                               want[:3] + (want[3:5] if nd else ()))):
                    assert x[b].tobytes() == np.ascontiguousarray(w).tobytes(), (nint_u, nint_ym, b, k)
                assert got[6][b].tobytes() == want[6].tobytes()


# ---- the handle -------------------------------------------------------------------------------------------------------------
HP, HC = 6, 2


def handle_for(o, lib=None, seed=0):
    h = mpcqp.api.Handle(o.B, o.nxh, o.nu, o.ny, o.nd, HP, HC, lib=lib)
    rng = np.random.default_rng(seed)
    h.set_weights(rng.uniform(0.5, 2.0, (o.B, h.nY)), rng.uniform(0.1, 1.0, (o.B, h.nDU)), rng.uniform(0.0, 0.5, (o.B, h.nU)), np.full(o.B, 1e5))
    return h


def abi(g):
    nd = g["Bd"].shape[2]
    cm = mpcqp.colmajor
    return [cm(g["A"]), cm(g["Bu"]), cm(g["C"]), np.ascontiguousarray(g["Ts"]), cm(g["Bd"]) if nd else None, cm(g["Dd"]) if nd else None]


def options(g, method="tustin", nint_u=0, nint_ym=1, i_ym=None):
    B, nx, nu = g["Bu"].shape
    return mpcqp.C2dOptions(B, nx, nu, g["C"].shape[1], g["Bd"].shape[2], nint_u, nint_ym, i_ym, method)


TABLES = (mpcqp.api.GET_HESSIAN, mpcqp.api.GET_STEPRESP, mpcqp.api.GET_KMAT, mpcqp.api.GET_BVEC)


def tables(h):
    return [h.get(w).tobytes() for w in TABLES]


def check_handle(shape, method, lib=None):
    """set_model_continuous == c2d followed by set_model: H̃, the step responses, K and B bit-identical; so is the read-back."""
    g = golden(shape)
    nd = g["Bd"].shape[2]
    o = options(g, method)
    dop = np.random.default_rng(5).standard_normal((o.B, o.nxd))
    ha, hb = handle_for(o, lib), handle_for(o, lib)
    st = ha.set_model_continuous(o, *abi(g), dop)
    assert not st.any()
    res = run(g, method, lib=lib, nint_ym=1, dop=dop)
    cm = mpcqp.colmajor
    hb.set_model(cm(res[0]), cm(res[1]), cm(res[2]), cm(res[3]) if nd else None, cm(res[4]) if nd else None, res[6])
    assert tables(ha) == tables(hb)
    back = ha.get_model()
    for x, w in zip(back, res[:5] + (res[6],)):
        assert (x is None and w is None) or x.tobytes() == w.tobytes()


def check_device_stream(lib=None, shape=(12, 4, 0, 12)):
    """The _device call on a torch stream, followed by step_device with no synchronisation between them, against the host
    variant: bit for bit."""
    import torch
    g = golden(shape)
    o = options(g)
    dev = torch.device("cuda", 0)
    ha, hb = handle_for(o, lib), handle_for(o, lib)
    B = o.B
    rng = np.random.default_rng(1)
    x, lu, ry = rng.standard_normal((B, o.nxh)), np.zeros((B, o.nu)), rng.standard_normal((B, ha.nY))
    assert not ha.set_model_continuous(o, *abi(g)).any()
    Za = np.zeros((B, ha.nZ))
    ua, sa, _ = ha.step(x, lu, ry, Za)[:3]
    t = lambda a, dt=torch.float64: torch.as_tensor(np.array(a, order="C"), dtype=dt, device=dev)
    args = [t(a) for a in abi(g)[:4]]
    st_d, xd, lud, ryd = torch.zeros(B, dtype=torch.int32, device=dev), t(x), t(lu), t(ry)
    Zd, ud, sd, itd = t(np.zeros((B, ha.nZ))), t(np.zeros((B, o.nu))), torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        hb.set_model_continuous_device(o, args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), args[3].data_ptr(), st_d.data_ptr(),
                                       stream=s.cuda_stream)
        hb.step_device(xd.data_ptr(), lud.data_ptr(), ryd.data_ptr(), Zd.data_ptr(), ud.data_ptr(), sd.data_ptr(), itd.data_ptr(),
                       stream=s.cuda_stream)
    s.synchronize()
    assert not st_d.cpu().numpy().any()
    assert ud.cpu().numpy().tobytes() == np.ascontiguousarray(ua).tobytes() and Zd.cpu().numpy().tobytes() == Za.tobytes()
    assert tables(ha) == tables(hb)


def check_refusals(lib=None, shape=(12, 4, 0, 12)):
    """A batch of 7: member 2 gets a NaN, member 5 Ts = 0.  Both are refused and keep their H̃; the other five are bit-equal to
    the same batch without the two; the controller warns with the count."""
    g = {k: v[:7].copy() for k, v in golden(shape).items()}
    good = options(g)
    h = handle_for(good, lib)
    first = dict(g, A=0.5 * g["A"])
    assert not h.set_model_continuous(good, *abi(first)).any()
    H0 = h.get(mpcqp.api.GET_HESSIAN)
    model0 = h.get_model()
    bad = dict(g, A=g["A"].copy(), Ts=g["Ts"].copy())
    bad["A"][2, 1, 3] = np.nan
    bad["Ts"][5] = 0.0
    st = h.set_model_continuous(good, *abi(bad))
    assert st.tolist() == [0, 0, 2, 0, 0, 2, 0]
    H1, model1 = h.get(mpcqp.api.GET_HESSIAN), h.get_model()
    assert H1[[2, 5]].tobytes() == H0[[2, 5]].tobytes()
    assert model1[0][[2, 5]].tobytes() == model0[0][[2, 5]].tobytes()
    keep = [0, 1, 3, 4, 6]
    five = {k: np.ascontiguousarray(v[keep]) for k, v in g.items()}
    o5 = options(five)
    h5 = mpcqp.api.Handle(5, o5.nxh, o5.nu, o5.ny, 0, HP, HC, lib=lib)
    rng = np.random.default_rng(0)       # (the weights of handle_for, its members 0, 1, 3, 4, 6)
    w = [rng.uniform(0.5, 2.0, (7, h.nY)), rng.uniform(0.1, 1.0, (7, h.nDU)), rng.uniform(0.0, 0.5, (7, h.nU))]
    h5.set_weights(*[np.ascontiguousarray(a[keep]) for a in w], np.full(5, 1e5))
    assert not h5.set_model_continuous(o5, *abi(five)).any()
    assert h5.get(mpcqp.api.GET_HESSIAN).tobytes() == H1[keep].tobytes()
    assert h5.get_model()[0].tobytes() == model1[0][keep].tobytes()
    # the standalone call: the refused members' outputs are not written
    res = run(bad, lib=lib, nint_ym=1, out=[np.full_like(m, 7.0) for m in model1[:3]] + [None, None])
    assert res[5].tolist() == st.tolist() and (res[0][[2, 5]] == 7.0).all() and res[0][keep].tobytes() == model1[0][keep].tobytes()
    # the controller: one warning with the count
    import pytest
    kw = dict(Hp=HP, Hc=HC, lib=lib)
    mpc = mpcqp.BatchLinMPC.from_continuous(first["A"], g["Bu"], g["C"], g["Ts"], nint_ym=1, **kw)
    with pytest.warns(RuntimeWarning, match=r"\(2 of 7 controllers\)") as rec:
        mpc.setmodel_continuous(bad["A"], g["Bu"], g["C"], bad["Ts"])
    assert len([x for x in rec if issubclass(x.category, RuntimeWarning)]) == 1
    assert mpc.c2d_status.tolist() == st.tolist() and mpc._Ahat.tobytes() == model1[0].tobytes()
    with pytest.warns(RuntimeWarning, match=r"\(2 of 7 controllers\)"):
        z = mpcqp.BatchLinMPC.from_continuous(bad["A"], g["Bu"], g["C"], bad["Ts"], nint_ym=1, **kw)
    assert not z._Ahat[[2, 5]].any()


def check_tiled(lib=None, shape=(12, 4, 0, 12), B=1027):
    """The 7 models of the shape tiled to B = 1027: each bit-equal to its twin."""
    g = {k: v[:7] for k, v in golden(shape).items()}
    idx = np.arange(B) % 7
    big = {k: np.ascontiguousarray(v[idx]) for k, v in g.items()}
    small, tiled = run(g, lib=lib, nint_ym=1), run(big, lib=lib, nint_ym=1)
    assert not tiled[5].any()
    for x, y in zip(small[:3], tiled[:3]):
        assert y.tobytes() == np.ascontiguousarray(x[idx]).tobytes()


def check_end_to_end(lib=None):
    """Reference doctest T8 (ext/LinearMPCext.jl:255-269) from the continuous model 2 / (10 s + 1): u = 17.577311."""
    mpc = mpcqp.BatchLinMPC.from_continuous(-0.1, 0.5, 0.4, 1.0, nint_ym=1, Hp=10, Hc=2, lib=lib)
    assert mpc.nxh == 2 and not mpc.c2d_status.any()
    mpc.setestimator(steady=dict(Qhat=np.eye(2), Rhat=np.eye(1)))
    mpc.preparestate([1.0])
    u = mpc.moveinput(mpc.xhat0, [10.0])
    assert round(float(u[0, 0]), 6) == 17.577311


def check_setmodel_gains(lib=None, shape=(2, 1, 0, 12)):
    """setmodel_continuous on a controller with steady= (then luenberger=) leaves the same gain, bit for bit, as setmodel with
    the discrete matrices; so do x̂op / f̂op and the condensed tables."""
    g = {k: v[[0, 1, 3, 5]] for k, v in golden(shape).items()}      # (|M Ts| = 0.01 or 1: Φ is far from singular, so that every
    B, nx = 4, shape[0]                                              # observer pole can be placed)
    g2 = dict(g, A=0.7 * g["A"])
    kw = dict(Hp=HP, Hc=HC, lib=lib)
    for est in (dict(steady=dict(Qhat=np.eye(nx + 1), Rhat=np.eye(1))), dict(luenberger=dict(poles=np.linspace(0.2, 0.6, nx + 1)))):
        a = mpcqp.BatchLinMPC.from_continuous(g["A"], g["Bu"], g["C"], g["Ts"], nint_ym=1, **kw)
        b = mpcqp.BatchLinMPC.from_continuous(g["A"], g["Bu"], g["C"], g["Ts"], nint_ym=1, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            a.setestimator(**est)
            b.setestimator(**est)
            K0 = a.hd.kf_gain()
            xop, fop = np.full((B, nx), 0.25), np.full((B, nx), 0.5)
            a.setmodel_continuous(g2["A"], g["Bu"], g["C"], g["Ts"], xop=xop, fop=fop)
            res = run(g2, lib=lib, nint_ym=1)
            pad = lambda v: np.hstack([v, np.zeros((B, 1))])
            b.setmodel(res[0], res[1], res[2], xhop=pad(xop), fhop=pad(fop))
        assert not a.hd.kf_status().any()
        assert a.hd.kf_gain().tobytes() == b.hd.kf_gain().tobytes() and a.hd.kf_gain().tobytes() != K0.tobytes()
        assert tables(a.hd) == tables(b.hd) and a._Ahat.tobytes() == b._Ahat.tobytes() and a._Chat.tobytes() == b._Chat.tobytes()
        assert a.xhop.tobytes() == b.xhop.tobytes() and a.fhop.tobytes() == b.fhop.tobytes()
        assert a.hd.get_model()[5].tobytes() == b.hd.get_model()[5].tobytes()


def check_contract(lib=None):
    """Null pointers, mismatched dimensions, the limits, and the unchanged handle after each refusal."""
    import ctypes as C
    import pytest
    lib_ = lib or mpcqp.api.load_library()
    err = lambda code: pytest.raises(mpcqp.MpcqpError, match="error %d:" % code)
    g = {k: v[:3] for k, v in golden((2, 1, 0, 12)).items()}
    o = options(g)
    h = handle_for(o, lib)
    assert not h.set_model_continuous(o, *abi(g)).any()
    before = tables(h) + [m.tobytes() for m in h.get_model() if m is not None]
    same = lambda: tables(h) + [m.tobytes() for m in h.get_model() if m is not None] == before
    a = abi(g)
    for k in (0, 1, 2, 3):                                  # MPCQP_ERR_NULL
        miss = list(a)
        miss[k] = None
        with err(-1):
            h.set_model_continuous(o, *miss)
    st = np.zeros(3, np.int32)
    cin = mpcqp.api.C2dIn(*[mpcqp.api._ptr(x) for x in a[:3]], None, None, mpcqp.api._ptr(a[3]), None)
    assert lib_.mpcqp_set_model_continuous(h.h, None, C.byref(cin), mpcqp.api._ptr(st)) == -1
    assert lib_.mpcqp_set_model_continuous(h.h, C.byref(o.spec), C.byref(cin), None) == -1
    assert lib_.mpcqp_c2d(C.byref(o.spec), C.byref(cin), None, mpcqp.api._ptr(st)) == -1
    # the handle's nx̂ is that of nint_ym = 1: anything else is MPCQP_ERR_ARG
    for other in (options(g, nint_ym=0), options(g, nint_ym=2), options(g, nint_u=1, nint_ym=1)):
        with err(-3):
            h.set_model_continuous(other, *a)
    g2 = {k: v[:2] for k, v in g.items()}
    with err(-3):                                           # another batch
        h.set_model_continuous(options(g2), *abi(g2))
    bad = options(g)
    bad.spec.d_method = 5
    with err(-3):
        h.set_model_continuous(bad, *a)
    bad = options(g)
    bad.spec.nx = 0
    with err(-2):
        h.set_model_continuous(bad, *a)
    assert same()
    # beyond the limits: block order 33; nx̂ = 65
    nx, nu, nd, B = UNSUPPORTED
    rng = np.random.default_rng(0)
    big = (-np.eye(nx)[None].repeat(B, 0), rng.standard_normal((B, nx, nu)), rng.standard_normal((B, 1, nx)), 1.0)
    with err(-4):
        mpcqp.c2d(*big, lib=lib)
    with err(-4):
        mpcqp.c2d(*big, nint_ym=1, lib=lib)
    hbig = mpcqp.api.Handle(B, nx + 1, nu, 1, 0, HP, HC, lib=lib)
    with err(-4):
        hbig.set_model_continuous(mpcqp.C2dOptions(B, nx, nu, 1, 0, 0, 1), mpcqp.colmajor(big[0]), mpcqp.colmajor(big[1]),
                                  mpcqp.colmajor(big[2]), np.ones(B))
    with err(-5):                                           # ... and it still has no model
        hbig.get(mpcqp.api.GET_KMAT)
    with err(-4):
        mpcqp.c2d(g["A"], g["Bu"], g["C"], g["Ts"], nint_ym=63, lib=lib)
    # a discretised model serves as the plant of sim
    res = run(g, lib=lib)
    h.sim_set_plant(*[mpcqp.colmajor(m) for m in res[:3]])
    assert same()


def refused_by_stock_library(lib):
    """A library without the launcher links (weak declaration) and answers MPCQP_ERR_UNSUPPORTED; set_model still works."""
    import pytest
    g = {k: v[:3] for k, v in golden((2, 1, 0, 12)).items()}
    o = options(g)
    with pytest.raises(mpcqp.MpcqpError, match="error -4:"):
        run(g, lib=lib)
    h = handle_for(o, lib)
    with pytest.raises(mpcqp.MpcqpError, match="error -4:"):
        h.set_model_continuous(o, *abi(g))
    with pytest.raises(mpcqp.MpcqpError, match="error -5:"):
        h.get(mpcqp.api.GET_KMAT)
    h.set_model(np.zeros((3, o.nxh, o.nxh)), np.ones((3, o.nu, o.nxh)), np.ones((3, o.nxh, o.ny)))
    assert h.get(mpcqp.api.GET_KMAT).shape == (3, o.nxh, h.nY)
