"""The batched ExplicitMPC on the CPU wave emulator (tests/emu/libmpcqp_emu_explicit.so: csrc/explicit_bodies.h under the
launchers of tests/emu/emu_explicit.cpp).  Every comparison with the oracle's closed form -H̃⁻¹ q̃ is held to
explicit_util.BAR = 1e-9 * max(1, max|reference|); the reference's own known answers keep the reference's tolerances
(test/3_test_predictive_control.jl:640-670, 743-771, 1593-1630)."""
import os
import subprocess

import numpy as np
import pytest

import mpcqp
from tests import emu_util, explicit_util as xu

BAR = xu.BAR
pytestmark = pytest.mark.slow


@pytest.fixture(scope="module")
def lib():
    return mpcqp.api.load_library(xu.build())


def _check(r, law=False):
    assert np.all(r["status"] == 0) and np.all(r["factor_status"] == 0)
    keys = ["Z", "u", "Y", "step_vs_mpcqp_step"] + (["law_tables"] if law else [])
    if law and "law_Z" in r:
        keys += ["law_Z", "law_vs_step", "law_u"]
        assert r["law_u_only"] == 0.0 and np.all(r["law_status"] == 0)
    print({k: r[k] for k in keys}, "cond", r["cond"])
    for k in keys:
        assert r[k] <= BAR, (k, r[k])


def test_T7_step_against_closed_form(lib):
    """Hp = 30, Hc = [2, 3, 4, 21] (test_gpu_parity.py T7's controller): explicit step and law against the oracle."""
    _check(xu.run_shape(lib, nx=3, nu=2, ny=2, Hp=30, Hc=[2, 3, 4, 21], B=3, law=True), law=True)


@pytest.mark.parametrize("law", [False, True])
def test_T7_closed_loop_against_unconstrained_linmpc(lib, law):
    """test/3_test_predictive_control.jl:1593-1630: U0 ≈ U1, rtol = atol = 1e-3."""
    U0, U1 = xu.run_T7_closed_loop(lib, law=law)
    assert np.allclose(U0, U1, rtol=1e-3, atol=1e-3)
    assert np.abs(U0 - U1).max() <= BAR * max(1.0, np.abs(U1).max())


def test_reference_known_answers(lib):
    """test/3_test_predictive_control.jl:640-670 at its tolerances."""
    model, kf, mpc = xu.tf_pair(5.0, 2.0, 3.0, lib=lib, Nwt=[0], Hp=1000, Hc=1)
    kf.preparestate([0])
    x = np.tile(kf.x0, (3, 1))
    assert mpc.moveinput(x, [5]) == pytest.approx(np.ones((3, 1)), abs=1e-2)
    u = mpc.moveinput(x, [5], lastu=[-1], want_info=True)
    assert u == pytest.approx(np.ones((3, 1)), abs=1e-2)
    info = mpc.getinfo()
    assert np.array_equal(info["u"], u)
    assert info["Ŷ"][:, -1] == pytest.approx(np.full(3, 5.0), abs=1e-2)
    assert info["ΔU"] == pytest.approx(np.full((3, 1), 2.0), abs=1e-2)
    assert np.all(np.isnan(info["x̂end"])) and info["U"].shape == (3, 1000)
    # the law serves the same call
    _, kf, mpc = xu.tf_pair(5.0, 2.0, 3.0, lib=lib, law=True, Nwt=[0], Hp=1000, Hc=1)
    assert mpc.moveinput(x, [5]) == pytest.approx(np.ones((3, 1)), abs=1e-2)
    # Mwt = Nwt = 0, Lwt = 1, R̂u = 12 (the reference's default horizons: Hp = 10 + nk, Hc = 2)
    _, kf, mpc = xu.tf_pair(5.0, 2.0, 3.0, lib=lib, Mwt=[0], Nwt=[0], Lwt=[1], Hp=10, Hc=2)
    assert mpc.moveinput(np.zeros((3, 2)), [0], Rhatu=np.full(10, 12.0)) == pytest.approx(np.full((3, 1), 12.0), abs=1e-2)
    # move blocking
    _, kf, mpc = xu.tf_pair(5.0, 2.0, 3.0, lib=lib, Hp=10, Hc=[1, 2, 3, 4], Nwt=[10])
    assert mpc.nb == [1, 2, 3, 4]
    mpc.moveinput(np.zeros((3, 2)), [5], want_info=True)
    dU = np.diff(mpc.getinfo()["U"], axis=1)
    assert np.abs(dU[:, [1, 3, 4, 6, 7, 8]]).max() <= 1e-9


def test_setconstraint_raises_and_constructor_keywords(lib):
    """:743-748, and the keywords ExplicitMPC does not have (explicitmpc.jl:135-179)."""
    _, _, mpc = xu.tf_pair(5.0, 2.0, 3.0, lib=lib, Hp=1, Hc=1)
    with pytest.raises(mpcqp.MpcqpError, match="ExplicitMPC does not support constraints"):
        mpc.setconstraint(umin=[0.0])
    for kw in (dict(Cwt=1e5), dict(transcription="MultipleShooting"), dict(Wy=np.ones((1, 1)))):
        with pytest.raises(TypeError):
            xu.tf_pair(5.0, 2.0, 3.0, lib=lib, Hp=2, Hc=1, **kw)


@pytest.mark.parametrize("law", [False, True])
def test_setmodel_with_new_operating_points(lib, law):
    """:750-771: u ≈ 2, 15, 13 (atol 1e-2) across two setmodel! calls."""
    from oracle import estim as es
    model, kf, mpc = xu.tf_pair(5.0, 2.0, 3.0, lib=lib, law=law, Nwt=[0], Hp=1000, Hc=1, yop=[10], uop=[1])
    assert np.all(mpc.Yop == 10.0) and np.all(mpc.Uop == 1.0)
    kf.preparestate([10])
    x = np.tile(kf.x0, (3, 1))
    assert mpc.moveinput(x, [15]) == pytest.approx(np.full((3, 1), 2.0), abs=1e-2)
    assert mpc.lastu0 == pytest.approx(np.full((3, 1), 1.0), abs=1e-2)
    rep = lambda a: np.broadcast_to(a, (3,) + a.shape).copy()
    mpc.setmodel(rep(kf.Ah), rep(kf.Bhu), rep(kf.Ch), yop=[20], uop=[11])
    assert np.all(mpc.Yop == 20.0) and np.all(mpc.Uop == 11.0)
    assert mpc.lastu0 == pytest.approx(np.full((3, 1), 2.0 - 11.0), abs=1e-2)
    assert mpc.moveinput(x, [40]) == pytest.approx(np.full((3, 1), 15.0), abs=1e-2)
    A, Bm, C = es.tf1_zoh(10.0, 2.0, 3.0)
    kf2 = es.SteadyKalmanFilterOracle(es.LinModelOracle(A, Bm, C, Ts=3.0))
    mpc.setmodel(rep(kf2.Ah), rep(kf2.Bhu), rep(kf2.Ch))
    # (x̂0 = [0, 0] in both realisations: y = yop is the estimate of this test at every call)
    assert mpc.moveinput(x, [40]) == pytest.approx(np.full((3, 1), 13.0), abs=1e-2)


def test_setmodel_with_new_state_operating_point_keeps_the_estimate(lib):
    """setmodel! with a new x̂op: the attached estimator's x̂ keeps its engineering value (x̂0 += x̂op_old - x̂op_new)."""
    _, kf, mpc = xu.tf_pair(5.0, 2.0, 3.0, lib=lib, Hp=5, Hc=1)
    mpc.setestimator(np.broadcast_to(kf.Khat, (3,) + kf.Khat.shape).copy(), xhat0=np.array([[0.3, -0.2], [1.0, 2.0], [0.0, 0.5]]))
    before, old = mpc.xhat0 + mpc.xhop, mpc.xhop.copy()
    rep = lambda a: np.broadcast_to(a, (3,) + a.shape).copy()
    mpc.setmodel(rep(kf.Ah), rep(kf.Bhu), rep(kf.Ch), xhop=[0.25, -1.5], fhop=[0.25, -1.5])
    assert np.array_equal(mpc.xhop, np.tile([0.25, -1.5], (3, 1))) and not np.array_equal(mpc.xhop, old)
    assert mpc.xhat0 + mpc.xhop == pytest.approx(before, abs=1e-15)


def test_moveinput_law_for_u_alone(lib):
    """`want_Z=False` on the law path: the table of nu rows per controller, the same u to the last bit, no Z̃."""
    cfg, bt = xu.random_batch(4, 2, 2, 12, 3, 5, seed=9)
    inp = xu.period_inputs(cfg, bt, seed=9)
    us = []
    for want_Z in (True, False):
        mpc, _ = xu.make_pair(cfg, bt, lib=lib, law=True)
        us.append(mpc.moveinput(inp["x"], inp["ry"], lastu=inp["lastu"], want_Z=want_Z))
        assert np.all(np.isnan(mpc.Z)) != want_Z and np.array_equal(mpc.lastu0, us[-1] - mpc.uop)
    assert np.array_equal(us[0], us[1])


SHAPES = {
    "C2": dict(nx=4, nu=2, ny=2, Hp=20, Hc=5, B=5, law=True),                       # n = 10
    "C3": dict(nx=12, nu=4, ny=4, Hp=30, Hc=10, B=3, law=True),                     # n = 40
    "n64": dict(nx=4, nu=4, ny=2, Hp=20, Hc=16, B=3, law=True),                     # n = 64: every lane owns a row
    "nd_preview_ops": dict(nx=3, nu=2, ny=2, Hp=12, Hc=3, B=4, nd=1, ops=True, preview=True, law=True),
    "nd_held_ops": dict(nx=3, nu=2, ny=2, Hp=12, Hc=3, B=7, nd=1, ops=True, law=True),
    "Lwt_Ru": dict(nx=4, nu=2, ny=2, Hp=10, Hc=3, B=3, weights=dict(Lwt=[0.3, 0.2]), full_ru=True),
    "Ry_full": dict(nx=4, nu=3, ny=2, Hp=9, Hc=[2, 3, 4], B=3, full_ry=True),
    "M_block": dict(nx=4, nu=2, ny=3, Hp=8, Hc=3, B=3, Mkind="block", law=True),
    "M_dense": dict(nx=4, nu=2, ny=2, Hp=8, Hc=3, B=3, Mkind="dense", law=True),
    "NL_dense": dict(nx=4, nu=2, ny=2, Hp=8, Hc=3, B=3, Nkind="dense", Lkind="dense", full_ru=True),
    "L_dense_two_chunks": dict(nx=4, nu=3, ny=2, Hp=30, Hc=3, B=3, Lkind="dense", full_ru=True),   # nU = 90 rows of L Cu
    "C3_Hp300": dict(nx=12, nu=4, ny=4, Hp=300, Hc=10, B=3, law=True),              # 63 KB of LDS
    "C3_Hp400": dict(nx=12, nu=4, ny=4, Hp=400, Hc=10, B=3),                        # 81 KB: beyond a launch's default limit
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(lib, name):
    kw = SHAPES[name]
    _check(xu.run_shape(lib, **kw), law=kw.get("law", False))


def test_keep_qp_returns_gradient_and_free_response(lib):
    """MPCQP_FLAG_KEEP_QP: q̃ and F of the explicit step through mpcqp_get, as after mpcqp_step."""
    cfg, bt = xu.random_batch(4, 2, 2, 9, 3, 3, seed=2)
    mpc = mpcqp.BatchExplicitMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], Hp=9, Hc=3, Lwt=[0.2, 0.1], keep_qp=True, lib=lib)
    _, orcs = xu.make_pair(cfg, bt, lib=lib, weights=dict(Lwt=[0.2, 0.1]), cls=xu._NoController)
    inp = xu.period_inputs(cfg, bt, seed=2)
    xu.step_call(mpc, inp, want_info=False)
    xu.oracle_period(orcs, inp)
    q, F = mpc.hd.get(mpcqp.GET_QTILDE), mpc.hd.get(mpcqp.GET_FVEC)
    assert xu.err(q, np.array([o.qt for o in orcs])) <= BAR and xu.err(F, np.array([o.F for o in orcs])) <= BAR


def test_n65_is_refused(lib):
    """nZ̃ = 65 (nu = 5, Hc = 13): MPCQP_ERR_UNSUPPORTED from prepare, as the header says; mpcqp_step goes on working."""
    cfg, bt = xu.random_batch(3, 5, 2, 14, 13, 3)
    with pytest.raises(mpcqp.MpcqpError, match="error -4"):
        xu.make_pair(cfg, bt, lib=lib)
    mpc = mpcqp.BatchLinMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], Hp=14, Hc=13, Cwt=np.inf, lib=lib)
    with pytest.raises(mpcqp.MpcqpError, match="error -5"):
        mpc.hd.explicit_step(bt["xhat0"], bt["lastu0"], np.tile(bt["ry"], 14))
    assert np.all(np.isfinite(mpc.moveinput(bt["xhat0"], bt["ry"]))) and np.all(mpc.status == 0)


def test_refresh_after_set_model(lib):
    r = xu.run_refresh(lib)
    print(r)
    assert r["step"] <= BAR and r["law"] <= BAR and r["law_tables"] <= BAR
    assert r["moved"] > 1e-6 and r["law_moved"] > 1e-6


def test_refresh_after_set_weights_and_recondense(lib):
    cfg, bt = xu.random_batch(4, 2, 2, 12, 3, 3, seed=6)
    mpc, _ = xu.make_pair(cfg, bt, lib=lib, law=True)
    inp = xu.period_inputs(cfg, bt)
    w = dict(Mwt=[2.0, 0.5], Nwt=[0.3, 0.2], Lwt=[0.1, 0.0])
    Zstale = xu.step_call(mpc, inp, want_info=False)[0]
    mpc.setweights(**w)
    _, orcs = xu.make_pair(cfg, bt, lib=lib, weights=w, cls=xu._NoController)
    Zo = xu.oracle_period(orcs, inp)[0]
    Z = xu.step_call(mpc, inp, want_info=False)[0]
    Zl = mpc.hd.explicit_law(inp["x"], inp["lastu"], inp["ry"])[0]
    assert xu.err(Z, Zo) <= BAR and xu.err(Zl, Zo) <= BAR and np.abs(Z - Zstale).max() > 1e-6
    mpc.hd.recondense_device()
    assert np.array_equal(xu.step_call(mpc, inp, want_info=False)[0], Z)


def test_status_policy(lib):
    r = xu.run_status_policy(lib)
    bad, ok, fl = r["bad"], r["regular"], r["failed"]
    others = [b for b in range(len(ok["st"])) if b != bad]
    assert np.all(ok["fst"] == 0) and fl["fst"][bad] == 2 and np.all(fl["fst"][others] == 0)
    for st in (fl["st"], fl["stl"]):
        assert st[bad] == 2 and np.all(st[others] == 0)
    for Z, u in ((fl["Z"], fl["u"]), (fl["Zl"], fl["ul"])):
        assert np.all(Z[bad] == 0.0) and np.array_equal(u[bad], r["lastu"][bad])
    assert np.all(fl["tab"][bad] == 0.0)
    for k in ("Z", "u", "Y", "Zl", "ul", "tab"):
        assert np.array_equal(fl[k][others], ok[k][others]), k


def _handle(lib, neps=0, B=2):
    cfg, bt = xu.random_batch(3, 2, 2, 6, 2, B)
    mpc = mpcqp.BatchLinMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], Hp=6, Hc=2, Cwt=1e5 if neps else np.inf, lib=lib)
    return mpc, bt


def test_refusals(lib):
    mpc, bt = _handle(lib, neps=1)
    with pytest.raises(mpcqp.MpcqpError, match="error -3"):
        mpc.hd.explicit_prepare()
    mpc, bt = _handle(lib)
    args = (bt["xhat0"], bt["lastu0"], np.tile(bt["ry"], 6))
    with pytest.raises(mpcqp.MpcqpError, match="error -5"):        # before a successful prepare
        mpc.hd.explicit_step(*args)
    with pytest.raises(mpcqp.MpcqpError, match="error -5"):
        mpc.hd.explicit_status()
    mpc.setconstraint(umax=[1.0, 1.0])                             # a finite bound before prepare
    with pytest.raises(mpcqp.MpcqpError, match="error -3"):
        mpc.hd.explicit_prepare()
    mpc, bt = _handle(lib)
    mpc.hd.explicit_prepare()
    Z = mpc.hd.explicit_step(*args)[0]
    with pytest.raises(mpcqp.MpcqpError, match="error -5"):        # law without with_law
        mpc.hd.explicit_law(bt["xhat0"], bt["lastu0"], bt["ry"])
    with pytest.raises(mpcqp.MpcqpError, match="error -5"):
        mpc.hd.get(mpcqp.api.GET_EXPLICIT_LAW)
    mpc.setconstraint(umax=[1.0, 1.0])                             # ... and after: the handle has received a row
    with pytest.raises(mpcqp.MpcqpError, match="error -5"):
        mpc.hd.explicit_step(*args)
    with pytest.raises(mpcqp.MpcqpError, match="error -5"):
        mpc.hd.explicit_status()
    mpc.setweights(Mwt=[3.0, 0.5])                                 # a setter on the constrained handle: no factor, no error ...
    mpc.hd.set_bounds()                                            # (no array: every bound group is dropped)
    Z2 = mpc.hd.explicit_step(*args)[0]                            # ... and the first explicit call without rows factors again
    ref, _ = _handle(lib)
    ref.setweights(Mwt=[3.0, 0.5])
    ref.hd.explicit_prepare()
    assert np.array_equal(Z2, ref.hd.explicit_step(*args)[0]) and np.abs(Z2 - Z).max() > 1e-6
    mpc, bt = _handle(lib)
    mpc.hd.set_transcription(mpcqp.api.MULTIPLE_SHOOTING)
    with pytest.raises(mpcqp.MpcqpError, match="error -3"):
        mpc.hd.explicit_prepare()
    mpc.hd.set_transcription(mpcqp.api.SINGLE_SHOOTING)
    with pytest.raises(mpcqp.MpcqpError, match="error -3"):        # unknown bits of with_law
        mpcqp.api._chk(lib, lib.mpcqp_explicit_prepare(mpc.hd.h, 4))
    h = mpcqp.Handle(2, 5, 2, 2, 0, 6, 2, neps=0, lib=lib)         # no model, no weights
    with pytest.raises(mpcqp.MpcqpError, match="error -5"):
        h.explicit_prepare()


def test_stock_emulator_library_refuses_and_still_steps():
    stock = mpcqp.api.load_library(emu_util.build())
    mpc, bt = _handle(stock)
    with pytest.raises(mpcqp.MpcqpError, match="error -4"):
        mpc.hd.explicit_prepare()
    u = mpc.moveinput(bt["xhat0"], bt["ry"])
    assert np.all(mpc.status == 0) and np.all(np.isfinite(u))




def test_host_code_under_sanitizers(tmp_path):
    """The explicit entry points in a stand-alone program under the address and undefined-behaviour sanitizers, linked
    against the emulator objects (the way tests/test_kf_cov.py checks its host code); nothing is loaded into python."""
    xu.build()
    exe = str(tmp_path / "explicit_asan")
    subprocess.check_call(xu.SANITIZER_CXX + ["-x", "c++", os.path.join(xu.CSRC, "mpcqp_host.hip"),
                                              os.path.join(xu.ROOT, "tests", "explicit_asan_main.cpp"), "-x", "none"]
                          + xu.SANITIZER_OBJS + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "explicit sanitizer run: ok" in out.stdout, out.stdout + out.stderr
