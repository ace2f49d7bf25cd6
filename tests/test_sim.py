"""`BatchLinMPC.sim` / mpcqp_sim on the CPU wave emulator (tests/emu/libmpcqp_emu_sim.so: csrc/sim_bodies.h under the launcher
of tests/emu/emu_sim.cpp, next to the emulated controller and estimator kernels).  The reference of every bar is the same run
one period at a time through preparestate / moveinput / updatestate around NumPy plants (tests/sim_util.py)."""
import os
import subprocess

import numpy as np
import pytest

import mpcqp
from tests import sim_util as su

pytestmark = pytest.mark.slow
VARIANTS = {"steady": {}, "time_varying": dict(estimator="tv"), "predictor_form": dict(direct=False),
            "ry_per_period": dict(ry_per_period=True)}


@pytest.fixture(scope="module")
def lib():
    return mpcqp.api.load_library(su.build())


def check_against_reference(lib, kind, variant):
    """nd = 1, operating points on every signal, a plant of another order with a gain mismatch, steps and noise on all four
    channels; every record within the bar of the kind."""
    case = su.Case(kind, fuse=False, **VARIANTS[variant])
    errs, res, ref, mpc = su.run_against_reference(case, lib)
    print(kind, variant, {k: f"{v:.2e}" for k, v in errs.items()})
    bar = su.BAR_QP if kind == "linmpc_umax" else su.BAR
    assert res.path == mpcqp.api.SIM_PATH_PERIOD and res.status.shape == (case.B, case.N)
    for k, v in errs.items():
        assert v <= bar, (k, v)
    if kind == "linmpc_umax":       # from the reference alone: some member-periods at the bound, some not
        at = np.abs(ref["U_data"] - (mpc.uop + case.umax)[:, :, None]) <= 1e-6
        assert at.any() and not at.all(), ref["U_data"]
    return errs


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", su.KINDS)
def test_per_period_path_against_reference(lib, kind, variant):
    check_against_reference(lib, kind, variant)


def test_input_setpoint_ru_takes_the_explicit_step(lib):
    """`ru` given: R̂u = repeat(ru, Hp), which the law does not serve -- the explicit step runs on the law handle."""
    case = su.Case("explicit_law", ru=True)
    errs, res, ref, _ = su.run_against_reference(case, lib)
    assert max(errs.values()) <= su.BAR, errs
    assert su.err(res.Ru_data, ref["Ru_data"]) == 0.0


BIG = dict(nx=12, nu=4, ny=4, Hp=6, Hc=2)        # nx̂ = 16 exactly
FUSED_CASES = {"small": dict(), "small_predictor": dict(direct=False), "nxhat16": dict(dims=BIG, nxp=12, N=3),
               "nxhat16_predictor": dict(dims=BIG, nxp=12, N=3, direct=False), "nxp16": dict(dims=BIG, nxp=16, N=3),
               "ones": dict(dims=dict(nx=1, nu=1, ny=1, Hp=5, Hc=2), nxp=1), "nd0_quiet": dict(nd=0, noise=False),
               "steady_from_QR": dict(estimator="steady_qr")}
FALLBACKS = {"nxhat17": ("explicit_law", dict(dims=dict(BIG, nx=13), B=3, N=3)), "nxp17": ("explicit_law", dict(dims=BIG, nxp=17, N=3)),
             "ry_per_period": ("explicit_law", dict(ry_per_period=True)), "time_varying": ("explicit_law", dict(estimator="tv")),
             "ru": ("explicit_law", dict(ru=True)), "explicit_step": ("explicit_step", dict()), "linmpc": ("linmpc", dict())}


def check_fused_against_per_period(lib, name):
    """Case 2: the single-launch path against `fuse=False` on the same explicit handles, nd = 1 with steps and noise (but in
    `nd0_quiet`), both forms; 1e-9 * max(1, max|reference|).  Measured: 7.3e-16 on the emulator, 8.8e-16 on the MI355X."""
    case = su.Case("explicit_law", **FUSED_CASES[name])
    fused, mpc = su.run(case.controller(lib), **case.args()), case.controller(lib)
    per = su.run(mpc, **{**case.args(), "fuse": False})
    assert fused.path == mpcqp.api.SIM_PATH_FUSED and per.path == mpcqp.api.SIM_PATH_PERIOD and mpc.hd.sim_path() == mpcqp.api.SIM_PATH_FUSED
    errs = {k: su.err(getattr(fused, k), getattr(per, k)) for k in su.RECORDS}
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= su.BAR and np.array_equal(fused.status, per.status), errs
    # and against the reference of case 1
    twin = case.controller(lib)
    ref = su.reference(twin, **case.args())
    errs, same = su.compare(fused, ref)
    assert same and max(errs.values()) <= su.BAR, errs


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_path_against_per_period_path(lib, name):
    check_fused_against_per_period(lib, name)


def check_fallback(lib, name):
    """What the single-launch path does not take runs on the per-period path, within the bar of case 1; the same handle shape
    without the condition is on the fused path (FUSED_CASES), so `path` here is a decision, not a constant."""
    kind, kw = FALLBACKS[name]
    case = su.Case(kind, **kw)
    errs, res, _, mpc = su.run_against_reference(case, lib)
    assert res.path == mpcqp.api.SIM_PATH_PERIOD and max(errs.values()) <= su.BAR, errs
    handle_fused = name in ("ry_per_period", "ru")       # the call, not the handle, keeps these off the fused path
    assert mpc.hd.sim_path() == (mpcqp.api.SIM_PATH_FUSED if handle_fused else mpcqp.api.SIM_PATH_PERIOD)


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_not_eligible_takes_the_per_period_path(lib, name):
    check_fallback(lib, name)


def check_member_alone(lib, kind, **kw):
    if kind == "linmpc_umax":
        return check_member_alone_bounded(lib)
    case = su.Case(kind, **kw)
    whole = su.run(case.controller(lib), **case.args())
    for b in range(case.B):
        alone = su.run(case.controller(lib, [b]), **case.args([b]))
        assert su.same_records(whole, alone, [b], [0]) == [], (kind, b)


def check_member_alone_bounded(lib):
    """The LinMPC with active bounds: mpcqp_step itself, which the period calls unchanged, gives a member alone another last
    bit than the member in a batch of five -- shown here on one `moveinput` of the same handles (7.3e-15 seen; the small-problem
    kernel shares its interior-point loop among the four controllers of a wavefront).  The simulation inherits that, so the
    property is held to BAR_QP, the bar of this kind against the reference, on every record (1.9e-14 seen over six periods)."""
    case = su.Case("linmpc_umax")
    m5, m1 = case.controller(lib), case.controller(lib, [0])
    x = case.xhat_0 - m5.xhop
    u5 = m5.moveinput(x, case.ry, case.d, lastu=case.lastu)
    u1 = m1.moveinput(x[:1], case.ry[:1], case.d[:1], lastu=case.lastu[:1])
    print("moveinput alone vs in the batch:", np.abs(u5[0] - u1[0]).max())
    assert su.err(u1[0], u5[0]) <= su.BAR_QP
    whole = su.run(case.controller(lib), **case.args())
    for b in range(case.B):
        alone = su.run(case.controller(lib, [b]), **case.args([b]))
        errs = {k: su.err(getattr(alone, k)[0], getattr(whole, k)[b]) for k in su.RECORDS}
        print(b, max(errs.values()))
        assert max(errs.values()) <= su.BAR_QP, (b, errs)


@pytest.mark.parametrize("kind", ["explicit_law", "explicit_law_per_period", "explicit_step", "linmpc", "linmpc_umax"])
def test_member_equals_itself_alone(lib, kind):
    """Bit for bit on both paths (`explicit_law` runs fused, `_per_period` the same with fuse=False); the LinMPC with active
    bounds at a stated bar, see check_member_alone_bounded."""
    if kind == "explicit_law_per_period":
        return check_member_alone(lib, "explicit_law", fuse=False)
    check_member_alone(lib, kind)


def check_two_halves(lib, kind, **kw):
    case = su.Case(kind, **kw)
    one, two = case.controller(lib), case.controller(lib)
    whole = su.run(one, **case.args())
    h = case.N // 2
    a = su.run(two, **case.args(periods=(0, h)))
    b = su.run(two, **case.args(periods=(h, case.N), first=False))
    for k in su.RECORDS:
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)], axis=2), getattr(whole, k)), k
    assert np.array_equal(np.concatenate([a.status, b.status], axis=1), whole.status)
    for k in ("xhat0", "lastu0", "Z", "sim_x0"):
        assert np.array_equal(getattr(one, k), getattr(two, k), equal_nan=True), k


@pytest.mark.parametrize("kind,kw", [("explicit_law", dict()), ("explicit_law", dict(direct=False)), ("explicit_law", dict(fuse=False)),
                                     ("explicit_law", dict(ry_per_period=True)), ("explicit_step", dict(estimator="tv")),
                                     ("linmpc_umax", dict(warm_dual=True)), ("linmpc", dict(direct=False))])
def test_two_runs_of_three_equal_one_of_six(lib, kind, kw):
    check_two_halves(lib, kind, **kw)


def check_nan(lib, kind, member=2, period=3, **kw):
    """A NaN draw in w_y of one member at one period, σy = 1: X̂ of that period is x̂ before it, the prediction runs, the
    neighbours keep their bits."""
    case = su.Case(kind, **kw)
    case.kw["y_noise"] = np.ones_like(case.kw["y_noise"])
    clean, mpc = case.controller(lib), case.controller(lib)
    draws = {k: v.copy() for k, v in case.draws.items()}
    draws["w_y"][member, :, period] = np.nan
    ref = su.run(clean, **case.args())
    su.run(mpc, **case.args(periods=(0, period)))
    before = mpc.xhat0 + mpc.xhop
    with pytest.warns(RuntimeWarning) as rec:
        pass_ = mpc.sim(**case.args(periods=(period, period + 1), first=False, draws=draws))
    assert any("skipping correction step (1 of 5 estimator periods)" in str(w.message) for w in rec)
    assert np.array_equal(pass_.X̂_data[member, :, 0], before[member])
    assert all(not np.array_equal(pass_.X̂_data[b, :, 0], before[b]) for b in range(case.B) if b != member)
    d0 = pass_.D_data[member, :, 0] - mpc.dop[member]
    u0 = pass_.U_data[member, :, 0] - mpc.uop[member]
    pred = (mpc._Ahat[member] @ (before[member] - mpc.xhop[member]) + mpc._Bhu[member] @ u0 + mpc._Bhd[member] @ d0
            + mpc.fhop[member] - mpc.xhop[member])
    assert su.err(mpc.xhat0[member], pred) <= 1e-12 and not np.array_equal(mpc.xhat0[member], before[member] - mpc.xhop[member])
    rest = su.run(mpc, **case.args(periods=(period + 1, case.N), first=False, draws=draws))
    others = [b for b in range(case.B) if b != member]
    for k in su.RECORDS:
        got = np.concatenate([pass_.__dict__[k], rest.__dict__[k]], axis=2)[others]
        assert np.array_equal(got, getattr(ref, k)[others][:, :, period:]), k
    assert np.isnan(pass_.Y_data[member, :, 0]).all()


@pytest.mark.parametrize("kind,kw", [("explicit_law", dict()), ("explicit_law", dict(fuse=False)), ("linmpc", dict())])
def test_nan_measurement_skips_one_members_correction(lib, kind, kw):
    check_nan(lib, kind, **kw)


def check_status_policy(lib, kind, bad=2, **kw):
    """An explicit member whose H̃ = 0 (explicit_util.run_status_policy): status 2 and U = lastu in every period; the
    neighbours are what they are in a run in which that member is regular."""
    case, regular = su.Case(kind, bad=bad, **kw), su.Case(kind, policy_weights=True, **kw)
    with pytest.warns(RuntimeWarning, match=r"MPC terminated without solution.*\(6 of 30 controller periods\)"):
        res = case.controller(lib).sim(**case.args())
    ok = su.run(regular.controller(lib), **regular.args())
    others = [b for b in range(case.B) if b != bad]
    assert np.all(res.status[bad] == 2) and np.all(res.status[others] == 0) and np.all(ok.status == 0)
    assert np.array_equal(res.U_data[bad], np.repeat(case.lastu[bad][:, None], case.N, axis=1))
    assert not np.array_equal(res.Ud_data[bad], res.U_data[bad])
    assert su.same_records(res, ok, others) == []


@pytest.mark.parametrize("kind,kw", [("explicit_law", dict()), ("explicit_law", dict(fuse=False)), ("explicit_step", dict())])
def test_explicit_status_2_member(lib, kind, kw):
    check_status_policy(lib, kind, **kw)


def check_waves(lib, monkeypatch, **kw):
    case = su.Case("explicit_law", dims=dict(nx=12, nu=4, ny=4, Hp=6, Hc=2), B=40, N=2, **kw)
    a = su.run(case.controller(lib), **case.args())
    monkeypatch.setenv("MPCQP_EXPLICIT_WAVES", "1")
    b = su.run(case.controller(lib), **case.args())
    assert su.same_records(a, b) == []


@pytest.mark.parametrize("kw", [dict(), dict(fuse=False)])
def test_results_do_not_depend_on_explicit_waves(lib, monkeypatch, kw):
    check_waves(lib, monkeypatch, **kw)


def check_refusals(lib):
    """The codes of include/mpcqp.h for mpcqp_sim_set_plant / mpcqp_sim, and the ValueErrors of `sim`."""
    case = su.Case("explicit_law")
    B, nxp, N = case.B, case.nxp, 2
    code = lambda n: pytest.raises(mpcqp.MpcqpError, match=f"error {n}:")
    bt, o = case.bt, case.bt["ops"]
    mpc = mpcqp.BatchExplicitMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], bt["Bhd"], bt["Dhd"], Hp=5, Hc=2, law=True, lib=lib, **o)
    hd = mpc.hd
    io = dict(ry=np.zeros((B, 1)), d=np.zeros((B, 1)), x0=np.zeros((B, nxp)), xhat0=np.zeros((B, 3)), lastu0=np.zeros((B, 1)),
              Ztilde=np.zeros((B, mpc.nZ)))
    with code(-5):                                  # no plant
        hd.sim(N, **io)
    cm = mpcqp.colmajor
    p = case.plant
    with code(-4):                                  # nxp = 65
        hd.sim_set_plant(np.zeros((B, 65, 65)), np.zeros((B, 1, 65)), np.zeros((B, 65, 1)))
    hd.sim_set_plant(cm(p["A"]), cm(p["Bu"]), cm(p["C"]), cm(p["Bd"]), cm(p["Dd"]))
    with code(-5):                                  # no estimator
        hd.sim(N, **io)
    mpc.setestimator(case.Khat)
    for n in (0, -3):
        with code(-3):
            hd.sim(n, **io)
    with code(-3):
        hd.sim(N, flags=8, **io)
    with code(-1):                                  # a σ without its draws
        hd.sim(N, sigma_y=np.ones((B, 1)), **io)
    for k in ("ry", "d", "x0", "xhat0", "lastu0"):
        with code(-1):
            hd.sim(N, **{**io, k: None})
    hd.sim(N, **{**io, "Ztilde": None})             # the law alone: u0 from the table of nu rows
    hd.sim(N, **io)
    # a controller that cannot step: a handle with a model and without weights
    raw = mpcqp.Handle(B, 3, 1, 1, 1, 5, 2, neps=0, lib=lib)
    raw.set_model(cm(bt["Ahat"]), cm(bt["Bhu"]), cm(bt["Chat"]), cm(bt["Bhd"]), cm(bt["Dhd"]))
    raw.sim_set_plant(cm(p["A"]), cm(p["Bu"]), cm(p["C"]))
    raw.kf_set(cm(case.Khat), np.arange(1))
    with code(-5):
        raw.sim(N, **io)
    # an interior-point controller needs Z̃
    lin = su.Case("linmpc").controller(lib)
    lin._sim_plant(case.plant)
    with code(-1):
        lin.hd.sim(N, **{**io, "Ztilde": None})
    # Python: the plant shares the controller's operating points; shapes
    kw = case.args()
    n, ry, d, ru = kw.pop("N"), kw.pop("ry"), kw.pop("d"), kw.pop("ru")
    for bad in (dict(kw["plant"], uop=o["uop"] + 1.0), dict(kw["plant"], yop=o["yop"] + 1.0), dict(kw["plant"], dop=o["dop"] + 1.0),
                dict(kw["plant"], Bu=np.zeros((B, nxp, 2))), dict(kw["plant"], C=np.zeros((B, 2, nxp))), dict(kw["plant"], E=1), None,
                (p["A"][:, :2], p["Bu"], p["C"])):
        with pytest.raises(ValueError):
            mpc.sim(n, ry, d, ru, **{**kw, "plant": bad})
    for bad in (dict(x_0=np.zeros(nxp + 1)), dict(u_noise=np.zeros(2)), dict(draws=dict(w_y=np.zeros((B, 1, n + 1)))), dict(draws=dict(w=1))):
        with pytest.raises(ValueError):
            mpc.sim(n, ry, d, ru, **{**kw, **bad})
    with pytest.raises(ValueError):
        mpc.sim(0, ry, d, ru, **kw)
    # seeded draws: the documented order w_d, w_y, w_u, w_x of default_rng(seed), each (B,n,N)
    kw.pop("draws")
    rng = np.random.default_rng(11)
    drawn = {k: rng.standard_normal((B, m, n)) for k, m in (("w_d", 1), ("w_y", 1), ("w_u", 1), ("w_x", nxp))}
    a = su.run(case.controller(lib), N=n, ry=ry, d=d, ru=ru, seed=11, **kw)
    b = su.run(case.controller(lib), N=n, ry=ry, d=d, ru=ru, draws=drawn, **kw)
    assert su.same_records(a, b) == []


def test_refusals_and_seeded_draws(lib):
    check_refusals(lib)


def test_stock_emulator_has_no_plant_kernel():
    """A library without the launcher of csrc/sim_launch.h refuses the plant: no quiet fall-back."""
    from tests import emu_util
    stock = mpcqp.api.load_library(emu_util.build())
    hd = mpcqp.Handle(2, 2, 1, 1, 0, 3, 1, neps=0, lib=stock)
    with pytest.raises(mpcqp.MpcqpError, match="error -4:"):
        hd.sim_set_plant(np.zeros((2, 2, 2)), np.zeros((2, 1, 2)), np.zeros((2, 2, 1)))


def test_host_code_under_sanitizers(tmp_path):
    """The simulation entry points in a stand-alone program under the address and undefined-behaviour sanitizers, linked against
    the emulator objects like tests/explicit_asan_main.cpp; nothing is loaded into python."""
    su.build()
    exe = str(tmp_path / "sim_asan")
    subprocess.check_call(su.SANITIZER_CXX + ["-x", "c++", os.path.join(su.CSRC, "mpcqp_host.hip"),
                                              os.path.join(su.ROOT, "tests", "sim_asan_main.cpp"), "-x", "none"]
                          + su.SANITIZER_OBJS + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "sim sanitizer run: ok" in out.stdout, out.stdout + out.stderr
