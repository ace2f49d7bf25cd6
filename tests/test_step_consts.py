"""The per-handle block of step constants (Model::stepc, csrc/mpcqp_host.hip: ensure_stepc / invalidate_stepc) and the
set-up's load phase (csrc/mpcqp_bodies.h: SetupLoads).

The block holds, per controller and (move-blocking interval, input channel), the tightest U0min / U0max of the interval and
the interval's sum of the L weights -- values a step used to form itself, in the same operation order.  So a step's results
do not change by a bit, whether the handle carries the block or not, and a STALE block is the one thing that can go wrong:
every setter that writes one of the block's inputs has to drop it.  The tests therefore compare, array by array and bit by
bit (np.array_equal), a handle that is updated setter by setter and stepped after every update with a fresh handle that
was given the same data from the start -- on the ahead-of-time C3 kernel (default and non-default move blocking), the
runtime-dimension kernel, a team kernel, and the CPU emulator, which links without the block's kernel and so pins the path
that forms the values inside the step.  Handle.step_consts_builds() counts the launches of the block's kernel: every GPU case
asserts that the block was built exactly once per change (so the comparison is of the path WITH the block), the emulator
case that it never was.

The data make a stale block visible: U0min / U0max vary over the horizon so that the tightest bound of the last interval
is not its first step, and L is non-zero and different for every step and channel (so the sums and the q~ loop matter).
B = 64 on the GPU; the emulator, which plays the 64 lanes of one wavefront on the host, runs 6 controllers."""
import glob
import os
import subprocess

import numpy as np
import pytest

import mpcqp
from mpcqp import synth
from oracle import condense as cd, qp
from tests import emu_util
from tests import team_util as tu

B = 64
TOL = 1e-5          # the oracle tolerance of tests/test_gpu_parity.py (relative dU error of a solve)
OUT = ("Z", "u0", "status", "iters", "Yhat")


def make_data(cfg, nb, seed, pattern="c3", B=B):
    """Models, weights, bounds and step inputs of B controllers; `pattern`: which bounds exist (row groups)."""
    rg = np.random.default_rng(seed)
    bt = synth.make_batch(cfg, B, seed=seed)
    nU, nY, nDU = cfg.nu * cfg.Hp, cfg.ny * cfg.Hp, cfg.nu * len(nb)
    jl = np.concatenate([[0], np.cumsum(nb)])
    # bounds that tighten towards the END of the horizon (plus noise): the tightest step of every interval of more than
    # one step is not its first one
    ramp = np.repeat(np.linspace(0.0, 0.25, cfg.Hp), cfg.nu)[None, :]
    umax = 0.9 - ramp + 0.02 * rg.random((B, nU))
    umin = -0.9 + ramp - 0.02 * rg.random((B, nU))
    if nb[-1] > 1:            # (the team case has Hc = Hp: every interval is one step)
        last = slice(jl[-2] * cfg.nu, nU)
        assert np.all(np.argmin(umax[:, last].reshape(B, -1, cfg.nu), axis=1) > 0)
        assert np.all(np.argmax(umin[:, last].reshape(B, -1, cfg.nu), axis=1) > 0)
    d = dict(A=mpcqp.colmajor(bt["Ahat"]), Bu=mpcqp.colmajor(bt["Bhu"]), C=mpcqp.colmajor(bt["Chat"]),
             Md=cfg.Mwt * (1.0 + 0.3 * rg.random((B, nY))), Nd=cfg.Nwt * (1.0 + 0.3 * rg.random((B, nDU))),
             Ld=0.05 + 0.1 * rg.random((B, nU)), Cw=np.full(B, cfg.Cwt),
             bounds=dict(U0min=umin, U0max=umax, Y0max=1.0 + 0.1 * rg.random((B, nY))),
             x=bt["xhat0"], lu=0.1 * bt["lastu0"], ry=bt["ry"],
             Ru=0.05 * rg.standard_normal((B, nU)), raw=bt)
    if pattern == "all":
        d["bounds"].update(Y0min=-1.2 - 0.1 * rg.random((B, nY)), DUmin=np.full((B, nDU), -0.4), DUmax=np.full((B, nDU), 0.4))
    assert len(np.unique(d["Ld"])) == d["Ld"].size
    return d


def new_handle(cfg, nb, lib, model, weights, bounds, flags=mpcqp.FLAG_RY_CONSTANT):
    B = model["x"].shape[0]
    default = list(nb) == [1] * (len(nb) - 1) + [cfg.Hp - len(nb) + 1]
    hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, len(nb), nb=None if default else list(nb), neps=1, flags=flags, lib=lib)
    hd.set_model(model["A"], model["Bu"], model["C"])
    hd.set_weights(weights["Md"], weights["Nd"], weights["Ld"], weights["Cw"])
    hd.set_bounds(**bounds["bounds"])
    return hd


def step(hd, inp, Zin, Ru=None):
    Z = Zin.copy()
    u0, st, it, yh = hd.step(inp["x"], inp["lu"], inp["ry"], Z, Ru=Ru, want_Yhat=True)
    return dict(Z=Z, u0=u0, status=st, iters=it, Yhat=yh)


def assert_same(a, b, what):
    for k in OUT:
        assert np.array_equal(a[k], b[k]), (what, k, np.argwhere(a[k] != b[k])[:3].tolist())


def fresh_versus_updated(cfg, nb, lib, prepare=None, kind=None, pattern="c3", Ru=False, flags=mpcqp.FLAG_RY_CONSTANT, B=B,
                         block=True):
    """Step; then change only the bounds, only the weights, only the model, stepping after each change: every output of
    every step equals that of a fresh handle that had the same data from the start.  Returns the last fresh result and
    its data.  (Warm start: every step gets the same previous Z~, so the only state a handle carries is the block.)
    `block`: the library has the block's kernel -- it then ran once per change, and once for a fresh handle."""
    d0, d1 = make_data(cfg, nb, 1, pattern, B), make_data(cfg, nb, 2, pattern, B)
    Zprev = 0.01 * np.random.default_rng(5).standard_normal((B, cfg.nu * len(nb) + 1))
    upd = new_handle(cfg, nb, lib, d0, d0, d0, flags)
    if prepare:
        prepare(upd)
    if kind is not None:
        assert upd.kernel_kind() == kind, upd.kernel_kind()
    stages = [("initial", d0, d0, d0), ("bounds", d0, d0, d1), ("weights", d0, d1, d1), ("model", d1, d1, d1)]
    last = None
    for n, (name, model, weights, bounds) in enumerate(stages):
        if name == "bounds":
            upd.set_bounds(**bounds["bounds"])
        elif name == "weights":
            upd.set_weights(weights["Md"], weights["Nd"], weights["Ld"], weights["Cw"])
        elif name == "model":
            upd.set_model(model["A"], model["Bu"], model["C"])
        ru = d1["Ru"] if Ru else None
        got = step(upd, d1, Zprev, Ru=ru)
        fresh = new_handle(cfg, nb, lib, model, weights, bounds, flags)
        if prepare:
            prepare(fresh)
        ref = step(fresh, d1, Zprev, Ru=ru)
        assert (upd.step_consts_builds(), fresh.step_consts_builds()) == ((n + 1, 1) if block else (0, 0)), name
        fresh.close()
        assert np.all(ref["status"] == 0), (name, ref["status"])
        assert_same(got, ref, name)
        if last is not None:       # (the data did change something: a test that compares equal things twice proves nothing)
            assert not np.array_equal(last["Z"], ref["Z"]), name
        last = ref
    upd.close()
    return last, d1


C3_NB = [1] * 9 + [21]
C3_BLOCKED = [1, 1, 1, 1, 2, 2, 3, 4, 5, 10]


def _prepare_aot(hd):
    assert hd.prepare() == mpcqp.api.KERNEL_AOT


# ---- 1. staleness on C3's ahead-of-time kernel (default move blocking) and on C3's dimensions with a move-blocking vector
#         (no ahead-of-time kernel has one: without mpcqp_prepare the runtime-dimension kernel takes it, nothing compiles)
@pytest.mark.gpu
def test_updated_handle_equals_fresh_handle_c3(hiplib):
    fresh_versus_updated(synth.C3, C3_NB, hiplib, prepare=_prepare_aot, kind=mpcqp.api.KERNEL_AOT)


@pytest.mark.gpu
def test_updated_handle_equals_fresh_handle_c3_cold_start(hiplib):
    fresh_versus_updated(synth.C3, C3_NB, hiplib, prepare=_prepare_aot, kind=mpcqp.api.KERNEL_AOT,
                         flags=mpcqp.FLAG_RY_CONSTANT | mpcqp.FLAG_COLD_START)


@pytest.mark.gpu
def test_updated_handle_equals_fresh_handle_c3_move_blocking(hiplib):
    assert sum(C3_BLOCKED) == synth.C3.Hp
    fresh_versus_updated(synth.C3, C3_BLOCKED, hiplib, kind=mpcqp.api.KERNEL_GENERIC)


# ---- 2. a per-step R̂u: q~ takes its loop over the horizon while H~ takes the block's sums; against the oracle
def _oracle_Z(cfg, nb, d, i, Ru):
    bt = d["raw"]
    nu, ny, Hp = cfg.nu, cfg.ny, cfg.Hp
    m = cd.LinMPCOracle(bt["Ahat"][i], bt["Bhu"][i], bt["Chat"][i], Hp=Hp, Hc=list(nb), Cwt=cfg.Cwt,
                        M_Hp=np.diag(d["Md"][i]), N_Hc=np.diag(d["Nd"][i]), L_Hp=np.diag(d["Ld"][i]))
    bd = d["bounds"]
    m.setconstraint(Umin=bd["U0min"][i], Umax=bd["U0max"][i], Ymax=bd["Y0max"][i])
    m.initpred(d["x"][i], d["lu"][i], d["ry"][i], Rhatu=Ru[i])
    m.linconstraint()
    z, st = qp.solve_qp(*m.qp_data(), m.warmstart())[:2]
    return z


@pytest.mark.gpu
def test_per_step_Ru_with_the_block_matches_the_oracle(hiplib):
    cfg = synth.C3
    got, d = fresh_versus_updated(cfg, C3_NB, hiplib, prepare=_prepare_aot, kind=mpcqp.api.KERNEL_AOT, Ru=True)
    nDU = cfg.nu * cfg.Hc
    for i in (0, 17, 63):
        z = _oracle_Z(cfg, C3_NB, d, i, d["Ru"])
        err = np.max(np.abs(got["Z"][i, :nDU] - z[:nDU])) / max(1.0, np.max(np.abs(z[:nDU])))
        print(f"[step_consts] R̂u case, member {i}: relative dU error vs oracle {err:.3e}")
        assert err <= TOL, (i, err)


# ---- 3. the runtime-dimension kernel: a shape with 16 < nZ~ <= 64 outside the ahead-of-time list, never prepared
@pytest.mark.gpu
def test_updated_handle_equals_fresh_handle_runtime_dims(hiplib):
    cfg = synth.Config("rt-consts", nx=5, nu=3, ny=2, Hp=13, Hc=7, umin=-0.9, umax=0.9, ymax=1.0)
    nb = [1, 2, 1, 1, 3, 1, 4]
    assert 16 < cfg.nu * len(nb) + 1 <= 64 and sum(nb) == cfg.Hp
    fresh_versus_updated(cfg, nb, hiplib, kind=mpcqp.api.KERNEL_GENERIC)


# ---- 3b. the setters of dense and block weights drop the block as well.  A dense L_Hp is the case a stale block would get
#          wrong in silence: the handle then carries NO block (the step sums the dense L itself), and gets one again when
#          the diagonal comes back
@pytest.mark.gpu
def test_dense_and_block_weight_setters_drop_the_block(hiplib):
    cfg, nb = synth.C3, C3_NB
    d = make_data(cfg, nb, 1)
    rg = np.random.default_rng(9)
    nU, nY = cfg.nu * cfg.Hp, cfg.ny * cfg.Hp
    S = 0.01 * rg.random((B, nU, nU))
    Ldense = np.einsum("bi,ij->bij", d["Ld"], np.eye(nU)) + S + S.transpose(0, 2, 1)
    T = 0.05 * cfg.Mwt * rg.random((B, cfg.Hp, cfg.ny, cfg.ny))
    Mblk = np.einsum("bti,ij->btij", d["Md"].reshape(B, cfg.Hp, cfg.ny), np.eye(cfg.ny)) + T + T.transpose(0, 1, 3, 2)
    Zprev = 0.01 * rg.standard_normal((B, cfg.nu * len(nb) + 1))
    stages = [("diagonal", lambda h: None, 1), ("dense L", lambda h: h.set_dense_weights(L_Hp=Ldense), 0),
              ("diagonal again", lambda h: h.set_dense_weights(), 1), ("block M", lambda h: h.set_output_weight_blocks(Mblk), 1)]
    upd, builds, last = new_handle(cfg, nb, hiplib, d, d, d), 0, None
    for name, change, built in stages:
        change(upd)
        got = step(upd, d, Zprev)
        builds += built
        fresh = new_handle(cfg, nb, hiplib, d, d, d)
        change(fresh)
        ref = step(fresh, d, Zprev)
        assert (upd.step_consts_builds(), fresh.step_consts_builds()) == (builds, built), name
        fresh.close()
        assert np.all(ref["status"] == 0), (name, ref["status"])
        assert_same(got, ref, name)
        if last is not None:
            assert not np.array_equal(last["Z"], ref["Z"]), name
        last = ref
    upd.close()


# ---- 4. a team kernel: nZ~ = 71 at T = 2, from the object tests/test_gpu_team.py builds -- under MPCQP_TEAM_TEST_CACHE when
#         that is set, else in the temporary directory of this pytest session (tests/test_gpu_team.py runs before this file)
def _team_cache(tmp_path_factory):
    root = os.environ.get("MPCQP_TEAM_TEST_CACHE")
    roots = [root] if root else sorted(glob.glob(os.path.join(str(tmp_path_factory.getbasetemp()), "team_cache*")))
    for r in roots:
        cache = os.path.join(r, "plain71_T2")
        if tu.spec_objects(cache):
            return cache
    return None


@pytest.mark.gpu
def test_updated_handle_equals_fresh_handle_team_of_two(hiplib, monkeypatch, tmp_path, tmp_path_factory):
    cache = _team_cache(tmp_path_factory)
    if not cache:
        pytest.skip("no plain71 specialisation at T = 2: tests/test_gpu_team.py has not run in this session and "
                    "MPCQP_TEAM_TEST_CACHE names no directory that holds one")
    assert tu.team_of_symbols(tu.kernel_symbols(tu.spec_objects(cache)[0], str(tmp_path / "syms"))) == 2
    monkeypatch.setenv("MPCQP_CACHE_DIR", cache)
    cfg = tu.plain_config("plain71")
    assert cfg.nu * cfg.Hc + 1 == 71

    def prepare(hd):
        assert hd.prepare() == mpcqp.api.KERNEL_ONDEMAND

    fresh_versus_updated(cfg, [1] * cfg.Hc, hiplib, prepare=prepare, kind=mpcqp.api.KERNEL_ONDEMAND)


# ---- 5. the CPU emulator: linked without the block's kernel, the handle never carries the block
@pytest.fixture(scope="module")
def emulib():
    lib = mpcqp.api.load_library(emu_util.build())
    yield lib
    mpcqp.api._lib = None


@pytest.mark.slow
def test_updated_handle_equals_fresh_handle_on_cpu_emulator(emulib):
    syms = subprocess.run(["nm", "-D", "--defined-only", emu_util.build()],
                          capture_output=True, text=True).stdout
    assert "launch_step_consts" not in syms         # the emulator keeps the path that forms the values inside the step
    fresh_versus_updated(synth.C3, C3_NB, emulib, B=6, block=False)
