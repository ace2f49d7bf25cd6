"""Custom linear constraints (Wy, Wu, Wd, Wr; construct.jl:1138-1160, execute.jl:337-364) on the stage-structured
MultipleShooting kernel (csrc/ms_bodies.h), without a GPU: the kernel body on the CPU wave emulator against the condensed
oracle (both transcriptions solve the same QP).  The GPU runs are in tests/test_gpu_ms_custom.py."""

import numpy as np
import pytest

import mpcqp
from mpcqp import api
from oracle import condense as cd
from tests import emu_util
from tests import ms_custom_util as mcu

TOL = 1e-5


@pytest.fixture(scope="module")
def emulib():
    return api.load_library(emu_util.build())


def test_t9_under_multiple_shooting_runs_on_the_stage_kernel(emulib):
    """T9 (test/3_test_predictive_control.jl:466-495: Wy; Wu; Wd + Wy; Wr + Wy) with transcription=MultipleShooting at
    Hp = 12: no reason mask, the stage-structured kernel, no fallback warning; ΔU and W as the condensed oracle's; the
    returned X̂0 is the model rolled out from the returned ΔU."""
    r = mcu.run_t9(lib=emulib, B=2, Hp=12)
    assert all(w == 0 for w in r["whys"]), r["whys"]
    assert all(k == api.KERNEL_MS for k in r["kinds"]), r["kinds"]
    assert r["worst"] <= TOL, r
    assert r["defect"] <= 1e-9 and r["xroll"] <= 1e-9, r


@pytest.mark.parametrize("Cwt", [1e5, np.inf])
@pytest.mark.parametrize("no_polish", [False, True])
def test_soft_custom_rows_closed_loop_on_the_stage_kernel(emulib, Cwt, no_polish):
    """Two custom rows mixing ŷ, u, d and r̂ on top of u / y bounds, move blocking [1, 2, 2] over Hp = 8 (steps without a free
    move, and rows at j = Hp): three closed-loop periods against the condensed oracle, with the slack (finite Cwt, soft
    rows) and without (hard rows), with the active-set polish and without it; a custom row is active at the optimum."""
    r = mcu.run_soft_custom(lib=emulib, B=2, Cwt=Cwt, no_polish=no_polish)
    assert all(k == api.KERNEL_MS for k in r["kinds"]) and all(w == 0 for w in r["whys"]), r
    assert r["worst"] <= TOL, r
    assert r["active"] <= 1e-6, r
    assert r["defect"] <= 1e-9 and r["xroll"] <= 1e-9, r
    if np.isfinite(Cwt):
        assert max(r["eps"]) > 1e-6          # (the slack is in play)


def test_reason_masks_compose_with_custom_rows(emulib):
    """A dense M_Hp together with custom rows: reason mask 1 (dense weights) only -- custom rows no longer add 2."""
    rng = np.random.default_rng(5)
    nx, nu, ny, Hp = 3, 2, 2, 6
    A = np.diag([0.8, 0.5, 0.3]); Bu, C = rng.standard_normal((nx, nu)), rng.standard_normal((ny, nx))
    M = np.kron(np.eye(Hp), np.array([[2.0, 0.3], [0.3, 1.0]]))
    M[0, 3] = M[3, 0] = 0.2
    kw = dict(Hp=Hp, Hc=2, M_Hp=M, Nwt=[0.1, 0.1], Wy=[[1.0, 0.5]], Wu=[[0.2, -0.3]])
    g = mpcqp.BatchLinMPC(mcu.rep(A, 2), mcu.rep(Bu, 2), mcu.rep(C, 2), transcription="MultipleShooting", lib=emulib, **kw)
    g.setconstraint(wmax=[0.7])
    with pytest.warns(RuntimeWarning, match=r"reason mask 1:"):
        g.moveinput(np.zeros((2, nx)), [0.5, 0.5])
    g.hd.set_transcription(api.MULTIPLE_SHOOTING)
    assert g.hd.transcription_supported() == 1
    o = cd.LinMPCOracle(A, Bu, C, **kw)
    o.setconstraint(wmax=[0.7])
    o.moveinput(np.zeros(nx), [0.5, 0.5])
    assert np.abs(g.Z[0, :o.nDU] - o.Zt[:o.nDU]).max() <= TOL


def test_custom_rows_without_bounds_keep_the_stage_kernel(emulib):
    """Custom rows declared but left at ±Inf: the stage kernel with the rows compiled in has no finite custom row, and the
    result equals the controller without custom rows."""
    rng = np.random.default_rng(2)
    A = np.diag([0.9, 0.4]); Bu, C = rng.standard_normal((2, 1)), rng.standard_normal((1, 2))
    kw = dict(Hp=7, Hc=3, Nwt=[0.1])
    out = []
    for extra in ({}, dict(Wy=[[1.0]])):
        g = mpcqp.BatchLinMPC(mcu.rep(A, 2), mcu.rep(Bu, 2), mcu.rep(C, 2), transcription="MultipleShooting", lib=emulib,
                              **kw, **extra)
        g.setconstraint(umin=[-0.4], umax=[0.4])
        mcu.no_fallback_step(g, np.tile([0.5, -0.2], (2, 1)), [1.0])
        assert g.kernel == api.KERNEL_MS and np.all(g.status == 0)
        out.append(g.Z.copy())
    assert np.abs(out[0] - out[1]).max() <= 1e-9


@pytest.mark.slow
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_custom_families_on_the_emulator(emulib, seed):
    """Randomised families with custom rows (nd > 0 with a varying preview, ±Inf holes, soft / hard rows, move blocking)
    under MultipleShooting against the condensed oracle."""
    r = mcu.random_custom_family(seed, lib=emulib, B=2)
    assert r["kind"] == api.KERNEL_MS and r["why"] == 0 and np.all(r["status"] == 0), r
    assert r["worst"] <= TOL, r
    assert r["defect"] <= 1e-9, r


def test_fused_loop_with_custom_rows_on_the_emulator(emulib):
    """mpcqp_loop_device equals the three separate entry points bit for bit on a MultipleShooting handle with custom rows."""
    assert mcu.fused_loop_custom(lib=emulib) == 0.0
