"""CPU tests of the Luenberger observer built from its poles (mpcqp_kf_set_poles): the placement body of
csrc/kf_place_bodies.h on the CPU wave emulator (tests/emu/emu_kf_place.cpp) through the C-ABI and the BatchLinMPC mirror, with
the checks of tests/kf_place_util.py, and the host code under the address and undefined-behaviour sanitizers in a stand-alone
program.  The GPU tests are in tests/test_gpu_kf_place.py."""
import os
import subprocess

import numpy as np
import pytest

import mpcqp
from tests import emu_util
from tests import kf_place_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda cases: ["n%d-m%d-B%d" % c[:3] for c in cases]


@pytest.fixture(scope="module")
def placelib():
    lib = mpcqp.api.load_library(pu.build())
    yield lib
    mpcqp.api._lib = None


def test_restatement_sets_tau():
    """The NumPy restatement places the poles of every input of the tests; its largest Bauer-Fike ratio, times 8, is TAU."""
    worst = 0.0
    for case in pu.all_pole_cases():
        ref = pu.place_ref(case)
        assert not ref["status"].any()
        ratio, lhs, _ = pu.worst_ratio(case, ref["K"])
        print((case["n"], case["m"], case["B"]), "ratio %.3g, max |eig - p| = %.3g, sweeps %s" % (ratio, lhs, ref["sweeps"].tolist()))
        worst = max(worst, ratio)
    print("largest ratio", worst, "TAU", pu.TAU)
    assert 8.0 * worst <= pu.TAU <= 8.0 * worst * 1.05


@pytest.mark.parametrize("spec", pu.SWEEP_CASES, ids=ids(pu.SWEEP_CASES))
def test_restatement_sweeps_improve_conditioning(spec):
    """The seeds of the sweep test: cond X at cap 0 at least 4 times cond X at cap 30 for every member."""
    case, c0, c30 = pu.sweep_refs(spec)
    print("ratios", (c0 / c30).tolist())
    assert (c0 >= 4.0 * c30).all()
    # ... and the restatement itself is on the right side of c* at both caps, by a margin
    cstar = np.sqrt(c0 * c30)
    v0, v30 = pu.condV(case, pu._sweep_refs[spec][1]["K"]), pu.condV(case, pu._sweep_refs[spec][2]["K"])
    print("cond V / c* at cap 30", (v30 / cstar).tolist(), "at cap 0", (v0 / cstar).tolist())
    assert (1.5 * v30 < cstar).all() and (v0 > 1.5 * cstar).all()


@pytest.mark.slow
@pytest.mark.parametrize("shape", pu.CASES, ids=ids(pu.CASES))
def test_emulator_poles_are_placed(placelib, shape):
    pu.check_placed(pu.make_case(*shape), lib=placelib)


@pytest.mark.slow
def test_emulator_closed_form(placelib):
    pu.check_closed_form(lib=placelib)


@pytest.mark.slow
@pytest.mark.parametrize("spec", pu.SWEEP_CASES, ids=ids(pu.SWEEP_CASES))
def test_emulator_sweeps_do_their_work(placelib, spec):
    pu.check_sweeps(spec, lib=placelib)


@pytest.mark.slow
@pytest.mark.parametrize("shape", pu.DEFAULT_POLE_CASES, ids=ids(pu.DEFAULT_POLE_CASES))
def test_emulator_reference_default_poles(placelib, shape):
    n, m, B = shape
    pu.check_placed(pu.make_case(n, m, B, poles=pu.default_poles(n)), lib=placelib)


@pytest.mark.slow
def test_emulator_repeated_poles(placelib):
    pu.check_placed(pu.make_case(**pu.REPEATED), lib=placelib)


@pytest.mark.slow
def test_emulator_refusals_stay_inside_their_member(placelib):
    pu.check_refusals(lib=placelib)


@pytest.mark.slow
def test_emulator_contract(placelib):
    pu.check_contract(lib=placelib)


@pytest.mark.slow
def test_refused_beyond_32_states(placelib):
    case = pu.make_case(33, 1, 2, poles=np.linspace(0.1, 0.8, 33))
    h = pu.make_handle(case, lib=placelib, place=False)
    pu.refused_then_kf_set(h, case)


def test_stock_emulator_refuses_the_placement():
    """A library without the launcher links (weak declaration) and answers MPCQP_ERR_UNSUPPORTED; a kf_set gain still works."""
    lib = mpcqp.api.load_library(emu_util.build())
    try:
        case = pu.make_case(4, 2, 2)
        pu.refused_then_kf_set(pu.make_handle(case, lib=lib, place=False), case)
    finally:
        mpcqp.api._lib = None


@pytest.mark.slow
@pytest.mark.parametrize("direct", [True, False], ids=["direct", "predictor"])
def test_emulator_controller(placelib, direct):
    """luenberger=dict(poles) against the same controller given the gain: the methods, sim and hd.loop_device, bit for bit."""
    pu.check_controller(direct, lib=placelib)


@pytest.mark.slow
def test_emulator_observer_error(placelib):
    pu.check_observer_error(lib=placelib)


@pytest.mark.slow
def test_emulator_setmodel_and_warning(placelib):
    pu.check_setmodel_and_warning(lib=placelib)


def test_mirror_validates_before_any_device_call():
    """BatchLinMPC.setestimator(luenberger=...): exclusive with the other estimator keywords, pole checks, and a handle
    without mpcqp_kf_set_poles -- all before anything is sent to the device."""
    class Recorder:
        calls = []
        def kf_set_poles(self, *a): self.calls.append(a)
        def kf_status(self): return np.zeros(2, np.int32)
    mpc = mpcqp.BatchLinMPC.__new__(mpcqp.BatchLinMPC)
    mpc.B, mpc.nxh, mpc.ny, mpc.nu, mpc.nd = 2, 3, 2, 1, 0
    mpc.xhop = np.zeros((2, 3))
    mpc.hd = Recorder()
    lu = dict(poles=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        mpc.setestimator(np.zeros((2, 3, 1)), luenberger=lu)
    with pytest.raises(ValueError):
        mpc.setestimator(luenberger=lu, steady=dict(Qhat=np.eye(3), Rhat=np.eye(1)))
    with pytest.raises(ValueError):
        mpc.setestimator(luenberger=lu, covariances=dict(Qhat=np.eye(3), Rhat=np.eye(1), P0=np.eye(3)))
    with pytest.raises(ValueError):
        mpc.setestimator(luenberger=lu, internal=dict())
    with pytest.raises(NotImplementedError):
        mpc.setestimator(luenberger=dict(poles=[0.1, 0.2 + 0.1j, 0.2 - 0.1j]))
    for bad in ([0.1, 0.2], [0.1, 0.2, 0.3, 0.4], np.full((3, 3), 0.1)):
        with pytest.raises(ValueError, match="poles length"):
            mpc.setestimator(luenberger=dict(poles=bad))
    for bad in ([0.1, 0.2, 1.0], [0.1, -1.2, 0.3], [0.1, np.nan, 0.3]):
        with pytest.raises(ValueError, match="inside the unit circle"):
            mpc.setestimator(luenberger=dict(poles=bad))
    with pytest.raises(ValueError, match="i_ym"):
        mpc.setestimator(luenberger=lu, i_ym=[0, 0])
    assert not Recorder.calls
    mpc.setestimator(luenberger=lu, i_ym=[1], xhat0=[1.0, 2.0, 3.0])
    assert mpc.kf_luenberger and not mpc.kf_steady and not mpc.kf_timevarying
    assert Recorder.calls[0][0].shape == (2, 3) and mpc.xhat0.shape == (2, 3)
    mpc.setestimator(luenberger=dict(), i_ym=[1])
    assert np.array_equal(Recorder.calls[1][0][0], 1e-3 * np.arange(1, 4) + 0.5)
    with pytest.raises(ValueError, match="covariance"):
        mpc.setstate(np.zeros(3), np.eye(3))
    mpc.hd = object()
    with pytest.raises(NotImplementedError):
        mpc.setestimator(luenberger=lu, i_ym=[1])


def test_host_code_under_sanitizers(tmp_path):
    """csrc/mpcqp_host.hip compiled for the host with -fsanitize=address,undefined into tests/kf_place_asan_main.cpp (its own
    main), with the emulator launcher compiled the same way: set, place again after a model swap, the read-backs, the
    refusals, handle destroyed.  No sanitizer goes into Python."""
    emu_util.build(emu_util.EST)
    exe = str(tmp_path / "kf_place_asan")
    subprocess.check_call(emu_util.SANITIZER_CXX + ["-x", "c++", os.path.join(emu_util.CSRC, "mpcqp_host.hip"),
                                                    os.path.join(emu_util.EMU, "emu_kf_place.cpp"),
                                                    os.path.join(ROOT, "tests", "kf_place_asan_main.cpp"), "-x", "none"]
                          + emu_util.SANITIZER_OBJS + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "kf place asan ok" in out.stdout, out.stdout + out.stderr
