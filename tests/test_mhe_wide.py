"""The wide MovingHorizonEstimator kernels (16 < max(nx̂, nym) <= 32, one estimator per wavefront) on the CPU: the bodies of
csrc/mhe_bodies.h with the 64-lane geometry, the plain-loop side of the staged products and the host's lane-stride handling,
run on the emulator library with the estimator launchers (tests/emu/libmpcqp_emu_est.so: the stock objects +
tests/emu/emu_mhe_wide.cpp and the Kalman-filter launchers) against oracle/mhe.py.  The stock emulator library has no wide launchers and keeps refusing such handles (tests/test_mhe.py).  The
GPU tests are in test_gpu_mhe_wide.py."""
import json
import os
import subprocess
import sys

import pytest

import mpcqp
from mpcqp import mhe as pm
from mpcqp import synth
from tests import emu_util
from tests import mhe_wide_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.slow
CASES = ["xhat17", "soft20", "what+vhat18"]


@pytest.fixture(scope="module")
def widelib_path():
    return emu_util.build(emu_util.EST)


@pytest.fixture(scope="module")
def forward(widelib_path):
    return wu.emulator_cases(mpcqp.api.load_library(widelib_path))


@pytest.fixture(scope="module")
def reverse(widelib_path):
    """The same cases with the fibers playing the lanes in reverse order (a missing sync between a lane's write and
    another lane's read shows in one of the two orders), in a child process: the order is read when a wavefront starts."""
    env = dict(os.environ, MPCQP_EMU_LANE_ORDER="reverse")
    out = subprocess.run([sys.executable, "-m", "tests.mhe_wide_util", widelib_path], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])


def _check(r, soft):
    assert r["ok"], r
    assert r["lanes"] == 64 and r["NX"] == 24, r
    assert r["ex"] <= wu.TOL and r["ew"] <= wu.TOL and r["ep"] <= 1e-12, r
    assert r["iters"] > 5, r                               # a real QP, not one Newton step
    if soft:
        assert r["ee"] <= wu.TOL * max(1.0, r["eps"]) and r["eps"] > 1e-3, r


@pytest.mark.parametrize("case", CASES)
def test_wide_cases_on_emulator_match_oracle(forward, case):
    _check(forward[case], case == "soft20")


@pytest.mark.parametrize("case", CASES)
def test_wide_cases_on_emulator_reverse_lane_order(reverse, forward, case):
    _check(reverse[case], case == "soft20")
    # the lane order changes which fiber runs first, not the arithmetic of a lane
    assert reverse[case]["ex"] == forward[case]["ex"] and reverse[case]["iters"] == forward[case]["iters"]


def test_wide_library_limits(widelib_path):
    lib = mpcqp.api.load_library(widelib_path)
    for kw in (dict(nx=30, nym=3), dict(nx=1, nym=33)):    # nx̂ = 33; nym = 33
        cfg = synth.MheConfig("big", nu=1, nd=0, He=2, **kw)
        bt = synth.make_mhe_batch(cfg, 1, seed=0)
        with pytest.raises(mpcqp.MpcqpError, match="not supported"):
            pm.BatchMHE(bt["Ahat"], bt["Bhu"], bt["Chm"], He=2, lib=lib)
    cfg = synth.MheConfig("edge", nx=14, nu=1, nym=2, nd=0, He=2)
    bt = synth.make_mhe_batch(cfg, 1, seed=0)
    bm = pm.BatchMHE(bt["Ahat"], bt["Bhu"], bt["Chm"], He=2, lib=lib)
    assert bm.handle.lanes_per_estimator() == 16 and bm.handle.register_columns() == 16
