"""E'w of the one-wavefront step kernel with nu = ny = 4 on its 16 x 4 lane map (csrc/mpcqp_bodies.h, Et_apply_share_):
lane (li, lk) multiplies ONE Toeplitz operand per horizon step into one accumulator per 16-column tile, the four Σ-row
partials of a column are added across the 16-lane rows and lane k keeps column k.

Shapes (Hc, Hp) at which that map can go wrong: half a tile column (Hc = 2: fewer than three zero blocks in front of the
table, the shape stays on the earlier form), exactly one tile column, a ragged second one, C3 itself, the ϵ row on lane
60, nDU = 64 without an idle lane -- and one nu = 2 shape, which must stay on the general form.  Every shape with a soft
ymax (the ϵ row, and with it the call that stops at a step t_hi < Hp) and with hard input bounds only; B = 64.

  * q̃ = 2 E'(M (F - r)) .. read back through MPCQP_GET_QTILDE against oracle/condense at 1e-11: E'w alone;
  * one cold and one warm step (shifted start) against the oracle's C port at the suite's tolerance.
"""
import dataclasses

import numpy as np
import pytest

import mpcqp
from mpcqp import synth
from tests.parity_util import make_controller, make_oracle, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5            # tests/test_gpu_parity.py
B = 64

# (nx, nu, ny, Hp, Hc)
SHAPES = {
    "half_tile": (6, 4, 4, 2, 2),
    "one_tile": (6, 4, 4, 5, 4),
    "ragged_second_tile": (6, 4, 4, 9, 5),
    "C3": (12, 4, 4, 30, 10),
    "eps_on_lane_60": (8, 4, 4, 15, 15),
    "nDU_64": (8, 4, 4, 17, 16),
    "nu_2": (6, 2, 4, 12, 6),
}
CASES = [(s, "soft") for s in SHAPES if s != "nDU_64"] + [(s, "hard") for s in SHAPES if s != "nu_2"]


def config(shape, pattern):
    nx, nu, ny, Hp, Hc = SHAPES[shape]
    cfg = synth.get_config(f"{nx},{nu},{ny},{Hp},{Hc}")       # C3's pattern: soft ymax, hard umin / umax
    if pattern == "hard":
        cfg = dataclasses.replace(cfg, ymax=np.inf, Cwt=np.inf)
    return cfg


@pytest.mark.parametrize("shape,pattern", CASES)
def test_etw_lane_map(shape, pattern, hiplib):
    from oracle import cport
    cfg = config(shape, pattern)
    nDU = cfg.nu * cfg.Hc
    assert nDU + (0 if np.isinf(cfg.Cwt) else 1) <= 64
    bt = synth.make_batch(cfg, B, seed=5)
    # (keep_qp: q̃ stays readable, and the steps of the small shapes run on the one-controller-per-wavefront kernel too)
    mpc = make_controller(cfg, bt, keep_qp=True)
    mpc.lastu0 = bt["lastu0"].copy()
    ref = cport.from_synth(cfg, bt)

    # cold step
    u1 = mpc.moveinput(bt["xhat0"], bt["ry"]).copy()
    assert mpc.hd.kernel_kind() in (mpcqp.api.KERNEL_AOT, mpcqp.api.KERNEL_ONDEMAND)
    assert np.all(mpc.status == mpcqp.STATUS_OPTIMAL), np.unique(mpc.status, return_counts=True)
    q = mpc.hd.get(mpcqp.GET_QTILDE)
    eq = 0.0
    for i in range(0, B, 7):
        m = make_oracle(cfg, bt, i)
        m.initpred(bt["xhat0"][i], bt["lastu0"][i], bt["ry"][i])
        eq = max(eq, np.abs(q[i] - m.qt).max() / max(1.0, np.abs(m.qt).max()))
    Zc, _, stc, _ = ref.step(bt["xhat0"], bt["lastu0"], bt["ry"])
    assert np.all(stc == 0)
    e1 = rel_err(mpc.Z, Zc, nDU).max()

    # warm step: both from their own shifted optimum, on the trajectory of the kernel's first move
    x1 = np.einsum("bij,bj->bi", bt["Ahat"], bt["xhat0"]) + np.einsum("bij,bj->bi", bt["Bhu"], u1)
    mpc.moveinput(x1, bt["ry"])
    assert np.all(mpc.status == mpcqp.STATUS_OPTIMAL), np.unique(mpc.status, return_counts=True)
    Zw, _, stw, _ = ref.step(x1, u1, bt["ry"], Z=Zc.copy(), cold=False)
    assert np.all(stw == 0)
    e2 = rel_err(mpc.Z, Zw, nDU).max()
    print(f"[etw] {shape}/{pattern}: kind {mpc.hd.kernel_kind()} q̃ err {eq:.2e} cold {e1:.2e} warm {e2:.2e}")
    assert eq <= 1e-11, eq
    assert e1 <= TOL, e1
    assert e2 <= TOL, e2
