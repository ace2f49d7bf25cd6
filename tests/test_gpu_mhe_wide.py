"""GPU parity of the wide MovingHorizonEstimator kernels (16 < max(nx̂, nym) <= 32: one estimator per wavefront, csrc/
mhe_wide_kernels.hip) against oracle/mhe.py through the C-ABI, with the bars of tests/test_gpu_mhe.py: every register-column
count of the family (24, 32), both forms, growing and moving windows, measured disturbances, every bound class hard and
soft, per channel and window-long, the Kalman-filter identity, and the boundaries to the 16-lane family and to 'not supported'.
Each configuration was run through the oracle alone first (all statuses 0, the named bound active in the listed share of
its solves); the seeds of the randomised families and of the window-long case were chosen that way too."""
import numpy as np
import pytest

import mpcqp
from mpcqp import mhe as pm
from mpcqp import synth
from tests import mhe_util
from tests import mhe_wide_util as wu
from tests.test_gpu_mhe import TOL, _batched_kf, _check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw, NX, bseed, dseed", [
    (dict(nx=14, nu=2, nym=3, nd=0, He=4, xabs=1.2), 24, 5, 5),                                 # nx̂ = 17; x̂ active in 10 of 21 solves
    (dict(nx=16, nu=2, nym=4, nd=1, He=6, xabs=1.2, vabs=0.6, direct=False), 24, 5, 5),         # nx̂ = 20; x̂: 13 of 27
    (dict(nx=20, nu=3, nym=4, nd=0, He=5, wabs=0.03), 24, 7, 0),                                # nx̂ = 24; ŵ: 12 of 21
    (dict(nx=26, nu=2, nym=6, nd=0, He=4, xabs=0.8), 32, 5, 5),                                 # nx̂ = 32; x̂: 8 of 21
    (dict(nx=12, nu=2, nym=20, nd=0, He=3, vabs=0.3), 32, 5, 5),                                # nym > 16: v̂ rows on lanes >= 16; v̂: 10 of 18
], ids=["nxh17", "nxh20+d+vhat predictor", "nxh24 what", "nxh32", "nym20 vhat"])
def test_wide_families_match_oracle(kw, NX, bseed, dseed):
    cfg = synth.MheConfig("wide", **kw)
    bt = synth.make_mhe_batch(cfg, 3, seed=bseed)
    rows, bm = mhe_util.run_periods(cfg, bt, cfg.He + 3, [0, 1, 2], seed=dseed)
    for r in rows:
        print(r["k"], r["Nk"], r["ex"], r["ew"], r["ep"], r["iters"].tolist())
    _check(rows)
    assert bm.handle.lanes_per_estimator() == 64
    assert bm.handle.register_columns() == NX              # max(nx̂, nym) rounded up to a multiple of eight
    assert max(r["iters"].max() for r in rows) > 5         # a real QP, not one Newton step
    assert rows[-1]["Nk"] == cfg.He


def test_wide_soft_constraints_match_oracle():
    """Finite Cwt and softness on x̂ and ŵ rows, nx̂ = 20 with a measured disturbance (oracle: largest ε = 0.0116)."""
    cfg = synth.MheConfig("wsoft", nx=16, nu=2, nym=4, nd=1, He=5, xabs=0.8, wabs=0.15, Cwt=1e4)
    bt = synth.make_mhe_batch(cfg, 3, seed=17)
    bounds = mhe_util.bounds_of(cfg)
    bounds.update({k: np.asarray(v, float) for k, v in wu.SOFT20.items()})
    rows, bm = mhe_util.run_periods(cfg, bt, cfg.He + 2, [0, 1, 2], seed=0, bounds=bounds)
    for r in rows:
        print(r["k"], r["ex"], r["ew"], r["ee"], r["eps"].max())
        assert all(s == 0 for s in r["ostatus"]) and np.all(r["status"] == 0), r
        assert r["ex"] <= TOL and r["ew"] <= TOL and r["ee"] <= TOL * max(1.0, r["eps"].max()), r
    assert max(r["eps"].max() for r in rows) > 1e-3
    assert bm.handle.lanes_per_estimator() == 64


def test_wide_unconstrained_is_the_kalman_filter():
    """nx̂ = 24, predictor form, no bounds, 16 estimators: every estimate equals the time-varying Kalman filter's, to the
    1e-9 of test_config5_batch_unconstrained_is_the_kalman_filter."""
    cfg = synth.MheConfig("wkf", nx=20, nu=2, nym=4, nd=0, He=5, direct=False)
    B = 16
    bt = synth.make_mhe_batch(cfg, B, seed=3)
    nper = cfg.He + 4
    Y, U, D = synth.make_mhe_data(cfg, bt, nper, seed=5)
    bm = mhe_util.make_product(cfg, bt, bounds={}, keep_windows=False)
    ref = _batched_kf(bt, cfg, Y, U, D)
    worst = 0.0
    for k in range(nper):
        bm.preparestate(Y[k])
        xg = bm.updatestate(U[k], Y[k])
        assert np.all(bm.status == 0)
        worst = max(worst, np.abs(xg - ref[k]).max() / max(1.0, np.abs(ref[k]).max()))
    print("worst", worst)
    assert bm.handle.lanes_per_estimator() == 64 and bm.handle.register_columns() == 24
    assert worst <= 1e-9, worst


@pytest.mark.parametrize("csoft", [False, True], ids=["hard", "window-long softness"])
def test_wide_window_long_bounds(csoft):
    """A bound (and a softness) per channel and stage at nx̂ = 20 (oracle alone, seed 21: a stage bound active in 20 of the
    24 (period, estimator) pairs, largest ε of the soft run 1.7e-3)."""
    cfg = synth.MheConfig("wwin", nx=16, nu=1, nym=4, nd=0, He=5, **({"Cwt": 1e4} if csoft else {}))
    eps = []
    ex, ew, active = wu.window_long_bounds(cfg, B=3, seed=21, nper=8, csoft=csoft, eps_seen=eps)
    print(ex, ew, active, max(eps) if eps else None)
    assert active > 0
    if csoft:
        assert max(eps) > 1e-3
    assert ex <= TOL and ew <= TOL, (ex, ew)


def test_wide_heterogeneous_members():
    """Eight estimators of nx̂ = 18 with different bound sets, one of them unbounded (a single Newton step)."""
    cfg = synth.MheConfig("whet", nx=15, nu=2, nym=3, nd=0, He=4)
    B = 8
    bt = synth.make_mhe_batch(cfg, B, seed=11)
    xmax = np.full((B, cfg.nxh), np.inf)
    xmin = np.full((B, cfg.nxh), -np.inf)
    xmax[0] = 0.6; xmin[0] = -0.6
    xmax[2, :2] = 0.3
    xmin[5, 1:] = -0.5
    xmax[7, 16:] = 0.2                                      # rows on lanes >= 16 only
    nper = 7
    Y, U, D = synth.make_mhe_data(cfg, bt, nper, seed=2)
    bm = mhe_util.make_product(cfg, bt, bounds={})
    bm.setconstraint(x̂min=xmin, x̂max=xmax)
    ors = [mhe_util.make_oracles(cfg, bt, [b], bounds=dict(xhatmin=xmin[b], xhatmax=xmax[b]))[0] for b in range(B)]
    for k in range(nper):
        xg = bm.preparestate(Y[k])
        xo = np.array([e.preparestate(Y[k][b]) for b, e in enumerate(ors)])
        assert all(e.status == 0 for e in ors)
        assert np.all(bm.status == 0) and np.abs(xg - xo).max() <= TOL * max(1.0, np.abs(xo).max())
        bm.updatestate(U[k], Y[k])
        for b, e in enumerate(ors):
            e.updatestate(U[k][b], Y[k][b])
    it = bm.getinfo()["iters"]
    assert it[1] == 0 and it[0] > 0                        # the unbounded estimator took its single Newton step
    assert bm.handle.lanes_per_estimator() == 64


@pytest.mark.parametrize("seed", [2, 3, 4, 5, 8, 9])
def test_wide_randomised_families_match_oracle(seed):
    """Random wide dimensions, forms, horizons, bound classes, hard / soft (mhe_wide_util.random_family_wide).  The seeds are
    those whose every window the oracle solves: no member is left out of the comparison."""
    worst, ncmp, nfail, total = wu.random_family_wide(seed)
    print(worst, ncmp, nfail, total)
    assert nfail == 0 and ncmp == total, (ncmp, nfail, total)
    assert worst <= 1e-5, worst                             # north-star tolerance


@pytest.mark.parametrize("kw", [dict(nx=30, nym=3), dict(nx=1, nym=33)], ids=["nxh33", "nym33"])
def test_beyond_32_is_not_supported(kw):
    cfg = synth.MheConfig("big", nu=1, nd=0, He=2, **kw)
    bt = synth.make_mhe_batch(cfg, 1, seed=0)
    with pytest.raises(mpcqp.MpcqpError, match="not supported"):
        pm.BatchMHE(bt["Ahat"], bt["Bhu"], bt["Chm"], He=2)


def test_both_families_in_one_process():
    """nx̂ = 16 stays on the 16-lane rows; a 16-lane handle and a wide one stepped alternately both match the oracle."""
    cn = synth.MheConfig("n16", nx=13, nu=2, nym=3, nd=0, He=4, xabs=1.2)
    cw = synth.MheConfig("w17", nx=14, nu=2, nym=3, nd=0, He=4, xabs=1.2)
    members, nper = [0, 1, 2], 7
    run = []
    for cfg in (cn, cw):
        bt = synth.make_mhe_batch(cfg, 3, seed=5)
        Y, U, D = synth.make_mhe_data(cfg, bt, nper, seed=5)
        run.append((cfg, Y, U, mhe_util.make_product(cfg, bt), mhe_util.make_oracles(cfg, bt, members)))
    assert run[0][3].handle.lanes_per_estimator() == 16 and run[0][3].handle.register_columns() == 16
    assert run[1][3].handle.lanes_per_estimator() == 64 and run[1][3].handle.register_columns() == 24
    for k in range(nper):
        for cfg, Y, U, bm, ors in run:
            xg = bm.preparestate(Y[k])
            xo = np.array([e.preparestate(Y[k][b]) for b, e in zip(members, ors)])
            assert np.all(bm.status == 0) and all(e.status == 0 for e in ors)
            assert np.abs(xg - xo).max() <= TOL * max(1.0, np.abs(xo).max()), (cfg.name, k)
            bm.updatestate(U[k], Y[k])
            for b, e in zip(members, ors):
                e.updatestate(U[k][b], Y[k][b])
