"""Helpers of the wide MovingHorizonEstimator tests (16 < max(nx̂, nym) <= 32, one estimator per wavefront; on the CPU: the
launchers of tests/emu/emu_mhe_wide.cpp in tests/emu/libmpcqp_emu_est.so, tests/emu_util.py): window-long bounds on a given
configuration, randomised wide families, and the cases of tests/test_mhe_wide.py (also runnable in a child
process: `python -m tests.mhe_wide_util <library>` prints them as JSON, which is how the lane orders are compared)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mpcqp  # noqa: E402
from mpcqp import synth  # noqa: E402
from tests import mhe_util  # noqa: E402

TOL = 2e-6          # tests/test_gpu_mhe.py: this interior-point method against the exact active-set optimum


def window_long_bounds(cfg, lib=None, B=3, seed=21, soft=False, nper=9, csoft=False, eps_seen=None, oracle_only=False):
    """mhe_util.window_long_bounds on the configuration `cfg` (that one fixes nx = 3): a bound per channel AND stage, hard, with
    per-channel softness (soft) or window-long softness (csoft; cfg.Cwt must be finite for both).  Returns the worst
    relative errors (x̂, Ŵ) and the number of (period, estimator) pairs with a stage bound active at the oracle's optimum.
    oracle_only: the oracle alone (errors 0), for choosing a seed on the CPU that meets the tests' conditions."""
    bt = synth.make_mhe_batch(cfg, B, seed=seed)
    Y, U, D = synth.make_mhe_data(cfg, bt, nper, seed=seed)
    rng = np.random.default_rng(seed)
    nx, nym, He = cfg.nxh, cfg.nym, cfg.He
    Xw = rng.uniform(0.3, 1.5, nx * (He + 1)); Xw[rng.random(Xw.size) < 0.3] = np.inf
    Ww = rng.uniform(0.05, 0.4, nx * He); Ww[rng.random(Ww.size) < 0.3] = np.inf
    Vw = rng.uniform(0.2, 0.8, nym * He); Vw[rng.random(Vw.size) < 0.3] = np.inf
    class _Absent:                      # (oracle_only: the product's calls go nowhere)
        def __getattr__(self, name):
            return lambda *a, **k: None
    bm = _Absent() if oracle_only else mhe_util.make_product(cfg, bt, lib=lib, bounds={})
    ors = mhe_util.make_oracles(cfg, bt, list(range(B)), bounds={})
    if soft:
        bm.setconstraint(c_x̂max=np.full(nx, 0.5), c_v̂min=np.ones(nym))
        for e in ors:
            e.setconstraint(c_xhatmax=np.full(nx, 0.5), c_vhatmin=np.ones(nym))
    if csoft:
        Cx0 = rng.uniform(0.1, 1.0, nx * (He + 1)); Cx0[rng.random(Cx0.size) < 0.4] = 0.0
        Cx1 = rng.uniform(0.1, 1.0, nx * (He + 1)); Cx1[rng.random(Cx1.size) < 0.4] = 0.0
        Cw1 = rng.uniform(0.1, 1.0, nx * He); Cw1[rng.random(Cw1.size) < 0.4] = 0.0
        Cv0 = rng.uniform(0.1, 1.0, nym * He); Cv0[rng.random(Cv0.size) < 0.4] = 0.0
        bm.setconstraint(C_x̂min=Cx0, C_x̂max=Cx1, C_ŵmax=Cw1, C_v̂min=Cv0)
        for e in ors:
            e.setconstraint(C_xhatmin=Cx0, C_xhatmax=Cx1, C_whatmax=Cw1, C_vhatmin=Cv0)
        Xw = np.where(np.isinf(Xw), Xw, 0.6 * Xw); Ww = np.where(np.isinf(Ww), Ww, 0.6 * Ww)     # tighter: the slack is used
    bm.setconstraint(X̂min=-Xw, X̂max=Xw, Ŵmin=-Ww, Ŵmax=Ww, V̂min=-Vw, V̂max=Vw)
    for e in ors:
        e.setconstraint(Xhatmin=-Xw, Xhatmax=Xw, Whatmin=-Ww, Whatmax=Ww, Vhatmin=-Vw, Vhatmax=Vw)
    ex = ew = 0.0
    active = 0
    for k in range(nper):
        d = D[k] if cfg.nd else None
        xg = bm.preparestate(Y[k], d)
        xo = np.array([e.preparestate(Y[k][b], d[b] if cfg.nd else ()) for b, e in enumerate(ors)])
        if not cfg.direct:
            xg = bm.updatestate(U[k], Y[k], d)
            xo = np.array([e.updatestate(U[k][b], Y[k][b], d[b] if cfg.nd else ()) for b, e in enumerate(ors)])
        assert all(e.status == 0 for e in ors), (k, [e.status for e in ors])
        Nk = ors[0].Nk
        Wo = np.array([e.Zt[e.neps + nx:e.neps + nx + Nk * nx] for e in ors])
        if not oracle_only:
            info = bm.getinfo()
            assert np.all(info["status"] == 0) and info["Nk"] == Nk, (k, info["status"])
            sc = max(1.0, np.abs(xo).max())
            ex = max(ex, np.abs(xg - xo).max() / sc)
            ew = max(ew, np.abs(info["Ŵ"] - Wo).max() / sc)
        if eps_seen is not None and np.isfinite(cfg.Cwt):
            eps_seen.append(max(float(e.Zt[0]) for e in ors))
        for b, e in enumerate(ors):
            Xb = Xw[nx:][(He - Nk) * nx:]
            active += int(np.any(np.abs(np.abs(e.X0[:Nk * nx]) - Xb) <= 1e-6) or np.any(np.abs(np.abs(Wo[b]) - Ww[(He - Nk) * nx:]) <= 1e-6))
        if cfg.direct:
            bm.updatestate(U[k], Y[k], d)
            for b, e in enumerate(ors):
                e.updatestate(U[k][b], Y[k][b], d[b] if cfg.nd else ())
    return ex, ew, active


def random_family_wide_config(seed):
    """The configuration, bounds and batch of one randomised wide family: nx in 13 .. 26, nym in 1 .. 6 with nx + nym <= 32
    (so 14 <= nx̂ <= 32; a draw with nx̂ <= 16 is redrawn), the other draws as mhe_util.random_family."""
    rng = np.random.default_rng(5000 + seed)
    while True:
        nx, nym = int(rng.integers(13, 27)), int(rng.integers(1, 7))
        if 16 < nx + nym <= 32:
            break
    kw = dict(nx=nx, nu=int(rng.integers(0, 4)), nym=nym, nd=int(rng.integers(0, 3)), He=int(rng.integers(1, 7)),
              direct=bool(rng.integers(0, 2)))
    cls = int(rng.integers(0, 6))           # 0 none, 1 x̂, 2 ŵ, 3 v̂, 4 x̂ + v̂, 5 ŵ + v̂
    if cls in (1, 4):
        kw["xabs"] = float(rng.uniform(0.6, 2.0))
    if cls in (2, 5):
        kw["wabs"] = float(rng.uniform(0.1, 0.4))
    if cls in (3, 4, 5):
        kw["vabs"] = float(rng.uniform(0.3, 0.8))
    soft = cls != 0 and rng.random() < 0.4
    if soft:
        kw["Cwt"] = float(10.0 ** rng.uniform(2, 5))
    cfg = synth.MheConfig(f"wfam{seed}", **kw)
    bounds = mhe_util.bounds_of(cfg)
    if soft:
        for key, n in (("xhat", cfg.nxh), ("what", cfg.nxh), ("vhat", cfg.nym)):
            if key + "min" in bounds:
                bounds["c_" + key + "min"] = np.where(rng.random(n) < 0.6, rng.uniform(0.2, 1.5, n), 0.0)
                bounds["c_" + key + "max"] = np.where(rng.random(n) < 0.6, rng.uniform(0.2, 1.5, n), 0.0)
    return cfg, bounds


def random_family_wide(seed, lib=None, B=3, oracle_only=False):
    """One randomised wide family through He + 3 periods on the product and on oracle/mhe.py, every member compared.
    Returns (worst relative error, compared solves, windows the oracle found infeasible, B * periods).  oracle_only: the
    oracle alone (seed selection on the CPU: nfail must be 0 for a seed the GPU test uses)."""
    cfg, bounds = random_family_wide_config(seed)
    bt = synth.make_mhe_batch(cfg, B, seed=seed)
    nper = cfg.He + 3
    Y, U, D = synth.make_mhe_data(cfg, bt, nper, seed=seed)
    bm = None if oracle_only else mhe_util.make_product(cfg, bt, lib=lib, bounds=bounds)
    ors = mhe_util.make_oracles(cfg, bt, range(B), bounds=bounds)
    clean = np.ones(B, bool)
    worst, ncmp, nfail = 0.0, 0, 0
    for k in range(nper):
        y, u, d = Y[k], U[k], (D[k] if cfg.nd else None)
        if bm is not None:
            xg = bm.preparestate(y, d)
            if not cfg.direct:
                xg = bm.updatestate(u, y, d)
        for b, e in enumerate(ors):
            xo = e.preparestate(y[b], d[b] if cfg.nd else ())
            if not cfg.direct:
                xo = e.updatestate(u[b], y[b], d[b] if cfg.nd else ())
            if not clean[b]:
                continue
            if e.status != 0:
                clean[b] = False
                nfail += 1
                continue
            if bm is not None:
                assert bm.status[b] == 0, (seed, k, b, "the product failed on a window the oracle solved")
                worst = max(worst, np.abs(xg[b] - xo).max() / max(1.0, np.abs(xo).max()))
            ncmp += 1
        if cfg.direct:
            if bm is not None:
                bm.updatestate(u, y, d)
            for b, e in enumerate(ors):
                e.updatestate(u[b], y[b], d[b] if cfg.nd else ())
    return worst, ncmp, nfail, B * nper


SOFT20 = dict(c_xhatmin=[1.0] * 20, c_xhatmax=[1.0] * 20, c_whatmin=[0.5] * 20, c_whatmax=[0.0] * 20)


def emulator_cases(lib):
    """The three cases of tests/test_mhe_wide.py on an emulator library with the wide launchers: worst relative errors per case."""
    out = {}
    # hard x̂ bounds, nx̂ = 17 (NX = 24): first row of the GPU table
    cfg = synth.MheConfig("w17", nx=14, nu=2, nym=3, nd=0, He=4, xabs=1.2)
    rows, bm = mhe_util.run_periods(cfg, synth.make_mhe_batch(cfg, 3, seed=5), cfg.He + 3, [0, 1, 2], lib=lib, seed=5)
    out["xhat17"] = _summary(rows, bm)
    # soft x̂ + ŵ bounds with a measured disturbance, nx̂ = 20, He = 3
    cfg = synth.MheConfig("wsoft", nx=16, nu=2, nym=4, nd=1, He=3, xabs=0.8, wabs=0.15, Cwt=1e4)
    bounds = mhe_util.bounds_of(cfg)
    bounds.update({k: np.asarray(v, float) for k, v in SOFT20.items()})
    rows, bm = mhe_util.run_periods(cfg, synth.make_mhe_batch(cfg, 3, seed=17), cfg.He + 2, [0, 1, 2], lib=lib, seed=0, bounds=bounds)
    out["soft20"] = _summary(rows, bm)
    # ŵ + v̂ bounds, nx̂ = 18, predictor form
    cfg = synth.MheConfig("wwv", nx=15, nu=1, nym=3, nd=0, He=3, wabs=0.03, vabs=0.6, direct=False)   # (oracle: ŵ active in 6 of 15 solves)
    rows, bm = mhe_util.run_periods(cfg, synth.make_mhe_batch(cfg, 3, seed=4), cfg.He + 2, [0, 1, 2], lib=lib, seed=4)
    out["what+vhat18"] = _summary(rows, bm)
    return out


def _summary(rows, bm):
    return dict(ex=max(r["ex"] for r in rows), ew=max(r["ew"] for r in rows), ep=max(r["ep"] for r in rows),
                ee=max(r["ee"] for r in rows), eps=max(float(np.max(r["eps"])) for r in rows),
                ok=bool(all((r["status"] == 0).all() and all(s == 0 for s in r["ostatus"]) for r in rows)),
                iters=int(max(r["iters"].max() for r in rows)), NX=bm.handle.register_columns(), lanes=bm.handle.lanes_per_estimator())


if __name__ == "__main__":
    print(json.dumps(emulator_cases(mpcqp.api.load_library(sys.argv[1]))))
