"""Register hand-offs of the one-row-per-lane step kernels (csrc/mpcqp_bodies.h: Step::lane_regs()).

In a compile-time specialisation with nZ~ <= 64 on one wavefront, lane k owns entry k of the vectors of a Newton solve, and
what it computes for its own entry -- its entry of G'w and of the right-hand side, of the solution dz, of Pu dz and its rows
of E dz -- goes to the next phase in a register instead of through an LDS store and a dependent read.  The arithmetic is
untouched, so the checks are the ones of any kernel: every controller of a batch against the oracle and against the
runtime-dimension kernel of the same handle data, which takes none of these paths.

Shapes: the smallest that take each form of the two products with E, each row-slot count, and each group of rows whose
difference w_max - w_min is handed over (CASES below).  B = 64, one period from a cold start and one warm-started period
whose inputs (x̂0 after the oracle's first move, lastu0, the same set point) are the same for all three solvers.

Tolerances: TOL = 1e-5 against the oracle, the bound of tests/test_step_consts.py and tests/test_gpu_parity.py, on the optima
that carry the oracle's active-set certificate (at least 80 % of every shape and period, asserted: seed 0 gives 95 % or
more everywhere); 1e-6 between the two kernels, the project's acceptance figure for an optimum, with equal status."""
import dataclasses

import numpy as np
import pytest

import mpcqp
from mpcqp import synth
from oracle import condense as cd, qp
from tests.parity_util import constraint_kwargs, rel_err

B = 64
SEED = 0
TOL = 1e-5          # relative dU error against a certified oracle optimum
TOL_KERNELS = 1e-6  # relative dU difference between two kernels of the library

# name -> ("nx,nu,ny,Hp,Hc" of synth.get_config: soft ymax + hard umin / umax, changes to that config, x̂max or None)
CASES = {
    # C3's forms of E v and E'w (nu = ny = 4), one Ŷ row slot per lane (the second is never valid), ϵ lane far below 64
    "c3_forms_one_slot": ("4,4,4,8,3", {}, None),
    # two Ŷ row slots with a ragged second one (nY = 80), nDU = 40 like C3
    "c3_forms_two_slots": ("4,4,4,20,10", {}, None),
    # Hc above MPCQP_EAPPLY44_HCMAX: the zero-padded general E v with C3's E'w; nZ~ = 61, next to the wavefront limit
    "general_Ev_c3_Etw": ("4,4,4,16,15", {}, None),
    # the general forms of both products (nu, ny not 4)
    "general_forms": ("3,2,3,12,5", {}, None),
    # no ϵ lane, no Ŷ rows: u bounds only
    "no_slack_u_only": ("4,4,4,8,3", dict(Cwt=np.inf, ymax=np.inf), None),
    # Δu bounds and ymin as well: the ΔU term of G'w and both sides of every pair
    "du_and_both_y_sides": ("4,2,2,10,4", dict(dumin=-0.2, dumax=0.2, ymin=-1.0), None),
    # a terminal bound x̂max: its rows keep the LDS path next to the register one (active for most members at 1.0)
    "terminal_xmax": ("4,4,4,8,3", {}, 1.0),
}


def _config(name):
    spec, over, xmax = CASES[name]
    return dataclasses.replace(synth.get_config(spec), **over), xmax


_REF = {}


def reference(name):
    """Oracle optima of both periods, their certificates and the inputs of the second period; computed once per shape."""
    if name in _REF:
        return _REF[name]
    cfg, xmax = _config(name)
    bt = synth.make_batch(cfg, B, seed=SEED)
    nZ = cfg.nu * cfg.Hc + (0 if np.isinf(cfg.Cwt) else 1)
    Z = np.zeros((2, B, nZ))
    cert = np.zeros((2, B), bool)
    x1, lu1 = np.zeros_like(bt["xhat0"]), np.zeros_like(bt["lastu0"])
    for i in range(B):
        m = cd.LinMPCOracle(bt["Ahat"][i], bt["Bhu"][i], bt["Chat"][i], Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt,
                            Mwt=np.full(cfg.ny, cfg.Mwt), Nwt=np.full(cfg.nu, cfg.Nwt), Lwt=np.full(cfg.nu, cfg.Lwt))
        kw = constraint_kwargs(cfg, oracle=True)
        if xmax is not None:
            kw["xhatmax"] = np.full(cfg.nxh, xmax)
        m.setconstraint(**kw)
        x, lu = bt["xhat0"][i], bt["lastu0"][i]
        for k in range(2):
            m.initpred(x, lu, bt["ry"][i])
            m.linconstraint()
            z, st, info = qp.solve_qp(*m.qp_data(), m.warmstart(), return_info=True)
            assert st == 0, (name, i, k, st)
            Z[k, i], cert[k, i] = z, info["certificate"] == "active-set"
            m.Zt = z
            if k == 0:
                lu = lu + z[:cfg.nu]
                x = bt["Ahat"][i] @ x + bt["Bhu"][i] @ lu
                x1[i], lu1[i] = x, lu
    for a in (Z, cert, x1, lu1):
        a.setflags(write=False)
    _REF[name] = dict(cfg=cfg, xmax=xmax, bt=bt, Z=Z, cert=cert, x=(bt["xhat0"], x1), lu=(bt["lastu0"], lu1))
    return _REF[name]


def two_periods(ref, lib, specialised):
    """Both periods on a handle of the shape's data: the shape's own specialisation (prepared), or the runtime-dimension
    kernel (never prepared, and no object of the shape within the library's reach: see the test).  FLAG_KEEP_QP keeps
    either away from the small-problem kernel."""
    cfg, bt = ref["cfg"], ref["bt"]
    neps = 0 if np.isinf(cfg.Cwt) else 1
    hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, cfg.Hc, neps=neps,
                      flags=mpcqp.FLAG_RY_CONSTANT | mpcqp.FLAG_KEEP_QP, lib=lib)
    hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
    hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt),
                   np.full(B, cfg.Cwt) if neps else None)
    full = lambda v, n: np.full((B, n), float(v)) if np.isfinite(v) else None
    hd.set_bounds(U0min=full(cfg.umin, hd.nU), U0max=full(cfg.umax, hd.nU), DUmin=full(cfg.dumin, hd.nDU),
                  DUmax=full(cfg.dumax, hd.nDU), Y0min=full(cfg.ymin, hd.nY), Y0max=full(cfg.ymax, hd.nY),
                  x0max=None if ref["xmax"] is None else np.full((B, cfg.nxh), ref["xmax"]))
    if specialised:
        assert hd.prepare() == mpcqp.api.KERNEL_ONDEMAND
        assert hd.kernel_kind() == mpcqp.api.KERNEL_ONDEMAND, hd.kernel_kind()
    Z = np.zeros((B, hd.nZ))           # (all zeros: the warm start of the first period is the cold start)
    out = []
    for k in range(2):
        u0, st, it = hd.step(ref["x"][k], ref["lu"][k], bt["ry"], Z)
        out.append(dict(Z=Z.copy(), status=st.copy(), iters=it.copy()))
    if not specialised:
        assert hd.kernel_kind() == mpcqp.api.KERNEL_GENERIC, hd.kernel_kind()
    hd.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_register_handoffs_against_oracle_and_runtime_kernel(hiplib, name, monkeypatch, tmp_path):
    ref = reference(name)
    cfg = ref["cfg"]
    nDU = cfg.nu * cfg.Hc
    assert nDU + (0 if np.isinf(cfg.Cwt) else 1) <= 64          # one row per lane
    # A step of an unprepared handle takes the shape's specialisation when a verified object is loaded or in the cache (from
    # this test's own prepare in an earlier session, say).  The runtime-dimension kernel therefore runs FIRST, with the
    # cache pointed at an empty directory; the prepare below then looks in (and builds into) the normal cache again.
    with monkeypatch.context() as mp:
        mp.setenv("MPCQP_CACHE_DIR", str(tmp_path))
        rtd = two_periods(ref, hiplib, False)
    spec = two_periods(ref, hiplib, True)
    for k in range(2):
        cert = ref["cert"][k]
        assert cert.mean() >= 0.8, (name, k, cert.mean())
        assert np.all(spec[k]["status"] == 0), (name, k, spec[k]["status"])
        err = rel_err(spec[k]["Z"], ref["Z"][k], nDU)
        dif = rel_err(spec[k]["Z"], rtd[k]["Z"], nDU)
        print(f"[lane_handoff] {name} period {k}: certified {cert.mean():.3f}, worst rel dU error vs oracle (certified) "
              f"{err[cert].max():.3e}, worst rel dU difference vs runtime-dimension kernel {dif.max():.3e}, "
              f"factorisations {spec[k]['iters'].mean():.2f}")
        assert err[cert].max() <= TOL, (name, k, int(np.argmax(np.where(cert, err, 0.0))), err[cert].max())
        assert np.array_equal(spec[k]["status"], rtd[k]["status"]), (name, k)
        assert dif.max() <= TOL_KERNELS, (name, k, int(np.argmax(dif)), dif.max())
