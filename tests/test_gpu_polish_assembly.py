"""Newton matrix of the active-set polish in the specialised step kernels (csrc/mpcqp_bodies.h: Step::add_GtDG<POL>,
Qp::EtDE_share_ with MK).

Where the matrix-core pass writes the whole triangle, a polish attempt builds Phi = H~ + rho G_A'G_A from the packed H~ that
K2 left in global memory and from the K steps (four rows of E each) that hold a row of the working set A; every other K step
is skipped by a wave-uniform branch.  The interior-point iterations, and the runtime-dimension kernel, still assemble the
whole E'DE.  95 % of the solves end in the polish, so its matrix decides the returned optimum: every controller of a batch is
compared with the oracle and with the runtime-dimension kernel of the same handle data, as in tests/test_gpu_phi_layout.py
(whose helpers, shapes and shared references this file uses).

Shapes (CASES): the smallest at which the assembly takes another path --
  one panel with the config's ymax (some K steps skipped), ymax never reached (A holds no Y^ row: every K step skipped, the
  pass writes H~ alone), ymax = -2 (the tightest bound the oracle still solves; most K steps stay in);
  a third tile row of one row (n = 33), four tile rows and one-row passes (n = 61);
  ny = 8 (two K steps per horizon step, register-operand form); nu = 2, ny = 3 (operands from LDS, ragged last K step);
  block output weights (H~ came packed before this change; the skip is new there).
"Every horizon step has a row in A" cannot be had for every controller of a batch with one scalar bound: a vertex of the
nZ~ = 13 problem has at most 13 active rows and the shared slack makes the active Y^ rows those of the largest violation.
At ymax = -2 every step is active in 13 (cold) and 15 (warm) of the 64 controllers and no controller has an empty mask; the
CPU half below asserts these counts' lower bounds (and the empty masks of the never-reached case) on the oracle's optima,
with a row counted as active when its slack is below 1e-9 (1 + |h|).

B = 64, seed 0, one cold and one warm period.  Tolerances and cap: those of tests/test_gpu_phi_layout.py -- 1e-5 against
certified oracle optima (at least 80 % of every shape and period, asserted for all eight cases by the CPU test below as
well), 1e-6 between the two kernels with equal status.  Bit-identity with the full assembly is not expected (Phi_A differs
by rounding; the polish re-evaluates its residuals exactly every round).

The optimum alone cannot tell a wrong polish matrix: the rounds then stagnate, z is restored and the interior-point
iterations finish within the same tolerances.  What shows is the factorisation count (`iters` = interior-point iterations
+ polish attempts).  The runtime-dimension kernel runs the same algorithm with the full assembly, and the polish ends about
nine solves in ten: a polish that no longer accepts costs each of them the failed attempt and at least one more
factorisation, 0.9 or more on the mean of a batch.  Rounding in Phi_A can at most move a marginal controller by an
attempt.  So the mean of the specialised kernel must not exceed that of the runtime-dimension kernel by more than
ITERS_ALLOWANCE = 0.1 (six controllers of 64 by one factorisation), for every case and period."""
import dataclasses

import numpy as np
import pytest

from mpcqp import synth
from oracle import condense as cd, qp
from tests import test_gpu_phi_layout as phi_layout
from tests.parity_util import constraint_kwargs, rel_err
from tests.test_gpu_phi_layout import runtime_lib  # noqa: F401  (fixture: the private instance for the runtime-dimension kernel)

B, SEED = phi_layout.B, phi_layout.SEED
TOL, TOL_KERNELS = phi_layout.TOL, phi_layout.TOL_KERNELS
ITERS_ALLOWANCE = 0.1   # mean factorisations, specialised over runtime-dimension kernel (see above)

# name -> ("nx,nu,ny,Hp,Hc" of synth.get_config, changes to that config, block output weights,
#          the case of tests/test_gpu_phi_layout.py with the same data (its reference is shared) or None)
CASES = {
    "n13_config_ymax": ("4,4,4,8,3", {}, False, "n13_one_panel_ragged"),
    "n13_ymax_never_reached": ("4,4,4,8,3", dict(ymax=1e3), False, None),
    "n13_ymax_tight": ("4,4,4,8,3", dict(ymax=-2.0), False, None),
    "n33_third_tile_row": ("4,4,4,12,8", {}, False, "n33_third_panel_one_row"),
    "n61_four_tile_rows": ("4,4,4,16,15", {}, False, "n61_four_panels"),
    "n13_ny8_two_k_steps_per_step": ("4,4,8,8,3", {}, False, None),
    "n11_nu2_ny3_operands_from_lds": ("3,2,3,12,5", {}, False, "n16_nu3_general_writeback"),
    "n13_block_weights": ("4,4,4,8,3", {}, True, "n13_block_weights_packed_H"),
}

_REF = {}


def reference(name):
    """Oracle optima of both periods, their certificates and the inputs of the second period (the layout of
    tests/test_gpu_phi_layout.py: reference), computed once per case."""
    if name in _REF:
        return _REF[name]
    spec, over, blocks, shared = CASES[name]
    if shared is not None:
        ref = phi_layout.reference(shared)
        assert ref["cfg"] == dataclasses.replace(synth.get_config(spec), **over) and bool(ref.get("blocks")) == blocks, name
        _REF[name] = ref
        return ref
    assert not blocks
    cfg = dataclasses.replace(synth.get_config(spec), **over)
    bt = synth.make_batch(cfg, B, seed=SEED)
    Z = np.zeros((2, B, cfg.nu * cfg.Hc + 1))
    cert = np.zeros((2, B), bool)
    x1, lu1 = np.zeros_like(bt["xhat0"]), np.zeros_like(bt["lastu0"])
    for i in range(B):
        m = cd.LinMPCOracle(bt["Ahat"][i], bt["Bhu"][i], bt["Chat"][i], Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt,
                            Mwt=np.full(cfg.ny, cfg.Mwt), Nwt=np.full(cfg.nu, cfg.Nwt), Lwt=np.full(cfg.nu, cfg.Lwt))
        m.setconstraint(**constraint_kwargs(cfg, oracle=True))
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
    _REF[name] = dict(cfg=cfg, blocks=False, bt=bt, Z=Z, cert=cert, x=(bt["xhat0"], x1), lu=(bt["lastu0"], lu1))
    return _REF[name]


def active_steps(ref, k):
    """Per controller: the number of horizon steps with an active Y^max row at the oracle's optimum of period k."""
    cfg, bt = ref["cfg"], ref["bt"]
    nU, nDU, nY = cfg.nu * cfg.Hp, cfg.nu * cfg.Hc, cfg.ny * cfg.Hp
    out = np.zeros(B, int)
    for i in range(B):
        m = cd.LinMPCOracle(bt["Ahat"][i], bt["Bhu"][i], bt["Chat"][i], Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt,
                            Mwt=np.full(cfg.ny, cfg.Mwt), Nwt=np.full(cfg.nu, cfg.Nwt), Lwt=np.full(cfg.nu, cfg.Lwt))
        m.setconstraint(**constraint_kwargs(cfg, oracle=True))
        m.initpred(ref["x"][k][i], ref["lu"][k][i], bt["ry"][i])
        b = m.linconstraint()
        rows = slice(2 * nU + 2 * nDU + nY, 2 * nU + 2 * nDU + 2 * nY)            # Y^max
        slack = b[rows] - m.A[rows] @ ref["Z"][k, i]
        out[i] = (slack <= 1e-9 * (1.0 + np.abs(b[rows]))).reshape(cfg.Hp, cfg.ny).any(axis=1).sum()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_alone_meets_the_cap_and_the_masks_are_what_the_case_says(name):
    """CPU: the cap of every case; the active steps of the cases that are about them."""
    ref = reference(name)
    Hp = ref["cfg"].Hp
    for k in range(2):
        assert ref["cert"][k].mean() >= 0.8, (name, k, ref["cert"][k].mean())
        if name not in ("n13_ymax_never_reached", "n13_ymax_tight", "n13_ny8_two_k_steps_per_step"):
            continue
        a = active_steps(ref, k)
        print(f"[polish_assembly] {name} period {k}: certified {ref['cert'][k].mean():.3f}, controllers by active steps "
              f"{np.bincount(a, minlength=Hp + 1).tolist()}")
        if name == "n13_ymax_never_reached":
            assert np.all(a == 0), (name, k)
        elif name == "n13_ymax_tight":
            assert np.all(a >= 1) and np.sum(a == Hp) >= 10, (name, k, np.bincount(a, minlength=Hp + 1))
        else:
            assert np.sum(a == 0) >= 1 and np.sum(a == Hp) >= 1, (name, k, np.bincount(a, minlength=Hp + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_polish_assembly_against_oracle_and_runtime_kernel(hiplib, runtime_lib, name, monkeypatch, tmp_path):  # noqa: F811
    ref = reference(name)
    cfg = ref["cfg"]
    nDU = cfg.nu * cfg.Hc
    # (the runtime-dimension kernel on the private instance, its cache pointed at an empty directory: see
    #  tests/test_gpu_phi_layout.py)
    with monkeypatch.context() as mp:
        mp.setenv("MPCQP_CACHE_DIR", str(tmp_path))
        rtd = phi_layout.two_periods(ref, runtime_lib, False)
    spec = phi_layout.two_periods(ref, hiplib, True)
    for k in range(2):
        cert = ref["cert"][k]
        assert cert.mean() >= 0.8, (name, k, cert.mean())
        assert np.all(spec[k]["status"] == 0), (name, k, spec[k]["status"])
        err = rel_err(spec[k]["Z"], ref["Z"][k], nDU)
        dif = rel_err(spec[k]["Z"], rtd[k]["Z"], nDU)
        print(f"[polish_assembly] {name} period {k}: certified {cert.mean():.3f}, worst rel dU error vs oracle (certified) "
              f"{err[cert].max():.3e}, worst rel dU difference vs runtime-dimension kernel {dif.max():.3e}, "
              f"factorisations {spec[k]['iters'].mean():.2f} (runtime-dimension kernel {rtd[k]['iters'].mean():.2f})")
        assert err[cert].max() <= TOL, (name, k, int(np.argmax(np.where(cert, err, 0.0))), err[cert].max())
        assert np.array_equal(spec[k]["status"], rtd[k]["status"]), (name, k)
        assert dif.max() <= TOL_KERNELS, (name, k, int(np.argmax(dif)), dif.max())
        assert spec[k]["iters"].mean() <= rtd[k]["iters"].mean() + ITERS_ALLOWANCE, \
            (name, k, spec[k]["iters"].mean(), rtd[k]["iters"].mean(), np.flatnonzero(spec[k]["iters"] > rtd[k]["iters"]))
