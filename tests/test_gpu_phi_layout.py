"""Column-block-major LDS layout of Φ in the one-row-per-lane step kernels (csrc/mpcqp_types.h: phi(); csrc/mpcqp_bodies.h:
Step::PHL).

A compile-time specialisation with nZ~ <= 64 on one wavefront keeps Φ as blocks of four columns (rows consecutive inside a
block, four doubles per row), so that with the column block a constant every address of the factorisation, of the write-backs
and of the substitutions is `row * 32 B + immediate`.  The arithmetic is untouched, so the checks are the ones of any kernel:
every controller of a batch against the oracle and against the runtime-dimension kernel of the same handle data, which keeps
the row-major packed layout (pk()).

Shapes: the smallest at which an index of the layout can go wrong (CASES below: one panel with a ragged last block, exactly
one panel, a second / third panel of one row, four panels, every lane a row, nu not 4, and a handle whose H~ comes packed from
global memory -- through the matrix-core pass and through the polish -- instead of being folded into the row weights).
B = 64, one period from a cold start and one warm-started period whose inputs are the same for all three solvers.

Tolerances: those of tests/test_gpu_lane_handoff.py -- 1e-5 against the oracle on the optima that carry its active-set
certificate (at least 80 % of every shape and period, asserted), 1e-6 between the two kernels with equal status."""
import dataclasses
import shutil

import numpy as np
import pytest

import mpcqp
from mpcqp import synth
from oracle import condense as cd, qp
from tests import test_gpu_lane_handoff as lane_handoff
from tests.parity_util import constraint_kwargs, rel_err

B = 64
SEED = 0
TOL = 1e-5          # relative dU error against a certified oracle optimum
TOL_KERNELS = 1e-6  # relative dU difference between two kernels of the library

NO_Y = dict(Cwt=np.inf, ymax=np.inf)
# name -> ("nx,nu,ny,Hp,Hc" of synth.get_config: soft ymax + hard umin / umax, changes to that config, block output weights,
#          the case of tests/test_gpu_lane_handoff.py with the same data (same B and seed: its reference is shared) or None)
CASES = {
    "n13_one_panel_ragged": ("4,4,4,8,3", {}, False, "c3_forms_one_slot"),
    "n16_one_panel_no_eps_load_H": ("4,4,4,8,4", NO_Y, False, None),       # no Y^ rows: the remapping load_H runs
    "n17_second_panel_one_row": ("4,4,4,8,4", {}, False, None),
    "n33_third_panel_one_row": ("4,4,4,12,8", {}, False, None),
    "n16_nu3_general_writeback": ("3,2,3,12,5", {}, False, "general_forms"),
    "n61_four_panels": ("4,4,4,16,15", {}, False, "general_Ev_c3_Etw"),
    "n64_every_lane_a_row": ("4,4,4,16,16", NO_Y, False, None),
    "n13_block_weights_packed_H": ("4,4,4,8,3", {}, True, None),           # fold_H off: packed H~ through Hg and the polish
}
assert (lane_handoff.B, lane_handoff.SEED) == (B, SEED)


def _mblk(cfg):
    """Symmetric output weight blocks: the config's diagonal weight with a coupling of the first two outputs."""
    blk = cfg.Mwt * np.eye(cfg.ny)
    blk[0, 1] = blk[1, 0] = 0.25 * cfg.Mwt
    return blk


_REF = {}


def reference(name):
    """Oracle optima of both periods, their certificates and the inputs of the second period; computed once per shape."""
    if name in _REF:
        return _REF[name]
    spec, over, blocks, shared = CASES[name]
    cfg = dataclasses.replace(synth.get_config(spec), **over)
    if shared is not None:
        ref = lane_handoff.reference(shared)
        assert ref["cfg"] == cfg and ref["xmax"] is None, (name, shared)
        _REF[name] = ref
        return ref
    bt = synth.make_batch(cfg, B, seed=SEED)
    nZ = cfg.nu * cfg.Hc + (0 if np.isinf(cfg.Cwt) else 1)
    Z = np.zeros((2, B, nZ))
    cert = np.zeros((2, B), bool)
    x1, lu1 = np.zeros_like(bt["xhat0"]), np.zeros_like(bt["lastu0"])
    wkw = dict(Mwt=np.full(cfg.ny, cfg.Mwt))
    if blocks:
        wkw = dict(M_Hp=np.kron(np.eye(cfg.Hp), _mblk(cfg)))
    for i in range(B):
        m = cd.LinMPCOracle(bt["Ahat"][i], bt["Bhu"][i], bt["Chat"][i], Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt,
                            Nwt=np.full(cfg.nu, cfg.Nwt), Lwt=np.full(cfg.nu, cfg.Lwt), **wkw)
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
    _REF[name] = dict(cfg=cfg, blocks=blocks, bt=bt, Z=Z, cert=cert, x=(bt["xhat0"], x1), lu=(bt["lastu0"], lu1))
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
    if ref.get("blocks"):
        hd.set_output_weight_blocks(np.broadcast_to(_mblk(cfg), (B, cfg.Hp, cfg.ny, cfg.ny)).copy())
    full = lambda v, n: np.full((B, n), float(v)) if np.isfinite(v) else None
    hd.set_bounds(U0min=full(cfg.umin, hd.nU), U0max=full(cfg.umax, hd.nU), DUmin=full(cfg.dumin, hd.nDU),
                  DUmax=full(cfg.dumax, hd.nDU), Y0min=full(cfg.ymin, hd.nY), Y0max=full(cfg.ymax, hd.nY))
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


@pytest.fixture(scope="module")
def runtime_lib(hiplib, tmp_path_factory):
    """A second, private instance of the library (a copy of the file, loaded next to the first) for the runtime-dimension
    kernel.  A step of an unprepared handle takes the shape's specialisation once a verified object of it is loaded, and an
    instance keeps what it has loaded: the shapes shared with tests/test_gpu_lane_handoff.py, and the shape this file uses
    with two kinds of weights, would otherwise run on their specialisation in both comparisons.  The copy has loaded
    nothing and only ever sees an empty cache directory (see the test)."""
    path = shutil.copy(hiplib._name, str(tmp_path_factory.mktemp("rtlib") / "libmpcqp_private.so"))
    keep = mpcqp.api._lib
    try:
        lib = mpcqp.api.load_library(path)
    finally:
        mpcqp.api._lib = keep           # (load_library(path) makes the new instance the default one)
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_phi_layout_against_oracle_and_runtime_kernel(hiplib, runtime_lib, name, monkeypatch, tmp_path):
    ref = reference(name)
    cfg = ref["cfg"]
    nDU = cfg.nu * cfg.Hc
    assert nDU + (0 if np.isinf(cfg.Cwt) else 1) <= 64          # one row per lane
    # The runtime-dimension kernel runs on the private instance with the cache pointed at an empty directory: a step of an
    # unprepared handle would otherwise take the shape's specialisation from the cache.  The prepare below then uses the
    # normal cache again.
    with monkeypatch.context() as mp:
        mp.setenv("MPCQP_CACHE_DIR", str(tmp_path))
        rtd = two_periods(ref, runtime_lib, False)
    spec = two_periods(ref, hiplib, True)
    for k in range(2):
        cert = ref["cert"][k]
        assert cert.mean() >= 0.8, (name, k, cert.mean())
        assert np.all(spec[k]["status"] == 0), (name, k, spec[k]["status"])
        err = rel_err(spec[k]["Z"], ref["Z"][k], nDU)
        dif = rel_err(spec[k]["Z"], rtd[k]["Z"], nDU)
        print(f"[phi_layout] {name} period {k}: certified {cert.mean():.3f}, worst rel dU error vs oracle (certified) "
              f"{err[cert].max():.3e}, worst rel dU difference vs runtime-dimension kernel {dif.max():.3e}, "
              f"factorisations {spec[k]['iters'].mean():.2f}")
        assert err[cert].max() <= TOL, (name, k, int(np.argmax(np.where(cert, err, 0.0))), err[cert].max())
        assert np.array_equal(spec[k]["status"], rtd[k]["status"]), (name, k)
        assert dif.max() <= TOL_KERNELS, (name, k, int(np.argmax(dif)), dif.max())
