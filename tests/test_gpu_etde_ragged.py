"""The ragged last tile row of E'DE on 4 x 4 x 4 matrix-core blocks (csrc/mpcqp_bodies.h, EtDE_share_, B4): with
nu = ny = 4, register operands, at least three tile rows and nDU mod 16 = 4 or 8, the one or two block rows of the last
tile row run on v_mfma_f64_4x4x4_4b, and the ϵ row of Phi is left to the caller (zeroed in the overwrite mode, set from H̃
where H̃ comes packed from global memory).

Shapes: one block row with a single step in the pass, two block rows with one step for the second, a longer horizon on
the same rows, C3 itself, four tile rows -- and three controls whose conditions keep them on the 16x16x4 form (nDU mod
16 = 12, no ragged row with the ϵ row on a tile boundary, nu = 2).  Which form a shape runs on is a property of the code
(the compile-time condition B4) that no check here can see: the controls pass on either form, they only show that the
shapes next to the condition's edges still compute the right thing.  B = 64.

test_etde_ragged_row, every shape with a soft ymax (the ϵ row) and with hard input bounds only:
  * H̃ = 2 E'ME + .. read back through MPCQP_GET_HESSIAN against oracle/condense at 1e-11: the matrix-core pass alone (K2,
    in-place mode, packed layout);
  * one cold and one warm step (shifted start) against the oracle's C port at the suite's tolerance, all optimal.  With
    the soft ymax that is the assembly in the overwrite mode with its zeroed ϵ row (column-block-major layout) in every
    factorisation.  With hard input bounds only there are no Ŷ rows, the step never calls the pass, and these cases cover
    K2's in-place pass alone;
  * soft C3: the mean number of factorisations of the cold step within 0.5 of the C port's.

test_etde_ragged_row_hard_outputs: a HARD ymax (Cwt = inf), the overwrite mode with nZ̃ = nDU -- no ϵ row to zero behind
the pass.  ymax = 2 instead of the soft cases' 1: a hard bound at 1 is infeasible for a quarter to a half of the members;
at 2 the C port still finds output rows active at the optimum and solves all but a few.  The batch is the first 64 of
128 members whose cold and warm problems the C port solves, on the C port's own trajectory.

test_etde_ragged_row_block_weights: block output weights (M_Hp = blkdiag of coupled 4 x 4 blocks) with the soft ymax.
H̃ is then not folded into the row factors: the pass gets it packed from global memory (Hg), adds it in the write-back
and copies its ϵ row.  One block row, two block rows, C3.  The C port has diagonal weights only, so the reference is
oracle/condense + oracle/qp on every ninth member (seconds for C3), compared where its optimum carries the active-set
certificate (at least 80 %, asserted, as in tests/test_gpu_phi_layout.py); status is checked on all 64.
"""
import dataclasses

import numpy as np
import pytest

import mpcqp
from mpcqp import synth
from oracle import condense as cd, qp
from tests.parity_util import constraint_kwargs, make_controller, make_oracle, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5            # tests/test_gpu_parity.py
B = 64

# (nx, nu, ny, Hp, Hc)
SHAPES = {
    "one_block_row_one_step": (6, 4, 4, 9, 9),
    "two_block_rows": (6, 4, 4, 10, 10),
    "two_block_rows_Hp12": (6, 4, 4, 12, 10),
    "C3": (12, 4, 4, 30, 10),
    "four_tile_rows": (8, 4, 4, 15, 14),
    "control_mod16_12": (6, 4, 4, 12, 11),
    "control_no_ragged_row": (6, 4, 4, 12, 12),
    "control_nu_2": (6, 2, 4, 12, 6),
}
CASES = [(s, p) for s in SHAPES for p in ("soft", "hard")]
HARD_Y_SHAPES = ["one_block_row_one_step", "two_block_rows_Hp12", "C3"]
BLOCK_SHAPES = ["one_block_row_one_step", "two_block_rows_Hp12", "C3"]
HARD_YMAX = 2.0
STRIDE_BLOCKS = 9     # members with an oracle of their own in the block-weight cases


def config(shape, pattern):
    nx, nu, ny, Hp, Hc = SHAPES[shape]
    cfg = synth.get_config(f"{nx},{nu},{ny},{Hp},{Hc}")       # C3's pattern: soft ymax, hard umin / umax
    if pattern == "hard":
        cfg = dataclasses.replace(cfg, ymax=np.inf, Cwt=np.inf)
    elif pattern == "hard_y":
        cfg = dataclasses.replace(cfg, ymax=HARD_YMAX, Cwt=np.inf)
    return cfg


@pytest.mark.parametrize("shape,pattern", CASES)
def test_etde_ragged_row(shape, pattern, hiplib):
    from oracle import cport
    cfg = config(shape, pattern)
    nDU = cfg.nu * cfg.Hc
    bt = synth.make_batch(cfg, B, seed=5)
    mpc = make_controller(cfg, bt, keep_qp=True)
    mpc.lastu0 = bt["lastu0"].copy()
    ref = cport.from_synth(cfg, bt)

    # cold step
    u1 = mpc.moveinput(bt["xhat0"], bt["ry"]).copy()
    assert mpc.hd.kernel_kind() in (mpcqp.api.KERNEL_AOT, mpcqp.api.KERNEL_ONDEMAND)
    assert np.all(mpc.status == mpcqp.STATUS_OPTIMAL), np.unique(mpc.status, return_counts=True)
    it1 = mpc.iters.copy()
    H = mpc.hd.get(mpcqp.GET_HESSIAN)
    eh = 0.0
    for i in range(0, B, 7):
        m = make_oracle(cfg, bt, i)
        m.initpred(bt["xhat0"][i], bt["lastu0"][i], bt["ry"][i])
        assert H[i].shape == m.Ht.shape
        eh = max(eh, np.abs(H[i] - m.Ht).max() / max(1.0, np.abs(m.Ht).max()))
        # (the ΔU block on its own scale as well: with a soft bound the slack weight dominates |H̃|∞)
        eh = max(eh, np.abs(H[i] - m.Ht)[:nDU, :nDU].max() / max(1.0, np.abs(m.Ht[:nDU, :nDU]).max()))
    Zc, _, stc, itc = ref.step(bt["xhat0"], bt["lastu0"], bt["ry"])
    assert np.all(stc == 0)
    e1 = rel_err(mpc.Z, Zc, nDU).max()

    # warm step: both from their own shifted optimum, on the trajectory of the kernel's first move
    x1 = np.einsum("bij,bj->bi", bt["Ahat"], bt["xhat0"]) + np.einsum("bij,bj->bi", bt["Bhu"], u1)
    mpc.moveinput(x1, bt["ry"])
    assert np.all(mpc.status == mpcqp.STATUS_OPTIMAL), np.unique(mpc.status, return_counts=True)
    Zw, _, stw, _ = ref.step(x1, u1, bt["ry"], Z=Zc.copy(), cold=False)
    assert np.all(stw == 0)
    e2 = rel_err(mpc.Z, Zw, nDU).max()
    print(f"[etde4] {shape}/{pattern}: kind {mpc.hd.kernel_kind()} H̃ err {eh:.2e} cold {e1:.2e} warm {e2:.2e} "
          f"iters {it1.mean():.2f} (C port {np.mean(itc):.2f})")
    assert eh <= 1e-11, eh
    assert e1 <= TOL, e1
    assert e2 <= TOL, e2
    if shape == "C3" and pattern == "soft":
        assert abs(it1.mean() - np.mean(itc)) <= 0.5, (it1.mean(), np.mean(itc))


@pytest.mark.parametrize("shape", HARD_Y_SHAPES)
def test_etde_ragged_row_hard_outputs(shape, hiplib):
    from oracle import cport
    cfg = config(shape, "hard_y")
    nDU = cfg.nu * cfg.Hc
    # the first B of 2 B members whose cold and warm problems the C port solves, on the C port's own trajectory: the
    # choice does not depend on the code under test
    pool = synth.make_batch(cfg, 2 * B, seed=5)
    ref = cport.from_synth(cfg, pool)
    Zp, u0p, stp, _ = ref.step(pool["xhat0"], pool["lastu0"], pool["ry"])
    xp = np.einsum("bij,bj->bi", pool["Ahat"], pool["xhat0"]) + np.einsum("bij,bj->bi", pool["Bhu"], u0p)
    Zq, _, stq, _ = ref.step(xp, u0p, pool["ry"], Z=Zp.copy(), cold=False)
    pick = np.flatnonzero((stp == 0) & (stq == 0))[:B]
    assert pick.size == B, pick.size
    bt = {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in pool.items()}
    Zc, u1, x1, Zw = Zp[pick], u0p[pick], xp[pick], Zq[pick]

    mpc = make_controller(cfg, bt, keep_qp=True)
    mpc.lastu0 = bt["lastu0"].copy()
    mpc.moveinput(bt["xhat0"], bt["ry"])
    assert mpc.hd.kernel_kind() in (mpcqp.api.KERNEL_AOT, mpcqp.api.KERNEL_ONDEMAND)
    assert np.all(mpc.status == mpcqp.STATUS_OPTIMAL), np.unique(mpc.status, return_counts=True)
    e1 = rel_err(mpc.Z, Zc, nDU).max()
    mpc.lastu0 = u1.copy()
    mpc.moveinput(x1, bt["ry"])
    assert np.all(mpc.status == mpcqp.STATUS_OPTIMAL), np.unique(mpc.status, return_counts=True)
    e2 = rel_err(mpc.Z, Zw, nDU).max()
    print(f"[etde4] {shape}/hard_y: kind {mpc.hd.kernel_kind()} members {pick[-1] + 1} tried for {B} "
          f"cold {e1:.2e} warm {e2:.2e}")
    assert e1 <= TOL, e1
    assert e2 <= TOL, e2


def _mblk(cfg):
    """Symmetric output weight block: the config's diagonal weight with a coupling of the first two outputs
    (tests/test_gpu_phi_layout.py)."""
    blk = cfg.Mwt * np.eye(cfg.ny)
    blk[0, 1] = blk[1, 0] = 0.25 * cfg.Mwt
    return blk


@pytest.mark.parametrize("shape", BLOCK_SHAPES)
def test_etde_ragged_row_block_weights(shape, hiplib):
    cfg = config(shape, "soft")
    nDU = cfg.nu * cfg.Hc
    bt = synth.make_batch(cfg, B, seed=5)
    M_Hp = np.kron(np.eye(cfg.Hp), _mblk(cfg))
    mpc = make_controller(cfg, bt, keep_qp=True, M_Hp=M_Hp)
    assert mpc.Mblk is not None
    mpc.lastu0 = bt["lastu0"].copy()

    u1 = mpc.moveinput(bt["xhat0"], bt["ry"]).copy()
    assert mpc.hd.kernel_kind() in (mpcqp.api.KERNEL_AOT, mpcqp.api.KERNEL_ONDEMAND)
    assert np.all(mpc.status == mpcqp.STATUS_OPTIMAL), np.unique(mpc.status, return_counts=True)
    Z1 = mpc.Z.copy()
    H = mpc.hd.get(mpcqp.GET_HESSIAN)
    x1 = np.einsum("bij,bj->bi", bt["Ahat"], bt["xhat0"]) + np.einsum("bij,bj->bi", bt["Bhu"], u1)
    mpc.moveinput(x1, bt["ry"])
    assert np.all(mpc.status == mpcqp.STATUS_OPTIMAL), np.unique(mpc.status, return_counts=True)
    Z2 = mpc.Z.copy()

    eh, err, cert = 0.0, [[], []], [[], []]
    for i in range(0, B, STRIDE_BLOCKS):
        m = cd.LinMPCOracle(bt["Ahat"][i], bt["Bhu"][i], bt["Chat"][i], Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt,
                            Nwt=np.full(cfg.nu, cfg.Nwt), Lwt=np.full(cfg.nu, cfg.Lwt), M_Hp=M_Hp)
        m.setconstraint(**constraint_kwargs(cfg, oracle=True))
        for k, (x, lu, Zk) in enumerate(((bt["xhat0"][i], bt["lastu0"][i], Z1), (x1[i], u1[i], Z2))):
            m.initpred(x, lu, bt["ry"][i])
            m.linconstraint()
            if k == 0:
                eh = max(eh, np.abs(H[i] - m.Ht).max() / max(1.0, np.abs(m.Ht).max()),
                         np.abs(H[i] - m.Ht)[:nDU, :nDU].max() / max(1.0, np.abs(m.Ht[:nDU, :nDU]).max()))
            z, st, info = qp.solve_qp(*m.qp_data(), m.warmstart(), return_info=True)
            assert st == 0, (shape, i, k, st)
            m.Zt = z
            err[k].append(rel_err(Zk[i:i + 1], z[None, :], nDU).max())
            cert[k].append(info["certificate"] == "active-set")
    err, cert = np.array(err), np.array(cert)
    print(f"[etde4] {shape}/block weights: kind {mpc.hd.kernel_kind()} H̃ err {eh:.2e} certified {cert.mean(axis=1)} "
          f"cold {err[0][cert[0]].max():.2e} warm {err[1][cert[1]].max():.2e}")
    assert eh <= 1e-11, eh
    for k in range(2):
        assert cert[k].mean() >= 0.8, (k, cert[k].mean())
        assert err[k][cert[k]].max() <= TOL, (k, err[k][cert[k]].max())
