"""Helpers of the option tests of the stage-structured (MultipleShooting) kernel: stage-separable Hermitian weight blocks
(M_Hp: ny x ny per step, N_Hc: nu x nu per free move, L_Hp: nu x nu per step; construct.jl:45-93, 837-845),
MPCQP_FLAG_WARM_DUAL and MPCQP_FLAG_KEEP_QP on that kernel, against the condensed oracle (both transcriptions solve the
same QP).  Written after tests/ms_custom_util.py, which is left as it is."""
import warnings

import numpy as np

import mpcqp
from mpcqp import api, synth
from oracle import condense as cd
from tests import ms_custom_util as mcu
from tests.parity_util import constraint_kwargs, make_controller, make_oracle, unstable_plant_members

TOL = 1e-5
# kept q~ / F of the stage kernel against the oracle, relative (tests/test_gpu_parity.py: 1e-11 on the condensed path).  The
# stage-form sums run in another order; worst error measured on the emulator over the cases of tests/test_ms_options.py:
# 7.6e-15 (F of 12,4,4,46,46 after 46 steps of its roll-out; 4.3e-16 at 3,4,2,46,46; deterministic).  The bound is 10 x that figure; the GPU figure has not been measured yet -- the GPU
# differs from the emulator by the order of its wave reductions only, and an error above 1e-9 would be a bug, not rounding.
KEEP_TOL = 7.6e-14

M_BLK = np.array([[2.0, 0.3], [0.3, 1.0]])
N_BLK = np.array([[0.2, 0.08], [0.08, 0.1]])
L_BLK = np.array([[0.05, -0.02], [-0.02, 0.03]])


def on_stage_kernel(g):
    """The assertions every case makes after a step: no reason mask, the stage-structured kernel, all OPTIMAL."""
    assert g.hd.transcription_supported() == 0, g.hd.transcription_supported()
    assert g.kernel == api.KERNEL_MS, g.kernel
    assert np.all(g.status == 0), g.status


def rel_to_oracle(g, o, i=0):
    """Relative difference of member i's ΔU and ϵ to the oracle's."""
    nDU = g.nDU
    worst = np.abs(g.Z[i, :nDU] - o.Zt[:nDU]).max() / max(1.0, np.abs(o.Zt[:nDU]).max())
    if g.Z.shape[1] > nDU:
        worst = max(worst, abs(g.Z[i, -1] - o.Zt[-1]) / max(1.0, abs(o.Zt[-1])))
    return float(worst)


def block_weights(Hp, nmoves, which, diag_only=False):
    """M_Hp / N_Hc / L_Hp = kron(I, block) for the letters in `which` (diag_only: the diagonals of the blocks alone)."""
    d = (lambda Bk: np.diag(np.diag(Bk))) if diag_only else (lambda Bk: Bk)
    kw = {}
    if "M" in which:
        kw["M_Hp"] = np.kron(np.eye(Hp), d(M_BLK))
    if "N" in which:
        kw["N_Hc"] = np.kron(np.eye(nmoves), d(N_BLK))
    if "L" in which:
        kw["L_Hp"] = np.kron(np.eye(Hp), d(L_BLK))
    return kw


def blocks_plant():
    """The plant, horizons and constraints of the block-weight closed loop (move blocking [1, 2, 2] extended to four moves
    over Hp = 8: steps without a free move)."""
    rng = np.random.default_rng(4)
    A = np.diag([0.85, 0.6, 0.3]); Bu = rng.standard_normal((3, 2)); C = rng.standard_normal((2, 3))
    x0 = 0.3 * rng.standard_normal(3)
    con = dict(umin=[-0.6, -1.0], umax=[1.4, 0.9], ymax=[0.6, 0.8])
    return A, Bu, C, x0, dict(Hp=8, Hc=[1, 2, 2], Cwt=1e5), con


def blocks_oracle_loop(which="MNL", diag_only=False, custom=False, periods=3, extra=None):
    """The closed loop on the oracle alone: per period (x̂0, u(k-1), ry, Z̃, status)."""
    A, Bu, C, x0, kw, con = blocks_plant()
    kw = dict(kw, **block_weights(8, 4, which, diag_only), **(extra or {}))
    if custom:
        kw.update(Wy=[[1.0, 0.5]], Wu=[[0.2, -0.3]]); con = dict(con, wmax=[0.7])
    o = cd.LinMPCOracle(A, Bu, C, **kw)
    o.setconstraint(**con)
    o.lastu0 = np.zeros(2)
    out = []
    for k in range(periods):
        ry = [2.5 + 0.2 * k, 0.4]
        lu = o.lastu0.copy()
        u = o.moveinput(x0, ry)
        out.append(dict(x0=x0.copy(), lu=lu, ry=ry, Z=o.Zt.copy(), status=o.status, u=u.copy()))
        x0 = A @ x0 + 0.5 * Bu @ u
    return out, (A, Bu, C, kw, con)


def blocks_closed_loop(lib=None, B=2, which="MNL", custom=False, transcription="MultipleShooting", raw_M=False):
    """Three closed-loop periods with stage-separable weight blocks on the stage kernel, every member driven along the
    oracle's trajectory.  raw_M: the M_Hp blocks are sent through mpcqp_set_dense_weights (what a caller of the C-ABI may do)
    instead of mpcqp_set_output_weight_blocks.  Returns dict(worst difference to the oracle, slack per period, defect)."""
    ref, (A, Bu, C, kw, con) = blocks_oracle_loop(which, custom=custom)
    assert all(r["status"] == 0 for r in ref)
    gkw = dict(kw)
    if raw_M:
        gkw.pop("M_Hp")
    g = mpcqp.BatchLinMPC(mcu.rep(A, B), mcu.rep(Bu, B), mcu.rep(C, B), lib=lib, transcription=transcription, **gkw)
    if raw_M:
        g.hd.set_dense_weights(M_Hp=mcu.rep(kw["M_Hp"], B), N_Hc=None if "N" not in which else mcu.rep(kw["N_Hc"], B),
                               L_Hp=None if "L" not in which else mcu.rep(kw["L_Hp"], B))
    g.setconstraint(**con)
    out = dict(worst=0.0, eps=[], defect=0.0)
    for r in ref:
        g.lastu0 = mcu.rep(r["lu"], B)
        mcu.no_fallback_step(g, np.tile(r["x0"], (B, 1)), r["ry"])
        on_stage_kernel(g)
        o = type("O", (), dict(Zt=r["Z"]))
        out["worst"] = max(out["worst"], max(rel_to_oracle(g, o, i) for i in range(B)))
        out["eps"].append(float(r["Z"][-1]))
        out["defect"] = max(out["defect"], float(g.hd.get(api.GET_MS_DEFECT).max()))
    return out


def blocks_matter_on_the_oracle():
    """max |ΔU(blocks) - ΔU(diagonals of the blocks)| per period, on the oracle: what a kernel that ignored the
    off-diagonal entries would be wrong by."""
    full, _ = blocks_oracle_loop("MNL")
    diag, _ = blocks_oracle_loop("MNL", diag_only=True)
    return [float(np.abs(a["Z"][:-1] - b["Z"][:-1]).max()) for a, b in zip(full, diag)]


def coupled_weight_case(lib, which, B=2):
    """A weight that couples two stages (N_Hc: moves 0 and 1; L_Hp: steps 1 and 2, which share a move-blocking interval)
    under MultipleShooting: returns (reason mask, the warning's text, worst difference to the oracle)."""
    A, Bu, C, x0, kw, con = blocks_plant()
    kw = dict(kw, **block_weights(8, 4, which))
    key = {"N": "N_Hc", "L": "L_Hp"}[which]
    W = kw[key].copy()
    W[0, 2] = W[2, 0] = 0.01
    if which == "L":
        W[0, 2] = W[2, 0] = 0.0
        W[2, 4] = W[4, 2] = 0.01
    kw[key] = W
    g = mpcqp.BatchLinMPC(mcu.rep(A, B), mcu.rep(Bu, B), mcu.rep(C, B), lib=lib, transcription="MultipleShooting", **kw)
    g.setconstraint(**con)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        g.moveinput(np.tile(x0, (B, 1)), [2.5, 0.4])
    g.hd.set_transcription(api.MULTIPLE_SHOOTING)
    why = g.hd.transcription_supported()
    o = cd.LinMPCOracle(A, Bu, C, **kw)
    o.setconstraint(**con)
    o.lastu0 = np.zeros(2)
    o.moveinput(x0, [2.5, 0.4])
    assert o.status == 0 and np.all(g.status == 0)
    return why, " | ".join(str(w.message) for w in rec), max(rel_to_oracle(g, o, i) for i in range(B))


def asymmetric_block_mask(lib, which, B=2):
    """Reason mask of a MultipleShooting handle whose N_Hc / L_Hp is block-diagonal with one block that is not symmetric
    (the stage kernel reads the blocks as symmetric matrices: mpcqp_set_dense_weights classifies such a matrix as not
    stage-separable), and of the same handle once the block is symmetric again."""
    A, Bu, C, x0, kw, con = blocks_plant()
    kw = dict(kw, **block_weights(8, 4, "MNL"))
    key = {"N": "N_Hc", "L": "L_Hp"}[which]
    g = mpcqp.BatchLinMPC(mcu.rep(A, B), mcu.rep(Bu, B), mcu.rep(C, B), lib=lib, transcription="MultipleShooting", **kw)
    g.hd.set_transcription(api.MULTIPLE_SHOOTING)
    W = {k: mcu.rep(kw[k], B) for k in ("M_Hp", "N_Hc", "L_Hp")}
    W[key][B - 1, 2, 3] += 1e-3            # block 1 of the last member: (0, 1) without (1, 0)
    g.hd.set_dense_weights(**W)
    bad = g.hd.transcription_supported()
    W[key][B - 1, 3, 2] += 1e-3
    g.hd.set_dense_weights(**W)
    return bad, g.hd.transcription_supported()


# ---- dual warm start ---------------------------------------------------------------------------------------------
WARM_CFG = synth.Config("cl", nx=3, nu=2, ny=2, Hp=8, Hc=3, umin=-0.6, umax=0.7, ymax=0.9)


def closed_loop_pair_ms(cfg, bt, steps, lib=None, noise=0.02, seed=1, **kw):
    """parity_util.closed_loop_pair under MultipleShooting: the same noisy closed loop run by two controllers on the stage
    kernel, the second with the keyword overrides `kw`; per step (Z_a, Z_b, it_a, it_b, defect_b)."""
    a = make_controller(cfg, bt, lib=lib, transcription="MultipleShooting")
    b_ = make_controller(cfg, bt, lib=lib, transcription="MultipleShooting", **kw)
    for c in (a, b_):
        c.lastu0 = bt["lastu0"].copy()
    x = bt["xhat0"].copy()
    rg = np.random.default_rng(seed)
    out = []
    for k in range(steps):
        ua = mcu.no_fallback_step(a, x, bt["ry"])
        mcu.no_fallback_step(b_, x, bt["ry"])
        on_stage_kernel(a); on_stage_kernel(b_)
        out.append((a.Z.copy(), b_.Z.copy(), a.iters.copy(), b_.iters.copy(), float(b_.hd.get(api.GET_MS_DEFECT).max())))
        x = (np.einsum("bij,bj->bi", bt["Ahat"], x) + np.einsum("bij,bj->bi", bt["Bhu"], ua)
             + noise * rg.standard_normal(x.shape))
        b_.lastu0 = a.lastu0.copy()      # keep the two loops on the same trajectory
    return out


def fused_loop_warm_dual(lib=None, B=3, periods=4, torch_device=None):
    """mpcqp_loop_device against the three separate entry points on a MultipleShooting handle with MPCQP_FLAG_WARM_DUAL
    (the shape of ms_custom_util.fused_loop_custom, custom rows included): max |difference| of x̂0, u0, Z̃ and of the
    iteration counts over the periods (expected 0), and whether any period after the first took another number of
    iterations than the same handle without the flag (the multipliers are in use)."""
    cfg = synth.Config("loopw", nx=3, nu=2, ny=2, Hp=8, Hc=3, umin=-0.6, umax=0.7, ymax=0.9)
    bt = synth.make_batch(cfg, B, seed=12)
    K = mpcqp.steady_kalman_gain(bt["Ahat"], bt["Chat"], np.eye(cfg.nxh), np.eye(cfg.ny))
    nw = 2
    Wy = np.array([[1.0, -0.5], [0.3, 0.8]]); Wu = np.array([[0.4, 0.0], [-0.6, 1.0]])

    def make(flags):
        hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, cfg.Hc, neps=1, flags=mpcqp.FLAG_RY_CONSTANT | flags, lib=lib)
        hd.set_transcription(api.MULTIPLE_SHOOTING)
        hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
        hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt), np.full(B, cfg.Cwt))
        hd.set_bounds(U0min=np.full((B, hd.nU), cfg.umin), U0max=np.full((B, hd.nU), cfg.umax), Y0max=np.full((B, hd.nY), cfg.ymax))
        hd.set_custom_constraints(nw, mpcqp.colmajor(mcu.rep(Wy, B)), mpcqp.colmajor(mcu.rep(Wu, B)))
        nW = nw * (cfg.Hp + 1)
        hd.set_custom_bounds(np.tile([-0.5, -np.inf], (B, cfg.Hp + 1)), np.tile([0.5, 0.4], (B, cfg.Hp + 1)),
                             np.ones((B, nW)), np.full((B, nW), 0.5))
        hd.kf_set(mpcqp.colmajor(K), np.arange(cfg.ny))
        assert hd.transcription_supported() == 0
        assert hd.prepare() == api.KERNEL_MS
        return hd

    if torch_device is None:
        new = lambda a: np.ascontiguousarray(a).copy()
        ptr = lambda a: a.ctypes.data
        host = lambda a: a
        sync = lambda: None
    else:
        import torch
        new = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch_device)
        ptr = lambda a: a.data_ptr()
        host = lambda a: a.cpu().numpy()
        sync = torch.cuda.synchronize
    runs = []
    for fused, flags in ((False, api.FLAG_WARM_DUAL), (True, api.FLAG_WARM_DUAL), (True, 0)):
        hd = make(flags)
        x = new(bt["xhat0"]); lu = new(bt["lastu0"]); ry = new(bt["ry"])
        Z = new(np.zeros((B, hd.nZ))); u0 = new(np.zeros((B, cfg.nu)))
        st = new(np.zeros(B, np.int32)); it = new(np.zeros(B, np.int32))
        rg = np.random.default_rng(7)
        out = []
        for k in range(periods):
            y = new(0.3 * rg.standard_normal((B, cfg.ny)))
            if fused:
                hd.loop_device(ptr(x), ptr(y), ptr(lu), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
            else:
                hd.kf_correct_device(ptr(x), ptr(y))
                hd.step_device(ptr(x), ptr(lu), ptr(ry), ptr(Z), ptr(u0), ptr(st), iters=ptr(it))
                hd.kf_predict_device(ptr(x), ptr(u0))
            sync()
            assert np.all(host(st) == 0)
            out.append((host(x).copy(), host(u0).copy(), host(Z).copy(), host(it).astype(float)))
            lu, u0 = u0, lu
        runs.append(out)
    diff = max(float(np.abs(a - b).max()) for pa, pb in zip(runs[0], runs[1]) for a, b in zip(pa, pb))
    used = any(np.any(pa[3] != pb[3]) for pa, pb in zip(runs[1][1:], runs[2][1:]))
    return diff, used


def warm_dual_validity(lib, change):
    """A warm_dual controller steps once, then `change(g)` is applied (a setter after which stored multipliers must not be
    used), then it steps again; a fresh controller that has seen the same `change` takes the second step from the same
    primal warm start.  Returns (max |ΔZ̃| between the two second steps, iteration counts equal, whether the unchanged
    warm_dual controller's second step differs from the fresh one's -- the multipliers are in use when nothing resets them)."""
    cfg, B = WARM_CFG, 2
    bt = synth.make_batch(cfg, B, seed=2)
    x2 = np.einsum("bij,bj->bi", bt["Ahat"], bt["xhat0"]) + 0.05

    def first():
        g = make_controller(cfg, bt, lib=lib, transcription="MultipleShooting", warm_dual=True)
        g.lastu0 = bt["lastu0"].copy()
        mcu.no_fallback_step(g, bt["xhat0"], bt["ry"])
        on_stage_kernel(g)
        return g

    def second(g):
        mcu.no_fallback_step(g, x2, bt["ry"])
        on_stage_kernel(g)
        return g.Z.copy(), g.iters.copy()

    kept, changed = first(), first()
    Z1, lu1 = changed.Z.copy(), changed.lastu0.copy()
    change(changed)
    fresh = make_controller(cfg, bt, lib=lib, transcription="MultipleShooting", warm_dual=True)
    change(fresh)
    fresh.Z[:] = Z1; fresh.lastu0 = lu1.copy()
    (Zc, itc), (Zf, itf) = second(changed), second(fresh)
    Zk, itk = second(kept)
    return float(np.abs(Zc - Zf).max()), bool(np.all(itc == itf)), bool(np.any(itk != itf) or np.any(Zk != Zf))


# ---- kept q̃ / F ----------------------------------------------------------------------------------------------------
def kept_qp_errors(g, o, i=0):
    """Relative error of MPCQP_GET_FVEC / MPCQP_GET_QTILDE of member i against the oracle's F, q̃ (after its initpred), in
    the measure of tests/test_gpu_parity.py::test_condensation_tables_match_oracle."""
    F, q = g.hd.get(api.GET_FVEC)[i], g.hd.get(api.GET_QTILDE)[i]
    return (float(np.abs(F - o.F).max() / max(1.0, np.abs(o.F).max())),
            float(np.abs(q - o.qt).max() / max(1.0, np.abs(o.qt).max())))


def kept_qp_beyond_lds(lib=None, B=1):
    """SingleShooting 3,4,2,46,46 with keep_qp (the condensed carve takes 185 KB of LDS: the stage kernel runs it): returns
    (F error, q̃ error) of member 0."""
    cfg = synth.get_config("3,4,2,46,46")
    bt = synth.make_batch(cfg, B, seed=11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")               # (the reroute to the stage kernel is announced: expected here)
        g = make_controller(cfg, bt, lib=lib, keep_qp=True)
        g.lastu0 = bt["lastu0"].copy()
        g.moveinput(bt["xhat0"], bt["ry"])
    on_stage_kernel(g)
    o = make_oracle(cfg, bt, 0)
    o.initpred(bt["xhat0"][0], bt["lastu0"][0], bt["ry"][0])
    return kept_qp_errors(g, o)


def kept_qp_with_blocks(lib=None, B=2):
    """The block-weight controller under MultipleShooting with keep_qp and a non-zero R̂u: the dense-L term of q̃."""
    A, Bu, C, x0, kw, con = blocks_plant()
    kw = dict(kw, **block_weights(8, 4, "MNL"))
    g = mpcqp.BatchLinMPC(mcu.rep(A, B), mcu.rep(Bu, B), mcu.rep(C, B), lib=lib, transcription="MultipleShooting",
                          keep_qp=True, **kw)
    g.setconstraint(**con)
    lu = np.array([0.3, -0.2])
    Ru = 0.3 * np.random.default_rng(9).standard_normal(16)
    g.lastu0 = mcu.rep(lu, B)
    mcu.no_fallback_step(g, np.tile(x0, (B, 1)), [2.5, 0.4], Rhatu=Ru)
    on_stage_kernel(g)
    o = cd.LinMPCOracle(A, Bu, C, **kw)
    o.setconstraint(**con)
    o.initpred(x0, lu, [2.5, 0.4], Rhatu=Ru)
    return kept_qp_errors(g, o, B - 1)


def kept_qp_with_disturbance(lib=None, B=2):
    """The block-weight controller under MultipleShooting with keep_qp and a measured disturbance (nd = 1, B̂d and D̂d
    non-zero, a D̂ that varies over the horizon): the D̂d D̂0 term of F, and R̂y - D̂d D̂0 in the gradient q̃."""
    A, Bu, C, x0, kw, con = blocks_plant()
    kw = dict(kw, **block_weights(8, 4, "MNL"))
    rng = np.random.default_rng(13)
    Bd, Dd = rng.standard_normal((3, 1)), rng.standard_normal((2, 1))
    d, Dhat = np.array([0.7]), 0.7 + 0.4 * rng.standard_normal(8)
    lu = np.array([0.3, -0.2])
    g = mpcqp.BatchLinMPC(mcu.rep(A, B), mcu.rep(Bu, B), mcu.rep(C, B), mcu.rep(Bd, B), mcu.rep(Dd, B), lib=lib,
                          transcription="MultipleShooting", keep_qp=True, **kw)
    g.setconstraint(**con)
    g.lastu0 = mcu.rep(lu, B)
    mcu.no_fallback_step(g, np.tile(x0, (B, 1)), [2.5, 0.4], d, Dhat=Dhat)
    on_stage_kernel(g)
    o = cd.LinMPCOracle(A, Bu, C, Bd, Dd, **kw)
    o.setconstraint(**con)
    o.initpred(x0, lu, [2.5, 0.4], d, Dhat)
    no_d = cd.LinMPCOracle(A, Bu, C, **kw)
    no_d.initpred(x0, lu, [2.5, 0.4])
    moved = min(float(np.abs(o.F - no_d.F).max()), float(np.abs(o.qt - no_d.qt).max()))     # what ignoring d would cost
    o.lastu0 = lu.copy()
    o.moveinput(x0, [2.5, 0.4], d, Dhat=Dhat)
    assert o.status == 0
    return kept_qp_errors(g, o, B - 1), moved, rel_to_oracle(g, o, B - 1)


# ---- beyond the LDS with everything ------------------------------------------------------------------------------------
def spd_blocks(rng, n, k, scale, diag):
    """blkdiag of k SPD n x n blocks."""
    W = np.zeros((n * k, n * k))
    for j in range(k):
        R = rng.standard_normal((n, n))
        W[j * n:(j + 1) * n, j * n:(j + 1) * n] = scale * (R @ R.T) / n + diag * np.eye(n)
    return W


def beyond_lds_with_everything(lib=None, B=2, check=(0, 1), periods=2, seed=21):
    """SingleShooting 12,4,4,46,46 (nZ̃ = 185, beyond the LDS of a CU) with stage-separable M / N / L blocks, warm_dual,
    keep_qp and the two soft custom rows of ms_custom_util.beyond_lds_with_custom_rows, `periods` closed-loop periods.
    Returns dict(worst difference of the checked members to the oracle, kept F / q̃ error of the first checked member)."""
    cfg = synth.get_config("12,4,4,46,46")
    bt = synth.make_batch(cfg, B, seed=11)
    rng = np.random.default_rng(3)
    Wy, Wu = 0.5 * rng.standard_normal((2, cfg.ny)), 0.5 * rng.standard_normal((2, cfg.nu))
    rw = np.random.default_rng(seed)
    kw = dict(Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt, Wy=Wy, Wu=Wu,
              M_Hp=spd_blocks(rw, cfg.ny, cfg.Hp, 0.5 * cfg.Mwt, cfg.Mwt),
              N_Hc=spd_blocks(rw, cfg.nu, cfg.Hc, 0.5 * cfg.Nwt, cfg.Nwt),
              L_Hp=spd_blocks(rw, cfg.nu, cfg.Hp, 0.02, 0.01))
    wcon = dict(wmin=[-0.8, -np.inf], wmax=[0.8, 0.6])
    if np.isfinite(cfg.Cwt):
        wcon.update(c_wmin=[1.0, 0.5], c_wmax=[1.0, 0.5])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")               # (the reroute to the stage kernel is announced: expected here)
        g = mpcqp.BatchLinMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], lib=lib, warm_dual=True, keep_qp=True, **kw)
        g.setconstraint(**constraint_kwargs(cfg), **wcon)
    g.lastu0 = bt["lastu0"].copy()
    orcs = {}
    for i in check:
        o = cd.LinMPCOracle(bt["Ahat"][i], bt["Bhu"][i], bt["Chat"][i], **kw)
        o.setconstraint(**constraint_kwargs(cfg, oracle=True), **wcon)
        o.lastu0 = bt["lastu0"][i].copy()
        orcs[i] = o
    x = bt["xhat0"].copy()
    out = dict(worst=0.0, keep=(0.0, 0.0))
    for k in range(periods):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            u = g.moveinput(x, bt["ry"])
        on_stage_kernel(g)
        for i, o in orcs.items():
            o.moveinput(x[i], bt["ry"][i])
            assert o.status == 0, (k, i, o.status)
            out["worst"] = max(out["worst"], rel_to_oracle(g, o, i))
        e = kept_qp_errors(g, orcs[check[0]], check[0])
        out["keep"] = (max(out["keep"][0], e[0]), max(out["keep"][1], e[1]))
        x = np.einsum("bij,bj->bi", bt["Ahat"], x) + 0.5 * np.einsum("bij,bj->bi", bt["Bhu"], u)
    return out


# ---- unstable plants -----------------------------------------------------------------------------------------------------
def unstable_plant_warm_blocks(lib=None, B=16, check=(0, 4, 8, 12), periods=3):
    """parity_util.unstable_plant_members under MultipleShooting with warm_dual and an N_Hc of SPD 2 x 2 blocks: closed loop,
    the plants driven by the returned inputs.  Returns dict(worst difference of the checked members, defect)."""
    mem = unstable_plant_members(B)
    st = lambda f: np.stack([f(m) for m in mem])
    nu = mem[0]["Bhu"].shape[1]
    kw = dict(mem[0]["kw"])
    kw.pop("Nwt")
    kw["N_Hc"] = spd_blocks(np.random.default_rng(5), nu, kw["Hc"], 0.05, 0.1)
    c = mem[0]["con"]
    g = mpcqp.BatchLinMPC(st(lambda m: m["Ah"]), st(lambda m: m["Bhu"]), st(lambda m: m["Ch"]), lib=lib,
                          transcription="MultipleShooting", warm_dual=True, **kw)
    g.setconstraint(umin=c["umin"], umax=c["umax"], Δumin=c["dumin"], Δumax=c["dumax"], ymax=c["ymax"])
    orcs = {}
    for i in check:
        o = cd.LinMPCOracle(mem[i]["Ah"], mem[i]["Bhu"], mem[i]["Ch"], **kw)
        o.setconstraint(**c)
        o.lastu0 = np.zeros(nu)
        orcs[i] = o
    x, ry = st(lambda m: m["x0"]), st(lambda m: m["ry"])
    out = dict(worst=0.0, defect=0.0)
    for k in range(periods):
        u = mcu.no_fallback_step(g, x, ry)
        on_stage_kernel(g)
        out["defect"] = max(out["defect"], float(g.hd.get(api.GET_MS_DEFECT).max()))
        for i, o in orcs.items():
            o.moveinput(x[i], ry[i])
            assert o.status == 0, (k, i, o.status)
            out["worst"] = max(out["worst"], rel_to_oracle(g, o, i))
        x = np.einsum("bij,bj->bi", st(lambda m: m["Ah"]), x) + np.einsum("bij,bj->bi", st(lambda m: m["Bhu"]), u)
    return out


def add_output_lower_bounds(g):
    """A row group more (Y0min) on the handle of a WARM_CFG controller: the stage kernel's row layout changes."""
    cfg, B, hd = WARM_CFG, g.B, g.hd
    hd.set_bounds(U0min=np.full((B, hd.nU), cfg.umin), U0max=np.full((B, hd.nU), cfg.umax),
                  Y0max=np.full((B, hd.nY), cfg.ymax), Y0min=np.full((B, hd.nY), -5.0))
