"""Helpers of the time-varying KalmanFilter tests (covariance / gain recursion of csrc/kf_cov_bodies.h behind the LinMPC
loop): a NumPy batch recursion written from the reference (src/estimator/kalman.jl:1235-1264 correct_estimate_kf!,
1275-1290 predict_estimate_kf!) with the drop policy of include/mpcqp.h, the shapes of the tests and their case runners.  On the CPU
the launcher is tests/emu/emu_kf_cov.cpp in tests/emu/libmpcqp_emu_est.so (tests/emu_util.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mpcqp  # noqa: E402
from mpcqp import synth  # noqa: E402

BAR = 1e-11         # K̂ and P̂ against the NumPy recursion, relative to max(1, max|.|) (see tests/test_gpu_kf_cov.py)


class NumpyKalmanCov:
    """P̂, K̂ and the status of B independent KalmanFilters, in the reference's order of operations; the corrected P̂ is kept as
    ½ (P̂ + P̂') like oracle/mhe.py.  A correction whose M̂ has no Cholesky factor or is not finite, or whose result is not
    finite, is dropped (status 2: P̂ and K̂ stay, and so does P̂ in the prediction of that period)."""

    def __init__(self, Qhat, Rhat, P0, i_ym):
        self.P = np.array(P0, float)
        B, n, _ = self.P.shape
        self.Q = np.broadcast_to(np.asarray(Qhat, float), (B, n, n)).copy()
        self.i_ym = np.asarray(i_ym, int)
        nym = len(self.i_ym)
        self.R = np.broadcast_to(np.asarray(Rhat, float), (B, nym, nym)).copy()
        self.K = np.zeros((B, n, nym))
        self.status = np.zeros(B, np.int32)

    def correct(self, Chat):
        for b in range(len(self.P)):
            Cm, P = Chat[b][self.i_ym], self.P[b]
            PCt = P @ Cm.T
            M = Cm @ PCt + self.R[b]
            ok = bool(np.isfinite(M).all())
            if ok:
                try:
                    np.linalg.cholesky(M)
                except np.linalg.LinAlgError:
                    ok = False
            if ok:
                K = np.linalg.solve(M.T, PCt.T).T              # rdiv!(K̂, cholesky(M̂))
                Pn = (np.eye(P.shape[0]) - K @ Cm) @ P
                Pn = 0.5 * (Pn + Pn.T)
                ok = bool(np.isfinite(Pn).all() and np.isfinite(K).all())
            if ok:
                self.P[b], self.K[b] = Pn, K
            self.status[b] = 0 if ok else 2

    def predict(self, Ahat):
        for b in range(len(self.P)):
            if self.status[b] == 2:
                continue
            Pn = Ahat[b] @ (self.P[b] @ Ahat[b].T) + self.Q[b]
            if np.isfinite(Pn).all():
                self.P[b] = Pn
            else:
                self.status[b] = 2


def rel(got, want):
    """max |got - want| relative to max(1, max |want|)."""
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, float(np.abs(want).max())))


# ---------------------------------------------------------------------------------------------
# shapes: dict(nxh, nu, ny, nd, i_ym, Ahat, Bhu, Chat, Bhd, Dhd, Qhat, Rhat, P0)
def _covs(rng, B, nxh, nym):
    """Dense symmetric positive definite Q̂, R̂, P̂_0 per member (a diagonal one would hide a transposed operand)."""
    def spd(n, lo, hi):
        G = rng.standard_normal((B, n, n)) / np.sqrt(n)
        M = 0.3 * G @ G.transpose(0, 2, 1) + np.eye(n) * rng.uniform(lo, hi, (B, 1, 1))
        return 0.5 * (M + M.transpose(0, 2, 1))
    return spd(nxh, 0.01, 0.05), spd(nym, 0.02, 0.1), spd(nxh, 0.5, 1.5)


def shape_linmpc(cfg, B, seed, i_ym=None, nd=0):
    """A LinMPC workload of modelpredictivecontrol.jl_amd/synth.py (C2, C3, ...), optionally with nd measured disturbances."""
    bt = synth.make_batch(cfg, B, seed=seed)
    rng = np.random.default_rng([seed, 77])
    i_ym = list(range(cfg.ny)) if i_ym is None else list(i_ym)
    Q, R, P0 = _covs(rng, B, cfg.nxh, len(i_ym))
    Bhd = Dhd = None
    if nd:
        Bhd = np.zeros((B, cfg.nxh, nd)); Bhd[:, :cfg.nx] = rng.standard_normal((B, cfg.nx, nd)) / np.sqrt(cfg.nx)
        Dhd = 0.1 * rng.standard_normal((B, cfg.ny, nd))
    return dict(nxh=cfg.nxh, nu=cfg.nu, ny=cfg.ny, nd=nd, i_ym=i_ym, Ahat=bt["Ahat"], Bhu=bt["Bhu"], Chat=bt["Chat"], Bhd=Bhd,
                Dhd=Dhd, Qhat=Q, Rhat=R, P0=P0, cfg=cfg, bt=bt)


def shape_mhe(mcfg, B, seed):
    """The augmented model of an MHE workload of synth.py (nx̂ = nx + nym: the wide shapes) with dense covariances."""
    bt = synth.make_mhe_batch(mcfg, B, seed=seed)
    rng = np.random.default_rng([seed, 78])
    Q, R, P0 = _covs(rng, B, mcfg.nxh, mcfg.nym)
    nd = mcfg.nd
    return dict(nxh=mcfg.nxh, nu=mcfg.nu, ny=mcfg.nym, nd=nd, i_ym=list(range(mcfg.nym)), Ahat=bt["Ahat"], Bhu=bt["Bhu"],
                Chat=bt["Chm"], Bhd=bt["Bhd"] if nd else None, Dhd=bt["Dhdm"] if nd else None, Qhat=Q, Rhat=R, P0=P0)


CFG_YM = synth.Config("ny=3, i_ym=[2,0], nd=1", nx=4, nu=2, ny=3, Hp=6, Hc=2)      # nx̂ = 7 (NX = 8), two of three outputs measured
MHE17 = synth.MheConfig("kf nx̂=17", nx=14, nu=2, nym=3, nd=0, He=1)                 # NX = 24
MHE32 = synth.MheConfig("kf nx̂=32", nx=26, nu=2, nym=6, nd=1, He=1)                 # NX = 32


def shape_c2(B=6, seed=21): return shape_linmpc(synth.C2, B, seed)
def shape_c3(B=7, seed=21): return shape_linmpc(synth.C3, B, seed)
def shape_ym(B=5, seed=21): return shape_linmpc(CFG_YM, B, seed, i_ym=[2, 0], nd=1)
def shape_17(B=3, seed=5): return shape_mhe(MHE17, B, seed)
def shape_32(B=3, seed=5): return shape_mhe(MHE32, B, seed)


def make_handle(sh, lib=None, Hp=2, Hc=1):
    """A raw C-ABI handle with the shape's model and the time-varying filter attached (no weights: estimator calls only)."""
    B = sh["Ahat"].shape[0]
    h = mpcqp.api.Handle(B, sh["nxh"], sh["nu"], sh["ny"], sh["nd"], Hp, Hc, lib=lib)
    cm = mpcqp.api.colmajor
    h.set_model(cm(sh["Ahat"]), cm(sh["Bhu"]), cm(sh["Chat"]), None if not sh["nd"] else cm(sh["Bhd"]), None if not sh["nd"] else cm(sh["Dhd"]))
    h.kf_set_covariances(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
    return h


def run_recursion(sh, nper, lib=None, seed=0):
    """nper periods of kf_correct + kf_predict (host pointers) on a handle of the shape against NumpyKalmanCov and, for x̂,
    against the NumPy filter driven by NumPy's gains.  Returns the worst relative errors of K̂, P̂ and x̂ over all periods
    and the handle."""
    h = make_handle(sh, lib=lib)
    B, nxh, nd = sh["Ahat"].shape[0], sh["nxh"], sh["nd"]
    ref = NumpyKalmanCov(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
    rng = np.random.default_rng([seed, 9])
    x = rng.standard_normal((B, nxh)); xr = x.copy()
    eK = eP = ex = 0.0
    for _ in range(nper):
        y, u = rng.standard_normal((B, len(sh["i_ym"]))), rng.standard_normal((B, sh["nu"]))
        d = rng.standard_normal((B, nd)) if nd else None
        h.kf_correct(x, y, d)
        ref.correct(sh["Chat"])
        for b in range(B):
            v = y[b] - sh["Chat"][b][sh["i_ym"]] @ xr[b] - (sh["Dhd"][b][sh["i_ym"]] @ d[b] if nd else 0.0)
            xr[b] = xr[b] + ref.K[b] @ v
        eK, eP, ex = max(eK, rel(h.kf_gain(), ref.K)), max(eP, rel(h.kf_covariance(), ref.P)), max(ex, rel(x, xr))
        h.kf_predict(x, u, d)
        ref.predict(sh["Ahat"])
        for b in range(B):
            xr[b] = sh["Ahat"][b] @ xr[b] + sh["Bhu"][b] @ u[b] + (sh["Bhd"][b] @ d[b] if nd else 0.0)
        eP, ex = max(eP, rel(h.kf_covariance(), ref.P)), max(ex, rel(x, xr))
    assert np.array_equal(h.kf_status(), ref.status) and not ref.status.any()
    return dict(eK=eK, eP=eP, ex=ex), h


def closed_loop(cfg, B, seed, nper, swaps=(), lib=None, check_u=True):
    """The (b) part of tests/test_gpu_parity.py::test_kalman_closed_loop_on_gpu with the time-varying filter: a batch of
    controllers with preparestate / moveinput / updatestate on the product against the oracle controller fed by the NumPy
    filter.  `swaps`: periods after which setmodel installs Â scaled by 0.9 and a perturbed B̂u (the NumPy filter and the
    oracle's state recursion get the same model; the oracle controller is not rebuilt, so u is compared up to the first swap
    only).  Returns the worst errors of u, x̂, K̂, P̂ (relative, see rel()), a second NumPy filter that never saw a swap, the
    product and the step statuses seen."""
    from tests.parity_util import make_controller, make_oracle
    sh = shape_linmpc(cfg, B, seed)
    bt = sh["bt"]
    gpu = make_controller(cfg, bt, lib=lib)
    gpu.setestimator(covariances=dict(Qhat=sh["Qhat"], Rhat=sh["Rhat"], P0=sh["P0"]), xhat0=bt["xhat0"])
    gpu.lastu0 = bt["lastu0"].copy()
    orcs = [make_oracle(cfg, bt, i) for i in range(B)]
    for i in range(B):
        orcs[i].lastu0 = bt["lastu0"][i].copy()
    ref = NumpyKalmanCov(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
    stale = NumpyKalmanCov(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
    A, Bu, A0 = bt["Ahat"].copy(), bt["Bhu"].copy(), bt["Ahat"].copy()
    xo, xp = bt["xhat0"].copy(), bt["xhat0"].copy()            # "plant" = the augmented model itself
    rng = np.random.default_rng(0)
    eu = ex = eK = eP = 0.0
    swapped = False
    statuses = []
    for k in range(nper):
        y = np.einsum("bij,bj->bi", bt["Chat"], xp) + 0.02 * rng.standard_normal((B, cfg.ny))
        gpu.preparestate(y)
        ref.correct(bt["Chat"]); stale.correct(bt["Chat"])
        eK, eP = max(eK, rel(gpu.hd.kf_gain(), ref.K)), max(eP, rel(gpu.hd.kf_covariance(), ref.P))
        ug = gpu.moveinput(None, bt["ry"])
        statuses.append(gpu.status.copy())
        for i in range(B):
            xo[i] = xo[i] + ref.K[i] @ (y[i] - bt["Chat"][i] @ xo[i])
            if check_u and not swapped:
                eu = max(eu, float(np.abs(ug[i] - orcs[i].moveinput(xo[i], bt["ry"][i])).max()))
            xo[i] = A[i] @ xo[i] + Bu[i] @ ug[i]
        gpu.updatestate(ug, y)
        ref.predict(A); stale.predict(A0)
        ex = max(ex, float(np.abs(gpu.xhat0 - xo).max() / max(1.0, np.abs(xo).max())))
        eP = max(eP, rel(gpu.hd.kf_covariance(), ref.P))
        xp = np.einsum("bij,bj->bi", A, xp) + np.einsum("bij,bj->bi", Bu, ug)
        if k + 1 in swaps:              # setmodel!: picked up by the next covariance launch with nothing else to call
            A = 0.9 * A
            Bu = Bu + 0.05 * rng.standard_normal(Bu.shape) * (np.abs(Bu) > 0)
            gpu.setmodel(A, Bu, bt["Chat"])
            swapped = True
    return dict(eu=eu, ex=ex, eK=eK, eP=eP), ref, stale, gpu, np.array(statuses)


def fused_vs_separate(B=64, periods=5, torch_device=None, multiple_shooting=False, lib=None):
    """tests/parity_util.fused_loop_vs_separate_steps on a time-varying handle: mpcqp_loop_device against kf_correct_device +
    step_device + kf_predict_device on the same resident data.  Returns the largest |difference| of x̂0, u0, Z̃, P̂ and K̂ over
    the periods (the same arithmetic: expected exactly 0) and the largest |K̂| seen (the filter did run)."""
    cfg = synth.Config("loop", nx=3, nu=2, ny=2, Hp=8, Hc=3, umin=-0.6, umax=0.7, ymax=0.9)
    sh = shape_linmpc(cfg, B, 12)
    bt = sh["bt"]

    def make():
        hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, cfg.Hc, neps=1,
                          flags=mpcqp.FLAG_RY_CONSTANT | (0 if multiple_shooting else mpcqp.FLAG_KEEP_QP), lib=lib)
        if multiple_shooting:
            hd.set_transcription(mpcqp.api.MULTIPLE_SHOOTING)
        hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
        hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt), np.full(B, cfg.Cwt))
        hd.set_bounds(U0min=np.full((B, hd.nU), cfg.umin), U0max=np.full((B, hd.nU), cfg.umax), Y0max=np.full((B, hd.nY), cfg.ymax))
        hd.kf_set_covariances(sh["Qhat"], sh["Rhat"], sh["P0"], sh["i_ym"])
        hd.prepare()
        return hd

    if torch_device is None:
        new, ptr, host, sync = (lambda a: np.ascontiguousarray(a).copy()), (lambda a: a.ctypes.data), (lambda a: a), (lambda: None)
    else:
        import torch
        new = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch_device)
        ptr, host, sync = (lambda a: a.data_ptr()), (lambda a: a.cpu().numpy()), torch.cuda.synchronize
    runs, kmax = [], 0.0
    for fused in (False, True):
        hd = make()
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
            assert np.all(host(st) == 0) and not hd.kf_status().any()
            out.append((host(x).copy(), host(u0).copy(), host(Z).copy(), hd.kf_covariance(), hd.kf_gain()))
            kmax = max(kmax, float(np.abs(out[-1][4]).max()))
            lu, u0 = u0, lu                      # u0 of this period is lastu0 of the next
        runs.append(out)
    return max(float(np.abs(a - b).max()) for pa, pb in zip(*runs) for a, b in zip(pa, pb)), kmax
