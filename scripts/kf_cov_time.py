"""Timing of the time-varying KalmanFilter of the LinMPC loop on resident data (HIP event timing around the launches):
  * `cov`:    the covariance / gain kernel alone (csrc/kf_kernels.hip, mode 3: correction + prediction of one period),
  * `loop`:   the fused loop period (mpcqp_loop_device) with the steady gain and with the time-varying filter,
  * `dare`:   the host-side alternative per model swap -- B SciPy DARE solves (steady_kalman_gain) plus the upload of K̂,
  * `forms`:  the fused loop period in the predictor form (mpcqp_kf_set_direct(0): step, correction, prediction) on the same
              data as `loop`, and kf_update_device (one covariance launch) against kf_correct_device + kf_predict_device (two).
One JSON line per measurement.  A library without mpcqp_kf_set_covariances (an older build) gives the steady loop only, so
the same script measures the yardstick on the parent commit.
Usage: python scripts/kf_cov_time.py [cov] [loop] [dare] [forms] [B ...] [nxh16|nxh24|nxh32 ...]   (defaults: everything; C3 shapes at
B = 65536 and 1024, nx̂ = 24 and 32 at B = 16384)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mpcqp  # noqa: E402
from mpcqp import synth  # noqa: E402

HAVE_TV = hasattr(mpcqp.Handle, "kf_set_covariances")
HAVE_DIRECT = hasattr(mpcqp.Handle, "kf_set_direct")
WARM, REPS = 3, 10
DEV = torch.device("cuda", 0)
WIDE = {24: dict(nx=20, nym=4), 32: dict(nx=26, nym=6)}


def covariances(rng, B, nxh, nym):
    def spd(n, lo, hi):
        G = rng.standard_normal((B, n, n)) / np.sqrt(n)
        return 0.3 * G @ G.transpose(0, 2, 1) + np.eye(n) * rng.uniform(lo, hi, (B, 1, 1))
    return spd(nxh, 0.01, 0.05), spd(nym, 0.02, 0.1), spd(nxh, 0.5, 1.5)


def model(nxh, B):
    """C3 itself at nx̂ = 16; above, the augmented model of an MHE workload of that size (estimator calls only)."""
    if nxh == 16:
        cfg = synth.C3
        bt = synth.make_batch(cfg, B, seed=0)
        return cfg, bt, bt["Ahat"], bt["Bhu"], bt["Chat"], cfg.ny
    mc = synth.MheConfig(f"kf{nxh}", nu=2, nd=0, He=1, **WIDE[nxh])
    bt = synth.make_mhe_batch(mc, B, seed=0)
    return None, bt, bt["Ahat"], bt["Bhu"], bt["Chm"], mc.nym


def timed(fn):
    """Median and minimum of REPS event-timed calls after WARM warm-up calls, ms."""
    s = torch.cuda.current_stream()
    for _ in range(WARM):
        fn(s.cuda_stream)
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(s.cuda_stream); e1.record(s)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def cov_alone(nxh, B):
    """The covariance kernel alone: kf_correct_device + kf_predict_device launch it around the two x̂ kernels, so the period
    of a handle in time-varying mode minus the same two calls on a steady handle is the kernel (both are reported)."""
    _, bt, A, Bu, C, ny = model(nxh, B)
    nu = Bu.shape[2]
    rng = np.random.default_rng(1)
    Q, R, P0 = covariances(rng, B, nxh, ny)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    x, y, u = T(np.zeros((B, nxh))), T(rng.standard_normal((B, ny))), T(rng.standard_normal((B, nu)))
    out = {}
    for tv in (False, True):
        hd = mpcqp.Handle(B, nxh, nu, ny, 0, 2, 1)
        hd.set_model(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(C))
        if tv:
            hd.kf_set_covariances(Q, R, P0, np.arange(ny))
        else:
            hd.kf_set(np.zeros((B, ny, nxh)), np.arange(ny))
        def period(sp):
            hd.kf_correct_device(x.data_ptr(), y.data_ptr(), stream=sp)
            hd.kf_predict_device(x.data_ptr(), u.data_ptr(), stream=sp)
        out[tv] = timed(period)
        if tv:
            bad = int((hd.kf_status() != 0).sum())
            lanes = hd.kf_lanes_per_estimator()
    nbytes = 8 * B * (4 * nxh * nxh + 2 * ny * nxh + ny * ny)         # Â, Q̂, P̂ in and out, Ĉm, K̂, R̂
    dt = out[True][0] - out[False][0]
    return dict(what="cov", nxh=nxh, nym=ny, B=B, lanes=lanes, correct_predict_steady_ms=round(out[False][0], 4),
                correct_predict_tv_ms=round(out[True][0], 4), cov_two_launches_ms=round(dt, 4), bytes_per_estimator=nbytes // B,
                gbytes_per_s=round(nbytes / max(dt, 1e-9) / 1e6, 1), dropped=bad)


def loop_period(B, direct=True):
    """mpcqp_loop_device at C3 shapes, warm-started closed loop against the augmented model as the plant: steady gain and
    time-varying filter on the same data.  direct=False: the predictor form."""
    cfg, bt, A, Bu, C, ny = model(16, B)
    nxh, nu = cfg.nxh, cfg.nu
    rng = np.random.default_rng(1)
    Q, R, P0 = covariances(rng, B, nxh, ny)
    nK = min(B, 256)                                                  # DARE on the host for a sample, models tiled to match
    for k in ("Ahat", "Bhu", "Chat"):
        bt[k] = np.tile(bt[k][:nK], (B // nK + 1, 1, 1))[:B]
    K = np.tile(mpcqp.steady_kalman_gain(bt["Ahat"][:nK], bt["Chat"][:nK], Q[0], R[0]), (B // nK + 1, 1, 1))[:B]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    res = {}
    for tv in ([False, True] if HAVE_TV else [False]):
        hd = mpcqp.Handle(B, nxh, nu, ny, 0, cfg.Hp, cfg.Hc, neps=1, flags=mpcqp.FLAG_RY_CONSTANT | mpcqp.FLAG_WARM_DUAL)
        hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
        hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt), np.full(B, cfg.Cwt))
        hd.set_bounds(U0min=np.full((B, hd.nU), cfg.umin), U0max=np.full((B, hd.nU), cfg.umax), Y0max=np.full((B, hd.nY), cfg.ymax))
        if tv:
            hd.kf_set_covariances(np.broadcast_to(Q[0], Q.shape), np.broadcast_to(R[0], R.shape), P0, np.arange(ny))
        else:
            hd.kf_set(mpcqp.colmajor(K), np.arange(ny))
        if not direct:
            hd.kf_set_direct(False)
        hd.prepare()
        Ad, Bd, Cd = T(bt["Ahat"]), T(bt["Bhu"]), T(bt["Chat"])
        xp = T(bt["xhat0"]).unsqueeze(2)
        xh, lu, ry = T(np.zeros((B, nxh))), T(bt["lastu0"]), T(bt["ry"])
        Z, u0 = T(np.zeros((B, hd.nZ))), T(np.zeros((B, nu)))
        st, it = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
        gen = torch.Generator(device=DEV); gen.manual_seed(0)
        s = torch.cuda.current_stream()
        ms, iters = [], []
        for k in range(WARM + REPS):
            y = torch.bmm(Cd, xp).squeeze(2) + 0.02 * torch.randn((B, ny), dtype=torch.float64, device=DEV, generator=gen)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            hd.loop_device(xh.data_ptr(), y.data_ptr(), lu.data_ptr(), ry.data_ptr(), Z.data_ptr(), u0.data_ptr(), st.data_ptr(),
                           iters=it.data_ptr(), stream=s.cuda_stream)
            e1.record(s)
            lu.copy_(u0)
            xp = torch.bmm(Ad, xp) + torch.bmm(Bd, u0.unsqueeze(2))
            torch.cuda.synchronize()
            if k >= WARM:
                ms.append(e0.elapsed_time(e1)); iters.append(float(it.double().mean()))
        res[tv] = dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), mean_iters=round(float(np.mean(iters)), 2),
                       not_optimal=int((st != 0).sum()))
    out = dict(what="loop" if direct else "loop_predictor_form", workload=cfg.name, B=B, steady=res[False])
    if True in res:
        out["time_varying"] = res[True]
        out["tv_over_steady"] = round(res[True]["median_ms"] / res[False]["median_ms"], 4)
    return out


def update_vs_two_calls(B, nxh=16):
    """updatestate! of the predictor form on a time-varying handle: kf_update_device (covariance mode 3, one launch) against
    kf_correct_device + kf_predict_device (modes 1 and 2)."""
    _, bt, A, Bu, C, ny = model(nxh, B)
    nu = Bu.shape[2]
    rng = np.random.default_rng(1)
    Q, R, P0 = covariances(rng, B, nxh, ny)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    x, y, u = T(np.zeros((B, nxh))), T(rng.standard_normal((B, ny))), T(rng.standard_normal((B, nu)))
    out = {}
    for one in (False, True):
        hd = mpcqp.Handle(B, nxh, nu, ny, 0, 2, 1)
        hd.set_model(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(C))
        hd.kf_set_covariances(Q, R, P0, np.arange(ny))
        def period(sp):
            if one:
                hd.kf_update_device(x.data_ptr(), u.data_ptr(), y.data_ptr(), stream=sp)
            else:
                hd.kf_correct_device(x.data_ptr(), y.data_ptr(), stream=sp)
                hd.kf_predict_device(x.data_ptr(), u.data_ptr(), stream=sp)
        out[one] = timed(period)
    return dict(what="update", nxh=nxh, B=B, kf_update_ms=round(out[True][0], 4), correct_plus_predict_ms=round(out[False][0], 4),
                ratio=round(out[True][0] / out[False][0], 4))


def dare_alternative(B=1024):
    """What a model swap costs with the steady filter: B DARE solves on the host (SciPy) and the upload of K̂."""
    cfg, bt, A, Bu, C, ny = model(16, B)
    rng = np.random.default_rng(1)
    Q, R, _ = covariances(rng, 1, cfg.nxh, ny)
    hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, ny, 0, 2, 1)
    hd.set_model(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(C))
    t0 = time.perf_counter()
    K = mpcqp.steady_kalman_gain(A, C, Q[0], R[0])
    t1 = time.perf_counter()
    hd.kf_set(mpcqp.colmajor(K), np.arange(ny))
    t2 = time.perf_counter()
    return dict(what="dare", B=B, nxh=cfg.nxh, dare_ms=round((t1 - t0) * 1e3, 2), upload_ms=round((t2 - t1) * 1e3, 3),
                ms_per_swap=round((t2 - t0) * 1e3, 2))


if __name__ == "__main__":
    args = sys.argv[1:]
    what = [a for a in args if a in ("cov", "loop", "dare", "forms")] or ["cov", "loop", "dare", "forms"]
    Bs = [int(a) for a in args if a.isdigit()]
    sizes = [int(a[3:]) for a in args if a.startswith("nxh")] or [16, 24, 32]
    if "cov" in what and HAVE_TV:
        for nxh in sizes:
            for B in (Bs or ([65536, 1024] if nxh == 16 else [16384])):
                print(json.dumps(cov_alone(nxh, B)), flush=True)
    if "loop" in what:
        for B in (Bs or [65536, 1024]):
            print(json.dumps(loop_period(B)), flush=True)
    if "dare" in what:
        print(json.dumps(dare_alternative()), flush=True)
    if "forms" in what and HAVE_DIRECT:
        for B in (Bs or [65536, 1024]):
            print(json.dumps(loop_period(B, direct=False)), flush=True)
        print(json.dumps(update_vs_two_calls((Bs or [65536])[0])), flush=True)
