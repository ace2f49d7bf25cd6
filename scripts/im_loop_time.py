"""Timing of LinMPC(InternalModel) on the device: C3 dimensions with nx̂ = nx = 12 (no output integrators: the InternalModel does
not augment the state; hard u, soft ymax as in the bench configuration), a general stochastic model with nxs = 4, a live
noisy loop: the plant is the model itself, so the measurement of a period is Ĉ x̂d + noise of that period (two torch kernels on
the same stream, timed on their own as `plant_torch`), and x̂0 = the estimator's own state.
  `loop_device`    the plant's two kernels and mpcqp_loop_device: correct, step, update on one stream, HIP events around N = 30
                   periods enqueued back to back on resident data, median of 5 windows after 2 warm-up windows, per period;
  `correct`, `step`, `update`   the three launches of that period alone, each N times back to back between its own pair of
                   events on the same state (median of 5 windows after 2), per launch; `estimator_bytes` is what the two
                   estimator kernels have to move per member and period, computed from the shapes, and `gbytes_per_s` that
                   over their time;
  `host_methods`   the same period through the host-pointer methods preparestate / moveinput / updatestate: wall clock per
                   period around calls that end in a device synchronisation, median of 5 after 2 warm-ups.
One JSON line per measurement.  Usage: python scripts/im_loop_time.py [B ...]   (default B: 65536 1024)."""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, NXS = 30, 4


def measure(B):
    import torch
    import mpcqp
    from mpcqp import api, synth
    cfg = synth.C3
    nx, nu, ny, Hp = cfg.nx, cfg.nu, cfg.ny, cfg.Hp
    dev = torch.device("cuda", 0)
    rg = np.random.default_rng(1)
    A = 0.9 * synth._stable_A(rg, nx, B)
    Bu, Cm = rg.standard_normal((B, nx, nu)) / np.sqrt(nx), rg.standard_normal((B, ny, nx)) / np.sqrt(nx)
    mpc = mpcqp.BatchLinMPC(A, Bu, Cm, Hp=Hp, Hc=cfg.Hc, Cwt=cfg.Cwt, Mwt=np.full(ny, cfg.Mwt), Nwt=np.full(nu, cfg.Nwt), Lwt=np.full(nu, cfg.Lwt))
    mpc.setconstraint(umin=np.full(nu, cfg.umin), umax=np.full(nu, cfg.umax), ymax=np.full(ny, cfg.ymax))
    # one ARMA(1,1) disturbance (z - beta) / (z - alpha) per output, alpha in [0.9, 1] (member 0: integrators), mixed by an
    # orthogonal similarity: Âs has the eigenvalues beta, so the inverse the estimator runs is stable and the loop is too
    alpha, beta = rg.uniform(0.9, 1.0, (B, NXS)), rg.uniform(0.2, 0.6, (B, NXS))
    alpha[0] = 1.0
    Q, _ = np.linalg.qr(rg.standard_normal((B, NXS, NXS)))
    eye = np.broadcast_to(np.eye(NXS), (B, NXS, NXS))
    stoch = (Q @ (alpha[:, :, None] * eye) @ Q.transpose(0, 2, 1), Q.copy(), ((alpha - beta)[:, :, None] * eye) @ Q.transpose(0, 2, 1), eye.copy())
    mpc.setestimator(internal=dict(stoch_ym=stoch))
    mpc._prepare_kernel()
    hd = mpc.hd
    hd.set_flags(hd.flags | api.FLAG_RY_CONSTANT)
    t = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)
    p = lambda a: a.data_ptr()
    out = lambda name, **kw: print(json.dumps(dict(B=B, what=name, kernel_kind=mpc.kernel, **kw)), flush=True)
    ys = [t(0.1 * rg.standard_normal((B, ny))) for _ in range(N)]          # the noisy measurements of a window
    xh, lu, Z, u0, st, ry = z(B, nx), z(B, nu), z(B, mpc.nZ), z(B, nu), z(B, dt=torch.int32), t(0.3 * rg.standard_normal((B, ny)))
    s = torch.cuda.current_stream()
    sp = s.cuda_stream

    def window(call):
        for k in range(N):
            call(k)

    def timed(call, warm=2, reps=5):
        for _ in range(warm):
            window(call)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); window(call); e1.record(s)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / N)
        return dict(ms=round(float(np.median(ms)), 5), ms_min=round(float(np.min(ms)), 5), ms_max=round(float(np.max(ms)), 5))

    ub, Ct, ybuf = [u0, lu], t(Cm), z(B, ny)

    def plant(k):       # y0m = Ĉ x̂d + the noise of the period
        torch.add(torch.bmm(Ct, xh.unsqueeze(2)).squeeze(2), ys[k], out=ybuf)

    def loop(k):        # (lastu0 = the u0 of the period before: two buffers in turn, N is even)
        plant(k)
        hd.loop_device(p(xh), p(ybuf), p(ub[(k + 1) % 2]), p(ry), p(Z), p(ub[k % 2]), p(st), stream=sp)
    r = timed(loop)
    out("loop_device", N=N, not_optimal=int(np.count_nonzero(st.cpu().numpy())), max_abs_u0=float(u0.abs().max()), **r)
    out("plant_torch", **timed(plant))
    # bytes per member and period of the two estimator kernels: As, Cs, Âs, B̂s, Ĉ rows, x̂d, x̂s, z, y0m, ŷs, B, Ŷs, B_eff in the
    # correction; Â, B̂u, x̂d twice, u0, x̂s, z in the update
    nY = ny * Hp
    cbytes = 8 * (2 * NXS * NXS + 2 * NXS * ny + ny * nx + nx + 3 * NXS + 2 * ny + 3 * nY)
    ubytes = 8 * (nx * nx + nx * nu + 2 * nx + nu + 2 * NXS)
    c = timed(lambda k: hd.im_correct_device(p(xh), p(ys[k]), stream=sp))
    out("correct", bytes_per_member=cbytes, gbytes_per_s=round(B * cbytes / c["ms"] * 1e-6, 1), **c)
    out("step", **timed(lambda k: hd.step_device(p(xh), p(lu), p(ry), p(Z), p(u0), p(st), stream=sp)))
    xu = xh.clone()
    u = timed(lambda k: hd.im_update_device(p(xu), p(u0), stream=sp))
    out("update", bytes_per_member=ubytes, gbytes_per_s=round(B * ubytes / u["ms"] * 1e-6, 1), **u)
    out("estimator_kernels", ms=round(c["ms"] + u["ms"], 5), estimator_bytes=cbytes + ubytes)

    ym, ryh = 0.1 * rg.standard_normal((N, B, ny)), ry.cpu().numpy()
    wall = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for k in range(7):
            t0 = time.perf_counter()
            mpc.preparestate(ym[k])
            uk = mpc.moveinput(None, ryh)
            mpc.updatestate(uk, ym[k])
            wall.append((time.perf_counter() - t0) * 1e3)
    out("host_methods", ms=round(float(np.median(wall[2:])), 4), ms_min=round(float(np.min(wall[2:])), 4), ms_max=round(float(np.max(wall[2:])), 4))


if __name__ == "__main__":
    for B in [int(a) for a in sys.argv[1:] if a.isdigit()] or [65536, 1024]:
        measure(B)
