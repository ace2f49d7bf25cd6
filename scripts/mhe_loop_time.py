"""Timing of LinMPC(MovingHorizonEstimator) on the device: C3 dimensions (the bench configuration: hard u, soft ymax), He = 20.
  `sim_mhe`        mpcqp_sim_device with the estimator attached: HIP events around N = 30 periods enqueued back to back on
                   resident data, median of 5 after 2 warm-ups (the window is full and moving from the first timed run on),
                   reported per period; `kernels_ms` is est.handle.last_ms() + mpc.hd.last_step_ms() of the last period of the
                   same run -- the two solve kernels alone -- so the difference is the plant kernel, the covariance launches,
                   the copies and whatever the hand-off costs;
  `host_methods`   the same period through the host-pointer public methods est.preparestate / mpc.moveinput(est.x̂0) /
                   est.updatestate on a held measurement (the only way a library without mpcqp_mhe_attach runs this loop):
                   wall clock per period, median of 5 after 2 warm-ups; `kernels_ms` as above;
  `initstate`      mpcqp_est_initstate_device, HIP events, median of 10 after 3 warm-ups, for the whole batch;
  `initstate_numpy` np.linalg.lstsq member by member, 1024 members, wall clock (reported for 1024 members, not scaled).
One JSON line per measurement.  Usage: python scripts/mhe_loop_time.py [B ...]   (default B: 65536 1024)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, HE = 30, 20


def measure(B):
    import torch
    import mpcqp
    from mpcqp import synth
    from tests.parity_util import make_controller
    cfg = synth.C3
    dev = torch.device("cuda", 0)
    bt = synth.make_batch(cfg, B, seed=0)
    rg = np.random.default_rng(1)
    nxh, nu, ny, nxp = cfg.nxh, cfg.nu, cfg.ny, cfg.nx
    t = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)
    p = lambda a: a.data_ptr()
    out = lambda name, **kw: print(json.dumps(dict(B=B, what=name, **kw)), flush=True)
    rep = lambda M: np.broadcast_to(M, (B,) + M.shape).copy()
    mpc = make_controller(cfg, bt)
    est = mpcqp.BatchMHE(bt["Ahat"], bt["Bhu"], bt["Chat"], He=HE, Q̂=rep(0.1 * np.eye(nxh)), R̂=rep(0.1 * np.eye(ny)), P̂_0=rep(0.5 * np.eye(nxh)))
    mpc.setestimator(mhe=est)
    mpc._prepare_kernel()
    hd = mpc.hd
    A, Bu, Cm = bt["Ahat"][:, :nxp, :nxp], 1.2 * bt["Bhu"][:, :nxp], bt["Chat"][:, :, :nxp]
    hd.sim_set_plant(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(Cm))
    draws = {k: t(rg.standard_normal((B, N, n))) for k, n in (("w_u", nu), ("w_y", ny), ("w_x", nxp))}
    sig = {k: t(np.full((B, n), 0.01)) for k, n in (("sigma_u", nu), ("sigma_y", ny), ("sigma_x", nxp))}
    x0, xh, lu, st, ry, Z = z(B, nxp), t(bt["xhat0"]), t(bt["lastu0"]), z(B, N, dt=torch.int32), t(bt["ry"]), z(B, mpc.nZ)
    kw = {k: p(v) for k, v in {**draws, **sig}.items()}
    s = torch.cuda.current_stream()
    fn = lambda: hd.sim_device(N, stream=s.cuda_stream, ry=p(ry), x0=p(x0), xhat0=p(xh), lastu0=p(lu), status=p(st), Ztilde=p(Z), **kw)
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / N)
    est_bad = int(np.count_nonzero(hd.sim_est_status(N)))
    out("sim_mhe", N=N, He=HE, ms_per_period=round(float(np.median(ms)), 5), ms_min=round(float(np.min(ms)), 5),
        kernels_ms=round(est.handle.last_ms() + hd.last_step_ms(), 5), est_last_ms=round(est.handle.last_ms(), 5),
        step_last_ms=round(hd.last_step_ms(), 5), controller_not_optimal=int(np.count_nonzero(st.cpu().numpy())), estimator_not_solved=est_bad)

    # the host-pointer public methods, held measurement
    ym, ryh = 0.1 * rg.standard_normal((B, ny)), bt["ry"]
    wall = []
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for k in range(7):
            t0 = time.perf_counter()
            est.preparestate(ym)
            u = mpc.moveinput(est.x̂0, ryh)
            est.updatestate(u, ym)
            wall.append((time.perf_counter() - t0) * 1e3)
    out("host_methods", ms_per_period=round(float(np.median(wall[2:])), 4), ms_min=round(float(np.min(wall[2:])), 4),
        kernels_ms=round(est.handle.last_ms() + hd.last_step_ms(), 5))

    # initstate: the QR kernel for the whole batch, NumPy's lstsq for 1024 members
    u0, y0m, xi, ist = t(bt["lastu0"]), t(ym), z(B, nxh), z(B, dt=torch.int32)
    call = lambda: hd.est_initstate_device(p(xi), p(u0), p(y0m), p(ist), stream=s.cuda_stream)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); call(); e1.record(s)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    out("initstate", ms=round(float(np.median(ms)), 5), ms_min=round(float(np.min(ms)), 5), not_solved=int(np.count_nonzero(ist.cpu().numpy())))
    nn = min(B, 1024)
    M = np.concatenate([np.eye(nxh) - bt["Ahat"][:nn], bt["Chat"][:nn]], axis=1)
    rhs = np.concatenate([np.einsum("bij,bj->bi", bt["Bhu"][:nn], bt["lastu0"][:nn]), ym[:nn]], axis=1)
    t0 = time.perf_counter()
    ref = np.array([np.linalg.lstsq(M[b], rhs[b], rcond=None)[0] for b in range(nn)])
    out("initstate_numpy", members=nn, ms=round((time.perf_counter() - t0) * 1e3, 3),
        max_abs_diff=float(np.abs(xi.cpu().numpy()[:nn] - ref).max()))


if __name__ == "__main__":
    for B in [int(a) for a in sys.argv[1:] if a.isdigit()] or [65536, 1024]:
        measure(B)
