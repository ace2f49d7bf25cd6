"""Timing of the closed-loop simulation (mpcqp_sim_device) against what a period cost before it, on resident data: HIP events
around N = 100 periods enqueued back to back, median of 10 after 3 warm-ups, reported per period.  C3 dimensions.
  `floor`         mpcqp_kf_correct_device + mpcqp_explicit_law_device (u0 alone) + mpcqp_kf_predict_device per period, on an
                  unconstrained handle with the law: a period without any plant, y0m held.  Every library since the
                  ExplicitMPC has these entry points: with --lib PATH this is the floor on a build of the parent commit;
  `sim_explicit`  mpcqp_sim_device on that handle with MPCQP_SIM_FLAG_NO_FUSE: the same three launches plus k_sim_plant per
                  period, all records asked for (`sim_explicit_norec`: none), noise on all channels;
  `sim_fused`     the same call without the flag: the whole loop in one launch of k_sim_explicit (`sim_fused_norec`: no records);
  `loop`          mpcqp_loop_device on the C3 bench configuration (hard u, soft ymax, steady gain): estimator and step fused
                  in one launch, no plant.  Also on a parent build;
  `sim_c3`        mpcqp_sim_device on that handle: un-fused estimator calls, the step, the plant kernel.
One JSON line per measurement.  `python scripts/sim_time.py compare PARENT_LIB [B ...]` runs parent and tree in fresh child
processes, alternating, two passes each.  Usage: python scripts/sim_time.py [compare PARENT_LIB | --lib PATH] [B ...]
(default B: 65536 1024)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, REPS, N = 3, 10, 100


def timed(fn, torch):
    s = torch.cuda.current_stream()
    for _ in range(WARM):
        fn(s.cuda_stream)
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(s.cuda_stream); e1.record(s)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / N)
    return float(np.median(ms)), float(np.min(ms))


def measure(B, tag):
    import torch
    import mpcqp
    from mpcqp import synth
    cfg = synth.C3
    dev = torch.device("cuda", 0)
    bt = synth.make_batch(cfg, B, seed=0)
    rg = np.random.default_rng(1)
    nxh, nu, ny, nxp = cfg.nxh, cfg.nu, cfg.ny, cfg.nx
    t = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)
    p = lambda a: a.data_ptr()
    out = lambda name, ms, **kw: print(json.dumps(dict(lib=tag, B=B, N=N, what=name, ms_per_period=round(ms[0], 5),
                                                       ms_min=round(ms[1], 5), **kw)), flush=True)
    # the steady gain of Q̂ = R̂ = 0.1 I, solved on the device: the loops below stay bounded over the 1300 periods they run
    Q, R = np.broadcast_to(0.1 * np.eye(nxh), (B, nxh, nxh)), np.broadcast_to(0.1 * np.eye(ny), (B, ny, ny))
    y = t(0.1 * rg.standard_normal((B, ny)))
    # the plant of the simulations: the controller's own plant part (nxp = 12)
    A, Bu, Cm = bt["Ahat"][:, :nxp, :nxp], 1.2 * bt["Bhu"][:, :nxp], bt["Chat"][:, :, :nxp]
    draws = {k: t(rg.standard_normal((B, N, n))) for k, n in (("w_u", nu), ("w_y", ny), ("w_x", nxp))}
    sig = {k: t(np.full((B, n), 0.01)) for k, n in (("sigma_u", nu), ("sigma_y", ny), ("sigma_x", nxp))}
    rec = lambda: dict(Y=z(B, N, ny), X=z(B, N, nxp), Xhat=z(B, N, nxh), Yhat=z(B, N, ny), U=z(B, N, nu), Ud=z(B, N, nu))

    def sim_call(hd, Z, records, flags=0):
        x0, xh, lu, st = z(B, nxp), t(bt["xhat0"]), t(bt["lastu0"]), z(B, N, dt=torch.int32)
        ry = t(bt["ry"])
        r = rec() if records else {}
        kw = {k: p(v) for k, v in {**draws, **sig, **r}.items()}
        keep = (x0, xh, lu, st, ry, r)
        return keep, lambda s: hd.sim_device(N, flags=flags, stream=s, ry=p(ry), x0=p(x0), xhat0=p(xh), lastu0=p(lu), status=p(st),
                                             Ztilde=0 if Z is None else p(Z), **kw)

    # -- the explicit handle ----------------------------------------------------------------------------------------------
    mpc = mpcqp.BatchExplicitMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], Hp=cfg.Hp, Hc=cfg.Hc, law=True)
    hd = mpc.hd
    hd.kf_set_steady(Q, R, np.arange(ny))
    xh, lu, ry, u0, st = t(bt["xhat0"]), t(bt["lastu0"]), t(bt["ry"]), z(B, nu), z(B, dt=torch.int32)

    def floor(s):
        for _ in range(N):
            hd.kf_correct_device(p(xh), p(y), stream=s)
            hd.explicit_law_device(p(xh), p(lu), p(ry), p(u0), p(st), stream=s)
            hd.kf_predict_device(p(xh), p(u0), stream=s)
    out("floor", timed(floor, torch))
    if hasattr(hd.lib, "mpcqp_sim"):
        hd.sim_set_plant(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(Cm))
        for name, records, flags in (("sim_explicit", True, mpcqp.api.SIM_FLAG_NO_FUSE), ("sim_explicit_norec", False, mpcqp.api.SIM_FLAG_NO_FUSE),
                                     ("sim_fused", True, 0), ("sim_fused_norec", False, 0)):
            keep, fn = sim_call(hd, None, records, flags)
            out(name, timed(fn, torch), path=hd.sim_path() if not flags else mpcqp.api.SIM_PATH_PERIOD)
            del keep
    del mpc, hd

    # -- the C3 bench configuration ---------------------------------------------------------------------------------------
    from tests.parity_util import make_controller
    mpc = make_controller(cfg, bt)
    hd = mpc.hd
    hd.set_flags(hd.flags | mpcqp.FLAG_RY_CONSTANT)
    kind = hd.prepare()
    hd.kf_set_steady(Q, R, np.arange(ny))
    xh, Z, it = t(bt["xhat0"]), z(B, mpc.nZ), z(B, dt=torch.int32)
    bufs = [t(bt["lastu0"]), z(B, nu)]

    def loop(s):
        for k in range(N):
            hd.loop_device(p(xh), p(y), p(bufs[k % 2]), p(ry), p(Z), p(bufs[(k + 1) % 2]), p(st), iters=p(it), stream=s)
    out("loop", timed(loop, torch), kernel_kind=kind)
    if hasattr(hd.lib, "mpcqp_sim"):
        hd.sim_set_plant(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(Cm))
        Z.zero_()
        keep, fn = sim_call(hd, Z, True)
        out("sim_c3", timed(fn, torch), kernel_kind=kind, path=hd.sim_path())


def main():
    args = sys.argv[1:]
    if args and args[0] == "compare":
        parent, rest = os.path.abspath(args[1]), args[2:]
        me = os.path.abspath(__file__)
        with tempfile.TemporaryDirectory(prefix="mpcqp_spec_") as tmp:
            env = dict(os.environ, MPCQP_CACHE_DIR=os.environ.get("MPCQP_CACHE_DIR") or tmp)
            for _ in range(2):                  # parent, tree, parent, tree: one fresh child process each, one at a time
                for lib in (parent, None):
                    cmd = [sys.executable, me] + (["--lib", lib] if lib else []) + rest
                    subprocess.run(cmd, check=True, timeout=300, env=env)
        return
    tag = "tree"
    if args and args[0] == "--lib":
        os.environ["MPCQP_LIB"] = args[1]
        tag, args = os.path.basename(args[1]), args[2:]
    for B in [int(a) for a in args if a.isdigit()] or [65536, 1024]:
        measure(B, tag)


if __name__ == "__main__":
    main()
