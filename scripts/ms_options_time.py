"""Developer tool: cost of the options of the MultipleShooting kernel on one batch -- (1) M / N / L as stage-separable block
matrices against the same weights as diagonals (the blocks ARE the diagonals: the same QP, the block code path), (2)
MPCQP_FLAG_KEEP_QP, (3) closed-loop periods/s with the plain start against MPCQP_FLAG_WARM_DUAL:
python scripts/ms_options_time.py CFG B [lib.so]"""
import os
import sys
import warnings

sys.path.insert(0, '.')
import numpy as np

import mpcqp
from mpcqp import synth
from tests.parity_util import constraint_kwargs

cfg = synth.get_config(sys.argv[1]); B = int(sys.argv[2])
lib = mpcqp.api.load_library(os.path.abspath(sys.argv[3])) if len(sys.argv) > 3 else None
bt = synth.make_batch(cfg, B, seed=0)
nmoves = cfg.Hc if np.isscalar(cfg.Hc) else len(cfg.Hc)


def controller(**kw):
    base = dict(Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt, Mwt=np.full(cfg.ny, cfg.Mwt), Nwt=np.full(cfg.nu, cfg.Nwt),
                Lwt=np.full(cfg.nu, cfg.Lwt))
    base.update(kw)
    mpc = mpcqp.BatchLinMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], transcription="MultipleShooting", lib=lib, **base)
    mpc.setconstraint(**constraint_kwargs(cfg))
    return mpc


def cold_steps(mpc, reps=4):
    ms = []
    for rep in range(reps):
        mpc.lastu0 = bt["lastu0"].copy(); mpc.Z[:] = 0
        mpc.moveinput(bt["xhat0"], bt["ry"]); ms.append(mpc.hd.last_step_ms())
    return ms


res = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    blocks = dict(M_Hp=np.kron(np.eye(cfg.Hp), np.diag(np.full(cfg.ny, cfg.Mwt))),
                  N_Hc=np.kron(np.eye(nmoves), np.diag(np.full(cfg.nu, cfg.Nwt))),
                  L_Hp=np.kron(np.eye(cfg.Hp), np.diag(np.full(cfg.nu, cfg.Lwt))))
    for name, kw in (("diagonals", dict(cold_start=True)), ("blocks", dict(cold_start=True, **blocks)),
                     ("keep_qp", dict(cold_start=True, keep_qp=True))):
        mpc = controller(**kw)
        ms = cold_steps(mpc)
        res[name] = min(ms[1:])
        print(f"{name}: kernel kind {mpc.kernel} mask {mpc.hd.transcription_supported()} ms {['%.2f' % m for m in ms]} status "
              f"{np.bincount(mpc.status, minlength=3)} iters {mpc.iters.mean():.2f}", flush=True)
        del mpc
    print(f"time ratio blocks / diagonals: {res['blocks'] / res['diagonals']:.3f}")
    print(f"time ratio keep_qp / plain: {res['keep_qp'] / res['diagonals']:.3f}")
    # closed loop: the plants driven by the returned inputs plus state noise, 6 periods, the first one left out
    for name, kw in (("plain", {}), ("warm_dual", dict(warm_dual=True))):
        mpc = controller(**kw)
        mpc.lastu0 = bt["lastu0"].copy()
        x = bt["xhat0"].copy()
        rg = np.random.default_rng(1)
        ms, its = [], []
        for k in range(6):
            u = mpc.moveinput(x, bt["ry"])
            ms.append(mpc.hd.last_step_ms()); its.append(mpc.iters.mean())
            x = np.einsum("bij,bj->bi", bt["Ahat"], x) + np.einsum("bij,bj->bi", bt["Bhu"], u) + 0.02 * rg.standard_normal(x.shape)
        res[name] = np.mean(ms[1:])
        print(f"closed loop {name}: ms {['%.2f' % m for m in ms]} iters {['%.2f' % i for i in its]} status "
              f"{np.bincount(mpc.status, minlength=3)} -> {1e3 / res[name]:.2f} periods/s of {B} controllers", flush=True)
        del mpc
    print(f"closed-loop time ratio warm_dual / plain: {res['warm_dual'] / res['plain']:.3f}")
