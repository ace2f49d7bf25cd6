"""Developer tool: cost of custom linear constraints on the MultipleShooting kernel -- the same batch with nw = 0 and
with nw = 2 soft custom rows (Wy, Wu random, wide bounds): python scripts/ms_custom_time.py CFG B [lib.so]"""
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
rng = np.random.default_rng(0)
Wy, Wu = 0.5 * rng.standard_normal((2, cfg.ny)), 0.5 * rng.standard_normal((2, cfg.nu))
res = {}
for nw in (0, 2):
    kw = dict(Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt, Mwt=np.full(cfg.ny, cfg.Mwt), Nwt=np.full(cfg.nu, cfg.Nwt),
              Lwt=np.full(cfg.nu, cfg.Lwt), cold_start=True)
    con = constraint_kwargs(cfg)
    if nw:
        kw.update(Wy=Wy, Wu=Wu)
        con.update(wmin=[-1.0, -np.inf], wmax=[1.0, 0.8])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mpc = mpcqp.BatchLinMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], transcription="MultipleShooting", lib=lib, **kw)
        mpc.setconstraint(**con)
        ms = []
        for rep in range(4):
            mpc.lastu0 = bt["lastu0"].copy(); mpc.Z[:] = 0
            mpc.moveinput(bt["xhat0"], bt["ry"]); ms.append(mpc.hd.last_step_ms())
    res[nw] = min(ms[1:])
    print(f"nw={nw}: kernel kind {mpc.kernel} lds {mpc.hd.lds_bytes()} ms {['%.2f' % m for m in ms]} status "
          f"{np.bincount(mpc.status, minlength=3)} iters {mpc.iters.mean():.2f}", flush=True)
print(f"time ratio nw=2 / nw=0: {res[2] / res[0]:.3f}")
