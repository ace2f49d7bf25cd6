"""Timing of the wide MHE solve kernels (one estimator per wavefront, nx̂ = 24 and 32) on resident data at hard x̂ bounds and
He = 20, next to the 16-lane kernel at nx̂ = 16 (scaling reference) and to the C port oracle/mhe_ref.c at nx̂ = 24 on the
host's threads.  Prints one JSON line per measurement: steady-state periods (full window), kernel ms from the handle's
HIP events.  MPCQP_LIB selects another build of the library (A/B of the matrix-core and the broadcast form of the products).
Usage: python scripts/mhe_wide_time.py [B ...] (default 4096 16384); `cport` as an argument adds the host measurement."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import mpcqp  # noqa: E402
from mpcqp import synth, mhe as pm  # noqa: E402
import mhe_util  # noqa: E402

if os.environ.get("MPCQP_LIB"):
    mpcqp.api._lib = mpcqp.api.load_library(os.environ["MPCQP_LIB"])

HE, XABS, STEADY = 20, 1.2, 4
CONFIGS = {16: dict(nx=12, nym=4), 24: dict(nx=20, nym=4), 32: dict(nx=26, nym=6)}


def config(nxh):
    return synth.MheConfig(f"time{nxh}", nu=2, nd=0, He=HE, xabs=XABS, **CONFIGS[nxh])


def gpu(nxh, B):
    cfg = config(nxh)
    nper = cfg.He + STEADY
    bt = synth.make_mhe_batch(cfg, B, seed=1)
    Y, U, _ = synth.make_mhe_data(cfg, bt, nper, seed=0)
    bm = mhe_util.make_product(cfg, bt, keep_windows=False)
    h = bm.handle
    dev = torch.device("cuda:0")
    Yd, Ud = torch.tensor(Y, device=dev), torch.tensor(U, device=dev)
    ms, iters, bad = [], [], 0
    for k in range(nper):
        h.prepare_device(Yd[k].data_ptr(), 0)
        h.update_device(Ud[k].data_ptr(), Yd[k].data_ptr(), 0)
        h.sync()
        if k >= cfg.He:
            ms.append(h.last_ms())
            iters.append(float(h.get(pm.GET_ITERS).mean()))
            bad += int((h.get(pm.GET_STATUS) != 0).sum())
    m = float(np.mean(ms))
    return dict(what="gpu", nxh=nxh, B=B, He=HE, lanes=h.lanes_per_estimator(), NX=h.register_columns(), kernel_ms=round(m, 3),
                periods_per_s=round(B / (m * 1e-3)), mean_iters=round(float(np.mean(iters)), 2), failed=bad,
                lib=os.path.basename(os.environ.get("MPCQP_LIB", mpcqp.DEFAULT_LIB)))


def cport(nxh, n=256, K=6):
    from oracle import mhe_cport
    cfg = config(nxh)
    bt = synth.make_mhe_batch(cfg, n, seed=1)
    Y, U, _ = synth.make_mhe_data(cfg, bt, cfg.He + K, seed=0)
    t0 = time.perf_counter()
    mhe_cport.run(bt, Y[:cfg.He], U[:cfg.He], cfg.He, cfg.xabs)
    t_fill = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, it, st = mhe_cport.run(bt, Y, U, cfg.He, cfg.xabs)
    t_all = time.perf_counter() - t0
    return dict(what="oracle/mhe_ref.c", nxh=nxh, estimators=n, periods=K, threads=int(mhe_cport.threads()),
                periods_per_s=round(n * K / max(t_all - t_fill, 1e-9)), mean_iters=round(float(it[cfg.He:].mean()), 2),
                all_solved=bool((st == 0).all()))


if __name__ == "__main__":
    args = sys.argv[1:]
    Bs = [int(a) for a in args if a.isdigit()] or [4096, 16384]
    sizes = [int(a[3:]) for a in args if a.startswith("nxh")] or [16, 24, 32]
    for nxh in sizes:
        for B in Bs:
            print(json.dumps(gpu(nxh, B)), flush=True)
    if "cport" in args:
        print(json.dumps(cport(24)), flush=True)
