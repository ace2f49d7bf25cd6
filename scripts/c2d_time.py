"""Timing of the discretisation of continuous-time models (csrc/c2d_kernels.hip: k_c2d, one launch per batch) at C3 dimensions
(nx = 12, nu = 4, ny = 4, nint_ym = 1, so nx̂ = 16; |A Ts| about 1), HIP events on resident data, median and minimum of 10
after 3 warm-ups:
  * `kernel`: mpcqp_c2d_device alone at B = 65536 and 1024;
  * `handle`: mpcqp_set_model_continuous_device against mpcqp_recondense_device alone on the same C3 handle (B = 1024) in the
              same session -- the difference is what discretising adds to the setmodel! path;
  * `host`:   scipy.linalg.expm member by member for the 1024, on the host.
One JSON line per measurement.
Usage: python scripts/c2d_time.py [kernel] [handle] [host] [B ...]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402,F401
import mpcqp  # noqa: E402
from mpcqp import synth  # noqa: E402
import kf_cov_time as kt  # noqa: E402

NX, NU, NY = 12, 4, 4
DEV = torch.device("cuda", 0)


def models(B, distinct=64):
    """Stable continuous models (eigenvalues in -[0.02, 1] under a random similarity, plus 0.3 skew), Ts with |M Ts|_1 = 1."""
    rng = np.random.default_rng(0)
    A, Bu, C, Ts = [], [], [], []
    for _ in range(min(B, distinct)):
        S = rng.standard_normal((NX, NX)) + 2.0 * np.eye(NX)
        G = rng.standard_normal((NX, NX)) / np.sqrt(NX)
        A.append(S @ np.diag(-rng.uniform(0.02, 1.0, NX)) @ np.linalg.inv(S) + 0.3 * (G - G.T))
        Bu.append(rng.standard_normal((NX, NU)))
        C.append(rng.standard_normal((NY, NX)))
        Ts.append(1.0 / np.linalg.norm(np.hstack([A[-1], Bu[-1]]), 1))
    idx = np.arange(B) % len(A)
    return tuple(np.ascontiguousarray(np.array(a)[idx]) for a in (A, Bu, C, Ts))


def device_args(A, Bu, C, Ts):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return [T(mpcqp.colmajor(A)), T(mpcqp.colmajor(Bu)), T(mpcqp.colmajor(C)), T(Ts)]


def kernel(B):
    A, Bu, C, Ts = models(B)
    o = mpcqp.C2dOptions(B, NX, NU, NY, 0, 0, 1)
    d = device_args(A, Bu, C, Ts)
    z = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=DEV)
    out = [z(B, o.nxh * o.nxh), z(B, o.nxh * NU), z(B, NY * o.nxh)]
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    med, mn = kt.timed(lambda sp: mpcqp.c2d_device(o, *[t.data_ptr() for t in d], *[t.data_ptr() for t in out], st.data_ptr(), stream=sp))
    return dict(what="kernel", B=B, nx=NX, nu=NU, nxh=o.nxh, c2d_median_ms=round(med, 4), c2d_min_ms=round(mn, 4),
                refused=int(st.cpu().numpy().astype(bool).sum()))


def handle(B=1024):
    cfg = synth.C3
    A, Bu, C, Ts = models(B)
    o = mpcqp.C2dOptions(B, NX, NU, NY, 0, 0, 1)
    assert o.nxh == cfg.nxh and (cfg.nu, cfg.ny) == (NU, NY)
    hd = mpcqp.Handle(B, cfg.nxh, NU, NY, 0, cfg.Hp, cfg.Hc)
    hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt), np.full(B, cfg.Cwt))
    d = device_args(A, Bu, C, Ts)
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    ptr = [t.data_ptr() for t in d]
    both = kt.timed(lambda sp: hd.set_model_continuous_device(o, *ptr, st.data_ptr(), stream=sp))
    rec = kt.timed(lambda sp: hd.recondense_device(stream=sp))
    return dict(what="handle", B=B, set_model_continuous_median_ms=round(both[0], 4), set_model_continuous_min_ms=round(both[1], 4),
                recondense_median_ms=round(rec[0], 4), recondense_min_ms=round(rec[1], 4),
                added_median_ms=round(both[0] - rec[0], 4), refused=int(st.cpu().numpy().astype(bool).sum()))


def host(B=1024):
    import scipy.linalg
    A, Bu, C, Ts = models(B)
    M = np.zeros((B, NX + NU, NX + NU))
    M[:, :NX] = np.concatenate([A, Bu], axis=2)
    t0 = time.perf_counter()
    for b in range(B):
        scipy.linalg.expm(M[b] * Ts[b])
    t1 = time.perf_counter()
    return dict(what="host", B=B, scipy_expm_ms_total=round((t1 - t0) * 1e3, 1), scipy_expm_ms_per_member=round((t1 - t0) * 1e3 / B, 4))


if __name__ == "__main__":
    args = sys.argv[1:]
    what = [a for a in args if a in ("kernel", "handle", "host")] or ["kernel", "handle", "host"]
    if "kernel" in what:
        for B in [int(a) for a in args if a.isdigit()] or [65536, 1024]:
            print(json.dumps(kernel(B)), flush=True)
    if "handle" in what:
        print(json.dumps(handle()), flush=True)
    if "host" in what:
        print(json.dumps(host()), flush=True)
