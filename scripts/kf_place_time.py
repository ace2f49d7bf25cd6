"""Timing of the pole placement of the Luenberger observer (csrc/kf_place_kernels.hip: k_kf_place, one launch per placement) on
resident data, HIP events around mpcqp_kf_place_device: median and minimum of 10 after 3 warm-ups, with the mean sweep count
of the batch.
  * `place`: C3 shapes (nx̂ = 16, nym = 4) at B = 65536 and 1024, default cap, poles linspace(0.2, 0.8, nx̂);
  * `host`:  the alternative per model swap -- scipy.signal.place_poles(method="KNV0") on the dual pair, member by member, on a
             sample of the 1024, extrapolated to the batch, with the largest pole error of both on that sample.
One JSON line per measurement.
Usage: python scripts/kf_place_time.py [place] [host] [B ...]"""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402,F401
import mpcqp  # noqa: E402
import kf_cov_time as kt  # noqa: E402

SAMPLE = 16


def poles_for(nxh):
    return np.linspace(0.2, 0.8, nxh)


def pole_error(A, Cm, K, p):
    w = np.linalg.eigvals(A @ (np.eye(A.shape[0]) - K @ Cm))
    return float(np.abs(np.sort_complex(w) - np.sort(p)).max())


def place(B):
    cfg, bt, A, Bu, C, ny = kt.model(16, B)
    p = np.broadcast_to(poles_for(cfg.nxh), (B, cfg.nxh)).copy()
    hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, ny, 0, 2, 1)
    hd.set_model(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(C))
    t0 = time.perf_counter()
    hd.kf_set_poles(p, np.arange(ny))                           # (uploads the poles and places once)
    t1 = time.perf_counter()
    med, mn = kt.timed(lambda sp: hd.kf_place_device(stream=sp))
    sw, st, K = hd.kf_place_sweeps(), hd.kf_status(), hd.kf_gain()
    ok = np.flatnonzero(st == 0)[:SAMPLE]
    err = max((pole_error(A[b], C[b], K[b], p[b]) for b in ok), default=float("nan"))
    return dict(what="place", nxh=cfg.nxh, nym=ny, B=B, place_median_ms=round(med, 4), place_min_ms=round(mn, 4),
                mean_sweeps=round(float(sw.mean()), 2), max_sweeps=int(sw.max()), not_placed=int((st != 0).sum()),
                set_poles_wall_ms=round((t1 - t0) * 1e3, 2), pole_err_sample=err)


def host_alternative(B=1024):
    from scipy.signal import place_poles
    cfg, bt, A, Bu, C, ny = kt.model(16, B)
    p = poles_for(cfg.nxh)
    t0 = time.perf_counter()
    errs = []
    for b in range(SAMPLE):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                     # ("Convergence was not reached after maxiter iterations")
            res = place_poles(A[b].T, (C[b] @ A[b]).T, p, method="KNV0")
        errs.append(pole_error(A[b], C[b], res.gain_matrix.T, p))
    t1 = time.perf_counter()
    per = (t1 - t0) * 1e3 / SAMPLE
    return dict(what="host", B=B, nxh=cfg.nxh, sample=SAMPLE, scipy_ms_per_member=round(per, 3), ms_per_swap_extrapolated=round(per * B, 1),
                pole_err_sample=float(max(errs)))


if __name__ == "__main__":
    args = sys.argv[1:]
    what = [a for a in args if a in ("place", "host")] or ["place", "host"]
    if "place" in what:
        for B in [int(a) for a in args if a.isdigit()] or [65536, 1024]:
            print(json.dumps(place(B)), flush=True)
    if "host" in what:
        print(json.dumps(host_alternative()), flush=True)
