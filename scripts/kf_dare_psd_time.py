"""Timing of the steady-state Riccati solve with a positive SEMIdefinite Q̂ (csrc/kf_kernels.hip: k_kf_dare* followed by the
second pass k_kf_dare_psd*) on resident data, HIP events around mpcqp_kf_solve_steady_device: median and minimum of 10 after 3
warm-ups, with the mean iteration count of the batch and how many estimators the square-root form served.
  * `solve`:    Q̂ = B_w B_w' (the `lowrank` generator of tests/kf_dare_psd_util.py) at C3, B = 65536 and 1024, and at nx̂ = 24
                and 32, B = 16384 (models of scripts/kf_cov_time.py), each beside the definite Q̂ of scripts/kf_dare_time.py on
                the same shape;
  * `definite`: the definite solve alone -- what the added pass costs a batch that does not need it; run it on two builds
                of the library (MPCQP_LIB) in one session;
  * `host`:     the alternative at C3, B = 1024: steady_kalman_gain (B SciPy DARE solves) on the same semidefinite Q̂.
One JSON line per measurement.
Usage: python scripts/kf_dare_psd_time.py [solve] [definite] [host] [B ...] [nxh16|nxh24|nxh32 ...] [run=LABEL]"""
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
import kf_cov_time as kt  # noqa: E402


def lowrank(B, nxh, ny):
    """Q̂ = B_w B_w' with max(1, npl // 3) columns into the npl = nx̂ - ny plant states, diag(U(0.3, 1)) on the integrators."""
    rng = np.random.default_rng(5)
    npl = nxh - ny
    Bw = rng.standard_normal((B, npl, max(1, npl // 3)))
    Q = np.zeros((B, nxh, nxh))
    Q[:, :npl, :npl] = Bw @ Bw.transpose(0, 2, 1)
    Q[:, range(npl, nxh), range(npl, nxh)] = rng.uniform(0.3, 1.0, (B, nxh - npl))
    return 0.5 * (Q + Q.transpose(0, 2, 1))


def solve(nxh, B, semidefinite, run=None):
    _, bt, A, Bu, C, ny = kt.model(nxh, B)
    nu = Bu.shape[2]
    Q, R, _ = kt.covariances(np.random.default_rng(1), B, nxh, ny)
    if semidefinite:
        Q = lowrank(B, nxh, ny)
    hd = mpcqp.Handle(B, nxh, nu, ny, 0, 2, 1)
    hd.set_model(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(C))
    hd.kf_set_steady(Q, R, np.arange(ny))
    med, mn = kt.timed(lambda sp: hd.kf_solve_steady_device(stream=sp))
    it, st = hd.kf_steady_iters(), hd.kf_status()
    path = hd.kf_steady_path() if hasattr(hd.lib, "mpcqp_kf_steady_path") else np.zeros(B, np.int32)
    refused_with_gain = int((hd.kf_gain().any(axis=(1, 2)) & (st != 0)).sum())      # must be 0: a status never comes with a gain
    nK = min(B, 64)                                             # the result is the host's, on a sample
    K = mpcqp.steady_kalman_gain(A[:nK], C[:nK], Q[:nK], R[:nK])
    err = float(np.abs(hd.kf_gain()[:nK] - K).max() / max(1.0, np.abs(K).max()))
    out = dict(what="semidefinite" if semidefinite else "definite", nxh=nxh, nym=ny, B=B, solve_median_ms=round(med, 4),
               solve_min_ms=round(mn, 4), mean_iters=round(float(it.mean()), 2), max_iters=int(it.max()),
               not_solved=int((st != 0).sum()), refused_with_gain=refused_with_gain, square_root_form=int(path.sum()), gain_err_vs_host_sample=err)
    if run:
        out["run"] = run
    return out


def host_alternative(B=1024):
    cfg, bt, A, Bu, C, ny = kt.model(16, B)
    _, R, _ = kt.covariances(np.random.default_rng(1), B, cfg.nxh, ny)
    Q = lowrank(B, cfg.nxh, ny)
    t0 = time.perf_counter()
    mpcqp.steady_kalman_gain(A, C, Q, R)
    t1 = time.perf_counter()
    return dict(what="host", B=B, nxh=cfg.nxh, dare_ms=round((t1 - t0) * 1e3, 2))


if __name__ == "__main__":
    args = sys.argv[1:]
    what = [a for a in args if a in ("solve", "definite", "host")] or ["solve", "host"]
    Bs = [int(a) for a in args if a.isdigit()]
    sizes = [int(a[3:]) for a in args if a.startswith("nxh")] or [16, 24, 32]
    run = next((a[4:] for a in args if a.startswith("run=")), None)
    for nxh in sizes:
        for B in (Bs or ([65536, 1024] if nxh == 16 else [16384])):
            if "solve" in what:
                print(json.dumps(solve(nxh, B, True, run)), flush=True)
            if "solve" in what or "definite" in what:
                print(json.dumps(solve(nxh, B, False, run)), flush=True)
    if "host" in what:
        print(json.dumps(host_alternative()), flush=True)
