"""Timing of the steady-state Riccati solve of the SteadyKalmanFilter (csrc/kf_kernels.hip: k_kf_dare*, one launch per solve)
on resident data, HIP events around mpcqp_kf_solve_steady_device: median and minimum of 10 after 3 warm-ups, with the mean
doubling-iteration count of the batch.
  * `solve`: C3 shapes at B = 65536 and 1024, nx̂ = 24 and 32 at B = 16384 (models and covariances of scripts/kf_cov_time.py);
             nx̂ = 33, 48 and 64 (csrc/kf_dare_lds_kernels.hip: k_kf_dare_lds, one estimator per workgroup) at B = 65536 and
             1024 -- 256 distinct estimators tiled to B, with SciPy's time per estimator on this host next to it;
  * `host`:  the alternative per model swap at C3, B = 1024 -- steady_kalman_gain (B SciPy DARE solves) plus the upload of K̂.
One JSON line per measurement.
Usage: python scripts/kf_dare_time.py [solve] [host] [B ...] [nxh16|nxh24|nxh32|nxh33|nxh48|nxh64 ...]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402
import mpcqp  # noqa: E402
import kf_cov_time as kt  # noqa: E402


LDS = {33: dict(nx=30, nym=3), 48: dict(nx=42, nym=6), 64: dict(nx=56, nym=8)}       # beyond 32: the LDS-resident kernels
LDS_DISTINCT = 256


def lds_model(nxh, B):
    """The augmented model of an MHE workload of that size and its covariances: LDS_DISTINCT estimators tiled to B."""
    from mpcqp import synth
    mc = synth.MheConfig(f"kf{nxh}", nu=2, nd=0, He=1, **LDS[nxh])
    n = min(B, LDS_DISTINCT)
    bt = synth.make_mhe_batch(mc, n, seed=0)
    Q, R, _ = kt.covariances(np.random.default_rng(1), n, nxh, mc.nym)
    idx = np.arange(B) % n
    return [np.ascontiguousarray(a[idx]) for a in (bt["Ahat"], bt["Bhu"], bt["Chm"], Q, R)] + [mc.nym]


def solve(nxh, B):
    if nxh in LDS:
        A, Bu, C, Q, R, ny = lds_model(nxh, B)
    else:
        _, bt, A, Bu, C, ny = kt.model(nxh, B)
        Q, R, _ = kt.covariances(np.random.default_rng(1), B, nxh, ny)
    nu = Bu.shape[2]
    hd = mpcqp.Handle(B, nxh, nu, ny, 0, 2, 1)
    hd.set_model(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(C))
    t0 = time.perf_counter()
    hd.kf_set_steady(Q, R, np.arange(ny))                       # (uploads Q̂, R̂ and solves once)
    t1 = time.perf_counter()
    med, mn = kt.timed(lambda sp: hd.kf_solve_steady_device(stream=sp))
    it, st = hd.kf_steady_iters(), hd.kf_status()
    nK = min(B, 64)                                             # the result is the host's, on a sample
    t2 = time.perf_counter()
    K = mpcqp.steady_kalman_gain(A[:nK], C[:nK], Q[:nK], R[:nK])
    host_ms = (time.perf_counter() - t2) * 1e3 / nK
    err = float(np.abs(hd.kf_gain()[:nK] - K).max() / max(1.0, np.abs(K).max()))
    return dict(what="solve", nxh=nxh, nym=ny, B=B, lanes=hd.kf_lanes_per_estimator(), solve_median_ms=round(med, 4),
                solve_min_ms=round(mn, 4), mean_iters=round(float(it.mean()), 2), max_iters=int(it.max()),
                not_solved=int((st != 0).sum()), set_steady_wall_ms=round((t1 - t0) * 1e3, 2), gain_err_vs_host_sample=err,
                scipy_ms_per_estimator=round(host_ms, 3))


def host_alternative(B=1024):
    cfg, bt, A, Bu, C, ny = kt.model(16, B)
    Q, R, _ = kt.covariances(np.random.default_rng(1), B, cfg.nxh, ny)
    hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, ny, 0, 2, 1)
    hd.set_model(mpcqp.colmajor(A), mpcqp.colmajor(Bu), mpcqp.colmajor(C))
    t0 = time.perf_counter()
    K = mpcqp.steady_kalman_gain(A, C, Q, R)
    t1 = time.perf_counter()
    hd.kf_set(mpcqp.colmajor(K), np.arange(ny))
    t2 = time.perf_counter()
    return dict(what="host", B=B, nxh=cfg.nxh, dare_ms=round((t1 - t0) * 1e3, 2), upload_ms=round((t2 - t1) * 1e3, 3),
                ms_per_swap=round((t2 - t0) * 1e3, 2))


if __name__ == "__main__":
    args = sys.argv[1:]
    what = [a for a in args if a in ("solve", "host")] or ["solve", "host"]
    Bs = [int(a) for a in args if a.isdigit()]
    sizes = [int(a[3:]) for a in args if a.startswith("nxh")] or [16, 24, 32]
    if "solve" in what:
        for nxh in sizes:
            for B in (Bs or ([65536, 1024] if nxh == 16 or nxh in LDS else [16384])):
                print(json.dumps(solve(nxh, B)), flush=True)
    if "host" in what:
        print(json.dumps(host_alternative()), flush=True)
