"""How much of E'DE a polish assembly needs ("polish assembly"): CPU only, C port + oracle/condense.py.

For the first N instances of the bench batch (synth.make_batch(C3, N, seed=0), cold start) this prints

  a    number of horizon steps with at least one Ŷ bound row active AT THE OPTIMUM (the proxy for "a row in
       A = {lam > s} at polish entry": the C port returns no multipliers; a row counts as active when its slack
       h - G z is below 1e-9 (1 + |h|), three orders above the polish's own acceptance threshold for r_A);
  f_p  polish factorisations per solve of the C port.  The port reports `iters` = passes + polish attempts for a polished
       solve and passes alone otherwise; the pass p* at which a solve ends is found by running the same cold batch with
       max_iter = 1, 2, ..: an instance is solved at max_iter = K exactly when p* < K (the trajectory does not depend on
       max_iter), so attempts = iters - p* for the polished ones.  Solves that end on the interior-point test have
       iters == p*; their failed attempts (at most 4 in the port, 3 in the kernel) are not visible and are bounded.

Usage: python scripts/polish_active_steps.py [N]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpcqp import synth                      # noqa: E402
from oracle import condense as cd, cport     # noqa: E402
from tests.parity_util import constraint_kwargs  # noqa: E402


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    cfg = synth.C3
    bt = synth.make_batch(cfg, N, seed=0)
    ref = cport.from_synth(cfg, bt)
    Z, _, st, it = ref.step(bt["xhat0"], bt["lastu0"], bt["ry"])
    Z, it = Z.copy(), it.copy()
    assert np.all(st == 0), st
    # pass at which each solve ends
    pstar = np.zeros(N, int)
    for K in range(1, int(it.max()) + 2):
        _, _, stK, _ = ref.step(bt["xhat0"], bt["lastu0"], bt["ry"], max_iter=K)
        pstar += (stK != 0)
    att = it - pstar
    pol = att > 0
    print(f"instances {N}: factorisations (passes + polish attempts) mean {it.mean():.3f}; polished {pol.mean():.4f}")
    print(f"polish attempts of the polished solves: mean {att[pol].mean():.3f}, histogram "
          f"{np.bincount(att[pol]).tolist()} (index = attempts)")
    lo = (att[pol].sum() + 0 * (~pol).sum()) / N
    hi = (att[pol].sum() + 3 * (~pol).sum()) / N
    print(f"f_p over all solves: {lo:.3f} .. {hi:.3f} (unpolished solves: 0 .. 3 failed attempts each)")
    print(f"interior-point factorisations per solve (iters - attempts, unpolished at 0 attempts): {(it - att).mean():.3f}")
    # active Ŷ rows at the optimum, by horizon step
    nU, nDU, nY = cfg.nu * cfg.Hp, cfg.nu * cfg.Hc, cfg.ny * cfg.Hp
    off = 2 * nU + 2 * nDU
    a = np.zeros(N, int)
    rows = np.zeros(N, int)
    steps = np.zeros((N, cfg.Hp), bool)
    for i in range(N):
        m = cd.LinMPCOracle(bt["Ahat"][i], bt["Bhu"][i], bt["Chat"][i], Hp=cfg.Hp, Hc=cfg.Hc, Cwt=cfg.Cwt,
                            Mwt=np.full(cfg.ny, cfg.Mwt), Nwt=np.full(cfg.nu, cfg.Nwt), Lwt=np.full(cfg.nu, cfg.Lwt))
        m.setconstraint(**constraint_kwargs(cfg, oracle=True))
        m.initpred(bt["xhat0"][i], bt["lastu0"][i], bt["ry"][i])
        b = m.linconstraint()
        A_y, b_y = m.A[off:off + 2 * nY], b[off:off + 2 * nY]
        fin = np.isfinite(b_y)
        slack = np.where(fin, np.where(fin, b_y, 0.0) - A_y @ Z[i], np.inf)
        act = slack <= 1e-9 * (1.0 + np.abs(np.where(fin, b_y, 0.0)))
        act = act[:nY] | act[nY:]
        rows[i] = act.sum()
        steps[i] = act.reshape(cfg.Hp, cfg.ny).any(axis=1)
        a[i] = steps[i].sum()
    h = np.bincount(a, minlength=cfg.Hp + 1)
    print(f"a (horizon steps with an active Ŷ row, of {cfg.Hp}): mean {a.mean():.3f}, median {int(np.median(a))}, "
          f"90 % {int(np.percentile(a, 90))}, 99 % {int(np.percentile(a, 99))}, max {a.max()}; a = 0: {np.mean(a == 0):.4f}")
    print("histogram of a:", {int(k): int(v) for k, v in enumerate(h) if v})
    print(f"active Ŷ rows per solve: mean {rows.mean():.3f}, max {rows.max()}")
    # matrix-core instructions a masked assembly of these steps issues: tile row I (16 / nu block columns of nu) sees K step
    # kk >= DJ I and issues I + 1 of them there (EtDE_share_, register-operand form)
    QK, DJ, NT = cfg.ny // 4, (cfg.ny // 4) * (16 // cfg.nu), (nDU + 15) // 16
    per_step = [QK * sum(I + 1 for I in range(NT) if t * QK >= DJ * I) for t in range(cfg.Hp)]
    mf = steps @ np.array(per_step)
    print(f"MFMAs of a full assembly: {sum(per_step)} (per horizon step {per_step[0]} .. {per_step[-1]}); of the active steps "
          f"alone: mean {mf.mean():.2f}, max {mf.max()}")


if __name__ == "__main__":
    main()
