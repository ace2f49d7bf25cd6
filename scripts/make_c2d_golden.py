"""Inputs and 60-digit truths of the discretisation tests (tests/c2d_util.py), written to tests/golden/c2d/<shape>.npz.

Per shape (nx, nu, nd, B): continuous models of three families, each member with a sample time that scales the 1-norm of
M Ts, M = [[A, Bu, Bd], [0, 0]], to 0.01, 1, 30 or 300:
    stable      eigenvalues in -[0.02, 1] under a random similarity, plus 0.3 times a skew-symmetric matrix
    stiff       symmetric, eigenvalues -1e-3 ... -1e3
    non-normal  strictly upper triangular N(0, 1) * 3, minus a diagonal in [0.1, 1]
and the first nx rows [Φ Γu Γd] of exp(M Ts) by mpmath.expm at 60 digits, stored as a pair of doubles hi + lo.  The block
without Bd (the Tustin treatment of the measured disturbances) is the leading part of the same rows.

    python scripts/make_c2d_golden.py            # a few minutes; needs mpmath
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "c2d")
SHAPES = [(1, 1, 0, 3), (2, 1, 0, 12), (12, 4, 0, 12), (12, 4, 2, 6), (28, 4, 0, 4), (16, 4, 0, 4)]
NORMS = (0.01, 1.0, 30.0, 300.0)
COMBOS = [(f, s) for s in range(4) for f in range(3)]       # member b: COMBOS[5 b mod 12] (family, norm)


def ny_of(nx):
    return 1 if nx <= 2 else 4


def family(rng, f, nx):
    if f == 0:
        S = rng.standard_normal((nx, nx)) + 2.0 * np.eye(nx)
        G = rng.standard_normal((nx, nx)) / np.sqrt(nx)
        return S @ np.diag(-rng.uniform(0.02, 1.0, nx)) @ np.linalg.inv(S) + 0.3 * (G - G.T)
    if f == 1:
        Q, _ = np.linalg.qr(rng.standard_normal((nx, nx)))
        A = Q @ np.diag(-np.logspace(-3, 3, nx)) @ Q.T
        return 0.5 * (A + A.T)
    return np.triu(3.0 * rng.standard_normal((nx, nx)), 1) - np.diag(rng.uniform(0.1, 1.0, nx))


def make(shape):
    nx, nu, nd, B = shape
    ny = ny_of(nx)
    rng = np.random.default_rng(1000 * nx + 10 * nu + nd)
    N = nx + nu + nd
    d = {k: [] for k in ("A", "Bu", "Bd", "C", "Dd", "Ts", "hi", "lo", "family", "norm")}
    mp.mp.dps = 60
    for b in range(B):
        f, s = COMBOS[(5 * b) % 12]
        A, Bu, Bd = family(rng, f, nx), rng.standard_normal((nx, nu)), rng.standard_normal((nx, nd))
        M = np.zeros((N, N))
        M[:nx] = np.hstack([A, Bu, Bd])
        Ts = NORMS[s] / np.linalg.norm(M, 1)
        E = mp.expm(mp.matrix(M.tolist()) * mp.mpf(Ts))
        hi = np.array([[float(E[i, j]) for j in range(N)] for i in range(nx)])
        lo = np.array([[float(E[i, j] - mp.mpf(hi[i, j])) for j in range(N)] for i in range(nx)])
        for k, v in zip(d, (A, Bu, Bd, rng.standard_normal((ny, nx)), rng.standard_normal((ny, nd)), Ts, hi, lo, f, s)):
            d[k].append(v)
        print(shape, "member", b, "family", f, "norm", NORMS[s], flush=True)
    os.makedirs(OUT, exist_ok=True)
    np.savez(os.path.join(OUT, "%d_%d_%d_%d.npz" % shape), **{k: np.array(v) for k, v in d.items()})


if __name__ == "__main__":
    for shape in SHAPES:
        if len(sys.argv) == 1 or "%d_%d_%d_%d" % shape in sys.argv[1:]:
            make(shape)
