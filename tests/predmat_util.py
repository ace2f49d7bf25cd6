"""K1 (init_predmat, transcription.jl:115-194) table by table: every prediction table the kernel writes -- Σ, K, B, Gd and the
terminal tables ex̂, kx̂, bx̂, Xd -- read back with mpcqp_get and compared entry by entry with a 50-digit `mpmath` evaluation of
the definitions (powers and cumulative sums, as oracle/condense.init_predmat states them; not the kernel's recurrences), on the
float64 model exactly as it was uploaded.

The error bar is derived, not tuned.  Both forms of the kernel (predmat_body: LDS loops; predmat_mfma: matrix-core chains)
evaluate

    W(t+1) = Â W(t) + [B̂u | dop | 0]      W = [S(t) B̂u | S(t) dop | Â^t B̂d]
    P(t+1) = P(t) Â,  P(0) = Ĉ Â           T(t+1) = T(t) Â,  T(0) = Â
    outputs  Ĉ W(t), P(t), T(Hp-1) and columns of W(t)

and products with the exact zeros of a padded tile add no error.  With u = 2^-53 and γ = k u / (1 - k u), k = nx̂ + 2, any
summation order, fused or not, satisfies component by component (Higham, Accuracy and Stability of Numerical Algorithms,
section 3.5)

    e_W(t+1) = |Â| e_W(t) + γ (|Â| |W(t)| + |[B̂u dop 0]|),  e_W(0) = 0
    e_P(0) = γ |Ĉ| |Â|,  e_P(t+1) = e_P(t) |Â| + γ |P(t)| |Â|;   the same for T with e_T(0) = 0
    error of Ĉ W(t) <= |Ĉ| e_W(t) + γ |Ĉ| |W(t)|

ex̂, bx̂ and Xd take e_W, K takes e_P, kx̂ takes e_T.  The assertion is |device - truth| <= bound for every entry of every table
of every member.  Two conditions, checked on the reference alone (check_reference), keep the bar from hiding anything: the
bound's largest entry is at most 1e-10 of the table's largest entry, and no table's truth is all zero except B and bx̂ when no
offset is given."""
import functools
import os
import pickle
import sys

import numpy as np

import mpcqp
from mpcqp import api

DIGITS = 50
NB = 5                      # members of a case's batch
TABLES = ("S", "K", "B", "Gd", "ex", "kx", "bx", "Xd")
TERMINAL = ("ex", "kx", "bx", "Xd")
GETS = {"S": api.GET_STEPRESP, "K": api.GET_KMAT, "B": api.GET_BVEC, "Gd": api.GET_GDTAB, "ex": api.GET_EXHAT,
        "kx": api.GET_KXHAT, "bx": api.GET_BXHAT, "Xd": api.GET_XDTAB}
MAX_REL_BOUND = 1e-10       # the bound's largest entry over the table's largest entry, at most

# name: (nx̂, nu, ny, nd, Hp, Hc, move-blocking vector or None, ρ, offset given, form at the default threshold, eligible for
# the matrix cores).  The smallest shapes that take each path:
CASES = {
    "scalar_Hp1":        (1, 1, 1, 0, 1, 1, None, 1.0, True, 0, True),         # no recursion step at all; kx̂ = Â; Σ_0 = Ĉ B̂u
    "below_one_k_step":  (3, 2, 2, 1, 5, 3, (1, 1, 3), 1.0, True, 0, True),    # nx̂ < 4: only the first of the four K steps holds data
    "nx9_default_lds":   (9, 3, 2, 2, 7, 3, (1, 2, 4), 1.0, True, 0, True),
    "nx10_default_mfma": (10, 3, 2, 2, 7, 3, (1, 2, 4), 1.0, True, 1, True),   # nx̂ no multiple of 4; uneven blocking moves the ex̂ blocks
    "nx16_dense":        (16, 4, 4, 2, 6, 3, None, 1.0, True, 1, True),        # C3's tile with nothing zero
    "cols_16":           (12, 5, 3, 10, 5, 2, None, 1.0, True, 1, True),       # nu + 1 + nd = 16: lane 15 of a row is a Gd column
    "cols_17":           (12, 5, 3, 11, 5, 2, None, 1.0, True, 0, False),      # one past
    "ny_16":             (11, 2, 16, 1, 4, 2, None, 1.0, True, 1, True),       # every Ĉ row of the tile
    "ny_17":             (11, 2, 17, 1, 4, 2, None, 1.0, True, 0, False),
    "nx17_lds":          (17, 2, 2, 1, 5, 2, None, 1.0, True, 0, False),       # nx̂² > 4 · 64 elements per strided loop
    "nx33_lds":          (33, 3, 2, 1, 4, 2, None, 1.0, True, 0, False),       # 18 passes of the strided loops
    "Hc_eq_Hp":          (12, 2, 2, 0, 6, 6, None, 1.0, True, 1, True),        # ex̂ block j at t = Hp - j - 1 for every j
    "Hc_1":              (12, 2, 2, 1, 6, 1, None, 1.0, True, 1, True),        # one block, taken at the last step
    "unstable":          (12, 2, 2, 1, 20, 4, None, 1.3, True, 1, True),       # growth of about 190 over the horizon
    "no_offset":         (10, 3, 2, 2, 7, 3, (1, 2, 4), 1.0, False, 1, True),  # B and bx̂ exactly 0.0
}


def blocking(case):
    """the move-blocking vector of a case (the default: Hc - 1 single steps, the rest in the last interval)"""
    _, _, _, _, Hp, Hc, nb = CASES[case][:7]
    return list(nb) if nb is not None else [1] * (Hc - 1) + [Hp - Hc + 1]


@functools.lru_cache(maxsize=None)
def model(case):
    """B = 5 heterogeneous members, member i from default_rng([seed, i]): Â dense and non-symmetric (an orthogonal similarity of
    a diagonal in ρ·[0.3, 1] plus 0.2/√nx̂ times a strictly upper-triangular normal matrix), B̂u, Ĉ, B̂d and f̂op - x̂op dense
    normal draws with no structural zero.  Arrays with a leading batch axis; Dd is zero (K1 does not read it)."""
    nx, nu, ny, nd, Hp, Hc, _, rho, offset = CASES[case][:9]
    seed = list(CASES).index(case)
    A, Bu, C, Bd, dop = [], [], [], [], []
    for i in range(NB):
        rng = np.random.default_rng([seed, i])
        Q, _ = np.linalg.qr(rng.standard_normal((nx, nx)))
        lam = rho * rng.uniform(0.3, 1.0, nx)
        A.append(Q @ np.diag(lam) @ Q.T + 0.2 / np.sqrt(nx) * np.triu(rng.standard_normal((nx, nx)), 1))
        Bu.append(rng.standard_normal((nx, nu)))
        C.append(rng.standard_normal((ny, nx)))
        Bd.append(rng.standard_normal((nx, nd)))
        dop.append(rng.standard_normal(nx) if offset else np.zeros(nx))
    out = dict(A=np.array(A), Bu=np.array(Bu), C=np.array(C), Bd=np.array(Bd), dop=np.array(dop))
    for a in out.values():
        a.setflags(write=False)
    return out


def _mp(a):
    import mpmath as mp
    a = np.asarray(a, float)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = mp.mpf(float(a[idx]))
    return out


def _member_truth(A, Bu, C, Bd, dop, Hp, jl):
    """The eight tables of one member in the layouts of mpcqp_get (object arrays of mpf), and their bounds (float64)."""
    import mpmath as mp
    nx, nu = Bu.shape
    ny, nd = C.shape[0], Bd.shape[1]
    with mp.workdps(DIGITS):
        Am, Bm, Cm, Bdm, dm = _mp(A), _mp(Bu), _mp(C), _mp(Bd), _mp(dop)
        eye = _mp(np.eye(nx))
        Apow = [eye]                                           # Â^j, j = 0 .. Hp            (transcription.jl:122-126)
        for j in range(Hp):
            Apow.append(Apow[-1].dot(Am))
        S = [Apow[0]]                                          # S(m) = Â^0 + ... + Â^m      (transcription.jl:128)
        for j in range(1, Hp):
            S.append(S[-1] + Apow[j])
        SB = [S[t].dot(Bm) for t in range(Hp)]                 # S(t) B̂u
        Sd = [S[t].dot(dm) for t in range(Hp)]                 # S(t)(f̂op - x̂op)
        AX = [Apow[t].dot(Bdm) for t in range(Hp)]             # Â^t B̂d
        P = [Cm.dot(Apow[t + 1]) for t in range(Hp)]           # Ĉ Â^(t+1)
        tr = {
            "S": np.array([Cm.dot(SB[t]).T for t in range(Hp)], dtype=object).reshape(Hp, nu, ny),
            "K": np.concatenate(P, axis=0).T,
            "B": np.concatenate([Cm.dot(Sd[t]) for t in range(Hp)]),
            "Gd": np.array([Cm.dot(AX[t]) for t in range(Hp)], dtype=object).reshape(Hp, ny, nd),
            "ex": np.array([SB[Hp - jl[j] - 1] for j in range(len(jl) - 1)], dtype=object).reshape(len(jl) - 1, nx, nu),
            "kx": Apow[Hp].T.copy(),                           # column-major Â^Hp
            "bx": Sd[Hp - 1],
            "Xd": np.array(AX, dtype=object).reshape(Hp, nx, nd),
        }
        f = lambda a: np.abs(a).astype(float)
        # |W(t)|, |P(t)|, |T(t)| of the recurrences, from the truth
        aW = [np.hstack([f(SB[t]), f(Sd[t])[:, None], f(AX[t])]) for t in range(Hp)]
        aP = [f(P[t]) for t in range(Hp)]
        aT = [f(Apow[t + 1]) for t in range(Hp)]
    aA, aC = np.abs(A), np.abs(C)
    c0 = np.hstack([np.abs(Bu), np.abs(dop)[:, None], np.zeros((nx, nd))])
    k = nx + 2
    g = k * 2.0 ** -53 / (1 - k * 2.0 ** -53)
    eW, eP, eT = [np.zeros((nx, nu + 1 + nd))], [g * aC @ aA], [np.zeros((nx, nx))]
    for t in range(Hp - 1):
        eW.append(aA @ eW[t] + g * (aA @ aW[t] + c0))
        eP.append(eP[t] @ aA + g * aP[t] @ aA)
        eT.append(eT[t] @ aA + g * aT[t] @ aA)
    eCW = [aC @ eW[t] + g * aC @ aW[t] for t in range(Hp)]     # error of Ĉ W(t): columns [Σ | B | Gd]
    bd = {
        "S": np.array([eCW[t][:, :nu].T for t in range(Hp)]).reshape(Hp, nu, ny),
        "K": np.concatenate(eP, axis=0).T,
        "B": np.concatenate([eCW[t][:, nu] for t in range(Hp)]),
        "Gd": np.array([eCW[t][:, nu + 1:] for t in range(Hp)]).reshape(Hp, ny, nd),
        "ex": np.array([eW[Hp - jl[j] - 1][:, :nu] for j in range(len(jl) - 1)]).reshape(len(jl) - 1, nx, nu),
        "kx": eT[Hp - 1].T.copy(),
        "bx": eW[Hp - 1][:, nu],
        "Xd": np.array([eW[t][:, nu + 1:] for t in range(Hp)]).reshape(Hp, nx, nd),
    }
    return tr, bd


_loaded = {}      # truths handed over by a parent process (load_truths)


@functools.lru_cache(maxsize=None)
def truth(case):
    """(truth, bound): {table: array with a leading batch axis}; computed once per process and case, never modified."""
    if case in _loaded:
        return _loaded[case]
    nx, nu, ny, nd, Hp, Hc = CASES[case][:6]
    m = model(case)
    jl = np.concatenate([[0], np.cumsum(blocking(case))]).astype(int)
    per = [_member_truth(m["A"][i], m["Bu"][i], m["C"][i], m["Bd"][i], m["dop"][i], Hp, jl) for i in range(NB)]
    tr = {k: np.stack([p[0][k] for p in per]) for k in TABLES}
    bd = {k: np.stack([p[1][k] for p in per]) for k in TABLES}
    for a in list(tr.values()) + list(bd.values()):
        a.setflags(write=False)
    return tr, bd


def dump_truths(path):
    with open(path, "wb") as f:
        pickle.dump({c: truth(c) for c in CASES}, f)


def load_truths(path):
    with open(path, "rb") as f:
        _loaded.update(pickle.load(f))


def check_reference(case):
    """The two conditions on the reference alone; returns the largest bound / largest entry over the tables."""
    tr, bd = truth(case)
    nd, offset = CASES[case][3], CASES[case][8]
    worst = 0.0
    for k in TABLES:
        if nd == 0 and k in ("Gd", "Xd"):
            assert tr[k].size == 0
            continue
        for i in range(NB):
            top = float(np.abs(tr[k][i]).max())
            if k in ("B", "bx") and not offset:
                assert top == 0.0 and bd[k][i].max() == 0.0, (case, k, i)
                continue
            assert top > 0.0, (case, k, i, "truth is all zero")
            rel = bd[k][i].max() / top
            assert rel <= MAX_REL_BOUND, (case, k, i, rel)
            worst = max(worst, rel)
    return worst


def controller(case, lib=None, members=None, reverse=False):
    """A BatchLinMPC of the case's members (all five, or the listed ones), without bounds."""
    nx, nu, ny, nd, Hp, Hc = CASES[case][:6]
    kw = _model_args(case, members, reverse)
    mpc = mpcqp.BatchLinMPC(kw["A"], kw["Bu"], kw["C"], kw["Bd"], kw["Dd"], Hp=Hp, Hc=blocking(case), fhop=kw["dop"], lib=lib)
    assert (mpc.Hc, list(mpc.nb)) == (Hc, blocking(case))
    return mpc


def _model_args(case, members=None, reverse=False):
    nd, ny = CASES[case][3], CASES[case][2]
    m = model(case)
    idx = list(range(NB)) if members is None else list(members)
    if reverse:
        idx = idx[::-1]
    out = {k: np.ascontiguousarray(m[k][idx]) for k in ("A", "Bu", "C", "dop")}
    out["Bd"] = np.ascontiguousarray(m["Bd"][idx]) if nd else None
    out["Dd"] = np.zeros((len(idx), ny, nd)) if nd else None
    return out


def read_tables(mpc, names):
    nd = mpc.nd
    return {k: (np.zeros((mpc.B, 0)) if nd == 0 and k in ("Gd", "Xd") else mpc.hd.get(GETS[k])) for k in names}


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def ratios(case, got):
    """|device - truth| / bound, the worst entry of each table over the batch (0/0, an exact zero against a zero bound, is 0)."""
    import mpmath as mp
    tr, bd = truth(case)
    out = {}
    for k in TABLES:
        if tr[k].size == 0:
            continue
        assert got[k].shape == tr[k].shape, (case, k, got[k].shape, tr[k].shape)
        assert np.all(np.isfinite(got[k])), (case, k)
        with mp.workdps(DIGITS):
            err = np.abs(_mp(got[k]) - tr[k]).astype(float)
        r = np.where(err == 0.0, 0.0, err / np.where(bd[k] > 0.0, bd[k], np.finfo(float).tiny))
        out[k] = float(r.max())
    return out


def run_case(case, lib=None, form=None):
    """Everything the case checks on one library; returns {table: worst ratio}.  `form`: what predmat_form() has to report."""
    terminal_bound = {"x̂max": np.full(CASES[case][0], 1e3)}
    mpc = controller(case, lib)
    if form is not None:
        assert mpc.hd.predmat_form() == form, (case, mpc.hd.predmat_form(), form)
    plain = read_tables(mpc, TABLES[:4])                     # without terminal rows
    mpc.setconstraint(**terminal_bound)
    got = read_tables(mpc, TABLES)
    res = ratios(case, got)
    print("%-18s form %s  " % (case, mpc.hd.predmat_form()) + "  ".join("%s %.3f" % kv for kv in res.items()), flush=True)
    for k in TABLES[:4]:                                      # the terminal rows do not disturb the others
        assert same_bits(plain[k], got[k]), (case, k, "changes with the terminal bound")
    one = controller(case, lib, members=[3])                 # member 3 alone
    one.setconstraint(**terminal_bound)
    alone = read_tables(one, TABLES)
    for k in TABLES:
        assert same_bits(alone[k][0], got[k][3]), (case, k, "member 3 alone differs from member 3 of the batch")
    kw = _model_args(case, reverse=True)                     # setmodel follows
    mpc.setmodel(kw["A"], kw["Bu"], kw["C"], kw["Bd"], kw["Dd"], fhop=kw["dop"])
    rev = read_tables(mpc, TABLES)
    for k in TABLES:
        assert same_bits(rev[k], got[k][::-1]), (case, k, "setmodel with the members reversed")
    return res


def eligible(case):
    return CASES[case][10]


def child(mode):
    """Body of the GPU test's child processes (the threshold is read once per process): every case on the form the mode
    forces -- "mfma": MPCQP_K1_MFMA_MIN_NX=1, every eligible case on the matrix cores; "lds": =99, every case on the LDS loops
    -- against the truths of the file argv[1]; prints the worst ratio."""
    load_truths(sys.argv[1])
    assert os.environ["MPCQP_K1_MFMA_MIN_NX"] == {"mfma": "1", "lds": "99"}[mode]
    worst = 0.0
    for case in CASES:
        res = run_case(case, form=1 if mode == "mfma" and eligible(case) else 0)
        worst = max([worst] + list(res.values()))
    print("WORST", worst, flush=True)
