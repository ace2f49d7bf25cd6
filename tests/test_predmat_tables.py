"""K1's LDS form (predmat_body) on the CPU emulator at all fifteen shapes of tests/predmat_util.py: every entry of Σ, K, B, Gd,
ex̂, kx̂, bx̂ and Xd of every member against the 50-digit truth, within the derived error bar; the tables without and with the
terminal bound, member 3 alone, and setmodel with the members reversed, bit for bit.  The emulator has no matrix-core form:
predmat_form() is 0 everywhere."""
import pytest

from mpcqp import api
from tests import emu_util, predmat_util as pu


@pytest.fixture(scope="module")
def emulib():
    lib = api.load_library(emu_util.build())
    yield lib
    api._lib = None


@pytest.mark.parametrize("case", list(pu.CASES))
def test_reference_has_a_tight_bar_and_no_empty_table(case):
    """On the reference alone: the bound's largest entry is at most 1e-10 of the table's largest entry, and no table's truth
    is all zero except B and bx̂ without an offset (then both, and their bounds, are exactly zero)."""
    rel = pu.check_reference(case)
    print("%-18s largest bound / largest entry %.2e" % (case, rel))


def test_float64_recurrences_stay_well_inside_the_bar():
    """The bar is no formality the other way either: a plain float64 NumPy evaluation of the kernel's recurrences (not the
    kernel) uses part of it, and a relative perturbation of 1e-9 of one table breaks it."""
    import numpy as np
    case = "nx16_dense"
    nx, nu, ny, nd, Hp, Hc = pu.CASES[case][:6]
    m, (tr, bd) = pu.model(case), pu.truth(case)
    got = {k: np.zeros(tr[k].shape) for k in pu.TABLES}
    jl = np.concatenate([[0], np.cumsum(pu.blocking(case))])
    for i in range(pu.NB):
        A, C = m["A"][i], m["C"][i]
        c0 = np.hstack([m["Bu"][i], m["dop"][i][:, None], np.zeros((nx, nd))])
        W, P, T = np.hstack([m["Bu"][i], m["dop"][i][:, None], m["Bd"][i]]), C @ A, A.copy()
        for t in range(Hp):
            CW = C @ W
            got["S"][i, t], got["B"][i, t * ny:(t + 1) * ny], got["Gd"][i, t] = CW[:, :nu].T, CW[:, nu], CW[:, nu + 1:]
            got["K"][i, :, t * ny:(t + 1) * ny] = P.T
            got["Xd"][i, t] = W[:, nu + 1:]
            for j in range(Hc):
                if t == Hp - jl[j] - 1:
                    got["ex"][i, j] = W[:, :nu]
            if t == Hp - 1:
                got["bx"][i], got["kx"][i] = W[:, nu], T.T
            W, P, T = A @ W + c0, P @ A, T @ A
    res = pu.ratios(case, got)
    print(res)
    assert 0.0 < max(res.values()) <= 1.0, res
    got["Gd"] = got["Gd"] * (1 + 1e-9)
    assert pu.ratios(case, got)["Gd"] > 1.0


@pytest.mark.parametrize("case", list(pu.CASES))
def test_every_table_of_the_lds_form_on_the_emulator(case, emulib):
    res = pu.run_case(case, lib=emulib, form=0)
    assert max(res.values()) <= 1.0, res
