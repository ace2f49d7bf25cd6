"""The batched ExplicitMPC on the MI355X (csrc/explicit_kernels.hip): the runners of tests/explicit_util.py on the HIP
library, at the bar of tests/test_explicit.py -- 1e-9 * max(1, max|reference|) against the oracle's closed form -H̃⁻¹ q̃."""
import numpy as np
import pytest

import mpcqp
from tests import explicit_util as xu
from tests.test_explicit import SHAPES, _check

BAR = xu.BAR
pytestmark = pytest.mark.gpu


def test_T7_step_against_closed_form(hiplib):
    _check(xu.run_shape(None, nx=3, nu=2, ny=2, Hp=30, Hc=[2, 3, 4, 21], B=3, law=True), law=True)


def test_T7_closed_loop_against_unconstrained_linmpc(hiplib):
    U0, U1 = xu.run_T7_closed_loop(None, law=True)
    assert np.allclose(U0, U1, rtol=1e-3, atol=1e-3)
    assert np.abs(U0 - U1).max() <= BAR * max(1.0, np.abs(U1).max())


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(hiplib, name):
    kw = SHAPES[name]
    _check(xu.run_shape(None, **kw), law=kw.get("law", False))


def test_n65_is_refused(hiplib):
    cfg, bt = xu.random_batch(3, 5, 2, 14, 13, 3)
    with pytest.raises(mpcqp.MpcqpError, match="error -4"):
        xu.make_pair(cfg, bt)


def test_refresh_after_set_model(hiplib):
    r = xu.run_refresh(None)
    print(r)
    assert r["step"] <= BAR and r["law"] <= BAR and r["law_tables"] <= BAR
    assert r["moved"] > 1e-6 and r["law_moved"] > 1e-6


def test_status_policy(hiplib):
    r = xu.run_status_policy(None)
    bad, ok, fl = r["bad"], r["regular"], r["failed"]
    others = [b for b in range(len(ok["st"])) if b != bad]
    assert np.all(ok["fst"] == 0) and fl["fst"][bad] == 2 and np.all(fl["fst"][others] == 0)
    for st in (fl["st"], fl["stl"]):
        assert st[bad] == 2 and np.all(st[others] == 0)
    for Z, u in ((fl["Z"], fl["u"]), (fl["Zl"], fl["ul"])):
        assert np.all(Z[bad] == 0.0) and np.array_equal(u[bad], r["lastu"][bad])
    for k in ("Z", "u", "Y", "Zl", "ul", "tab"):
        assert np.array_equal(fl[k][others], ok[k][others]), k


def test_device_entry_points_on_torch_buffers(hiplib, monkeypatch):
    """B = 67 through the _device entry points on torch buffers: 67 * 40 rows of Z̃ are 41 groups of 64 and a ragged 42nd;
    with the grid capped at 3 wavefronts every wavefront loops over 14 groups.  u0 alone: 268 rows, 4 full groups + 12 rows."""
    import torch
    monkeypatch.setenv("MPCQP_EXPLICIT_WAVES", "3")
    B = 67
    cfg, bt = xu.random_batch(12, 4, 4, 12, 10, B, seed=8)
    mpc, orcs = xu.make_pair(cfg, bt, law=True)
    inp = xu.period_inputs(cfg, bt, seed=8)
    Zo, Uo, Yo = xu.oracle_period(orcs, inp)
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    x, lu, ry = t(inp["x"]), t(inp["lastu"]), t(inp["ry"])
    new = lambda *s, dt=torch.float64: torch.full(s, -7, dtype=dt, device=dev)
    Z, u0, Y, st = new(B, mpc.nZ), new(B, 4), new(B, mpc.nY), new(B, dt=torch.int32)
    Zl, ul, ul2, stl = new(B, mpc.nZ), new(B, 4), new(B, 4), new(B, dt=torch.int32)
    s = torch.cuda.current_stream().cuda_stream
    mpc.hd.set_flags(mpc.hd.flags | mpcqp.FLAG_RY_CONSTANT)
    p = lambda a: a.data_ptr()
    mpc.hd.explicit_step_device(p(x), p(lu), p(ry), p(Z), p(u0), p(st), Yhat0=p(Y), stream=s)
    mpc.hd.explicit_law_device(p(x), p(lu), p(ry), p(ul), p(stl), Z=p(Zl), stream=s)
    mpc.hd.explicit_law_device(p(x), p(lu), p(ry), p(ul2), p(stl), stream=s)
    torch.cuda.synchronize()
    g = lambda a: a.cpu().numpy()
    assert np.all(g(st) == 0) and np.all(g(stl) == 0)
    errs = dict(Z=xu.err(g(Z), Zo), u=xu.err(g(u0), Uo), Y=xu.err(g(Y), Yo), law_Z=xu.err(g(Zl), Zo), law_u=xu.err(g(ul), Uo),
                law_vs_step=xu.err(g(Zl), g(Z)))
    print(errs)
    assert max(errs.values()) <= BAR and np.array_equal(g(ul2), g(ul))
