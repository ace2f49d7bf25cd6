"""CPU tests of the discretisation of continuous-time models (mpcqp_c2d, mpcqp_set_model_continuous): the body of
csrc/c2d_bodies.h on the CPU wave emulator (tests/emu/emu_c2d.cpp) through the C-ABI and the BatchLinMPC mirror, with the
checks of tests/c2d_util.py, and the host code under the address and undefined-behaviour sanitizers in a stand-alone program.
The GPU tests are in tests/test_gpu_c2d.py."""
import os
import subprocess

import numpy as np
import pytest

import mpcqp
from tests import c2d_util as cu
from tests import emu_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda cases: ["nx%d-nu%d-nd%d-B%d-%s" % (c[0] + (c[1],)) for c in cases]


@pytest.fixture(scope="module")
def c2dlib():
    lib = mpcqp.api.load_library(cu.build())
    yield lib
    mpcqp.api._lib = None


def test_golden_inputs_keep_the_bar_tight():
    """SciPy's own error on every stored member stays at or below 1e-11 (the condition under which 8 e_scipy is a bar)."""
    worst = 0.0
    for shape, method in cu.ACCURACY_CASES:
        g = cu.golden(shape)
        nx, nu, nd, B = shape
        N = nx + nu + (nd if method == "zoh" else 0)
        for b in range(B):
            import scipy.linalg
            e = cu.rel_err(scipy.linalg.expm(cu.block(g, b, N) * g["Ts"][b])[:nx], g["hi"][b][:, :N], g["lo"][b][:, :N])
            worst = max(worst, e)
            assert np.abs(g["lo"][b]).max() <= np.spacing(np.abs(g["hi"][b]).max())
    print("largest e_scipy", worst)
    assert worst <= 1e-11


@pytest.mark.slow
@pytest.mark.parametrize("case", cu.ACCURACY_CASES, ids=ids(cu.ACCURACY_CASES))
def test_emulator_exponential_accuracy(c2dlib, case):
    print("ratios to SciPy", ["%.2f" % r for r in cu.check_accuracy(*case, lib=c2dlib)])


@pytest.mark.slow
def test_emulator_closed_forms(c2dlib):
    cu.check_closed_forms(lib=c2dlib)


@pytest.mark.slow
def test_emulator_tustin(c2dlib):
    print("ratios to SciPy", ["%.2f" % r for r in cu.check_tustin(lib=c2dlib)])


@pytest.mark.slow
@pytest.mark.parametrize("case", [((12, 4, 0, 12), "tustin"), ((12, 4, 2, 6), "tustin"), ((12, 4, 2, 6), "zoh"), ((16, 4, 0, 4), "tustin")],
                         ids=["nd0", "tustin", "zoh", "nx16"])
def test_emulator_augmentation_bit_for_bit(c2dlib, case):
    cu.check_augmentation(*case, lib=c2dlib)


@pytest.mark.slow
@pytest.mark.parametrize("case", [((12, 4, 0, 12), "tustin"), ((12, 4, 2, 6), "tustin"), ((12, 4, 2, 6), "zoh")], ids=["nd0", "tustin", "zoh"])
def test_emulator_handle_path(c2dlib, case):
    cu.check_handle(*case, lib=c2dlib)


@pytest.mark.slow
def test_emulator_refusals_stay_inside_their_member(c2dlib):
    cu.check_refusals(lib=c2dlib)


@pytest.mark.slow
def test_emulator_tiled_batch_equals_its_twin(c2dlib):
    cu.check_tiled(lib=c2dlib)


@pytest.mark.slow
def test_emulator_end_to_end_T8(c2dlib):
    cu.check_end_to_end(lib=c2dlib)


@pytest.mark.slow
def test_emulator_setmodel_continuous_gains(c2dlib):
    cu.check_setmodel_gains(lib=c2dlib)


@pytest.mark.slow
def test_emulator_contract(c2dlib):
    cu.check_contract(lib=c2dlib)


def test_stock_emulator_refuses_the_discretisation():
    lib = mpcqp.api.load_library(emu_util.build())
    try:
        cu.refused_by_stock_library(lib)
    finally:
        mpcqp.api._lib = None


def test_options_validate_before_any_device_call():
    """C2dOptions: the reference's messages for nint and i_ym, the default nint_ym, the sizes."""
    o = mpcqp.C2dOptions(3, 4, 2, 3, 1, nint_ym=None)
    assert (o.nxd, o.nxh, o.nint_ym.tolist(), o.tustin) == (8, 11, [1, 1, 1], True)
    o = mpcqp.C2dOptions(3, 4, 2, 3, 1, nint_u=[1, 0], nint_ym=None, d_method="zoh")
    assert (o.nxd, o.nxh, o.nint_ym.tolist(), o.tustin) == (4, 5, [0, 0, 0], False)
    assert mpcqp.C2dOptions(3, 4, 2, 3, 0, nint_ym=[2, 1], i_ym=[2, 0]).nxh == 7
    for kw in (dict(nint_u=[1]), dict(nint_ym=[1, 1]), dict(nint_u=[-1, 0]), dict(i_ym=[0, 0]), dict(i_ym=[3]), dict(d_method="foh")):
        with pytest.raises(ValueError):
            mpcqp.C2dOptions(3, 4, 2, 3, 0, **kw)


def test_host_code_under_sanitizers(tmp_path):
    """csrc/mpcqp_host.hip compiled for the host with -fsanitize=address,undefined into tests/c2d_asan_main.cpp (its own main),
    with the emulator launcher compiled the same way.  No sanitizer goes into Python."""
    emu_util.build(emu_util.EST)
    exe = str(tmp_path / "c2d_asan")
    subprocess.check_call(emu_util.SANITIZER_CXX + ["-x", "c++", os.path.join(emu_util.CSRC, "mpcqp_host.hip"),
                                                    os.path.join(emu_util.EMU, "emu_c2d.cpp"),
                                                    os.path.join(ROOT, "tests", "c2d_asan_main.cpp"), "-x", "none"]
                          + emu_util.SANITIZER_OBJS + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "c2d asan ok" in out.stdout, out.stdout + out.stderr
