"""GPU tests of the discretisation of continuous-time models (csrc/c2d_kernels.hip: k_c2d<NX>, one member per wavefront)
through the C-ABI and the BatchLinMPC mirror: the checks of tests/c2d_util.py, the same ones tests/test_c2d.py runs on the CPU
wave emulator, with the same bars."""
import pytest

from tests import c2d_util as cu

pytestmark = pytest.mark.gpu
ids = lambda cases: ["nx%d-nu%d-nd%d-B%d-%s" % (c[0] + (c[1],)) for c in cases]


@pytest.mark.parametrize("case", cu.ACCURACY_CASES, ids=ids(cu.ACCURACY_CASES))
def test_exponential_accuracy(hiplib, case):
    print("ratios to SciPy", ["%.2f" % r for r in cu.check_accuracy(*case)])


def test_closed_forms(hiplib):
    cu.check_closed_forms()


def test_tustin(hiplib):
    print("ratios to SciPy", ["%.2f" % r for r in cu.check_tustin()])


@pytest.mark.parametrize("case", [((12, 4, 0, 12), "tustin"), ((12, 4, 2, 6), "tustin"), ((12, 4, 2, 6), "zoh"), ((16, 4, 0, 4), "tustin")],
                         ids=["nd0", "tustin", "zoh", "nx16"])
def test_augmentation_bit_for_bit(hiplib, case):
    cu.check_augmentation(*case)


@pytest.mark.parametrize("case", [((12, 4, 0, 12), "tustin"), ((12, 4, 2, 6), "tustin"), ((12, 4, 2, 6), "zoh")], ids=["nd0", "tustin", "zoh"])
def test_handle_path(hiplib, case):
    cu.check_handle(*case)


def test_device_call_on_a_stream_then_step(hiplib):
    cu.check_device_stream()


def test_refusals_stay_inside_their_member(hiplib):
    cu.check_refusals()


def test_tiled_batch_equals_its_twin(hiplib):
    cu.check_tiled()


def test_end_to_end_T8(hiplib):
    cu.check_end_to_end()


def test_setmodel_continuous_gains(hiplib):
    cu.check_setmodel_gains()


def test_contract(hiplib):
    cu.check_contract()
