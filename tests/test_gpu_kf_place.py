"""GPU tests of the Luenberger observer built from its poles (csrc/kf_place_kernels.hip: k_kf_place<NX>, one member per
wavefront) through the C-ABI and the BatchLinMPC mirror: the checks of tests/kf_place_util.py, the same ones
tests/test_kf_place.py runs on the CPU wave emulator, with the same bars."""
import numpy as np
import pytest

from tests import kf_place_util as pu

pytestmark = pytest.mark.gpu
ids = lambda cases: ["n%d-m%d-B%d" % c[:3] for c in cases]


@pytest.mark.parametrize("shape", pu.CASES, ids=ids(pu.CASES))
def test_poles_are_placed(hiplib, shape):
    """(16, 4) and below keep the reflectors of every admissible subspace in LDS; (32, 8) rebuilds them at each visit."""
    pu.check_placed(pu.make_case(*shape))


def test_closed_form(hiplib):
    pu.check_closed_form()


@pytest.mark.parametrize("spec", pu.SWEEP_CASES, ids=ids(pu.SWEEP_CASES))
def test_sweeps_do_their_work(hiplib, spec):
    pu.check_sweeps(spec)


@pytest.mark.parametrize("shape", pu.DEFAULT_POLE_CASES, ids=ids(pu.DEFAULT_POLE_CASES))
def test_reference_default_poles(hiplib, shape):
    n, m, B = shape
    pu.check_placed(pu.make_case(n, m, B, poles=pu.default_poles(n)))


def test_repeated_poles(hiplib):
    pu.check_placed(pu.make_case(**pu.REPEATED))


def test_refusals_stay_inside_their_member(hiplib):
    pu.check_refusals()


def test_contract(hiplib):
    pu.check_contract(torch_stream=True)


def test_refused_beyond_32_states(hiplib):
    case = pu.make_case(33, 1, 2, poles=np.linspace(0.1, 0.8, 33))
    pu.refused_then_kf_set(pu.make_handle(case, place=False), case)


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "predictor"])
def test_controller(hiplib, direct):
    import torch
    pu.check_controller(direct, torch_device=torch.device("cuda", 0))


def test_observer_error(hiplib):
    pu.check_observer_error()


def test_setmodel_and_warning(hiplib):
    pu.check_setmodel_and_warning()


def test_tiled_batch_equals_its_twin(hiplib):
    """The seven models of (16, 4) tiled to B = 1027 (more workgroups than fit the device at once): every member bit-equal to
    its twin of the B = 7 batch."""
    case = pu.make_case(16, 4, 7)
    h7 = pu.make_handle(case)
    B = 1027
    idx = np.arange(B) % 7
    big = dict(case, B=B, **{k: np.ascontiguousarray(case[k][idx]) for k in ("Ahat", "Bhu", "Chat", "poles")})
    hb = pu.make_handle(big)
    assert not h7.kf_status().any() and not hb.kf_status().any()
    assert np.array_equal(hb.kf_place_sweeps(), h7.kf_place_sweeps()[idx])
    assert hb.kf_gain().tobytes() == h7.kf_gain()[idx].tobytes()
