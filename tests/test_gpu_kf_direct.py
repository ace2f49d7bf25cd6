"""GPU tests of the predictor form (direct=False) and of missing measurements in the Kalman filters of the LinMPC loop: the
cases of tests/test_kf_direct.py on the HIP library (k_kf_cov<NX> / k_kf_cov_wide<NX> with the NaN rule, kf_correct_lds in
the condensed and the stage step kernels in both placements, mpcqp_kf_update), at the same shapes and bars."""
import numpy as np
import pytest

from tests import kf_direct_util as kd
from tests import kf_util as ku
from tests.test_kf_direct import check_miss_and_drop

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("steady", [True, False], ids=["steady", "time-varying"])
def test_predictor_form_is_the_filter_form_reordered(hiplib, steady):
    """C2, B = 6, 8 periods: x̂0, P̂ and K̂ of the two forms bit-equal after every period; preparestate of the predictor form does
    nothing and its moveinput is a plain controller's on x̂ₖ₋₁(k)."""
    assert kd.run_forms(steady) > 1e-2


@pytest.mark.parametrize("shape,lanes", [(ku.shape_c2, 16), (ku.shape_ym, 16), (ku.shape_17, 64), (ku.shape_32, 64)],
                         ids=["C2-B6", "iym20-nd1-B5", "nx17-B3", "nx32-B3"])
def test_misses_per_member(hiplib, shape, lanes):
    """12 periods with per-member misses (one NaN channel or all) and one period with ym=None, both kernel families: a missed
    correction keeps x̂0, P̂, K̂ bit for bit with status 1, everything follows NumPy at the bars."""
    res = kd.run_misses(shape())
    print(res)
    assert res["lanes"] == lanes and res["nmiss"] > 0
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR and res["ex"] <= kd.XBAR, res


@pytest.mark.parametrize("shape,lanes", [(ku.shape_c2, 16), (ku.shape_17, 64)], ids=["C2-B6", "nx17-B3"])
def test_misses_per_member_predictor_form(hiplib, shape, lanes):
    res = kd.run_misses(shape(), direct=False)
    print(res)
    assert res["lanes"] == lanes
    assert res["eK"] <= ku.BAR and res["eP"] <= ku.BAR and res["ex"] <= kd.XBAR, res


def test_miss_and_drop_together(hiplib):
    """B = 5, estimator 3 with R̂ = -10 I, NaN for estimator 1 in period 1 and for estimator 3 in period 2: statuses follow the
    0 / 1 / 2 rule, and estimator 3's P̂ has been predicted after its miss."""
    check_miss_and_drop(None)


@pytest.mark.parametrize("ms", [False, True], ids=["condensed", "MultipleShooting"])
@pytest.mark.parametrize("tv", [True, False], ids=["time-varying", "steady"])
@pytest.mark.parametrize("direct", [1, 0], ids=["direct1", "direct0"])
def test_fused_equals_separate_with_misses(hiplib, direct, tv, ms):
    """mpcqp_loop_device against the separate entry points on torch device buffers, B = 64, five periods, NaN in a tenth of the
    (estimator, period) pairs: x̂0, u0, Z̃, K̂ and P̂ differ by exactly 0.0; the missed estimators' step statuses are 0."""
    import torch
    diff, kmax, nmiss = kd.fused_variants(direct, tv, ms, torch_device=torch.device("cuda", 0))
    assert diff == 0.0 and kmax > 1e-2 and nmiss > 10, (diff, kmax, nmiss)
