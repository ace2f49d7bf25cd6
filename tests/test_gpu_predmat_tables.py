"""K1 on the device, both forms (predmat_body: LDS loops; predmat_mfma: chains of v_mfma_f64_16x16x4), at the fifteen shapes of
tests/predmat_util.py: every entry of Σ, K, B, Gd, ex̂, kx̂, bx̂ and Xd of every member against the 50-digit truth within the
derived error bar, plus the bit-for-bit checks of run_case.  In this process the threshold MPCQP_K1_MFMA_MIN_NX has its
default (10) and predmat_form() must report the form the table of cases names; two child processes (the threshold is read
once per process) force the matrix cores onto every eligible shape, and the LDS loops onto every shape -- the 10 <= nx̂ <= 16
ones included, which the LDS kernel never sees by default.

Measured on an MI355X, worst |device - truth| / bound over the tables of a case (the two forms agree to the three digits
printed wherever both can run: both accumulate with fused multiply-adds in the same order): scalar_Hp1 0.198,
below_one_k_step 0.198, nx9_default_lds 0.150, nx10_default_mfma 0.178, nx16_dense 0.176, cols_16 0.190, cols_17 0.235, ny_16 0.216,
ny_17 0.229, nx17_lds 0.144, nx33_lds 0.086, Hc_eq_Hp 0.242, Hc_1 0.193, unstable 0.136, no_offset 0.212 (B and bx̂ exactly 0)."""
import os
import subprocess
import sys

import pytest

from tests import predmat_util as pu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(pu.CASES))
def test_every_table_at_the_default_threshold(case, hiplib):
    pu.check_reference(case)
    res = pu.run_case(case, form=pu.CASES[case][9])
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("mode,min_nx", [("mfma", "1"), ("lds", "99")])
def test_every_table_on_a_forced_form(mode, min_nx, hiplib, tmp_path):
    """`mfma`: every eligible case (all but cols_17, ny_17, nx17_lds, nx33_lds) must report form 1; `lds`: every case form 0."""
    assert sorted(c for c in pu.CASES if not pu.eligible(c)) == ["cols_17", "nx17_lds", "nx33_lds", "ny_17"]
    truths = str(tmp_path / "truths.pkl")
    pu.dump_truths(truths)
    code = ("import sys; sys.path.insert(0, '.')\n"
            "from tests import predmat_util as pu\n"
            "pu.child(%r)\n" % mode)
    env = dict(os.environ, MPCQP_K1_MFMA_MIN_NX=min_nx)
    out = subprocess.run([sys.executable, "-c", code, truths], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    worst = float(out.stdout.split("WORST")[1].split()[0])
    assert worst <= 1.0, out.stdout[-4000:]
