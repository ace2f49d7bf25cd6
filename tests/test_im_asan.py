"""Host code of the InternalModel entry points under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
(tests/im_asan_main.cpp, its own main) around csrc/mpcqp_host.hip, in the manner of tests/test_kf_cov.py.  CPU only; no
sanitizer goes into Python."""
import os
import subprocess

import pytest

from tests import emu_util, im_util as iu

pytestmark = pytest.mark.slow
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_under_sanitizers(tmp_path):
    emu_util.build(emu_util.EST)
    iu.build()
    exe = str(tmp_path / "im_asan")
    objs = emu_util.SANITIZER_OBJS + [os.path.join(emu_util.EMU, "emu_im.o")]
    subprocess.check_call(emu_util.SANITIZER_CXX + ["-x", "c++", os.path.join(emu_util.CSRC, "mpcqp_host.hip"),
                                                    os.path.join(ROOT, "tests", "im_asan_main.cpp"), "-x", "none"] + objs + ["-ldl", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "im asan ok" in out.stdout, out.stdout + out.stderr
