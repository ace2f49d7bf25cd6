"""Team-size invariance of the team step kernels (k_step_team<SD, T>, csrc/mpcqp_devwave.h).

A team of T wavefronts shares the work of wavefront 0's step: the same operations per entry, disjoint entries per wavefront.
So the results of one problem are BIT-IDENTICAL whatever the team size -- which makes the comparison of two team sizes the
sharpest detector there is for a wrong share, a missing barrier, a helper that reads its mailbox arguments too early or a DPP
read hazard: each of them changes bits, while an interior-point iteration compared with an oracle at 1e-5 converges past it.
None of that code runs on the CPU emulator (NTEAM = 1 there).

Every case runs as the product default (no flag), with -DMPCQP_TEAM=1, =2 and =4, each in a fresh child process with a
private specialisation cache (tests/team_util.py); every array of every period must be equal, every variant must have been
accepted by mpcqp_prepare's self-test (KERNEL_ONDEMAND), and the cached object must really hold the claimed kernel.

The GPU children run one after another, each under its own time limit.  A child that ends by a signal, an abort or its
time limit ends the whole pytest session (pytest.exit, non-zero): nothing more is started on a device that may have faulted.

Compile cost: 32 objects of 25 - 60 s each.  The plain shapes are prebuilt concurrently (mpcqp_prebuild needs no GPU); the
variants with custom rows or dense weights compile inside their child's mpcqp_prepare.  MPCQP_TEAM_TEST_CACHE=<dir> keeps
the objects between runs (default: a temporary directory)."""
import os
import time

import numpy as np
import pytest

import mpcqp
from tests import team_util as tu

pytestmark = pytest.mark.gpu
T0 = time.time()


@pytest.fixture(scope="module")
def cache_root(tmp_path_factory, hiplib):
    """The root of the private caches, with the plain-shape objects of every variant built (concurrently, no GPU)."""
    root = os.environ.get("MPCQP_TEAM_TEST_CACHE") or str(tmp_path_factory.mktemp("team_cache"))
    os.makedirs(root, exist_ok=True)
    jobs, seen = [], set()
    for c in tu.CASES.values():
        if c.plain and c.obj == c.name and c.obj not in seen:
            seen.add(c.obj)
            jobs += [(c.name, T, tu.make_cache(root, c.obj, T)) for T in tu.VARIANTS]
    t = time.time()
    tu.prebuild_many(jobs)
    print(f"\n[team] {len(jobs)} plain-shape objects prebuilt in {time.time() - t:.0f} s")
    yield root
    print(f"\n[team] tests/test_gpu_team.py: {time.time() - T0:.0f} s wall time")


@pytest.mark.parametrize("case", list(tu.CASES))
def test_results_do_not_depend_on_the_team_size(case, cache_root, tmp_path):
    c = tu.CASES[case]
    runs = {}
    for T in tu.VARIANTS:
        cache = tu.make_cache(cache_root, c.obj, T)
        try:
            runs[T] = tu.run_variant(case, T, cache, str(tmp_path / f"{case}_T{T}.npz"))
        except tu.ChildDied as e:
            pytest.exit(f"GPU child died, no further GPU process is started: {e}", returncode=3)
        # accepted by mpcqp_prepare's comparison with the runtime-dimension kernel
        assert int(runs[T]["kind"]) == mpcqp.api.KERNEL_ONDEMAND, (case, T, int(runs[T]["kind"]))
        # the object the child loaded holds the kernel this variant claims (a flag that silently did nothing fails here)
        objs = tu.spec_objects(cache)
        assert len(objs) == 1, objs
        team = tu.team_of_symbols(tu.kernel_symbols(objs[0], str(tmp_path / f"syms_T{T}")))
        assert team == (T or c.auto), f"{case}: MPCQP_TEAM={T or 'unset'} built a team of {team}, expected {T or c.auto}"
        assert int(runs[T]["periods"]) == c.periods >= 2
        assert runs[T]["p0_Z"].shape == (tu.B_TEAM, c.nZ) and tu.B_TEAM >= 96
    # the members are different problems (a batch of copies would hide a share that depends on the workgroup's neighbours)
    assert len(np.unique(runs[1]["p0_Z"], axis=0)) == tu.B_TEAM
    for a, b in ((1, 2), (1, 4), (2, 4), (0, c.auto)):
        d = tu.first_difference(runs[a], runs[b])
        assert d is None, (f"{case} ({c.why}): team sizes {a or 'default'} and {b} differ first in period {d[0]}, array {d[1]}, "
                           f"entry (member, index) {d[2]}: {d[3]!r} vs {d[4]!r}")
