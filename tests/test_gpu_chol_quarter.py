"""In-panel update of the one-wavefront, one-row-per-lane factorisation on quarter tiles (csrc/mpcqp_bodies.h:
Step::chol_block_update_q4).

After each block of four columns of a 16-column panel the later column blocks of the panel are updated with one
v_mfma_f64_4x4x4_4b per (row tile, later column block) instead of one v_mfma_f64_16x16x4 per row tile.  The arithmetic per
entry is the same; what can go wrong is an index: the B operand's row (clamped in the matrix's last, ragged column block),
the result lane's entry (row block q, row i, column j), the entries without a slot (above the diagonal in the panel's own
tile, rows beyond n in a ragged last tile) and the order of the write-backs.  The runtime-dimension kernel keeps the left-
looking factorisation on the packed layout, so it is the reference inside the library; the oracle is the one outside.

Shapes (tests/test_gpu_phi_layout.py CASES, same data, same B and seed: the oracle optima are shared with that file):
  n = 13  one panel, the last column block has one column (B rows clamped)
  n = 16  exactly one panel
  n = 17, n = 33  a last panel of one row: the block updates of the panels in front meet a tile whose only real row is
                  clamped in 15 of 16 lanes
  n = 61  four panels, all three Bk in three of them, a ragged last block
  n = 64  every lane a row, nothing ragged
  n = 13 with block output weights: H~ packed from global memory in front of the factorisation

Checks: (1) both periods of the phi-layout test: 1e-5 against the certified oracle optima, 1e-6 and equal statuses against
the runtime-dimension kernel; (2) n = 17 and n = 61: the iterate after exactly 1, 2 and 3 interior-point iterations
(mpcqp_set_iteration_limit + MPCQP_FLAG_KEEP_ITERATE) agrees with the runtime-dimension kernel's to 1e-8 -- the comparison
mpcqp_prepare makes before it accepts a specialisation: same algorithm on the same data, the kernels differ by rounding
(1e-13), while a wrong factor entry moves the first Newton step by its own size instead of hiding behind the convergence."""
import os
import shutil

import numpy as np
import pytest

import mpcqp
from tests import test_gpu_phi_layout as phi_layout
from tests.parity_util import rel_err
from tests.test_gpu_phi_layout import runtime_lib  # noqa: F401  (fixture: a private library instance without specialisations)

B = phi_layout.B
TOL = phi_layout.TOL                    # 1e-5: relative dU error against a certified oracle optimum
TOL_KERNELS = phi_layout.TOL_KERNELS    # 1e-6: relative dU difference between two kernels of the library
TOL_ITERATE = 1e-8                      # relative difference of the first iterates (mpcqp_prepare's bound)

SHAPES = ["n13_one_panel_ragged", "n16_one_panel_no_eps_load_H", "n17_second_panel_one_row", "n33_third_panel_one_row",
          "n61_four_panels", "n64_every_lane_a_row", "n13_block_weights_packed_H"]
ITERATE_SHAPES = ["n17_second_panel_one_row", "n61_four_panels"]
assert (TOL, TOL_KERNELS) == (1e-5, 1e-6) and B == 64 and set(SHAPES) <= set(phi_layout.CASES)


@pytest.fixture(scope="module")
def spec_lib(hiplib, tmp_path_factory):
    """A third instance of the library for the specialised runs.  An instance keeps the specialisations it has loaded, and
    an unprepared handle then runs on them: prepared on the session's own instance, these shapes would take the
    runtime-dimension kernel away from the files that run later and compare against it on that instance
    (tests/test_gpu_lane_handoff.py shares two shapes).  The copy sits in <tmp>/lib next to a link to the kernel sources,
    which the library looks for beside its own directory when it compiles a specialisation."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(hiplib._name)))
    root = tmp_path_factory.mktemp("speclib")
    (root / "lib").mkdir()
    os.symlink(os.path.join(pkg, "csrc"), str(root / "csrc"))
    path = shutil.copy(hiplib._name, str(root / "lib" / "libmpcqp_quarter.so"))
    keep = mpcqp.api._lib
    try:
        lib = mpcqp.api.load_library(path)
    finally:
        mpcqp.api._lib = keep
    return lib


@pytest.fixture
def product_cache(hiplib, monkeypatch):
    """The specialised runs of the private instance use the product's own cache directory."""
    monkeypatch.setenv("MPCQP_CACHE_DIR", os.path.join(os.path.dirname(os.path.abspath(hiplib._name)), "spec_cache"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_quarter_tile_update_against_oracle_and_runtime_kernel(hiplib, runtime_lib, spec_lib, product_cache, name, monkeypatch, tmp_path):  # noqa: F811
    hiplib = spec_lib
    ref = phi_layout.reference(name)
    cfg = ref["cfg"]
    nDU = cfg.nu * cfg.Hc
    nZ = nDU + (0 if np.isinf(cfg.Cwt) else 1)
    assert nZ == int(name[1:3]) and nZ <= 64
    with monkeypatch.context() as mp:             # (an empty cache: the unprepared handle stays on the runtime-dimension kernel)
        mp.setenv("MPCQP_CACHE_DIR", str(tmp_path))
        rtd = phi_layout.two_periods(ref, runtime_lib, False)
    spec = phi_layout.two_periods(ref, hiplib, True)
    for k in range(2):
        cert = ref["cert"][k]
        assert cert.mean() >= 0.8, (name, k, cert.mean())
        err = rel_err(spec[k]["Z"], ref["Z"][k], nDU)
        dif = rel_err(spec[k]["Z"], rtd[k]["Z"], nDU)
        print(f"[chol_quarter] {name} period {k}: certified {cert.mean():.3f}, worst rel dU error vs oracle (certified) "
              f"{err[cert].max():.3e}, worst rel dU difference vs runtime-dimension kernel {dif.max():.3e}, "
              f"factorisations {spec[k]['iters'].mean():.2f}")
        assert np.all(spec[k]["status"] == 0), (name, k, spec[k]["status"])
        assert err[cert].max() <= TOL, (name, k, int(np.argmax(np.where(cert, err, 0.0))), err[cert].max())
        assert np.array_equal(spec[k]["status"], rtd[k]["status"]), (name, k)
        assert dif.max() <= TOL_KERNELS, (name, k, int(np.argmax(dif)), dif.max())


def first_iterates(ref, lib, specialised):
    """The iterates after exactly 1, 2 and 3 interior-point iterations from a cold start, on the shape's specialisation or
    on the runtime-dimension kernel (handle as in phi_layout.two_periods)."""
    cfg, bt = ref["cfg"], ref["bt"]
    neps = 0 if np.isinf(cfg.Cwt) else 1
    hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, cfg.Hc, neps=neps,
                      flags=mpcqp.FLAG_RY_CONSTANT | mpcqp.FLAG_KEEP_QP | mpcqp.FLAG_COLD_START | mpcqp.FLAG_KEEP_ITERATE, lib=lib)
    hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
    hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt),
                   np.full(B, cfg.Cwt) if neps else None)
    full = lambda v, n: np.full((B, n), float(v)) if np.isfinite(v) else None
    hd.set_bounds(U0min=full(cfg.umin, hd.nU), U0max=full(cfg.umax, hd.nU), DUmin=full(cfg.dumin, hd.nDU),
                  DUmax=full(cfg.dumax, hd.nDU), Y0min=full(cfg.ymin, hd.nY), Y0max=full(cfg.ymax, hd.nY))
    if specialised:
        assert hd.prepare() == mpcqp.api.KERNEL_ONDEMAND
    out = []
    for k in (1, 2, 3):
        hd.set_iteration_limit(k)
        Z = np.zeros((B, hd.nZ))
        u0, st, it = hd.step(ref["x"][0], ref["lu"][0], bt["ry"], Z)
        out.append(dict(Z=Z, status=st.copy(), iters=it.copy()))
    assert hd.kernel_kind() == (mpcqp.api.KERNEL_ONDEMAND if specialised else mpcqp.api.KERNEL_GENERIC), hd.kernel_kind()
    hd.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITERATE_SHAPES)
def test_first_iterates_agree_with_runtime_kernel(hiplib, runtime_lib, spec_lib, product_cache, name, monkeypatch, tmp_path):  # noqa: F811
    hiplib = spec_lib
    ref = phi_layout.reference(name)
    with monkeypatch.context() as mp:
        mp.setenv("MPCQP_CACHE_DIR", str(tmp_path))
        rtd = first_iterates(ref, runtime_lib, False)
    spec = first_iterates(ref, hiplib, True)
    for k in range(3):
        zs, zr = spec[k]["Z"], rtd[k]["Z"]
        assert np.all(np.isfinite(zs)) and np.all(np.isfinite(zr)), (name, k + 1)
        dif = np.max(np.abs(zs - zr), axis=1) / np.maximum(1.0, np.max(np.abs(zr), axis=1))      # all of Z~, the slack included
        print(f"[chol_quarter] {name} iterate {k + 1}: worst rel difference vs runtime-dimension kernel {dif.max():.3e}, "
              f"factorisations {spec[k]['iters'].max()} / {rtd[k]['iters'].max()}")
        assert np.array_equal(spec[k]["status"], rtd[k]["status"]), (name, k + 1)
        assert dif.max() <= TOL_ITERATE, (name, k + 1, int(np.argmax(dif)), dif.max())
