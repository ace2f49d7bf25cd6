"""Host-side mirror of the reference's LinMPC interface over the C-ABI of include/mpcqp.h.

Two layers:

* `Handle` -- 1:1 ctypes binding of the C entry points (what a Julia `ccall` shim binds, see
  INTEGRATION.md).  Works with host (NumPy) pointers or raw device pointers.
* `BatchLinMPC` -- B logical `LinMPC` controllers of identical dimensions with the reference's
  vocabulary: constructor keywords of `LinMPC(estim; Hp, Hc, Mwt, Nwt, Lwt, Cwt)`
  (/root/reference/src/controller/linmpc.jl:288-316), `setconstraint!` keywords
  (src/controller/construct.jl:324-350), `moveinput!` arguments (src/controller/execute.jl:59-70),
  `getinfo` keys (src/controller/execute.jl:145-198), and the same error behaviour
  (DimensionMismatch -> ValueError, ArgumentError -> ValueError, status policy of
  src/controller/execute.jl:482-503).

There is no CPU fallback: the shared library is the HIP build and every compute call needs a GPU.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import types
import warnings

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "lib", "libmpcqp.so")

# flags / codes of include/mpcqp.h
FLAG_RY_CONSTANT, FLAG_COLD_START, FLAG_KEEP_QP, FLAG_WARM_DUAL, FLAG_NO_POLISH, FLAG_KEEP_ITERATE = 1, 2, 4, 8, 16, 32
KERNEL_GENERIC, KERNEL_AOT, KERNEL_ONDEMAND, KERNEL_SMALL, KERNEL_MS = 0, 1, 2, 3, 4
SINGLE_SHOOTING, MULTIPLE_SHOOTING = 0, 1
STATUS_OPTIMAL, STATUS_ITERATION_LIMIT, STATUS_ERROR = 0, 1, 2
GET_HESSIAN, GET_STEPRESP, GET_KMAT, GET_BVEC, GET_QTILDE, GET_FVEC, GET_AUDIT, GET_XHAT_MS, GET_MS_DEFECT = 1, 2, 3, 4, 5, 6, 7, 8, 9
GET_KF_COV, GET_KF_GAIN = 10, 11
GET_EXPLICIT_LAW = 12
GET_IM_XS, GET_IM_YS, GET_IM_YHATS = 13, 14, 15
GET_MODEL_AHAT, GET_MODEL_BU, GET_MODEL_C, GET_MODEL_BD, GET_MODEL_DD, GET_MODEL_DOP = 16, 17, 18, 19, 20, 21
GET_GDTAB, GET_XDTAB, GET_EXHAT, GET_KXHAT, GET_BXHAT = 22, 23, 24, 25, 26      # K1's remaining tables, device layouts
C2D_TUSTIN, C2D_ZOH = 0, 1                       # mpcqp_c2d_spec.d_method
C2D_OK, C2D_REFUSED = 0, 2                       # per-member status of mpcqp_c2d / mpcqp_set_model_continuous
IM_STATUS_OK, IM_STATUS_SINGULAR = 0, 2          # mpcqp_im_status
EXPLICIT_LAW = 1       # bit of mpcqp_explicit_prepare's with_law
SIM_FLAG_RY_PER_PERIOD, SIM_FLAG_NO_FUSE = 1, 2     # mpcqp_sim_io.flags
SIM_PATH_PERIOD, SIM_PATH_FUSED = 0, 1    # mpcqp_sim_path
KF_STATUS_OK, KF_STATUS_DROPPED = 0, 2
KF_STEADY_OK, KF_STEADY_NOT_CONVERGED, KF_STEADY_BROKE_DOWN = 0, 1, 2      # mpcqp_kf_status after mpcqp_kf_set_steady
EXPORTS = ("mpcqp_version", "mpcqp_strerror", "mpcqp_last_hip_error", "mpcqp_create",
           "mpcqp_destroy", "mpcqp_get_sizes", "mpcqp_set_model", "mpcqp_set_weights",
           "mpcqp_set_bounds", "mpcqp_step", "mpcqp_step_device", "mpcqp_loop_device", "mpcqp_recondense_device",
           "mpcqp_get", "mpcqp_last_step_ms", "mpcqp_last_condense_ms", "mpcqp_last_predmat_ms", "mpcqp_kf_set",
           "mpcqp_kf_correct", "mpcqp_kf_predict", "mpcqp_kf_correct_device", "mpcqp_kf_predict_device",
           "mpcqp_kf_set_covariances", "mpcqp_kf_set_state_covariance", "mpcqp_kf_status", "mpcqp_kf_lanes_per_estimator",
           "mpcqp_kf_set_direct", "mpcqp_kf_update", "mpcqp_kf_update_device",
           "mpcqp_kf_set_steady", "mpcqp_kf_solve_steady", "mpcqp_kf_solve_steady_device", "mpcqp_kf_steady_iters",
           "mpcqp_kf_steady_path",
           "mpcqp_kf_set_poles", "mpcqp_kf_place", "mpcqp_kf_place_device", "mpcqp_kf_set_place_cap", "mpcqp_kf_place_sweeps",
           "mpcqp_explicit_prepare", "mpcqp_explicit_status", "mpcqp_explicit_step", "mpcqp_explicit_step_device",
           "mpcqp_explicit_law", "mpcqp_explicit_law_device",
           "mpcqp_sim_set_plant", "mpcqp_sim", "mpcqp_sim_device", "mpcqp_sim_path",
           "mpcqp_set_model_continuous", "mpcqp_set_model_continuous_device",
           "mpcqp_im_set", "mpcqp_im_status", "mpcqp_im_correct", "mpcqp_im_correct_device", "mpcqp_im_update", "mpcqp_im_update_device",
           "mpcqp_set_output_weight_blocks", "mpcqp_set_dense_weights", "mpcqp_set_custom_constraints", "mpcqp_set_custom_bounds",
           "mpcqp_set_flags", "mpcqp_set_iteration_limit", "mpcqp_set_transcription", "mpcqp_transcription_supported", "mpcqp_set_current_setpoint", "mpcqp_prepare", "mpcqp_kernel_kind", "mpcqp_predmat_form", "mpcqp_lds_bytes", "mpcqp_row_groups", "mpcqp_step_consts_builds", "mpcqp_prebuild",
           "mpcqp_last_build_error", "mpcqp_multi_create", "mpcqp_multi_destroy", "mpcqp_multi_ndev",
           "mpcqp_multi_handle", "mpcqp_multi_shard", "mpcqp_multi_set_model", "mpcqp_multi_set_weights",
           "mpcqp_multi_set_bounds", "mpcqp_multi_prepare", "mpcqp_multi_step", "mpcqp_multi_gather_device",
           "mpcqp_multi_scatter_device")

_ct = C                     # (ctypes under a name that a parameter called C does not shadow)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class Dims(C.Structure):
    _fields_ = [("batch", C.c_int32), ("nxhat", C.c_int32), ("nu", C.c_int32), ("ny", C.c_int32),
                ("nd", C.c_int32), ("Hp", C.c_int32), ("Hc", C.c_int32), ("nb", _ip),
                ("neps", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32),
                ("max_iter", C.c_int32), ("gap_tol", C.c_double), ("res_tol", C.c_double),
                ("dual_reg", C.c_double)]


class Sizes(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("nZ", "nDU", "nU", "nY", "nD")]


BOUND_FIELDS = ("U0min", "U0max", "DUmin", "DUmax", "Y0min", "Y0max", "x0min", "x0max",
                "C_umin", "C_umax", "C_dumin", "C_dumax", "C_ymin", "C_ymax", "c_x0min", "c_x0max")


class Bounds(C.Structure):
    _fields_ = [(k, _dp) for k in BOUND_FIELDS]


class C2dSpec(C.Structure):
    """mpcqp_c2d_spec of include/mpcqp.h"""
    _fields_ = [(k, C.c_int32) for k in ("batch", "nx", "nu", "ny", "nd", "nym", "d_method")] + [(k, _ip) for k in ("nint_u", "nint_ym", "i_ym")]


class C2dIn(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("A", "Bu", "C", "Bd", "Dd", "Ts", "dop")]


class C2dOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("Ahat", "Bu", "C", "Bd", "Dd", "dop")]


SIM_IO_IN = ("ry", "Ru", "d", "u_step", "y_step", "d_step", "sigma_u", "sigma_y", "sigma_d", "sigma_x", "w_u", "w_y", "w_d", "w_x")
SIM_IO_STATE = ("x0", "xhat0", "lastu0", "Ztilde")
SIM_IO_RECORDS = ("Y", "X", "D", "Xhat", "Yhat", "U", "Ud")


class SimIO(C.Structure):
    """mpcqp_sim_io of include/mpcqp.h"""
    _fields_ = ([("N", C.c_int32), ("flags", C.c_uint32)] + [(k, C.c_void_p) for k in SIM_IO_IN + SIM_IO_STATE + SIM_IO_RECORDS]
                + [("status", C.c_void_p)])


class MpcqpError(RuntimeError):
    pass


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own libamdhip64.so.7 /
    libhsa-runtime64.so.1 (same SONAMEs as /opt/rocm/lib, RPATH $ORIGIN); the dynamic loader keeps
    whichever copy is mapped first.  If this library pulls in /opt/rocm's copy first, a later
    `import torch` binds to it and reports "No HIP GPUs are available" (torch 2.10+rocm7.0 against
    the 7.2 runtime).  When torch is installed but not imported yet, map its copy first so that both
    orders of import give the same process image as `import torch; import mpcqp`.
    MPCQP_SYSTEM_HIP=1 keeps the system runtime (a process that never imports torch)."""
    import sys
    if "torch" in sys.modules or os.environ.get("MPCQP_SYSTEM_HIP") == "1":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(rt):
        C.CDLL(rt, mode=C.RTLD_GLOBAL)


def _check_hip_runtime(lib):
    """The library is built against the system ROCm; the process may run on another HIP runtime (the PyTorch wheel's copy,
    see _share_hip_runtime_with_torch).  A different MAJOR version is worth a warning."""
    import re
    import warnings
    m = re.search(r"HIP (\d+)\.(\d+)", lib.mpcqp_version().decode())
    try:
        rt = C.CDLL("libamdhip64.so")              # (already mapped: resolves to the copy this process uses)
        v = C.c_int(0)
        if not m or int(m.group(1)) == 0 or rt.hipRuntimeGetVersion(C.byref(v)) != 0:       # (0.0: the CPU emulator build)
            return
    except (OSError, AttributeError):
        return
    if v.value // 10000000 != int(m.group(1)):
        warnings.warn(f"mpcqp: built against HIP {m.group(1)}.{m.group(2)}, running on HIP runtime {v.value // 10000000}."
                      f"{v.value // 100000 % 100} (MPCQP_SYSTEM_HIP=1 keeps the system runtime in processes that never import torch)",
                      RuntimeWarning, stacklevel=3)


def load_library(path: str | None = None):
    """Load (once) the HIP shared library.  `path` is for tests only; the environment variable MPCQP_LIB names another build
    of the same library (developer A/B runs of bench.py, scripts/build_variant.sh)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("MPCQP_LIB") or DEFAULT_LIB
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: the HIP extension is not built (run `python -c 'import "
            f"__graft_entry__ as g; g.build()'` or `make -C modelpredictivecontrol.jl_amd/csrc`). "
            "There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(path)
    lib.mpcqp_version.restype = C.c_char_p
    _check_hip_runtime(lib)
    lib.mpcqp_strerror.restype = C.c_char_p
    lib.mpcqp_strerror.argtypes = [C.c_int]
    lib.mpcqp_last_hip_error.restype = C.c_char_p
    lib.mpcqp_create.argtypes = [C.POINTER(Dims), C.POINTER(C.c_void_p)]
    lib.mpcqp_destroy.argtypes = [C.c_void_p]
    lib.mpcqp_get_sizes.argtypes = [C.c_void_p, C.POINTER(Sizes)]
    lib.mpcqp_set_model.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    lib.mpcqp_set_weights.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    lib.mpcqp_set_bounds.argtypes = [C.c_void_p, C.POINTER(Bounds)]
    lib.mpcqp_set_output_weight_blocks.argtypes = [C.c_void_p, C.c_void_p]
    lib.mpcqp_set_dense_weights.argtypes = [C.c_void_p] * 4
    lib.mpcqp_set_flags.argtypes = [C.c_void_p, C.c_uint32]
    lib.mpcqp_set_iteration_limit.argtypes = [C.c_void_p, C.c_int32]
    lib.mpcqp_set_transcription.argtypes = [C.c_void_p, C.c_int32]
    lib.mpcqp_transcription_supported.argtypes = [C.c_void_p]
    lib.mpcqp_set_custom_constraints.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    lib.mpcqp_set_custom_bounds.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    lib.mpcqp_step.argtypes = [C.c_void_p] + [C.c_void_p] * 11
    lib.mpcqp_step_device.argtypes = [C.c_void_p] + [C.c_void_p] * 12
    lib.mpcqp_loop_device.argtypes = [C.c_void_p] + [C.c_void_p] * 13
    lib.mpcqp_recondense_device.argtypes = [C.c_void_p, C.c_void_p]
    lib.mpcqp_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.mpcqp_last_step_ms.restype = C.c_double
    lib.mpcqp_last_step_ms.argtypes = [C.c_void_p]
    lib.mpcqp_last_condense_ms.restype = C.c_double
    lib.mpcqp_last_condense_ms.argtypes = [C.c_void_p]
    lib.mpcqp_last_predmat_ms.restype = C.c_double
    lib.mpcqp_last_predmat_ms.argtypes = [C.c_void_p]
    lib.mpcqp_kf_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.mpcqp_kf_correct.argtypes = [C.c_void_p] * 4
    lib.mpcqp_kf_predict.argtypes = [C.c_void_p] * 4
    lib.mpcqp_kf_correct_device.argtypes = [C.c_void_p] * 5
    lib.mpcqp_kf_predict_device.argtypes = [C.c_void_p] * 5
    lib.mpcqp_kf_set_covariances.argtypes = [C.c_void_p] * 5 + [C.c_int32]
    lib.mpcqp_kf_set_state_covariance.argtypes = [C.c_void_p, C.c_void_p]
    lib.mpcqp_kf_status.argtypes = [C.c_void_p, C.c_void_p]
    lib.mpcqp_kf_lanes_per_estimator.argtypes = [C.c_void_p]
    lib.mpcqp_kf_set_direct.argtypes = [C.c_void_p, C.c_int32]
    lib.mpcqp_kf_update.argtypes = [C.c_void_p] * 5
    lib.mpcqp_kf_update_device.argtypes = [C.c_void_p] * 6
    if hasattr(lib, "mpcqp_kf_set_steady"):        # (an older build of the library: Handle then has no kf_*_steady methods)
        lib.mpcqp_kf_set_steady.argtypes = [C.c_void_p] * 4 + [C.c_int32]
        lib.mpcqp_kf_solve_steady.argtypes = [C.c_void_p]
        lib.mpcqp_kf_solve_steady_device.argtypes = [C.c_void_p, C.c_void_p]
        lib.mpcqp_kf_steady_iters.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "mpcqp_kf_steady_path"):       # (a build without the square-root pass: Handle then has no kf_steady_path)
        lib.mpcqp_kf_steady_path.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "mpcqp_kf_set_poles"):         # (an older build of the library: Handle then has no kf_set_poles ... methods)
        lib.mpcqp_kf_set_poles.argtypes = [C.c_void_p] * 3 + [C.c_int32]
        lib.mpcqp_kf_place.argtypes = [C.c_void_p]
        lib.mpcqp_kf_place_device.argtypes = [C.c_void_p, C.c_void_p]
        lib.mpcqp_kf_set_place_cap.argtypes = [C.c_void_p, C.c_int32]
        lib.mpcqp_kf_place_sweeps.argtypes = [C.c_void_p, C.c_void_p]
    lib.mpcqp_set_current_setpoint.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "mpcqp_explicit_prepare"):
        lib.mpcqp_explicit_prepare.argtypes = [C.c_void_p, C.c_int32]
        lib.mpcqp_explicit_status.argtypes = [C.c_void_p, C.c_void_p]
        lib.mpcqp_explicit_step.argtypes = [C.c_void_p] * 11
        lib.mpcqp_explicit_step_device.argtypes = [C.c_void_p] * 12
        lib.mpcqp_explicit_law.argtypes = [C.c_void_p] * 8
        lib.mpcqp_explicit_law_device.argtypes = [C.c_void_p] * 9
    if hasattr(lib, "mpcqp_sim"):
        lib.mpcqp_sim_set_plant.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        lib.mpcqp_sim.argtypes = [C.c_void_p, C.POINTER(SimIO)]
        lib.mpcqp_sim_device.argtypes = [C.c_void_p, C.POINTER(SimIO), C.c_void_p]
        lib.mpcqp_sim_path.argtypes = [C.c_void_p]
    if hasattr(lib, "mpcqp_mhe_attach"):           # (include/mpcqp_mhe.h: the entry points that take a controller handle)
        lib.mpcqp_mhe_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        lib.mpcqp_sim_est_status.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.mpcqp_est_initstate.argtypes = [C.c_void_p] * 6
        lib.mpcqp_est_initstate_device.argtypes = [C.c_void_p] * 7
    if hasattr(lib, "mpcqp_im_set"):               # (InternalModel)
        lib.mpcqp_im_set.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32]
        lib.mpcqp_im_status.argtypes = [C.c_void_p, C.c_void_p]
        lib.mpcqp_im_correct.argtypes = [C.c_void_p] * 4
        lib.mpcqp_im_correct_device.argtypes = [C.c_void_p] * 5
        lib.mpcqp_im_update.argtypes = [C.c_void_p] * 4
        lib.mpcqp_im_update_device.argtypes = [C.c_void_p] * 5
    if hasattr(lib, "mpcqp_c2d"):                  # (LinModel(sys, Ts) + augment_model on the device)
        lib.mpcqp_c2d_sizes.argtypes = [C.POINTER(C2dSpec), _ip, _ip]
        lib.mpcqp_c2d.argtypes = [C.POINTER(C2dSpec), C.POINTER(C2dIn), C.POINTER(C2dOut), C.c_void_p]
        lib.mpcqp_c2d_device.argtypes = [C.POINTER(C2dSpec), C.POINTER(C2dIn), C.POINTER(C2dOut), C.c_void_p, C.c_void_p]
        lib.mpcqp_set_model_continuous.argtypes = [C.c_void_p, C.POINTER(C2dSpec), C.POINTER(C2dIn), C.c_void_p]
        lib.mpcqp_set_model_continuous_device.argtypes = [C.c_void_p, C.POINTER(C2dSpec), C.POINTER(C2dIn), C.c_void_p, C.c_void_p]
    lib.mpcqp_prepare.argtypes = [C.c_void_p]
    lib.mpcqp_kernel_kind.argtypes = [C.c_void_p]
    lib.mpcqp_predmat_form.argtypes = [C.c_void_p]
    lib.mpcqp_lds_bytes.argtypes = [C.c_void_p]
    lib.mpcqp_step_consts_builds.argtypes = [C.c_void_p]
    lib.mpcqp_row_groups.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.mpcqp_prebuild.argtypes = [C.POINTER(Dims), C.c_uint32]
    lib.mpcqp_last_build_error.restype = C.c_char_p
    lib.mpcqp_multi_create.argtypes = [C.POINTER(Dims), _ip, C.c_int32, C.POINTER(C.c_void_p)]
    lib.mpcqp_multi_destroy.argtypes = [C.c_void_p]
    lib.mpcqp_multi_ndev.argtypes = [C.c_void_p]
    lib.mpcqp_multi_handle.restype = C.c_void_p
    lib.mpcqp_multi_handle.argtypes = [C.c_void_p, C.c_int32]
    lib.mpcqp_multi_shard.argtypes = [C.c_void_p, C.c_int32, _ip, _ip]
    lib.mpcqp_multi_set_model.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    lib.mpcqp_multi_set_weights.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    lib.mpcqp_multi_set_bounds.argtypes = [C.c_void_p, C.POINTER(Bounds)]
    lib.mpcqp_multi_prepare.argtypes = [C.c_void_p]
    lib.mpcqp_multi_step.argtypes = [C.c_void_p] + [C.c_void_p] * 11
    lib.mpcqp_multi_gather_device.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
    lib.mpcqp_multi_scatter_device.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 4
    _lib = lib
    return lib


def _chk(lib, rc):
    if rc != 0:
        msg = lib.mpcqp_strerror(rc).decode()
        if rc == -6:
            msg += ": " + lib.mpcqp_last_hip_error().decode()
        raise MpcqpError(f"mpcqp error {rc}: {msg}")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def colmajor(M):
    """(B, rows, cols) logical -> the ABI's column-major-per-problem buffer (= Julia (rows,cols,B))."""
    return _f64(np.asarray(M, float).transpose(0, 2, 1))


# -- LinModel(sys, Ts) + augment_model for a batch of continuous-time models (csrc/c2d_bodies.h)
class C2dOptions:
    """Dimensions and options of a discretisation, validated the way the reference validates them (init_integrators,
    validate_ym: ValueError), and the mpcqp_c2d_spec that carries them.  `nint_u` / `nint_ym`: 0 (no integrator) or one count
    per input / measured output; `nint_ym=None`: one per measured output, none when any nint_u != 0 (nothing is pruned: the
    reference's default_nint checks observability per model, which cannot vary inside a batch of one shape)."""

    def __init__(self, B, nx, nu, ny, nd, nint_u=0, nint_ym=0, i_ym=None, d_method="tustin"):
        self.B, self.nx, self.nu, self.ny, self.nd = int(B), int(nx), int(nu), int(ny), int(nd)
        iy = np.arange(ny) if i_ym is None else np.asarray(i_ym, int).reshape(-1)
        if iy.size and (len(set(iy.tolist())) != iy.size or iy.min() < 0 or iy.max() >= ny):
            raise ValueError("Measured output indices i_ym should contains valid and unique indices")
        def counts(v, n, name):
            a = np.zeros(n, int) if np.isscalar(v) and v == 0 else np.full(n, int(v)) if np.isscalar(v) else np.asarray(v, int).reshape(-1)
            if a.size != n:
                raise ValueError(f"nint_{name} length ({a.size}) ≠ n{name} ({n})")
            if np.any(a < 0):
                raise ValueError(f"nint_{name} values should be ≥ 0")
            return a
        self.nint_u = counts(nint_u, nu, "u")
        if nint_ym is None:
            nint_ym = 0 if self.nint_u.any() else 1
        self.nint_ym = counts(nint_ym, iy.size, "ym")
        if d_method not in ("tustin", "zoh"):
            raise ValueError("d_method should be \"tustin\" or \"zoh\"")
        self.d_method, self.i_ym = d_method, iy
        self.tustin = nd > 0 and d_method == "tustin"
        self.nxd = 2 * nx if self.tustin else nx
        self.nxh = self.nxd + int(self.nint_u.sum()) + int(self.nint_ym.sum())
        self._keep = [np.ascontiguousarray(a, np.int32) for a in (self.nint_u, self.nint_ym, iy)]
        k = self._keep
        self.spec = C2dSpec(batch=B, nx=nx, nu=nu, ny=ny, nd=nd, nym=iy.size, d_method=C2D_ZOH if d_method == "zoh" else C2D_TUSTIN,
                            nint_u=k[0].ctypes.data_as(_ip), nint_ym=k[1].ctypes.data_as(_ip) if iy.size else None,
                            i_ym=k[2].ctypes.data_as(_ip) if iy.size else None)


def _c2d_inputs(A, Bu, Cm, Ts, Bd, Dd):
    """(B,·,·) logical arrays -> ABI buffers; Ts scalar or (B,)."""
    A, Bu, Cm, Bd, Dd = _c2d_batch(A, Bu, Cm, Bd, Dd)
    B, nx, nu = Bu.shape
    ny = Cm.shape[1]
    if A.shape != (B, nx, nx) or Cm.shape != (B, ny, nx):
        raise ValueError("DimensionMismatch between A, Bu, C")
    nd = 0 if Bd is None else np.asarray(Bd).shape[2]
    if nd > 0:
        Bd = np.asarray(Bd, float)
        Dd = np.zeros((B, ny, nd)) if Dd is None else np.asarray(Dd, float)
        if Bd.shape != (B, nx, nd) or Dd.shape != (B, ny, nd):
            raise ValueError("DimensionMismatch between A, Bd, Dd")
    ts = np.broadcast_to(np.asarray(Ts, float), (B,)).copy()
    bufs = [colmajor(A), colmajor(Bu), colmajor(Cm), colmajor(Bd) if nd > 0 else None, colmajor(Dd) if nd > 0 else None, ts]
    return (B, nx, nu, ny, nd), bufs


def _c2d_batch(*mats):
    """A single model given without the batch axis (scalars included) gets one."""
    def one(M):
        if M is None:
            return None
        M = np.asarray(M, float)
        return M if M.ndim == 3 else np.atleast_2d(M)[None]
    return tuple(one(M) for M in mats)


def c2d(A, Bu, C, Ts, Bd=None, Dd=None, *, nint_u=0, nint_ym=0, i_ym=None, d_method="tustin", dop=None, out=None, lib=None):
    """`LinModel(sys, Ts)` + `augment_model` for a batch of continuous-time models (include/mpcqp.h: mpcqp_c2d): zero-order hold
    for the manipulated inputs, Tustin (or, with d_method="zoh", zero-order hold) for the measured disturbances, the integrators
    of nint_u / nint_ym appended.  A (B,nx,nx), Bu (B,nx,nu), C (B,ny,nx), Bd (B,nx,nd), Dd (B,ny,nd), Ts scalar or (B,).
    Returns (Ahat, Bhu, Chat, Bhd, Dhd, status) with a leading batch axis (Bhd, Dhd None when nd = 0), and the padded dop
    behind them when `dop` (B,nx_dis) is given.  A member with status 2 was refused: its slices hold zeros, or what `out` (a
    tuple of arrays of the result's shapes, e.g. the model in use) held."""
    lib = lib or load_library()
    if not hasattr(lib, "mpcqp_c2d"):
        raise NotImplementedError("this library has no mpcqp_c2d")
    (B, nx, nu, ny, nd), bufs = _c2d_inputs(A, Bu, C, Ts, Bd, Dd)
    o = C2dOptions(B, nx, nu, ny, nd, nint_u, nint_ym, i_ym, d_method)
    nxh = o.nxh
    shapes = [(B, nxh, nxh), (B, nu, nxh), (B, nxh, ny), (B, nd, nxh), (B, nd, ny)]       # (ABI: column-major per member)
    res = [np.zeros(sh) for sh in shapes]
    if out is not None:
        for r_, src in zip(res, out):
            if src is not None and r_.size:
                r_[...] = np.asarray(src, float).transpose(0, 2, 1)
    dopv = None if dop is None else _f64(np.broadcast_to(np.asarray(dop, float), (B, o.nxd)))
    doph = None if dop is None else np.zeros((B, nxh))
    status = np.zeros(B, np.int32)
    cin = C2dIn(*[_ptr(b) for b in bufs], _ptr(dopv))
    cout = C2dOut(_ptr(res[0]), _ptr(res[1]), _ptr(res[2]), _ptr(res[3]) if nd else None, _ptr(res[4]) if nd else None, _ptr(doph))
    _chk(lib, lib.mpcqp_c2d(_ct.byref(o.spec), _ct.byref(cin), _ct.byref(cout), _ptr(status)))
    mats = [np.ascontiguousarray(r_.transpose(0, 2, 1)) for r_ in res]
    ret = (mats[0], mats[1], mats[2], mats[3] if nd else None, mats[4] if nd else None, status)
    return ret if dop is None else ret + (doph,)


def c2d_device(opts, A, Bu, C, Ts, Ahat, Bhu, Chat, status, Bd=0, Dd=0, dop=0, Bhd=0, Dhd=0, dophat=0, stream=0, lib=None):
    """mpcqp_c2d_device: `opts` a C2dOptions, everything else raw device addresses in ABI layout; enqueued on `stream`."""
    lib = lib or load_library()
    v = lambda p: _ct.c_void_p(int(p)) if p else None
    cin = C2dIn(*[v(p) for p in (A, Bu, C, Bd, Dd, Ts, dop)])
    cout = C2dOut(*[v(p) for p in (Ahat, Bhu, Chat, Bhd, Dhd, dophat)])
    _chk(lib, lib.mpcqp_c2d_device(_ct.byref(opts.spec), _ct.byref(cin), _ct.byref(cout), v(status), v(stream)))


# -- SteadyKalmanFilter from Q̂ and R̂: the gain solved for on the device (csrc/kf_dare_bodies.h).  Methods of Handle, bound
# only when the library exports the entry points
def _kf_set_steady(self, Qhat, Rhat, i_ym):
    """Qhat (B,nx̂,nx̂) symmetric positive semidefinite, Rhat (B,nym,nym) symmetric positive definite.  Solves the Riccati equation of every member on the
    resident model; kf_gain() / kf_covariance() / kf_status() / kf_steady_iters() read the result back."""
    iy = np.ascontiguousarray(i_ym, dtype=np.int32)
    _chk(self.lib, self.lib.mpcqp_kf_set_steady(self.h, _ptr(colmajor(Qhat)), _ptr(colmajor(Rhat)), _ptr(iy), int(iy.size)))
    self.nym = int(iy.size)


def _kf_solve_steady(self):
    """Solve again on the model that is resident now (after set_model); host-synchronous."""
    _chk(self.lib, self.lib.mpcqp_kf_solve_steady(self.h))


def _kf_solve_steady_device(self, stream=0):
    _chk(self.lib, self.lib.mpcqp_kf_solve_steady_device(self.h, C.c_void_p(stream)))


def _kf_steady_iters(self):
    """(B,) int32 doubling iterations of the last solve."""
    out = np.empty(self.B, np.int32)
    _chk(self.lib, self.lib.mpcqp_kf_steady_iters(self.h, _ptr(out)))
    return out


def _kf_steady_path(self):
    """(B,) int32: 0 the estimator was solved by (or left with) the definite form of the iteration, 1 the square-root form ran
    for it (a semidefinite Q̂)."""
    out = np.empty(self.B, np.int32)
    _chk(self.lib, self.lib.mpcqp_kf_steady_path(self.h, _ptr(out)))
    return out


_STEADY_METHODS = {f.__name__[1:]: f for f in (_kf_set_steady, _kf_solve_steady, _kf_solve_steady_device, _kf_steady_iters)}


# -- Luenberger observer from its poles: the gain placed on the device (csrc/kf_place_bodies.h).  Methods of Handle, bound only
# when the library exports the entry points
def _kf_set_poles(self, poles, i_ym):
    """poles (B,nx̂) real, inside the unit circle.  Places them on the resident model: the eigenvalues of Â (I - K̂ Ĉm);
    kf_gain() / kf_status() / kf_place_sweeps() read the result back."""
    iy = np.ascontiguousarray(i_ym, dtype=np.int32)
    _chk(self.lib, self.lib.mpcqp_kf_set_poles(self.h, _ptr(_f64(poles)), _ptr(iy), int(iy.size)))
    self.nym = int(iy.size)


def _kf_place(self):
    """Place again on the model that is resident now (after set_model); host-synchronous."""
    _chk(self.lib, self.lib.mpcqp_kf_place(self.h))


def _kf_place_device(self, stream=0):
    _chk(self.lib, self.lib.mpcqp_kf_place_device(self.h, C.c_void_p(stream)))


def _kf_set_place_cap(self, cap):
    """Most sweeps of the placements that follow, 0 .. 100 (default 30)."""
    _chk(self.lib, self.lib.mpcqp_kf_set_place_cap(self.h, int(cap)))


def _kf_place_sweeps(self):
    """(B,) int32 sweeps of the last placement."""
    out = np.empty(self.B, np.int32)
    _chk(self.lib, self.lib.mpcqp_kf_place_sweeps(self.h, _ptr(out)))
    return out


_PLACE_METHODS = {f.__name__[1:]: f for f in (_kf_set_poles, _kf_place, _kf_place_device, _kf_set_place_cap, _kf_place_sweeps)}


class Handle:
    """Thin binding of the C-ABI; array arguments are already in ABI layout."""

    def __init__(self, B, nxhat, nu, ny, nd, Hp, Hc, nb=None, neps=1, device=0, flags=0,
                 max_iter=0, gap_tol=0.0, res_tol=0.0, dual_reg=0.0, lib=None):
        self.lib = lib or load_library()
        self._nb = None
        d = Dims(batch=B, nxhat=nxhat, nu=nu, ny=ny, nd=nd, Hp=Hp, Hc=Hc, neps=neps, device=device,
                 flags=flags, max_iter=max_iter, gap_tol=gap_tol, res_tol=res_tol, dual_reg=dual_reg)
        if nb is not None:
            self._nb = (C.c_int32 * len(nb))(*[int(v) for v in nb])
            d.nb = C.cast(self._nb, _ip)
        self.h = C.c_void_p()
        _chk(self.lib, self.lib.mpcqp_create(C.byref(d), C.byref(self.h)))
        s = Sizes()
        _chk(self.lib, self.lib.mpcqp_get_sizes(self.h, C.byref(s)))
        self.B, self.nxhat, self.nu, self.ny, self.nd, self.Hp, self.Hc = B, nxhat, nu, ny, nd, Hp, Hc
        self.nZ, self.nDU, self.nU, self.nY, self.nD = s.nZ, s.nDU, s.nU, s.nY, s.nD
        self.flags = flags
        self._keep = []

    def __getattr__(self, name):
        # kf_set_steady, kf_solve_steady, kf_solve_steady_device, kf_steady_iters: there only when the library exports them
        f = _STEADY_METHODS.get(name)
        if f is not None and hasattr(self.__dict__.get("lib"), "mpcqp_kf_set_steady"):
            return types.MethodType(f, self)
        if name == "kf_steady_path" and hasattr(self.__dict__.get("lib"), "mpcqp_kf_steady_path"):
            return types.MethodType(_kf_steady_path, self)
        f = _PLACE_METHODS.get(name)
        if f is not None and hasattr(self.__dict__.get("lib"), "mpcqp_kf_set_poles"):
            return types.MethodType(f, self)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.mpcqp_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_model(self, Ahat, Bu, Cm, Bd=None, Dd=None, dop=None):
        args = [None if a is None else _f64(a) for a in (Ahat, Bu, Cm, Bd, Dd, dop)]
        _chk(self.lib, self.lib.mpcqp_set_model(self.h, *[_ptr(a) for a in args]))

    def set_model_continuous(self, opts, A, Bu, Cm, Ts, Bd=None, Dd=None, dop=None):
        """mpcqp_set_model_continuous: `opts` a C2dOptions, the arrays in ABI layout (host).  Returns status (B,) int32."""
        if not hasattr(self.lib, "mpcqp_set_model_continuous"):
            raise NotImplementedError("this library has no mpcqp_set_model_continuous")
        args = [None if a is None else _f64(a) for a in (A, Bu, Cm, Bd, Dd, Ts, dop)]
        cin = C2dIn(*[_ptr(a) for a in args])
        st = np.zeros(self.B, np.int32)
        _chk(self.lib, self.lib.mpcqp_set_model_continuous(self.h, C.byref(opts.spec), C.byref(cin), _ptr(st)))
        return st

    def set_model_continuous_device(self, opts, A, Bu, Cm, Ts, status, Bd=0, Dd=0, dop=0, stream=0):
        """mpcqp_set_model_continuous_device: raw device addresses; the launch, K1, K2 and the refreshes are enqueued on `stream`."""
        if not hasattr(self.lib, "mpcqp_set_model_continuous_device"):
            raise NotImplementedError("this library has no mpcqp_set_model_continuous_device")
        v = lambda p: C.c_void_p(int(p)) if p else None
        cin = C2dIn(*[v(p) for p in (A, Bu, Cm, Bd, Dd, Ts, dop)])
        _chk(self.lib, self.lib.mpcqp_set_model_continuous_device(self.h, C.byref(opts.spec), C.byref(cin), v(status), v(stream)))

    def get_model(self):
        """The resident model read back: (Ahat, Bhu, Chat, Bhd, Dhd, dop) with a leading batch axis (Bhd, Dhd None when nd = 0)."""
        shapes = {GET_MODEL_AHAT: (self.nxhat, self.nxhat), GET_MODEL_BU: (self.nu, self.nxhat), GET_MODEL_C: (self.nxhat, self.ny),
                  GET_MODEL_BD: (self.nd, self.nxhat), GET_MODEL_DD: (self.nd, self.ny)}
        res = []
        for which, sh in shapes.items():
            if self.nd == 0 and which in (GET_MODEL_BD, GET_MODEL_DD):
                res.append(None)
                continue
            out = np.empty((self.B,) + sh)
            _chk(self.lib, self.lib.mpcqp_get(self.h, which, _ptr(out)))
            res.append(np.ascontiguousarray(out.transpose(0, 2, 1)))
        dop = np.empty((self.B, self.nxhat))
        _chk(self.lib, self.lib.mpcqp_get(self.h, GET_MODEL_DOP, _ptr(dop)))
        return tuple(res) + (dop,)

    def set_weights(self, Mdiag, Ndiag, Ldiag, Cwt=None):
        args = [None if a is None else _f64(a) for a in (Mdiag, Ndiag, Ldiag, Cwt)]
        _chk(self.lib, self.lib.mpcqp_set_weights(self.h, *[_ptr(a) for a in args]))

    def set_output_weight_blocks(self, Mblk):
        """Mblk (B, Hp, ny, ny), symmetric blocks, or None (back to the diagonal weight)."""
        a = None if Mblk is None else _f64(np.asarray(Mblk, float).transpose(0, 1, 3, 2))
        _chk(self.lib, self.lib.mpcqp_set_output_weight_blocks(self.h, _ptr(a)))

    def set_dense_weights(self, M_Hp=None, N_Hc=None, L_Hp=None):
        """Dense symmetric weights (B, n, n) or None; they replace the diagonals of set_weights."""
        arrs = [None if a is None else colmajor(a) for a in (M_Hp, N_Hc, L_Hp)]
        _chk(self.lib, self.lib.mpcqp_set_dense_weights(self.h, *[_ptr(a) for a in arrs]))

    def set_flags(self, flags):
        _chk(self.lib, self.lib.mpcqp_set_flags(self.h, int(flags)))
        self.flags = int(flags)

    def set_transcription(self, transcription):
        """MPCQP_SINGLE_SHOOTING / MPCQP_MULTIPLE_SHOOTING (the stage-structured kernel, csrc/ms_bodies.h)."""
        _chk(self.lib, self.lib.mpcqp_set_transcription(self.h, int(transcription)))

    def transcription_supported(self):
        """0 when the handle's transcription can run; else the reason mask of include/mpcqp.h."""
        return self.lib.mpcqp_transcription_supported(self.h)

    def set_iteration_limit(self, max_iter):
        _chk(self.lib, self.lib.mpcqp_set_iteration_limit(self.h, int(max_iter)))

    def set_current_setpoint(self, ry_now):
        a = None if ry_now is None else _f64(ry_now)
        _chk(self.lib, self.lib.mpcqp_set_current_setpoint(self.h, _ptr(a)))

    def prepare(self):
        """Build/load the specialised step kernel of the current shape and constraint pattern
        (mpcqp_prepare); returns KERNEL_GENERIC / KERNEL_AOT / KERNEL_ONDEMAND.  Steps never compile."""
        k = self.lib.mpcqp_prepare(self.h)
        if k < 0:
            _chk(self.lib, k)
        if k == KERNEL_GENERIC:
            msg = self.lib.mpcqp_last_build_error().decode()
            if msg:
                warnings.warn(f"mpcqp: specialised kernel not available, using the runtime-dimension "
                              f"kernel ({msg})", RuntimeWarning)
        return k

    def lds_bytes(self):
        return self.lib.mpcqp_lds_bytes(self.h)

    def kernel_kind(self):
        return self.lib.mpcqp_kernel_kind(self.h)

    def predmat_form(self):
        """Which form of K1 builds this handle's prediction tables in this process: 0 the LDS loops, 1 the matrix cores."""
        return self.lib.mpcqp_predmat_form(self.h)

    def step_consts_builds(self):
        """How often the handle has built its block of step constants (0: the steps form the values themselves)."""
        return self.lib.mpcqp_step_consts_builds(self.h)

    def row_groups(self):
        g = C.c_uint32()
        _chk(self.lib, self.lib.mpcqp_row_groups(self.h, C.byref(g)))
        return int(g.value)

    def set_custom_constraints(self, nw, Wy=None, Wu=None, Wd=None, Wr=None, w_op=None):
        args = [None if a is None else _f64(a) for a in (Wy, Wu, Wd, Wr, w_op)]
        _chk(self.lib, self.lib.mpcqp_set_custom_constraints(self.h, int(nw), *[_ptr(a) for a in args]))

    def set_custom_bounds(self, Wmin=None, Wmax=None, C_wmin=None, C_wmax=None):
        args = [None if a is None else _f64(a) for a in (Wmin, Wmax, C_wmin, C_wmax)]
        _chk(self.lib, self.lib.mpcqp_set_custom_bounds(self.h, *[_ptr(a) for a in args]))

    def set_bounds(self, **kw):
        b = Bounds()
        keep = []
        for k in BOUND_FIELDS:
            v = kw.get(k)
            if v is not None:
                a = _f64(v)
                keep.append(a)
                setattr(b, k, a.ctypes.data_as(_dp))
        _chk(self.lib, self.lib.mpcqp_set_bounds(self.h, C.byref(b)))

    def step(self, xhat0, lastu0, Ry, Z, Ru=None, d0=None, Dhat0=None, want_Yhat=False):
        """Host-pointer step.  Z (B,nZ) is updated in place.  Returns u0, status, iters[, Yhat0]."""
        B = self.B
        x, lu, ry = _f64(xhat0), _f64(lastu0), _f64(Ry)
        ru = None if Ru is None else _f64(Ru)
        dd0 = None if d0 is None else _f64(d0)
        dh = None if Dhat0 is None else _f64(Dhat0)
        nry = self.ny if (self.flags & FLAG_RY_CONSTANT) else self.nY
        if x.size != B * self.nxhat or lu.size != B * self.nu or ry.size != B * nry or Z.size != B * self.nZ:
            raise ValueError("DimensionMismatch in step arguments")
        assert Z.dtype == np.float64 and Z.flags.c_contiguous
        u0 = np.empty((B, self.nu))
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        yh = np.empty((B, self.nY)) if want_Yhat else None
        _chk(self.lib, self.lib.mpcqp_step(self.h, _ptr(x), _ptr(lu), _ptr(ry), _ptr(ru), _ptr(dd0),
                                           _ptr(dh), _ptr(Z), _ptr(u0), _ptr(status), _ptr(iters),
                                           _ptr(yh)))
        return (u0, status, iters, yh) if want_Yhat else (u0, status, iters)

    def step_device(self, xhat0, lastu0, Ry, Z, u0, status, iters=0, Ru=0, d0=0, Dhat0=0, Yhat0=0,
                    stream=0):
        """All arguments are integer device addresses (0 = NULL); asynchronous on `stream`."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_step_device(self.h, v(xhat0), v(lastu0), v(Ry), v(Ru), v(d0),
                                                  v(Dhat0), v(Z), v(u0), v(status), v(iters),
                                                  v(Yhat0), v(stream)))

    def loop_device(self, xhat0, y0m, lastu0, Ry, Z, u0, status, iters=0, Ru=0, d0=0, Dhat0=0, Yhat0=0, stream=0):
        """preparestate! + moveinput! + updatestate! of one period in one launch (mpcqp_loop_device);
        integer device addresses, xhat0 updated in place."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_loop_device(self.h, v(xhat0), v(y0m), v(lastu0), v(Ry), v(Ru), v(d0), v(Dhat0),
                                                  v(Z), v(u0), v(status), v(iters), v(Yhat0), v(stream)))

    # -- ExplicitMPC: H̃ factored once (explicit_prepare), then a solve (explicit_step) or a gain (explicit_law) per period
    def explicit_prepare(self, law=False):
        """mpcqp_explicit_prepare: factor every controller's H̃ on the device; `law=True` builds the law tables too."""
        _chk(self.lib, self.lib.mpcqp_explicit_prepare(self.h, EXPLICIT_LAW if law else 0))

    def explicit_status(self):
        """(B,) int32: 0 factored, 2 H̃ not positive definite / not finite."""
        out = np.empty(self.B, np.int32)
        _chk(self.lib, self.lib.mpcqp_explicit_status(self.h, _ptr(out)))
        return out

    def explicit_step(self, xhat0, lastu0, Ry, Ru=None, d0=None, Dhat0=None, want_Yhat=False):
        """Host-pointer explicit step.  Returns Z (B,nZ), u0, status[, Yhat0]."""
        B = self.B
        x, lu, ry = _f64(xhat0), _f64(lastu0), _f64(Ry)
        ru, dd0, dh = (None if a is None else _f64(a) for a in (Ru, d0, Dhat0))
        nry = self.ny if (self.flags & FLAG_RY_CONSTANT) else self.nY
        if (x.size != B * self.nxhat or lu.size != B * self.nu or ry.size != B * nry or (ru is not None and ru.size != B * self.nU)
                or (dd0 is not None and dd0.size != B * self.nd) or (dh is not None and dh.size != B * self.nD)):
            raise ValueError("DimensionMismatch in step arguments")
        Z, u0, status = np.empty((B, self.nZ)), np.empty((B, self.nu)), np.empty(B, np.int32)
        yh = np.empty((B, self.nY)) if want_Yhat else None
        _chk(self.lib, self.lib.mpcqp_explicit_step(self.h, _ptr(x), _ptr(lu), _ptr(ry), _ptr(ru), _ptr(dd0), _ptr(dh),
                                                    _ptr(Z), _ptr(u0), _ptr(status), _ptr(yh)))
        return (Z, u0, status, yh) if want_Yhat else (Z, u0, status)

    def explicit_step_device(self, xhat0, lastu0, Ry, Z, u0, status, Ru=0, d0=0, Dhat0=0, Yhat0=0, stream=0):
        """All arguments are integer device addresses (0 = NULL); asynchronous on `stream`."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_explicit_step_device(self.h, v(xhat0), v(lastu0), v(Ry), v(Ru), v(d0), v(Dhat0),
                                                           v(Z), v(u0), v(status), v(Yhat0), v(stream)))

    def explicit_law(self, xhat0, lastu0, ry, d0=None, want_Z=True):
        """Host-pointer law call: Z̃ = g0 + Gx x̂0 + Gu lastu0 + Gr ry + Gd d0.  Returns Z (or None with want_Z=False), u0, status."""
        B = self.B
        x, lu, r = _f64(xhat0), _f64(lastu0), _f64(ry)
        dd0 = None if d0 is None else _f64(d0)
        if x.size != B * self.nxhat or lu.size != B * self.nu or r.size != B * self.ny or (dd0 is not None and dd0.size != B * self.nd):
            raise ValueError("DimensionMismatch in law arguments")
        Z = np.empty((B, self.nZ)) if want_Z else None
        u0, status = np.empty((B, self.nu)), np.empty(B, np.int32)
        _chk(self.lib, self.lib.mpcqp_explicit_law(self.h, _ptr(x), _ptr(lu), _ptr(r), _ptr(dd0), _ptr(Z), _ptr(u0), _ptr(status)))
        return Z, u0, status

    def explicit_law_device(self, xhat0, lastu0, ry, u0, status, Z=0, d0=0, stream=0):
        """Integer device addresses (Z = 0: u0 alone); asynchronous on `stream`."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_explicit_law_device(self.h, v(xhat0), v(lastu0), v(ry), v(d0), v(Z), v(u0), v(status), v(stream)))

    # -- sim!: closed loops of the whole batch, the plant on the device
    def sim_set_plant(self, A, Bu, Cm, Bd=None, Dd=None, fx=None):
        """mpcqp_sim_set_plant: A (B,nxp,nxp), Bu, Cm, Bd, Dd in ABI layout (see `colmajor`), fx = fop - xop (B,nxp)."""
        args = [None if a is None else _f64(a) for a in (A, Bu, Cm, Bd, Dd, fx)]
        nxp = int(round(np.sqrt(args[0].size // self.B)))
        _chk(self.lib, self.lib.mpcqp_sim_set_plant(self.h, nxp, *[_ptr(a) for a in args]))
        self.nxp = nxp

    def sim_path(self):
        return self.lib.mpcqp_sim_path(self.h)

    def sim(self, N, flags=0, **arrays):
        """Host-pointer mpcqp_sim.  `arrays`: the fields of mpcqp_sim_io by name, NumPy arrays in ABI layout ([B][n] or
        [B][N][n]) or None; float64 and C-contiguous ones among x0, xhat0, lastu0, Ztilde and the records are written in place."""
        io = SimIO(N=int(N), flags=int(flags))
        keep = []
        for k, v in arrays.items():
            if v is None:
                continue
            if k in SIM_IO_IN:
                v = _f64(v)
            elif k == "status":
                if v.dtype != np.int32 or not v.flags.c_contiguous:
                    raise ValueError("status must be a C-contiguous int32 array")
            elif k in SIM_IO_STATE + SIM_IO_RECORDS:
                if v.dtype != np.float64 or not v.flags.c_contiguous:
                    raise ValueError(f"{k} must be a C-contiguous float64 array (it is written in place)")
            else:
                raise TypeError(f"mpcqp_sim_io has no field {k!r}")
            keep.append(v)
            setattr(io, k, v.ctypes.data)
        _chk(self.lib, self.lib.mpcqp_sim(self.h, C.byref(io)))

    def sim_device(self, N, flags=0, stream=0, **addresses):
        """mpcqp_sim_device: the fields of mpcqp_sim_io as integer device addresses (0 = NULL); asynchronous on `stream`."""
        io = SimIO(N=int(N), flags=int(flags))
        for k, v in addresses.items():
            if k not in SIM_IO_IN + SIM_IO_STATE + SIM_IO_RECORDS + ("status",):
                raise TypeError(f"mpcqp_sim_io has no field {k!r}")
            setattr(io, k, int(v) if v else None)
        _chk(self.lib, self.lib.mpcqp_sim_device(self.h, C.byref(io), C.c_void_p(int(stream)) if stream else None))

    def recondense_device(self, stream=0):
        _chk(self.lib, self.lib.mpcqp_recondense_device(self.h, C.c_void_p(int(stream)) if stream else None))

    # -- LinMPC(MovingHorizonEstimator) and the estimator half of initstate! (include/mpcqp_mhe.h) ------------
    def mhe_attach(self, est, i_ym=None):
        """mpcqp_mhe_attach: `est` an `mhe.MheHandle` (borrowed: this object keeps a reference) or None to detach; i_ym the
        measured rows of Ĉ."""
        if not hasattr(self.lib, "mpcqp_mhe_attach"):
            raise NotImplementedError("this library has no mpcqp_mhe_attach")
        if est is None:
            _chk(self.lib, self.lib.mpcqp_mhe_attach(self.h, None, None, 0))
            self._mhe = None
            return
        iy = np.ascontiguousarray(i_ym, dtype=np.int32)
        _chk(self.lib, self.lib.mpcqp_mhe_attach(self.h, est._h, _ptr(iy), int(iy.size)))
        self._mhe, self.nym = est, int(iy.size)

    def sim_est_status(self, N):
        """(N,B) int32: the attached estimator's status after every period of the last `sim` / `sim_device`."""
        out = np.empty((int(N), self.B), np.int32)
        _chk(self.lib, self.lib.mpcqp_sim_est_status(self.h, _ptr(out), int(N)))
        return out

    def est_initstate(self, xhat0, u0, y0m, d0=None):
        """mpcqp_est_initstate: x̂0 (B,nx̂) float64, written in place for the members that solve; returns status (B,)."""
        assert xhat0.dtype == np.float64 and xhat0.flags.c_contiguous
        if not hasattr(self.lib, "mpcqp_est_initstate"):
            raise NotImplementedError("this library has no mpcqp_est_initstate")
        u, y, dd = _f64(u0), _f64(y0m), (None if d0 is None else _f64(d0))
        st = np.empty(self.B, np.int32)
        _chk(self.lib, self.lib.mpcqp_est_initstate(self.h, _ptr(xhat0), _ptr(u), _ptr(y), _ptr(dd), _ptr(st)))
        return st

    def est_initstate_device(self, xhat0, u0, y0m, status, d0=0, stream=0):
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_est_initstate_device(self.h, v(xhat0), v(u0), v(y0m), v(d0), v(status), v(stream)))

    def get(self, which):
        shape = {GET_HESSIAN: (self.B, self.nZ, self.nZ), GET_STEPRESP: (self.B, self.Hp, self.nu, self.ny),
                 GET_KMAT: (self.B, self.nxhat, self.nY), GET_BVEC: (self.B, self.nY),
                 GET_QTILDE: (self.B, self.nZ), GET_FVEC: (self.B, self.nY), GET_AUDIT: (self.B, 4),
                 GET_XHAT_MS: (self.B, self.Hp, self.nxhat), GET_MS_DEFECT: (self.B,),
                 GET_EXPLICIT_LAW: (self.B, 1 + self.nxhat + self.nu + self.ny + self.nd, self.nZ),
                 GET_KF_COV: (self.B, self.nxhat, self.nxhat), GET_KF_GAIN: (self.B, getattr(self, "nym", 0), self.nxhat),
                 GET_IM_XS: (self.B, getattr(self, "nxs", 0)), GET_IM_YS: (self.B, self.ny), GET_IM_YHATS: (self.B, self.nY),
                 GET_GDTAB: (self.B, self.Hp, self.ny, self.nd), GET_XDTAB: (self.B, self.Hp, self.nxhat, self.nd),
                 GET_EXHAT: (self.B, self.Hc, self.nxhat, self.nu), GET_KXHAT: (self.B, self.nxhat, self.nxhat),
                 GET_BXHAT: (self.B, self.nxhat)}[which]
        out = np.empty(shape)
        _chk(self.lib, self.lib.mpcqp_get(self.h, which, _ptr(out)))
        return out

    def audit(self):
        """What the convergence test of the last step saw: dict of (B,) arrays -- complementarity gap `mu`, relative
        dual / primal residuals `rd`, `rp`, and `polished` (the returned point passed the KKT check of the polish)."""
        a = self.get(GET_AUDIT)
        return {"mu": a[:, 0], "rd": a[:, 1], "rp": a[:, 2], "polished": a[:, 3] > 0.5}

    def last_step_ms(self):
        return self.lib.mpcqp_last_step_ms(self.h)

    # -- InternalModel (csrc/im_bodies.h) ------------------------------------------------------
    def im_set(self, stoch, i_ym):
        """mpcqp_im_set: `stoch` None (the default stochastic model: the identity in all four matrices) or (As, Bs, Cs, Ds) in
        ABI layout -- colmajor() of (B,nxs,nxs), (B,nxs,nym), (B,nym,nxs), (B,nym,nym); i_ym the measured rows of Ĉ."""
        if not hasattr(self.lib, "mpcqp_im_set"):
            raise NotImplementedError("this library has no mpcqp_im_set")
        iy = np.ascontiguousarray(i_ym, dtype=np.int32)
        if stoch is None:
            nxs, arrs = int(iy.size), [None] * 4
        else:
            arrs = [None if a is None else _f64(a) for a in stoch]
            nxs = int(arrs[0].shape[-1]) if arrs[0] is not None else 0
        _chk(self.lib, self.lib.mpcqp_im_set(self.h, nxs, *[_ptr(a) for a in arrs], _ptr(iy), int(iy.size)))
        self.nym, self.nxs = int(iy.size), nxs

    def im_status(self):
        """(B,) int32: 0 ready, 2 the member's Ds is singular (its stochastic part is off)."""
        out = np.empty(self.B, np.int32)
        _chk(self.lib, self.lib.mpcqp_im_status(self.h, _ptr(out)))
        return out

    def im_correct(self, xhat0, y0m, d0=None):
        """ŷs, Ŷs and B + Ŷs from x̂0 = x̂d (B,nx) -- not changed -- and y0m (B,nym)."""
        x, y, dd = _f64(xhat0), _f64(y0m), (None if d0 is None else _f64(d0))
        _chk(self.lib, self.lib.mpcqp_im_correct(self.h, _ptr(x), _ptr(y), _ptr(dd)))

    def im_update(self, xhat0, u0, d0=None):
        """x̂d <- Â x̂d + B̂u u0 + B̂d d0 + (f̂op - x̂op) in place on the (B,nx) host array, x̂s <- Âs x̂s + B̂s ŷs on the device."""
        assert xhat0.dtype == np.float64 and xhat0.flags.c_contiguous
        u, dd = _f64(u0), (None if d0 is None else _f64(d0))
        _chk(self.lib, self.lib.mpcqp_im_update(self.h, _ptr(xhat0), _ptr(u), _ptr(dd)))

    def im_correct_device(self, xhat0, y0m, d0=0, stream=0):
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_im_correct_device(self.h, v(xhat0), v(y0m), v(d0), v(stream)))

    def im_update_device(self, xhat0, u0, d0=0, stream=0):
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_im_update_device(self.h, v(xhat0), v(u0), v(d0), v(stream)))

    def im_state(self):
        """x̂s (B,nxs), ŷs (B,ny), Ŷs (B,nY) of the InternalModel."""
        return self.get(GET_IM_XS), self.get(GET_IM_YS), self.get(GET_IM_YHATS)

    # -- SteadyKalmanFilter steps -----------------------------------------------
    def kf_set(self, Khat, i_ym):
        K = _f64(Khat)
        iy = np.ascontiguousarray(i_ym, dtype=np.int32)
        self.nym = int(iy.size)
        _chk(self.lib, self.lib.mpcqp_kf_set(self.h, _ptr(K), _ptr(iy), self.nym))

    # -- time-varying KalmanFilter: covariance / gain recursion on the device (csrc/kf_kernels.hip) --------
    def kf_set_covariances(self, Qhat, Rhat, P0, i_ym):
        """Qhat (B,nx̂,nx̂), Rhat (B,nym,nym), P0 (B,nx̂,nx̂) or None (keep P̂: the Q̂, R̂ keywords of setmodel!), symmetric.
        The handle then runs the covariance recursion ahead of kf_correct / kf_predict / loop_device."""
        iy = np.ascontiguousarray(i_ym, dtype=np.int32)
        arrs = [None if a is None else colmajor(a) for a in (Qhat, Rhat, P0)]
        _chk(self.lib, self.lib.mpcqp_kf_set_covariances(self.h, *[_ptr(a) for a in arrs], _ptr(iy), int(iy.size)))
        self.nym = int(iy.size)

    def kf_set_state_covariance(self, P):
        _chk(self.lib, self.lib.mpcqp_kf_set_state_covariance(self.h, _ptr(colmajor(P))))

    def kf_covariance(self):
        """P̂ (B,nx̂,nx̂)."""
        return self.get(GET_KF_COV).transpose(0, 2, 1).copy()

    def kf_gain(self):
        """K̂ (B,nx̂,nym): the steady gain, or K̂(k) of the last correction."""
        return self.get(GET_KF_GAIN).transpose(0, 2, 1).copy()

    def kf_status(self):
        """(B,) int32, what became of the last correction attempt: 0 done, 1 skipped for a missing measurement (P̂ and K̂ keep
        their bits, the prediction runs), 2 dropped (include/mpcqp.h)."""
        out = np.empty(self.B, np.int32)
        _chk(self.lib, self.lib.mpcqp_kf_status(self.h, _ptr(out)))
        return out

    def kf_lanes_per_estimator(self):
        """0 on a steady gain; 16 / 64 lanes per estimator of the covariance kernel otherwise."""
        n = self.lib.mpcqp_kf_lanes_per_estimator(self.h)
        if n < 0:
            _chk(self.lib, n)
        return n

    def kf_set_direct(self, direct):
        """True (default): filter form; False: predictor form -- loop_device then runs step, correction, prediction.  The
        gain stays the filter-form gain in both forms (include/mpcqp.h)."""
        _chk(self.lib, self.lib.mpcqp_kf_set_direct(self.h, 1 if direct else 0))

    def kf_correct(self, xhat0, y0m, d0=None):
        """x̂0 += K̂ (y0m - Ĉm x̂0 - D̂dm d0), in place on the (B,nx̂) host array.  A member whose y0m row holds a NaN keeps
        its x̂0 (missed correction); y0m=None: every member misses."""
        assert xhat0.dtype == np.float64 and xhat0.flags.c_contiguous
        y, dd = (None if y0m is None else _f64(y0m)), (None if d0 is None else _f64(d0))
        _chk(self.lib, self.lib.mpcqp_kf_correct(self.h, _ptr(xhat0), _ptr(y), _ptr(dd)))

    def kf_predict(self, xhat0, u0, d0=None):
        """x̂0 <- Â x̂0 + B̂u u0 + B̂d d0 + (f̂op - x̂op), in place on the (B,nx̂) host array."""
        assert xhat0.dtype == np.float64 and xhat0.flags.c_contiguous
        u, dd = _f64(u0), (None if d0 is None else _f64(d0))
        _chk(self.lib, self.lib.mpcqp_kf_predict(self.h, _ptr(xhat0), _ptr(u), _ptr(dd)))

    def kf_update(self, xhat0, u0, y0m=None, d0=None):
        """Correction, then prediction (`updatestate!` of a direct=false estimator), in place on the (B,nx̂) host array;
        bit-equal to kf_correct followed by kf_predict.  y0m=None is the reference's `ym = nothing`: prediction only."""
        assert xhat0.dtype == np.float64 and xhat0.flags.c_contiguous
        u, y, dd = _f64(u0), (None if y0m is None else _f64(y0m)), (None if d0 is None else _f64(d0))
        _chk(self.lib, self.lib.mpcqp_kf_update(self.h, _ptr(xhat0), _ptr(u), _ptr(y), _ptr(dd)))

    def kf_update_device(self, xhat0, u0, y0m=0, d0=0, stream=0):
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_kf_update_device(self.h, v(xhat0), v(u0), v(y0m), v(d0), v(stream)))

    def kf_correct_device(self, xhat0, y0m, d0=0, stream=0):
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_kf_correct_device(self.h, v(xhat0), v(y0m), v(d0), v(stream)))

    def kf_predict_device(self, xhat0, u0, d0=0, stream=0):
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_kf_predict_device(self.h, v(xhat0), v(u0), v(d0), v(stream)))

    def last_condense_ms(self):
        return self.lib.mpcqp_last_condense_ms(self.h)

    def last_predmat_ms(self):
        return self.lib.mpcqp_last_predmat_ms(self.h)


class MultiHandle:
    """Binding of the mpcqp_multi_* entry points: one batch over several GPUs of a node (an ordinal
    may repeat), whole-batch HOST arrays in, whole-batch HOST arrays out."""

    def __init__(self, B, nxhat, nu, ny, nd, Hp, Hc, devices, nb=None, neps=1, flags=0, max_iter=0,
                 gap_tol=0.0, res_tol=0.0, dual_reg=0.0, lib=None):
        self.lib = lib or load_library()
        d = Dims(batch=B, nxhat=nxhat, nu=nu, ny=ny, nd=nd, Hp=Hp, Hc=Hc, neps=neps, device=0, flags=flags,
                 max_iter=max_iter, gap_tol=gap_tol, res_tol=res_tol, dual_reg=dual_reg)
        self._nb = None
        if nb is not None:
            self._nb = (C.c_int32 * len(nb))(*[int(v) for v in nb])
            d.nb = C.cast(self._nb, _ip)
        dev = (C.c_int32 * len(devices))(*[int(v) for v in devices])
        self.h = C.c_void_p()
        _chk(self.lib, self.lib.mpcqp_multi_create(C.byref(d), dev, len(devices), C.byref(self.h)))
        self.B, self.nxhat, self.nu, self.ny, self.nd, self.Hp, self.Hc = B, nxhat, nu, ny, nd, Hp, Hc
        self.nDU, self.nZ, self.nU, self.nY, self.nD = nu * Hc, nu * Hc + neps, nu * Hp, ny * Hp, nd * Hp
        self.flags = flags
        self._devices = [int(v) for v in devices]
        self.ndev = self.lib.mpcqp_multi_ndev(self.h)

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.mpcqp_multi_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard(self, g):
        o, n = C.c_int32(), C.c_int32()
        _chk(self.lib, self.lib.mpcqp_multi_shard(self.h, g, C.byref(o), C.byref(n)))
        return int(o.value), int(n.value)

    def set_model(self, Ahat, Bu, Cm, Bd=None, Dd=None, dop=None):
        args = [None if a is None else _f64(a) for a in (Ahat, Bu, Cm, Bd, Dd, dop)]
        _chk(self.lib, self.lib.mpcqp_multi_set_model(self.h, *[_ptr(a) for a in args]))

    def set_weights(self, Mdiag, Ndiag, Ldiag, Cwt=None):
        args = [None if a is None else _f64(a) for a in (Mdiag, Ndiag, Ldiag, Cwt)]
        _chk(self.lib, self.lib.mpcqp_multi_set_weights(self.h, *[_ptr(a) for a in args]))

    def set_bounds(self, **kw):
        b = Bounds()
        keep = []
        for k in BOUND_FIELDS:
            v = kw.get(k)
            if v is not None:
                a = _f64(v)
                keep.append(a)
                setattr(b, k, a.ctypes.data_as(_dp))
        _chk(self.lib, self.lib.mpcqp_multi_set_bounds(self.h, C.byref(b)))

    def prepare(self):
        k = self.lib.mpcqp_multi_prepare(self.h)
        if k < 0:
            _chk(self.lib, k)
        return k

    def step(self, xhat0, lastu0, Ry, Z, Ru=None, d0=None, Dhat0=None, want_Yhat=False):
        B = self.B
        x, lu, ry = _f64(xhat0), _f64(lastu0), _f64(Ry)
        ru = None if Ru is None else _f64(Ru)
        dd0 = None if d0 is None else _f64(d0)
        dh = None if Dhat0 is None else _f64(Dhat0)
        assert Z.dtype == np.float64 and Z.flags.c_contiguous and Z.size == B * self.nZ
        u0 = np.empty((B, self.nu)); status = np.empty(B, np.int32); iters = np.empty(B, np.int32)
        yh = np.empty((B, self.nY)) if want_Yhat else None
        _chk(self.lib, self.lib.mpcqp_multi_step(self.h, _ptr(x), _ptr(lu), _ptr(ry), _ptr(ru), _ptr(dd0), _ptr(dh),
                                                 _ptr(Z), _ptr(u0), _ptr(status), _ptr(iters), _ptr(yh)))
        return (u0, status, iters, yh) if want_Yhat else (u0, status, iters)


    # ---- device-resident path: per-device buffers, nothing crosses PCIe --------------------------------------
    def device_of(self, g):
        """CUDA/HIP ordinal the shard g lives on (as given to the constructor)."""
        return self._devices[g]

    def step_device_shard(self, g, xhat0, lastu0, Ry, Z, u0, status, iters=0, stream=0):
        """mpcqp_step_device on the handle of shard g: integer device addresses of that shard's buffers."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        hg = C.c_void_p(self.lib.mpcqp_multi_handle(self.h, g))
        _chk(self.lib, self.lib.mpcqp_step_device(hg, v(xhat0), v(lastu0), v(Ry), None, None, None, v(Z), v(u0), v(status),
                                                  v(iters), None, v(stream)))

    def scatter_device(self, root, xhat0_root, lastu0_root, Ry_root, ry_rows, xhat0_shards, lastu0_shards, Ry_shards, stream=0):
        """mpcqp_multi_scatter_device: whole-batch inputs on device `root` -> the shards' buffers (integer addresses)."""
        arr = lambda ps: (C.c_void_p * len(ps))(*[C.c_void_p(int(p)) for p in ps])
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_multi_scatter_device(self.h, root, v(xhat0_root), v(lastu0_root), v(Ry_root), int(ry_rows),
                                                          arr(xhat0_shards), arr(lastu0_shards), arr(Ry_shards), v(stream)))

    def gather_device(self, root, Z_shards, u0_shards, status_shards, Z_root, u0_root, status_root, stream=0):
        """mpcqp_multi_gather_device: the shards' Z̃, u0, status -> whole-batch buffers on device `root`."""
        arr = lambda ps: (C.c_void_p * len(ps))(*[C.c_void_p(int(p)) for p in ps])
        v = lambda p: C.c_void_p(int(p)) if p else None
        _chk(self.lib, self.lib.mpcqp_multi_gather_device(self.h, root, arr(Z_shards), arr(u0_shards), arr(status_shards),
                                                         v(Z_root), v(u0_root), v(status_root), v(stream)))


def steady_kalman_gain(Ahat, Chat, Qhat, Rhat, i_ym=None):
    """K̂ of `SteadyKalmanFilter` for a batch: filter-form gain P Ĉm'(Ĉm P Ĉm' + R̂)^-1 with P the
    predictor DARE solution (`init_skf`, src/estimator/kalman.jl:204-236; construction-time,
    host-side like the reference, which calls ControlSystemsBase.kalman)."""
    from scipy.linalg import solve_discrete_are
    Ahat, Chat = np.asarray(Ahat, float), np.asarray(Chat, float)
    B, ny, nxh = Chat.shape
    i_ym = np.arange(ny) if i_ym is None else np.asarray(i_ym, int)
    Q = np.broadcast_to(np.asarray(Qhat, float), (B, nxh, nxh))
    R = np.broadcast_to(np.asarray(Rhat, float), (B, len(i_ym), len(i_ym)))
    K = np.empty((B, nxh, len(i_ym)))
    for b in range(B):
        Cm = Chat[b][i_ym]
        P = solve_discrete_are(Ahat[b].T, Cm.T, Q[b], R[b])
        K[b] = P @ Cm.T @ np.linalg.inv(Cm @ P @ Cm.T + R[b])
    return K


def move_blocking(Hp, Hc):
    """`move_blocking` (src/controller/construct.jl:629-660): integer or vector Hc -> nb."""
    if np.isscalar(Hc):
        Hc = int(Hc)
        nb = [1] * Hc
        if Hc > 0:
            nb[-1] = Hp - Hc + 1
        return nb
    nb = [int(v) for v in Hc]
    if not all(v > 0 for v in nb):
        raise ValueError("Move blocking vector must be strictly positive integers.")
    if sum(nb) < Hp:
        nb = nb + [Hp - sum(nb)]
    elif sum(nb) > Hp:
        keep = int(np.argmax(np.cumsum(nb) >= Hp)) + 1
        nb = nb[:keep]
        if sum(nb) > Hp:
            nb[-1] = Hp - sum(nb[:-1])
    return nb


@dataclasses.dataclass
class SimResult:
    """What `BatchLinMPC.sim` returns: the fields of the reference's `SimResult` (src/plot_sim.jl:1-60) with a leading batch
    axis, each (B,n,N) in engineering units -- X̂_data is the estimate after the correction of its period -- plus `status`
    (B,N), the controller's status per period, `path`, the execution path of the run (api.SIM_PATH_PERIOD), and, with a
    MovingHorizonEstimator attached, `est_status` (B,N), the estimator's status per period (None otherwise)."""
    N: int
    Y_data: np.ndarray
    Ry_data: np.ndarray
    Ŷ_data: np.ndarray
    U_data: np.ndarray
    Ud_data: np.ndarray
    Ru_data: np.ndarray
    D_data: np.ndarray
    X_data: np.ndarray
    X̂_data: np.ndarray
    status: np.ndarray
    path: int
    est_status: np.ndarray = None

    Yhat_data = property(lambda self: self.Ŷ_data)         # the reference's ASCII aliases
    Xhat_data = property(lambda self: self.X̂_data)


class BatchLinMPC:
    """B independent `LinMPC` controllers on augmented models (Â, B̂u, Ĉ, B̂d, D̂d), one GPU.

    Array arguments carry a leading batch axis: Ahat (B,nx̂,nx̂), Bhu (B,nx̂,nu), Chat (B,ny,nx̂),
    Bhd (B,nx̂,nd), Dhd (B,ny,nd).  Weights are per channel (ny / nu values, shared or (B,·)),
    repeated over the horizons like `Diagonal(repeat(Mwt, Hp))`; Cwt scalar or (B,).
    """

    def __init__(self, Ahat, Bhu, Chat, Bhd=None, Dhd=None, *, Hp, Hc=2, Mwt=None, Nwt=None,
                 Lwt=None, M_Hp=None, N_Hc=None, L_Hp=None, Cwt=1e5, Wy=None, Wu=None, Wd=None, Wr=None, uop=None, yop=None, dop=None, xhop=None, fhop=None, device=0,
                 cold_start=False, keep_qp=False, warm_dual=False, max_iter=0, gap_tol=0.0, res_tol=0.0, dual_reg=0.0,
                 transcription="SingleShooting", lib=None):
        # `transcription` (LinMPC keyword, linmpc.jl:288-316).  MultipleShooting (Z = [ΔU; X̂0] with the model as
        # equality constraints, transcription.jl:217-240, 373-414, 913-928) runs on the stage-structured kernel of
        # csrc/ms_bodies.h (Riccati recursion inside the interior-point iteration; H̃ and E are never formed): what the
        # reference recommends for unstable plants / long horizons, construct.jl:855-866.  Handles that kernel does not
        # take (block / dense weight matrices, custom linear constraints, stage data beyond the LDS) keep the condensed
        # kernels -- same optimal ΔU -- with a warning; getinfo returns Z̃ in the transcription's layout either way.
        if transcription not in ("SingleShooting", "MultipleShooting"):
            raise NotImplementedError(f"transcription {transcription!r}: only SingleShooting / MultipleShooting (LinModel)")
        self.transcription = transcription
        Ahat, Bhu, Chat = (np.asarray(a, float) for a in (Ahat, Bhu, Chat))
        if Ahat.ndim != 3 or Bhu.ndim != 3 or Chat.ndim != 3:
            raise ValueError("model matrices need a leading batch axis")
        B, nxh, nu = Bhu.shape
        ny = Chat.shape[1]
        nd = 0 if Bhd is None else np.asarray(Bhd).shape[2]
        if Ahat.shape != (B, nxh, nxh) or Chat.shape != (B, ny, nxh):
            raise ValueError("DimensionMismatch between Ahat, Bhu, Chat")
        Hp = int(Hp)
        if Hp < 1:
            raise ValueError("Prediction horizon Hp should be ≥ 1")
        nb = move_blocking(Hp, Hc)
        Hc = len(nb)
        if Hc < 1:
            raise ValueError("Control horizon Hc should be ≥ 1")
        if Hc > Hp:
            raise ValueError("Control horizon Hc should be ≤ prediction horizon Hp")
        cw = np.broadcast_to(np.asarray(Cwt, float), (B,)).copy()
        if np.any(cw < 0):
            raise ValueError("Cwt weight should be ≥ 0")
        if np.isinf(cw).any() and not np.isinf(cw).all():
            raise ValueError("Cwt must be finite for all controllers of a batch, or Inf for all")
        self.neps = 0 if np.isinf(cw).all() else 1
        self.B, self.nxh, self.nu, self.ny, self.nd, self.Hp, self.Hc, self.nb = B, nxh, nu, ny, nd, Hp, Hc, nb
        flags = (FLAG_RY_CONSTANT * 0 | (FLAG_COLD_START if cold_start else 0) | (FLAG_KEEP_QP if keep_qp else 0)
                 | (FLAG_WARM_DUAL if warm_dual else 0))
        self.hd = Handle(B, nxh, nu, ny, nd, Hp, Hc, nb=nb, neps=self.neps, device=device, flags=flags,
                         max_iter=max_iter, gap_tol=gap_tol, res_tol=res_tol, dual_reg=dual_reg, lib=lib)
        self.nZ, self.nDU, self.nU, self.nY = self.hd.nZ, self.hd.nDU, self.hd.nU, self.hd.nY
        vec = lambda v, n: np.zeros((B, n)) if v is None else np.broadcast_to(np.asarray(v, float), (B, n)).copy()
        self.uop, self.yop, self.dop = vec(uop, nu), vec(yop, ny), vec(dop, nd)
        self.xhop, self.fhop = vec(xhop, nxh), vec(fhop, nxh)
        self.Uop, self.Yop, self.Dop = np.tile(self.uop, Hp), np.tile(self.yop, Hp), np.tile(self.dop, Hp)
        self.Cwt = cw
        self.setmodel(Ahat, Bhu, Chat, Bhd, Dhd)
        self.setweights(Mwt, Nwt, Lwt, M_Hp=M_Hp, N_Hc=N_Hc, L_Hp=L_Hp)
        # custom linear constraints (validate_custom_lincon, src/controller/construct.jl:666-694)
        given = [np.asarray(W, float) for W in (Wy, Wu, Wd, Wr) if W is not None]
        self.nw = 0
        if given:
            first = given[0]
            self.nw = (first.shape[0] if first.ndim == 2 else first.shape[1]) if first.ndim >= 2 else 1
        nw = self.nw
        def wmat(Wm, n, name):
            if Wm is None:
                return np.zeros((B, nw, n))
            a = np.asarray(Wm, float)
            if a.ndim == 1:
                a = a.reshape(1, -1)
            if a.ndim == 2:
                a = np.broadcast_to(a, (B,) + a.shape)
            if a.shape[2] != n:
                raise ValueError(f"{name} must have {n} columns")           # DimensionMismatch, :686-689
            if a.shape[1] != nw:
                raise ValueError("Wy, Wu, Wd and Wr must have the same number of rows")
            return a.copy()
        self.Wy, self.Wu, self.Wd, self.Wr = wmat(Wy, ny, "Wy"), wmat(Wu, nu, "Wu"), wmat(Wd, nd, "Wd"), wmat(Wr, ny, "Wr")
        self._wb = dict(Wmin=None, Wmax=None, C_wmin=None, C_wmax=None)
        if nw > 0:
            w_op = (np.einsum("bij,bj->bi", self.Wy, self.yop) + np.einsum("bij,bj->bi", self.Wu, self.uop)
                    + np.einsum("bij,bj->bi", self.Wr, self.yop))
            if nd > 0:
                w_op = w_op + np.einsum("bij,bj->bi", self.Wd, self.dop)
            self.hd.set_custom_constraints(nw, colmajor(self.Wy), colmajor(self.Wu),
                                           colmajor(self.Wd) if nd > 0 else None, colmajor(self.Wr), w_op)
        # default constraints: none (src/controller/construct.jl:887-913)
        self._b = {k: None for k in BOUND_FIELDS}
        self._prepared = False                     # specialised kernel built/loaded for the current pattern
        self.Z = np.zeros((B, self.nZ))            # mpc.Z̃ (previous optimum)
        self.lastu0 = np.zeros((B, nu))            # mpc.lastu0
        self.solved_once = False
        self.status = np.zeros(B, np.int32)
        self.iters = np.zeros(B, np.int32)

    # -- model / weights ---------------------------------------------------------------------
    def setmodel(self, Ahat, Bhu, Chat, Bhd=None, Dhd=None, *, xhop=None, fhop=None):
        """`setmodel!` re-condensation path (src/controller/execute.jl:684-790): K1 (+K2).  `xhop` / `fhop`: new x̂op / f̂op; the
        state of an attached Kalman filter or InternalModel keeps its engineering value (`estim.x̂0 .+= x̂op_old .- x̂op_new`).
        An InternalModel keeps x̂s, ŷs and its stochastic model (setmodel_estimator!, internal_model.jl:241-257): the next
        step uses the new model with the Ŷs of the last correction."""
        if xhop is not None:
            new = np.broadcast_to(np.asarray(xhop, float), (self.B, self.nxh)).copy()
            if getattr(self, "mhe", None) is None and "_xhat0" in self.__dict__:
                self.xhat0 = self.xhat0 + self.xhop - new
            self.xhop = new
        if fhop is not None:
            self.fhop = np.broadcast_to(np.asarray(fhop, float), (self.B, self.nxh)).copy()
        dopv = self.fhop - self.xhop
        self._Ahat, self._Bhu = np.asarray(Ahat, float).copy(), np.asarray(Bhu, float).copy()
        self._Chat = np.asarray(Chat, float).copy()
        self._Bhd = None if self.nd == 0 else np.asarray(Bhd, float).copy()
        self._Dhd = None if self.nd == 0 else np.asarray(Dhd, float).copy()
        self.hd.set_model(colmajor(Ahat), colmajor(Bhu), colmajor(Chat),
                          None if self.nd == 0 else colmajor(Bhd),
                          None if self.nd == 0 else colmajor(Dhd),
                          dopv if np.any(dopv != 0) else None)
        self._model_changed()

    def _model_changed(self):
        """What follows a new resident model: the estimator gains that are solved from it, and the attached estimator."""
        if getattr(self, "kf_steady", False):      # SteadyKalmanFilter from Q̂ and R̂: the gain follows the model
            self.hd.kf_solve_steady()
            self._warn_steady()
        if getattr(self, "kf_luenberger", False):  # Luenberger from its poles: so does this one
            self.hd.kf_place()
            self._warn_luenberger()
        est = getattr(self, "mhe", None)
        if est is not None:                        # the attached MovingHorizonEstimator: the measured rows of Ĉ and D̂d
            ops = self.__dict__.pop("_mhe_ops", {})
            est.setmodel(self._Ahat, self._Bhu, self._Chat[:, self.i_ym], self._Bhd,
                         None if self.nd == 0 else self._Dhd[:, self.i_ym], **ops)

    # -- continuous-time models: LinModel(sys, Ts) + augment_model on the device (csrc/c2d_bodies.h) --------------
    @classmethod
    def from_continuous(cls, A, Bu, C, Ts, Bd=None, Dd=None, *, nint_u=0, nint_ym=None, i_ym=None, d_method="tustin",
                        xop=None, fop=None, lib=None, **kw):
        """`LinMPC(LinModel(sys, Ts))` for a batch of continuous-time models: A (B,nx,nx), Bu (B,nx,nu), C (B,ny,nx), Bd
        (B,nx,nd), Dd (B,ny,nd) (a single model may come without the batch axis, scalars included), Ts scalar or (B,).  Every
        member is discretised on the device -- zero-order hold for the manipulated inputs, Tustin for the measured
        disturbances (linmodel.jl:165-198; d_method="zoh": zero-order hold for them too, one state vector) -- and augmented
        with the integrators of nint_u / nint_ym (construct.jl:305-323; nint_ym=None: one per measured output, none when any
        nint_u != 0; nothing is pruned, there is no sminreal / minreal).  `xop` / `fop` (nx_dis values) are padded with zeros
        to x̂op / f̂op.  The other keywords are the constructor's.  `c2d_status` holds the per-member status: a member with
        2 was refused (one RuntimeWarning with the count) and has a zero model."""
        (B, nx, nu, ny, nd), _ = _c2d_inputs(A, Bu, C, Ts, Bd, Dd)
        o = C2dOptions(B, nx, nu, ny, nd, nint_u, nint_ym, i_ym, d_method)
        A, Bu, C, Bd, Dd = _c2d_batch(A, Bu, C, Bd, Dd)
        Ah, Bh, Ch, Bdh, Ddh, st = c2d(A, Bu, C, Ts, Bd, Dd, nint_u=o.nint_u, nint_ym=o.nint_ym, i_ym=o.i_ym, d_method=d_method, lib=lib)
        pad = lambda v: None if v is None else np.hstack([np.broadcast_to(np.asarray(v, float), (B, o.nxd)), np.zeros((B, o.nxh - o.nxd))])
        self = cls(Ah, Bh, Ch, Bdh, Ddh, xhop=pad(xop), fhop=pad(fop), lib=lib, **kw)
        self._c2d_opts, self.c2d_status = o, st
        self._warn_c2d()
        return self

    def setmodel_continuous(self, A, Bu, C, Ts, Bd=None, Dd=None, *, nint_u=None, nint_ym=None, i_ym=None, d_method=None,
                            xop=None, fop=None):
        """`setmodel!` from continuous-time matrices: the discretisation and augmentation of `from_continuous`, written by the
        kernel straight into the resident model, then the re-condensation -- one call, nothing computed on the host -- and
        everything `setmodel` does once the model is in place (the steady gain solved again, the poles placed again, an
        attached MovingHorizonEstimator handed the new model, x̂op / f̂op).  The options default to those of `from_continuous`.
        A refused member (status 2 in `c2d_status`, one RuntimeWarning with the count) keeps the model it had."""
        (B, nx, nu, ny, nd), bufs = _c2d_inputs(A, Bu, C, Ts, Bd, Dd)
        prev = getattr(self, "_c2d_opts", None)
        pick = lambda v, name, default: v if v is not None else (getattr(prev, name) if prev is not None else default)
        o = C2dOptions(B, nx, nu, ny, nd, pick(nint_u, "nint_u", 0), nint_ym if nint_ym is not None or prev is None else prev.nint_ym,
                       pick(i_ym, "i_ym", None), pick(d_method, "d_method", "tustin"))
        if (B, o.nxh, nu, ny, nd) != (self.B, self.nxh, self.nu, self.ny, self.nd):
            raise ValueError("DimensionMismatch between the continuous model with its integrators and the controller")
        pad = lambda v: np.hstack([np.broadcast_to(np.asarray(v, float), (B, o.nxd)), np.zeros((B, o.nxh - o.nxd))])
        if xop is not None:
            new = pad(xop)
            if getattr(self, "mhe", None) is None and "_xhat0" in self.__dict__:
                self.xhat0 = self.xhat0 + self.xhop - new
            self.xhop = new
        if fop is not None:
            self.fhop = pad(fop)
        dopv = (self.fhop - self.xhop)[:, :o.nxd]
        st = self.hd.set_model_continuous(o, *bufs[:3], bufs[5], bufs[3], bufs[4], _f64(dopv) if np.any(dopv != 0) else None)
        self._Ahat, self._Bhu, self._Chat, self._Bhd, self._Dhd, _ = self.hd.get_model()     # (the mirrors: what the device produced)
        self._c2d_opts, self.c2d_status = o, st
        self._warn_c2d()
        self._model_changed()

    def _warn_c2d(self):
        """One warning for the members whose continuous model could not be discretised."""
        n = int(np.count_nonzero(self.c2d_status))
        if n:
            warnings.warn("Cannot discretise the continuous model: a value is not finite, Ts is not positive or I - Ts/2 A is "
                          f"singular, the previous model (or zero) stays ({n} of {self.B} controllers)", RuntimeWarning)

    def setweights(self, Mwt=None, Nwt=None, Lwt=None, M_Hp=None, N_Hc=None, L_Hp=None):
        """Defaults of src/general.jl:3-6 (Mwt=1, Nwt=0.1, Lwt=0).  `M_Hp` (nY,nY), `N_Hc` (nΔU,nΔU), `L_Hp`
        (nU,nU) -- each also (B,n,n) -- are the reference's full weight matrices (src/controller/linmpc.jl:205-214,
        construct.jl:45-93); they override the per-channel vectors.  A block-diagonal M_Hp = blkdiag(M_1..M_Hp)
        (e.g. a terminal cost) keeps the specialised step kernels; an M_Hp or L_Hp that couples different prediction
        steps runs on the runtime-dimension kernel; a dense N_Hc only changes H̃."""
        B, Hp, Hc, ny = self.B, self.Hp, self.Hc, self.ny
        w = lambda v, n, dflt: (np.full((B, n), dflt) if v is None
                                else np.broadcast_to(np.asarray(v, float), (B, n)).copy())
        M, N, L = w(Mwt, self.ny, 1.0), w(Nwt, self.nu, 0.1), w(Lwt, self.nu, 0.0)
        for name, a in (("Mwt", M), ("Nwt", N), ("Lwt", L)):
            if np.any(a < 0):
                raise ValueError(f"{name} values should be nonnegative")
        self.Mwt, self.Nwt, self.Lwt = M, N, L
        self.hd.set_weights(np.tile(M, Hp), np.tile(N, Hc), np.tile(L, Hp),
                            self.Cwt if self.neps else None)

        def full(Mx, n, name):
            if Mx is None:
                return None
            Mf = np.asarray(Mx, float)
            if Mf.shape == (n, n):
                Mf = np.broadcast_to(Mf, (B, n, n))
            if Mf.shape != (B, n, n):
                raise ValueError(f"{name} size should be ({n}, {n})")
            if not np.allclose(Mf, Mf.transpose(0, 2, 1), rtol=0, atol=1e-12 * max(1.0, np.abs(Mf).max())):
                raise ValueError(f"{name} should be Hermitian")
            return np.ascontiguousarray(Mf)

        self.Mblk, self.Mfull = None, None
        Mf, self.Ndense, self.Ldense = full(M_Hp, self.nY, "M_Hp"), full(N_Hc, self.nDU, "N_Hc"), full(L_Hp, self.nU, "L_Hp")
        if Mf is not None:
            blk = np.stack([Mf[:, t * ny:(t + 1) * ny, t * ny:(t + 1) * ny] for t in range(Hp)], axis=1)
            off = Mf.copy()
            for t in range(Hp):
                off[:, t * ny:(t + 1) * ny, t * ny:(t + 1) * ny] = 0.0
            if np.any(off != 0.0):
                self.Mfull = Mf                      # couples different prediction steps: dense path
            else:
                self.Mblk = blk
        if self.Mblk is not None:
            self.hd.set_output_weight_blocks(self.Mblk)
        elif getattr(self, "_had_blocks", False):
            self.hd.set_output_weight_blocks(None)
        self._had_blocks = self.Mblk is not None
        dense = (self.Mfull, self.Ndense, self.Ldense)
        if any(a is not None for a in dense) or getattr(self, "_had_dense", False):
            self.hd.set_dense_weights(*dense)
        self._had_dense = any(a is not None for a in dense)
        self._prepared = False

    # -- constraints --------------------------------------------------------------------------
    def setconstraint(self, *, umin=None, umax=None, Δumin=None, Δumax=None, ymin=None, ymax=None,
                      x̂min=None, x̂max=None, Umin=None, Umax=None, ΔUmin=None, ΔUmax=None,
                      Ymin=None, Ymax=None, c_umin=None, c_umax=None, c_Δumin=None, c_Δumax=None,
                      c_ymin=None, c_ymax=None, c_x̂min=None, c_x̂max=None,
                      Deltaumin=None, Deltaumax=None, xhatmin=None, xhatmax=None,
                      DeltaUmin=None, DeltaUmax=None, c_Deltaumin=None, c_Deltaumax=None,
                      c_xhatmin=None, c_xhatmax=None, wmin=None, wmax=None, Wmin=None, Wmax=None,
                      c_wmin=None, c_wmax=None, C_wmin=None, C_wmax=None,
                      C_umin=None, C_umax=None, C_Δumin=None, C_Δumax=None, C_ymin=None, C_ymax=None,
                      C_Deltaumin=None, C_Deltaumax=None):
        """`setconstraint!` (src/controller/construct.jl:324-559), with the ASCII
        aliases.  Bounds are engineering values (operating points are subtracted here, :356-435);
        per-channel vectors (n,) or (B,n) are repeated over the horizon, capitalised keywords take
        the whole horizon."""
        Δumin = Deltaumin if Δumin is None else Δumin
        Δumax = Deltaumax if Δumax is None else Δumax
        x̂min = xhatmin if x̂min is None else x̂min
        x̂max = xhatmax if x̂max is None else x̂max
        ΔUmin = DeltaUmin if ΔUmin is None else ΔUmin
        ΔUmax = DeltaUmax if ΔUmax is None else ΔUmax
        c_Δumin = c_Deltaumin if c_Δumin is None else c_Δumin
        c_Δumax = c_Deltaumax if c_Δumax is None else c_Δumax
        c_x̂min = c_xhatmin if c_x̂min is None else c_x̂min
        c_x̂max = c_xhatmax if c_x̂max is None else c_x̂max
        B, Hp, Hc, nu, ny, nxh = self.B, self.Hp, self.Hc, self.nu, self.ny, self.nxh

        def rep(v, n, reps, name):
            a = np.asarray(v, float)
            if a.shape not in ((n,), (B, n)):
                raise ValueError(f"{name} size must be ({n},)")
            return np.tile(np.broadcast_to(a, (B, n)), reps)

        def full(v, n, name):
            a = np.asarray(v, float)
            if a.shape not in ((n,), (B, n)):
                raise ValueError(f"{name} size must be ({n},)")
            return np.broadcast_to(a, (B, n)).copy()

        new = dict(self._b)
        if Umin is not None:
            new["U0min"] = full(Umin, nu * Hp, "Umin") - self.Uop
        elif umin is not None:
            new["U0min"] = rep(umin, nu, Hp, "umin") - self.Uop
        if Umax is not None:
            new["U0max"] = full(Umax, nu * Hp, "Umax") - self.Uop
        elif umax is not None:
            new["U0max"] = rep(umax, nu, Hp, "umax") - self.Uop
        if ΔUmin is not None:
            new["DUmin"] = full(ΔUmin, nu * Hc, "ΔUmin")
        elif Δumin is not None:
            new["DUmin"] = rep(Δumin, nu, Hc, "Δumin")
        if ΔUmax is not None:
            new["DUmax"] = full(ΔUmax, nu * Hc, "ΔUmax")
        elif Δumax is not None:
            new["DUmax"] = rep(Δumax, nu, Hc, "Δumax")
        if Ymin is not None:
            new["Y0min"] = full(Ymin, ny * Hp, "Ymin") - self.Yop
        elif ymin is not None:
            new["Y0min"] = rep(ymin, ny, Hp, "ymin") - self.Yop
        if Ymax is not None:
            new["Y0max"] = full(Ymax, ny * Hp, "Ymax") - self.Yop
        elif ymax is not None:
            new["Y0max"] = rep(ymax, ny, Hp, "ymax") - self.Yop
        if x̂min is not None:
            new["x0min"] = full(x̂min, nxh, "x̂min") - self.xhop
        if x̂max is not None:
            new["x0max"] = full(x̂max, nxh, "x̂max") - self.xhop
        # softness: per channel (repeated over the horizon) or horizon-long `C_umin` ... `C_ymax` (construct.jl:446-509).  A
        # C_umin / C_umax that varies inside a move-blocking interval sends the handle to the stage-structured kernel
        # (mpcqp_set_bounds), which keeps one input row per step.
        C_Δumin = C_Deltaumin if C_Δumin is None else C_Δumin
        C_Δumax = C_Deltaumax if C_Δumax is None else C_Δumax
        ecr = dict(C_umin=(c_umin, nu, Hp, C_umin), C_umax=(c_umax, nu, Hp, C_umax), C_dumin=(c_Δumin, nu, Hc, C_Δumin),
                   C_dumax=(c_Δumax, nu, Hc, C_Δumax), C_ymin=(c_ymin, ny, Hp, C_ymin), C_ymax=(c_ymax, ny, Hp, C_ymax),
                   c_x0min=(c_x̂min, nxh, 1, None), c_x0max=(c_x̂max, nxh, 1, None))
        if any(v[0] is not None or v[3] is not None for v in ecr.values()):
            if self.neps != 1:
                raise ValueError("Slack variable weight Cwt must be finite to set softness parameters")
            if self.solved_once:
                raise RuntimeError("Cannot set softness parameters after calling moveinput!")
        for k, (v, n, reps, whole) in ecr.items():
            if whole is not None or v is not None:
                a = full(whole, n * reps, k) if whole is not None else rep(v, n, reps, k)
                if np.any(a < 0):
                    raise ValueError(f"{k} weights should be non-negative")
                new[k] = a
                self._prepared = False         # (the kernel that takes the handle may change, see above)
        if self.solved_once:
            # src/controller/construct.jl:541-551: the ±Inf pattern is frozen after the first solve
            for k in BOUND_FIELDS[:8]:
                old_inf = np.isinf(self._b[k]) if self._b[k] is not None else True
                new_inf = np.isinf(new[k]) if new[k] is not None else True
                if np.any(old_inf != new_inf):
                    raise RuntimeError("Cannot modify ±Inf constraints after calling moveinput!")
        # custom linear constraints: wmin/wmax (nw,) repeated over the Hp+1 steps, or Wmin/Wmax
        # (nw (Hp+1),) (construct.jl:411-426, 487-494)
        neww = dict(self._wb)
        nW = self.nw * (Hp + 1)
        for key, per, whole, nm in (("Wmin", wmin, Wmin, "wmin"), ("Wmax", wmax, Wmax, "wmax"),
                                    ("C_wmin", c_wmin, C_wmin, "c_wmin"), ("C_wmax", c_wmax, C_wmax, "c_wmax")):
            if whole is not None:
                neww[key] = full(whole, nW, nm.capitalize())
            elif per is not None:
                neww[key] = rep(per, self.nw, Hp + 1, nm)
        for key in ("C_wmin", "C_wmax"):
            if neww[key] is not self._wb[key]:
                if self.neps != 1:
                    raise ValueError("Slack variable weight Cwt must be finite to set softness parameters")
                if self.solved_once:
                    raise RuntimeError("Cannot set softness parameters after calling moveinput!")
                if np.any(neww[key] < 0):
                    raise ValueError(f"{key} weights should be non-negative")
        if self.solved_once:
            for key in ("Wmin", "Wmax"):
                old_inf = np.isinf(self._wb[key]) if self._wb[key] is not None else True
                new_inf = np.isinf(neww[key]) if neww[key] is not None else True
                if np.any(old_inf != new_inf):
                    raise RuntimeError("Cannot modify ±Inf constraints after calling moveinput!")
        self._b = new
        self.hd.set_bounds(**{k: v for k, v in new.items() if v is not None})
        self._prepared = False
        if self.nw > 0 and any(neww[k] is not self._wb[k] for k in neww):
            fin = lambda a: None if a is None or np.all(np.isinf(a)) else a
            self.hd.set_custom_bounds(fin(neww["Wmin"]), fin(neww["Wmax"]), neww["C_wmin"], neww["C_wmax"])
        self._wb = neww
        return self

    # -- estimator steps on both sides of moveinput! (SteadyKalmanFilter) ---------------------
    @property
    def xhat0(self):
        """The attached estimator's x̂0 (deviation, (B,nx̂)): this object's own array behind a Kalman filter, a mirror of
        `mhe.x̂0` behind a MovingHorizonEstimator (assigning it is `setstate!`: x̂0 and nothing else)."""
        est = self.__dict__.get("mhe")
        if est is not None:
            return est.x̂0
        if "_xhat0" not in self.__dict__:
            raise AttributeError("xhat0")
        return self.__dict__["_xhat0"]

    @xhat0.setter
    def xhat0(self, v):
        est = self.__dict__.get("mhe")
        if est is not None:
            est.x̂0 = _f64(v).copy()
            est.handle.set_state(est.x̂0)
        else:
            self.__dict__["_xhat0"] = v

    def _attach_mhe(self, est, i_ym, direct):
        from .mhe import BatchMHE
        if not isinstance(est, BatchMHE):
            raise ValueError("mhe must be a BatchMHE")
        if est.handle.lib is not self.hd.lib:
            raise ValueError("the estimator and the controller were created on different libraries")
        i_ym = np.arange(self.ny) if i_ym is None else np.asarray(i_ym, int)
        if (est.B, est.nx̂, est.nu, est.nd, est.nym) != (self.B, self.nxh, self.nu, self.nd, len(i_ym)):
            raise ValueError(f"DimensionMismatch: the estimator's (B, nx̂, nu, nd, nym) = {(est.B, est.nx̂, est.nu, est.nd, est.nym)}, "
                             f"the controller's {(self.B, self.nxh, self.nu, self.nd, len(i_ym))}")
        if len(i_ym) < 1 or i_ym.min() < 0 or i_ym.max() >= self.ny or len(set(i_ym.tolist())) != len(i_ym):
            raise ValueError("i_ym: unique indices of measured outputs in 0 .. ny-1")
        if direct is not None and bool(direct) != est.direct:
            raise ValueError(f"direct={direct} contradicts the estimator's direct={est.direct}: the form is the estimator's own")
        for name, mine, its in (("uop", self.uop, est.uop), ("yop[i_ym]", self.yop[:, i_ym], est.yop_m), ("dop", self.dop, est.dop),
                                ("x̂op", self.xhop, est.x̂op), ("f̂op", self.fhop, est.f̂op)):
            if not np.array_equal(mine, its):
                raise ValueError(f"the estimator's {name} must be the controller's")
        self.hd.mhe_attach(est.handle, i_ym)
        self.i_ym, self.mhe, self.direct, self.internal = i_ym, est, est.direct, False
        self.kf_timevarying = self.kf_steady = self.kf_luenberger = False
        return self

    def setestimator(self, Khat=None, i_ym=None, xhat0=None, *, covariances=None, steady=None, direct=None, mhe=None, internal=None,
                     luenberger=None):
        """Attach a SteadyKalmanFilter: Khat (B,nx̂,nym) steady-state gain (see
        `steady_kalman_gain`), i_ym measured-output indices (default all).  The estimate x̂0
        (deviation, (B,nx̂)) is then carried by this object like `mpc.estim.x̂0`.

        `covariances=dict(Qhat=…, Rhat=…, P0=…)` attaches the time-varying `KalmanFilter` instead (kalman.jl:1235-1290):
        Q̂ (nx̂,nx̂), R̂ (nym,nym), P̂_0 (nx̂,nx̂), each shared or with a leading batch axis.  P̂ and K̂(k) then live on the
        device and follow `preparestate` / `updatestate` (and `setmodel`: the recursion reads the current model).

        `steady=dict(Qhat=…, Rhat=…)` is the SteadyKalmanFilter as the reference constructs it, from Q̂ and R̂ (kalman.jl:205-222):
        the steady-state gain of every member is solved for on the device (R̂ positive definite, Q̂ positive semidefinite,
        max(nx̂, nym) <= 32; `getinfo()["kf_steady_path"]` tells which form of the iteration served a member), and `setmodel`
        solves again on the new model --
        which the reference's SteadyKalmanFilter refuses.  Members whose equation has no solution (an undetectable pair) or
        whose solve broke down keep a zero gain and are counted in one RuntimeWarning; `getinfo` shows `kf_status`.

        `direct=False` is the predictor form (kalman.jl:112): `preparestate` does nothing, `moveinput` works on x̂ₖ₋₁(k) and
        `updatestate(u, ym, d)` corrects and then predicts.  Khat is the FILTER-form gain in both forms (what
        `steady_kalman_gain` returns): the library applies x̂ <- Â (x̂ + K̂ v) + ... like `update_estimate!`.

        In both forms a member whose `ym` row holds a NaN, or every member when `ym` is None, skips the correction of that
        period (RuntimeWarning with the count); its prediction runs.

        `mhe=est` puts a `BatchMHE` behind the controller, `LinMPC(MovingHorizonEstimator(...))` of the manual: same batch, nx̂,
        nu, nd, library and operating points (uop, yop[i_ym], dop, x̂op), nym = len(i_ym); the form is `est.direct` (a `direct=`
        that contradicts it is an error).  `est` is borrowed and shared: `preparestate`, `updatestate`, `setstate` and
        `setmodel` (the rows i_ym of Ĉ and D̂d) forward to it, `mpc.xhat0` is `est.x̂0`, `moveinput(None, …)` reads it,
        `getinfo()["estim"]` is `est.getinfo()`, and `sim` / `hd.loop_device` run it on the device without a copy of x̂0.

        `internal=dict(stoch_ym=None | (As, Bs, Cs, Ds))` attaches the `InternalModel` (see `setinternalmodel`).

        `luenberger=dict(poles=None)` attaches the `Luenberger` observer (see `setluenberger`): the gain of every member is
        placed on the device from the observer poles."""
        if ((Khat is not None) + (covariances is not None) + (steady is not None) + (mhe is not None) + (internal is not None)
                + (luenberger is not None)) > 1:
            raise ValueError("give one of Khat (SteadyKalmanFilter), steady (SteadyKalmanFilter from Q̂ and R̂), covariances (KalmanFilter), "
                             "mhe (MovingHorizonEstimator), internal (InternalModel) or luenberger (Luenberger)")
        if internal is not None:
            if direct is not None and not direct:
                raise ValueError("direct=False: the InternalModel is always in the filter form")
            return self.setinternalmodel(**internal, i_ym=i_ym, xhat0=xhat0)
        self.internal = False
        if mhe is not None:
            if xhat0 is not None:
                raise ValueError("xhat0: the estimate is the MovingHorizonEstimator's own (est.setstate)")
            return self._attach_mhe(mhe, i_ym, direct)
        direct = True if direct is None else direct
        if covariances is not None:
            return self.setkalmanfilter(**covariances, i_ym=i_ym, xhat0=xhat0, direct=direct)
        if steady is not None:
            return self.setsteadykalmanfilter(**steady, i_ym=i_ym, xhat0=xhat0, direct=direct)
        if luenberger is not None:
            return self.setluenberger(**luenberger, i_ym=i_ym, xhat0=xhat0, direct=direct)
        if Khat is None:
            raise ValueError("setestimator needs Khat, steady, covariances, luenberger or mhe")
        self.__dict__.pop("mhe", None)              # (mpcqp_kf_set detaches a MovingHorizonEstimator)
        self.kf_timevarying = self.kf_steady = self.kf_luenberger = False
        self.i_ym = np.arange(self.ny) if i_ym is None else np.asarray(i_ym, int)
        Khat = np.asarray(Khat, float)
        if Khat.shape != (self.B, self.nxh, len(self.i_ym)):
            raise ValueError("Khat size must be (B, nx̂, nym)")
        self._set_direct(direct)
        self.hd.kf_set(colmajor(Khat), self.i_ym)
        self.xhat0 = np.zeros((self.B, self.nxh)) if xhat0 is None else _f64(np.broadcast_to(xhat0, (self.B, self.nxh))).copy()
        return self

    def setinternalmodel(self, stoch_ym=None, i_ym=None, xhat0=None):
        """The `InternalModel` estimator (src/estimator/internal_model.jl): the state is the model's own (no augmentation, so
        nx̂ = nx), and the mismatch between the measurements and the model's outputs drives a stochastic model on the
        measured outputs, `stoch_ym=(As, Bs, Cs, Ds)` -- (nxs,nxs), (nxs,nym), (nym,nxs), (nym,nym), each shared or with a
        leading batch axis; None: the identity in all four, one integrator-free pass-through per measured output, the
        reference's default.  Its prediction Ŷs over the horizon is added to the controller's free response on the device:
        `preparestate` computes ŷs and Ŷs, every `moveinput` that follows uses them in the objective and in the output bounds,
        `updatestate` advances x̂d = x̂0 and x̂s.  `evaloutput`, `getinfo()["Ŷs"]` and `getinfo()["ŷ"]` include them.
        Like the reference's constructor this raises ValueError for a model with an eigenvalue on or outside the unit circle,
        for a `Ds` that is zero and for `Cs` / `Ds` whose row count is not nym.  Members whose `Ds` is singular are counted in
        one RuntimeWarning; their stochastic part stays off (`getinfo()["im_status"]` 2).  Not available with custom linear
        constraints, MultipleShooting or on `BatchExplicitMPC` (include/mpcqp.h)."""
        B = self.B
        i_ym = np.arange(self.ny) if i_ym is None else np.asarray(i_ym, int)
        nym = len(i_ym)
        if nym < 1 or i_ym.min() < 0 or i_ym.max() >= self.ny or len(set(i_ym.tolist())) != nym:
            raise ValueError("i_ym: unique indices of measured outputs in 0 .. ny-1")
        if np.any(np.abs(np.linalg.eigvals(self._Ahat)) >= 1.0):
            raise ValueError("InternalModel does not support integrating or unstable model")
        stoch = None
        if stoch_ym is not None:
            mats = [np.asarray(a, float) for a in stoch_ym]
            if len(mats) != 4 or any(a.ndim not in (2, 3) for a in mats):
                raise ValueError("stoch_ym: (As, Bs, Cs, Ds)")
            mats = [np.broadcast_to(a, (B,) + a.shape[-2:]) for a in mats]
            As, Bs, Cs, Ds = mats
            nxs = As.shape[-1]
            if Cs.shape[1] != nym or Ds.shape[1] != nym:
                raise ValueError(f"Stochastic model output quantity ({Cs.shape[1]}) is different from measured output quantity ({nym})")
            if nxs < 1 or As.shape != (B, nxs, nxs) or Bs.shape != (B, nxs, nym) or Cs.shape != (B, nym, nxs) or Ds.shape != (B, nym, nym):
                raise ValueError("DimensionMismatch between As, Bs, Cs, Ds")
            if np.any(np.all(Ds == 0, axis=(1, 2))):
                raise ValueError("Stochastic model requires a nonzero direct transmission matrix D")
            stoch = [colmajor(a) for a in mats]
        self.hd.im_set(stoch, i_ym)
        self.__dict__.pop("mhe", None)
        self.i_ym, self.internal, self.direct, self._hd_direct = i_ym, True, True, True      # (mpcqp_im_set puts the handle in the filter form)
        self.kf_timevarying = self.kf_steady = self.kf_luenberger = False
        self.xhat0 = np.zeros((B, self.nxh)) if xhat0 is None else _f64(np.broadcast_to(xhat0, (B, self.nxh))).copy()
        n = int(np.count_nonzero(self.hd.im_status()))
        if n:
            warnings.warn(f"InternalModel: Ds is singular, the stochastic part of the estimator is off ({n} of {B} estimators)", RuntimeWarning)
        return self

    def evaloutput(self, d=None):
        """`evaloutput(estim, d)`: ŷ = Ĉ x̂0 + D̂d d0 + yop, + ŷs of the last `preparestate` behind an InternalModel."""
        if not hasattr(self, "i_ym"):
            raise ValueError("no estimator attached (setestimator)")
        y = np.einsum("bij,bj->bi", self._Chat, self.xhat0) + self.yop
        if self.nd > 0:
            y = y + np.einsum("bij,bj->bi", self._Dhd, self._bc(d, self.nd, "d") - self.dop)
        if getattr(self, "internal", False):
            y = y + self.hd.get(GET_IM_YS)
        return y

    def _set_direct(self, direct):
        """The form of the estimator about to be attached, settled before the estimator itself goes to the device.  The
        handle's flag (default: filter form) survives its setters, so it is told about a change only.  A handle without
        mpcqp_kf_set_direct cannot run the predictor form: NotImplementedError, and nothing has been sent to it."""
        direct = bool(direct)
        if direct != getattr(self, "_hd_direct", True):
            if not hasattr(self.hd, "kf_set_direct"):
                raise NotImplementedError("direct=False (predictor form): this handle has no mpcqp_kf_set_direct")
            self.hd.kf_set_direct(direct)
            self._hd_direct = direct
        self.direct = direct

    def _cov(self, M, n, name):
        a = np.asarray(M, float)
        if a.shape == (n, n):
            a = np.broadcast_to(a, (self.B, n, n))
        if a.shape != (self.B, n, n):
            raise ValueError(f"{name} size must be ({n}, {n})")
        if not np.allclose(a, a.transpose(0, 2, 1), rtol=0.0, atol=1e-12 * max(float(np.abs(a).max()), 0.0)):
            raise ValueError(f"{name} must be Hermitian")                # (the reference's Hermitian{NT} fields)
        return a

    def setkalmanfilter(self, Qhat, Rhat, P0, i_ym=None, xhat0=None, direct=True):
        """The time-varying `KalmanFilter` (see `setestimator(covariances=…)`); keyword names are the reference's Q̂, R̂, P̂_0."""
        self.i_ym = np.arange(self.ny) if i_ym is None else np.asarray(i_ym, int)
        nym = len(self.i_ym)
        Qhat, Rhat, P0 = self._cov(Qhat, self.nxh, "Q̂"), self._cov(Rhat, nym, "R̂"), self._cov(P0, self.nxh, "P̂_0")
        self._set_direct(direct)
        self.hd.kf_set_covariances(Qhat, Rhat, P0, self.i_ym)
        self.__dict__.pop("mhe", None)
        self.internal = False
        self._P0 = P0.copy()                        # P̂_0, for initstate (init_estimate_cov!)
        self.kf_timevarying, self.kf_steady, self.kf_luenberger = True, False, False
        self.xhat0 = np.zeros((self.B, self.nxh)) if xhat0 is None else _f64(np.broadcast_to(xhat0, (self.B, self.nxh))).copy()
        return self

    def setsteadykalmanfilter(self, Qhat, Rhat, i_ym=None, xhat0=None, direct=True):
        """The `SteadyKalmanFilter` from Q̂ and R̂ (see `setestimator(steady=…)`)."""
        if not hasattr(self.hd, "kf_set_steady"):
            raise NotImplementedError("steady=dict(Qhat, Rhat): this handle has no mpcqp_kf_set_steady")
        self.i_ym = np.arange(self.ny) if i_ym is None else np.asarray(i_ym, int)
        Qhat, Rhat = self._cov(Qhat, self.nxh, "Q̂"), self._cov(Rhat, len(self.i_ym), "R̂")
        self._set_direct(direct)
        self.hd.kf_set_steady(Qhat, Rhat, self.i_ym)
        self.__dict__.pop("mhe", None)
        self.internal = False
        self.kf_timevarying, self.kf_steady, self.kf_luenberger = False, True, False
        self._warn_steady()
        self.xhat0 = np.zeros((self.B, self.nxh)) if xhat0 is None else _f64(np.broadcast_to(xhat0, (self.B, self.nxh))).copy()
        return self

    def setluenberger(self, poles=None, i_ym=None, xhat0=None, direct=True):
        """The `Luenberger` observer (src/estimator/luenberger.jl): `poles` are the nx̂ observer poles, (nx̂,) shared or (B,nx̂),
        real and inside the unit circle (default: the reference's `1e-3*(1:nx̂) .+ 0.5`).  The gain of every member is placed
        on the device (robust placement of Kautsky, Nichols and Van Dooren; max(nx̂, nym) <= 32; a pole may be repeated up to
        nym times): the eigenvalues of Â (I - K̂ Ĉm) are the poles in both forms of `direct`.  From then on the estimator runs
        like one with a given steady gain, and `setmodel` places again on the new model -- which the reference's Luenberger
        refuses.  Members whose placement broke down (an unobservable mode, a singular Â without a pole at 0, ...) keep the
        previous gain (or zero) and are counted in one RuntimeWarning; `getinfo` shows `K̂`, `kf_status` and `place_sweeps`.
        Deviations from the reference: complex poles are not implemented, and the placement works on the measured rows Ĉm
        (the reference places on all of Ĉ and drops the unmeasured columns, which agrees when every output is measured)."""
        i_ym = np.arange(self.ny) if i_ym is None else np.asarray(i_ym, int)
        if len(i_ym) < 1 or i_ym.min() < 0 or i_ym.max() >= self.ny or len(set(i_ym.tolist())) != len(i_ym):
            raise ValueError("i_ym: unique indices of measured outputs in 0 .. ny-1")
        p = 1e-3 * np.arange(1, self.nxh + 1) + 0.5 if poles is None else np.asarray(poles)
        if np.iscomplexobj(p):
            if np.any(p.imag != 0):
                raise NotImplementedError("complex observer poles are not implemented: real poles only")
            p = p.real
        p = np.asarray(p, float)
        if p.ndim not in (1, 2) or p.shape[-1] != self.nxh or (p.ndim == 2 and p.shape[0] != self.B):
            raise ValueError(f"poles length ({p.shape[-1] if p.ndim else 0}) ≠ nx̂ ({self.nxh})")
        if not np.all(np.abs(p) < 1.0):
            raise ValueError("Observer poles should be inside the unit circles.")
        if not hasattr(self.hd, "kf_set_poles"):
            raise NotImplementedError("luenberger=dict(poles): this handle has no mpcqp_kf_set_poles")
        p = _f64(np.broadcast_to(p, (self.B, self.nxh)))
        self._set_direct(direct)
        self.hd.kf_set_poles(p, i_ym)
        self.i_ym = i_ym
        self.__dict__.pop("mhe", None)
        self.internal = False
        self.kf_timevarying, self.kf_steady, self.kf_luenberger = False, False, True
        self._warn_luenberger()
        self.xhat0 = np.zeros((self.B, self.nxh)) if xhat0 is None else _f64(np.broadcast_to(xhat0, (self.B, self.nxh))).copy()
        return self

    def _warn_luenberger(self):
        """One warning for the members whose poles could not be placed (luenberger.jl:38-42)."""
        n = int(np.count_nonzero(self.hd.kf_status()))
        if n:
            warnings.warn(f"Cannot compute the Luenberger gain K̂ with specified poles. ({n} of {self.B} estimators)", RuntimeWarning)

    def _warn_steady(self):
        """One warning for the members whose steady-state gain could not be computed (kalman.jl:211-221)."""
        n = int(np.count_nonzero(self.hd.kf_status()))
        if n:
            warnings.warn("Cannot compute the optimal Kalman gain K̂ for the SteadyKalmanFilter: the pair is not detectable or "
                          f"the solve broke down, the previous gain (or zero) stays ({n} of {self.B} estimators)", RuntimeWarning)

    def setcovariances(self, Qhat, Rhat):
        """The Q̂, R̂ keywords of `setmodel!`: new noise covariances.  KalmanFilter: P̂ and x̂0 stay.  SteadyKalmanFilter from Q̂
        and R̂ (`setestimator(steady=…)`): the gain is solved for again."""
        if getattr(self, "kf_steady", False):
            self.hd.kf_set_steady(self._cov(Qhat, self.nxh, "Q̂"), self._cov(Rhat, len(self.i_ym), "R̂"), self.i_ym)
            return self._warn_steady()
        if not getattr(self, "kf_timevarying", False):
            raise ValueError("Q̂ and R̂ can only be replaced on a KalmanFilter (setestimator(covariances=…)) or a "
                             "SteadyKalmanFilter built from them (setestimator(steady=…))")
        self.hd.kf_set_covariances(self._cov(Qhat, self.nxh, "Q̂"), self._cov(Rhat, len(self.i_ym), "R̂"), None, self.i_ym)

    def setstate(self, xhat, Phat=None):
        """`setstate!(estim, x̂, P̂)` (src/estimator/execute.jl): x̂ (nx̂,) or (B,nx̂) in engineering units; P̂ only on a
        time-varying KalmanFilter."""
        if not hasattr(self, "i_ym"):
            raise ValueError("no estimator attached (setestimator)")
        if getattr(self, "mhe", None) is not None:      # (a covariance raises there, as in the reference)
            self.mhe.setstate(self._bc(xhat, self.nxh, "x̂"), Phat)
            return self
        if Phat is not None:
            if getattr(self, "kf_luenberger", False):
                raise ValueError("Luenberger does not compute an estimation covariance matrix P̂.")
            if not getattr(self, "kf_timevarying", False):
                raise ValueError("the SteadyKalmanFilter has no covariance estimate P̂ to set")
            self.hd.kf_set_state_covariance(self._cov(Phat, self.nxh, "P̂"))
        self.xhat0 = _f64(self._bc(xhat, self.nxh, "x̂") - self.xhop).copy()
        return self

    def _y0m(self, ym):
        """y0m of a period, or None for `ym = nothing`; warns once when members miss the correction (kalman.jl:245-251)."""
        y0m = None if ym is None else self._bc(ym, len(self.i_ym), "ym") - self.yop[:, self.i_ym]
        n = self.B if y0m is None else int(np.isnan(y0m).any(axis=1).sum())
        if n:
            warnings.warn("NaN values in the Kalman filter measurements ym: skipping correction step "
                          f"({n} of {self.B} estimators)", RuntimeWarning)
        return y0m

    def preparestate(self, ym, d=None):
        """`preparestate!` (src/estimator/execute.jl:334-345 -> correct_estimate_obsv!,
        kalman.jl:284-295): x̂0 += K̂ (y0m - Ĉm x̂0 - D̂dm d0).  Returns x̂ = x̂0 + x̂op.  Members with a NaN in `ym` (all of
        them with ym=None) keep their x̂0.  Predictor form (direct=False): nothing to do, no device call."""
        if getattr(self, "mhe", None) is not None:      # preparestate!(estim::MovingHorizonEstimator): one solve (direct form)
            return self._mhe_period(self.mhe.preparestate(ym, d), self.direct)
        if getattr(self, "internal", False):            # correct_estimate!(estim::InternalModel): ŷs and Ŷs, x̂0 stays
            y0m = self._bc(ym, len(self.i_ym), "ym") - self.yop[:, self.i_ym]
            n = int((~np.isfinite(y0m)).any(axis=1).sum())
            if n:
                warnings.warn(f"NaN values in the internal model measurements ym: assigning them ŷs=0 ({n} of {self.B} estimators)",
                              RuntimeWarning)
            self.hd.im_correct(self.xhat0, y0m, None if self.nd == 0 else self._bc(d, self.nd, "d") - self.dop)
            return self.xhat0 + self.xhop
        if not getattr(self, "direct", True):
            return self.xhat0 + self.xhop
        y0m = self._y0m(ym)
        d0 = None if self.nd == 0 else self._bc(d, self.nd, "d") - self.dop
        self.hd.kf_correct(self.xhat0, y0m, d0)       # (y0m None: a time-varying filter records the miss, status 1)
        return self.xhat0 + self.xhop

    def updatestate(self, u, ym=None, d=None):
        """`updatestate!` (src/estimator/execute.jl:374-386 -> predict_estimate_obsv!,
        kalman.jl:298-309): x̂0 <- Â x̂0 + B̂u u0 + B̂d d0 + f̂op - x̂op.  Predictor form (direct=False): the correction with
        `ym` first (kalman.jl:276-281, 520-525; ym=None or NaN rows: skipped), then the prediction."""
        if getattr(self, "mhe", None) is not None:
            if ym is None:
                raise ValueError("updatestate: the MovingHorizonEstimator needs ym")
            return self._mhe_period(self.mhe.updatestate(u, ym, d), not self.direct)
        u0 = self._bc(u, self.nu, "u") - self.uop
        d0 = None if self.nd == 0 else self._bc(d, self.nd, "d") - self.dop
        if getattr(self, "internal", False):
            self.hd.im_update(self.xhat0, u0, d0)
        elif getattr(self, "direct", True):
            self.hd.kf_predict(self.xhat0, u0, d0)
        else:
            self.hd.kf_update(self.xhat0, u0, self._y0m(ym), d0)
        return self.xhat0 + self.xhop

    def _mhe_period(self, xhat, solved):
        """One warning for the members whose MovingHorizonEstimator solve of this call failed (mhe/execute.jl:596-606)."""
        if solved:
            self._warn_mhe(self.mhe.status, self.B, "estimators")
        return xhat

    @staticmethod
    def _warn_mhe(status, total, what):
        nerr, nwarn = int(np.sum(status == 2)), int(np.sum(status == 1))
        if nerr:      # @error branch, src/estimator/mhe/execute.jl:596-600
            warnings.warn(f"MHE terminated without solution: estimation in open-loop ({nerr} of {total} {what})", RuntimeWarning)
        if nwarn:     # @warn branch, :602-606
            warnings.warn("MHE termination status not OPTIMAL or LOCALLY_SOLVED: keeping solution anyway "
                          f"({nwarn} of {total} {what})", RuntimeWarning)

    # -- per-step ---------------------------------------------------------------------------
    def initstate(self, u, ym=None, d=None):
        """`initstate!(mpc, u, ym, d)` (src/controller/execute.jl:9-13).  With `ym=None` the controller part only: Z̃ = 0,
        lastu0 = u - uop.  With `ym` (nym,) / (B,nym) also the estimator half (src/estimator/execute.jl:208-259): every member's
        x̂0 becomes the least-squares solution of  [I - Â; Ĉm] x̂0 = [B̂u u0 + B̂d d0 + f̂op - x̂op; y0m - D̂dm d0]  -- the steady
        state with ŷm = ym, a bumpless transfer -- solved on the device (QR, one member per wavefront), then
        `init_estimate_cov!`: P̂ <- P̂_0 on a time-varying KalmanFilter, `est.initstate(x̂, u, d)` on a MovingHorizonEstimator
        (windows emptied, P̄ <- P̂_0), nothing on a steady filter.  Members whose matrix has no full column rank (an integrating
        plant with an integrator on the same channel) keep their x̂0 -- the reference returns the minimum-norm solution there --
        and are counted in one RuntimeWarning.  Returns x̂ (B,nx̂) when `ym` is given."""
        self.Z[:] = 0.0
        self.lastu0 = np.broadcast_to(np.asarray(u, float), (self.B, self.nu)) - self.uop
        if ym is None:
            return None
        if not hasattr(self, "i_ym"):
            raise ValueError("no estimator attached (setestimator)")
        y0m = self._bc(ym, len(self.i_ym), "ym") - self.yop[:, self.i_ym]
        d0 = None if self.nd == 0 else self._bc(d, self.nd, "d") - self.dop
        xh = _f64(self.xhat0).copy()
        st = self.hd.est_initstate(xh, self.lastu0, y0m, d0)
        est = getattr(self, "mhe", None)
        if est is not None:
            est.initstate(xh + self.xhop, self.lastu0 + self.uop, None if self.nd == 0 else d0 + self.dop)
        else:
            self.xhat0 = xh
            if getattr(self, "kf_timevarying", False):
                self.hd.kf_set_state_covariance(self._P0)
        self.init_status = st
        n = int(np.count_nonzero(st))
        if n:
            warnings.warn(("initstate!: I - Â or I - Âs is singular, x̂0 and x̂s are left unchanged " if getattr(self, "internal", False) else
                           "initstate!: [I - Â; Ĉm] has no full column rank, the estimate x̂0 is left unchanged ")
                          + 
                          f"({n} of {self.B} estimators)", RuntimeWarning)
        return self.xhat0 + self.xhop

    def _prepare_kernel(self):
        """The kernel the steps of this controller run on, built or loaded once per constraint pattern."""
        self._ms_kernel = False
        if self.transcription == "MultipleShooting":
            self.hd.set_transcription(MULTIPLE_SHOOTING)
            why = self.hd.transcription_supported()
            if why:
                self.hd.set_transcription(SINGLE_SHOOTING)
                warnings.warn("mpcqp: MultipleShooting kernel not available for this controller (reason mask "
                              f"{why}: 1 weights that couple stages, 4 LDS): the SingleShooting "
                              "kernels solve the same problem", RuntimeWarning)
            else:
                self._ms_kernel = True
        self.kernel = KERNEL_MS if self._ms_kernel else self.hd.prepare()
        if self.kernel == KERNEL_MS and not self._ms_kernel and self.nZ <= 256 and self.hd.lds_bytes() > 160 * 1024:
            # (the reroute used to be silent -- the condensed problem does not fit the LDS of a CU in the
            #  carve-up of the runtime-dimension kernel; same QP, solved in stage form, an order of magnitude slower)
            warnings.warn(f"mpcqp: the condensed problem (nZ̃ = {self.nZ}, {self.hd.lds_bytes()} B of LDS) does not fit one "
                          "compute unit: the SingleShooting controller's steps run on the stage-structured "
                          "(MultipleShooting) kernel", RuntimeWarning)
        self._ms_kernel = self.kernel == KERNEL_MS       # (also: nZ̃ > 256, which only the stage-structured kernel takes)
        self._prepared = True

    def moveinput(self, xhat0, ry=None, d=None, *, lastu=None, Dhat=None, Rhaty=None, Rhatu=None,
                  want_info=False):
        """`moveinput!` for the whole batch (src/controller/execute.jl:59-80).

        xhat0 (B,nx̂) is `estim.x̂0` (deviation); ry (B,ny)/(ny,), d (B,nd), `lastu`, `Rhaty`
        (B,ny*Hp), `Rhatu` (B,nu*Hp), `Dhat` (B,nd*Hp) are engineering values like the reference.
        Returns u (B,nu)."""
        B = self.B
        xhat0, ry, held, Rhaty, Rhatu, lastu0, d0, Dh0 = self._period_args(xhat0, ry, d, lastu, Dhat, Rhaty, Rhatu)
        if self.nw > 0 and not held:               # r̂e(k) = ry(k) for the Wr term (execute.jl:351)
            self.hd.set_current_setpoint(ry - self.yop)
        if not self._prepared:                     # like JuMP's model build: before the loop, not in mpcqp_step
            self._prepare_kernel()
        out = self.hd.step(xhat0, lastu0, (ry - self.yop) if held else (Rhaty - self.Yop), self.Z,
                           Ru=None if Rhatu is None else Rhatu - self.Uop, d0=d0, Dhat0=Dh0,
                           want_Yhat=want_info)
        u0, self.status, self.iters = out[0], out[1], out[2]
        self._Yhat0 = out[3] if want_info else None
        self._period_record(xhat0, ry, held, Rhaty, Rhatu, lastu0, d0, Dh0)
        nerr = int(np.sum(self.status == STATUS_ERROR))
        nwarn = int(np.sum(self.status == STATUS_ITERATION_LIMIT))
        if nerr:      # @error branch, src/controller/execute.jl:484-489
            warnings.warn(f"MPC terminated without solution: returning last solution shifted "
                          f"({nerr} of {B} controllers)", RuntimeWarning)
        if nwarn:     # @warn branch, :491-496
            warnings.warn(f"MPC termination status not OPTIMAL: keeping solution anyway "
                          f"({nwarn} of {B} controllers)", RuntimeWarning)
        self.lastu0 = u0.copy()                       # getinput!: lastu0 <- u - uop
        return u0 + self.uop

    __call__ = moveinput

    # -- sim!: N closed-loop periods of the whole batch, the plant on the device -------------------------------------------
    def _sim_prepare(self):
        if not self._prepared:
            self._prepare_kernel()

    def _sim_plant(self, plant):
        """`plant` of `sim`: (A, Bu, C[, Bd, Dd]) or a dict of them with optional uop / yop / dop (which have to be the
        controller's) and xop / fop (the plant's own).  Sends the plant to the handle; returns nxp and the plant's xop (B,nxp)."""
        B, nu, ny, nd = self.B, self.nu, self.ny, self.nd
        if plant is None:
            raise ValueError("sim needs plant=(A, Bu, C[, Bd, Dd]): the controller holds the augmented model only")
        if isinstance(plant, dict):
            p = dict(plant)
        else:
            p = dict(zip(("A", "Bu", "C", "Bd", "Dd"), plant))
        unknown = set(p) - {"A", "Bu", "C", "Bd", "Dd", "uop", "yop", "dop", "xop", "fop"}
        if unknown or any(k not in p for k in ("A", "Bu", "C")):
            raise ValueError(f"plant needs A, Bu, C and takes Bd, Dd, uop, yop, dop, xop, fop (got {sorted(p)})")

        def mat(k, rows, cols):
            a = p.get(k)
            if a is None:
                return None
            a = np.asarray(a, float)
            if a.ndim == 2:
                a = np.broadcast_to(a, (B,) + a.shape)
            if a.shape != (B, rows, cols):
                raise ValueError(f"plant {k} size must be ({rows}, {cols})")       # DimensionMismatch
            return a
        A0 = np.asarray(p["A"], float)
        if A0.ndim not in (2, 3) or A0.shape[-1] != A0.shape[-2]:
            raise ValueError("plant A must be square")
        nxp = A0.shape[-1]
        A, Bu, Cm = mat("A", nxp, nxp), mat("Bu", nxp, nu), mat("C", ny, nxp)
        Bd, Dd = mat("Bd", nxp, nd), mat("Dd", ny, nd)
        if nd == 0:
            Bd = Dd = None
        for k, mine in (("uop", self.uop), ("yop", self.yop), ("dop", self.dop)):
            if p.get(k) is not None and not np.array_equal(np.broadcast_to(np.asarray(p[k], float), mine.shape), mine):
                raise ValueError(f"the plant's {k} must be the controller's")
        vec = lambda k: np.zeros((B, nxp)) if p.get(k) is None else np.broadcast_to(np.asarray(p[k], float), (B, nxp)).copy()
        xop, fop = vec("xop"), vec("fop")
        fx = fop - xop
        self.hd.sim_set_plant(colmajor(A), colmajor(Bu), colmajor(Cm), None if Bd is None else colmajor(Bd),
                              None if Dd is None else colmajor(Dd), fx if np.any(fx != 0) else None)
        return nxp, xop

    def sim(self, N, ry=None, d=None, ru=None, *, plant=None, u_step=None, u_noise=None, y_step=None, y_noise=None,
            d_step=None, d_noise=None, x_noise=None, x_0=None, xhat_0=None, lastu=None, seed=None, draws=None, fuse=True,
            initstate=False):
        """`sim!(mpc, N, ry, d, ru; plant, u_step, u_noise, y_step, y_noise, d_step, d_noise, x_noise, x_0, x̂_0, lastu)`
        (src/plot_sim.jl:241-319) for every controller of the batch: N periods of preparestate / moveinput / updatestate
        around a plant that runs on the device, without a host synchronisation between the periods.  Returns a `SimResult`.

        Arguments are engineering values.  ry (ny,) / (B,ny) is held over the run, (B,ny,N) gives one per period (default
        yop + 1); d (nd,) / (B,nd) (default dop); ru (nu,) / (B,nu) the input set point, held (default uop).  Steps and noise
        standard deviations are (n,) / (B,n).  `plant`: see `_sim_plant`; it shares the controller's uop, yop and dop.
        x_0 (nxp,) / (B,nxp): the plant state; None continues from the end of the previous `sim` (the plant's xop at first).
        xhat_0: the estimate; None continues from the attached estimator's state.  `initstate=True` does what
        `sim_closedloop!` does first (src/plot_sim.jl:289-290): `initstate(lastu, lasty[i_ym], lastd)` with `lasty` the plant's
        output at x_0 and d (no step, no noise), then `setstate` when `xhat_0` is given; the default leaves the estimator as it
        is.  With a MovingHorizonEstimator attached (`setestimator(mhe=…)`) every period runs the estimator's solve on the
        device, `SimResult.est_status` holds its status per period, failed solves are counted in one warning per run, and a NaN
        in a measurement is passed to the estimator unchanged (missed measurements are a Kalman-filter feature of the
        reference, kalman.jl:245-251).  lastu: None continues from `self.lastu0`.  Afterwards `self.xhat0`, `self.lastu0`, `self.Z` and `self.status` are
        those of the last period, so `preparestate` / `moveinput` / `updatestate` can go on from there.

        The noise of period i is σ∘w[:, :, i] with standard-normal draws w: `draws=dict(w_d=…, w_y=…, w_u=…, w_x=…)`, each
        (B,n,N) with n = nd, ny, nu, nxp, or -- for the channels not given -- `numpy.random.default_rng(seed)` drawing
        standard_normal((B,n,N)) in the order w_d, w_y, w_u, w_x (all four are drawn, whatever noise is asked for).
        `fuse=False` keeps the run on the per-period launches; otherwise an explicit-law controller with a steady gain and
        dimensions up to 16, `ry` held and no `ru`, runs the whole loop in one launch (`SimResult.path`: api.SIM_PATH_FUSED)."""
        B, nu, ny, nd = self.B, self.nu, self.ny, self.nd
        N = int(N)
        if N < 1:
            raise ValueError("N should be ≥ 1")
        if not hasattr(self, "i_ym"):
            raise ValueError("no estimator attached (setestimator)")
        if not hasattr(self.hd.lib, "mpcqp_sim"):
            raise NotImplementedError("sim: this library has no mpcqp_sim")
        nxp, xop = self._sim_plant(plant)
        flags = 0 if fuse else SIM_FLAG_NO_FUSE
        ry = self.yop + 1.0 if ry is None else np.asarray(ry, float)
        if ry.shape == (B, ny, N):
            flags |= SIM_FLAG_RY_PER_PERIOD
            Ry_data = ry.copy()
            ry0 = _f64((ry - self.yop[:, :, None]).transpose(0, 2, 1))
        else:
            ry = self._bc(ry, ny, "ry")
            Ry_data = np.repeat(ry[:, :, None], N, axis=2)
            ry0 = ry - self.yop
        d0 = None
        if nd > 0:
            d0 = self._bc(self.dop if d is None else d, nd, "d") - self.dop
        elif d is not None and np.size(d) != 0:
            raise ValueError("d size must be (0,)")
        Ru0 = None
        Ru_data = np.repeat(self.uop[:, :, None], N, axis=2)
        if ru is not None:
            ru = self._bc(ru, nu, "ru")
            Ru_data = np.repeat(ru[:, :, None], N, axis=2)
            Ru0 = np.tile(ru - self.uop, self.Hp)
        opt = lambda v, n, name: None if v is None or n == 0 else _f64(self._bc(v, n, name))
        steps = dict(u_step=opt(u_step, nu, "u_step"), y_step=opt(y_step, ny, "y_step"), d_step=opt(d_step, nd, "d_step"))
        sig = dict(sigma_u=opt(u_noise, nu, "u_noise"), sigma_y=opt(y_noise, ny, "y_noise"), sigma_d=opt(d_noise, nd, "d_noise"),
                   sigma_x=opt(x_noise, nxp, "x_noise"))
        rng = np.random.default_rng(seed)
        given = dict(draws or {})
        if set(given) - {"w_d", "w_y", "w_u", "w_x"}:
            raise ValueError("draws takes w_d, w_y, w_u, w_x")
        w = {}
        for k, n in (("w_d", nd), ("w_y", ny), ("w_u", nu), ("w_x", nxp)):
            drawn = rng.standard_normal((B, n, N))
            a = drawn if given.get(k) is None else np.asarray(given[k], float)
            if a.shape != (B, n, N):
                raise ValueError(f"draws[{k!r}] size must be ({B}, {n}, {N})")
            w[k] = _f64(a.transpose(0, 2, 1)) if sig["sigma_" + k[2]] is not None else None
        if x_0 is not None:
            x0 = _f64(self._bc(x_0, nxp, "x_0") - xop).copy()
        elif getattr(self, "sim_x0", None) is not None and self.sim_x0.shape == (B, nxp):
            x0 = self.sim_x0.copy()
        else:
            x0 = np.zeros((B, nxp))
        lu = _f64(self.lastu0).copy() if lastu is None else _f64(self._bc(lastu, nu, "lastu") - self.uop).copy()
        if initstate:         # sim_closedloop!: initstate!(est_mpc, lastu, lasty[i_ym], lastd), then setstate! (plot_sim.jl:289-290)
            p = plant if isinstance(plant, dict) else dict(zip(("A", "Bu", "C", "Bd", "Dd"), plant))
            bcm = lambda a: np.broadcast_to(np.asarray(a, float), (B,) + np.shape(a)[-2:])
            lasty0 = np.einsum("bij,bj->bi", bcm(p["C"]), x0)
            if nd > 0 and p.get("Dd") is not None:
                lasty0 = lasty0 + np.einsum("bij,bj->bi", bcm(p["Dd"]), d0)
            self.initstate(lu + self.uop, (lasty0 + self.yop)[:, self.i_ym], None if nd == 0 else d0 + self.dop)
            if xhat_0 is not None:
                self.setstate(self._bc(xhat_0, self.nxh, "x̂_0"))
            xh = _f64(self.xhat0).copy()
        else:
            xh = self.xhat0.copy() if xhat_0 is None else _f64(self._bc(xhat_0, self.nxh, "x̂_0") - self.xhop).copy()
        self._sim_prepare()
        # the single-launch path (include/mpcqp.h: MPCQP_SIM_PATH_FUSED) computes u alone: self.Z is NaN after such a run, as
        # after moveinput(..., want_Z=False)
        fused = fuse and Ru0 is None and not (flags & SIM_FLAG_RY_PER_PERIOD) and self.hd.sim_path() == SIM_PATH_FUSED
        Z = None if fused else _f64(self.Z).copy()
        rec = {k: np.empty((B, N, n)) for k, n in (("Y", ny), ("X", nxp), ("D", nd), ("Xhat", self.nxh), ("Yhat", ny), ("U", nu), ("Ud", nu))}
        status = np.empty((B, N), np.int32)
        self.hd.sim(N, flags, ry=ry0, Ru=Ru0, d=d0, **steps, **sig, **w, x0=x0, xhat0=xh, lastu0=lu, Ztilde=Z, status=status,
                    **{k: (v if v.size else None) for k, v in rec.items()})
        est = getattr(self, "mhe", None)
        est_status = None
        if est is not None:       # the estimator's device state went on with the run; its host mirror follows
            from .mhe import GET_STATUS
            est.x̂0, est.status = xh, est.handle.get(GET_STATUS)
            est_status = self.hd.sim_est_status(N).T.copy()
            self.sim_x0, self.lastu0 = x0, lu
        else:
            self.sim_x0, self.xhat0, self.lastu0 = x0, xh, lu
        self.Z = np.full((B, self.nZ), np.nan) if fused else Z
        self.status = status[:, -1].copy()
        self.iters = np.zeros(B, np.int32)
        nerr, nwarn = int(np.sum(status == STATUS_ERROR)), int(np.sum(status == STATUS_ITERATION_LIMIT))
        if nerr:      # @error branch, src/controller/execute.jl:484-489: once per run
            warnings.warn(f"MPC terminated without solution: returning last solution shifted "
                          f"({nerr} of {B * N} controller periods)", RuntimeWarning)
        if nwarn:     # @warn branch, :491-496
            warnings.warn(f"MPC termination status not OPTIMAL: keeping solution anyway "
                          f"({nwarn} of {B * N} controller periods)", RuntimeWarning)
        if est is not None:
            self._warn_mhe(est_status, B * N, "estimator periods")
        nmiss = 0 if est is not None else int(np.isnan(rec["Y"][:, :, self.i_ym]).any(axis=2).sum())
        if nmiss and getattr(self, "internal", False):
            warnings.warn(f"NaN values in the internal model measurements ym: assigning them ŷs=0 ({nmiss} of {B * N} estimator periods)",
                          RuntimeWarning)
        elif nmiss:   # kalman.jl:245-251
            warnings.warn("NaN values in the Kalman filter measurements ym: skipping correction step "
                          f"({nmiss} of {B * N} estimator periods)", RuntimeWarning)
        t = lambda k, op: rec[k].transpose(0, 2, 1) + op[:, :, None]
        return SimResult(N=N, Y_data=t("Y", self.yop), Ry_data=Ry_data, Ŷ_data=t("Yhat", self.yop), U_data=t("U", self.uop),
                         Ud_data=t("Ud", self.uop), Ru_data=Ru_data, D_data=t("D", self.dop), X_data=t("X", xop),
                         X̂_data=t("Xhat", self.xhop), status=status, path=SIM_PATH_FUSED if fused else SIM_PATH_PERIOD,
                         est_status=est_status)

    def _period_args(self, xhat0, ry, d, lastu, Dhat, Rhaty, Rhatu):
        """The arguments of `moveinput` checked, broadcast over the batch and turned into what a step takes: x̂0, ry
        (engineering), whether R̂y is ry held over the horizon (MPCQP_FLAG_RY_CONSTANT is set accordingly), R̂y, R̂u
        (engineering, or None), and the deviations lastu0, d0, D̂0."""
        B, Hp = self.B, self.Hp
        if xhat0 is None:
            xhat0 = self.xhat0                      # the attached estimator's state (setestimator)
        xhat0 = np.asarray(xhat0, float)
        if xhat0.shape != (B, self.nxh):
            raise ValueError(f"xhat0 size must be ({B},{self.nxh})")
        bc = lambda v, n, name: self._bc(v, n, name)
        ry = self.yop if ry is None else bc(ry, self.ny, "ry")
        held = Rhaty is None                      # R̂y = repeat(ry, Hp): send ry once (MPCQP_FLAG_RY_CONSTANT)
        Rhaty = None if held else bc(Rhaty, self.nY, "R̂y")
        want = (self.hd.flags | FLAG_RY_CONSTANT) if held else (self.hd.flags & ~FLAG_RY_CONSTANT)
        if want != self.hd.flags:
            self.hd.set_flags(want)
        Rhatu = None if Rhatu is None else bc(Rhatu, self.nU, "R̂u")
        lastu0 = self.lastu0 if lastu is None else bc(lastu, self.nu, "lastu") - self.uop
        d0 = Dh0 = None
        if self.nd > 0:
            d = bc(d, self.nd, "d")
            Dhat = np.tile(d, Hp) if Dhat is None else bc(Dhat, self.nd * Hp, "D̂")
            d0, Dh0 = d - self.dop, Dhat - self.Dop
        elif d is not None and np.size(d) != 0:
            raise ValueError("d size must be (0,)")
        return xhat0, ry, held, Rhaty, Rhatu, lastu0, d0, Dh0

    def _period_record(self, xhat0, ry, held, Rhaty, Rhatu, lastu0, d0, Dh0):
        """What `getinfo` and the next period need of the period that has just been solved."""
        Hp = self.Hp
        self._lastu0_prev = lastu0
        self._winfo = (xhat0, np.tile(ry, Hp) if (held and self.nw > 0) else Rhaty, d0, Dh0)
        self._ry_now = ry.copy()
        self._ginfo = (xhat0.copy(), np.tile(ry, Hp) if held else Rhaty, self.Uop.copy() if Rhatu is None else Rhatu)
        self.solved_once = True

    def _bc(self, v, n, name):
        a = np.asarray(v, float)
        if a.shape == (n,):
            a = np.broadcast_to(a, (self.B, n))
        if a.shape != (self.B, n):
            raise ValueError(f"{name} size must be ({n},)")       # DimensionMismatch
        return a

    def getinfo(self):
        """`getinfo` (src/controller/execute.jl:145-198) for every controller of the batch: ΔU, ϵ, J,
        U, u, lastu, d, D̂, x̂, ŷ, Ŷ, x̂end, Ŷs, R̂y, R̂u, W (+ the reference's ASCII aliases).  Ŷ comes
        from the kernel (`moveinput(..., want_info=True)`, predict! transcription.jl:1136-1145); the
        quantities derived from it (J, ŷ-independent ones aside) need that flag too."""
        nu, Hc, Hp, ny, nd = self.nu, self.Hc, self.Hp, self.ny, self.nd
        DU = self.Z[:, :self.nDU]
        blk = np.repeat(np.arange(Hc), self.nb)
        cum = np.cumsum(DU.reshape(self.B, Hc, nu), axis=1)
        U0 = cum[:, blk, :].reshape(self.B, -1) + np.tile(self._lastu0_prev, self.Hp)
        xhat0, Rhaty, Rhatu = self._ginfo
        _, _, d0, Dh0 = self._winfo
        eps = self.Z[:, -1].copy() if self.neps else np.zeros(self.B)
        info = {"ΔU": DU.copy(), "ϵ": eps, "u": self.lastu0 + self.uop, "U": U0 + self.Uop,
                "lastu": self._lastu0_prev + self.uop, "x̂": xhat0 + self.xhop, "R̂y": Rhaty.copy(), "R̂u": Rhatu.copy(),
                "d": (d0 + self.dop) if nd > 0 else np.zeros((self.B, 0)),
                "D̂": (Dh0 + self.Dop) if nd > 0 else np.zeros((self.B, 0)),
                "Ŷs": np.zeros((self.B, self.nY))}          # stochastic predictions: InternalModel only (predictstoch!)
        # ŷ(k) = Ĉ x̂0 + D̂d d0 + yop (evaloutput, execute.jl:297-314)
        yk = np.einsum("bij,bj->bi", self._Chat, xhat0) + self.yop
        if nd > 0:
            yk = yk + np.einsum("bij,bj->bi", self._Dhd, d0)
        if getattr(self, "internal", False):        # the Ŷs and ŷs of the last correction: what the step used (predictstoch!)
            info["Ŷs"], info["im_status"] = self.hd.get(GET_IM_YHATS), self.hd.im_status()
            info["x̂s"], info["ŷs"] = self.hd.get(GET_IM_XS), self.hd.get(GET_IM_YS)
            yk = yk + info["ŷs"]
        info["ŷ"] = yk
        # x̂end = x̂0(k+Hp): the augmented model driven by the optimal inputs (predict!, transcription.jl:1136-1145)
        x = xhat0.copy()
        dop_x = self.fhop - self.xhop
        U0s = U0.reshape(self.B, Hp, nu)
        X0 = np.empty((self.B, Hp, self.nxh))
        for t in range(Hp):
            x = np.einsum("bij,bj->bi", self._Ahat, x) + np.einsum("bij,bj->bi", self._Bhu, U0s[:, t]) + dop_x
            if nd > 0:
                dt = d0 if t == 0 else Dh0[:, (t - 1) * nd:t * nd]
                x = x + np.einsum("bij,bj->bi", self._Bhd, dt)
            X0[:, t] = x
        if getattr(self, "_ms_kernel", False):     # X̂0 is part of the MultipleShooting decision vector: the kernel's own
            X0 = self.hd.get(GET_XHAT_MS)
            x = X0[:, -1]
        info["x̂end"] = x + self.xhop
        if getattr(self, "kf_timevarying", False) or getattr(self, "kf_steady", False):
            # the estimator's covariance (P̂∞ of a steady solve), gain and per-estimator status
            info["P̂"], info["K̂"], info["kf_status"] = self.hd.kf_covariance(), self.hd.kf_gain(), self.hd.kf_status()
            if getattr(self, "kf_steady", False) and hasattr(self.hd, "kf_steady_path"):
                info["kf_steady_path"] = self.hd.kf_steady_path()      # 1: solved by the square-root form (semidefinite Q̂)
        if getattr(self, "kf_luenberger", False):  # the placed gain, per-member status and sweep counts
            info["K̂"], info["kf_status"], info["place_sweeps"] = self.hd.kf_gain(), self.hd.kf_status(), self.hd.kf_place_sweeps()
        if getattr(self, "mhe", None) is not None:
            info["estim"] = self.mhe.getinfo()
        # decision vector in the transcription's layout: [ΔU; ϵ] or [ΔU; X̂0(k+1..k+Hp); ϵ] (get_nZ_mpc, transcription.jl:2-7)
        parts = [DU] + ([X0.reshape(self.B, -1)] if self.transcription == "MultipleShooting" else []) + ([eps[:, None]] if self.neps else [])
        info["Z̃"] = np.concatenate(parts, axis=1)
        info["X̂0"] = X0.reshape(self.B, -1)
        if self._Yhat0 is not None:
            info["Ŷ"] = self._Yhat0 + self.Yop
            # J = (Ŷ-R̂y)'M(Ŷ-R̂y) + ΔU'N ΔU + (U-R̂u)'L(U-R̂u) + C ϵ²   (obj_nonlinprog!, general.jl:107 with r)
            ey, eu = info["Ŷ"] - Rhaty, info["U"] - Rhatu
            if getattr(self, "Mfull", None) is not None:
                Jy = np.einsum("bi,bij,bj->b", ey, self.Mfull, ey)
            elif self.Mblk is not None:
                eyb = ey.reshape(self.B, Hp, ny)
                Jy = np.einsum("bti,btij,btj->b", eyb, self.Mblk, eyb)
            else:
                Jy = np.sum(np.tile(self.Mwt, Hp) * ey * ey, axis=1)
            Jdu = (np.einsum("bi,bij,bj->b", DU, self.Ndense, DU) if getattr(self, "Ndense", None) is not None
                   else np.sum(np.tile(self.Nwt, Hc) * DU * DU, axis=1))
            Ju = (np.einsum("bi,bij,bj->b", eu, self.Ldense, eu) if getattr(self, "Ldense", None) is not None
                  else np.sum(np.tile(self.Lwt, Hp) * eu * eu, axis=1))
            info["J"] = Jy + Jdu + Ju + (self.Cwt * eps * eps if self.neps else 0.0)
            if self.nw > 0:       # W = Wy ŷe + Wu ue + Wd d̂e + Wr r̂e   (execute.jl:221, relaxW)
                xhat0, Rhaty, d0, Dh0 = self._winfo
                Hp, ny, nd = self.Hp, self.ny, self.nd
                yk = np.einsum("bij,bj->bi", self._Chat, xhat0) + self.yop
                if nd > 0:
                    yk = yk + np.einsum("bij,bj->bi", self._Dhd, d0)
                ye = np.concatenate([yk, info["Ŷ"]], axis=1).reshape(self.B, Hp + 1, ny)
                U = info["U"].reshape(self.B, Hp, nu)
                ue = np.concatenate([U, U[:, -1:, :]], axis=1)
                re = np.concatenate([self._ry_now, Rhaty], axis=1).reshape(self.B, Hp + 1, ny)
                Wv = (np.einsum("bij,btj->bti", self.Wy, ye) + np.einsum("bij,btj->bti", self.Wu, ue)
                      + np.einsum("bij,btj->bti", self.Wr, re))
                if nd > 0:
                    de = np.concatenate([d0 + self.dop, Dh0 + self.Dop], axis=1).reshape(self.B, Hp + 1, nd)
                    Wv = Wv + np.einsum("bij,btj->bti", self.Wd, de)
                info["W"] = Wv.reshape(self.B, -1)
        for a, k in (("DeltaU", "ΔU"), ("epsilon", "ϵ"), ("Dhat", "D̂"), ("xhat", "x̂"), ("yhat", "ŷ"), ("Yhat", "Ŷ"),
                     ("xhatend", "x̂end"), ("Yhats", "Ŷs"), ("Rhaty", "R̂y"), ("Rhatu", "R̂u"), ("Ztilde", "Z̃"), ("Xhat0", "X̂0"), ("Phat", "P̂"), ("Khat", "K̂")):
            if k in info:
                info[a] = info[k]
        return info


class BatchExplicitMPC(BatchLinMPC):
    """B independent `ExplicitMPC` controllers (src/controller/explicitmpc.jl:135-179): the LinMPC without constraints, H̃
    factored once on the device and Z̃ = -H̃⁻¹ q̃ applied every period.  Like the reference's constructor it has no `Cwt`,
    `Wy` ... `Wr` and `transcription` keywords.  `law=True` also builds the affine law of the default call
    `moveinput(x̂0, ry, d)`; a period without a horizon-long argument (R̂y, R̂u, D̂) is then one table product.

    Estimator, `setmodel` / `setweights` (factor and law follow), `initstate` and `moveinput` are those of `BatchLinMPC`."""

    def __init__(self, Ahat, Bhu, Chat, Bhd=None, Dhd=None, *, Hp, Hc=2, Mwt=None, Nwt=None, Lwt=None, M_Hp=None, N_Hc=None,
                 L_Hp=None, law=False, uop=None, yop=None, dop=None, xhop=None, fhop=None, device=0, keep_qp=False, lib=None):
        self.law = bool(law)
        self._explicit_ready = False
        super().__init__(Ahat, Bhu, Chat, Bhd, Dhd, Hp=Hp, Hc=Hc, Mwt=Mwt, Nwt=Nwt, Lwt=Lwt, M_Hp=M_Hp, N_Hc=N_Hc, L_Hp=L_Hp,
                         Cwt=np.inf, uop=uop, yop=yop, dop=dop, xhop=xhop, fhop=fhop, device=device, keep_qp=keep_qp, lib=lib)
        self.hd.explicit_prepare(law=self.law)
        self._explicit_ready = True
        self._warn_factor()

    def _warn_factor(self):
        n = int(np.count_nonzero(self.hd.explicit_status()))
        if n:
            warnings.warn(f"ExplicitMPC: H̃ is not positive definite, Z̃ = 0 is returned ({n} of {self.B} controllers)", RuntimeWarning)

    def setmodel(self, Ahat, Bhu, Chat, Bhd=None, Dhd=None, *, uop=None, yop=None, dop=None, xhop=None, fhop=None):
        """`setmodel!` (execute.jl:684-790): new model matrices and, optionally, new operating points -- lastu0 then moves
        with uop like the reference's (`mpc.lastu0 .+= uop_old .- uop_new`, execute.jl:726), and the state of an attached
        estimator with x̂op (`estim.x̂0 .+= x̂op_old .- x̂op_new`)."""
        B, Hp = self.B, self.Hp
        vec = lambda v, n, old: old if v is None else np.broadcast_to(np.asarray(v, float), (B, n)).copy()
        if uop is not None:
            new = vec(uop, self.nu, None)
            self.lastu0 = self.lastu0 + self.uop - new
            self.uop = new
        self.yop, self.dop = vec(yop, self.ny, self.yop), vec(dop, self.nd, self.dop)
        if xhop is not None:                   # the attached estimator's state keeps its engineering value (x̂0 += x̂op_old - x̂op_new)
            new = vec(xhop, self.nxh, None)
            if getattr(self, "mhe", None) is None and getattr(self, "xhat0", None) is not None:
                self.xhat0 = self.xhat0 + self.xhop - new
            self.xhop = new
        self.fhop = vec(fhop, self.nxh, self.fhop)
        if getattr(self, "mhe", None) is not None:      # the estimator moves its windows, x̂0 and bounds itself (BatchMHE.setmodel)
            self._mhe_ops = dict(uop=self.uop, yop_m=self.yop[:, self.i_ym], dop=self.dop, x̂op=self.xhop, f̂op=self.fhop)
        self.Uop, self.Yop, self.Dop = np.tile(self.uop, Hp), np.tile(self.yop, Hp), np.tile(self.dop, Hp)
        super().setmodel(Ahat, Bhu, Chat, Bhd, Dhd)
        if self._explicit_ready:               # (the handle has refreshed factor and law inside mpcqp_set_model)
            self._warn_factor()

    def setweights(self, Mwt=None, Nwt=None, Lwt=None, M_Hp=None, N_Hc=None, L_Hp=None):
        super().setweights(Mwt, Nwt, Lwt, M_Hp=M_Hp, N_Hc=N_Hc, L_Hp=L_Hp)
        if self._explicit_ready:
            self._warn_factor()

    def setconstraint(self, **kw):
        raise MpcqpError("ExplicitMPC does not support constraints.")       # explicitmpc.jl:182-184

    def _sim_prepare(self):
        """`sim` runs the law when it was built and `ru` is None, else the explicit step: no interior-point kernel to prepare."""

    def moveinput(self, xhat0, ry=None, d=None, *, lastu=None, Dhat=None, Rhaty=None, Rhatu=None, want_info=False, want_Z=True):
        """`moveinput!` (execute.jl:59-80) on the explicit paths: the law when it was built and no horizon-long argument is
        given (and Ŷ is not asked for), else the explicit step.  The law computes all of Z̃ (the table of nZ̃ rows per
        controller); `want_Z=False` asks it for u alone, from the table of nu rows -- `self.Z` is NaN after such a period and
        `getinfo` has nothing to report.  The explicit step always returns Z̃."""
        default_D = Dhat is None
        xhat0, ry, held, Rhaty, Rhatu, lastu0, d0, Dh0 = self._period_args(xhat0, ry, d, lastu, Dhat, Rhaty, Rhatu)
        if self.law and held and Rhatu is None and default_D and not want_info:
            Z, u0, self.status = self.hd.explicit_law(xhat0, lastu0, ry - self.yop, d0, want_Z=want_Z)
            self.Z = np.full((self.B, self.nZ), np.nan) if Z is None else Z
            self._Yhat0 = None
        else:
            out = self.hd.explicit_step(xhat0, lastu0, (ry - self.yop) if held else (Rhaty - self.Yop),
                                        Ru=None if Rhatu is None else Rhatu - self.Uop, d0=d0, Dhat0=Dh0, want_Yhat=want_info)
            self.Z, u0, self.status = out[0], out[1], out[2]
            self._Yhat0 = out[3] if want_info else None
        self.iters = np.zeros(self.B, np.int32)
        self._period_record(xhat0, ry, held, Rhaty, Rhatu, lastu0, d0, Dh0)
        self.lastu0 = u0.copy()
        return u0 + self.uop

    __call__ = moveinput

    def getinfo(self):
        """`getinfo` of the ExplicitMPC (explicitmpc.jl:200-220): as BatchLinMPC, with x̂end filled with NaN (:217)."""
        info = super().getinfo()
        info["x̂end"] = np.full((self.B, self.nxh), np.nan)
        info["xhatend"] = info["x̂end"]
        return info
