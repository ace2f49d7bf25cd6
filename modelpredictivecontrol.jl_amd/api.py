"""Host-side mirror of the reference's LinMPC interface over the C-ABI of include/mpcqp.h.

Two layers:

* `Handle` (this file) -- 1:1 ctypes binding of the C entry points (what a Julia `ccall` shim binds, see
  INTEGRATION.md).  Works with host (NumPy) pointers or raw device pointers.
* `BatchLinMPC` (controller.py, re-exported at the end of this file) -- B logical `LinMPC` controllers of identical dimensions with the reference's
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
import os
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


def _addr(p):
    """An integer device address (or a stream) as the pointer argument it is; 0 = NULL."""
    return C.c_void_p(int(p)) if p else None


def colmajor(M):
    """(B, rows, cols) logical -> the ABI's column-major-per-problem buffer (= Julia (rows,cols,B))."""
    return _f64(np.asarray(M, float).transpose(0, 2, 1))


def _ptrs(arrays, conv=_f64):
    """Optional arrays -> (what `conv` made of them, their pointers); None stays None.  The caller holds the first list
    over the library call: the pointers are borrowed from it."""
    keep = [None if a is None else conv(a) for a in arrays]
    return keep, [_ptr(a) for a in keep]


def _stage_step(hd, xhat0, lastu0, Ry, Ru, d0, Dhat0, Z=None):
    """The host-pointer arguments of a step of `hd` (Handle or MultiHandle) as float64 buffers, every size checked; Z̃, where
    the call updates it in place, has to be the caller's float64 C-contiguous array."""
    B = hd.B
    args = [_f64(xhat0), _f64(lastu0), _f64(Ry)] + _ptrs((Ru, d0, Dhat0))[0]
    nry = hd.ny if (hd.flags & FLAG_RY_CONSTANT) else hd.nY
    for a, n in zip(args, (hd.nxhat, hd.nu, nry, hd.nU, hd.nd, hd.nD)):
        if a is not None and a.size != B * n:
            raise ValueError("DimensionMismatch in step arguments")
    if Z is not None:
        if Z.size != B * hd.nZ:
            raise ValueError("DimensionMismatch in step arguments")
        assert Z.dtype == np.float64 and Z.flags.c_contiguous
    return args


def _host_step(hd, fn, xhat0, lastu0, Ry, Z, Ru, d0, Dhat0, want_Yhat):
    """mpcqp_step / mpcqp_multi_step on host pointers: Z (B,nZ) is updated in place.  Returns u0, status, iters[, Yhat0]."""
    B = hd.B
    args = _stage_step(hd, xhat0, lastu0, Ry, Ru, d0, Dhat0, Z)
    u0, status, iters = np.empty((B, hd.nu)), np.empty(B, np.int32), np.empty(B, np.int32)
    yh = np.empty((B, hd.nY)) if want_Yhat else None
    _chk(hd.lib, fn(hd.h, *[_ptr(a) for a in args], _ptr(Z), _ptr(u0), _ptr(status), _ptr(iters), _ptr(yh)))
    return (u0, status, iters, yh) if want_Yhat else (u0, status, iters)


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
    cin = C2dIn(*[_addr(p) for p in (A, Bu, C, Bd, Dd, Ts, dop)])
    cout = C2dOut(*[_addr(p) for p in (Ahat, Bhu, Chat, Bhd, Dhd, dophat)])
    _chk(lib, lib.mpcqp_c2d_device(_ct.byref(opts.spec), _ct.byref(cin), _ct.byref(cout), _addr(status), _addr(stream)))


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

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.mpcqp_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _need(self, name):
        """An entry point that an older or a variant build of the library may lack (load_library binds those it finds)."""
        if not hasattr(self.lib, name):
            raise NotImplementedError(f"this library has no {name}")
        return getattr(self.lib, name)

    def _read_i32(self, fn, *args):
        """The (B,) int32 that `fn(h, *args, out)` fills."""
        out = np.zeros(self.B, np.int32)
        _chk(self.lib, fn(self.h, *args, _ptr(out)))
        return out

    def set_model(self, Ahat, Bu, Cm, Bd=None, Dd=None, dop=None):
        keep, ptrs = _ptrs((Ahat, Bu, Cm, Bd, Dd, dop))
        _chk(self.lib, self.lib.mpcqp_set_model(self.h, *ptrs))

    def set_model_continuous(self, opts, A, Bu, Cm, Ts, Bd=None, Dd=None, dop=None):
        """mpcqp_set_model_continuous: `opts` a C2dOptions, the arrays in ABI layout (host).  Returns status (B,) int32."""
        fn = self._need("mpcqp_set_model_continuous")
        keep, ptrs = _ptrs((A, Bu, Cm, Bd, Dd, Ts, dop))
        cin = C2dIn(*ptrs)
        return self._read_i32(fn, C.byref(opts.spec), C.byref(cin))

    def set_model_continuous_device(self, opts, A, Bu, Cm, Ts, status, Bd=0, Dd=0, dop=0, stream=0):
        """mpcqp_set_model_continuous_device: raw device addresses; the launch, K1, K2 and the refreshes are enqueued on `stream`."""
        self._need("mpcqp_set_model_continuous_device")
        cin = C2dIn(*[_addr(p) for p in (A, Bu, Cm, Bd, Dd, Ts, dop)])
        _chk(self.lib, self.lib.mpcqp_set_model_continuous_device(self.h, C.byref(opts.spec), C.byref(cin), _addr(status), _addr(stream)))

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
        keep, ptrs = _ptrs((Mdiag, Ndiag, Ldiag, Cwt))
        _chk(self.lib, self.lib.mpcqp_set_weights(self.h, *ptrs))

    def set_output_weight_blocks(self, Mblk):
        """Mblk (B, Hp, ny, ny), symmetric blocks, or None (back to the diagonal weight)."""
        a = None if Mblk is None else _f64(np.asarray(Mblk, float).transpose(0, 1, 3, 2))
        _chk(self.lib, self.lib.mpcqp_set_output_weight_blocks(self.h, _ptr(a)))

    def set_dense_weights(self, M_Hp=None, N_Hc=None, L_Hp=None):
        """Dense symmetric weights (B, n, n) or None; they replace the diagonals of set_weights."""
        keep, ptrs = _ptrs((M_Hp, N_Hc, L_Hp), colmajor)
        _chk(self.lib, self.lib.mpcqp_set_dense_weights(self.h, *ptrs))

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
        keep, ptrs = _ptrs((Wy, Wu, Wd, Wr, w_op))
        _chk(self.lib, self.lib.mpcqp_set_custom_constraints(self.h, int(nw), *ptrs))

    def set_custom_bounds(self, Wmin=None, Wmax=None, C_wmin=None, C_wmax=None):
        keep, ptrs = _ptrs((Wmin, Wmax, C_wmin, C_wmax))
        _chk(self.lib, self.lib.mpcqp_set_custom_bounds(self.h, *ptrs))

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
        return _host_step(self, self.lib.mpcqp_step, xhat0, lastu0, Ry, Z, Ru, d0, Dhat0, want_Yhat)

    def step_device(self, xhat0, lastu0, Ry, Z, u0, status, iters=0, Ru=0, d0=0, Dhat0=0, Yhat0=0,
                    stream=0):
        """All arguments are integer device addresses (0 = NULL); asynchronous on `stream`."""
        _chk(self.lib, self.lib.mpcqp_step_device(self.h, _addr(xhat0), _addr(lastu0), _addr(Ry), _addr(Ru), _addr(d0),
                                                  _addr(Dhat0), _addr(Z), _addr(u0), _addr(status), _addr(iters),
                                                  _addr(Yhat0), _addr(stream)))

    def loop_device(self, xhat0, y0m, lastu0, Ry, Z, u0, status, iters=0, Ru=0, d0=0, Dhat0=0, Yhat0=0, stream=0):
        """preparestate! + moveinput! + updatestate! of one period in one launch (mpcqp_loop_device);
        integer device addresses, xhat0 updated in place."""
        _chk(self.lib, self.lib.mpcqp_loop_device(self.h, _addr(xhat0), _addr(y0m), _addr(lastu0), _addr(Ry), _addr(Ru), _addr(d0), _addr(Dhat0),
                                                  _addr(Z), _addr(u0), _addr(status), _addr(iters), _addr(Yhat0), _addr(stream)))

    # -- ExplicitMPC: H̃ factored once (explicit_prepare), then a solve (explicit_step) or a gain (explicit_law) per period
    def explicit_prepare(self, law=False):
        """mpcqp_explicit_prepare: factor every controller's H̃ on the device; `law=True` builds the law tables too."""
        _chk(self.lib, self.lib.mpcqp_explicit_prepare(self.h, EXPLICIT_LAW if law else 0))

    def explicit_status(self):
        """(B,) int32: 0 factored, 2 H̃ not positive definite / not finite."""
        return self._read_i32(self.lib.mpcqp_explicit_status)

    def explicit_step(self, xhat0, lastu0, Ry, Ru=None, d0=None, Dhat0=None, want_Yhat=False):
        """Host-pointer explicit step.  Returns Z (B,nZ), u0, status[, Yhat0]."""
        B = self.B
        args = _stage_step(self, xhat0, lastu0, Ry, Ru, d0, Dhat0)
        Z, u0, status = np.empty((B, self.nZ)), np.empty((B, self.nu)), np.empty(B, np.int32)
        yh = np.empty((B, self.nY)) if want_Yhat else None
        _chk(self.lib, self.lib.mpcqp_explicit_step(self.h, *[_ptr(a) for a in args], _ptr(Z), _ptr(u0), _ptr(status), _ptr(yh)))
        return (Z, u0, status, yh) if want_Yhat else (Z, u0, status)

    def explicit_step_device(self, xhat0, lastu0, Ry, Z, u0, status, Ru=0, d0=0, Dhat0=0, Yhat0=0, stream=0):
        """All arguments are integer device addresses (0 = NULL); asynchronous on `stream`."""
        _chk(self.lib, self.lib.mpcqp_explicit_step_device(self.h, _addr(xhat0), _addr(lastu0), _addr(Ry), _addr(Ru), _addr(d0), _addr(Dhat0),
                                                           _addr(Z), _addr(u0), _addr(status), _addr(Yhat0), _addr(stream)))

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
        _chk(self.lib, self.lib.mpcqp_explicit_law_device(self.h, _addr(xhat0), _addr(lastu0), _addr(ry), _addr(d0), _addr(Z), _addr(u0), _addr(status), _addr(stream)))

    # -- sim!: closed loops of the whole batch, the plant on the device
    def sim_set_plant(self, A, Bu, Cm, Bd=None, Dd=None, fx=None):
        """mpcqp_sim_set_plant: A (B,nxp,nxp), Bu, Cm, Bd, Dd in ABI layout (see `colmajor`), fx = fop - xop (B,nxp)."""
        keep, ptrs = _ptrs((A, Bu, Cm, Bd, Dd, fx))
        nxp = int(round(np.sqrt(keep[0].size // self.B)))
        _chk(self.lib, self.lib.mpcqp_sim_set_plant(self.h, nxp, *ptrs))
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
        _chk(self.lib, self.lib.mpcqp_sim_device(self.h, C.byref(io), _addr(stream)))

    def recondense_device(self, stream=0):
        _chk(self.lib, self.lib.mpcqp_recondense_device(self.h, _addr(stream)))

    # -- LinMPC(MovingHorizonEstimator) and the estimator half of initstate! (include/mpcqp_mhe.h) ------------
    def mhe_attach(self, est, i_ym=None):
        """mpcqp_mhe_attach: `est` an `mhe.MheHandle` (borrowed: this object keeps a reference) or None to detach; i_ym the
        measured rows of Ĉ."""
        self._need("mpcqp_mhe_attach")
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
        fn = self._need("mpcqp_est_initstate")
        keep, ptrs = _ptrs((u0, y0m, d0))
        return self._read_i32(fn, _ptr(xhat0), *ptrs)

    def est_initstate_device(self, xhat0, u0, y0m, status, d0=0, stream=0):
        _chk(self.lib, self.lib.mpcqp_est_initstate_device(self.h, _addr(xhat0), _addr(u0), _addr(y0m), _addr(d0), _addr(status), _addr(stream)))

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
        fn = self._need("mpcqp_im_set")
        iy = np.ascontiguousarray(i_ym, dtype=np.int32)
        arrs, ptrs = _ptrs([None] * 4 if stoch is None else stoch)
        nxs = int(iy.size) if stoch is None else int(arrs[0].shape[-1]) if arrs[0] is not None else 0
        _chk(self.lib, fn(self.h, nxs, *ptrs, _ptr(iy), int(iy.size)))
        self.nym, self.nxs = int(iy.size), nxs

    def im_status(self):
        """(B,) int32: 0 ready, 2 the member's Ds is singular (its stochastic part is off)."""
        return self._read_i32(self.lib.mpcqp_im_status)

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
        _chk(self.lib, self.lib.mpcqp_im_correct_device(self.h, _addr(xhat0), _addr(y0m), _addr(d0), _addr(stream)))

    def im_update_device(self, xhat0, u0, d0=0, stream=0):
        _chk(self.lib, self.lib.mpcqp_im_update_device(self.h, _addr(xhat0), _addr(u0), _addr(d0), _addr(stream)))

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
        keep, ptrs = _ptrs((Qhat, Rhat, P0), colmajor)
        _chk(self.lib, self.lib.mpcqp_kf_set_covariances(self.h, *ptrs, _ptr(iy), int(iy.size)))
        self.nym = int(iy.size)

    # -- SteadyKalmanFilter from Q̂ and R̂: the gain solved for on the device (csrc/kf_dare_bodies.h)
    def kf_set_steady(self, Qhat, Rhat, i_ym):
        """Qhat (B,nx̂,nx̂) symmetric positive semidefinite, Rhat (B,nym,nym) symmetric positive definite.  Solves the Riccati
        equation of every member on the resident model; kf_gain() / kf_covariance() / kf_status() / kf_steady_iters() read
        the result back.  max(nx̂, nym) <= 64 (-4 beyond); above 32 the operands of the solve live in LDS, one member per
        workgroup (csrc/kf_dare_lds_bodies.h), Q̂ has to be positive definite (status 2 otherwise), and kf_set_covariances,
        kf_set_poles and est_initstate still answer -4 on such a handle, which keeps its solved gain."""
        fn = self._need("mpcqp_kf_set_steady")
        iy = np.ascontiguousarray(i_ym, dtype=np.int32)
        _chk(self.lib, fn(self.h, _ptr(colmajor(Qhat)), _ptr(colmajor(Rhat)), _ptr(iy), int(iy.size)))
        self.nym = int(iy.size)

    def kf_solve_steady(self):
        """Solve again on the model that is resident now (after set_model); host-synchronous."""
        _chk(self.lib, self._need("mpcqp_kf_solve_steady")(self.h))

    def kf_solve_steady_device(self, stream=0):
        _chk(self.lib, self._need("mpcqp_kf_solve_steady_device")(self.h, C.c_void_p(stream)))

    def kf_steady_iters(self):
        """(B,) int32 doubling iterations of the last solve."""
        return self._read_i32(self._need("mpcqp_kf_steady_iters"))

    def kf_steady_path(self):
        """(B,) int32: 0 the estimator was solved by (or left with) the definite form of the iteration, 1 the square-root
        form ran for it (a semidefinite Q̂)."""
        return self._read_i32(self._need("mpcqp_kf_steady_path"))

    # -- Luenberger observer from its poles: the gain placed on the device (csrc/kf_place_bodies.h)
    def kf_set_poles(self, poles, i_ym):
        """poles (B,nx̂) real, inside the unit circle.  Places them on the resident model: the eigenvalues of Â (I - K̂ Ĉm);
        kf_gain() / kf_status() / kf_place_sweeps() read the result back."""
        fn = self._need("mpcqp_kf_set_poles")
        iy = np.ascontiguousarray(i_ym, dtype=np.int32)
        _chk(self.lib, fn(self.h, _ptr(_f64(poles)), _ptr(iy), int(iy.size)))
        self.nym = int(iy.size)

    def kf_place(self):
        """Place again on the model that is resident now (after set_model); host-synchronous."""
        _chk(self.lib, self._need("mpcqp_kf_place")(self.h))

    def kf_place_device(self, stream=0):
        _chk(self.lib, self._need("mpcqp_kf_place_device")(self.h, C.c_void_p(stream)))

    def kf_set_place_cap(self, cap):
        """Most sweeps of the placements that follow, 0 .. 100 (default 30)."""
        _chk(self.lib, self._need("mpcqp_kf_set_place_cap")(self.h, int(cap)))

    def kf_place_sweeps(self):
        """(B,) int32 sweeps of the last placement."""
        return self._read_i32(self._need("mpcqp_kf_place_sweeps"))

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
        return self._read_i32(self.lib.mpcqp_kf_status)

    def kf_lanes_per_estimator(self):
        """0 on a steady gain; 16 / 64 lanes per estimator of the covariance kernel otherwise; 256 (a workgroup of four
        wavefronts) after kf_set_steady beyond 32 states or measured outputs."""
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
        _chk(self.lib, self.lib.mpcqp_kf_update_device(self.h, _addr(xhat0), _addr(u0), _addr(y0m), _addr(d0), _addr(stream)))

    def kf_correct_device(self, xhat0, y0m, d0=0, stream=0):
        _chk(self.lib, self.lib.mpcqp_kf_correct_device(self.h, _addr(xhat0), _addr(y0m), _addr(d0), _addr(stream)))

    def kf_predict_device(self, xhat0, u0, d0=0, stream=0):
        _chk(self.lib, self.lib.mpcqp_kf_predict_device(self.h, _addr(xhat0), _addr(u0), _addr(d0), _addr(stream)))

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
        keep, ptrs = _ptrs((Ahat, Bu, Cm, Bd, Dd, dop))
        _chk(self.lib, self.lib.mpcqp_multi_set_model(self.h, *ptrs))

    def set_weights(self, Mdiag, Ndiag, Ldiag, Cwt=None):
        keep, ptrs = _ptrs((Mdiag, Ndiag, Ldiag, Cwt))
        _chk(self.lib, self.lib.mpcqp_multi_set_weights(self.h, *ptrs))

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
        return _host_step(self, self.lib.mpcqp_multi_step, xhat0, lastu0, Ry, Z, Ru, d0, Dhat0, want_Yhat)

    # ---- device-resident path: per-device buffers, nothing crosses PCIe --------------------------------------
    def device_of(self, g):
        """CUDA/HIP ordinal the shard g lives on (as given to the constructor)."""
        return self._devices[g]

    def step_device_shard(self, g, xhat0, lastu0, Ry, Z, u0, status, iters=0, stream=0):
        """mpcqp_step_device on the handle of shard g: integer device addresses of that shard's buffers."""
        hg = C.c_void_p(self.lib.mpcqp_multi_handle(self.h, g))
        _chk(self.lib, self.lib.mpcqp_step_device(hg, _addr(xhat0), _addr(lastu0), _addr(Ry), None, None, None, _addr(Z), _addr(u0), _addr(status),
                                                  _addr(iters), None, _addr(stream)))

    def scatter_device(self, root, xhat0_root, lastu0_root, Ry_root, ry_rows, xhat0_shards, lastu0_shards, Ry_shards, stream=0):
        """mpcqp_multi_scatter_device: whole-batch inputs on device `root` -> the shards' buffers (integer addresses)."""
        arr = lambda ps: (C.c_void_p * len(ps))(*[C.c_void_p(int(p)) for p in ps])
        _chk(self.lib, self.lib.mpcqp_multi_scatter_device(self.h, root, _addr(xhat0_root), _addr(lastu0_root), _addr(Ry_root), int(ry_rows),
                                                          arr(xhat0_shards), arr(lastu0_shards), arr(Ry_shards), _addr(stream)))

    def gather_device(self, root, Z_shards, u0_shards, status_shards, Z_root, u0_root, status_root, stream=0):
        """mpcqp_multi_gather_device: the shards' Z̃, u0, status -> whole-batch buffers on device `root`."""
        arr = lambda ps: (C.c_void_p * len(ps))(*[C.c_void_p(int(p)) for p in ps])
        _chk(self.lib, self.lib.mpcqp_multi_gather_device(self.h, root, arr(Z_shards), arr(u0_shards), arr(status_shards),
                                                         _addr(Z_root), _addr(u0_root), _addr(status_root), _addr(stream)))


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


# The controllers built on this binding live in controller.py; they stay importable from here, where the package's
# __init__ files and every caller look for them.  (At the end of the file: controller.py imports the names above.)
from .controller import BatchExplicitMPC, BatchLinMPC, SimResult  # noqa: E402,F401
