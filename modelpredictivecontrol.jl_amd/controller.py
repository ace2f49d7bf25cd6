"""`BatchLinMPC` and `BatchExplicitMPC`: the reference's LinMPC / ExplicitMPC vocabulary for a batch of controllers, on
the ctypes binding of api.py (see that file's docstring for the two layers and the reference's line numbers)."""
from __future__ import annotations

import dataclasses
import warnings

import numpy as np

from .api import (BOUND_FIELDS, FLAG_COLD_START, FLAG_KEEP_QP, FLAG_RY_CONSTANT, FLAG_WARM_DUAL, GET_IM_XS, GET_IM_YHATS,
                  GET_IM_YS, GET_XHAT_MS, KERNEL_MS, MULTIPLE_SHOOTING, SIM_FLAG_NO_FUSE, SIM_FLAG_RY_PER_PERIOD,
                  SIM_PATH_FUSED, SIM_PATH_PERIOD, SINGLE_SHOOTING, STATUS_ERROR, STATUS_ITERATION_LIMIT, C2dOptions, Handle,
                  MpcqpError, _c2d_batch, _c2d_inputs, _f64, c2d, colmajor, move_blocking)


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


# the estimator behind a BatchLinMPC (`est_kind`): none, a given steady gain, the time-varying KalmanFilter, the
# SteadyKalmanFilter from Q̂ and R̂, the Luenberger observer, a MovingHorizonEstimator, the InternalModel
EST_NONE, EST_GAIN, EST_TIMEVARYING, EST_STEADY, EST_LUENBERGER, EST_MHE, EST_INTERNAL = (
    "none", "gain", "timevarying", "steady", "luenberger", "mhe", "internal")


class BatchLinMPC:
    """B independent `LinMPC` controllers on augmented models (Â, B̂u, Ĉ, B̂d, D̂d), one GPU.

    Array arguments carry a leading batch axis: Ahat (B,nx̂,nx̂), Bhu (B,nx̂,nu), Chat (B,ny,nx̂),
    Bhd (B,nx̂,nd), Dhd (B,ny,nd).  Weights are per channel (ny / nu values, shared or (B,·)),
    repeated over the horizons like `Diagonal(repeat(Mwt, Hp))`; Cwt scalar or (B,).
    """

    est_kind = EST_NONE       # which estimator is attached: assigned by _adopt_estimator alone
    mhe = None                # the BatchMHE behind EST_MHE
    _hd_direct = True         # the form the handle is in (filter form until mpcqp_kf_set_direct says otherwise)
    kf_timevarying = property(lambda self: self.est_kind == EST_TIMEVARYING)
    kf_steady = property(lambda self: self.est_kind == EST_STEADY)
    kf_luenberger = property(lambda self: self.est_kind == EST_LUENBERGER)
    internal = property(lambda self: self.est_kind == EST_INTERNAL)

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
            self._shift_xhop(np.broadcast_to(np.asarray(xhop, float), (self.B, self.nxh)).copy())
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

    def _shift_xhop(self, new):
        """x̂op <- new; the estimate keeps its engineering value (`estim.x̂0 .+= x̂op_old .- x̂op_new`).  A
        MovingHorizonEstimator owns its state, and a controller that never had an estimate has nothing to shift."""
        if self.mhe is None and self.__dict__.get("_xhat0") is not None:
            self.xhat0 = self.xhat0 + self.xhop - new
        self.xhop = new

    def _model_changed(self):
        """What follows a new resident model: the estimator gains that are solved from it, and the attached estimator."""
        kind = self.est_kind
        if kind == EST_STEADY:                     # SteadyKalmanFilter from Q̂ and R̂: the gain follows the model
            self.hd.kf_solve_steady()
            self._warn_steady()
        elif kind == EST_LUENBERGER:               # Luenberger from its poles: so does this one
            self.hd.kf_place()
            self._warn_luenberger()
        elif kind == EST_MHE:                      # the attached MovingHorizonEstimator: the measured rows of Ĉ and D̂d
            ops = self.__dict__.pop("_mhe_ops", {})
            self.mhe.setmodel(self._Ahat, self._Bhu, self._Chat[:, self.i_ym], self._Bhd,
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
            self._shift_xhop(pad(xop))
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
        if self.mhe is not None:
            return self.mhe.x̂0
        if "_xhat0" not in self.__dict__:
            raise AttributeError("xhat0")
        return self.__dict__["_xhat0"]

    @xhat0.setter
    def xhat0(self, v):
        est = self.mhe
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
        i_ym = self._measured(i_ym, validate=False)
        if (est.B, est.nx̂, est.nu, est.nd, est.nym) != (self.B, self.nxh, self.nu, self.nd, len(i_ym)):
            raise ValueError(f"DimensionMismatch: the estimator's (B, nx̂, nu, nd, nym) = {(est.B, est.nx̂, est.nu, est.nd, est.nym)}, "
                             f"the controller's {(self.B, self.nxh, self.nu, self.nd, len(i_ym))}")
        self._measured(i_ym)
        if direct is not None and bool(direct) != est.direct:
            raise ValueError(f"direct={direct} contradicts the estimator's direct={est.direct}: the form is the estimator's own")
        for name, mine, its in (("uop", self.uop, est.uop), ("yop[i_ym]", self.yop[:, i_ym], est.yop_m), ("dop", self.dop, est.dop),
                                ("x̂op", self.xhop, est.x̂op), ("f̂op", self.fhop, est.f̂op)):
            if not np.array_equal(mine, its):
                raise ValueError(f"the estimator's {name} must be the controller's")
        self.hd.mhe_attach(est.handle, i_ym)
        return self._adopt_estimator(EST_MHE, i_ym, est.direct, None, est)

    def _measured(self, i_ym, validate=True):
        """i_ym of a setter: every output by default; `validate=False` leaves a bad index to the library (MpcqpError)."""
        i_ym = np.arange(self.ny) if i_ym is None else np.asarray(i_ym, int)
        if validate and (len(i_ym) < 1 or i_ym.min() < 0 or i_ym.max() >= self.ny or len(set(i_ym.tolist())) != len(i_ym)):
            raise ValueError("i_ym: unique indices of measured outputs in 0 .. ny-1")
        return i_ym

    def _adopt_estimator(self, kind, i_ym, direct, xhat0, est=None):
        """The tail of every estimator setter, reached once its checks and the library call have succeeded: the one place
        that says which estimator is attached.  `est`: the BatchMHE of EST_MHE, whose x̂0 is the estimate; every other kind
        starts from `xhat0` (default zero) in this object's own array."""
        self.est_kind, self.i_ym, self.direct = kind, i_ym, bool(direct)
        if est is not None:
            self.mhe = est
        else:
            self.__dict__.pop("mhe", None)
            self.xhat0 = np.zeros((self.B, self.nxh)) if xhat0 is None else _f64(np.broadcast_to(xhat0, (self.B, self.nxh))).copy()
        return self

    def _need_estimator(self):
        if self.est_kind == EST_NONE:
            raise ValueError("no estimator attached (setestimator)")
        return self.est_kind

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
        max(nx̂, nym) <= 64; `getinfo()["kf_steady_path"]` tells which form of the iteration served a member; beyond 32 states
        or measured outputs Q̂ has to be positive definite -- a semidefinite one gets `kf_status` 2 -- and `initstate`,
        `covariances=` and `luenberger=` still stop at 32 there, with the error -4 they give today), and `setmodel`
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
        i_ym = self._measured(i_ym, validate=False)
        Khat = np.asarray(Khat, float)
        if Khat.shape != (self.B, self.nxh, len(i_ym)):
            raise ValueError("Khat size must be (B, nx̂, nym)")
        self._set_direct(direct)
        self.hd.kf_set(colmajor(Khat), i_ym)        # (mpcqp_kf_set detaches a MovingHorizonEstimator)
        return self._adopt_estimator(EST_GAIN, i_ym, direct, xhat0)

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
        i_ym = self._measured(i_ym)
        nym = len(i_ym)
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
        self._hd_direct = True                      # (mpcqp_im_set puts the handle in the filter form)
        self._adopt_estimator(EST_INTERNAL, i_ym, True, xhat0)
        n = int(np.count_nonzero(self.hd.im_status()))
        if n:
            warnings.warn(f"InternalModel: Ds is singular, the stochastic part of the estimator is off ({n} of {B} estimators)", RuntimeWarning)
        return self

    def evaloutput(self, d=None):
        """`evaloutput(estim, d)`: ŷ = Ĉ x̂0 + D̂d d0 + yop, + ŷs of the last `preparestate` behind an InternalModel."""
        kind = self._need_estimator()
        y = self._yhat_now(self.xhat0, self._d0(d))
        return y + self.hd.get(GET_IM_YS) if kind == EST_INTERNAL else y

    def _yhat_now(self, xhat0, d0):
        """ŷ(k) = Ĉ x̂0 + D̂d d0 + yop (evaloutput, execute.jl:297-314), without the ŷs of an InternalModel."""
        y = np.einsum("bij,bj->bi", self._Chat, xhat0) + self.yop
        return y + np.einsum("bij,bj->bi", self._Dhd, d0) if self.nd > 0 else y

    def _set_direct(self, direct):
        """The form of the estimator about to be attached, settled on the handle before the estimator itself goes to the
        device (`direct` of the mirror follows in _adopt_estimator, once the setter has succeeded).  The handle's flag
        (default: filter form) survives its setters, so it is told about a change only.  A handle without
        mpcqp_kf_set_direct cannot run the predictor form: NotImplementedError, and nothing has been sent to it."""
        direct = bool(direct)
        if direct != self._hd_direct:
            if not hasattr(self.hd, "kf_set_direct"):
                raise NotImplementedError("direct=False (predictor form): this handle has no mpcqp_kf_set_direct")
            self.hd.kf_set_direct(direct)
            self._hd_direct = direct

    def _has(self, entry):
        """Whether the handle's library exports mpcqp_<entry>.  A stand-in handle without `.lib` (the mirror tests') is asked
        for the method of that name instead."""
        lib = getattr(self.hd, "lib", None)
        return hasattr(self.hd, entry) if lib is None else hasattr(lib, "mpcqp_" + entry)

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
        i_ym = self._measured(i_ym, validate=False)
        Qhat, Rhat, P0 = self._cov(Qhat, self.nxh, "Q̂"), self._cov(Rhat, len(i_ym), "R̂"), self._cov(P0, self.nxh, "P̂_0")
        self._set_direct(direct)
        self.hd.kf_set_covariances(Qhat, Rhat, P0, i_ym)
        self._P0 = P0.copy()                        # P̂_0, for initstate (init_estimate_cov!)
        return self._adopt_estimator(EST_TIMEVARYING, i_ym, direct, xhat0)

    def setsteadykalmanfilter(self, Qhat, Rhat, i_ym=None, xhat0=None, direct=True):
        """The `SteadyKalmanFilter` from Q̂ and R̂ (see `setestimator(steady=…)`)."""
        if not self._has("kf_set_steady"):
            raise NotImplementedError("steady=dict(Qhat, Rhat): this handle has no mpcqp_kf_set_steady")
        i_ym = self._measured(i_ym, validate=False)
        Qhat, Rhat = self._cov(Qhat, self.nxh, "Q̂"), self._cov(Rhat, len(i_ym), "R̂")
        self._set_direct(direct)
        self.hd.kf_set_steady(Qhat, Rhat, i_ym)
        self._adopt_estimator(EST_STEADY, i_ym, direct, xhat0)
        self._warn_steady()
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
        i_ym = self._measured(i_ym)
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
        if not self._has("kf_set_poles"):
            raise NotImplementedError("luenberger=dict(poles): this handle has no mpcqp_kf_set_poles")
        p = _f64(np.broadcast_to(p, (self.B, self.nxh)))
        self._set_direct(direct)
        self.hd.kf_set_poles(p, i_ym)
        self._adopt_estimator(EST_LUENBERGER, i_ym, direct, xhat0)
        self._warn_luenberger()
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
        if self.est_kind == EST_STEADY:
            self.hd.kf_set_steady(self._cov(Qhat, self.nxh, "Q̂"), self._cov(Rhat, len(self.i_ym), "R̂"), self.i_ym)
            return self._warn_steady()
        if self.est_kind != EST_TIMEVARYING:
            raise ValueError("Q̂ and R̂ can only be replaced on a KalmanFilter (setestimator(covariances=…)) or a "
                             "SteadyKalmanFilter built from them (setestimator(steady=…))")
        self.hd.kf_set_covariances(self._cov(Qhat, self.nxh, "Q̂"), self._cov(Rhat, len(self.i_ym), "R̂"), None, self.i_ym)

    def setstate(self, xhat, Phat=None):
        """`setstate!(estim, x̂, P̂)` (src/estimator/execute.jl): x̂ (nx̂,) or (B,nx̂) in engineering units; P̂ only on a
        time-varying KalmanFilter."""
        kind = self._need_estimator()
        if kind == EST_MHE:                             # (a covariance raises there, as in the reference)
            self.mhe.setstate(self._bc(xhat, self.nxh, "x̂"), Phat)
            return self
        if Phat is not None:
            if kind == EST_LUENBERGER:
                raise ValueError("Luenberger does not compute an estimation covariance matrix P̂.")
            if kind != EST_TIMEVARYING:
                raise ValueError("the SteadyKalmanFilter has no covariance estimate P̂ to set")
            self.hd.kf_set_state_covariance(self._cov(Phat, self.nxh, "P̂"))
        self.xhat0 = _f64(self._bc(xhat, self.nxh, "x̂") - self.xhop).copy()
        return self

    def _y0m(self, ym):
        """y0m of a period, or None for `ym = nothing`; warns once when members miss the correction (kalman.jl:245-251)."""
        y0m = None if ym is None else self._y0m_of(ym)
        self._warn_kf_nan(self.B if y0m is None else int(np.isnan(y0m).any(axis=1).sum()), self.B, "estimators")
        return y0m

    def _y0m_of(self, ym):
        return self._bc(ym, len(self.i_ym), "ym") - self.yop[:, self.i_ym]

    def _d0(self, d):
        return None if self.nd == 0 else self._bc(d, self.nd, "d") - self.dop

    @staticmethod
    def _warn_kf_nan(n, total, what):
        if n:         # kalman.jl:245-251
            warnings.warn("NaN values in the Kalman filter measurements ym: skipping correction step "
                          f"({n} of {total} {what})", RuntimeWarning)

    @staticmethod
    def _warn_im_nan(n, total, what):
        if n:
            warnings.warn(f"NaN values in the internal model measurements ym: assigning them ŷs=0 ({n} of {total} {what})",
                          RuntimeWarning)

    def preparestate(self, ym, d=None):
        """`preparestate!` (src/estimator/execute.jl:334-345 -> correct_estimate_obsv!,
        kalman.jl:284-295): x̂0 += K̂ (y0m - Ĉm x̂0 - D̂dm d0).  Returns x̂ = x̂0 + x̂op.  Members with a NaN in `ym` (all of
        them with ym=None) keep their x̂0.  Predictor form (direct=False): nothing to do, no device call."""
        kind = self._need_estimator()
        if kind == EST_MHE:                             # preparestate!(estim::MovingHorizonEstimator): one solve (direct form)
            return self._mhe_period(self.mhe.preparestate(ym, d), self.direct)
        if kind == EST_INTERNAL:                        # correct_estimate!(estim::InternalModel): ŷs and Ŷs, x̂0 stays
            y0m = self._y0m_of(ym)
            self._warn_im_nan(int((~np.isfinite(y0m)).any(axis=1).sum()), self.B, "estimators")
            self.hd.im_correct(self.xhat0, y0m, self._d0(d))
        elif self.direct:
            y0m = self._y0m(ym)
            self.hd.kf_correct(self.xhat0, y0m, self._d0(d))      # (y0m None: a time-varying filter records the miss, status 1)
        return self.xhat0 + self.xhop

    def updatestate(self, u, ym=None, d=None):
        """`updatestate!` (src/estimator/execute.jl:374-386 -> predict_estimate_obsv!,
        kalman.jl:298-309): x̂0 <- Â x̂0 + B̂u u0 + B̂d d0 + f̂op - x̂op.  Predictor form (direct=False): the correction with
        `ym` first (kalman.jl:276-281, 520-525; ym=None or NaN rows: skipped), then the prediction."""
        kind = self._need_estimator()
        if kind == EST_MHE:
            if ym is None:
                raise ValueError("updatestate: the MovingHorizonEstimator needs ym")
            return self._mhe_period(self.mhe.updatestate(u, ym, d), not self.direct)
        u0, d0 = self._bc(u, self.nu, "u") - self.uop, self._d0(d)
        if kind == EST_INTERNAL:
            self.hd.im_update(self.xhat0, u0, d0)
        elif self.direct:
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

    @staticmethod
    def _warn_qp_status(status, total, what):
        nerr, nwarn = int(np.sum(status == STATUS_ERROR)), int(np.sum(status == STATUS_ITERATION_LIMIT))
        if nerr:      # @error branch, src/controller/execute.jl:484-489
            warnings.warn(f"MPC terminated without solution: returning last solution shifted ({nerr} of {total} {what})", RuntimeWarning)
        if nwarn:     # @warn branch, :491-496
            warnings.warn(f"MPC termination status not OPTIMAL: keeping solution anyway ({nwarn} of {total} {what})", RuntimeWarning)

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
        kind = self._need_estimator()
        y0m, d0 = self._y0m_of(ym), self._d0(d)
        xh = _f64(self.xhat0).copy()
        st = self.hd.est_initstate(xh, self.lastu0, y0m, d0)
        if kind == EST_MHE:
            self.mhe.initstate(xh + self.xhop, self.lastu0 + self.uop, None if self.nd == 0 else d0 + self.dop)
        else:
            self.xhat0 = xh
            if kind == EST_TIMEVARYING:
                self.hd.kf_set_state_covariance(self._P0)
        self.init_status = st
        n = int(np.count_nonzero(st))
        if n:
            warnings.warn(("initstate!: I - Â or I - Âs is singular, x̂0 and x̂s are left unchanged " if kind == EST_INTERNAL else
                           "initstate!: [I - Â; Ĉm] has no full column rank, the estimate x̂0 is left unchanged ")
                          + f"({n} of {self.B} estimators)", RuntimeWarning)
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
        self._warn_qp_status(self.status, B, "controllers")
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
        kind = self._need_estimator()
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
        est_status = None
        if kind == EST_MHE:       # the estimator's device state went on with the run; its host mirror follows
            from .mhe import GET_STATUS
            est = self.mhe
            est.x̂0, est.status = xh, est.handle.get(GET_STATUS)
            est_status = self.hd.sim_est_status(N).T.copy()
            self.sim_x0, self.lastu0 = x0, lu
        else:
            self.sim_x0, self.xhat0, self.lastu0 = x0, xh, lu
        self.Z = np.full((B, self.nZ), np.nan) if fused else Z
        self.status = status[:, -1].copy()
        self.iters = np.zeros(B, np.int32)
        self._warn_qp_status(status, B * N, "controller periods")      # (once per run)
        if kind == EST_MHE:
            self._warn_mhe(est_status, B * N, "estimator periods")
        else:
            nmiss = int(np.isnan(rec["Y"][:, :, self.i_ym]).any(axis=2).sum())
            (self._warn_im_nan if kind == EST_INTERNAL else self._warn_kf_nan)(nmiss, B * N, "estimator periods")
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
        kind = self.est_kind
        yk = self._yhat_now(xhat0, d0)
        if kind == EST_INTERNAL:                    # the Ŷs and ŷs of the last correction: what the step used (predictstoch!)
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
        if kind in (EST_TIMEVARYING, EST_STEADY):
            # the estimator's covariance (P̂∞ of a steady solve), gain and per-estimator status
            info["P̂"], info["K̂"], info["kf_status"] = self.hd.kf_covariance(), self.hd.kf_gain(), self.hd.kf_status()
            if kind == EST_STEADY and self._has("kf_steady_path"):
                info["kf_steady_path"] = self.hd.kf_steady_path()      # 1: solved by the square-root form (semidefinite Q̂)
        elif kind == EST_LUENBERGER:               # the placed gain, per-member status and sweep counts
            info["K̂"], info["kf_status"], info["place_sweeps"] = self.hd.kf_gain(), self.hd.kf_status(), self.hd.kf_place_sweeps()
        elif kind == EST_MHE:
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
                ye = np.concatenate([self._yhat_now(xhat0, d0), info["Ŷ"]], axis=1).reshape(self.B, Hp + 1, ny)
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
            self._shift_xhop(vec(xhop, self.nxh, None))
        self.fhop = vec(fhop, self.nxh, self.fhop)
        if self.mhe is not None:      # the estimator moves its windows, x̂0 and bounds itself (BatchMHE.setmodel)
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
