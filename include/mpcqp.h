/*
 * mpcqp.h -- C-ABI of the MI355X-native batched LinMPC step (condense + QP solve).
 *
 * Drop-in boundary for the LinMPC `moveinput!` hot path of JuliaControl/ModelPredictiveControl.jl
 * v2.11.0 (citations are relative to /root/reference).  The reference has no FFI of its own for
 * this path: the seam is the `optim::JuMP.GenericModel` field (src/controller/linmpc.jl:14,245)
 * driven by five JuMP calls -- set_normalized_rhs (src/controller/transcription.jl:845),
 * set_objective_coefficient (src/controller/execute.jl:513), set_start_value
 * (src/controller/transcription.jl:1005), optimize! (src/controller/execute.jl:472) and value
 * (:502).  This library replaces, for a batch of B independent controllers of identical
 * dimensions:
 *
 *     mpcqp_set_model    <->  init_predmat   src/controller/transcription.jl:115-194   (kernel K1)
 *     mpcqp_set_weights  <->  init_quadprog  src/controller/construct.jl:837-845       (kernel K2)
 *     mpcqp_set_bounds   <->  setconstraint! src/controller/construct.jl:324-559 (bound vectors,
 *                             softness columns, Inf = absent row: transcription.jl:692-700)
 *     mpcqp_step         <->  initpred! + linconstraint! + optim_objective! + getinput!
 *                             src/controller/execute.jl:247-277, transcription.jl:811-848,
 *                             execute.jl:466-505, execute.jl:536-546                   (kernel K3)
 *
 * Conventions
 *   - plain C, no C++/torch types; every array is float64 unless stated.
 *   - batch layout: problem-major, COLUMN-major inside a problem, i.e. exactly a Julia
 *     Array{Float64,3} of size (rows, cols, B) / Array{Float64,2} of size (n, B) passed as
 *     Ptr{Float64} with zero copy.
 *   - all signals are DEVIATION variables (operating points already subtracted), as the
 *     reference stores them (con.U0min = umin - Uop, src/controller/construct.jl:359).
 *   - +-Inf in a bound means "row absent" (the i_b rule).  A NULL bound pointer means the whole
 *     group is absent; a NULL softness pointer means the reference defaults (0 for u and Δu,
 *     1 for y and x̂end, src/controller/construct.jl:909-913).
 *   - host entry points (`*_host` suffix omitted) take HOST pointers and are synchronous, like
 *     `moveinput!`; the `_device` twins take DEVICE pointers of the handle's GPU, enqueue on the
 *     given hipStream_t (passed as void*) and return immediately -- this is what a resident
 *     closed loop (and bench.py) uses.
 *   - return value: 0 = ok, negative = API misuse (mirrors the DimensionMismatch/ArgumentError
 *     of validate_args, src/controller/construct.jl:702-710).  Nothing throws across the ABI.
 *   - per-problem solver outcome in status[]: see MPCQP_STATUS_*; on MPCQP_STATUS_ERROR the
 *     returned Z̃ is the shifted warm start (src/controller/execute.jl:499-500).
 *   - a handle is NOT thread-safe (neither is a LinMPC: its buffers are mutated in place,
 *     src/controller/construct.jl:4-16); distinct handles are independent.
 */
#ifndef MPCQP_H
#define MPCQP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpcqp_handle_s* mpcqp_handle;

/* error codes (return values) */
#define MPCQP_OK                 0
#define MPCQP_ERR_NULL          -1   /* required pointer is NULL                              */
#define MPCQP_ERR_DIMS          -2   /* inconsistent dimensions (DimensionMismatch)           */
#define MPCQP_ERR_ARG           -3   /* illegal value (ArgumentError)                         */
#define MPCQP_ERR_UNSUPPORTED   -4   /* legal in the reference, not built here (see DESIGN)   */
#define MPCQP_ERR_ORDER         -5   /* call order: model/weights/bounds before step          */
#define MPCQP_ERR_DEVICE        -6   /* HIP runtime error (mpcqp_last_hip_error for detail)   */
#define MPCQP_ERR_NOMEM         -7

/* per-problem solver status, cf. issolved/iserror src/general.jl:52-61 */
#define MPCQP_STATUS_OPTIMAL          0
#define MPCQP_STATUS_ITERATION_LIMIT  1   /* solution kept (@warn branch, execute.jl:491-496)  */
#define MPCQP_STATUS_ERROR            2   /* infeasible / numerical: warm start returned       */

/* flags of mpcqp_dims.flags */
#define MPCQP_FLAG_RY_CONSTANT   (1u << 0)  /* Ry is (ny,B): ry held over Hp, like R̂y=repeat(ry,Hp) */
#define MPCQP_FLAG_COLD_START    (1u << 1)  /* ignore Ztilde on input: warm start = 0              */
#define MPCQP_FLAG_KEEP_QP       (1u << 2)  /* keep q̃ and F of the last step for mpcqp_get         */
#define MPCQP_FLAG_WARM_DUAL     (1u << 3)  /* closed loop: keep the multipliers between steps and  */
                                            /* start the next solve around them (and the shifted Z̃) */
#define MPCQP_FLAG_NO_POLISH     (1u << 4)  /* skip the active-set polish of the interior-point iterate */
                                            /* (measurements only: the polish is what bounds the error) */
#define MPCQP_FLAG_KEEP_ITERATE  (1u << 5)  /* diagnostics: a solve that stops at max_iter returns its iterate as it is  */
                                            /* (status ITERATION_LIMIT) instead of taking the error branch -- with       */
                                            /* mpcqp_set_iteration_limit(k) this exposes the k-th interior-point iterate; */
                                            /* mpcqp_prepare compares the first iterates of an on-demand kernel with the  */
                                            /* runtime-dimension kernel's this way                                        */

typedef struct {
    int32_t  batch;     /* B: number of independent controllers                              */
    int32_t  nxhat;     /* augmented states nx̂ (estimator/construct.jl:305-323)               */
    int32_t  nu, ny, nd;
    int32_t  Hp;        /* prediction horizon                                                 */
    int32_t  Hc;        /* number of free moves = length(nb) (construct.jl:629-660)           */
    const int32_t* nb;  /* [Hc] move-blocking lengths, sum == Hp; NULL = [1,..,1,Hp-Hc+1]     */
    int32_t  neps;      /* 1 iff Cwt is finite (slack variable ϵ present, construct.jl:903)   */
    int32_t  device;    /* HIP device ordinal                                                 */
    uint32_t flags;     /* MPCQP_FLAG_*                                                       */
    int32_t  max_iter;  /* interior-point iteration cap, 0 = default (80)                      */
    double   gap_tol;   /* absolute mean complementarity target, 0 = default (1e-12)          */
    double   res_tol;   /* relative primal/dual residual target, 0 = default (1e-11)          */
    double   dual_reg;  /* dual proximal regularisation δ, 0 = default (1e-12)                */
} mpcqp_dims;

/* sizes derived from dims (for allocating caller-side arrays) */
typedef struct {
    int32_t nZ;      /* nu*Hc + neps  (decision vector Z̃ = [ΔU; ϵ])                         */
    int32_t nDU;     /* nu*Hc                                                                */
    int32_t nU;      /* nu*Hp                                                                */
    int32_t nY;      /* ny*Hp                                                                */
    int32_t nD;      /* nd*Hp                                                                */
} mpcqp_sizes;

const char* mpcqp_version(void);
const char* mpcqp_strerror(int code);
const char* mpcqp_last_hip_error(void);

int mpcqp_create(const mpcqp_dims* dims, mpcqp_handle* out);
int mpcqp_destroy(mpcqp_handle h);
int mpcqp_get_sizes(mpcqp_handle h, mpcqp_sizes* out);

/* Augmented model of every controller (estim.Â, B̂u, Ĉ, B̂d, D̂d, f̂op - x̂op;
 * src/controller/transcription.jl:118,190).  Ahat (nx̂,nx̂,B), Bu (nx̂,nu,B), C (ny,nx̂,B),
 * Bd (nx̂,nd,B) / Dd (ny,nd,B) (NULL iff nd == 0), fop_minus_xop (nx̂,B) or NULL (= 0).
 * Runs K1 (prediction tables) and, when weights are already set, K2 (Hessian) -- this is also
 * the `setmodel!` path (src/controller/execute.jl:684-790).                                  */
int mpcqp_set_model(mpcqp_handle h, const double* Ahat, const double* Bu, const double* C,
                    const double* Bd, const double* Dd, const double* fop_minus_xop);

/* Diagonal weights: Mdiag (nY,B), Ndiag (nDU,B), Ldiag (nU,B), Cwt (B) (ignored when neps == 0).
 * (`Diagonal(repeat(Mwt,Hp))` etc., src/controller/linmpc.jl:236-238.)  Runs K2 when the model
 * is set.  Block-diagonal M_Hp: mpcqp_set_output_weight_blocks; dense M_Hp / N_Hc / L_Hp: mpcqp_set_dense_weights. */
int mpcqp_set_weights(mpcqp_handle h, const double* Mdiag, const double* Ndiag,
                      const double* Ldiag, const double* Cwt);

/* Transcription of the handle (the `transcription` keyword of LinMPC, src/controller/linmpc.jl:205-216):
 *   MPCQP_SINGLE_SHOOTING    Z = ΔU, the condensed QP (default; kernels K1-K3)
 *   MPCQP_MULTIPLE_SHOOTING  Z = [ΔU; X̂0], the model as equality constraints (src/controller/transcription.jl:196-240,
 *                            303-414, 913-928): solved in its stage form by a Riccati recursion inside the interior-point
 *                            iteration -- what the reference recommends when cond(H̃) is large (unstable plants, long
 *                            horizons; src/controller/construct.jl:855-866).  Same objective, bounds and softness, hence the
 *                            same optimal ΔU; mpcqp_step writes Z̃ = [ΔU; ϵ] as always and X̂0 is read with
 *                            mpcqp_get(MPCQP_GET_XHAT_MS).
 * Not every handle can run MultipleShooting: mpcqp_transcription_supported returns 0 when it can, else a bit mask
 * (1 a weight matrix of mpcqp_set_dense_weights that couples different stages -- such a cost is not block-tridiagonal and no
 * Riccati recursion solves it -- or output-weight blocks beyond ny = 256; 4 stage data beyond 160 KB of LDS.  2, custom linear
 * constraints, and 8, MPCQP_FLAG_KEEP_QP / _WARM_DUAL, are kept as values but no longer set: the stage-structured kernel takes
 * them).  A step of an unsupported MultipleShooting handle returns MPCQP_ERR_UNSUPPORTED, and so do mpcqp_prepare and
 * mpcqp_kernel_kind for it (the Python mirror then keeps the SingleShooting kernels and says so).  The fused Kalman loop
 * (mpcqp_loop_device) runs on the stage-structured kernel too (round 6; MPCQP_ERR_UNSUPPORTED before).
 *
 * Size: a SingleShooting handle with nZ̃ = nu Hc + nϵ > 256 has no condensed kernel (its Newton matrix does not fit the
 * LDS); it runs the same QP on the stage-structured kernel, whose cost is linear in the horizons -- the reference has no
 * size limit (transcription.jl:2-4).  mpcqp_kernel_kind reports MPCQP_KERNEL_MS for it; the condensed tables
 * (MPCQP_GET_HESSIAN, _STEPRESP, _KMAT, _BVEC) do not exist for such a handle (MPCQP_ERR_UNSUPPORTED).  The same holds for a
 * handle of nZ̃ <= 256 whose condensed problem does not fit the 160 KB of LDS of a CU (nZ̃ beyond ~165 at nu = ny = 3 ... 4): its
 * steps run on the stage-structured kernel (MPCQP_KERNEL_MS), its prediction tables exist, its packed Hessian does not. */
#define MPCQP_SINGLE_SHOOTING    0
#define MPCQP_MULTIPLE_SHOOTING  1
int mpcqp_set_transcription(mpcqp_handle h, int32_t transcription);
int mpcqp_transcription_supported(mpcqp_handle h);

/* Interior-point iteration cap of the following steps (0 = default, 80); the analogue of the solver time limit the
 * reference sets from Ts (src/controller/linmpc.jl:329, src/general.jl:110-121).  With MPCQP_FLAG_KEEP_ITERATE a capped
 * solve returns its iterate (diagnostics). */
int mpcqp_set_iteration_limit(mpcqp_handle h, int32_t max_iter);

/* Replace the MPCQP_FLAG_* set of the handle (they are read at every step): e.g. switch between a
 * set point held over the horizon (Ry (ny,B), MPCQP_FLAG_RY_CONSTANT) and a full R̂y (nY,B), or
 * between cold and warm starts.  Unknown bits: MPCQP_ERR_ARG.                                    */
int mpcqp_set_flags(mpcqp_handle h, uint32_t flags);

/* Block-diagonal output weight M_Hp = blkdiag(M_1, ..., M_Hp) with symmetric ny x ny blocks,
 * Mblk (ny,ny,Hp,B); replaces Mdiag of mpcqp_set_weights (call that first: N, L, C come from it).
 * This is the `M_Hp=` keyword of LinMPC (src/controller/linmpc.jl:205-214) for the weights the
 * reference's own tests use: a terminal cost, M_Hp = blkdiag(M, ..., M, P)
 * (test/3_test_predictive_control.jl:498-527).  NULL returns to the diagonal weight.  A weight that
 * couples different prediction steps goes through mpcqp_set_dense_weights.                        */
int mpcqp_set_output_weight_blocks(mpcqp_handle h, const double* Mblk);

/* Dense (Hermitian) weight matrices, the reference's M_Hp=, N_Hc=, L_Hp= keywords in full generality
 * (src/controller/construct.jl:45-93, 837-845; linmpc.jl:205-214): M_Hp (nY,nY,B) may couple different
 * prediction steps, N_Hc (nDU,nDU,B) different moves, L_Hp (nU,nU,B) different inputs/steps.  Each replaces the
 * corresponding diagonal of mpcqp_set_weights (NULL: keep the diagonal / block form); call after
 * mpcqp_set_weights.  H~ is rebuilt (K2, runtime-dimension kernel).  With a dense M_Hp or L_Hp the step
 * evaluates M (F - R^y) and L (Tu lastu0 - R^u) densely: on an on-demand specialisation that carries these products
 * (mpcqp_prepare AFTER this call; the kernels compiled into the library do not) or on the runtime-dimension kernel; a
 * dense N_Hc only changes H~ and keeps every specialised step kernel.
 * The stage-structured kernel (MultipleShooting, and SingleShooting handles beyond the condensed kernels) takes a matrix
 * that is STAGE-SEPARABLE: every entry outside its diagonal blocks -- ny x ny per prediction step for M_Hp, nu x nu per
 * free move for N_Hc, nu x nu per step for L_Hp -- is exactly 0.0 in every member of the batch (an L_Hp entry that couples
 * two steps of one move-blocking interval is not separable) and every diagonal block is symmetric, entry for entry.  The
 * matrices are classified here, from the host pointers; one that couples stages, or has a block that is not symmetric,
 * gives reason 1 of mpcqp_transcription_supported.  A stage-separable M_Hp given here takes precedence over the blocks of
 * an earlier mpcqp_set_output_weight_blocks on that kernel (its blocks are copied out and uploaded here, once); M_Hp =
 * NULL gives the earlier blocks back.                                                                                 */
int mpcqp_set_dense_weights(mpcqp_handle h, const double* M_Hp, const double* N_Hc, const double* L_Hp);

/* Custom linear inequality constraints over k .. k+Hp (keywords Wy, Wu, Wd, Wr of LinMPC,
 * src/controller/construct.jl:666-694; relaxW :1086-1160; linconstraint_custom!,
 * src/controller/execute.jl:337-364):
 *     wmin <= Wy ŷe + Wu ue + Wd d̂e + Wr r̂e <= wmax,     nw rows per step, Hp+1 steps
 * Wy (nw,ny,B), Wu (nw,nu,B), Wd (nw,nd,B) or NULL, Wr (nw,ny,B) or NULL.  The constraints are
 * written on engineering values while this ABI works in deviation variables: w_op (nw,B) =
 * Wy yop + Wu uop + Wd dop + Wr yop (NULL = 0) carries the operating points.  r̂e(k): see
 * mpcqp_set_current_setpoint.  nw = 0 removes them.
 * Bounds and softness (default 1, like c_wmin/c_wmax): Wmin, Wmax, C_wmin, C_wmax (nw (Hp+1), B),
 * NULL = absent (±Inf).  Problems with custom constraints run on an on-demand specialisation that has the rows
 * compiled in (mpcqp_prepare after this call) or on the runtime-dimension kernel; under MPCQP_MULTIPLE_SHOOTING, and
 * for a SingleShooting problem beyond the LDS (see mpcqp_set_transcription), on the stage-structured kernel, which
 * has its own instantiation with the rows (a handle without them keeps the kernel it had).                    */
int mpcqp_set_custom_constraints(mpcqp_handle h, int nw, const double* Wy, const double* Wu,
                                 const double* Wd, const double* Wr, const double* w_op);
int mpcqp_set_custom_bounds(mpcqp_handle h, const double* Wmin, const double* Wmax,
                            const double* C_wmin, const double* C_wmax);
/* r̂e(k), the first ny entries of the extended set point vector the Wr term multiplies, is the CURRENT
 * set point ry(k) (src/controller/execute.jl:351).  With a held set point (MPCQP_FLAG_RY_CONSTANT) the
 * library has it already; with a full R̂y trajectory pass ry(k) - yop here, (ny,B), before the step
 * (NULL: back to the first block of R̂y).                                                          */
int mpcqp_set_current_setpoint(mpcqp_handle h, const double* ry_now);

/* Bounds (deviation values) and softness (ECR) vectors; shapes (nU,B), (nDU,B), (nY,B), (nx̂,B).
 * Field order follows ControllerConstraint (src/controller/construct.jl:126-199).            */
typedef struct {
    const double *U0min, *U0max;       /* (nU,B)  */
    const double *DUmin, *DUmax;       /* (nDU,B) */
    const double *Y0min, *Y0max;       /* (nY,B)  */
    const double *x0min, *x0max;       /* (nx̂,B)  terminal */
    const double *C_umin, *C_umax;     /* (nU,B)  softness, NULL = 0 */
    const double *C_dumin, *C_dumax;   /* (nDU,B) NULL = 0 */
    const double *C_ymin, *C_ymax;     /* (nY,B)  NULL = 1 */
    const double *c_x0min, *c_x0max;   /* (nx̂,B)  NULL = 1 */
} mpcqp_bounds;
int mpcqp_set_bounds(mpcqp_handle h, const mpcqp_bounds* bounds);

/* One control period for the whole batch (== B calls of moveinput!, execute.jl:59-80).
 *   xhat0  (nx̂,B)  estim.x̂0                       lastu0 (nu,B)  u(k-1) - uop
 *   Ry     (nY,B) or (ny,B) with MPCQP_FLAG_RY_CONSTANT: R̂y - Yop (deviation setpoints)
 *   Ru     (nU,B) R̂u - Uop, or NULL (= 0, the default R̂u = Uop)
 *   d0     (nd,B), Dhat0 (nD,B): measured disturbance and its preview (NULL iff nd == 0)
 *   Ztilde (nZ,B) in: previous optimum (shifted inside, transcription.jl:997-1007);
 *                 out: optimum (or the shifted warm start when status == ERROR)
 *   u0     (nu,B) out: u(k) - uop = Z̃[1:nu] + lastu0 (execute.jl:536-546)
 *   status (B) int32, iters (B) int32 (NULL allowed for iters)
 *   Yhat0  (nY,B) optional out: Ŷ0 = Ẽ Z̃ + F (predict!, transcription.jl:1136-1145); NULL ok
 */
int mpcqp_step(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* Ry,
               const double* Ru, const double* d0, const double* Dhat0, double* Ztilde,
               double* u0, int32_t* status, int32_t* iters, double* Yhat0);

/* Same with DEVICE pointers on the handle's GPU, asynchronous on `stream` (a hipStream_t). */
int mpcqp_step_device(mpcqp_handle h, const double* xhat0, const double* lastu0,
                      const double* Ry, const double* Ru, const double* d0, const double* Dhat0,
                      double* Ztilde, double* u0, int32_t* status, int32_t* iters,
                      double* Yhat0, void* stream);

/* One control period of a resident closed loop in ONE launch: preparestate! (SteadyKalmanFilter
 * correction with the measurement y0m (nym,B), kalman.jl:284-295), moveinput! and updatestate!
 * (kalman.jl:298-309, with the input just computed) inside the step kernel.  xhat0 (nx̂,B) is updated
 * in place: in = x̂0(k|k-1), out = x̂0(k+1|k); everything else as mpcqp_step_device (u0 of one period
 * is lastu0 of the next: swap the two buffers).  Needs mpcqp_kf_set.  DEVICE pointers.          */
int mpcqp_loop_device(mpcqp_handle h, double* xhat0, const double* y0m, const double* lastu0,
                      const double* Ry, const double* Ru, const double* d0, const double* Dhat0,
                      double* Ztilde, double* u0, int32_t* status, int32_t* iters, double* Yhat0,
                      void* stream);

/* Re-run K1+K2 on the resident model/weights (timing of the setmodel! path). */
int mpcqp_recondense_device(mpcqp_handle h, void* stream);

/* Read back condensed quantities for parity tests / getinfo (host pointers).
 *   HESSIAN  H̃ (nZ,nZ,B)                       construct.jl:837-845
 *   STEPRESP Σ_m = Ĉ S(m) B̂u (ny,nu,Hp,B)       transcription.jl:134-139 (E is block-Toeplitz in it)
 *   KMAT     K (nY,nx̂,B)                        transcription.jl:143-147
 *   BVEC     B (nY,B)                           transcription.jl:184-192
 *   QTILDE   q̃ (nZ,B), FVEC F (nY,B) of the last step (needs MPCQP_FLAG_KEEP_QP); the condensed definitions and layout
 *            (Ŷ0 = E ΔU + F; q̃ over Z̃ = [ΔU; ϵ]) also when the step ran on the stage-structured kernel, which never forms E
 */
#define MPCQP_GET_HESSIAN   1
#define MPCQP_GET_STEPRESP  2
#define MPCQP_GET_KMAT      3
#define MPCQP_GET_BVEC      4
#define MPCQP_GET_QTILDE    5
#define MPCQP_GET_FVEC      6
#define MPCQP_GET_AUDIT     7   /* (4,B) of the last step: final complementarity gap mu, dual residual / its scale, primal
                                 * residual / its scale, 1.0 if the returned point passed the active-set polish's KKT check */
#define MPCQP_GET_XHAT_MS   8   /* (nx̂,Hp,B): X̂0(k+1..k+Hp) of the last MultipleShooting step -- the second block of the
                                 * reference's decision vector Z = [ΔU; X̂0] (src/controller/transcription.jl:5-7) */
#define MPCQP_GET_MS_DEFECT 9   /* (B): max |E_S Z + F_S| (defect of the model equations, transcription.jl:303-327) of it */
#define MPCQP_GET_KF_COV    10  /* (nx̂,nx̂,B): P̂ of the time-varying KalmanFilter, P̂∞ after mpcqp_kf_set_steady (MPCQP_ERR_ORDER on a gain from mpcqp_kf_set) */
#define MPCQP_GET_KF_GAIN   11  /* (nx̂,nym,B): K̂ the estimator steps use -- the steady gain or K̂(k) of the last correction */
#define MPCQP_GET_IM_XS     13  /* (nxs,B): x̂s of the InternalModel estimator (mpcqp_im_set) */
#define MPCQP_GET_IM_YS     14  /* (ny,B):  ŷs of its last correction (0 in the unmeasured rows) */
#define MPCQP_GET_IM_YHATS  15  /* (nY,B):  Ŷs of its last correction, the term the steps add to the model's B */
#define MPCQP_GET_EXPLICIT_LAW 12 /* (nZ, 1+nx̂+nu+ny+nd, B): the law [g0 Gx Gu Gr Gd] of mpcqp_explicit_prepare(h, MPCQP_EXPLICIT_LAW) */
/* the resident model, in the layouts of mpcqp_set_model (what mpcqp_set_model_continuous wrote, or the arrays of the last
 * mpcqp_set_model): Â (nx̂,nx̂,B), B̂u (nx̂,nu,B), Ĉ (ny,nx̂,B), B̂d (nx̂,nd,B), D̂d (ny,nd,B) -- MPCQP_ERR_ARG for the last two
 * when nd = 0 -- and f̂op - x̂op (nx̂,B), zeros when none is set */
#define MPCQP_GET_MODEL_AHAT 16
#define MPCQP_GET_MODEL_BU   17
#define MPCQP_GET_MODEL_C    18
#define MPCQP_GET_MODEL_BD   19
#define MPCQP_GET_MODEL_DD   20
#define MPCQP_GET_MODEL_DOP  21
/* the remaining prediction tables of K1 (init_predmat, transcription.jl:115-194), as they lie on the device (row-major inside a
 * member unless said otherwise).  MPCQP_ERR_UNSUPPORTED on a handle whose problem only the stage-structured kernel takes
 * (nothing is condensed); MPCQP_ERR_ORDER before mpcqp_set_model and -- the last four -- while the terminal tables are not
 * built (they are built with the first finite x̂ bound of mpcqp_set_bounds); MPCQP_ERR_ARG for GDTAB / XDTAB when nd = 0.
 *   GDTAB  [B][Hp][ny][nd]   block t = Ĉ Â^t B̂d          (G, and J below its diagonal: transcription.jl:172-179)
 *   XDTAB  [B][Hp][nx̂][nd]   block t = Â^t B̂d            (gx̂ = block Hp-1, jx̂ block j = block Hp-j-1: transcription.jl:167, 180)
 *   EXHAT  [B][Hc][nx̂][nu]   block j = S(Hp - j_j - 1) B̂u, j_j the first step of move-blocking interval j (transcription.jl:164)
 *   KXHAT  [B] nx̂ x nx̂ column-major   Â^Hp              (transcription.jl:142)
 *   BXHAT  [B][nx̂]           S(Hp-1)(f̂op - x̂op), zeros when none is set      (transcription.jl:191) */
#define MPCQP_GET_GDTAB      22
#define MPCQP_GET_XDTAB      23
#define MPCQP_GET_EXHAT      24
#define MPCQP_GET_KXHAT      25
#define MPCQP_GET_BXHAT      26
int mpcqp_get(mpcqp_handle h, int which, double* out);
/* Which form of K1 builds this handle's prediction tables in this process: 0 the LDS loops, 1 the chains of
 * v_mfma_f64_16x16x4 (nx̂ <= 16, ny <= 16, nu + 1 + nd <= 16 and nx̂ >= MPCQP_K1_MFMA_MIN_NX, default 10; the environment
 * variable of that name, read once, moves the threshold).  Both forms write the same tables. */
int mpcqp_predmat_form(mpcqp_handle h);

/* ---- LinModel(sys, Ts) and augment_model for the whole batch, on the device --------------------------------------------
 * What the reference does on the host before LinMPC(model) exists: LinModel(sys, Ts) (src/model/linmodel.jl:165-198) turns a
 * continuous model into a discrete one -- c2d(sysu, Ts, :zoh) for the manipulated inputs, c2d(sysd, Ts, :tustin) for the
 * measured disturbances, stacked as [sysu_dis sysd_dis] -- and augment_model (src/estimator/construct.jl:305-323, with
 * init_estimstoch / init_integrators :172-252) appends the integrators of nint_u / nint_ym.  Here every member of the batch is
 * discretised and augmented in one launch (csrc/c2d_bodies.h), each with its own sample time.
 *
 *   inputs   A (nx,nx,B), Bu (nx,nu,B), C (ny,nx,B), Bd (nx,nd,B), Dd (ny,nd,B) continuous time, layouts of mpcqp_set_model;
 *            Ts (B); dop (nx_dis,B) = fop - xop of the discrete plant's states, may be NULL; Bd and Dd only with nd > 0
 *   spec     dimensions; nint_u [nu], nint_ym [nym] (NULL: no integrator), i_ym [nym] (NULL: 0 .. nym-1), shared by the batch;
 *            d_method: MPCQP_C2D_TUSTIN, the reference's treatment of the measured disturbances, or MPCQP_C2D_ZOH, a
 *            deviation that keeps one state vector
 *   ZOH      exp([[A, Bu(, Bd)], [0, 0]] Ts) = [[Φ, Γu(, Γd)], [0, I]]; Bd is in the block only with MPCQP_C2D_ZOH
 *   Tustin   (nd > 0 and MPCQP_C2D_TUSTIN) a = Ts/2, W = (I - aA)⁻¹: At = W (I + aA), Bt = W Bd Ts, Ct = C W, Dt = Dd + a C W Bd.
 *            The plant is then x = [xu; xd]: A = blkdiag(Φ, At), Bu = [Γu; 0], Bd = [0; Bt], C = [C, Ct], Dd = Dt, so that
 *            nx_dis = 2 nx; otherwise nx_dis = nx
 *   outputs  Â = [A, Bu Cs_u; 0, As], B̂u = [Bu; 0], Ĉ = [C, Cs_y], B̂d = [Bd; 0], D̂d = Dd, dop padded with zeros;
 *            nx̂ = nx_dis + Σ nint_u + Σ nint_ym (mpcqp_c2d_sizes).  Cs_u and Cs_y hold 0 and 1: those blocks are copies
 *   status   (B) int32: 0 written; 2 refused -- an input that is not finite, Ts not finite or <= 0, I - aA or the Padé
 *            denominator singular (a pivot at or below 64 eps times the largest), a scaled norm beyond 5.37 x 2^64, a result
 *            that is not finite.  NOTHING is written for a refused member: its outputs keep what they held (on a handle: the
 *            model it had; zeros on a handle that had none), and the other members are unaffected, bit for bit.
 * Not done: the reference's sminreal / minreal after the discretisation (they change the realisation, not the input-output
 * map), the pruning of integrators by default_nint and the observability check of augment_model -- nint_ym is what the
 * caller gives.  Limits (MPCQP_ERR_UNSUPPORTED): nx + nu (+ nd with MPCQP_C2D_ZOH) > 32; with the Tustin block also ny > 32 or
 * nd > 32; nx̂ > 64; a shard of mpcqp_multi_create; a library built without the kernel.  MPCQP_ERR_DIMS / _ARG: dimensions
 * below 1, nym > ny, an unknown d_method, a negative nint, i_ym out of range or repeated.
 *
 * mpcqp_c2d         host pointers, synchronous, no handle.
 * mpcqp_c2d_device  DEVICE pointers (status too), enqueued on `stream`.
 * mpcqp_set_model_continuous[_device]  the kernel writes straight into the handle's resident model; then everything
 *                   mpcqp_set_model / mpcqp_recondense_device do (K1, K2, the InternalModel's B + Ŷs, the refresh of a prepared
 *                   explicit factor) -- in the _device form on `stream`, with no host synchronisation; `in` and `status` are
 *                   DEVICE pointers there.  dop NULL: the handle has no f̂op - x̂op afterwards, as with mpcqp_set_model.  The
 *                   handle's batch, nx̂, nu, ny, nd must be those the spec implies: MPCQP_ERR_ARG otherwise, and the handle keeps
 *                   what it had, as after every other refusal.  Like mpcqp_set_model it does NOT re-solve estimator gains. */
#define MPCQP_C2D_TUSTIN 0
#define MPCQP_C2D_ZOH    1
typedef struct mpcqp_c2d_spec {
    int32_t batch, nx, nu, ny, nd, nym;
    int32_t d_method;
    const int32_t* nint_u;
    const int32_t* nint_ym;
    const int32_t* i_ym;
} mpcqp_c2d_spec;
typedef struct mpcqp_c2d_in {
    const double *A, *Bu, *C, *Bd, *Dd, *Ts, *dop;
} mpcqp_c2d_in;
typedef struct mpcqp_c2d_out {
    double *Ahat, *Bu, *C, *Bd, *Dd, *dop;
} mpcqp_c2d_out;
int mpcqp_c2d_sizes(const mpcqp_c2d_spec* spec, int32_t* nx_dis, int32_t* nxhat);
int mpcqp_c2d(const mpcqp_c2d_spec* spec, const mpcqp_c2d_in* in, const mpcqp_c2d_out* out, int32_t* status);
int mpcqp_c2d_device(const mpcqp_c2d_spec* spec, const mpcqp_c2d_in* in, const mpcqp_c2d_out* out, int32_t* status, void* stream);
int mpcqp_set_model_continuous(mpcqp_handle h, const mpcqp_c2d_spec* spec, const mpcqp_c2d_in* in, int32_t* status);
int mpcqp_set_model_continuous_device(mpcqp_handle h, const mpcqp_c2d_spec* spec, const mpcqp_c2d_in* in, int32_t* status,
                                      void* stream);

/* ---- ExplicitMPC (src/controller/explicitmpc.jl): the unconstrained LinMPC, H̃ factored once, Z̃ = -H̃⁻¹ q̃ every period ------
 * Two per-period paths on the handle of a controller WITHOUT constraints, beside mpcqp_step (which goes on working):
 *   mpcqp_explicit_step[_device]  inputs, layouts, MPCQP_FLAG_RY_CONSTANT / _KEEP_QP and Yhat0 of mpcqp_step[_device]; Ztilde
 *                                 is output only (ExplicitMPC has no warm start), there is no iteration count.  Per period
 *                                 F, q̃ and a product with the stored H̃⁻¹: no factorisation, no interior-point code.
 *   mpcqp_explicit_law[_device]   with set point, disturbance and R̂u = Uop held over the horizon -- the reference's default call
 *                                 moveinput!(mpc, ry, d), execute.jl:59-70 -- the period is the affine map
 *                                     Z̃ = g0 + Gx x̂0 + Gu lastu0 + Gr ry + Gd d0,    u0 = Z̃[1:nu] + lastu0
 *                                 ry (ny,B), d0 (nd,B) or NULL; Ztilde == NULL: u0 alone, from a table of nu rows per
 *                                 controller.  By definition the result of mpcqp_explicit_step with MPCQP_FLAG_RY_CONSTANT,
 *                                 Ru = NULL and Dhat0 = repeat(d0).  Several controllers per wavefront; bandwidth-bound.
 * mpcqp_explicit_prepare(h, with_law): with_law = 0 or MPCQP_EXPLICIT_LAW (the law tables are built too, by superposition:
 *   the explicit step on the 1+nx̂+nu+ny+nd unit inputs, on device buffers).  A kernel of its own factors every controller's
 *   H̃ on the device and keeps H̃⁻¹ (two substitutions with the factor were measured slower); nothing is computed
 *   on the host.
 *     MPCQP_ERR_ORDER        no model or no weights yet
 *     MPCQP_ERR_ARG          neps = 1, a bound or custom-row group on the handle (any array given to mpcqp_set_bounds /
 *                            mpcqp_set_custom_bounds counts, whatever it holds), or the MultipleShooting transcription --
 *                            "ExplicitMPC does not support constraints", and it has no Cwt / transcription keyword
 *     MPCQP_ERR_UNSUPPORTED  nZ̃ = nu Hc > 64 (one row of H̃ per lane; 65 is refused, not served), a handle without a
 *                            condensed Hessian (nZ̃ > 256, or a problem beyond the LDS of the condensed step kernels: the
 *                            handles mpcqp_get(MPCQP_GET_HESSIAN) refuses), or a library built without the kernels.  Every
 *                            other handle with nZ̃ <= 64 is served, whatever Hp: the period keeps 2 ny Hp + ny nu Hp +
 *                            nZ̃ (nZ̃ + 1) / 2 doubles in LDS, less than mpcqp_step does for the same handle
 *   A prepared handle refreshes the factor (and the law) inside mpcqp_set_model, mpcqp_set_weights,
 *   mpcqp_set_output_weight_blocks, mpcqp_set_dense_weights and mpcqp_recondense_device (there on the caller's stream): an
 *   explicit call never sees a stale factor.  A handle that receives a bound group, neps or MultipleShooting afterwards
 *   answers MPCQP_ERR_ORDER to the explicit calls (mpcqp_explicit_status included) until the rows are gone; its setters go on
 *   working and do not factor, and the first explicit call after the rows are gone factors again, on that call's stream.
 *   MPCQP_ERR_ORDER is also the answer of a handle that was never prepared, and of mpcqp_explicit_law without
 *   MPCQP_EXPLICIT_LAW.  mpcqp_explicit_prepare may be repeated (to add or drop the law); tables a running law call reads
 *   are rebuilt behind it.
 * The law kernel runs a persistent grid of 16 wavefronts per compute unit.  The environment variable MPCQP_EXPLICIT_WAVES = n
 *   (n >= 1) caps that grid at n wavefronts; it is read by mpcqp_explicit_prepare -- not by the per-period calls -- and the
 *   handle keeps the grid it was prepared with.  Results do not depend on it.
 * mpcqp_explicit_status: out [B], 0 factored, 2 H̃ not positive definite or not finite (where the reference's cholesky
 *   throws).  Such a controller gets status 2, Z̃ = 0 and u0 = lastu0 from every explicit call (Ŷ0 = F); the rest of the
 *   batch is unaffected, bit for bit -- the policy of the Kalman kernels.  status [B] of the per-period calls: 0 or 2. */
#define MPCQP_EXPLICIT_LAW           1
int mpcqp_explicit_prepare(mpcqp_handle h, int32_t with_law);
int mpcqp_explicit_status(mpcqp_handle h, int32_t* out);
int mpcqp_explicit_step(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* Ry, const double* Ru,
                        const double* d0, const double* Dhat0, double* Ztilde, double* u0, int32_t* status, double* Yhat0);
int mpcqp_explicit_step_device(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* Ry,
                               const double* Ru, const double* d0, const double* Dhat0, double* Ztilde, double* u0,
                               int32_t* status, double* Yhat0, void* stream);
int mpcqp_explicit_law(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* ry, const double* d0,
                       double* Ztilde, double* u0, int32_t* status);
int mpcqp_explicit_law_device(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* ry,
                              const double* d0, double* Ztilde, double* u0, int32_t* status, void* stream);

/* ---- next row: the Kalman filter steps on both sides of moveinput! ----------------
 * correction, correct_estimate_obsv! (src/estimator/kalman.jl:284-295):
 *       x̂0 += K̂ (y0m - Ĉm x̂0 - D̂dm d0)
 * prediction, predict_estimate_obsv! (src/estimator/kalman.jl:298-309):
 *       x̂0 <- Â x̂0 + B̂u u0 + B̂d d0 + (f̂op - x̂op)
 * on the model given to mpcqp_set_model, so that a closed loop keeps x̂0 resident on the GPU.
 * Khat (nx̂,nym,B) is the steady-state gain (the reference gets it from
 * ControlSystemsBase.kalman at construction, kalman.jl:204-236: host-side, once);
 * i_ym [nym] are the 0-based indices of the measured outputs.  nx̂ <= 64.
 *
 * Missing measurements (kalman.jl:245-251, 478-484; execute.jl:335,375).  Estimator b MISSES the correction of a period
 * when any of the nym entries of its y0m row is NaN -- the reference's any(isnan, y0m); Inf is a measurement -- or when
 * the period has no y0m at all (mpcqp_kf_correct[_device] or mpcqp_kf_update[_device] with y0m == NULL, `ym = nothing`).  On a missed correction x̂0 keeps its
 * bits (and so do P̂ and K̂ of a time-varying handle); the prediction of that period DOES run.  The decision is per
 * estimator: the rest of the batch is untouched.  mpcqp_kf_correct[_device], mpcqp_kf_update[_device] and
 * mpcqp_loop_device all follow the rule.
 *
 * The two forms of the estimator (`direct`, kalman.jl:112).  Filter form, direct = true (the default): a period is
 * correction with y0m(k) [preparestate!], step, prediction with u0(k) [updatestate!].  Predictor form, direct = false:
 * preparestate! does nothing, the step works on x̂ as it stands, x̂_{k-1}(k), and updatestate! runs the correction and then
 * the prediction (kalman.jl:276-281, 520-525) -- the input of period k does not wait for y(k).  The arithmetic of each
 * half is that of the filter form.  The gain stays the caller's and stays the FILTER-form gain: the library applies
 * x̂ <- Â (x̂ + K̂ v) + ... like update_estimate!, so the Khat to hand over is the same in both forms (the reference's own
 * direct = false gain, Â K̂, is not what is expected here).
 * mpcqp_kf_set_direct: 1 (default) or 0; anything else MPCQP_ERR_ARG.  A property of the handle that mpcqp_kf_set and
 * mpcqp_kf_set_covariances leave alone.  It changes the one entry point whose order is fixed inside a launch:
 * mpcqp_loop_device runs correction -> step -> prediction with 1 and step -> correction -> prediction with 0.
 * mpcqp_kf_update[_device]: correction, then prediction -- updatestate! of a direct = false estimator; legal whatever the
 * flag.  The result equals mpcqp_kf_correct followed by mpcqp_kf_predict bit for bit.  y0m == NULL: no correction for
 * any estimator.  MPCQP_ERR_ORDER before a model and an estimator are attached.                                   */
int mpcqp_kf_set(mpcqp_handle h, const double* Khat, const int32_t* i_ym, int32_t nym);
int mpcqp_kf_set_direct(mpcqp_handle h, int32_t direct);
/* xhat0 (nx̂,B) in/out, y0m (nym,B) -- or NULL in mpcqp_kf_correct / mpcqp_kf_update: no measurement this period --,
 * d0 (nd,B) or NULL, u0 (nu,B): host pointers, synchronous */
int mpcqp_kf_correct(mpcqp_handle h, double* xhat0, const double* y0m, const double* d0);
int mpcqp_kf_predict(mpcqp_handle h, double* xhat0, const double* u0, const double* d0);
int mpcqp_kf_update(mpcqp_handle h, double* xhat0, const double* u0, const double* y0m, const double* d0);
/* device pointers, asynchronous on `stream` */
int mpcqp_kf_correct_device(mpcqp_handle h, double* xhat0, const double* y0m, const double* d0, void* stream);
int mpcqp_kf_predict_device(mpcqp_handle h, double* xhat0, const double* u0, const double* d0, void* stream);
int mpcqp_kf_update_device(mpcqp_handle h, double* xhat0, const double* u0, const double* y0m, const double* d0,
                           void* stream);

/* ---- the time-varying KalmanFilter (src/estimator/kalman.jl:1235-1290) ----------------------------
 * The estimator the reference asks for when the model changes during the run ("SteadyKalmanFilter does not support
 * setmodel! (use KalmanFilter instead)", kalman.jl:229-232).  The covariance recursion
 *       correction   M̂ = Ĉm P̂ Ĉm' + R̂,  K̂ = P̂ Ĉm' M̂⁻¹,  P̂ <- (I - K̂ Ĉm) P̂      (stored as ½ (P̂ + P̂'))
 *       prediction   P̂ <- Â P̂ Â' + Q̂
 * depends on WHICH measurements are missing and on nothing else in the data: a kernel of its own advances P̂ and writes
 * K̂(k) into the gain buffer of the handle, on the stream and ahead of the estimator step that reads it.  There are NO
 * new per-period calls -- on a handle in time-varying mode
 *       mpcqp_kf_correct / _correct_device   run the covariance correction, then the state correction with K̂(k);
 *       mpcqp_kf_predict / _predict_device   run the state prediction, then the covariance prediction;
 *       mpcqp_kf_update / _update_device     run both halves of the covariance period in ONE launch (P̂ moves once), then
 *                                            the state correction and the state prediction; with y0m == NULL the
 *                                            covariance prediction alone, and every status becomes 1;
 *       mpcqp_loop_device                    runs both halves of the covariance period (given y0m), then the fused step,
 *                                            in either form.
 * Every launch reads the model that is resident at that moment: a mpcqp_set_model between two periods is picked up
 * with nothing else to call.
 *
 * mpcqp_kf_set_covariances: Qhat (nx̂,nx̂,B), Rhat (nym,nym,B), P0 (nx̂,nx̂,B), i_ym [nym] as in mpcqp_kf_set.  Puts the
 * handle in time-varying mode with K̂ = 0, P̂ = P0 and every status 0.  Matrices that are not symmetric (beyond 1e-12 of
 * their largest entry): MPCQP_ERR_ARG.  max(nx̂, nym) > 32, or a build without the kernel: MPCQP_ERR_UNSUPPORTED (the
 * handle keeps what it had).  Called again with P0 == NULL (same nym) it replaces Q̂ and R̂ and keeps P̂ and K̂ -- the Q̂, R̂
 * keywords of setmodel!.  A later mpcqp_kf_set returns the handle to the steady gain.
 * mpcqp_kf_set_state_covariance: P (nx̂,nx̂,B) replaces P̂ -- setstate!(estim, x̂, P̂).
 * mpcqp_kf_status: out [B], what became of the last correction attempt of each estimator (MPCQP_ERR_ORDER on a gain
 * from mpcqp_kf_set, which keeps no status; after mpcqp_kf_set_steady: the outcome of the solve, see below):
 *       0  done.
 *       1  skipped for a missing measurement (see above): P̂ and K̂ keep their bits -- MPCQP_GET_KF_GAIN goes on showing
 *          the K̂ of the last correction that ran -- and the prediction of that period runs, P̂ <- Â P̂ Â' + Q̂.
 *       2  dropped because M̂ was not positive definite or not finite, or the new P̂ / K̂ was not finite (where the
 *          reference's cholesky! throws): P̂ and K̂ keep their values, and so does P̂ in the prediction of that period --
 *          only status 2 holds the covariance prediction back; the next correction that succeeds puts 0 back.
 * The other estimators of the batch and the LinMPC step statuses are unaffected.
 * mpcqp_kf_lanes_per_estimator: 0 on a gain from mpcqp_kf_set, else 16 (max(nx̂, nym) <= 16: four estimators per wavefront) or 64;
 * after mpcqp_kf_set_steady with 32 < max(nx̂, nym) <= 64: 64 T, T the wavefronts of the workgroup that held an estimator in
 * the last solve (256 by default). */
int mpcqp_kf_set_covariances(mpcqp_handle h, const double* Qhat, const double* Rhat, const double* P0,
                             const int32_t* i_ym, int32_t nym);
int mpcqp_kf_set_state_covariance(mpcqp_handle h, const double* P);
int mpcqp_kf_status(mpcqp_handle h, int32_t* out);
int mpcqp_kf_lanes_per_estimator(mpcqp_handle h);

/* ---- the SteadyKalmanFilter from Q̂ and R̂: the steady-state gain computed on the device ------------
 * What the reference computes once per estimator on the host (kalman.jl:205-222) and refuses to redo after setmodel!
 * (kalman.jl:229-232): here every estimator of the batch solves the discrete algebraic Riccati equation of the predictor
 * form,  P = Â P Â' - Â P Ĉm' (Ĉm P Ĉm' + R̂)⁻¹ Ĉm P Â' + Q̂,  on the model that is resident, by the structure-preserving
 * doubling iteration (csrc/kf_dare_bodies.h; at most 40 iterations, stopped when P moves by less than 1e-13 of
 * max(1, max|P|)), and K̂ = P̂∞ Ĉm' (Ĉm P̂∞ Ĉm' + R̂)⁻¹, the filter-form gain of mpcqp_kf_set, lands in the gain buffer of
 * the handle.  R̂ has to be positive definite; Q̂ may be positive SEMIdefinite (noise through fewer channels than states,
 * delay states, a σQ with zeros).  The solve makes two passes over the batch: the first inverts H(k) (H(0) = Q̂) without
 * pivoting, which serves a definite Q̂; an estimator it leaves broken down, or whose Q̂ is numerically singular (smallest
 * pivot <= 1e-10 max diag Q̂), is solved again by the square-root form of
 * the same iteration (csrc/kf_dare_bodies.h, its square-root form: H(k) = L L' without pivoting, columns of pivots <= 0 dropped,
 * S = L (I + L'GL)⁻¹ L').  There a pivot of H(k) below -1e-8 max(1, max diag H(k)) is no rounding: an indefinite Q̂ keeps
 * status 2.  A build without the second pass (the kernel is missing) gives a semidefinite Q̂ status 2, as before.
 * 32 < max(nx̂, nym) <= 64: the same iteration in its definite form with the operands in LDS, one estimator per workgroup
 * of T wavefronts (csrc/kf_dare_lds_bodies.h; T = 4).  There is no second pass at this size: an estimator whose Q̂ is
 * numerically singular by the rule above, semidefinite or indefinite gets status 2, and mpcqp_kf_steady_path answers 0
 * for every estimator.  MPCQP_KF_DARE_TEAM = 1, 2 or 4 in the environment (read at every solve; any other value is
 * ignored) picks another compiled T -- a test hook: the result is bit-identical for every T.
 *
 * mpcqp_kf_set_steady: Qhat (nx̂,nx̂,B), Rhat (nym,nym,B), i_ym [nym]: layouts, symmetry check (MPCQP_ERR_ARG) and i_ym
 * validation of mpcqp_kf_set_covariances.  Needs the model (MPCQP_ERR_ORDER).  Stores Q̂ and R̂, fills K̂, P̂∞ and the
 * status with zeros, and solves (host-synchronous).  max(nx̂, nym) > 64, or a build without the kernel of that size (one
 * without the LDS-resident kernels stops at 32): MPCQP_ERR_UNSUPPORTED, and the handle keeps what it had.  (Only this
 * solve goes beyond 32: mpcqp_kf_set_covariances, mpcqp_kf_set_poles and mpcqp_est_initstate keep answering
 * MPCQP_ERR_UNSUPPORTED there, and a steady handle of that size keeps its solved gain when they do.)  In every other respect the handle is then one with a steady
 * gain: no launch is added to a period, and mpcqp_kf_correct / _predict / _update / mpcqp_loop_device are those of
 * mpcqp_kf_set, in both forms of mpcqp_kf_set_direct.
 * mpcqp_kf_solve_steady / _solve_steady_device: solve again on the model resident now (host-synchronous / enqueued on
 * `stream`, ordered like every other *_device call).  mpcqp_set_model does NOT do this by itself: until the caller
 * re-solves, the gain of the previous model stays in use.
 * mpcqp_kf_steady_iters: out [B], doubling iterations of the last solve (of the pass that produced the estimator's result).
 * mpcqp_kf_steady_path: out [B], which pass that was: 0 solved by, or left with, the definite form; 1 the square-root form
 * ran for this estimator (whatever its status).  MPCQP_ERR_ORDER outside the mode, like mpcqp_kf_steady_iters.
 * On such a handle
 *       mpcqp_kf_status   answers, per estimator, 0 solved; 1 not converged within the cap (the batch form of the
 *                         reference's "Cannot compute the optimal Kalman gain": an undetectable pair); 2 broke down: a
 *                         pivot of R̂ or of I + L'GL was outside (0, inf), H(k) had a negative pivot beyond rounding (see
 *                         above), or a value was not finite.  With 1 or 2
 *                         the estimator's K̂ and P̂∞ keep their previous contents (zeros after mpcqp_kf_set_steady) -- or
 *                         are set to zero, where the first pass had written a result for a numerically singular Q̂ and
 *                         the second pass refuses the estimator: a non-zero status never comes with a gain of that
 *                         solve; the rest of the batch is unaffected, bit for bit;
 *       MPCQP_GET_KF_COV  returns P̂∞;
 *       mpcqp_kf_lanes_per_estimator answers 16 or 64, beyond 32 states or measured outputs 64 T (256).
 * A later mpcqp_kf_set or mpcqp_kf_set_covariances leaves the mode: mpcqp_kf_solve_steady[_device],
 * mpcqp_kf_steady_iters and mpcqp_kf_steady_path then answer MPCQP_ERR_ORDER. */
int mpcqp_kf_set_steady(mpcqp_handle h, const double* Qhat, const double* Rhat, const int32_t* i_ym, int32_t nym);
int mpcqp_kf_solve_steady(mpcqp_handle h);
int mpcqp_kf_solve_steady_device(mpcqp_handle h, void* stream);
int mpcqp_kf_steady_iters(mpcqp_handle h, int32_t* out);
int mpcqp_kf_steady_path(mpcqp_handle h, int32_t* out);

/* ---- the Luenberger observer from its poles: the gain placed on the device ---------------------------
 * What the reference computes once per estimator on the host, K̂ = place(Â, Ĉ, poles, :o; direct) (luenberger.jl:38-42),
 * and refuses to redo after setmodel! (luenberger.jl:150-157): here every member of the batch places its poles on the
 * model that is resident, by the robust placement of Kautsky, Nichols and Van Dooren ("method 0", csrc/kf_place_bodies.h),
 * on the dual pair F = Â', G = (Ĉm Â)'.  The gain that lands in the gain buffer is the filter-form gain of mpcqp_kf_set:
 * the poles are the eigenvalues of Â (I - K̂ Ĉm), whatever mpcqp_kf_set_direct says (direct = false: the reference's own
 * gain is Â K̂, with the same poles).  Real poles only; a pole may be repeated up to nym times.  Ĉm is the measured rows of
 * Ĉ: the reference places on all of Ĉ and drops the unmeasured columns afterwards, which agrees with this only when every
 * output is measured.  A singular Â forces eigenvalues at 0: unless 0 is among the poles such a member gets status 2.
 * nym > nx̂: the first nx̂ measured outputs carry the gain, the other columns of K̂ are zero.
 *
 * mpcqp_kf_set_poles: poles (nx̂,B), i_ym [nym] validated as in mpcqp_kf_set_covariances.  A pole that is not finite or has
 * |p| >= 1: MPCQP_ERR_ARG.  Needs the model (MPCQP_ERR_ORDER).  max(nx̂, nym) > 32, or a build without the kernel:
 * MPCQP_ERR_UNSUPPORTED, and the handle keeps what it had.  Otherwise: stores the poles, fills K̂, the status and the sweep
 * counts with zeros, and places (host-synchronous).  In every other respect the handle is then one with a steady gain: no
 * launch is added to a period, and mpcqp_kf_correct / _predict / _update, mpcqp_loop_device, mpcqp_sim (the fused path
 * wherever a gain from mpcqp_kf_set qualifies) and mpcqp_est_initstate are those of mpcqp_kf_set, in both forms.
 * mpcqp_kf_place / _place_device: place again on the model resident now (host-synchronous / enqueued on `stream`).
 * mpcqp_set_model does NOT do this by itself: until the caller places again, the gain of the previous model stays in use.
 * mpcqp_kf_set_place_cap: most sweeps of the next placements, 0 .. 100 (default 30; 0 returns the starting vectors);
 * anything else MPCQP_ERR_ARG.  The sweeps stop earlier once |det X| moves by no more than 1e-3 of its value.
 * mpcqp_kf_place_sweeps: out [B], sweeps of the last placement.
 * On such a handle
 *       mpcqp_kf_status   answers, per member, 0 placed; 2 broke down: (Ĉm Â)' has no full column rank, a mode is
 *                         unobservable, a pole is repeated more often than there are outputs, or a value was not finite.
 *                         With 2 the member's K̂ keeps its previous contents (zeros after mpcqp_kf_set_poles); the rest of
 *                         the batch is unaffected, bit for bit;
 *       MPCQP_GET_KF_GAIN returns K̂;  MPCQP_GET_KF_COV answers MPCQP_ERR_ORDER (an observer has no covariance);
 *       mpcqp_kf_lanes_per_estimator answers 64.
 * A later mpcqp_kf_set, mpcqp_kf_set_steady or mpcqp_kf_set_covariances leaves the mode: the four calls below
 * mpcqp_kf_set_poles then answer MPCQP_ERR_ORDER, as mpcqp_kf_steady_* do on a handle in this mode. */
int mpcqp_kf_set_poles(mpcqp_handle h, const double* poles, const int32_t* i_ym, int32_t nym);
int mpcqp_kf_place(mpcqp_handle h);
int mpcqp_kf_place_device(mpcqp_handle h, void* stream);
int mpcqp_kf_set_place_cap(mpcqp_handle h, int32_t cap);
int mpcqp_kf_place_sweeps(mpcqp_handle h, int32_t* out);

/* ---- sim!: closed loops of the whole batch with the plant on the device (src/plot_sim.jl:241-319) ----------------
 * mpcqp_sim_set_plant attaches one LinModel per controller, the `plant` keyword of sim!: A (nxp,nxp,B), Bu (nxp,nu,B),
 * C (ny,nxp,B), Bd (nxp,nd,B), Dd (ny,nd,B), fx = fop - xop (nxp,B); Bd, Dd and fx may be NULL (zero).  Layouts of
 * mpcqp_set_model, deviation variables.  The plant has the handle's nu, ny and nd; nxp is its own (a mismatched plant of
 * another order is legal).  The arrays are copied; the call may be repeated.  nxp < 1: MPCQP_ERR_ARG; nxp > 64, a handle with
 * max(nu, ny, nd) > 64 or a library built without the kernel: MPCQP_ERR_UNSUPPORTED.
 *
 * mpcqp_sim (host pointers, synchronous) / mpcqp_sim_device (device pointers, asynchronous on `stream`) run io->N periods of
 * sim_closedloop! for every controller, without a host synchronisation between the periods.  Period i = 0..N-1:
 *     1. d0  = d + d_step + σd∘w_d[i]
 *     2. y0  = C x0 + Dd d0 + y_step + σy∘w_y[i],  y0m = y0[i_ym]
 *     3. preparestate!: the correction (direct = 1; nothing with direct = 0)
 *     4. records Y, X, D, X̂ -- the estimate after the correction -- and Ŷ = Ĉ x̂0 + D̂d d0
 *     5. moveinput!: mpcqp_explicit_law on a handle prepared with MPCQP_EXPLICIT_LAW (io->Ru == NULL), mpcqp_explicit_step on
 *        another prepared explicit handle, else mpcqp_step; set point and disturbance held over the horizon
 *     6. ud0 = u0 + u_step + σu∘w_u[i]; records U, Ud
 *     7. x0 <- A x0 + Bu ud0 + Bd d0 + fx + σx∘w_x[i]
 *     8. updatestate!: the prediction (direct = 1), or the correction with y0m and then the prediction (direct = 0)
 * The launches of a period are the existing device entry points (mpcqp_kf_correct_device, the controller's,
 * mpcqp_kf_predict_device / _update_device) and the kernel k_sim_plant between them: one launch of it does items 6-7 of period i
 * and items 1-2 of period i+1, a second one writes X̂ and Ŷ when either is asked for.  Every estimator (steady, time-varying,
 * both forms, the NaN rule: a NaN in y0m -- a NaN draw in w_y with its σ -- skips that member's correction) and every
 * controller kernel is served as those entry points serve it.
 *   ry       (ny,B), held over the run; (ny,N,B) with MPCQP_SIM_FLAG_RY_PER_PERIOD
 *   Ru       (nU,B) or NULL, as in mpcqp_step (the `ru` of sim!, repeated over Hp)
 *   d        (nd,B) (NULL iff nd == 0)
 *   *_step, sigma_*   (n,B) or NULL: u, y, d (nu, ny, nd) and, the σ only, x (nxp)
 *   w_*      (n,N,B) standard-normal draws, inputs so that a run is reproducible and the host can check it exactly: read
 *            only with their σ, which they are scaled by; a σ without its draws: MPCQP_ERR_NULL
 *   x0 (nxp,B), xhat0 (nx̂,B), lastu0 (nu,B)   in/out: the state of period N on return
 *   Ztilde   (nZ,B) in/out, the warm start of mpcqp_step and Z̃ of the last period; may be NULL on the law path (u0 alone, from
 *            the table of nu rows), MPCQP_ERR_NULL elsewhere.  A handle with MPCQP_FLAG_WARM_DUAL keeps its multipliers: two
 *            calls of N/2 periods equal one of N
 *   Y (ny) X (nxp) D (nd) Xhat (nx̂) Yhat (ny) U (nu) Ud (nu)   records (n,N,B), each may be NULL (not written)
 *   status   (N,B) int32 or NULL: the status of the controller's call per period
 * MPCQP_ERR_ARG for N <= 0 or an unknown flag; MPCQP_ERR_ORDER without a plant, an estimator or a controller that can step
 * (model and weights; an explicit handle that has become constrained).
 * Two execution paths serve the call; mpcqp_sim_path tells which one the handle gets (for a call with ry held, Ru == NULL and
 * without MPCQP_SIM_FLAG_NO_FUSE; any other call takes the per-period path):
 *   MPCQP_SIM_PATH_PERIOD  the launches above; every handle.
 *   MPCQP_SIM_PATH_FUSED   kernel k_sim_explicit runs the whole N-period loop in ONE launch: a handle prepared with
 *                          MPCQP_EXPLICIT_LAW whose gain is steady (mpcqp_kf_set or mpcqp_kf_set_steady) and whose
 *                          max(nx̂, nxp, nu, ny, nd, nym) <= 16.  One controller per 16-lane row, its tables loaded once; both
 *                          values of `direct`; the NaN rule and the status-2 policy (u0 = lastu0 every period) per member.  It
 *                          computes u0 alone: Ztilde is neither read nor written.  Results agree with the per-period path to
 *                          rounding (the sums run in another order), not bit for bit.
 * While mpcqp_sim_device enqueues the per-period path it sets MPCQP_FLAG_RY_CONSTANT and clears the set point of
 * mpcqp_set_current_setpoint on the handle, and puts both back before it returns: like every call on a handle, it must not
 * run beside another call on the same handle (a handle is not thread-safe, see the top of this file). */
#define MPCQP_SIM_FLAG_RY_PER_PERIOD (1u << 0)
#define MPCQP_SIM_FLAG_NO_FUSE       (1u << 1)
#define MPCQP_SIM_PATH_PERIOD        0
#define MPCQP_SIM_PATH_FUSED         1
typedef struct {
    int32_t  N;
    uint32_t flags;       /* MPCQP_SIM_FLAG_* */
    const double *ry, *Ru, *d;
    const double *u_step, *y_step, *d_step;
    const double *sigma_u, *sigma_y, *sigma_d, *sigma_x;
    const double *w_u, *w_y, *w_d, *w_x;
    double *x0, *xhat0, *lastu0, *Ztilde;
    double *Y, *X, *D, *Xhat, *Yhat, *U, *Ud;
    int32_t* status;
} mpcqp_sim_io;
int mpcqp_sim_set_plant(mpcqp_handle h, int32_t nxp, const double* A, const double* Bu, const double* C, const double* Bd,
                        const double* Dd, const double* fx);
int mpcqp_sim(mpcqp_handle h, const mpcqp_sim_io* io);
int mpcqp_sim_device(mpcqp_handle h, const mpcqp_sim_io* io, void* stream);
int mpcqp_sim_path(mpcqp_handle h);


/* ---- InternalModel (src/estimator/internal_model.jl): the estimator that changes the controller's free response ----------
 * The state is not augmented (Â = A, nx̂ = nx).  A stochastic model on the MEASURED outputs, As (nxs,nxs,B), Bs (nxs,nym,B),
 * Cs (nym,nxs,B), Ds (nym,nym,B), column-major per member like the model -- all four NULL: the identity in all four with
 * nxs = nym, the reference's default -- gives per period
 *     correct   ŷs[i_ym[j]] = y0m[j] - (Ĉm x̂d + D̂dm d0)[j]   (0 for a y0m[j] that is not finite, 0 in the unmeasured rows;
 *               x̂0 = x̂d is not touched), then block t = 1..Hp of Ŷs = Cs As^(t-1) (Âs x̂s + B̂s ŷs) -- the Ks x̂s + Ps ŷs of
 *               init_stochpred, as a recurrence -- and B_eff = B + Ŷs
 *     step      every mpcqp_step[_device] of the handle reads B_eff in place of the model's B: F, Ŷ, the gradient and the
 *               output-bound rows carry Ŷs.  The step kernels are the ones of a handle without this estimator.
 *     update    x̂d <- Â x̂d + B̂u u0 + B̂d d0 + (f̂op - x̂op),  x̂s <- Âs x̂s + B̂s ŷs
 * with B̂s = Bs Ds⁻¹ and Âs = As - B̂s Cs from the set-up (k_im_setup: elimination with partial pivoting, per member).
 * mpcqp_im_set replaces whatever estimator the handle had and zeroes x̂s, ŷs and Ŷs.  mpcqp_set_model keeps x̂s, ŷs, Ŷs and
 * the stochastic model: the next step uses the new B with the Ŷs of the last correction.  mpcqp_im_status (B) int32:
 *       0  ready
 *       2  Ds of the member is singular (a zero or non-finite pivot): its stochastic part is off, ŷs = Ŷs = 0 always
 * mpcqp_loop_device on such a handle enqueues correct, step, update on the caller's stream and updates xhat0 in place;
 * mpcqp_sim[_device] takes it on the per-period path (the Ŷ record is Ĉ x̂0 + D̂d d0 + ŷs); mpcqp_est_initstate[_device] is
 * init_estimate!: x̂d = (I - Â)⁻¹ (B̂u u0 + B̂d d0 + f̂op - x̂op), ŷs from it, x̂s = (I - Âs)⁻¹ B̂s ŷs; status 1 for a member one
 * of whose two systems is singular, which keeps its x̂0, x̂s and ŷs.
 * Limits (MPCQP_ERR_UNSUPPORTED): max(nx, nu, ny, nd, nxs) > 32; a handle whose steps run on the stage-structured kernel
 * (MultipleShooting, or SingleShooting beyond the condensed kernels: it does not read B); custom linear constraints (nw > 0:
 * their ŷ(k) term would need ŷs inside the kernel); mpcqp_explicit_* on such a handle; a shard handle of mpcqp_multi_*; a
 * library built without the kernels.  mpcqp_kf_set_direct(h, 0) on such a handle: MPCQP_ERR_ARG (the estimator is always in
 * the filter form).  nym < 1, nym > ny: MPCQP_ERR_DIMS; nxs < 1, i_ym out of range or repeated, some but not all of the
 * four matrices NULL: MPCQP_ERR_ARG.  A refused call changes nothing. */
int mpcqp_im_set(mpcqp_handle h, int32_t nxs, const double* As, const double* Bs, const double* Cs, const double* Ds,
                 const int32_t* i_ym, int32_t nym);
int mpcqp_im_status(mpcqp_handle h, int32_t* out);
int mpcqp_im_correct(mpcqp_handle h, const double* xhat0, const double* y0m, const double* d0);
int mpcqp_im_correct_device(mpcqp_handle h, const double* xhat0, const double* y0m, const double* d0, void* stream);
int mpcqp_im_update(mpcqp_handle h, double* xhat0, const double* u0, const double* d0);
int mpcqp_im_update_device(mpcqp_handle h, double* xhat0, const double* u0, const double* d0, void* stream);

/* ---- which kernel runs a step; building specialised kernels ahead of the control loop -----------
 * A step runs on (MPCQP_KERNEL_AOT) a kernel specialised on the handle's dimensions that is compiled
 * into the library (the BASELINE shapes, csrc/mpcqp_dispatch.h), (MPCQP_KERNEL_ONDEMAND) a kernel
 * specialised on demand for these dimensions and this pattern of constraint groups, compiled with
 * the installation's hipcc and cached (csrc/mpcqp_kernels.hip), or (MPCQP_KERNEL_GENERIC) the
 * runtime-dimension kernel (same source and numerics, about 4x slower; also the kernel of problems
 * with nZ > 128).  mpcqp_step NEVER compiles: without a call of
 * mpcqp_prepare (or a cached object from an earlier run / from mpcqp_prebuild) it uses the generic
 * kernel.  The JuMP analogue is the one-time model build of init_optimization!
 * (src/controller/linmpc.jl:303-339), which also happens before the control loop.
 *   mpcqp_prepare      after mpcqp_set_bounds (the pattern of constraint groups is part of the key):
 *                      compiles if needed (seconds, once per shape and machine), loads, returns the
 *                      MPCQP_KERNEL_* kind the steps will run on (>= 0) or a negative error code.
 *                      An on-demand kernel that has not been checked on this machine is first compared
 *                      with the runtime-dimension kernel on a few controllers of the handle (one cold
 *                      step, pseudo-random states and set points); it is used only if the two agree -- optimum and
 *                      status, and the specialisation does not need half as many iterations again --
 *                      (marker <object>.ok), otherwise it is renamed <object>.bad, the generic kernel
 *                      is used and mpcqp_last_build_error says why.  Objects are keyed by the kernel
 *                      revision AND the identity of the compiler binary that built them.
 *   mpcqp_kernel_kind  the kind a step would run on right now; never compiles.
 *   mpcqp_row_groups   the handle's pattern of constraint groups (bit g: group g may hold finite rows;
 *                      0 box lower [hard dUmin; also the row eps >= 0 when no output-bound group exists -- with
 *                      one, that row rides there as an extra row with a zero row of E, softness 1, bound 0 (kernel
 *                      revision 10: a whole row slot less in the step kernel)], 1 box upper, 2 Umin, 3 Umax,
 *                      4 soft dUmin, 5 soft dUmax, 6 Ymin, 7 Ymax, 8 xhat-min, 9 xhat-max, 10 Wmin, 11 Wmax).
 *                      Use the value a handle of the same constraint pattern reports, e.g. BASELINE config 3 (hard
 *                      umin / umax, soft ymax): 0x8c.
 *   mpcqp_prebuild     compile-only (no GPU, no handle): for build pipelines; dims->batch is ignored.  Returns the
 *                      MPCQP_KERNEL_* kind of the shape (>= 0) or a negative error code.  The package ships a manifest
 *                      of shapes (spec_manifest.txt: `nu ny nxhat Hp Hc neps row_groups`) that its build and
 *                      `python -m mpcqp.prebuild [manifest]` turn into cached objects, so that a machine without
 *                      hipcc still runs a declared set of shapes on specialised kernels.  A row_groups value with bit 0
 *                      next to an output-bound group and without bit 1 (a manifest line written before kernel revision
 *                      10, e.g. 0x8d) is still compiled, but mpcqp_last_build_error then says that only a controller
 *                      with hard dUmin and no dUmax bounds matches the object (0x8d -> 0x8c).
 *                      Beyond one row per lane (nZ~ > 64) the object holds a kernel that runs a team of two or four
 *                      wavefronts per controller when the problem's LDS footprint leaves SIMDs idle (round 6: same
 *                      results, same ABI; -DMPCQP_TEAM=1 in MPCQP_JIT_FLAGS keeps one wavefront per controller).
 *   mpcqp_last_build_error  text of the last failed build of this thread (or the note above).
 * Environment: MPCQP_CACHE_DIR (default: <library dir>/spec_cache if writable, else
 * $XDG_CACHE_HOME/mpcqp or ~/.cache/mpcqp), HIPCC (compiler binary), MPCQP_JIT=0 (never specialise). */
#define MPCQP_KERNEL_GENERIC   0
#define MPCQP_KERNEL_AOT       1
#define MPCQP_KERNEL_ONDEMAND  2
#define MPCQP_KERNEL_SMALL     3   /* nZ~ <= 16 with box, input-bound and (<= 64 in all) output-bound / terminal rows: four controllers per wavefront
                                    * (csrc/mpcqp_small_bodies.h); a step that fuses the Kalman steps (mpcqp_loop_device)
                                    * runs on the kernel the other rules select, and so does a handle WITH output-bound / terminal
                                    * rows of at most 1024 controllers when its own specialisation is available (measured 1.5 times
                                    * faster there; MPCQP_SMALL_Y=1 keeps it on this kernel) */
#define MPCQP_KERNEL_MS        4   /* MultipleShooting handles (mpcqp_set_transcription): the stage-structured kernel
                                    * (csrc/ms_bodies.h): Riccati recursion over the horizon, H̃ and E never formed */
int mpcqp_prepare(mpcqp_handle h);
/* LDS bytes one problem needs in the step kernel (160 KB per CU: the number of problems resident per CU follows). */
int mpcqp_lds_bytes(mpcqp_handle h);
int mpcqp_kernel_kind(mpcqp_handle h);
int mpcqp_row_groups(mpcqp_handle h, uint32_t* row_groups);
/* How often the handle has built its block of step constants so far (per move-blocking interval and input channel the
 * tightest U0min / U0max and the sum of the L weights; built before the first step or in mpcqp_prepare, and again after a
 * setter changed the model, the weights or the bounds).  0 for a handle whose steps form these values themselves
 * (dense L_Hp, MultipleShooting). */
int mpcqp_step_consts_builds(mpcqp_handle h);
int mpcqp_prebuild(const mpcqp_dims* dims, uint32_t row_groups);
const char* mpcqp_last_build_error(void);

/* ---- several GPUs of one node behind one handle (contiguous shards, no coupling) -------
 * mpcqp_multi_create makes one handle per entry of device_ids (an ordinal may repeat) and gives
 * device g the problems [off_g, off_g + B_g) of the batch, B_g = floor(B/ndev) (+1 for the first
 * B mod ndev devices).  Every array is problem-major, so a shard is ONE contiguous slice of each
 * caller array: the set_* / step entry points below take the whole-batch HOST arrays of their
 * single-device twins, slice them, and drive all devices concurrently (one stream per device; the
 * step is enqueued everywhere before anything is awaited; results are copied back into the caller's
 * arrays slice by slice -- the gather).  mpcqp_multi_handle gives the single-device handle of a shard
 * for everything else (mpcqp_get, kf_*, prepare ...); mpcqp_multi_shard its offset and size.
 * Device-resident data: call mpcqp_step_device on the shard handles with per-device pointers, and
 * mpcqp_multi_gather_device to collect Z (nZ,B), u0 (nu,B), status (B) of all shards into buffers on
 * one root device (hipMemcpyPeerAsync over xGMI; stream = a stream of the root device, or NULL);
 * mpcqp_multi_scatter_device is the way in: per-period inputs born on one device, sliced to the shards. */
typedef struct mpcqp_multi_s* mpcqp_multi;
int mpcqp_multi_create(const mpcqp_dims* dims, const int32_t* device_ids, int32_t ndev, mpcqp_multi* out);
int mpcqp_multi_destroy(mpcqp_multi mh);
int mpcqp_multi_ndev(mpcqp_multi mh);
mpcqp_handle mpcqp_multi_handle(mpcqp_multi mh, int32_t g);
int mpcqp_multi_shard(mpcqp_multi mh, int32_t g, int32_t* offset, int32_t* count);
int mpcqp_multi_set_model(mpcqp_multi mh, const double* Ahat, const double* Bu, const double* C,
                          const double* Bd, const double* Dd, const double* fop_minus_xop);
int mpcqp_multi_set_weights(mpcqp_multi mh, const double* Mdiag, const double* Ndiag,
                            const double* Ldiag, const double* Cwt);
int mpcqp_multi_set_bounds(mpcqp_multi mh, const mpcqp_bounds* bounds);
int mpcqp_multi_prepare(mpcqp_multi mh);
int mpcqp_multi_step(mpcqp_multi mh, const double* xhat0, const double* lastu0, const double* Ry,
                     const double* Ru, const double* d0, const double* Dhat0, double* Ztilde,
                     double* u0, int32_t* status, int32_t* iters, double* Yhat0);
int mpcqp_multi_gather_device(mpcqp_multi mh, int32_t root, const double* const* Z_shards,
                              const double* const* u0_shards, const int32_t* const* status_shards,
                              double* Z_root, double* u0_root, int32_t* status_root, void* stream);

/* The scatter of a period's inputs that were born on ONE device (the estimates of a plant-wide observer, set points of
 * a supervisory layer): x̂0 (nx̂,B), lastu0 (nu,B) and Ry (ry_rows,B; ry_rows = ny with MPCQP_FLAG_RY_CONSTANT, else ny Hp)
 * on `root` are sliced into the per-device buffers of the shards, hipMemcpyPeerAsync over xGMI on `stream` (a stream of
 * the root device, or NULL: the root handle's stream, synchronised before returning).  Twin of the gather above.     */
int mpcqp_multi_scatter_device(mpcqp_multi mh, int32_t root, const double* xhat0_root, const double* lastu0_root,
                               const double* Ry_root, int32_t ry_rows, double* const* xhat0_shards,
                               double* const* lastu0_shards, double* const* Ry_shards, void* stream);

/* Device time of the kernels of the last step / recondense on this handle, measured with HIP
 * events on the stream they ran on (milliseconds; < 0 if not available).                     */
double mpcqp_last_step_ms(mpcqp_handle h);
double mpcqp_last_condense_ms(mpcqp_handle h);
double mpcqp_last_predmat_ms(mpcqp_handle h);    /* K1 part of the last condensation (K2 = the rest) */

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_H */
