# MPCQPShim.jl -- the binding a ModelPredictiveControl.jl maintainer adds to run the `moveinput!`
# body of a BATCH of LinMPC controllers (identical dimensions) on MI355X through libmpcqp.so
# (C-ABI: include/mpcqp.h).  Everything else -- LinModel, estimators, LinMPC construction,
# setconstraint! bookkeeping, updatestate! -- stays the reference's Julia code.
#
# Julia is not part of the image this repository is built in, so this file is exercised by reading,
# not by CI: the same ABI is driven by modelpredictivecontrol.jl_amd/api.py (ctypes) and by
# tests/abi_c_client.c (plain C), whose call sequences this file mirrors one to one.
#
#   using ModelPredictiveControl, .MPCQPShim
#   mpcs  = [LinMPC(...) for _ in 1:B];  foreach(c -> setconstraint!(c; ...), mpcs)
#   batch = MPCQPShim.BatchLinMPC(mpcs)              # uploads models, weights, bounds; builds the kernel
#   u     = moveinput!(batch, ry)                    # (nu, B): one control period of all B controllers
module MPCQPShim

using ModelPredictiveControl
using LinearAlgebra: diag, Diagonal
import ModelPredictiveControl: moveinput!, LinMPC

const lib = get(ENV, "MPCQP_LIB", "libmpcqp.so")

const FLAG_RY_CONSTANT = 0x1          # Ry is (ny, B): ry held over Hp (the reference's default R̂y = repeat(ry, Hp))
const FLAG_COLD_START  = 0x2
const FLAG_WARM_DUAL   = 0x8
const STATUS_ITERATION_LIMIT, STATUS_ERROR = 1, 2

struct Dims                           # == mpcqp_dims
    batch::Cint; nxhat::Cint; nu::Cint; ny::Cint; nd::Cint; Hp::Cint; Hc::Cint
    nb::Ptr{Cint}; neps::Cint; device::Cint; flags::Cuint; max_iter::Cint
    gap_tol::Cdouble; res_tol::Cdouble; dual_reg::Cdouble
end

struct Bounds                         # == mpcqp_bounds: 16 pointers, C_NULL = group absent / default softness
    U0min::Ptr{Float64}; U0max::Ptr{Float64}; DUmin::Ptr{Float64}; DUmax::Ptr{Float64}
    Y0min::Ptr{Float64}; Y0max::Ptr{Float64}; x0min::Ptr{Float64}; x0max::Ptr{Float64}
    C_umin::Ptr{Float64}; C_umax::Ptr{Float64}; C_dumin::Ptr{Float64}; C_dumax::Ptr{Float64}
    C_ymin::Ptr{Float64}; C_ymax::Ptr{Float64}; c_x0min::Ptr{Float64}; c_x0max::Ptr{Float64}
end

mutable struct BatchLinMPC
    h::Ptr{Cvoid}
    mpcs::Vector{<:LinMPC}            # the logical controllers (same dimensions)
    Z̃::Matrix{Float64}                # (nZ̃, B) previous optima = warm start of the next period
    lastu0::Matrix{Float64}           # (nu, B)
    kernel::Int                       # MPCQP_KERNEL_* the steps run on
    flags::Cuint                      # MPCQP_FLAG_* given to the constructor (moveinput! only toggles RY_CONSTANT)
end

function check(rc::Integer)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:mpcqp_strerror, lib), Cstring, (Cint,), rc))
    rc == -6 && (msg *= ": " * unsafe_string(ccall((:mpcqp_last_hip_error, lib), Cstring, ())))
    error("mpcqp error $rc: $msg")
end

cat3(f, mpcs) = cat((f(c) for c in mpcs)...; dims=3)     # (rows, cols, B): the ABI layout, zero copy
cat2(f, mpcs) = reduce(hcat, (f(c) for c in mpcs))       # (n, B)
ptr_or_null(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)

"""
    push_bounds!(h, mpcs)

`mpcqp_set_bounds` from the `ControllerConstraint` of every controller
(src/controller/construct.jl:126-199).  Bounds are the deviation vectors the reference stores
(`con.U0min = umin - Uop`, :359); `±Inf` = absent row (the `i_b` rule, transcription.jl:692-700).
Softness: the last column of the `A_*` blocks is `-C` (relaxU / relaxΔU, construct.jl:1029-1083);
`C_ymin, C_ymax, c_x̂min, c_x̂max` are stored as such.  A group whose bounds are all infinite for
every controller is passed as NULL (the kernel is specialised on the set of groups present).
"""
function push_bounds!(h::Ptr{Cvoid}, mpcs)
    soft = mpcs[1].nϵ == 1
    grp(f) = (a = cat2(c -> f(c.con), mpcs); all(isinf, a) ? nothing : a)
    sft(a, f) = (soft && a !== nothing) ? cat2(c -> f(c.con), mpcs) : nothing
    U0min, U0max = grp(c -> c.U0min), grp(c -> c.U0max)
    DUmin, DUmax = grp(c -> c.ΔUmin), grp(c -> c.ΔUmax)
    Y0min, Y0max = grp(c -> c.Y0min), grp(c -> c.Y0max)
    x0min, x0max = grp(c -> c.x̂0min), grp(c -> c.x̂0max)
    C_umin  = sft(U0min, c -> -Vector(c.A_Umin[:, end]));   C_umax  = sft(U0max, c -> -Vector(c.A_Umax[:, end]))
    C_dumin = sft(DUmin, c -> -Vector(c.A_ΔUmin[:, end]));  C_dumax = sft(DUmax, c -> -Vector(c.A_ΔUmax[:, end]))
    C_ymin  = sft(Y0min, c -> c.C_ymin);                    C_ymax  = sft(Y0max, c -> c.C_ymax)
    c_x0min = sft(x0min, c -> c.c_x̂min);                    c_x0max = sft(x0max, c -> c.c_x̂max)
    arrs = (U0min, U0max, DUmin, DUmax, Y0min, Y0max, x0min, x0max,
            C_umin, C_umax, C_dumin, C_dumax, C_ymin, C_ymax, c_x0min, c_x0max)
    GC.@preserve arrs begin
        b = Bounds(map(ptr_or_null, arrs)...)
        check(ccall((:mpcqp_set_bounds, lib), Cint, (Ptr{Cvoid}, Ref{Bounds}), h, b))
    end
    return nothing
end

"block-diagonal `M_Hp` (e.g. a terminal cost): blocks as (ny, ny, Hp, B), after mpcqp_set_weights"
function push_blockweight!(h::Ptr{Cvoid}, mpcs)
    ny, Hp = mpcs[1].estim.model.ny, mpcs[1].Hp
    Mb = Array{Float64}(undef, ny, ny, Hp, length(mpcs))
    for (b, c) in enumerate(mpcs), t in 1:Hp
        Mb[:, :, t, b] .= c.weights.M_Hp[(t-1)*ny+1:t*ny, (t-1)*ny+1:t*ny]
    end
    check(ccall((:mpcqp_set_output_weight_blocks, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), h, Mb))
end

isdiagonal(M) = all(iszero, M - Diagonal(diag(M)))

function BatchLinMPC(mpcs::Vector{<:LinMPC}; device::Integer=0, flags::Unsigned=FLAG_RY_CONSTANT)
    m = mpcs[1]; est = m.estim; model = est.model; B = length(mpcs)
    all(c -> (c.Hp, c.Hc, c.nϵ, c.nb) == (m.Hp, m.Hc, m.nϵ, m.nb), mpcs) ||
        throw(DimensionMismatch("all controllers of a batch need the same horizons"))
    nb = Cint.(m.nb)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve nb begin
        d = Dims(B, est.nx̂, model.nu, model.ny, model.nd, m.Hp, m.Hc, pointer(nb), m.nϵ, device,
                 flags, 0, 0.0, 0.0, 0.0)
        check(ccall((:mpcqp_create, lib), Cint, (Ref{Dims}, Ref{Ptr{Cvoid}}), d, h))
    end
    nd = model.nd
    Â, B̂u, Ĉ = cat3(c -> c.estim.Â, mpcs), cat3(c -> c.estim.B̂u, mpcs), cat3(c -> c.estim.Ĉ, mpcs)
    B̂d = nd > 0 ? cat3(c -> c.estim.B̂d, mpcs) : nothing
    D̂d = nd > 0 ? cat3(c -> c.estim.D̂d, mpcs) : nothing
    dop = cat2(c -> c.estim.f̂op - c.estim.x̂op, mpcs)
    GC.@preserve Â B̂u Ĉ B̂d D̂d dop check(ccall((:mpcqp_set_model, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h[], Â, B̂u, Ĉ, ptr_or_null(B̂d), ptr_or_null(D̂d), dop))
    nΔU = model.nu * m.Hc
    Md = cat2(c -> diag(c.weights.M_Hp), mpcs)
    Nd = cat2(c -> diag(c.weights.Ñ_Hc)[1:nΔU], mpcs)
    Ld = cat2(c -> diag(c.weights.L_Hp), mpcs)
    Cw = Float64[m.nϵ == 1 ? c.weights.Ñ_Hc[end, end] : Inf for c in mpcs]
    GC.@preserve Md Nd Ld Cw check(ccall((:mpcqp_set_weights, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h[], Md, Nd, Ld, Cw))
    isdiagonal(m.weights.M_Hp) || push_blockweight!(h[], mpcs)
    push_bounds!(h[], mpcs)
    # the specialised kernel of this shape and constraint pattern: built here (once per shape and
    # machine, cached), never inside a step -- the analogue of init_optimization! (linmpc.jl:303-339)
    # transcription of the controllers (LinMPC keyword, linmpc.jl:205-216): MultipleShooting runs on the stage-structured
    # kernel (include/mpcqp.h: mpcqp_set_transcription) when the handle qualifies, else the condensed kernels solve the
    # same problem
    if m.transcription isa MultipleShooting
        check(ccall((:mpcqp_set_transcription, lib), Cint, (Ptr{Cvoid}, Cint), h[], 1))
        if ccall((:mpcqp_transcription_supported, lib), Cint, (Ptr{Cvoid},), h[]) != 0
            @warn "MultipleShooting kernel not available for these controllers: the SingleShooting kernels solve the same problem"
            check(ccall((:mpcqp_set_transcription, lib), Cint, (Ptr{Cvoid}, Cint), h[], 0))
        end
    end
    kernel = ccall((:mpcqp_prepare, lib), Cint, (Ptr{Cvoid},), h[])
    kernel < 0 && check(kernel)
    b = BatchLinMPC(h[], mpcs, zeros(m.nϵ + nΔU, B), cat2(c -> c.lastu0, mpcs), kernel, Cuint(flags))
    finalizer(x -> ccall((:mpcqp_destroy, lib), Cint, (Ptr{Cvoid},), x.h), b)
    return b
end

"""
    moveinput!(b::BatchLinMPC, ry, d=...; R̂y=nothing, R̂u=nothing, D̂=nothing) -> u (nu, B)

Drop-in for `moveinput!` over the batch (src/controller/execute.jl:59-80): `ry` (ny, B), `d` (nd, B).
The estimates `x̂0` are read from the controllers' estimators (`preparestate!` stays Julia-side).
"""
function moveinput!(b::BatchLinMPC, ry::AbstractMatrix, d::AbstractMatrix=zeros(0, size(ry, 2));
                    R̂y=nothing, R̂u=nothing, D̂=nothing)
    m = b.mpcs[1]; model = m.estim.model; B = length(b.mpcs); Hp = m.Hp
    x̂0  = cat2(c -> c.estim.x̂0, b.mpcs)
    yop = cat2(c -> c.estim.model.yop, b.mpcs); uop = cat2(c -> c.estim.model.uop, b.mpcs)
    held = R̂y === nothing                                       # the held set point is sent once
    flags = held ? (b.flags | Cuint(FLAG_RY_CONSTANT)) : (b.flags & ~Cuint(FLAG_RY_CONSTANT))
    check(ccall((:mpcqp_set_flags, lib), Cint, (Ptr{Cvoid}, Cuint), b.h, flags))
    Ry0 = held ? Matrix{Float64}(ry .- yop) : Matrix{Float64}(R̂y .- repeat(yop, Hp))
    Ru0 = R̂u === nothing ? nothing : Matrix{Float64}(R̂u .- repeat(uop, Hp))
    d0 = D̂0 = nothing
    if model.nd > 0
        dop = cat2(c -> c.estim.model.dop, b.mpcs)
        d0 = Matrix{Float64}(d .- dop)
        D̂0 = D̂ === nothing ? repeat(d0, Hp) : Matrix{Float64}(D̂ .- repeat(dop, Hp))
    end
    u0 = similar(b.lastu0); status = zeros(Cint, B); iters = zeros(Cint, B)
    GC.@preserve x̂0 Ry0 Ru0 d0 D̂0 u0 status iters check(ccall((:mpcqp_step, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Ptr{Float64}),
        b.h, x̂0, b.lastu0, Ry0, ptr_or_null(Ru0), ptr_or_null(d0), ptr_or_null(D̂0), b.Z̃, u0, status, iters, C_NULL))
    any(==(STATUS_ERROR), status) && @error "MPC terminated without solution: returning last solution shifted"
    any(==(STATUS_ITERATION_LIMIT), status) && @warn "MPC termination status not OPTIMAL: keeping solution anyway"
    b.lastu0 .= u0                                              # getinput!: lastu0 <- u - uop
    for (i, c) in enumerate(b.mpcs)                             # keep the logical controllers in sync
        c.Z̃ .= @view b.Z̃[:, i]; c.lastu0 .= @view u0[:, i]
    end
    return u0 .+ uop
end

# ------------------------------------------------------------------------------------------------
# Time-varying KalmanFilter behind the batch (include/mpcqp.h, "the time-varying KalmanFilter"): P̂ and K̂(k) live on the
# device and follow mpcqp_kf_correct / mpcqp_kf_predict / mpcqp_loop_device, on the model that is resident at that moment
# (a setmodel! -> mpcqp_set_model between two periods needs nothing else).  Both forms: `direct` of the estimators goes to
# mpcqp_kf_set_direct, and update_kalmanfilter! is updatestate! of the predictor form.  Call sequence = the one of
# modelpredictivecontrol.jl_amd/api.py (BatchLinMPC.setestimator(covariances=...)), which the GPU tests drive; these ccalls
# have not been run (no Julia on the build machines).
import ModelPredictiveControl: KalmanFilter

"Q̂, R̂, P̂ of the batch's KalmanFilters to the device; `keepP = true` replaces Q̂ and R̂ only (the keywords of setmodel!)."
function push_kalmanfilter!(b::BatchLinMPC; keepP::Bool=false)
    es = [c.estim for c in b.mpcs]
    all(e -> e isa KalmanFilter && e.direct == es[1].direct, es) || throw(ArgumentError("time-varying filter: KalmanFilters of one form (direct)"))
    stack3(f) = cat((Matrix{Float64}(f(e)) for e in es)...; dims=3)          # (n, n, B)
    Q̂, R̂, P̂ = stack3(e -> e.cov.Q̂), stack3(e -> e.cov.R̂), stack3(e -> e.cov.P̂)
    i_ym = Cint.(es[1].i_ym .- 1)                                            # 0-based
    GC.@preserve Q̂ R̂ P̂ i_ym check(ccall((:mpcqp_kf_set_covariances, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Cint),
        b.h, Q̂, R̂, keepP ? C_NULL : pointer(P̂), i_ym, length(i_ym)))
    set_direct!(b, es[1].direct)
    return b
end

"`direct` of the batch's estimators: true filter form, false predictor form (mpcqp_loop_device: step, correction, prediction)."
set_direct!(b::BatchLinMPC, direct::Bool) =
    check(ccall((:mpcqp_kf_set_direct, lib), Cint, (Ptr{Cvoid}, Int32), b.h, direct ? 1 : 0))

"""
updatestate! of a direct=false batch: correction with y0m (nym, B), then prediction with u0 (nu, B), in place on x̂0 (nx̂, B).
`y0m = nothing` skips every correction; a NaN in a column of y0m skips that estimator's (status 1 in pull_kalmanfilter).
The K̂ behind a steady gain is the FILTER-form gain in both forms (include/mpcqp.h).
"""
function update_kalmanfilter!(b::BatchLinMPC, x̂0::Matrix{Float64}, u0::Matrix{Float64}, y0m::Union{Nothing,Matrix{Float64}},
                              d0::Union{Nothing,Matrix{Float64}}=nothing)
    GC.@preserve x̂0 u0 y0m d0 check(ccall((:mpcqp_kf_update, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        b.h, x̂0, u0, y0m === nothing ? C_NULL : pointer(y0m), d0 === nothing ? C_NULL : pointer(d0)))
    return x̂0
end

"The same with device pointers, asynchronous on `stream` (y0m, d0: C_NULL allowed as above)."
update_kalmanfilter_device!(b::BatchLinMPC, x̂0::Ptr{Float64}, u0::Ptr{Float64}, y0m::Ptr{Float64}, d0::Ptr{Float64},
                            stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:mpcqp_kf_update_device, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}), b.h, x̂0, u0, y0m, d0, stream))

"setstate!(estim, x̂, P̂) for the batch: P (nx̂, nx̂, B)."
set_state_covariance!(b::BatchLinMPC, P::Array{Float64,3}) =
    check(ccall((:mpcqp_kf_set_state_covariance, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.h, P))

"P̂ (nx̂, nx̂, B), K̂ (nx̂, nym, B) and the per-estimator status (0 done, 1 skipped for a missing measurement, 2 dropped) back into Julia."
function pull_kalmanfilter(b::BatchLinMPC)
    e = b.mpcs[1].estim
    nx̂, nym, B = e.nx̂, e.nym, length(b.mpcs)
    P̂, K̂, st = Array{Float64}(undef, nx̂, nx̂, B), Array{Float64}(undef, nx̂, nym, B), Vector{Cint}(undef, B)
    check(ccall((:mpcqp_get, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), b.h, 10 #= MPCQP_GET_KF_COV =#, P̂))
    check(ccall((:mpcqp_get, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), b.h, 11 #= MPCQP_GET_KF_GAIN =#, K̂))
    check(ccall((:mpcqp_kf_status, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}), b.h, st))
    lanes = ccall((:mpcqp_kf_lanes_per_estimator, lib), Cint, (Ptr{Cvoid},), b.h)      # 0 steady gain, 16 or 64
    return (; P̂, K̂, status=st, lanes)
end

# ------------------------------------------------------------------------------------------------
# SteadyKalmanFilter from Q̂ and R̂ behind the batch (include/mpcqp.h, "the SteadyKalmanFilter from Q̂ and R̂"): the steady-state
# gain of every estimator is solved for on the device from the resident model, and solved again on request after a
# setmodel! -> mpcqp_set_model (which the reference's SteadyKalmanFilter refuses).  Q̂ and R̂ positive definite,
# max(nx̂, nym) <= 32.  pull_kalmanfilter reads K̂, P̂∞ and the status (0 solved, 1 not converged: undetectable, 2 broke down)
# back.  Call sequence = BatchLinMPC.setestimator(steady=...) of api.py; these ccalls have not been run either.
import ModelPredictiveControl: SteadyKalmanFilter

"Q̂, R̂ of the batch's SteadyKalmanFilters to the device, and the first solve."
function push_steadykalmanfilter!(b::BatchLinMPC)
    es = [c.estim for c in b.mpcs]
    all(e -> e isa SteadyKalmanFilter && e.direct == es[1].direct, es) || throw(ArgumentError("steady filter: SteadyKalmanFilters of one form (direct)"))
    stack3(f) = cat((Matrix{Float64}(f(e)) for e in es)...; dims=3)          # (n, n, B)
    Q̂, R̂ = stack3(e -> e.cov.Q̂), stack3(e -> e.cov.R̂)
    i_ym = Cint.(es[1].i_ym .- 1)                                            # 0-based
    GC.@preserve Q̂ R̂ i_ym check(ccall((:mpcqp_kf_set_steady, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Cint), b.h, Q̂, R̂, i_ym, length(i_ym)))
    set_direct!(b, es[1].direct)
    return b
end

"Solve again on the model resident now (after mpcqp_set_model): until then the gain of the previous model is in use."
solve_steadykalmanfilter!(b::BatchLinMPC) = check(ccall((:mpcqp_kf_solve_steady, lib), Cint, (Ptr{Cvoid},), b.h))

"The same, asynchronous on `stream`."
solve_steadykalmanfilter_device!(b::BatchLinMPC, stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:mpcqp_kf_solve_steady_device, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), b.h, stream))

"Doubling iterations of the last solve, per estimator."
function steadykalmanfilter_iters(b::BatchLinMPC)
    it = Vector{Cint}(undef, length(b.mpcs))
    check(ccall((:mpcqp_kf_steady_iters, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}), b.h, it))
    return it
end

# ------------------------------------------------------------------------------------------------
# Luenberger observer behind the batch (include/mpcqp.h, "the Luenberger observer from its poles"): the gain of every member is
# placed on the device from the resident model and the observer poles, and placed again on request after a setmodel! ->
# mpcqp_set_model (which the reference's Luenberger refuses).  Real poles inside the unit circle, max(nx̂, nym) <= 32; the gain is
# the filter-form gain in both forms of `direct`.  pull_luenberger reads K̂, the status (0 placed, 2 broke down) and the sweep
# counts back.  Call sequence = BatchLinMPC.setestimator(luenberger=...) of api.py; these ccalls have not been run.
import ModelPredictiveControl: Luenberger

"The poles of the batch's Luenberger observers ((nx̂, B), real) to the device, and the first placement."
function push_luenberger!(b::BatchLinMPC, poles::AbstractMatrix{<:Real})
    es = [c.estim for c in b.mpcs]
    all(e -> e isa Luenberger && e.direct == es[1].direct, es) || throw(ArgumentError("Luenberger observers of one form (direct)"))
    size(poles) == (es[1].nx̂, length(es)) || throw(ArgumentError("poles: (nx̂, B)"))
    p = Matrix{Float64}(poles)
    i_ym = Cint.(es[1].i_ym .- 1)                                            # 0-based
    GC.@preserve p i_ym check(ccall((:mpcqp_kf_set_poles, lib), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cint}, Cint), b.h, p, i_ym, length(i_ym)))
    set_direct!(b, es[1].direct)
    return b
end

"Place again on the model resident now (after mpcqp_set_model): until then the gain of the previous model is in use."
place_luenberger!(b::BatchLinMPC) = check(ccall((:mpcqp_kf_place, lib), Cint, (Ptr{Cvoid},), b.h))

"The same, asynchronous on `stream`."
place_luenberger_device!(b::BatchLinMPC, stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:mpcqp_kf_place_device, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), b.h, stream))

"Most sweeps of the placements that follow, 0 .. 100 (default 30)."
set_luenberger_cap!(b::BatchLinMPC, cap::Integer) = check(ccall((:mpcqp_kf_set_place_cap, lib), Cint, (Ptr{Cvoid}, Cint), b.h, cap))

"K̂ (nx̂, nym, B), the status and the sweeps of the last placement, per member."
function pull_luenberger(b::BatchLinMPC)
    B, e = length(b.mpcs), b.mpcs[1].estim
    K̂ = Array{Float64}(undef, e.nx̂, e.nym, B)
    st, sw = Vector{Cint}(undef, B), Vector{Cint}(undef, B)
    check(ccall((:mpcqp_get, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), b.h, 11, K̂))      # MPCQP_GET_KF_GAIN
    check(ccall((:mpcqp_kf_status, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}), b.h, st))
    check(ccall((:mpcqp_kf_place_sweeps, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}), b.h, sw))
    return (; K̂, status=st, sweeps=sw)
end

# ------------------------------------------------------------------------------------------------
# Continuous-time models (include/mpcqp.h, "LinModel(sys, Ts) and augment_model for the whole batch"): what LinModel(sys, Ts)
# and augment_model do per model on the host, for every member in one launch.  Declarations only: not run here.
struct C2dSpec                         # == mpcqp_c2d_spec
    batch::Cint; nx::Cint; nu::Cint; ny::Cint; nd::Cint; nym::Cint; d_method::Cint     # d_method: 0 Tustin, 1 zero-order hold
    nint_u::Ptr{Cint}; nint_ym::Ptr{Cint}; i_ym::Ptr{Cint}                             # C_NULL: none / none / 1:nym
end
struct C2dIn                           # == mpcqp_c2d_in; Bd, Dd: nd > 0; dop = fop - xop (nx_dis, B) or C_NULL
    A::Ptr{Float64}; Bu::Ptr{Float64}; C::Ptr{Float64}; Bd::Ptr{Float64}; Dd::Ptr{Float64}; Ts::Ptr{Float64}; dop::Ptr{Float64}
end
struct C2dOut                          # == mpcqp_c2d_out
    Â::Ptr{Float64}; B̂u::Ptr{Float64}; Ĉ::Ptr{Float64}; B̂d::Ptr{Float64}; D̂d::Ptr{Float64}; dop::Ptr{Float64}
end

"(nx_dis, nx̂) of a discretisation: nx_dis = 2nx with the Tustin block, nx̂ = nx_dis + sum(nint_u) + sum(nint_ym)."
function c2d_sizes(spec::C2dSpec)
    nxd, nx̂ = Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:mpcqp_c2d_sizes, lib), Cint, (Ref{C2dSpec}, Ref{Cint}, Ref{Cint}), spec, nxd, nx̂))
    return Int(nxd[]), Int(nx̂[])
end

"""
    c2d(A, Bu, C, Ts; Bd, Dd, nint_u, nint_ym, i_ym, d_method=:tustin) -> (; Â, B̂u, Ĉ, B̂d, D̂d, status)

Discretise and augment a batch of continuous-time models: A (nx, nx, B), Bu (nx, nu, B), C (ny, nx, B), Bd (nx, nd, B),
Dd (ny, nd, B), Ts (B).  `i_ym` is one-based.  status 2: the member was refused and its slices are zero.
"""
function c2d(A::Array{Float64,3}, Bu::Array{Float64,3}, C::Array{Float64,3}, Ts::Vector{Float64};
             Bd::Array{Float64,3}=zeros(size(A, 1), 0, size(A, 3)), Dd::Array{Float64,3}=zeros(size(C, 1), 0, size(A, 3)),
             nint_u::Vector{<:Integer}=zeros(Int, size(Bu, 2)), nint_ym::Vector{<:Integer}=zeros(Int, size(C, 1)),
             i_ym::Vector{<:Integer}=collect(1:length(nint_ym)), d_method::Symbol=:tustin)
    nx, nu, B = size(Bu); ny, nd = size(C, 1), size(Bd, 2)
    nu_, nym_, iy = Cint.(nint_u), Cint.(nint_ym), Cint.(i_ym .- 1)
    st = zeros(Cint, B)
    GC.@preserve nu_ nym_ iy A Bu C Bd Dd Ts begin
        spec = C2dSpec(B, nx, nu, ny, nd, length(iy), d_method === :zoh ? 1 : 0, pointer(nu_), pointer(nym_), pointer(iy))
        _, nx̂ = c2d_sizes(spec)
        Â, B̂u, Ĉ, B̂d, D̂d = zeros(nx̂, nx̂, B), zeros(nx̂, nu, B), zeros(ny, nx̂, B), zeros(nx̂, nd, B), zeros(ny, nd, B)
        p(M) = isempty(M) ? Ptr{Float64}(C_NULL) : pointer(M)
        cin = C2dIn(pointer(A), pointer(Bu), pointer(C), p(Bd), p(Dd), pointer(Ts), C_NULL)
        GC.@preserve Â B̂u Ĉ B̂d D̂d begin
            cout = C2dOut(pointer(Â), pointer(B̂u), pointer(Ĉ), p(B̂d), p(D̂d), C_NULL)
            check(ccall((:mpcqp_c2d, lib), Cint, (Ref{C2dSpec}, Ref{C2dIn}, Ref{C2dOut}, Ptr{Cint}), spec, cin, cout, st))
        end
    end
    return (; Â, B̂u, Ĉ, B̂d, D̂d, status=st)
end

"`setmodel!` of the batch from continuous-time matrices (host arrays): the kernel writes the resident model, K1 and K2 follow.
Estimator gains are not solved again (solve_steadykalmanfilter!, place_luenberger!).  Returns the per-member status."
function setmodel_continuous!(b::BatchLinMPC, spec::C2dSpec, cin::C2dIn)
    st = zeros(Cint, length(b.mpcs))
    check(ccall((:mpcqp_set_model_continuous, lib), Cint, (Ptr{Cvoid}, Ref{C2dSpec}, Ref{C2dIn}, Ptr{Cint}), b.h, spec, cin, st))
    return st
end

"The same with device pointers (`cin` and `status`), asynchronous on `stream`: no host synchronisation up to and including K2."
setmodel_continuous_device!(b::BatchLinMPC, spec::C2dSpec, cin::C2dIn, status::Ptr{Cint}, stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:mpcqp_set_model_continuous_device, lib), Cint, (Ptr{Cvoid}, Ref{C2dSpec}, Ref{C2dIn}, Ptr{Cint}, Ptr{Cvoid}),
                b.h, spec, cin, status, stream))

"The resident model read back: (; Â, B̂u, Ĉ, B̂d, D̂d) in the layouts of mpcqp_set_model (MPCQP_GET_MODEL_*)."
function pull_model(b::BatchLinMPC)
    B, m = length(b.mpcs), b.mpcs[1]
    e = m.estim
    nu, ny, nd = e.model.nu, e.model.ny, e.model.nd
    get(which, dims...) = (M = Array{Float64}(undef, dims...); check(ccall((:mpcqp_get, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), b.h, which, M)); M)
    Â, B̂u, Ĉ = get(16, e.nx̂, e.nx̂, B), get(17, e.nx̂, nu, B), get(18, ny, e.nx̂, B)
    B̂d, D̂d = nd > 0 ? (get(19, e.nx̂, nd, B), get(20, ny, nd, B)) : (zeros(e.nx̂, 0, B), zeros(ny, 0, B))
    return (; Â, B̂u, Ĉ, B̂d, D̂d)
end

# ------------------------------------------------------------------------------------------------
# InternalModel behind the batch (include/mpcqp.h, "InternalModel"): the stochastic model on the measured outputs goes to the
# device once, Âs and B̂s are computed there; per period correct (ŷs, Ŷs, B + Ŷs for the steps), the unchanged step, update.
# Call sequence = BatchLinMPC.setestimator(internal=...) of api.py; these ccalls have not been run.
import ModelPredictiveControl: InternalModel

"As, Bs, Cs, Ds of the batch's InternalModels (restricted to the measured outputs) to the device."
function push_internalmodel!(b::BatchLinMPC)
    es = [c.estim for c in b.mpcs]
    all(e -> e isa InternalModel && e.i_ym == es[1].i_ym && e.nxs == es[1].nxs, es) || throw(ArgumentError("InternalModels with one i_ym and nxs"))
    iy = es[1].i_ym
    stack3(f) = cat((Matrix{Float64}(f(e)) for e in es)...; dims=3)
    As, Bs, Cs, Ds = stack3(e -> e.As), stack3(e -> e.Bs[:, iy]), stack3(e -> e.Cs[iy, :]), stack3(e -> e.Ds[iy, iy])
    i_ym = Cint.(iy .- 1)                                                    # 0-based
    GC.@preserve As Bs Cs Ds i_ym check(ccall((:mpcqp_im_set, lib), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Cint), b.h, es[1].nxs, As, Bs, Cs, Ds, i_ym, length(i_ym)))
    return b
end

"preparestate! of the batch: ŷs and Ŷs from x̂0 = x̂d (nx, B) and y0m (nym, B); x̂0 is not changed."
correct_internalmodel!(b::BatchLinMPC, x̂0::Matrix{Float64}, y0m::Matrix{Float64}, d0::Matrix{Float64}=zeros(0, size(x̂0, 2))) =
    GC.@preserve x̂0 y0m d0 check(ccall((:mpcqp_im_correct, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                       b.h, x̂0, y0m, isempty(d0) ? C_NULL : pointer(d0)))

"updatestate! of the batch: x̂d in place, x̂s on the device."
update_internalmodel!(b::BatchLinMPC, x̂0::Matrix{Float64}, u0::Matrix{Float64}, d0::Matrix{Float64}=zeros(0, size(x̂0, 2))) =
    GC.@preserve x̂0 u0 d0 check(ccall((:mpcqp_im_update, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                      b.h, x̂0, u0, isempty(d0) ? C_NULL : pointer(d0)))

"The device entry points (asynchronous on `stream`) and the set-up's status (2: Ds singular)."
correct_internalmodel_device!(b::BatchLinMPC, x̂0::Ptr{Float64}, y0m::Ptr{Float64}, d0::Ptr{Float64}, stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:mpcqp_im_correct_device, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}), b.h, x̂0, y0m, d0, stream))
update_internalmodel_device!(b::BatchLinMPC, x̂0::Ptr{Float64}, u0::Ptr{Float64}, d0::Ptr{Float64}, stream::Ptr{Cvoid}=C_NULL) =
    check(ccall((:mpcqp_im_update_device, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}), b.h, x̂0, u0, d0, stream))
function internalmodel_status(b::BatchLinMPC)
    st = Vector{Cint}(undef, length(b.mpcs))
    check(ccall((:mpcqp_im_status, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}), b.h, st))
    return st
end

# ------------------------------------------------------------------------------------------------
# Batch of linear MovingHorizonEstimator objects (include/mpcqp_mhe.h; SURVEY 8 row f2).  The estimators keep
# their Julia fields; preparestate! / updatestate! of the BATCH run on the device.  Call sequence = the one of
# modelpredictivecontrol.jl_amd/mhe.py (BatchMHE), which the GPU tests drive.
import ModelPredictiveControl: preparestate!, updatestate!, MovingHorizonEstimator

struct MheDims                        # == mpcqp_mhe_dims
    batch::Cint; nxhat::Cint; nu::Cint; nym::Cint; nd::Cint; He::Cint; direct::Cint; device::Cint
    flags::Cuint; max_iter::Cint; gap_tol::Cdouble; res_tol::Cdouble; dual_reg::Cdouble
end

mutable struct BatchMHE
    h::Ptr{Cvoid}
    estims::Vector{MovingHorizonEstimator}
    x̂0::Matrix{Float64}              # (nx̂, B)
end

function BatchMHE(estims::Vector{<:MovingHorizonEstimator}; device::Integer=0)
    e = estims[1]; B = length(estims); model = e.model
    d = MheDims(B, e.nx̂, model.nu, e.nym, model.nd, e.He, e.direct ? 1 : 0, device, 0, 0, 0.0, 0.0, 0.0)
    h = Ref{Ptr{Cvoid}}()
    check(ccall((:mpcqp_mhe_create, lib), Cint, (Ref{MheDims}, Ref{Ptr{Cvoid}}), d, h))
    cat3(f) = cat((Matrix(f(c)) for c in estims)...; dims=3)
    cat2(f) = hcat((f(c) for c in estims)...)
    nd = model.nd
    check(ccall((:mpcqp_mhe_set_model, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
          Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h[],
          cat3(c -> c.Â), cat3(c -> c.B̂u), cat3(c -> c.Ĉm), nd > 0 ? cat3(c -> c.B̂d) : C_NULL,
          nd > 0 ? cat3(c -> c.D̂dm) : C_NULL, cat2(c -> c.f̂op - c.x̂op), cat3(c -> c.cov.Q̂), cat3(c -> c.cov.R̂)))
    # bounds of setconstraint! as the reference keeps them: window-long vectors (con.x̂0min for the arrival state, then
    # con.X̂0min; con.Ŵmin; con.V̂min -- a per-channel keyword fills the whole vector, construct.jl:890-935), so the
    # window-long entry points are the faithful binding whatever mix of keywords the user called
    check(ccall((:mpcqp_mhe_set_bounds_window, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
          Ptr{Float64}, Ptr{Float64}), h[],
          cat2(c -> vcat(c.con.x̂0min, c.con.X̂0min)), cat2(c -> vcat(c.con.x̂0max, c.con.X̂0max)),
          cat2(c -> Vector(c.con.Ŵmin)), cat2(c -> Vector(c.con.Ŵmax)), cat2(c -> Vector(c.con.V̂min)), cat2(c -> Vector(c.con.V̂max))))
    if !isinf(e.C)         # soft constraints: Cwt and the softness of every row (first column of the A_* matrices = -C, construct.jl:964-1000)
        check(ccall((:mpcqp_mhe_set_softness_window, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
              Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h[], [c.C for c in estims],
              cat2(c -> vcat(-Vector(c.con.A_x̂min[:, 1]), c.con.C_x̂min)), cat2(c -> vcat(-Vector(c.con.A_x̂max[:, 1]), c.con.C_x̂max)),
              cat2(c -> -Vector(c.con.A_Ŵmin[:, 1])), cat2(c -> -Vector(c.con.A_Ŵmax[:, 1])),
              cat2(c -> Vector(c.con.C_v̂min)), cat2(c -> Vector(c.con.C_v̂max))))
    end
    x̂0 = cat2(c -> c.x̂0)
    check(ccall((:mpcqp_mhe_init, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h[],
          x̂0, cat3(c -> c.cov.P̂_0), nd > 0 ? cat2(c -> c.D0[1:nd]) : C_NULL, cat2(c -> c.lastu0)))
    return BatchMHE(h[], estims, x̂0)
end

function pull_state!(b::BatchMHE)
    check(ccall((:mpcqp_mhe_get, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), b.h, 0 #= MPCQP_MHE_XHAT0 =#, b.x̂0))
    for (i, c) in enumerate(b.estims); c.x̂0 .= @view b.x̂0[:, i]; end
    return b.x̂0 .+ hcat((c.x̂op for c in b.estims)...)
end

# preparestate!(estim, ym, d) over the batch (execute.jl:44-57): ym (nym, B), d (nd, B)
function preparestate!(b::BatchMHE, ym::AbstractMatrix, d::AbstractMatrix=zeros(0, size(ym, 2)))
    e = b.estims[1]
    y0m = ym .- hcat((c.model.yop[c.i_ym] for c in b.estims)...)
    d0 = d .- hcat((c.model.dop for c in b.estims)...)
    nbad = ccall((:mpcqp_mhe_prepare, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), b.h, y0m,
                 e.model.nd > 0 ? d0 : C_NULL)
    nbad < 0 && check(nbad)
    nbad > 0 && @warn "MHE termination status not OPTIMAL for $nbad estimators: keeping the open-loop estimate"
    return pull_state!(b)
end

# updatestate!(estim, u, ym, d) over the batch (execute.jl:76-88)
function updatestate!(b::BatchMHE, u::AbstractMatrix, ym::AbstractMatrix, d::AbstractMatrix=zeros(0, size(ym, 2)))
    e = b.estims[1]
    u0 = u .- hcat((c.model.uop for c in b.estims)...)
    y0m = ym .- hcat((c.model.yop[c.i_ym] for c in b.estims)...)
    d0 = d .- hcat((c.model.dop for c in b.estims)...)
    nbad = ccall((:mpcqp_mhe_update, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.h, u0, y0m,
                 e.model.nd > 0 ? d0 : C_NULL)
    nbad < 0 && check(nbad)
    return pull_state!(b)
end

end # module
