# MIOC.jl -- Julia binding of libmioc (include/mioc.h) for the reference's trust-region subproblem.
#
# A maintainer of Jonas477/mixed-integer-optimal-control---algorithm-tools adds this file next to
# multi-trust.jl and makes the three edits shown in INTEGRATION.md.  Only `ccall` and Base are used, so
# it adds no package dependency.  The switching-cost weights for p not in {1, Inf} are computed here,
# with Julia's own `^`, exactly as HelpFunctions.jl:63-67 computes them, so the device uses
# bit-identical weights for every p.
module MIOC

export Context, set_levels!, set_cost!, bellman_TRM!, eval_u_TRM!

const libmioc = get(ENV, "MIOC_LIB",
    joinpath(@__DIR__, "..", "mixed-integer-optimal-control---algorithm-tools_amd", "lib", "libmioc.so"))

const MIOC_OK = Int32(0)
const MIOC_EINEXACT = Int32(-2)
const P_INF, P_ONE, P_INTLUT, P_TABLE = Int32(0), Int32(1), Int32(2), Int32(3)
# mioc_set_option: 0 keeps the separable DP on the general persistent driver (default 1: the one-row driver where it fits)
const MIOC_OPT_SDT_ROW_OWNER = Int32(10)

mutable struct Context
    ptr::Ptr{Cvoid}
    M::Int
    L::Int
    nu::Vector{Vector{Int64}}
    tuples::Vector{NTuple}
end

function check(ctx::Context, rc::Int32)
    rc == MIOC_OK && return nothing
    msg = unsafe_string(ccall((:mioc_last_error, libmioc), Cstring, (Ptr{Cvoid},), ctx.ptr))
    # the reference raises InexactError from convert(Int64, ...) (HelpFunctions.jl:37,57)
    rc == MIOC_EINEXACT && throw(InexactError(:convert, Int64, msg))
    error("libmioc error $rc: $msg")
end

function destroy!(ctx::Context)
    if ctx.ptr != C_NULL
        ccall((:mioc_destroy, libmioc), Int32, (Ptr{Cvoid},), ctx.ptr)
        ctx.ptr = C_NULL
    end
    nothing
end

"""
    Context(device = 0)

Device context: owns the value fronts and the compact argmin table that replace `U` and `Φ`
(multi-trust.jl:71-77).  Not thread-safe; use one per task.
"""
function Context(device::Integer = 0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:mioc_create, libmioc), Int32, (Int32, Ptr{Ptr{Cvoid}}), device, r)
    rc == MIOC_OK || error("mioc_create(device=$device) failed with $rc (no visible HIP device?)")
    ctx = Context(r[], 0, 0, Vector{Int64}[], NTuple[])
    finalizer(destroy!, ctx)
end

"""
    set_levels!(ctx, nu, iterator)

Flatten `obj.𝓥` and `obj.iterator` (product_iterator / bounded_sum_iterator,
AdmissibleIterators.jl:9-49) into the device level table, keeping the iterator order.
"""
function set_levels!(ctx::Context, nu::Vector{Vector{Int64}}, iterator)
    M = length(nu)
    tup = [Tuple(t) for t in iterator]
    counts = Int64[length(v) for v in nu]
    values = reduce(vcat, nu)
    flat = Int32[t[m] for t in tup for m in 1:M]          # tuple-major, 1-based
    check(ctx, ccall((:mioc_set_levels, libmioc), Int32,
                     (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int32}),
                     ctx.ptr, M, counts, values, length(tup), flat))
    ctx.M, ctx.L, ctx.nu, ctx.tuples = M, length(tup), nu, tup
    nothing
end

# the reference weight (Σ_m |ν_jm - ν_lm|^p)^(1/p) with Julia's own arithmetic (HelpFunctions.jl:63-67)
function ref_weight(nu, l, j, p)
    t = 0.
    for m = 1:length(nu)
        t += abs(nu[m][j[m]] - nu[m][l[m]])^p
    end
    t^(1/p)
end

"""
    set_cost!(ctx, β, p)

p = Inf and p = 1 are evaluated exactly on the device.  Any other p ships Julia's weights: an L×L table
(MIOC_P_TABLE), so every p is bit-identical to the reference loop.
"""
function set_cost!(ctx::Context, β::Float64, p)
    if p == Inf
        kind, tab = P_INF, Float64[]
    elseif p == 1
        kind, tab = P_ONE, Float64[]
    else
        kind = P_TABLE
        # row-major by target l, source j fastest: tab[l*L + j] (0-based ranks), as mioc.h MIOC_P_TABLE
        tab = Float64[ref_weight(ctx.nu, l, j, p) for l in ctx.tuples for j in ctx.tuples]
    end
    check(ctx, ccall((:mioc_set_cost, libmioc), Int32, (Ptr{Cvoid}, Int32, Int64, Float64, Int64, Ptr{Float64}),
                     ctx.ptr, kind, 1, β, length(tab), isempty(tab) ? C_NULL : pointer(tab)))
    nothing
end

"""
    bellman_TRM!(ctx, ∇f, u_old, B, Δt)

Replaces `bellman_TRM!(∇f, u_old, B, β, p, Δt, nu, U, Φ, iterator)` (HelpFunctions.jl:20-83); β, p, nu and
the iterator were bound by set_cost!/set_levels!, and U/Φ stay on the device.
"""
function bellman_TRM!(ctx::Context, ∇f::Matrix{Float64}, u_old::Matrix{Float64}, B::Int64, Δt::Float64)
    nx, nt = size(u_old)
    size(∇f) == (nx, nt) || throw(DimensionMismatch("∇f and u_old differ in shape"))
    check(ctx, ccall((:mioc_bellman, libmioc), Int32,
                     (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Float64),
                     ctx.ptr, ∇f, u_old, nx, nt, B, Δt))
    nothing
end

"""
    eval_u_TRM!(ctx, u, B) -> Φ*

Replaces `eval_u_TRM!(u, u_old, U, Φ, B, nu)` (HelpFunctions.jl:98-124).  `B` may be smaller than the
budget of the last bellman_TRM! call (the halving path, multi-trust.jl:108-110).
"""
function eval_u_TRM!(ctx::Context, u::Matrix{Float64}, B::Int64)
    phi = Ref{Float64}(0.0)
    check(ctx, ccall((:mioc_backtrack, libmioc), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
                     ctx.ptr, B, u, phi, C_NULL))
    phi[]
end

"""
    pred(ctx) -> (int_val, TV_old, TV_new, pred)

The reductions of multi-trust.jl:117-126 for the last eval_u_TRM! on the device: int_val = Δt·Σ_j
∇f[:,j]'(u_old[:,j] - u[:,j]), TV_p (HelpFunctions.jl:251-268) of u_old and of u with the context's p, and
pred = int_val + β(TV_old - TV_new).  Sums run in the reference's loop order.
"""
function pred(ctx::Context)
    iv, to, tn, pr = Ref(0.0), Ref(0.0), Ref(0.0), Ref(0.0)
    check(ctx, ccall((:mioc_pred, libmioc), Int32,
                     (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}, Ref{Float64}, Ref{Float64}), ctx.ptr, iv, to, tn, pr))
    (iv[], to[], tn[], pr[])
end

"""
    heat_setup!(ctx, obj)

Hands the matrices a PDE objective (example_heat.jl's HeatObj, PDEObjective.jl) already holds to the device:
M_invA, M_invF, M, state0, yd, T0, T1, γ (example_heat.jl:101-115).  StateMat = I + τ·M_invA is factored once
there.  Call again whenever those matrices change.
"""
function heat_setup!(ctx::Context, obj)
    M_invA = Matrix{Float64}(obj.M_invA)
    M_invF = Matrix{Float64}(obj.M_invF)
    M = Matrix{Float64}(obj.M)
    N, nx = size(M_invF)
    nt = size(obj.yd, 2) - 1
    check(ctx, ccall((:mioc_heat_setup, libmioc), Int32,
                     (Ptr{Cvoid}, Int64, Int64, Int64, Float64, Float64, Float64,
                      Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     ctx.ptr, N, nx, nt, obj.T0, obj.T1, obj.γ, M_invA, M_invF, M,
                     Vector{Float64}(obj.state0), Matrix{Float64}(obj.yd)))
    nothing
end

"""
    heat_eval!(ctx, x, df) -> fval

eval_f_helper + eval_df_helper of PDEObjective.jl:142-199 for the control x (nx × nt) in one device call: returns
the objective value and, unless `df` is `nothing`, writes the gradient at x into df (nx × nt).
"""
function heat_eval!(ctx::Context, x::Matrix{Float64}, df::Union{Matrix{Float64},Nothing})
    df === nothing || size(df) == size(x) || throw(DimensionMismatch("df and x differ in shape"))
    J = Ref{Float64}(0.0)
    check(ctx, ccall((:mioc_heat_eval, libmioc), Int32,
                     (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Float64}, Ptr{Float64}), ctx.ptr, 1, x, J,
                     df === nothing ? Ptr{Float64}(C_NULL) : df))
    J[]
end

"""
    conv_setup(ctx, obj)

Hands the data of the convolution objective (example_convolution.jl's ConvObj) to the device: κ = obj.K[2:end, 1],
obj.fvec, T0, T1.  The device never stores K: it relies on K being strictly lower triangular Toeplitz
(toeplitz, example_convolution.jl:104-125), which is checked here.  Call again whenever K or fvec change.
"""
function conv_setup(ctx::Context, obj)
    K = obj.K
    nt = Int(size(K, 2))
    size(K, 1) == nt + 1 || throw(DimensionMismatch("K must be (nt+1) x nt"))
    kappa = Vector{Float64}(K[2:end, 1])
    for c in 1:nt, r in 1:nt+1
        K[r, c] == (r - c >= 1 ? kappa[r - c] : 0.0) ||
            throw(ArgumentError("obj.K is not strictly lower triangular Toeplitz at ($r, $c)"))
    end
    fvec = Vector{Float64}(obj.fvec)
    length(fvec) == nt + 1 || throw(DimensionMismatch("fvec must have nt+1 entries"))
    check(ctx, ccall((:mioc_conv_setup, libmioc), Int32,
                     (Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Ptr{Float64}),
                     ctx.ptr, nt, obj.T0, obj.T1, kappa, fvec))
    nothing
end

"""
    conv_eval!(ctx, x, df) -> fval

eval_f_helper + eval_df_helper of example_convolution.jl:128-141 for the control x (1 × nt) in one device call:
returns the objective value and, unless `df` is `nothing`, writes the gradient at x into df (1 × nt).
"""
function conv_eval!(ctx::Context, x::Matrix{Float64}, df::Union{Matrix{Float64},Nothing})
    df === nothing || size(df) == size(x) || throw(DimensionMismatch("df and x differ in shape"))
    J = Ref{Float64}(0.0)
    check(ctx, ccall((:mioc_conv_eval, libmioc), Int32,
                     (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Float64}, Ptr{Float64}), ctx.ptr, 1, x, J,
                     df === nothing ? Ptr{Float64}(C_NULL) : df))
    J[]
end

"""
    conv_eval_device!(ctx, K, d_x, d_J, d_df)

The batched device entry (mioc_conv_eval_device): K controls already in device memory (K × 1 × nt), enqueued on the
context's stream; d_J / d_df may be C_NULL.
"""
function conv_eval_device!(ctx::Context, K::Integer, d_x::Ptr{Float64}, d_J::Ptr{Float64}, d_df::Ptr{Float64})
    check(ctx, ccall((:mioc_conv_eval_device, libmioc), Int32,
                     (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, K, d_x, d_J, d_df))
    nothing
end

# ---- user-defined ODE objectives: the six hooks of an AbstractODEObjective (ODEObjective.jl:243-248) as HIP source
# text, compiled at run time for gfx950 (mioc_ode_program_*; the hook contract is in include/mioc.h) ----------------

const ODE_INTEGRATORS = Dict(:euler => Int32(0), :heun => Int32(1), :rk4 => Int32(2), :beuler => Int32(16),
                             :midpoint => Int32(17))  # MIOC_ODE_INT_*
const ODE_DERIVE = Dict(:Fy => Int32(1), :Fu => Int32(2), :Gy => Int32(4), :Gu => Int32(8))  # MIOC_ODE_DERIVE_*

"""
    ode_program_create(hooks, ny, nx, nparams; integrator = :euler, substeps = 1, derive = Symbol[]) -> Ptr{Cvoid}

Compile the hook text (needs no context and no GPU).  A compile failure raises an error carrying the compiler's log,
whose diagnostics name the text's own lines (`hooks:3:…`).  mioc_ode_program_create_ex: `:euler` is the reference's
scheme, what mioc_ode_program_create compiles (substeps must be 1); `:heun` and `:rk4` take `substeps` (1..64) steps inside every control interval and return the exact gradient of their
discrete objective, so the control grid nt (and with it the DP) can be much coarser (include/mioc.h, "Integrators").
`:beuler` (backward Euler) and `:midpoint` (the implicit midpoint rule) are the implicit schemes for stiff dynamics,
with `substeps` likewise: Newton's method per substep on the device (at most 12 updates, relative size 1e-10), the
gradient by the implicit function theorem; a restart whose iteration fails has NaN for J and its df row
(include/mioc.h, "Implicit integrators").
The program carries both; `ode_program_eval_device!` is unchanged.
`derive` (mioc_ode_program_create_ad): `:all` or a collection of `:Fy`, `:Fu`, `:Gy`, `:Gu`, the hooks that the library
generates from F and G by forward-mode AD; the text then defines F and G as templates over the scalar type and only
the other hooks by hand (include/mioc.h, "Derived hooks").  Empty: all six hooks are the text's, as before.
"""
function ode_program_create(hooks::String, ny::Integer, nx::Integer, nparams::Integer; integrator::Symbol = :euler,
                            substeps::Integer = 1, derive = Symbol[])
    haskey(ODE_INTEGRATORS, integrator) || error("integrator must be :euler, :heun, :rk4, :beuler or :midpoint")
    names = derive === :all ? collect(keys(ODE_DERIVE)) : collect(derive)
    all(n -> haskey(ODE_DERIVE, n), names) || error("derive must be :all or a collection of :Fy, :Fu, :Gy, :Gu")
    mask = reduce(|, (ODE_DERIVE[n] for n in names); init = Int32(0))
    r = Ref{Ptr{Cvoid}}(C_NULL)
    log = zeros(UInt8, 1 << 16)
    rc = ccall((:mioc_ode_program_create_ad, libmioc), Int32,
               (Cstring, Int32, Int32, Int32, Int32, Int32, Int32, Ptr{Ptr{Cvoid}}, Ptr{UInt8}, Int64), hooks, ny, nx,
               nparams, ODE_INTEGRATORS[integrator], substeps, mask, r, log, length(log))
    rc == MIOC_OK || error("mioc_ode_program_create_ad failed with $rc:\n" * unsafe_string(pointer(log)))
    r[]
end

"""
    ode_program_destroy(prog)

Unload and free a program (after the work that uses it: every device it ran on is synchronised first).
"""
ode_program_destroy(prog::Ptr{Cvoid}) = (ccall((:mioc_ode_program_destroy, libmioc), Int32, (Ptr{Cvoid},), prog); nothing)

"""
    ode_program_eval_device!(ctx, prog, K, d_x, nt, T0, T1, state0, params, d_J, d_df)

The batched device entry (mioc_ode_program_eval_device): K controls already in device memory (K × nx × nt), enqueued
on the context's stream; state0 (ny) and params (nparams) are host vectors; d_J / d_df may be C_NULL.
"""
function ode_program_eval_device!(ctx::Context, prog::Ptr{Cvoid}, K::Integer, d_x::Ptr{Float64}, nt::Integer,
                                  T0::Float64, T1::Float64, state0::Vector{Float64}, params::Vector{Float64},
                                  d_J::Ptr{Float64}, d_df::Ptr{Float64})
    check(ctx, ccall((:mioc_ode_program_eval_device, libmioc), Int32,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Float64, Float64, Ptr{Float64}, Ptr{Float64},
                      Ptr{Float64}, Ptr{Float64}), ctx.ptr, prog, K, d_x, nt, T0, T1, state0, params, d_J, d_df))
    nothing
end

# ---- a terminal cost, sampled data and the state trajectory (include/mioc.h, "Terminal cost, sampled data, state
# output").  Thin wrappers of the two entries; they have not been run under Julia (none is installed where this was
# written).
const MIOC_ODE_TERMINAL = Int32(1)
const MIOC_ODE_STATES = Int32(2)
const MIOC_ODE_DERIVE_EY = Int32(16)

"""
    ode_program_create_bolza(hooks, ny, nx, nparams; ndata = 0, terminal = false, states = false,
                             integrator = :euler, substeps = 1, derive = Symbol[]) -> Ptr{Cvoid}

`ode_program_create` with `ndata` (0..16) columns of sampled data behind the parameters (`p[NP + e]`), a terminal cost
(`terminal`: the text also defines E and Ey, or `derive` names `:Ey`; `:all` then includes it) and the state
trajectory as an output (`states`) (mioc_ode_program_create_bolza).
"""
function ode_program_create_bolza(hooks::String, ny::Integer, nx::Integer, nparams::Integer; ndata::Integer = 0,
                                  terminal::Bool = false, states::Bool = false, integrator::Symbol = :euler,
                                  substeps::Integer = 1, derive = Symbol[])
    haskey(ODE_INTEGRATORS, integrator) || error("integrator must be :euler, :heun, :rk4, :beuler or :midpoint")
    bits = terminal ? merge(ODE_DERIVE, Dict(:Ey => MIOC_ODE_DERIVE_EY)) : ODE_DERIVE
    names = derive === :all ? collect(keys(bits)) : collect(derive)
    all(n -> haskey(bits, n), names) ||
        error("derive must be :all or a collection of :Fy, :Fu, :Gy, :Gu (:Ey with terminal)")
    mask = reduce(|, (bits[n] for n in names); init = Int32(0))
    flags = (terminal ? MIOC_ODE_TERMINAL : Int32(0)) | (states ? MIOC_ODE_STATES : Int32(0))
    r = Ref{Ptr{Cvoid}}(C_NULL)
    log = zeros(UInt8, 1 << 16)
    rc = ccall((:mioc_ode_program_create_bolza, libmioc), Int32,
               (Cstring, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Ptr{Ptr{Cvoid}}, Ptr{UInt8}, Int64),
               hooks, ny, nx, nparams, ndata, ODE_INTEGRATORS[integrator], substeps, mask, flags, r, log, length(log))
    rc == MIOC_OK || error("mioc_ode_program_create_bolza failed with $rc:\n" * unsafe_string(pointer(log)))
    r[]
end

"""
    ode_program_eval_bolza_device!(ctx, prog, nu, K, d_x, nt, T0, T1, state0, params, d_data, d_J, d_df, d_Y)

The eval entry with the data (`d_data`: nt × ndata doubles on the device, row i for control column i; C_NULL for a
program without data) and the states (`d_Y`: K × (nt+1) × ny doubles, or C_NULL).  `nu = 0`: every control is the
DP's; `nu ≥ 1`: a mixed control (mioc_ode_program_eval_bolza_device).
"""
function ode_program_eval_bolza_device!(ctx::Context, prog::Ptr{Cvoid}, nu::Integer, K::Integer, d_x::Ptr{Float64},
                                        nt::Integer, T0::Float64, T1::Float64, state0::Vector{Float64},
                                        params::Vector{Float64}, d_data::Ptr{Float64}, d_J::Ptr{Float64},
                                        d_df::Ptr{Float64}, d_Y::Ptr{Float64})
    check(ctx, ccall((:mioc_ode_program_eval_bolza_device, libmioc), Int32,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Float64, Float64, Ptr{Float64},
                      Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, prog, nu, K, d_x,
                     nt, T0, T1, state0, params, d_data, d_J, d_df, d_Y))
    nothing
end

# ---- scenarios: restart q of a call solves scenario q % S (include/mioc.h, "Scenarios").  Thin wrappers of the two
# entries; they have not been run under Julia (none is installed where this was written).
const MIOC_ODE_SCEN = Int32(1)
const MIOC_ODE_SCEN_DATA = Int32(2)

"""
    ode_program_create_scen(hooks, ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen) -> Ptr{Cvoid}

mioc_ode_program_create_scen with the C entry's own integer arguments (`integrator`: a value of `ODE_INTEGRATORS`;
`scen`: `MIOC_ODE_SCEN`, or `MIOC_ODE_SCEN | MIOC_ODE_SCEN_DATA` with `ndata > 0`; 0 is `ode_program_create_bolza`).
"""
function ode_program_create_scen(hooks::String, ny::Integer, nx::Integer, nparams::Integer, ndata::Integer,
                                 integrator::Integer, substeps::Integer, derive::Integer, flags::Integer,
                                 scen::Integer)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    log = zeros(UInt8, 1 << 16)
    rc = ccall((:mioc_ode_program_create_scen, libmioc), Int32,
               (Cstring, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Ptr{Ptr{Cvoid}}, Ptr{UInt8},
                Int64), hooks, ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen, r, log, length(log))
    rc == MIOC_OK || error("mioc_ode_program_create_scen failed with $rc:\n" * unsafe_string(pointer(log)))
    r[]
end

"""
    ode_program_source_scen(hooks, ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen; noinline = false)

The text `ode_program_create_scen` would compile (mioc_ode_program_source_scen), as a String.
"""
function ode_program_source_scen(hooks::String, ny::Integer, nx::Integer, nparams::Integer, ndata::Integer,
                                 integrator::Integer, substeps::Integer, derive::Integer, flags::Integer,
                                 scen::Integer; noinline::Bool = false)
    sig = (Cstring, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Ptr{UInt8}, Int64)
    need = ccall((:mioc_ode_program_source_scen, libmioc), Int64, sig, hooks, ny, nx, nparams, ndata, integrator,
                 substeps, derive, flags, scen, noinline, C_NULL, 0)
    need >= 0 || error("mioc_ode_program_source_scen failed with $need")
    buf = zeros(UInt8, need + 1)
    ccall((:mioc_ode_program_source_scen, libmioc), Int64, sig, hooks, ny, nx, nparams, ndata, integrator, substeps,
          derive, flags, scen, noinline, buf, length(buf))
    unsafe_string(pointer(buf))
end

"""
    ode_program_eval_scen_device!(ctx, prog, nu, K, d_x, nt, T0, T1, S, d_state0, d_params, d_data, d_J, d_df, d_Y)

`ode_program_eval_bolza_device!` for a program compiled with scenarios (mioc_ode_program_eval_scen_device): device
arrays with the scenario index fastest, `d_state0` ny × S, `d_params` nparams × S (C_NULL with nparams = 0), `d_data`
nt × ndata, or nt × ndata × S with `MIOC_ODE_SCEN_DATA`; K must be a multiple of S.
"""
function ode_program_eval_scen_device!(ctx::Context, prog::Ptr{Cvoid}, nu::Integer, K::Integer, d_x::Ptr{Float64},
                                       nt::Integer, T0::Float64, T1::Float64, S::Integer, d_state0::Ptr{Float64},
                                       d_params::Ptr{Float64}, d_data::Ptr{Float64}, d_J::Ptr{Float64},
                                       d_df::Ptr{Float64}, d_Y::Ptr{Float64})
    check(ctx, ccall((:mioc_ode_program_eval_scen_device, libmioc), Int32,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Float64, Float64, Int64, Ptr{Float64},
                      Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, prog, nu, K, d_x,
                     nt, T0, T1, S, d_state0, d_params, d_data, d_J, d_df, d_Y))
    nothing
end

# ---- sensitivities: dJ/dparams and dJ/dstate0 as outputs of an evaluation (include/mioc.h, "Sensitivities").  Thin
# wrappers of the two entries, like those of the scenarios; they have not been run under Julia.
const MIOC_ODE_SENS_P = Int32(1)
const MIOC_ODE_SENS_Y0 = Int32(2)
const MIOC_ODE_DERIVE_FP = Int32(32)
const MIOC_ODE_DERIVE_GP = Int32(64)
const MIOC_ODE_DERIVE_EP = Int32(128)

"""
    ode_program_create_sens(hooks, ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen, sens) -> Ptr{Cvoid}

mioc_ode_program_create_sens with the C entry's own integer arguments (`sens`: `MIOC_ODE_SENS_P`, `MIOC_ODE_SENS_Y0` or
both; 0 is `ode_program_create_scen`; not with the integrator `:euler`).  With `MIOC_ODE_SENS_P` the text also defines
Fp, Gp (and Ep with a terminal cost), or `derive` carries `MIOC_ODE_DERIVE_FP` / `_GP` / `_EP` and F, G, E are
templates over the state type and the parameter type.
"""
function ode_program_create_sens(hooks::String, ny::Integer, nx::Integer, nparams::Integer, ndata::Integer,
                                 integrator::Integer, substeps::Integer, derive::Integer, flags::Integer,
                                 scen::Integer, sens::Integer)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    log = zeros(UInt8, 1 << 16)
    rc = ccall((:mioc_ode_program_create_sens, libmioc), Int32,
               (Cstring, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Ptr{Ptr{Cvoid}},
                Ptr{UInt8}, Int64), hooks, ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen, sens, r,
               log, length(log))
    rc == MIOC_OK || error("mioc_ode_program_create_sens failed with $rc:\n" * unsafe_string(pointer(log)))
    r[]
end

"""
    ode_program_eval_sens_device!(ctx, prog, nu, K, d_x, nt, T0, T1, S, state0, params, d_data, d_J, d_df, d_Y,
                                  d_Jp, d_Jy0)

The eval entry with the sensitivities (mioc_ode_program_eval_sens_device): `d_Jp` K × nparams and `d_Jy0` K × ny
doubles on the device, each or C_NULL.  `S = 0`: a program without scenarios, `state0` and `params` are host
`Vector{Float64}` as for `ode_program_eval_bolza_device!`; `S ≥ 1`: a scenario program, they are device pointers as for
`ode_program_eval_scen_device!`, and restart q's rows are the derivatives in scenario q % S's own values.
"""
function ode_program_eval_sens_device!(ctx::Context, prog::Ptr{Cvoid}, nu::Integer, K::Integer, d_x::Ptr{Float64},
                                       nt::Integer, T0::Float64, T1::Float64, S::Integer,
                                       state0::Union{Vector{Float64},Ptr{Float64}},
                                       params::Union{Vector{Float64},Ptr{Float64}}, d_data::Ptr{Float64},
                                       d_J::Ptr{Float64}, d_df::Ptr{Float64}, d_Y::Ptr{Float64}, d_Jp::Ptr{Float64},
                                       d_Jy0::Ptr{Float64})
    check(ctx, ccall((:mioc_ode_program_eval_sens_device, libmioc), Int32,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Float64, Float64, Int64, Ptr{Float64},
                      Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     ctx.ptr, prog, nu, K, d_x, nt, T0, T1, S, state0, params, d_data, d_J, d_df, d_Y, d_Jp, d_Jy0))
    nothing
end

# ---- mixed controls: nu continuous controls in front of the DP's integer ones (include/mioc.h, "Mixed controls").
# Thin wrappers of the six entries; they have not been run under Julia (none is installed where this was written).

"""
    ode_program_eval_mixed_device!(ctx, prog, nu, K, d_x, nt, T0, T1, state0, params, d_J, d_df)

`ode_program_eval_device!` for a mixed control: the first `nu` of the program's nx controls are continuous and the
context's levels describe the other nx - nu (mioc_ode_program_eval_mixed_device).  K may be the K·R candidates of a fan.
"""
function ode_program_eval_mixed_device!(ctx::Context, prog::Ptr{Cvoid}, nu::Integer, K::Integer, d_x::Ptr{Float64},
                                        nt::Integer, T0::Float64, T1::Float64, state0::Vector{Float64},
                                        params::Vector{Float64}, d_J::Ptr{Float64}, d_df::Ptr{Float64})
    check(ctx, ccall((:mioc_ode_program_eval_mixed_device, libmioc), Int32,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Float64, Float64, Ptr{Float64},
                      Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, prog, nu, K, d_x, nt, T0, T1, state0, params,
                     d_J, d_df))
    nothing
end

"""
    rows_copy_device!(ctx, K, nt, d_dst, dst_nx, dst_row0, d_src, src_nx, src_row0, nrows)

dst[k][i][dst_row0 + r] = src[k][i][src_row0 + r] (0-based rows, r < nrows): the split and the join around the DP
(mioc_rows_copy_device); enqueued, gated by the TRM state's gate word.
"""
function rows_copy_device!(ctx::Context, K::Integer, nt::Integer, d_dst::Ptr{Float64}, dst_nx::Integer,
                           dst_row0::Integer, d_src::Ptr{Float64}, src_nx::Integer, src_row0::Integer, nrows::Integer)
    check(ctx, ccall((:mioc_rows_copy_device, libmioc), Int32,
                     (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64), ctx.ptr,
                     K, nt, d_dst, dst_nx, dst_row0, d_src, src_nx, src_row0, nrows))
    nothing
end

"""
    mixed_state_bytes(K)

Bytes of the device state block of the continuous step for K restarts (mioc_mixed_state_bytes): zero it and write the
first step size into its K doubles at offset 16.
"""
mixed_state_bytes(K::Integer) = ccall((:mioc_mixed_state_bytes, libmioc), Int64, (Int64,), K)

"""
    mixed_fan_device!(ctx, K, R, nu, nx, nt, tau, d_x, d_df, d_lo, d_hi, d_mstate, d_xfan, d_slope)

The R line-search candidates of every restart and their Armijo slopes (mioc_mixed_fan_device); d_xfan is R × K × nx × nt.
"""
function mixed_fan_device!(ctx::Context, K::Integer, R::Integer, nu::Integer, nx::Integer, nt::Integer, tau::Float64,
                           d_x::Ptr{Float64}, d_df::Ptr{Float64}, d_lo::Ptr{Float64}, d_hi::Ptr{Float64},
                           d_mstate::Ptr{Cvoid}, d_xfan::Ptr{Float64}, d_slope::Ptr{Float64})
    check(ctx, ccall((:mioc_mixed_fan_device, libmioc), Int32,
                     (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Int64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                      Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, K, R, nu, nx, nt, tau, d_x, d_df,
                     d_lo, d_hi, d_mstate, d_xfan, d_slope))
    nothing
end

"""
    mixed_select_device!(ctx, K, R, nu, nx, nt, c1, smax, ctol, d_mstate, d_trm_state, d_xfan, d_slope, d_Jfan, d_J_old, d_x)

Per restart the first candidate that passes the Armijo test, the step-size update and the finality rule
(mioc_mixed_select_device).
"""
function mixed_select_device!(ctx::Context, K::Integer, R::Integer, nu::Integer, nx::Integer, nt::Integer, c1::Float64,
                              smax::Float64, ctol::Float64, d_mstate::Ptr{Cvoid}, d_trm_state::Ptr{Cvoid},
                              d_xfan::Ptr{Float64}, d_slope::Ptr{Float64}, d_Jfan::Ptr{Float64}, d_J_old::Ptr{Float64},
                              d_x::Ptr{Float64})
    check(ctx, ccall((:mioc_mixed_select_device, libmioc), Int32,
                     (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Int64, Float64, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid},
                      Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, K, R, nu, nx, nt,
                     c1, smax, ctol, d_mstate, d_trm_state, d_xfan, d_slope, d_Jfan, d_J_old, d_x))
    nothing
end

"""
    mixed_poll(ctx, d_mstate, d_trm_state) -> (inner, live)

One stream synchronisation: any restart inside its inner loop, any restart that can still move (mioc_mixed_poll).
"""
function mixed_poll(ctx::Context, d_mstate::Ptr{Cvoid}, d_trm_state::Ptr{Cvoid})
    out = zeros(Int32, 2)
    check(ctx, ccall((:mioc_mixed_poll, libmioc), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}), ctx.ptr,
                     d_mstate, d_trm_state, out))
    (out[1] != 0, out[2] != 0)
end

end # module
