# ColumnNDE.jl — thin `ccall` layer over libcolnde.so (include/colnde.h) that keeps the reference's call signatures.
# NOT EXECUTED IN THIS REPOSITORY'S CI: the build image has no Julia (SURVEY §8c).  It mirrors, call for call, the ctypes front-end
# that IS tested (climateparameterizations.jl_amd/nde.py, wind_mixing.py, free_convection.py, distributed.py); the struct layout it
# relies on is checked field by field against include/colnde.h by tests/test_abi.py::test_julia_config_mirrors_the_header, and the
# same ABI is driven from plain C by tests/abi_smoke.c.
module ColumnNDE

using Flux, ChainRulesCore

const libcolnde = get(ENV, "COLNDE_LIB", "libcolnde.so")

# mirror of `colnde_config` (field order = include/colnde.h)
Base.@kwdef mutable struct Config
    model::Int32 = 0; Nz::Int32 = 32; n_layers::Int32 = 3
    layer_sizes::NTuple{9,Int32} = (96, 50, 20, 31, 0, 0, 0, 0, 0)
    activations::NTuple{8,Int32} = (2, 2, 0, 0, 0, 0, 0, 0)              # COLNDE_ACT_MISH, MISH, IDENTITY
    modified_pacanowski_philander::Int32 = 1; convective_adjustment::Int32 = 0; zero_weights::Int32 = 1
    smooth_NN::Int32 = 0; smooth_Ri::Int32 = 0; diurnal::Int32 = 0; train_gradient::Int32 = 1; inplace_variant::Int32 = 0
    H::Float32 = 256; tau::Float32 = 172800; f::Float32 = 1f-4; g::Float32 = 9.81f0; alpha::Float32 = 1.67f-4
    nu0::Float32 = 1f-4; nu_minus::Float32 = 1f-1; Ric::Float32 = 0.25f0; dRi::Float32 = 1f0; Pr::Float32 = 1f0
    kappa::Float32 = 10f0; eps::Float32 = 1f-7
    mu::NTuple{6,Float32} = (0, 0, 0, 0, 0, 0); sigma::NTuple{6,Float32} = (1, 1, 1, 1, 1, 1)
    ca_K::Float32 = 10f0
    n_save::Int32 = 2; substeps::Int32 = 2; save_times::Ptr{Float32} = C_NULL
    n_columns::Int32 = 1; device::Int32 = 0; engine::Int32 = 0
    stepper::Int32 = 0; rkc_stages::Int32 = 0                            # COLNDE_STEPPER_RK4 / _RKC2 (stands where the reference uses ROCK4)
    matrix_arithmetic::Int32 = 0                                         # COLNDE_MATRIX_BF16X3_EXACT (0, default) / COLNDE_MATRIX_F32_MFMA (1)
    reltol::Float32 = 0                                                  # solve(...; reltol=1f-3) (0 = 1f-3); with substeps = 0 the handle chooses the sub-step count from it
end

const MATRIX_BF16X3_EXACT = Int32(0)   # Float32 Dense products as six bf16 MFMA products of exact three-way operand splits, f32 accumulation
const MATRIX_F32_MFMA = Int32(1)       # v_mfma_f32_* throughout

check(rc) = rc == 0 || error(unsafe_string(ccall((:colnde_last_error, libcolnde), Cstring, ())))

mutable struct Handle
    ptr::Ptr{Cvoid}; n_params::Int; n_state::Int; n_save::Int; n_columns::Int; n_nets::Int
end

"least RK4 sub-steps per save interval inside the stability bound / stages of the RKC2 step (no GPU needed)"
function min_substeps(cfg::Config, save_times::Vector{Float32})
    cfg.n_save = length(save_times)
    GC.@preserve save_times begin
        cfg.save_times = pointer(save_times)
        ccall((:colnde_min_substeps, libcolnde), Cint, (Ref{Config},), cfg)
    end
end
function rkc_stages(cfg::Config, save_times::Vector{Float32})
    cfg.n_save = length(save_times)
    GC.@preserve save_times begin
        cfg.save_times = pointer(save_times)
        ccall((:colnde_rkc_stages, libcolnde), Cint, (Ref{Config},), cfg)
    end
end

"constants/scalings/conditions as built by prepare_parameters_NDE_training (NDE_training.jl:1-44); t_train ./ τ as save_times"
function Handle(cfg::Config, save_times::Vector{Float32})
    cfg.n_save = length(save_times)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve save_times begin
        cfg.save_times = pointer(save_times)
        check(ccall((:colnde_create, libcolnde), Cint, (Ref{Config}, Ref{Ptr{Cvoid}}), cfg, out))
    end
    h = Handle(out[], ccall((:colnde_n_params, libcolnde), Cint, (Ptr{Cvoid},), out[]),
               cfg.model == 0 ? 3cfg.Nz : cfg.Nz, cfg.n_save, cfg.n_columns, cfg.model == 0 ? 3 : 1)
    finalizer(x -> ccall((:colnde_destroy, libcolnde), Cvoid, (Ptr{Cvoid},), x.ptr), h)
end

"uvT₀s, BCs, uvT_trains of train_NDE (NDE_training.jl:220-243): one column per simulation"
set_problem!(h::Handle, uvT₀s::Matrix{Float32}, BCs::Matrix{Float32}, uvT_trains::Union{Nothing,Array{Float32,3}}) =
    check(ccall((:colnde_set_problem, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                h.ptr, uvT₀s, BCs, uvT_trains === nothing ? C_NULL : uvT_trains))   # Julia 96×n / 6×n / 96×Nt×n arrays ARE the C layouts

"NDE(x, p, t) with p = [weights; BCs] — wind_mixing/src/NDE_training.jl:56-66"
function NDE(h::Handle, x::Vector{Float32}, p::Vector{Float32}, t)
    dx = similar(x)
    NDE!(h, dx, x, p, t); dx
end

"diurnal overload NDE(x, p, t) — NDE_training.jl:68-81: `p` carries only 5 BCs, wT_top(t) comes from Qᵇ (parsed from the file name,
data_containers.jl:138-152); create the handle with diurnal = 1 and pass Qᵇ here (it fills the sixth BC slot of the C ABI)"
function NDE(h::Handle, x::Vector{Float32}, p::Vector{Float32}, t, Qᵇ::Real)
    length(p) == h.n_params + 5 || error("the diurnal NDE takes p = [weights; uw_b, uw_t, vw_b, vw_t, wT_b]")
    NDE(h, x, vcat(p, Float32(Qᵇ)), t)
end

"NDE!(dx, x, p, t) — wind_mixing/src/training_postprocessing.jl:131-153 (create the handle with inplace_variant = 1)"
function NDE!(h::Handle, dx, x, p, t)
    w = @view p[1:h.n_params]; bc = @view p[h.n_params+1:end]
    check(ccall((:colnde_rhs, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ptr{Float32}, Cint),
                h.ptr, x, w, bc, Float32(t), dx, 1))
    nothing
end

"[Array(solve(prob_NDEs[i], …; p=[weights; BCs[i]], saveat=t_train)) for i in 1:n_simulations] — NDE_training.jl:291,403"
function solve_NDE(h::Handle, weights::Vector{Float32})
    sol = Array{Float32}(undef, h.n_state, h.n_save, h.n_columns)
    check(ccall((:colnde_forward, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, weights, sol))
    [sol[:, :, i] for i in 1:h.n_columns]
end

const KEYS = (:u, :v, :T, :∂u∂z, :∂v∂z, :∂T∂z)

"loss_NDE / loss_gradient_NDE(weights, BCs) — NDE_training.jl:290-323: (total, scaled_losses, loss_scalings)"
function loss_gradient_NDE(h::Handle, weights, loss_scalings::NamedTuple)
    sc = Float32[loss_scalings[k] for k in KEYS]; terms = zeros(Float32, 6); total = Ref{Float32}(0)
    check(ccall((:colnde_loss, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ref{Float32}),
                h.ptr, weights, sc, terms, total))
    total[], NamedTuple{KEYS}(Tuple(terms)), loss_scalings
end

"∇loss: value and gradient in one call (replaces Zygote through InterpolatingAdjoint — NDE_training.jl:327-333)"
function ∇loss(h::Handle, weights, loss_scalings::NamedTuple)
    sc = Float32[loss_scalings[k] for k in KEYS]; terms = zeros(Float32, 6); total = Ref{Float32}(0)
    grad = similar(weights)
    check(ccall((:colnde_loss_grad, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ref{Float32}, Ptr{Float32}),
                h.ptr, weights, sc, terms, total, grad))
    total[], NamedTuple{KEYS}(Tuple(terms)), grad
end

# OptimizationFunction(loss, AutoZygote()) keeps working: the rrule routes the pullback to the HIP adjoint
function ChainRulesCore.rrule(::typeof(loss_gradient_NDE), h::Handle, weights, loss_scalings)
    total, losses, grad = ∇loss(h, weights, loss_scalings)
    pullback(ȳ) = (NoTangent(), NoTangent(), ȳ[1] .* grad, NoTangent())
    (total, losses, loss_scalings), pullback
end

# ---- free convection: FreeConvectionNDE / ConvectiveAdjustmentNDE (model = 1 / 2) -------------------------------------------

"∂T∂t(T, p, t) with p = [weights; bottom_flux, top_flux, σ_T, σ_wT, H, τ] — free_convection/src/free_convection_nde.jl:29-38,
convective_adjustment_nde.jl:33-48 (the four trailing scalars are constants of the handle's configuration)"
function ∂T∂t(h::Handle, T::Vector{Float32}, p::Vector{Float32}, t)
    dT = similar(T); w = @view p[1:h.n_params]; bc = @view p[h.n_params+1:h.n_params+2]
    check(ccall((:colnde_rhs, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ptr{Float32}, Cint),
                h.ptr, T, w, bc, Float32(t), dT, 1))
    dT
end

"solve_nde(nde, NN, T₀, alg, nde_params) for every simulation of the handle — free_convection/src/solve.jl:1-6: Nz × Nt per simulation"
solve_nde(h::Handle, NN) = solve_NDE(h, first(Flux.destructure(NN)))

"nde_loss() = Flux.mse(cat(nde_sols...), true_sols) [+ causal_penalty(NN)] — free_convection/src/training.jl:55-62"
function nde_loss(h::Handle, NN; causal_penalty=nothing)
    θ = first(Flux.destructure(NN))
    terms = zeros(Float32, 6); total = Ref{Float32}(0)
    check(ccall((:colnde_loss, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ref{Float32}),
                h.ptr, θ, Float32[0, 0, 1, 0, 0, 0], terms, total))
    causal_penalty === nothing ? total[] : total[] + causal_penalty(NN)
end

"value of nde_loss and its gradient as a `Zygote.Grads` keyed by the arrays of `Flux.params(NN)` — what `Flux.train!`
(training.jl:71) obtains from `gradient(() -> nde_loss(), ps)`.  `Flux.destructure` concatenates exactly the arrays of
`Flux.params(NN)` in order (W₁, b₁, W₂, b₂, …), so the flat HIP gradient is cut back along the same sizes."
function nde_loss_gradient(h::Handle, NN; causal_penalty=nothing)
    θ = first(Flux.destructure(NN)); ps = Flux.params(NN)
    terms = zeros(Float32, 6); total = Ref{Float32}(0); grad = similar(θ)
    check(ccall((:colnde_loss_grad, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ref{Float32}, Ptr{Float32}),
                h.ptr, θ, Float32[0, 0, 1, 0, 0, 0], terms, total, grad))
    gs = IdDict{Any,Any}(); o = 0
    for p in ps
        gs[p] = reshape(grad[o+1:o+length(p)], size(p)); o += length(p)
    end
    loss = total[]
    if causal_penalty !== nothing                      # a function of the weights alone: Zygote differentiates it as before
        pen, back = Flux.Zygote.pullback(() -> causal_penalty(NN), ps)
        gp = back(one(pen)); loss += pen
        for p in ps
            gp[p] === nothing || (gs[p] = gs[p] .+ gp[p])
        end
    end
    loss, Flux.Zygote.Grads(gs, ps)
end

"train_neural_differential_equation! — training.jl:44-74: `Flux.train!(nde_loss, Flux.params(NN), repeated((), epochs), opt, cb)`
with the gradient from the HIP adjoint; `opt`'s state is keyed by the arrays of `Flux.params(NN)` and persists across calls, as in Flux"
function train_neural_differential_equation!(h::Handle, NN, opt, epochs; cb=() -> nothing, causal_penalty=nothing)
    ps = Flux.params(NN)
    for _ in 1:epochs
        _, gs = nde_loss_gradient(h, NN; causal_penalty)
        Flux.Optimise.update!(opt, ps, gs)
        cb()
    end
    nothing
end

"compute_neural_network_forcing!(params, model) — free_convection/double_gyre_nn.jl:149-168: T_interior is `interior(model.tracers.T)`
permuted to (Nz, Nx·Ny); surface_flux (Nx·Ny) is the relaxation flux of :163; writes −∂z wT into `forcing` (Nz, Nx·Ny)"
function compute_neural_network_forcing!(forcing::Matrix{Float32}, h::Handle, weights::Vector{Float32}, T_interior::Matrix{Float32},
                                         surface_flux::Vector{Float32}, Lz)
    check(ccall((:colnde_infer_forcing, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ptr{Float32}, Cint),
                h.ptr, weights, T_interior, surface_flux, Float32(Lz), forcing, size(T_interior, 2)))
    forcing
end

"predict_flux(uvT, BCs, ...) — wind_mixing/src/NDE_training.jl:83-147 (exported at WindMixing.jl:6): (uw, vw, wT) on the Nz+1 faces for ONE state, as the
reference returns them; `p = [weights; BCs]` as for NDE"
function predict_flux(h::Handle, x::Vector{Float32}, p::Vector{Float32}, t=0)
    w = @view p[1:h.n_params]; bc = @view p[h.n_params+1:end]
    nn = h.n_nets                                                          # wind mixing: three nets on the 3 Nz state
    Nz = h.n_state ÷ nn
    fl = Matrix{Float32}(undef, Nz + 1, nn)                                 # column-major (Nz+1) x nn = C-order [nn][Nz+1]
    check(ccall((:colnde_flux, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ptr{Float32}, Cint),
                h.ptr, x, w, bc, Float32(t), fl, 1))
    nn == 3 ? (fl[:, 1], fl[:, 2], fl[:, 3]) : fl[:, 1]
end

"loss_per_tstep (wind_mixing/src/loss.jl:44-46) of the six profile terms of every simulation: n_save x 6 x n_simulations"
function loss_per_tstep(h::Handle, weights::Vector{Float32})
    out = Array{Float32}(undef, h.n_save, 6, h.n_columns)
    check(ccall((:colnde_loss_per_tstep, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, weights, out))
    out
end

"dataset-level solve_nde(ds, NN, NDEType, algorithm, T_scaling, wT_scaling) — free_convection/src/solve.jl:8-51: the solution of every simulation and the
flux wT re-evaluated at each saved step (min(0, 10 ∂T/∂z) included for ConvectiveAdjustmentNDE), both unscaled: (T = Nz x Nt x n, wT = (Nz+1) x Nt x n).
`BCs` (2 x n: scaled bottom and top flux) are the ones given to set_problem!."
function solve_nde(h::Handle, NN, BCs::Matrix{Float32}, T_scaling, wT_scaling)
    θ = first(Flux.destructure(NN))
    sols = solve_NDE(h, θ)
    h.n_nets == 1 || error("solve_nde(ds-level) is the free-convection driver: a T-only handle")
    Nz = h.n_state
    T = Array{Float32}(undef, Nz, h.n_save, h.n_columns); wT = Array{Float32}(undef, Nz + 1, h.n_save, h.n_columns)
    for i in 1:h.n_columns, n in 1:h.n_save
        T[:, n, i] .= sols[i][:, n]
        wT[:, n, i] .= predict_flux(h, sols[i][:, n], vcat(θ, BCs[:, i]), 0)
    end
    (T=inv(T_scaling).(T), wT=inv(wT_scaling).(wT))
end

"Richardson estimate of the solve's error at the current sub-step count (max |e| / (1f-3 + |u|): colnde_error_estimate) — what `reltol` bounds here"
function error_estimate(h::Handle, weights::Vector{Float32})
    est = Ref{Float32}(0)
    check(ccall((:colnde_error_estimate, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ref{Float32}), h.ptr, weights, est)); est[]
end
"the least power-of-two sub-step count meeting reltol (0: the handle's); kept by the handle — colnde_choose_substeps"
function choose_substeps!(h::Handle, weights::Vector{Float32}, reltol=0f0)
    s = Ref{Cint}(0); est = Ref{Float32}(0)
    check(ccall((:colnde_choose_substeps, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Cfloat, Ref{Cint}, Ref{Float32}), h.ptr, weights, reltol, s, est))
    Int(s[]), est[]
end
substeps(h::Handle) = ccall((:colnde_substeps, libcolnde), Cint, (Ptr{Cvoid},), h.ptr)
"impose a sub-step count (column shards: choose_substeps! on every rank, MAX over ranks, set_substeps! — colnde_set_substeps)"
set_substeps!(h::Handle, n::Integer) = (check(ccall((:colnde_set_substeps, libcolnde), Cint, (Ptr{Cvoid}, Cint), h.ptr, n)); h)

"the RK4 stability bound of every save interval's own length, n_save - 1 counts (no GPU) — colnde_schedule_min"
function schedule_min(cfg::Config, save_times::Vector{Float32})
    cfg.n_save = length(save_times)
    counts = Vector{Cint}(undef, length(save_times) - 1)
    GC.@preserve save_times begin
        cfg.save_times = pointer(save_times)
        check(ccall((:colnde_schedule_min, libcolnde), Cint, (Ref{Config}, Ptr{Cint}), cfg, counts))
    end
    Int.(counts)
end
"impose a step schedule: the RK4 steps of every save interval, the same for all columns and members (`nothing` clears it) — colnde_set_schedule"
function set_schedule!(h::Handle, counts::Union{Nothing,AbstractVector{<:Integer}})
    c = counts === nothing ? Ptr{Cint}(C_NULL) : Vector{Cint}(counts)
    check(ccall((:colnde_set_schedule, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Cint}), h.ptr, c)); h
end
"the steps of every save interval in use (n_save - 1 counts; their sum is the solve's step total) — colnde_schedule"
function schedule(h::Handle, n_save::Integer)
    counts = Vector{Cint}(undef, n_save - 1)
    total = ccall((:colnde_schedule, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Cint}), h.ptr, counts)
    total < 0 && check(Cint(1))
    Int.(counts)
end
"double the save intervals that carry the error until the estimate meets reltol (0: the handle's); kept by the handle — colnde_choose_schedule"
function choose_schedule!(h::Handle, weights::Vector{Float32}, n_save::Integer, reltol=0f0)
    counts = Vector{Cint}(undef, n_save - 1); est = Ref{Float32}(0)
    check(ccall((:colnde_choose_schedule, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Cfloat, Ptr{Cint}, Ref{Float32}), h.ptr, weights, reltol, counts, est))
    Int.(counts), est[]
end

"+∂z wT as compute_neural_network_forcing! stores it in params.∂z_wT_NN (double_gyre_nn.jl:165; the forcing function negates it, :135)"
function compute_∂z_wT!(dz_wT::Matrix{Float32}, h::Handle, weights::Vector{Float32}, T_interior::Matrix{Float32}, surface_flux::Vector{Float32}, Lz)
    check(ccall((:colnde_infer_dz_wT, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ptr{Float32}, Cint),
                h.ptr, weights, T_interior, surface_flux, Float32(Lz), dz_wT, size(T_interior, 2)))
    dz_wT
end

"switch an existing handle between MATRIX_BF16X3_EXACT and MATRIX_F32_MFMA (the tapes stay; a planned dW GEMM takes the new arithmetic's slice count) — colnde_set_matrix_arithmetic"
set_matrix_arithmetic!(h::Handle, ma) = check(ccall((:colnde_set_matrix_arithmetic, libcolnde), Cint, (Ptr{Cvoid}, Cint), h.ptr, ma))
matrix_arithmetic(h::Handle) = ccall((:colnde_matrix_arithmetic, libcolnde), Cint, (Ptr{Cvoid},), h.ptr)

"how the gradient path runs: (engine, block_columns, n_blocks, z1_taped [regtile], time_segments [fc32], dw_taped, dw_slices, split_forward,
split_adjoint, split_rich_tape, approximate_gradient = the one-switch-pattern RKC2 pullback, see COLNDE_STEPPER_RKC2 in colnde.h,
bf16x3_forward / _adjoint / _dw = which kernel families run the exact three-way bf16 split) — colnde_plan (info[3] is the Z1-tape flag on
the regtile engine, engine 2, and the number of time segments on fc32, engine 3: the same mapping as nde.py's plan())"
function plan(h::Handle)
    info = zeros(Cint, 8)
    check(ccall((:colnde_plan, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Cint}), h.ptr, info))
    engine = info[1]
    (engine=engine, block_columns=info[2], n_blocks=info[3], z1_taped=info[4] != 0 && engine == 2, time_segments=engine == 3 ? Int(info[4]) : 0,
     dw_taped=info[5] != 0, dw_slices=info[6],
     split_forward=(info[7] & 1) != 0, split_adjoint=(info[7] & 2) != 0, split_rich_tape=(info[7] & 4) != 0,
     approximate_gradient=(info[8] & 1) != 0, bf16x3_forward=(info[8] & 2) != 0, bf16x3_adjoint=(info[8] & 4) != 0, bf16x3_dw=(info[8] & 8) != 0)
end

"""The plan spelled out, plus every COLNDE_* tuning switch set in this process that the library reads — colnde_describe."""
function describe(h::Handle)
    need = ccall((:colnde_describe, libcolnde), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint), h.ptr, C_NULL, 0)
    need > 0 || error(unsafe_string(ccall((:colnde_last_error, libcolnde), Cstring, ())))
    buf = Vector{UInt8}(undef, need)
    ccall((:colnde_describe, libcolnde), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint), h.ptr, buf, need)
    return unsafe_string(pointer(buf))
end

"The reference's closures at the reference's ARITIES, closed over a handle: what `ODEProblem`, `OptimizationFunction` and `Flux.train!` are handed
today.  `NDE(x, p, t)` (NDE_training.jl:56), `NDE!(dx, x, p, t)` (training_postprocessing.jl:131; create that handle with inplace_variant = 1),
`loss_NDE(weights, BCs)` / `loss_gradient_NDE(weights, BCs)` (NDE_training.jl:290-323; BCs were given to set_problem! and are ignored here, as the
reference's closures capture everything but the weights), `∂T∂t(T, p, t)` (free_convection_nde.jl:29)."
function reference_closures(h::Handle, loss_scalings::NamedTuple=(u=1f0, v=1f0, T=1f0, ∂u∂z=5f-3, ∂v∂z=5f-3, ∂T∂z=5f-3))
    (NDE=(x, p, t) -> NDE(h, x, p, t),
     NDE! =(dx, x, p, t) -> NDE!(h, dx, x, p, t),
     ∂T∂t=(T, p, t) -> ∂T∂t(h, T, p, t),
     # loss_NDE (NDE_training.jl:290-301, the train_gradient = false objective) sets ∂u∂z = ∂v∂z = ∂T∂z = 0 before the scalings are applied
     # (and it returns the UNCHANGED loss_scalings as its third value, :300)
     loss_NDE=(weights, BCs) -> begin
         total, scaled, _ = loss_gradient_NDE(h, weights, merge(loss_scalings, (∂u∂z=0f0, ∂v∂z=0f0, ∂T∂z=0f0)))
         (total, scaled, loss_scalings)
     end,
     loss_gradient_NDE=(weights, BCs) -> loss_gradient_NDE(h, weights, loss_scalings))
end

# ---- multi-GPU: one Julia process per GPU, columns sharded, ONE exchange per optimiser iteration (include/colnde.h, colnde_comm_*) ----
mutable struct Comm
    ptr::Ptr{Cvoid}
end
"rank 0 makes the 128-byte RCCL id and hands it to every rank (MPI.Bcast!, a file, a socket) before `Comm(...)`"
function comm_unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:colnde_comm_unique_id, libcolnde), Cint, (Ptr{UInt8},), id)); id
end
function Comm(rank, nranks, unique_id::Vector{UInt8}, device=0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:colnde_comm_create, libcolnde), Cint, (Cint, Cint, Ptr{UInt8}, Cint, Ref{Ptr{Cvoid}}), rank, nranks, unique_id, device, out))
    c = Comm(out[]); finalizer(x -> ccall((:colnde_comm_destroy, libcolnde), Cvoid, (Ptr{Cvoid},), x.ptr), c)
end
"set_global_columns!(h, N): losses and gradients of this rank are normalised by the GLOBAL simulation count (NDE_training.jl:312-317)"
set_global_columns!(h::Handle, N) = check(ccall((:colnde_set_global_columns, libcolnde), Cint, (Ptr{Cvoid}, Int64), h.ptr, N))
"SUM over the ranks of the device result buffer [grad; 6 terms; total; 0] of colnde_loss_grad_dev, on the handle's stream"
allreduce_result!(h::Handle, c::Comm, d_out::Ptr{Float32}) =
    check(ccall((:colnde_allreduce_result_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}), h.ptr, c.ptr, d_out))

"convective_adjustment!(model, Δt, K) — free_convection/double_gyre_nn.jl:27-62: T is `interior(model.tracers.T)` permuted to
(Nz, Nx·Ny) column-major (= C-order [column][level]); halos are `nothing` for flux-bounded T (zero-gradient fill) or the two
halo planes Oceananigans filled"
function convective_adjustment!(h::Handle, T::Matrix{Float32}, Δt, Δz, K; halo_bottom=nothing, halo_top=nothing)
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom); ht = halo_top === nothing ? C_NULL : pointer(halo_top)
    GC.@preserve halo_bottom halo_top check(ccall((:colnde_convective_adjustment, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Cfloat, Ptr{Float32}, Cint),
        h.ptr, T, hb, ht, Δt, Δz, K, T, size(T, 2)))
    T
end

"progress_neural_network(simulation) of the free-convection embedding — free_convection/src/oceananigans_nn.jl:153-165, per column of
double_gyre_nn.jl:211-234 — for ALL columns in one call: fills ∂z_wT_NN from T as given (:159-160), then convective_adjustment!(model, Δt, K)
on T in place (:162; Δz = Lz/Nz).  T (Nz, n_columns) column-major, surface_flux one value per column, halos as convective_adjustment!;
wT_faces (Nz+1, n_columns), when given, receives diagnose_wT_NN (:100-118) of the state as given"
function progress_neural_network!(h::Handle, θ::Vector{Float32}, T::Matrix{Float32}, surface_flux::Vector{Float32}, Lz, Δt, K,
                                  ∂z_wT_NN::Matrix{Float32}; halo_bottom=nothing, halo_top=nothing, wT_faces=nothing)
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom); ht = halo_top === nothing ? C_NULL : pointer(halo_top)
    fc = wT_faces === nothing ? C_NULL : pointer(wT_faces)
    GC.@preserve halo_bottom halo_top wT_faces check(ccall((:colnde_fc_embedded_step, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Cfloat, Ptr{Float32}, Ptr{Float32},
         Ptr{Float32}, Cint),
        h.ptr, θ, T, surface_flux, hb, ht, Lz, Δt, K, ∂z_wT_NN, T, fc, size(T, 2)))
    nothing
end

"diagnose_wT_NN(model) — free_convection/src/oceananigans_nn.jl:100-118 — for all columns in one call: wT_NN .- κ .* ∂T∂z on the Nz+1 faces,
κ = K where the face gradient is negative; returns (Nz+1, n_columns)"
function diagnose_wT_NN(h::Handle, θ::Vector{Float32}, T::Matrix{Float32}, surface_flux::Vector{Float32}, Lz, K; halo_bottom=nothing, halo_top=nothing)
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom); ht = halo_top === nothing ? C_NULL : pointer(halo_top)
    wT = Matrix{Float32}(undef, size(T, 1) + 1, size(T, 2))
    GC.@preserve halo_bottom halo_top check(ccall((:colnde_fc_diagnose_wT, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Ptr{Float32}, Cint),
        h.ptr, θ, T, surface_flux, hb, ht, Lz, K, wT, size(T, 2)))
    wT
end

"modified_pacanowski_philander!(model, constants, Δt, p, convective_adjustment) — wind_mixing/src/NDE_oceananigans.jl:61-101: u, v, T are
`interior(model.velocities.u)[:]` … as (Nz, n_columns) column-major matrices (= C-order [column][level]), updated in place; `p` is the
reference's diffusivity dictionary, `constants` its NamedTuple; halo_bottom (n_columns, 3) column-major = C-order [3][n_columns] or nothing"
function modified_pacanowski_philander!(h::Handle, u::Matrix{Float32}, v::Matrix{Float32}, T::Matrix{Float32}, constants, Δt, Δz, p,
                                        convective_adjustment; halo_bottom=nothing)
    params = Float32[p["ν₀"], p["ν₋"], p["ΔRi"], p["Riᶜ"], p["Pr"], constants.α, constants.g]
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom)
    GC.@preserve halo_bottom check(ccall((:colnde_implicit_diffusion, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Ptr{Float32}, Cint,
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint),
        h.ptr, u, v, T, hb, Δt, Δz, params, convective_adjustment ? 1 : 0, u, v, T, size(T, 2)))
    nothing
end

"NN_uw_forcing, NN_vw_forcing, NN_wT_forcing (wind_mixing/src/NDE_oceananigans.jl:288-329) of every column: u, v, T as (Nz, n_columns)
matrices in the ocean model's units, top_fluxes (n_columns, 3) column-major = C-order [3][n_columns] (uw, vw, wT at the top face; a diurnal
wT_flux(t) as its value at t).  Returns the three forcings −∂z(flux) (:333, :338, :343)"
function NN_forcings(h::Handle, θ::Vector{Float32}, u::Matrix{Float32}, v::Matrix{Float32}, T::Matrix{Float32}, top_fluxes::Matrix{Float32}, Lz)
    ∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN = similar(T), similar(T), similar(T)
    check(ccall((:colnde_wm_infer_dz_flux, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint),
        h.ptr, θ, u, v, T, top_fluxes, Lz, ∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN, size(T, 2)))
    (-∂z_uw_NN, -∂z_vw_NN, -∂z_wT_NN)
end

"progress_neural_network(simulation) — wind_mixing/src/NDE_oceananigans.jl:380-405: fills ∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN from the state as
given, then modified_pacanowski_philander! on u, v, T in place (Δz = Lz/Nz); `p`, `constants`, halo_bottom as modified_pacanowski_philander!"
function progress_neural_network(h::Handle, θ::Vector{Float32}, u::Matrix{Float32}, v::Matrix{Float32}, T::Matrix{Float32},
                                 top_fluxes::Matrix{Float32}, Lz, constants, Δt, p, convective_adjustment,
                                 ∂z_uw_NN::Matrix{Float32}, ∂z_vw_NN::Matrix{Float32}, ∂z_wT_NN::Matrix{Float32}; halo_bottom=nothing)
    params = Float32[p["ν₀"], p["ν₋"], p["ΔRi"], p["Riᶜ"], p["Pr"], constants.α, constants.g]
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom)
    GC.@preserve halo_bottom check(ccall((:colnde_wm_embedded_step, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Ptr{Float32}, Cint,
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint),
        h.ptr, θ, u, v, T, top_fluxes, hb, Lz, Δt, params, convective_adjustment ? 1 : 0, ∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN, u, v, T, size(T, 2)))
    nothing
end

"diagnose_NN_flux_uw, diagnose_NN_flux_vw, diagnose_NN_flux_wT (wind_mixing/src/NDE_oceananigans.jl:226-286) of every column: the total
fluxes the embedding saves with a state, each (Nz+1, n_columns); arguments as NN_forcings and modified_pacanowski_philander!, halo_top like
halo_bottom (the cells above the column)"
function diagnose_NN_flux(h::Handle, θ::Vector{Float32}, u::Matrix{Float32}, v::Matrix{Float32}, T::Matrix{Float32}, top_fluxes::Matrix{Float32},
                          Lz, constants, p, convective_adjustment; halo_bottom=nothing, halo_top=nothing)
    params = Float32[p["ν₀"], p["ν₋"], p["ΔRi"], p["Riᶜ"], p["Pr"], constants.α, constants.g]
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom); ht = halo_top === nothing ? C_NULL : pointer(halo_top)
    uw, vw, wT = (Matrix{Float32}(undef, size(T, 1) + 1, size(T, 2)) for _ in 1:3)
    GC.@preserve halo_bottom halo_top check(ccall((:colnde_wm_diagnose_flux, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ptr{Float32}, Cint,
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint),
        h.ptr, θ, u, v, T, top_fluxes, hb, ht, Lz, params, convective_adjustment ? 1 : 0, uw, vw, wT, size(T, 2)))
    (uw, vw, wT)
end

"progress_neural_network and diagnose_NN_flux_* of the same state in one call: as progress_neural_network, and returns (uw, vw, wT) of the
state as given (before the step)"
function progress_neural_network_flux(h::Handle, θ::Vector{Float32}, u::Matrix{Float32}, v::Matrix{Float32}, T::Matrix{Float32},
                                      top_fluxes::Matrix{Float32}, Lz, constants, Δt, p, convective_adjustment,
                                      ∂z_uw_NN::Matrix{Float32}, ∂z_vw_NN::Matrix{Float32}, ∂z_wT_NN::Matrix{Float32}; halo_bottom=nothing, halo_top=nothing)
    params = Float32[p["ν₀"], p["ν₋"], p["ΔRi"], p["Riᶜ"], p["Pr"], constants.α, constants.g]
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom); ht = halo_top === nothing ? C_NULL : pointer(halo_top)
    uw, vw, wT = (Matrix{Float32}(undef, size(T, 1) + 1, size(T, 2)) for _ in 1:3)
    GC.@preserve halo_bottom halo_top check(ccall((:colnde_wm_embedded_step_flux, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Ptr{Float32}, Cint,
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint),
        h.ptr, θ, u, v, T, top_fluxes, hb, ht, Lz, Δt, params, convective_adjustment ? 1 : 0, ∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN, u, v, T, uw, vw, wT,
        size(T, 2)))
    (uw, vw, wT)
end

"progress_neural_network and diagnose_NN_flux_* for ALL K models of an ensemble handle in one launch (colnde_ensemble_wm_embedded): θ (n_params, K);
u, v, T and the ∂z arrays (Nz, n_columns, K), every model on its own state, stepped in place; top_fluxes (n_columns, 3), shared by the models;
`ps`: a vector of K parameter dictionaries, or nothing (the ensemble's own physics with the handle's α, g); halo_bottom, halo_top (n_columns, 3, K)
or nothing.  Returns (uw, vw, wT) of the states as given, each (Nz+1, n_columns, K).  Slice k is progress_neural_network_flux of model k, bit for bit.
A single (non-ensemble) handle is K = 1, and of ANY architecture: three nets of layer sizes 96-h1-...-31 with any activations at Nz = 32 (for instance the
3 x 96-400-400-31 of train_NDE.jl) are deployed by this call alone — progress_neural_network and the other single-model wrappers cover 96-50-20-31."
function ensemble_progress_neural_network_flux(h::Handle, θ::Matrix{Float32}, u::Array{Float32,3}, v::Array{Float32,3}, T::Array{Float32,3},
                                               top_fluxes::Matrix{Float32}, Lz, constants, Δt, ps, convective_adjustment,
                                               ∂z_uw_NN::Array{Float32,3}, ∂z_vw_NN::Array{Float32,3}, ∂z_wT_NN::Array{Float32,3};
                                               halo_bottom=nothing, halo_top=nothing)
    params = ps === nothing ? nothing : reduce(vcat, [Float32[p["ν₀"], p["ν₋"], p["ΔRi"], p["Riᶜ"], p["Pr"], constants.α, constants.g] for p in ps])
    pp = params === nothing ? C_NULL : pointer(params)
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom); ht = halo_top === nothing ? C_NULL : pointer(halo_top)
    uw, vw, wT = (Array{Float32,3}(undef, size(T, 1) + 1, size(T, 2), size(T, 3)) for _ in 1:3)
    GC.@preserve params halo_bottom halo_top check(ccall((:colnde_ensemble_wm_embedded, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Ptr{Float32}, Cint,
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint),
        h.ptr, θ, u, v, T, top_fluxes, hb, ht, Lz, Δt, pp, convective_adjustment ? 1 : 0, ∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN, u, v, T, uw, vw, wT,
        size(T, 2)))
    (uw, vw, wT)
end

"What NDE_profile (wind_mixing/src/training_postprocessing.jl:404-431, :310-317) evaluates on the saved states of a solve, for ALL K members of a
wind-mixing ensemble handle at once (colnde_ensemble_profile): θ (n_params, K); sol (3Nz, n_save, n_columns, K), scaled units — the states to
diagnose, nothing is solved; physics (5, K) = (ν₀, ν₋, ΔRi, Riᶜ, Pr) per member for this call only (ν₀ = ν₋ = 0: the *_NN_only fluxes), or nothing:
the handle's.  Returns (uw, vw, wT, Ri), each (Nz+1, n_save, n_columns, K) — predict_flux per state in scaled units and local_richardson without ϵ,
NaN on the two boundary faces as in the reference — and losses (n_save, 6, n_columns, K), loss_per_tstep against the truth of set_problem!."
function ensemble_NDE_profile_arrays(h::Handle, θ::Matrix{Float32}, sol::Array{Float32,4}; physics=nothing)
    pp = physics === nothing ? C_NULL : pointer(physics)
    Nz = size(sol, 1) ÷ 3
    uw, vw, wT, Ri = (Array{Float32,4}(undef, Nz + 1, size(sol, 2), size(sol, 3), size(sol, 4)) for _ in 1:4)
    losses = Array{Float32,4}(undef, size(sol, 2), 6, size(sol, 3), size(sol, 4))
    GC.@preserve physics check(ccall((:colnde_ensemble_profile, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
        h.ptr, θ, sol, pp, uw, vw, wT, Ri, losses))
    (uw, vw, wT, Ri, losses)
end

"progress_neural_network (free_convection/src/oceananigans_nn.jl:153-165) and diagnose_wT_NN (:100-118) for ALL K networks of a free-convection
ensemble handle — plain or --conv; a single handle, plain or conv, is K = 1 — in one launch (colnde_ensemble_fc_embedded): θ (n_params, K), or
nothing: the operand images the previous call on this handle packed; T and ∂z_wT_NN (Nz, n_columns, K), every member on its own state, adjusted in
place; surface_flux one value per column, shared by the members; halo_bottom, halo_top (n_columns, K) or nothing.  Returns wT_faces
(Nz+1, n_columns, K) of the states as given."
function ensemble_progress_neural_network!(h::Handle, θ::Union{Nothing,Matrix{Float32}}, T::Array{Float32,3}, surface_flux::Vector{Float32}, Lz, Δt, K,
                                           ∂z_wT_NN::Array{Float32,3}; halo_bottom=nothing, halo_top=nothing)
    w = θ === nothing ? C_NULL : pointer(θ)
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom); ht = halo_top === nothing ? C_NULL : pointer(halo_top)
    wT = Array{Float32,3}(undef, size(T, 1) + 1, size(T, 2), size(T, 3))
    GC.@preserve θ halo_bottom halo_top check(ccall((:colnde_ensemble_fc_embedded, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Cfloat, Ptr{Float32}, Ptr{Float32},
         Ptr{Float32}, Cint),
        h.ptr, w, T, surface_flux, hb, ht, Lz, Δt, K, ∂z_wT_NN, T, wT, size(T, 2)))
    wT
end

"diagnose_baseline_flux_uw, _vw, _wT (wind_mixing/src/NDE_oceananigans.jl:157-191): (−ν ∂z u, −ν ∂z v, −νT ∂z T) on the faces with the top
face replaced by the top flux, each (Nz+1, n_columns); no networks"
function diagnose_baseline_flux(h::Handle, u::Matrix{Float32}, v::Matrix{Float32}, T::Matrix{Float32}, top_fluxes::Matrix{Float32}, Δz, constants, p,
                                convective_adjustment; halo_bottom=nothing)
    params = Float32[p["ν₀"], p["ν₋"], p["ΔRi"], p["Riᶜ"], p["Pr"], constants.α, constants.g]
    hb = halo_bottom === nothing ? C_NULL : pointer(halo_bottom)
    uw, vw, wT = (Matrix{Float32}(undef, size(T, 1) + 1, size(T, 2)) for _ in 1:3)
    GC.@preserve halo_bottom check(ccall((:colnde_mpp_diagnose_flux, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ptr{Float32}, Cint,
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint),
        h.ptr, u, v, T, top_fluxes, hb, Δz, params, convective_adjustment ? 1 : 0, uw, vw, wT, size(T, 2)))
    (uw, vw, wT)
end

"Flux.Optimise.ADAM apply!/update! on device pointers (θ, ∇, m, v resident on the GPU); βᵗ = running powers kept by the caller"
function adam_step!(h::Handle, dθ::Ptr{Float32}, dg::Ptr{Float32}, dm::Ptr{Float32}, dv::Ptr{Float32}, η, β, ϵ, βᵗ, n)
    check(ccall((:colnde_adam_step_dev, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Cfloat, Cfloat, Cfloat, Cfloat, Cint),
        h.ptr, dθ, dg, dm, dv, η, β[1], β[2], ϵ, βᵗ[1], βᵗ[2], n))
    βᵗ .* β
end

"one `Flux.train!(NN_loss, Flux.params(NN), training_data, opt)` pass of train_NN (NN_training.jl:207-249) on device arrays: one ADAM
update per sample in `order`; returns (mean loss, βᵗ).  update = false evaluates `total_loss(training_data)` at fixed weights."
function pretrain_flux!(h::Handle, flux_type, dθ::Ptr{Float32}, dm::Ptr{Float32}, dv::Ptr{Float32}, dX::Ptr{Float32}, dBCs::Ptr{Float32},
                        dflux::Ptr{Float32}, dorder::Ptr{Int32}, n, gradient_scaling, η, β, ϵ, βᵗ::Vector{Float64}; update=true)
    loss = Ref{Float32}(0)
    check(ccall((:colnde_pretrain_flux_dev, libcolnde), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Cint,
         Cfloat, Cfloat, Cfloat, Cfloat, Cfloat, Ptr{Float64}, Cint, Ref{Float32}),
        h.ptr, flux_type, dθ, dm, dv, dX, dBCs, dflux, dorder, n, gradient_scaling, η, β[1], β[2], ϵ, βᵗ, update ? 1 : 0, loss))
    loss[], βᵗ
end

# ---- ensembles: K models of one architecture side by side — the sweep of wind_mixing/train_NDE_args.jl (activation ARGS[1], ADAM rate ARGS[2]
# at :143, Pacanowski-Philander constants ARGS[3] in the train_parameters Dict at :175), which trains one model per process

"K models of `cfg`'s architecture on the same columns; physics: K x 5 matrix of (ν₀, ν₋, ΔRi, Riᶜ, Pr) per model (row k = model k), or `nothing`"
function EnsembleHandle(cfg::Config, save_times::Vector{Float32}, n_models::Integer, physics=nothing)
    cfg.n_save = length(save_times)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    ph = physics === nothing ? C_NULL : Matrix{Float32}(permutedims(physics))       # C order [K][5]
    GC.@preserve save_times ph begin
        cfg.save_times = pointer(save_times)
        check(ccall((:colnde_create_ensemble, libcolnde), Cint, (Ref{Config}, Cint, Ptr{Float32}, Ref{Ptr{Cvoid}}),
                    cfg, n_models, ph === C_NULL ? Ptr{Float32}(C_NULL) : pointer(ph), out))
    end
    h = Handle(out[], ccall((:colnde_n_params, libcolnde), Cint, (Ptr{Cvoid},), out[]),
               3cfg.Nz, cfg.n_save, cfg.n_columns, 3)
    finalizer(x -> ccall((:colnde_destroy, libcolnde), Cvoid, (Ptr{Cvoid},), x.ptr), h)
end

"""K wind-mixing models of ANY architecture a tile16 handle trains (`colnde_create_tile_ensemble`): the wide nets of wind_mixing/train_NDE.jl:97-102
(96-400-400-31, 96-32-400-31, 96-400-31), other depths, activations and Nz.  `physics` as for `EnsembleHandle`.  Serves `ensemble_∇loss`, the
`ensemble_*_dev!` twins, `ensemble_adam_step!`, `set_physics!`; the member loss, step schedules, the embedding and `NDE_profile` calls refuse it."""
function TileEnsembleHandle(cfg::Config, save_times::Vector{Float32}, n_models::Integer, physics=nothing)
    cfg.n_save = length(save_times)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    ph = physics === nothing ? C_NULL : Matrix{Float32}(permutedims(physics))       # C order [K][5]
    GC.@preserve save_times ph begin
        cfg.save_times = pointer(save_times)
        check(ccall((:colnde_create_tile_ensemble, libcolnde), Cint, (Ref{Config}, Cint, Ptr{Float32}, Ref{Ptr{Cvoid}}),
                    cfg, n_models, ph === C_NULL ? Ptr{Float32}(C_NULL) : pointer(ph), out))
    end
    h = Handle(out[], ccall((:colnde_n_params, libcolnde), Cint, (Ptr{Cvoid},), out[]),
               3cfg.Nz, cfg.n_save, cfg.n_columns, 3)
    finalizer(x -> ccall((:colnde_destroy, libcolnde), Cvoid, (Ptr{Cvoid},), x.ptr), h)
end

n_models(h::Handle) = Int(ccall((:colnde_n_models, libcolnde), Cint, (Ptr{Cvoid},), h.ptr))

"new (ν₀, ν₋, ΔRi, Riᶜ, Pr) for every model: K x 5"
function set_physics!(h::Handle, physics::AbstractMatrix)
    ph = Matrix{Float32}(permutedims(physics))
    check(ccall((:colnde_ensemble_set_physics, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}), h.ptr, ph))
    h
end

"∇loss of every model: weights n_params x K (column k = model k); returns the (n_params + 8) x K result [∇θ; scaled terms(6); total; 0] per column"
function ensemble_∇loss(h::Handle, weights::AbstractMatrix{Float32}, loss_scalings::NamedTuple)
    sc = Float32[loss_scalings[k] for k in KEYS]
    out = zeros(Float32, h.n_params + 8, size(weights, 2))
    check(ccall((:colnde_ensemble_loss_grad, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                h.ptr, Matrix{Float32}(weights), sc, out))
    out
end

"device-pointer twins (handle's stream, not synchronised): solve, loss ([8] per model), loss + gradient ([n_params + 8] per model)"
ensemble_forward_dev!(h::Handle, dθ::Ptr{Float32}, dsol::Ptr{Float32}) =
    check(ccall((:colnde_ensemble_forward_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, dθ, dsol))
ensemble_loss_dev!(h::Handle, dθ::Ptr{Float32}, sc::Vector{Float32}, dout::Ptr{Float32}) =
    check(ccall((:colnde_ensemble_loss_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), h.ptr, dθ, sc, dout))
ensemble_loss_grad_dev!(h::Handle, dθ::Ptr{Float32}, sc::Vector{Float32}, dout::Ptr{Float32}) =
    check(ccall((:colnde_ensemble_loss_grad_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), h.ptr, dθ, sc, dout))

"""The error estimate of every member at every save point (colnde_ensemble_error_estimate): weights n_params x K -> n_save x K, column k what
`error_estimate` gives for member k at each save point alone.  With device weights (`Ptr{Float32}`) the `_dev` form; the result is a host array either way."""
function ensemble_error_estimate(h::Handle, weights::AbstractMatrix{Float32})
    est = zeros(Float32, h.n_save, size(weights, 2))
    check(ccall((:colnde_ensemble_error_estimate, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, Matrix{Float32}(weights), est))
    est
end
function ensemble_error_estimate(h::Handle, dθ::Ptr{Float32}, n_models::Integer)
    est = zeros(Float32, h.n_save, n_models)
    check(ccall((:colnde_ensemble_error_estimate_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, dθ, est))
    est
end
"""One step schedule for all K members of a wind-mixing ensemble (colnde_ensemble_choose_schedule): `choose_schedule!`'s greedy run on the maximum over
the members; the handle keeps it.  Returns (counts, estimates): n_save - 1 counts and every member's own estimate at them."""
function ensemble_choose_schedule!(h::Handle, weights::AbstractMatrix{Float32}, reltol=0f0)
    counts = Vector{Cint}(undef, h.n_save - 1); est = zeros(Float32, size(weights, 2))
    check(ccall((:colnde_ensemble_choose_schedule, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Cfloat, Ptr{Cint}, Ptr{Float32}),
                h.ptr, Matrix{Float32}(weights), reltol, counts, est))
    Int.(counts), est
end

"""The member loss (colnde_ensemble_set_member_loss): member k is differentiated under Σ_q s[q, k] Σ_c w[c, k] (term q of column c) / Σ_c w[c, k] —
`determine_loss_scalings` per run (wind_mixing/src/NDE_training.jl:256-288, loss.jl:11-31) and the run's own training simulations
(train_free_convection_nde.jl:60-66).  scalings 6 x K or `nothing` (every scaling 1), column_weights n_columns x K or `nothing` (every column 1);
both `nothing` clears it."""
function set_member_loss!(h::Handle, scalings::Union{Nothing,AbstractMatrix}, column_weights::Union{Nothing,AbstractMatrix})
    sc = scalings === nothing ? Ptr{Float32}(C_NULL) : Matrix{Float32}(scalings)
    cw = column_weights === nothing ? Ptr{Float32}(C_NULL) : Matrix{Float32}(column_weights)
    check(ccall((:colnde_ensemble_set_member_loss, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, sc, cw))
    h
end
"the loss of every model under the member loss that was set: device pointers, [8] per model (handle's stream, not synchronised)"
member_loss!(h::Handle, dθ::Ptr{Float32}, dout::Ptr{Float32}) =
    check(ccall((:colnde_ensemble_member_loss_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, dθ, dout))
"∇loss of every model under the member loss that was set: device pointers ([n_params + 8] per model), or host weights n_params x K -> (n_params + 8) x K"
member_loss_grad!(h::Handle, dθ::Ptr{Float32}, dout::Ptr{Float32}) =
    check(ccall((:colnde_ensemble_member_loss_grad_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, dθ, dout))
function member_loss_grad!(h::Handle, weights::AbstractMatrix{Float32})
    out = zeros(Float32, h.n_params + 8, size(weights, 2))
    check(ccall((:colnde_ensemble_member_loss_grad, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, Matrix{Float32}(weights), out))
    out
end

"ADAM for every model on device pointers: θ, m, v n_params x K, the gradient read from the loss-gradient result, η one rate per model (device)"
function ensemble_adam_step!(h::Handle, dθ::Ptr{Float32}, dresult::Ptr{Float32}, dm::Ptr{Float32}, dv::Ptr{Float32}, dη::Ptr{Float32}, β, ϵ, βᵗ)
    check(ccall((:colnde_ensemble_adam_step_dev, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Cfloat, Cfloat, Cfloat),
        h.ptr, dθ, dresult, dm, dv, dη, β[1], β[2], ϵ, βᵗ[1], βᵗ[2]))
    βᵗ .* β
end

# ---- free-convection ensembles: K networks of the fc32 shape on the same simulations — the sweep of free_convection/train_free_convection_nde.jl
# (seed, optimiser rate, --spatial_causality soft) and the judging of a run (free_convection/src/testing.jl: the network of every epoch re-solved)

"K networks Dense(Nz,4Nz,relu), Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1) (Nz = 32 | 64) of FreeConvectionNDE / ConvectiveAdjustmentNDE on the same columns;
accepted by the `ensemble_*` calls above (row k = the bits a single handle computes for model k), refused by `set_physics!` and the single-model calls"
function FreeConvectionEnsembleHandle(cfg::Config, save_times::Vector{Float32}, n_models::Integer)
    cfg.n_save = length(save_times)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve save_times begin
        cfg.save_times = pointer(save_times)
        check(ccall((:colnde_create_fc_ensemble, libcolnde), Cint, (Ref{Config}, Cint, Ref{Ptr{Cvoid}}), cfg, n_models, out))
    end
    h = Handle(out[], ccall((:colnde_n_params, libcolnde), Cint, (Ptr{Cvoid},), out[]), cfg.Nz, cfg.n_save, cfg.n_columns, 1)
    finalizer(x -> ccall((:colnde_destroy, libcolnde), Cvoid, (Ptr{Cvoid},), x.ptr), h)
end

"The free-convection driver's `--conv c` network (train_free_convection_nde.jl:110-122: Conv((c, 1), 1 => 1, relu) in front of Dense(Nz-c+1, 4Nz, relu),
Dense(4Nz, 4Nz, relu), Dense(4Nz, Nz-1)) on the fc32 kernels.  `cfg` is the PLAIN fc32 configuration (layer sizes Nz, 4Nz, 4Nz, Nz-1); the weight vector
is `vcat(vec.(Flux.params(NN))...)` of the conv chain: [w (c); b; vec(W1); b1; vec(W2); b2; vec(W3); b3], `h.n_params` entries.  Works with
set_problem!, forward!, loss, loss_grad!, loss_per_tstep and the device ADAM step; every other call refuses the handle by name."
function ConvHandle(cfg::Config, save_times::Vector{Float32}, conv::Integer)
    cfg.n_save = length(save_times)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve save_times begin
        cfg.save_times = pointer(save_times)
        check(ccall((:colnde_create_conv, libcolnde), Cint, (Ref{Config}, Cint, Ref{Ptr{Cvoid}}), cfg, conv, out))
    end
    h = Handle(out[], ccall((:colnde_n_params, libcolnde), Cint, (Ptr{Cvoid},), out[]), cfg.Nz, cfg.n_save, cfg.n_columns, 1)
    finalizer(x -> ccall((:colnde_destroy, libcolnde), Cvoid, (Ptr{Cvoid},), x.ptr), h)
end
const create_conv = ConvHandle

"K `--conv c` networks of one filter length on the same columns (`colnde_create_conv_ensemble`): `cfg` and the per-model weight layout are `ConvHandle`'s,
the K vectors are the columns of an `h.n_params x K` matrix; accepted by the `ensemble_*` calls (row k = the bits a `ConvHandle` computes for model k;
the causal penalty masks the 4Nz x (Nz-c+1) first Dense weight), refused by `set_physics!` and the single-model calls"
function ConvEnsembleHandle(cfg::Config, save_times::Vector{Float32}, conv::Integer, n_models::Integer)
    cfg.n_save = length(save_times)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve save_times begin
        cfg.save_times = pointer(save_times)
        check(ccall((:colnde_create_conv_ensemble, libcolnde), Cint, (Ref{Config}, Cint, Cint, Ref{Ptr{Cvoid}}), cfg, conv, n_models, out))
    end
    h = Handle(out[], ccall((:colnde_n_params, libcolnde), Cint, (Ptr{Cvoid},), out[]), cfg.Nz, cfg.n_save, cfg.n_columns, 1)
    finalizer(x -> ccall((:colnde_destroy, libcolnde), Cvoid, (Ptr{Cvoid},), x.ptr), h)
end

"c of a conv handle, 0 for every other handle"
conv_filter(h::Handle) = Int(ccall((:colnde_conv_filter, libcolnde), Cint, (Ptr{Cvoid},), h.ptr))

"dout[n, c, k] = mean over the levels of (sol - truth)² per save point n, simulation c and model k, scaled units: Flux.mse(true, nde, agg = x -> mean(x, dims=1))
of testing.jl:83 (plot_epoch_loss, animate_nde_loss); dsol is `ensemble_forward_dev!`'s output.  Device pointers, handle's stream."
ensemble_column_loss_dev!(h::Handle, dsol::Ptr{Float32}, dout::Ptr{Float32}) =
    check(ccall((:colnde_ensemble_column_loss_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, dsol, dout))

"the soft spatial-causality penalty of train_free_convection_nde.jl:186-197 added in place to the loss-gradient result: total += cₖ sum(abs2, W1ₖ[mask]),
gradient += 2 cₖ W1ₖ[mask]; dcoeff one coefficient per model (1: the reference's penalty, 0: row k untouched).  Device pointers, handle's stream."
ensemble_causal_penalty_dev!(h::Handle, dθ::Ptr{Float32}, dcoeff::Ptr{Float32}, dresult::Ptr{Float32}) =
    check(ccall((:colnde_ensemble_causal_penalty_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), h.ptr, dθ, dcoeff, dresult))

"one `Flux.train!(loss, ps, data, opt)` pass of the T → wT pre-training (train_free_convection_nde.jl:182-216) for all K networks of a free-convection
ensemble (plain or conv) in one launch: dθ, dm, dv K × n_params (row k = model k), dT, dbcs, dflux the n shared samples, dorder K × n (C_NULL: 1:n for
every model), dcoeff K penalty coefficients (C_NULL: none), optimiser 0 = ADAM | 1 = Descent (dm, dv may be C_NULL, βᵗ stays), dη K rates.
Returns (the K mean losses, βᵗ); update = false evaluates the loss over the data at fixed weights (`nn_callback`)."
function ensemble_pretrain_flux!(h::Handle, n_models, dθ::Ptr{Float32}, dm::Ptr{Float32}, dv::Ptr{Float32}, dT::Ptr{Float32}, dbcs::Ptr{Float32},
                                 dflux::Ptr{Float32}, dorder::Ptr{Int32}, n, dcoeff::Ptr{Float32}, optimiser, dη::Ptr{Float32}, β, ϵ,
                                 βᵗ::Vector{Float64}; update=true)
    loss = zeros(Float32, n_models)
    check(ccall((:colnde_ensemble_pretrain_flux_dev, libcolnde), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Cint, Ptr{Float32}, Cint,
         Ptr{Float32}, Cfloat, Cfloat, Cfloat, Ptr{Float64}, Cint, Ptr{Float32}),
        h.ptr, dθ, dm, dv, dT, dbcs, dflux, dorder, n, dcoeff, optimiser, dη, β[1], β[2], ϵ, βᵗ, update ? 1 : 0, loss))
    loss, βᵗ
end

"one `Flux.train!(NN_loss, Flux.params(NN), training_data, opt)` pass of `train_NN` (wind_mixing/src/NN_training.jl:207-249) for the K × 3 flux networks of a
wind-mixing ensemble in one launch, each model under its own (ν₀, ν₋, ΔRi, Riᶜ, Pr): nets a bit mask (bit j-1: net j of uw, vw, wT), dθ, dm, dv K × n_params,
dprofiles, dbcs the n shared samples, dflux the three nets' fluxes (33 × n × 3), dorder n × 3 × K (C_NULL: 1:n for every chain), dη 3 × K ADAM rates.
Returns (the 3 × K mean losses, βᵗ); update = false evaluates the loss over the data at fixed weights (`total_loss`)."
function ensemble_pretrain_wm_flux!(h::Handle, n_models, nets, dθ::Ptr{Float32}, dm::Ptr{Float32}, dv::Ptr{Float32}, dprofiles::Ptr{Float32},
                                    dbcs::Ptr{Float32}, dflux::Ptr{Float32}, dorder::Ptr{Int32}, n, gradient_scaling, dη::Ptr{Float32}, β, ϵ,
                                    βᵗ::Vector{Float64}; update=true)
    loss = zeros(Float32, 3, n_models)
    check(ccall((:colnde_ensemble_pretrain_wm_flux_dev, libcolnde), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Cint, Cfloat,
         Ptr{Float32}, Cfloat, Cfloat, Cfloat, Ptr{Float64}, Cint, Ptr{Float32}),
        h.ptr, nets, dθ, dm, dv, dprofiles, dbcs, dflux, dorder, n, gradient_scaling, dη, β[1], β[2], ϵ, βᵗ, update ? 1 : 0, loss))
    loss, βᵗ
end

# ---- the closure without networks: fitting (ν₀, ν₋, ΔRi, Riᶜ, Pr) — wind_mixing/src/diffusivity_parameter_optimisation.jl (DE :1-33,
# optimise_modified_pacanowski_philander :35-231; drivers wind_mixing/optimise_modified_pacanowski_philander.jl and ..._args.jl)

"RK4 stability bound for the constants `p = [ν₀, ν₋, ΔRi, Riᶜ, Pr]` (no GPU needed); -1: invalid configuration, ΔRi ≤ 0 or Pr ≤ 0"
function closure_min_substeps(cfg::Config, save_times::Vector{Float32}, p::Vector{Float32})
    cfg.n_save = length(save_times)
    GC.@preserve save_times begin
        cfg.save_times = pointer(save_times)
        ccall((:colnde_closure_min_substeps, libcolnde), Cint, (Ref{Config}, Ptr{Float32}), cfg, p)
    end
end

"K constant sets on the same columns (the column model WITHOUT the MLPs); cfg's layer fields and its own five constants are ignored"
function ClosureHandle(cfg::Config, save_times::Vector{Float32}, n_sets::Integer=1)
    cfg.n_save = length(save_times)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve save_times begin
        cfg.save_times = pointer(save_times)
        check(ccall((:colnde_create_closure, libcolnde), Cint, (Ref{Config}, Cint, Ref{Ptr{Cvoid}}), cfg, n_sets, out))
    end
    h = Handle(out[], 5, 3cfg.Nz, cfg.n_save, cfg.n_columns, 0)
    finalizer(x -> ccall((:colnde_destroy, libcolnde), Cvoid, (Ptr{Cvoid},), x.ptr), h)
end

"solve(prob_NDEs[i], ...; p=unscaled_parameters) for every simulation and set (:119,:152): parameters 5 x K; returns 3Nz x Nt x n_sim x K"
function closure_solve(h::Handle, parameters::AbstractMatrix{Float32})
    K = size(parameters, 2)
    sol = zeros(Float32, h.n_state, h.n_save, h.n_columns, K)
    check(ccall((:colnde_closure_forward, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, Matrix{Float32}(parameters), sol))
    sol
end

"loss_gradient_mpp and its gradient (:165-197): parameters 5 x K; returns 13 x K = [∂L/∂ν₀, ∂ν₋, ∂ΔRi, ∂Riᶜ, ∂Pr; scaled terms(6); total; 0] per column"
function closure_∇loss(h::Handle, parameters::AbstractMatrix{Float32}, loss_scalings::NamedTuple)
    sc = Float32[loss_scalings[k] for k in KEYS]
    out = zeros(Float32, 13, size(parameters, 2))
    check(ccall((:colnde_closure_loss_grad, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                h.ptr, Matrix{Float32}(parameters), sc, out))
    out
end

"device-pointer twins (handle's stream, not synchronised): dp [5 x K], dsol, dout8 [8 x K], dout [13 x K]"
closure_forward_dev!(h::Handle, dp::Ptr{Float32}, dsol::Ptr{Float32}) =
    check(ccall((:colnde_closure_forward_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), h.ptr, dp, dsol))
closure_loss_dev!(h::Handle, dp::Ptr{Float32}, sc::Vector{Float32}, dout8::Ptr{Float32}) =
    check(ccall((:colnde_closure_loss_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), h.ptr, dp, sc, dout8))
closure_loss_grad_dev!(h::Handle, dp::Ptr{Float32}, sc::Vector{Float32}, dout::Ptr{Float32}) =
    check(ccall((:colnde_closure_loss_grad_dev, libcolnde), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), h.ptr, dp, sc, dout))

"""
optimise_modified_pacanowski_philander (diffusivity_parameter_optimisation.jl:35-231) on a ClosureHandle that already holds the problem
(`set_problem!`: uvT₀s, BCs, uvT_trains — what the reference builds from train_files, tsteps and n_simulations at :39-108).  `optimizers`: Flux ADAM
objects (fields eta, beta); the scaled parameters s = p ./ p_initial start from ones (:44-48,:72-73), ∂L/∂s = p_initial .* ∂L/∂p, Flux's ADAM rule on the
host (5 K numbers), then clamp to [s_min, 10]: the reference's box is lb = 0, ub = 10 (:197); the lower edge s_min = 1f-3 is this project's, because
ΔRi = 0 and Pr = 0 are singular.  `starts`: 5 x K initial sets fitted side by side.  Returns (parameters 5 x K, losses iterations x K).
"""
function optimise_modified_pacanowski_philander(h::Handle, optimizers, maxiters; ν₀=1f-4, ν₋=1f-1, ΔRi=0.1f0, Riᶜ=0.25f0, Pr=1f0,
                                                train_gradient=true, gradient_scaling=5f-3, loss_scalings=nothing, starts=nothing, s_min=1f-3,
                                                cb=(args...) -> false)
    p₀ = starts === nothing ? reshape(Float32[ν₀, ν₋, ΔRi, Riᶜ, Pr], 5, 1) : Matrix{Float32}(starts)
    g = train_gradient ? Float32(gradient_scaling) : 0f0
    sc = loss_scalings === nothing ? (u=1f0, v=1f0, T=1f0, ∂u∂z=g, ∂v∂z=g, ∂T∂z=g) : loss_scalings
    s = ones(Float32, size(p₀))
    losses = Matrix{Float32}(undef, 0, size(p₀, 2))
    for (i, opt) in enumerate(optimizers)
        m, v, βᵗ = zero(s), zero(s), Float32[opt.beta[1], opt.beta[2]]
        for iter in 1:maxiters
            out = closure_∇loss(h, s .* p₀, sc)
            losses = vcat(losses, out[12:12, :])
            cb(s .* p₀, out[12, :], out[6:11, :], i, iter)
            ∇s = out[1:5, :] .* p₀
            m .= opt.beta[1] .* m .+ (1 - opt.beta[1]) .* ∇s
            v .= opt.beta[2] .* v .+ (1 - opt.beta[2]) .* ∇s .^ 2
            s .-= opt.eta .* m ./ (1 - βᵗ[1]) ./ (sqrt.(v ./ (1 - βᵗ[2])) .+ 1f-8)
            βᵗ .*= Float32[opt.beta[1], opt.beta[2]]
            clamp!(s, s_min, 10f0)
        end
    end
    s .* p₀, losses
end

end # module
