# MDHip.jl -- thin Julia binding of libmdhip.so (include/mdhip.h) that keeps the reference's
# names: Parameters, NVT/NVE, Potential, evaluate, LennardJones, PseudoHS, initialize_state,
# initialize_velocities, run_simulation!.  It is the drop-in for MolecularDynamics.jl's
# src/simulation.jl:40-178 path: user scripts keep their `run_simulation!(state, params, ens,
# total_steps, frequency, pathname)` call and the step loop runs on the GPU.
#
# NOT RUN in the build image (no Julia there).  It mirrors moleculardynamics/jl_amd/*.py one-to-one, which is
# what the test-suite drives through the same C ABI; tests/test_host_api.py parses every ccall / @ccall in this
# file and checks its symbol, argument count and argument types against include/mdhip.h.
module MDHip

using Random, Printf, LinearAlgebra, Statistics
using Distributions: Gamma
import CodecZstd                                    # compress=true: src/io.jl:207-223 (the reference's own dependency)

export Parameters, NVT, NVE, Brownian, Potential, evaluate, LennardJones, PseudoHS, Polydisperse,
       initialize_state, initialize_velocities, run_simulation!, LinearRamp, ExponentialRamp, fire_minimize!, minimize!,
       LennardJonesShifted, LennardJonesForceShifted, LennardJonesXPLOR, device_spec, RadialDistribution, compute_rdf,
       gofr, write_rdf, SelfDynamics, msd, alpha2, fs, van_hove, write_dynamics, write_van_hove,
       CageDynamics, bond_correlation, broken_distribution, write_cage, cage_particles,
       FourPoint, overlap, chi4, s4, s4_vectors, write_chi4, write_s4, chi4_last,
       StructureFactor, select_wave_vectors, compute_sq, sofq, fqt, fqt_normalised, write_sq, write_fqt,
       CurrentCorrelations, current_cl, current_ct, current_cl0, current_ct0, vacf, vacf0, write_currents, write_vacf,
       cur_last, mpc_setup!, mpc_marks!, mpc_sample!, mpc_reset!, mpc_last, mpc_read,
       simple_shear, pure_shear, volumetric, set_unitcell!, deform!, reduce_cell!, gauss_reduce, nonaffine_mark!, nonaffine,
       athermal_quasistatic_shear!, scale_cell!, deform_cell!, deform_state

const LIB = get(ENV, "MDHIP_LIB", joinpath(@__DIR__, "..", "moleculardynamics", "jl_amd", "csrc", "libmdhip.so"))

# ---- types: src/types.jl ---------------------------------------------------------------
abstract type Potential end
evaluate(pot::Potential, r::Real, s1::Real, s2::Real) =
    error("evaluate not implemented for potential type: $(typeof(pot))")          # src/types.jl:4-6
"""
Device description of a potential.  Either `(kind::Int, params::Vector{Float64})` for a built-in kind
(0 LennardJones, 1 PseudoHS, 2 Polydisperse, 3 modified LJ), or `(hip_source::String, entry::String, params)` for a
user potential: HIP source of `__device__ void entry(double r, double s1, double s2, const double* p, double* u,
double* f)` with f = -dU/dr -- the positional `evaluate(pot, r, sigma1, sigma2)` contract of src/pairwise.jl:31 --
compiled at run time (md_set_potential_source).  A subtype without a device form raises; nothing falls back to the CPU.
"""
device_spec(pot::Potential) = error("$(typeof(pot)) has no device form: define MDHip.device_spec")
energy_lrc(::Potential, N, V) = 0.0                                                # src/potentials.jl:281-293
pressure_lrc(::Potential, N, V) = 0.0

struct Parameters{P<:Potential,T<:AbstractFloat,N<:Integer}                        # src/types.jl:8-13
    ρ::T
    n_particles::N
    dt::T
    potential::P
end

abstract type Ensemble end
struct NVE <: Ensemble end
struct NVT{U,T<:AbstractFloat} <: Ensemble                                         # src/types.jl:36-44
    ktemp::U
    tau::T
end
NVT(ktemp::T, tau::T) where {T<:AbstractFloat} = NVT(step -> ktemp, tau)
struct Brownian{T<:AbstractFloat} <: Ensemble                                       # src/types.jl:46-49
    ktemp::T
end

# ---- potentials: src/potentials.jl ------------------------------------------------------
Base.@kwdef struct LennardJones <: Potential
    epsilon::Float64 = 1.0
    sigma::Float64 = 1.0
    r_cut::Float64 = 2.5
    tail_correction::Bool = false
end
function evaluate(p::LennardJones, r::Float64, s1::Float64, s2::Float64)          # src/potentials.jl:160-164,66-77
    σ = (s1 + s2) / 2.0
    r >= p.r_cut && return (0.0, 0.0)
    sr = σ / r; sr2 = sr * sr; sr6 = sr2 * sr2 * sr2; sr12 = sr6 * sr6
    return (4.0 * p.epsilon * (sr12 - sr6), 24.0 * p.epsilon * (2.0 * sr12 - sr6) / r)
end
device_spec(p::LennardJones) = (0, [p.epsilon, p.sigma, p.r_cut])
function energy_lrc(p::LennardJones, N, V)                                         # src/potentials.jl:111-141
    p.tail_correction || return 0.0
    ρ = N / V; x = p.sigma / p.r_cut
    return N * (8.0 * pi * ρ / 3.0) * (x^9 / 3.0 - x^3)
end
function pressure_lrc(p::LennardJones, N, V)
    p.tail_correction || return 0.0
    ρ = N / V; sr3 = (p.sigma / p.r_cut)^3
    return (16.0 * pi * ρ^2 / 3.0) * (2.0 * sr3^3 / 3.0 - sr3)
end

struct PseudoHS <: Potential
    lambda::Float64
end
PseudoHS() = PseudoHS(50.0)
const B_PARAM = 1.0204081632653061                                                  # src/potentials.jl:2-3
const A_PARAM = 134.5526623421209
function evaluate(p::PseudoHS, r::Float64, s1::Float64, s2::Float64)              # src/potentials.jl:11-29
    σ = (s1 + s2) / 2.0
    uij = 0.0; fij = 0.0
    if r < B_PARAM                                                                 # (the cutoff ignores sigma, as in the reference)
        uij = A_PARAM * ((σ / r)^p.lambda - (σ / r)^(p.lambda - 1.0)) + 1.0
        fij = A_PARAM * (p.lambda * (σ / r)^(p.lambda + 1.0) - (p.lambda - 1.0) * (σ / r)^p.lambda)
    end
    return (uij, fij)
end
device_spec(p::PseudoHS) = (1, [p.lambda])

Base.@kwdef struct Polydisperse <: Potential                                        # README.md:89-145
    rcut::Float64 = 1.25
    non_additivity::Float64 = 0.2
end
function evaluate(p::Polydisperse, r::Float64, s1::Float64, s2::Float64)          # README.md:89-145, positional (SURVEY.md D6)
    σ = 0.5 * (s1 + s2) * (1.0 - p.non_additivity * abs(s1 - s2))
    rc = p.rcut
    r < rc * σ || return (0.0, 0.0)
    c0 = -28.0 / rc^12; c2 = 48.0 / rc^14; c4 = -21.0 / rc^16
    u = (σ / r)^12 + c0 + c2 * (r / σ)^2 + c4 * (r / σ)^4
    f = 12.0 * σ^12 / r^13 - 2.0 * c2 * r / σ^2 - 4.0 * c4 * r^3 / σ^4
    return (u, f)
end
device_spec(p::Polydisperse) = (2, [p.rcut, p.non_additivity])

# shifted / force-shifted / XPLOR Lennard-Jones (src/potentials.jl:79-103,176-249; dead code in the reference):
# device kind 3 = MD_POT_LJ_MODIFIED, params {epsilon, sigma, r_cut, mode, r_on}; see include/mdhip.h
Base.@kwdef struct LennardJonesShifted <: Potential
    epsilon::Float64 = 1.0; sigma::Float64 = 1.0; r_cut::Float64 = 2.5
end
Base.@kwdef struct LennardJonesForceShifted <: Potential
    epsilon::Float64 = 1.0; sigma::Float64 = 1.0; r_cut::Float64 = 2.5
end
Base.@kwdef struct LennardJonesXPLOR <: Potential
    ϵ::Float64 = 1.0; σ::Float64 = 1.0; r_on::Float64 = 2.0; r_cut::Float64 = 2.5; tail_correction::Bool = false
end
device_spec(p::LennardJonesShifted) = (3, [p.epsilon, p.sigma, p.r_cut, 0.0, 0.0])
device_spec(p::LennardJonesForceShifted) = (3, [p.epsilon, p.sigma, p.r_cut, 1.0, 0.0])
device_spec(p::LennardJonesXPLOR) = (3, [p.ϵ, p.σ, p.r_cut, 2.0, p.r_on])

# ---- ramps: src/temperature_ramps.jl ----------------------------------------------------
struct LinearRamp; T_initial::Float64; T_final::Float64; n_steps::Int; end
function (r::LinearRamp)(step::Int)
    step > r.n_steps && return r.T_final
    step = clamp(step, 1, r.n_steps)
    r.n_steps == 1 && return r.T_final
    return r.T_initial + (r.T_final - r.T_initial) * (step - 1) / (r.n_steps - 1)
end
struct ExponentialRamp; T_initial::Float64; T_final::Float64; n_steps::Int; end
function (r::ExponentialRamp)(step::Int)
    step > r.n_steps && return r.T_final
    step = clamp(step, 1, r.n_steps)
    (r.n_steps == 1 || r.T_initial == r.T_final) && return r.T_final
    return r.T_initial * exp(log(r.T_final / r.T_initial) * (step - 1) / (r.n_steps - 1))
end

# ---- the handle -------------------------------------------------------------------------
mutable struct Device
    h::Ptr{Cvoid}
    dim::Int
    n::Int
end
function check(dev, rc)
    rc == 0 || error(unsafe_string(ccall((:md_last_error, LIB), Cstring, (Ptr{Cvoid},), dev === nothing ? C_NULL : dev.h)))
end
function Device(dim, n, unitcell::AbstractMatrix, cutoff; device_id=-1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    box = Matrix{Float64}(unitcell)                                  # column-major d x d, as the ABI wants
    rc = ccall((:md_create, LIB), Cint, (Cint, Int64, Ptr{Float64}, Float64, Cint, Ptr{Ptr{Cvoid}}),
               dim, n, box, cutoff, device_id, h)
    check(nothing, rc)
    dev = Device(h[], dim, n)
    finalizer(d -> ccall((:md_destroy, LIB), Cint, (Ptr{Cvoid},), d.h), dev)
    return dev
end

# Vector{<:AbstractVector} (the reference's Vector{MVector}: an array of pointers) <-> d x N matrix
pack(v, d) = (M = Matrix{Float64}(undef, d, length(v)); for (i, x) in enumerate(v); M[:, i] .= x; end; M)
unpack!(v, M) = (for i in eachindex(v); v[i] .= view(M, :, i); end; v)

mutable struct EnergyAndForces                                                      # src/types.jl:53-57
    energy::Float64
    virial::Float64
    forces::Vector{Vector{Float64}}
end
mutable struct ParticleSystem
    positions::Vector{Vector{Float64}}
    unitcell::Matrix{Float64}
    cutoff::Float64
    energy_and_forces::EnergyAndForces
    device::Device
end
mutable struct SimulationState                                                      # src/types.jl:15-32
    system::ParticleSystem
    diameters::Vector{Float64}
    rng::AbstractRNG
    unitcell::Matrix{Float64}
    velocities::Vector{Vector{Float64}}
    images::Matrix{Int32}
    dimension::Int
    nf::Float64
end

function initialize_velocities(ktemp, rng, n_particles, dimension)                  # src/initialization.jl:32-47
    V = randn(rng, dimension, n_particles)
    V .-= mean(V; dims=2)
    fs = sqrt(ktemp / (sum(abs2, V) / ((n_particles - 1) * dimension)))
    V .*= fs
    return [V[:, i] for i in 1:n_particles]
end

"initialize_state(params, pathname; dimension, cutoff, rng, unitcell, positions, diameters): src/initialization.jl:112-157.
Positions must be supplied (Packmol is not a dependency here)."
function initialize_state(params::Parameters, pathname::String; dimension::Int=3, cutoff=1.5,
                          rng::AbstractRNG=Random.Xoshiro(), unitcell=nothing, positions, diameters=nothing)
    n = length(positions)
    nf = dimension * (params.n_particles - 1.0)
    cell = unitcell === nothing ? Matrix{Float64}(I, dimension, dimension) .* (n / params.ρ)^(1.0 / dimension) :
           (unitcell isa Number ? Matrix{Float64}(I, dimension, dimension) .* unitcell : Matrix{Float64}(unitcell))
    diam = diameters === nothing ? ones(n) : Vector{Float64}(diameters)
    pos = [Vector{Float64}(p) for p in positions]
    forces = [zeros(dimension) for _ in 1:n]                                       # zero forces: src/initialization.jl:97-99
    dev = Device(dimension, n, cell, cutoff)
    sys = ParticleSystem(pos, cell, cutoff, EnergyAndForces(0.0, 0.0, forces), dev)
    return SimulationState(sys, diam, rng, cell, Vector{Vector{Float64}}(), zeros(Int32, dimension, n), dimension, nf)
end

function sum_noises(nf, rng)                                                        # src/thermostat.jl:1-18
    nf == 0.0 && return 0.0
    nf == 1.0 && return randn(rng)^2
    mod(nf, 2) == 0 && return 2.0 * rand(rng, Gamma(nf ÷ 2))
    return 2.0 * rand(rng, Gamma((nf - 1) ÷ 2)) + randn(rng)^2
end

# ---- device configuration: Potential -> md_set_potential / md_set_potential_source --------------------------------
function configure!(dev::Device, pot::Potential)
    spec = device_spec(pot)
    if length(spec) == 2
        kind, pp = spec
        p = Vector{Float64}(pp)
        check(dev, ccall((:md_set_potential, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Cint), dev.h, kind, p, length(p)))
    else
        src, entry, pp = spec
        p = Vector{Float64}(pp)
        check(dev, ccall((:md_set_potential_source, LIB), Cint, (Ptr{Cvoid}, Cstring, Cstring, Ptr{Float64}, Cint),
                         dev.h, String(src), String(entry), p, length(p)))
    end
    return nothing
end

function upload!(dev::Device, state::SimulationState; velocities::Bool=true)
    d = state.dimension
    X = pack(state.system.positions, d); F = pack(state.system.energy_and_forces.forces, d)
    V = velocities ? pack(state.velocities, d) : nothing
    check(dev, ccall((:md_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                     dev.h, X, velocities ? V : C_NULL, F, state.images, state.diameters))
    return nothing
end

"positions (wrapped), velocities, forces, images as d x N matrices"
function download(dev::Device)
    X = Matrix{Float64}(undef, dev.dim, dev.n); V = similar(X); F = similar(X)
    IM = Matrix{Int32}(undef, dev.dim, dev.n)
    check(dev, ccall((:md_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                     dev.h, X, V, F, IM))
    return X, V, F, IM
end

"start the asynchronous export of one frame (positions + images); collect it with `snapshot_end` after the next segment"
function snapshot_begin(dev::Device)
    check(dev, ccall((:md_snapshot_begin, LIB), Cint, (Ptr{Cvoid},), dev.h))
    return nothing
end

function snapshot_end(dev::Device)
    X = Matrix{Float64}(undef, dev.dim, dev.n)
    IM = Matrix{Int32}(undef, dev.dim, dev.n)
    check(dev, ccall((:md_snapshot_end, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}), dev.h, X, IM))
    return X, IM
end

# ---- g(r), sampled on the device (md_rdf_*; same normalisation and file format as analysis.py) ----------------------
"RadialDistribution(r_max, nbins; every=1): pair counts on nbins bins of width r_max/nbins, accumulated until reset!"
mutable struct RadialDistribution
    r_max::Float64
    nbins::Int
    every::Int
    edges::Vector{Float64}
    r::Vector{Float64}
    counts::Vector{Int64}
    nsamples::Int64
    n_particles::Int
    volume::Float64
    dimension::Int
end
function RadialDistribution(r_max, nbins; every::Int=1)
    (r_max > 0 && isfinite(r_max)) || error("r_max must be finite and > 0")
    1 <= nbins <= 8192 || error("nbins must be in 1..8192")
    every >= 1 || error("every must be >= 1")
    edges = Float64.(0:nbins) .* (r_max / nbins)
    return RadialDistribution(Float64(r_max), nbins, every, edges, (edges[1:end-1] .+ edges[2:end]) ./ 2,
                              zeros(Int64, nbins), 0, 0, 0.0, 3)
end
reset!(rdf::RadialDistribution) = (rdf.counts .= 0; rdf.nsamples = 0; rdf)

function rdf_setup!(dev::Device, rdf::RadialDistribution)
    check(dev, ccall((:md_rdf_setup, LIB), Cint, (Ptr{Cvoid}, Float64, Cint), dev.h, rdf.r_max, rdf.nbins))
end
rdf_sample!(dev::Device) = check(dev, ccall((:md_rdf_sample, LIB), Cint, (Ptr{Cvoid},), dev.h))
rdf_reset!(dev::Device) = check(dev, ccall((:md_rdf_reset, LIB), Cint, (Ptr{Cvoid},), dev.h))
function rdf_collect!(dev::Device, rdf::RadialDistribution, unitcell)
    counts = zeros(Int64, rdf.nbins); ns = Ref{Int64}(0)
    check(dev, ccall((:md_rdf_read, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), dev.h, counts, ns))
    rdf.counts .+= counts; rdf.nsamples += ns[]
    rdf.n_particles = dev.n; rdf.volume = abs(det(unitcell)); rdf.dimension = size(unitcell, 1)
    return rdf
end

"g_k = counts_k / (nsamples N (N-1) / (2V) V_k), V_k the shell volume (area in 2-D): 1 for an ideal gas"
function gofr(rdf::RadialDistribution)
    (rdf.nsamples == 0 || rdf.n_particles < 2) && return zeros(rdf.nbins)
    e = rdf.edges; N = rdf.n_particles
    Vk = rdf.dimension == 3 ? (4π / 3) .* (e[2:end] .^ 3 .- e[1:end-1] .^ 3) : π .* (e[2:end] .^ 2 .- e[1:end-1] .^ 2)
    return rdf.counts ./ (rdf.nsamples * N * (N - 1.0) / (2.0 * rdf.volume) .* Vk)
end

function write_rdf(path, rdf::RadialDistribution)
    g = gofr(rdf)
    open(path, "w") do io
        println(io, "# r g(r) count")
        for k in 1:rdf.nbins
            @printf(io, "%.6f %.6f %d\n", rdf.r[k], g[k], rdf.counts[k])
        end
    end
end

"compute_rdf(state, params, r_max, nbins): one device sample of g(r) of state's positions"
function compute_rdf(state::SimulationState, params::Parameters, r_max, nbins)
    rdf = RadialDistribution(r_max, nbins)
    dev = state.system.device
    X = pack(state.system.positions, state.dimension)
    check(dev, ccall((:md_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                     dev.h, X, C_NULL, C_NULL, state.images, C_NULL))
    rdf_setup!(dev, rdf)
    rdf_sample!(dev)
    return rdf_collect!(dev, rdf, state.unitcell)
end

# ---- self dynamics, sampled on the device (md_dyn_*; same schedule, normalisation and file formats as analysis.py) ------
"""
SelfDynamics(; q=(2π,), r_max=nothing, nbins=0, lags=nothing, origin_every=nothing): MSD, alpha2, F_s(q,t) and the van
Hove function, accumulated across run_simulation! calls until reset!.  lags=nothing is the log-time schedule of
`log_times=true` (origins at every multiple of maxlog = floor(1.35^40), samples at j*maxlog + l for the 39 distinct
l = floor(1.35^i)); explicit lags need origin_every = E (origins at m*E, samples at m*E + l, ceil(max l / E) slots
round-robin, at most 64).  Samples are taken before a new origin is stored at the same step.
"""
mutable struct SelfDynamics
    q::Vector{Float64}
    r_max::Float64
    nbins::Int
    lags::Vector{Int}
    origin_every::Int               # 0: the log-time schedule
    nslots::Int
    nsamples::Vector{Int64}
    sums::Matrix{Float64}           # (2 + nq) x nlags: sum d2, sum d4, sum s(q) per q
    hist::Matrix{Int64}             # nbins x nlags
    edges::Vector{Float64}
    r::Vector{Float64}
    n_particles::Int
    dimension::Int
    dt::Float64
end
const DYN_MAXLOG = floor(Int, 1.35^40)
_log_stops() = generate_log_times(; save=false)
function SelfDynamics(; q=(2π,), r_max=nothing, nbins::Int=0, lags=nothing, origin_every=nothing)
    qv = Float64.(collect(q))
    length(qv) <= 16 || error("at most 16 wavenumbers q")
    all(isfinite, qv) || error("every q must be finite")
    0 <= nbins <= 8192 || error("nbins must be in 0..8192")
    rm = 0.0
    if nbins > 0
        (r_max !== nothing && r_max > 0 && isfinite(r_max)) || error("r_max must be finite and > 0 when nbins > 0")
        rm = Float64(r_max)
    end
    if lags === nothing
        origin_every === nothing || error("origin_every needs explicit lags (the default is the log-time schedule)")
        lv = [s for s in _log_stops() if s <= DYN_MAXLOG]; E = 0; nslots = 1
    else
        lv = Int.(collect(lags))
        (!isempty(lv) && all(>=(1), lv)) || error("lags must be positive integers")
        allunique(lv) || error("lags must be distinct")
        (origin_every isa Integer && origin_every >= 1) || error("explicit lags need origin_every, a positive integer")
        E = Int(origin_every); nslots = cld(maximum(lv), E)
        nslots <= 64 || error("ceil(max lag / origin_every) = $nslots origin slots; at most 64")
    end
    edges = nbins > 0 ? Float64.(0:nbins) .* (rm / nbins) : [0.0]
    nl = length(lv)
    return SelfDynamics(qv, rm, nbins, lv, E, nslots, zeros(Int64, nl), zeros(2 + length(qv), nl), zeros(Int64, nbins, nl),
                        edges, (edges[1:end-1] .+ edges[2:end]) ./ 2, 0, 3, 1.0)
end
reset!(dyn::SelfDynamics) = (dyn.nsamples .= 0; dyn.sums .= 0; dyn.hist .= 0; dyn)

"stops, events: the sampler's steps in a run of T steps; events[s] = (samples [(slot, row)] 0-based, origin slot or -1)"
function dyn_schedule(dyn::SelfDynamics, T::Int)
    events = Dict{Int,Tuple{Vector{Tuple{Int,Int}},Int}}()
    if dyn.origin_every == 0
        row = Dict(l => k - 1 for (k, l) in enumerate(dyn.lags))
        for s in vcat(0, [t for t in _log_stops() if t < T])
            smp = Tuple{Int,Int}[]
            if s > 0
                j = (s - 1) ÷ DYN_MAXLOG
                haskey(row, s - j * DYN_MAXLOG) && push!(smp, (0, row[s - j * DYN_MAXLOG]))
            end
            events[s] = (smp, mod(s, DYN_MAXLOG) == 0 ? 0 : -1)
        end
    else
        E = dyn.origin_every; nsl = dyn.nslots
        for m in 0:cld(T, E)-1
            s = m * E
            events[s] = (get(events, s, (Tuple{Int,Int}[], -1))[1], mod(m, nsl))
        end
        for m in 0:cld(T, E)-1, (k, l) in enumerate(dyn.lags)      # origin order, then lag order: as analysis.py
            s = m * E + l
            s < T || continue
            ev = get!(events, s, (Tuple{Int,Int}[], -1))
            push!(ev[1], (mod(m, nsl), k - 1))
        end
    end
    return sort(collect(keys(events))), events
end

function dyn_setup!(dev::Device, dyn::SelfDynamics)
    check(dev, ccall((:md_dyn_setup, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Cint, Float64, Cint),
                     dev.h, dyn.nslots, length(dyn.lags), dyn.q, length(dyn.q), dyn.r_max, dyn.nbins))
end
dyn_origin!(dev::Device, slot::Integer) = check(dev, ccall((:md_dyn_origin, LIB), Cint, (Ptr{Cvoid}, Cint), dev.h, slot))
function dyn_sample!(dev::Device, slots::Vector{Int32}, rows::Vector{Int32})
    check(dev, ccall((:md_dyn_sample, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Cint), dev.h, slots, rows,
                     length(slots)))
end
dyn_reset!(dev::Device) = check(dev, ccall((:md_dyn_reset, LIB), Cint, (Ptr{Cvoid},), dev.h))
function dyn_act!(dev::Device, ev)
    smp, org = ev
    isempty(smp) || dyn_sample!(dev, Int32[a for (a, _) in smp], Int32[b for (_, b) in smp])
    org >= 0 && dyn_origin!(dev, org)
end
function dyn_collect!(dev::Device, dyn::SelfDynamics, dimension, dt)
    nl = length(dyn.lags)
    ns = zeros(Int64, nl); sums = zeros(2 + length(dyn.q), nl); hist = zeros(Int64, max(dyn.nbins, 1), nl)
    check(dev, ccall((:md_dyn_read, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}), dev.h, ns, sums, hist))
    dyn.nsamples .+= ns; dyn.sums .+= sums
    dyn.nbins > 0 && (dyn.hist .+= hist)
    dyn.n_particles = dev.n; dyn.dimension = dimension; dyn.dt = dt
    return dyn
end

_per(dyn::SelfDynamics, v) = [dyn.nsamples[k] > 0 ? v[k] / (dyn.n_particles * dyn.nsamples[k]) : NaN for k in eachindex(v)]
"<d^2> per lag"
msd(dyn::SelfDynamics) = _per(dyn, dyn.sums[1, :])
"d <d^4> / ((d + 2) <d^2>^2) - 1 per lag"
alpha2(dyn::SelfDynamics) = (d = dyn.dimension; d .* _per(dyn, dyn.sums[2, :]) ./ ((d + 2) .* msd(dyn) .^ 2) .- 1.0)
"F_s(q, t): nlags x nq, sum s / (d N ns)"
fs(dyn::SelfDynamics) = [dyn.nsamples[k] > 0 ? dyn.sums[2 + j, k] / (dyn.dimension * dyn.n_particles * dyn.nsamples[k]) : NaN
                         for k in eachindex(dyn.lags), j in eachindex(dyn.q)]
"G_s(r_k, t): nlags x nbins, count_k / (ns N V_k)"
function van_hove(dyn::SelfDynamics)
    e = dyn.edges
    Vk = dyn.dimension == 3 ? (4π / 3) .* (e[2:end] .^ 3 .- e[1:end-1] .^ 3) : π .* (e[2:end] .^ 2 .- e[1:end-1] .^ 2)
    return [dyn.nsamples[k] > 0 ? dyn.hist[b, k] / (dyn.nsamples[k] * dyn.n_particles * Vk[b]) : NaN
            for k in eachindex(dyn.lags), b in 1:dyn.nbins]
end

function write_dynamics(path, dyn::SelfDynamics; dt=dyn.dt)
    m = msd(dyn); a = alpha2(dyn); f = fs(dyn)
    open(path, "w") do io
        print(io, "# lag time msd alpha2")
        for q in dyn.q; print(io, " Fs(q=", @sprintf("%.6g", q), ")"); end
        println(io, " nsamples")
        for (k, l) in enumerate(dyn.lags)
            dyn.nsamples[k] > 0 || continue
            @printf(io, "%d %.6e %.6e %.6e", l, l * dt, m[k], a[k])
            for j in eachindex(dyn.q); @printf(io, " %.6e", f[k, j]); end
            @printf(io, " %d\n", dyn.nsamples[k])
        end
    end
end

function write_van_hove(path, dyn::SelfDynamics)
    g = van_hove(dyn)
    open(path, "w") do io
        println(io, "# lag r G_s count")
        first = true
        for (k, l) in enumerate(dyn.lags)
            dyn.nsamples[k] > 0 || continue
            first || println(io)
            first = false
            for b in 1:dyn.nbins
                @printf(io, "%d %.6f %.6e %d\n", l, dyn.r[b], g[k, b], dyn.hist[b, k])
            end
        end
    end
end

# ---- cage-relative dynamics and bond breaking, sampled on the device (md_cage_*; as analysis.py's CageDynamics) ---------
"""
CageDynamics(r_neigh; r_break=r_neigh, scaled=false, max_neighbours=16, q=(2π,), lags=nothing, origin_every=nothing):
the MSD, alpha2 and F_s(q,t) of the displacement relative to the mean displacement of the neighbours a particle had at
the time origin (closer than r_neigh, times sigma_ij if scaled), and the bond-breaking correlation C_B(t) (a bond is
broken when it is at least r_break long), accumulated across run_simulation! calls until reset!.  The schedule is
SelfDynamics' own.  More than max_neighbours (<= 32) neighbours at an origin is an error at the end of the run.
"""
mutable struct CageDynamics
    r_neigh::Float64
    r_break::Float64
    scaled::Bool
    max_neighbours::Int
    sched::SelfDynamics             # q, lags, origin_every, nslots: the schedule is SelfDynamics' own
    nsamples::Vector{Int64}
    sums::Matrix{Float64}           # (2 + nq) x nlags: sum d2, sum d4, sum s(q) per q, of the cage-relative displacement
    counts::Matrix{Int64}           # 3 x nlags: particles with neighbours, sum n_i, surviving bonds
    hist_broken::Matrix{Int64}      # 33 x nlags: particles by their number of broken bonds
    dimension::Int
    dt::Float64
end
function CageDynamics(r_neigh; r_break=nothing, scaled::Bool=false, max_neighbours::Int=16, q=(2π,), lags=nothing,
                      origin_every=nothing)
    (r_neigh > 0 && isfinite(r_neigh)) || error("r_neigh must be finite and > 0")
    rb = r_break === nothing ? Float64(r_neigh) : Float64(r_break)
    (isfinite(rb) && rb >= r_neigh) || error("r_break must be finite and >= r_neigh")
    1 <= max_neighbours <= 32 || error("max_neighbours must be in 1..32")
    sched = SelfDynamics(; q=q, lags=lags, origin_every=origin_every)
    nl = length(sched.lags)
    return CageDynamics(Float64(r_neigh), rb, scaled, max_neighbours, sched, zeros(Int64, nl),
                        zeros(2 + length(sched.q), nl), zeros(Int64, 3, nl), zeros(Int64, 33, nl), 3, 1.0)
end
reset!(cg::CageDynamics) = (cg.nsamples .= 0; cg.sums .= 0; cg.counts .= 0; cg.hist_broken .= 0; cg)
cage_schedule(cg::CageDynamics, T::Int) = dyn_schedule(cg.sched, T)

function cage_setup!(dev::Device, cg::CageDynamics)
    check(dev, ccall((:md_cage_setup, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Float64, Float64, Cint, Cint, Ptr{Float64}, Cint),
                     dev.h, cg.sched.nslots, length(cg.sched.lags), cg.r_neigh, cg.r_break, cg.scaled ? 1 : 0,
                     cg.max_neighbours, cg.sched.q, length(cg.sched.q)))
end
cage_origin!(dev::Device, slot::Integer) = check(dev, ccall((:md_cage_origin, LIB), Cint, (Ptr{Cvoid}, Cint), dev.h, slot))
function cage_sample!(dev::Device, slots::Vector{Int32}, rows::Vector{Int32})
    check(dev, ccall((:md_cage_sample, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Cint), dev.h, slots, rows,
                     length(slots)))
end
cage_reset!(dev::Device) = check(dev, ccall((:md_cage_reset, LIB), Cint, (Ptr{Cvoid},), dev.h))
"n_i, |Del^CR|^2 and the broken bonds of the last (slot, row) of the last cage_sample! call, in particle-id order"
function cage_particles(dev::Device)
    nnb = zeros(Int32, dev.n); d2 = zeros(dev.n); broken = zeros(Int32, dev.n)
    check(dev, ccall((:md_cage_particles, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}), dev.h, nnb, d2,
                     broken))
    return nnb, d2, broken
end
function cage_act!(dev::Device, ev)
    smp, org = ev
    isempty(smp) || cage_sample!(dev, Int32[a for (a, _) in smp], Int32[b for (_, b) in smp])
    org >= 0 && cage_origin!(dev, org)
end
function cage_collect!(dev::Device, cg::CageDynamics, dimension, dt)
    nl = length(cg.sched.lags)
    ns = zeros(Int64, nl); sums = zeros(2 + length(cg.sched.q), nl); counts = zeros(Int64, 3, nl)
    hist = zeros(Int64, 33, nl); overflow = zeros(Int64, 1)
    check(dev, ccall((:md_cage_read, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                     dev.h, ns, sums, counts, hist, overflow))
    overflow[1] == 0 || error("CageDynamics: $(overflow[1]) neighbours did not fit max_neighbours = $(cg.max_neighbours) " *
                              "entries per particle at the origins of this run: raise max_neighbours (at most 32) or " *
                              "lower r_neigh; nothing was accumulated")
    cg.nsamples .+= ns; cg.sums .+= sums; cg.counts .+= counts; cg.hist_broken .+= hist
    cg.dimension = dimension; cg.dt = dt
    return cg
end

_per(cg::CageDynamics, v) = [cg.counts[1, k] > 0 ? v[k] / cg.counts[1, k] : NaN for k in eachindex(v)]
"<|Del^CR|^2> per lag, over the particles that had neighbours"
msd(cg::CageDynamics) = _per(cg, cg.sums[1, :])
alpha2(cg::CageDynamics) = (d = cg.dimension; d .* _per(cg, cg.sums[2, :]) ./ ((d + 2) .* msd(cg) .^ 2) .- 1.0)
"cage-relative F_s(q, t): nlags x nq"
fs(cg::CageDynamics) = [cg.counts[1, k] > 0 ? cg.sums[2 + j, k] / (cg.dimension * cg.counts[1, k]) : NaN
                        for k in eachindex(cg.sched.lags), j in eachindex(cg.sched.q)]
"C_B(t) per lag: surviving bonds / origin bonds"
bond_correlation(cg::CageDynamics) = [cg.counts[2, k] > 0 ? cg.counts[3, k] / cg.counts[2, k] : NaN
                                      for k in eachindex(cg.sched.lags)]
"nlags x 33: the fraction of particles that lost b = 0..32 bonds"
broken_distribution(cg::CageDynamics) = [cg.counts[1, k] > 0 ? cg.hist_broken[b, k] / cg.counts[1, k] : NaN
                                         for k in eachindex(cg.sched.lags), b in 1:33]

function write_cage(path, cg::CageDynamics; dt=cg.dt)
    m = msd(cg); a = alpha2(cg); f = fs(cg); cb = bond_correlation(cg)
    open(path, "w") do io
        print(io, "# lag time msd_cr alpha2_cr")
        for q in cg.sched.q; print(io, " Fs_cr(q=", @sprintf("%.6g", q), ")"); end
        println(io, " C_B nsamples")
        for (k, l) in enumerate(cg.sched.lags)
            cg.nsamples[k] > 0 || continue
            @printf(io, "%d %.6e %.6e %.6e", l, l * dt, m[k], a[k])
            for j in eachindex(cg.sched.q); @printf(io, " %.6e", f[k, j]); end
            @printf(io, " %.6e %d\n", cb[k], cg.nsamples[k])
        end
    end
end


# ---- density modes, S(q) and coherent F(q,t), sampled on the device (md_sq_*; normalisation and file formats as analysis.py)
"""
select_wave_vectors(unitcell, q_max; dq=nothing, max_per_bin=16, seed=0) -> (n, q, bin): every integer vector n of the half
space (first non-zero component positive) with |q_n| <= q_max, q_n = 2pi U^-T n, thinned to at most max_per_bin per |q| bin
of width dq (default 2pi / the smallest face distance) by a permutation seeded with `seed`.  n is d x nvec (Int32), sorted
by bin, then by n.  Deterministic for given arguments (the permutation is Julia's, not numpy's).
"""
function select_wave_vectors(unitcell::AbstractMatrix, q_max::Real; dq=nothing, max_per_bin::Int=16, seed::Integer=0)
    d = size(unitcell, 1)
    (d in (2, 3) && size(unitcell, 2) == d) || error("unitcell must be a 2 x 2 or 3 x 3 matrix")
    (q_max > 0 && isfinite(q_max)) || error("q_max must be finite and > 0")
    max_per_bin >= 1 || error("max_per_bin must be >= 1")
    Ui = inv(Float64.(unitcell))
    w = dq === nothing ? 2π * maximum(norm(Ui[c, :]) for c in 1:d) : Float64(dq)
    (w > 0 && isfinite(w)) || error("dq must be finite and > 0")
    m = [floor(Int, norm(unitcell[:, c]) * q_max / 2π * (1 + 1e-12)) for c in 1:d]
    maximum(m) <= 32767 || error("q_max needs integer components beyond 32767")
    bins = Dict{Int,Vector{Tuple{Vector{Int},Float64}}}()
    r3 = d == 3 ? (-m[3]:m[3]) : (0:0)
    for n1 in 0:m[1], n2 in -m[2]:m[2], n3 in r3
        nv = d == 3 ? [n1, n2, n3] : [n1, n2]
        k = findfirst(!=(0), nv)
        (k === nothing || nv[k] < 0) && continue
        q = 2π * norm(Ui' * nv)
        q <= q_max || continue
        push!(get!(bins, floor(Int, q / w), Tuple{Vector{Int},Float64}[]), (nv, q))
    end
    isempty(bins) && error("no wave vector with |q| <= q_max: the smallest one of this cell is longer")
    rng = Random.Xoshiro(seed)
    ns = Vector{Int}[]; qs = Float64[]; bs = Int[]
    for b in sort(collect(keys(bins)))
        members = bins[b]
        keep = sort(randperm(rng, length(members))[1:min(max_per_bin, length(members))])
        for (nv, q) in sort(members[keep]; by=first)
            push!(ns, nv); push!(qs, q); push!(bs, b)
        end
    end
    length(ns) <= 16384 || error("$(length(ns)) wave vectors selected; at most 16384 (lower q_max or max_per_bin, or widen dq)")
    return Int32.(reduce(hcat, ns)), qs, bs
end

"""
StructureFactor(q_max; dq, max_per_bin=16, seed=0, every=1, lags, origin_every, dynamic=false): S(q) sampled at every
`every`-th output step of run_simulation!(...; sq) and, with dynamic=true, the coherent F(q,t) on SelfDynamics' schedule
(default: the log-time schedule; explicit lags need origin_every, at most 64 slots; samples before the new origin).
"""
mutable struct StructureFactor
    q_max::Float64
    dq::Union{Nothing,Float64}
    max_per_bin::Int
    seed::Int
    every::Int
    dynamic::Bool
    sched::Union{Nothing,SelfDynamics}   # the schedule (lags, origin_every, nslots) is SelfDynamics' own
    lags::Vector{Int}
    nslots::Int
    unitcell::Union{Nothing,Matrix{Float64}}
    n::Matrix{Int32}                     # d x nvec
    qvec::Vector{Float64}
    bin::Vector{Int}                     # per vector: index into q
    q::Vector{Float64}                   # mean |q| of a bin
    nvectors::Vector{Int}
    nstatic::Int64
    s2::Vector{Float64}
    nsamples::Vector{Int64}
    corr::Matrix{Float64}                # nvec x nlags
    n_particles::Int
    dt::Float64
end
function StructureFactor(q_max; dq=nothing, max_per_bin::Int=16, seed::Int=0, every::Int=1, lags=nothing,
                         origin_every=nothing, dynamic::Bool=false)
    (q_max > 0 && isfinite(q_max)) || error("q_max must be finite and > 0")
    (dq === nothing || (dq > 0 && isfinite(dq))) || error("dq must be finite and > 0")
    max_per_bin >= 1 || error("max_per_bin must be >= 1")
    every >= 1 || error("every must be >= 1")
    (dynamic || (lags === nothing && origin_every === nothing)) || error("lags and origin_every need dynamic=true")
    sched = dynamic ? SelfDynamics(; q=Float64[], lags=lags, origin_every=origin_every) : nothing
    lv = dynamic ? copy(sched.lags) : Int[]
    return StructureFactor(Float64(q_max), dq === nothing ? nothing : Float64(dq), max_per_bin, seed, every, dynamic, sched,
                           lv, dynamic ? sched.nslots : 0, nothing, zeros(Int32, 0, 0), Float64[], Int[], Float64[], Int[],
                           0, Float64[], zeros(Int64, length(lv)), zeros(0, length(lv)), 0, 1.0)
end
function reset!(sq::StructureFactor)
    sq.unitcell = nothing; sq.nstatic = 0; sq.nsamples .= 0
    sq.n = zeros(Int32, 0, 0); sq.s2 = Float64[]; sq.corr = zeros(0, length(sq.lags))
    return sq
end
sq_schedule(sq::StructureFactor, T::Int) = sq.dynamic ? dyn_schedule(sq.sched, T) : (Int[], nothing)

function sq_setup!(dev::Device, sq::StructureFactor, unitcell)
    U = Matrix{Float64}(unitcell)
    if sq.unitcell === nothing
        n, q, b = select_wave_vectors(U, sq.q_max; dq=sq.dq, max_per_bin=sq.max_per_bin, seed=sq.seed)
        ub = sort(unique(b))
        sq.unitcell = U; sq.n = n; sq.qvec = q; sq.bin = [searchsortedfirst(ub, x) for x in b]
        sq.nvectors = [count(==(k), sq.bin) for k in eachindex(ub)]
        sq.q = [sum(q[sq.bin .== k]) / sq.nvectors[k] for k in eachindex(ub)]
        sq.s2 = zeros(length(q)); sq.corr = zeros(length(q), length(sq.lags))
    else
        sq.unitcell == U || error("the unit cell differs from the one the wave vectors were selected for; reset! first")
    end
    check(dev, ccall((:md_sq_setup, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint, Cint, Cint),
                     dev.h, sq.n, size(sq.n, 2), sq.nslots, length(sq.lags)))
end
"rho of the current frame once; then the static sample, the correlations (slot, row), the origin store (-1: none)"
function sq_sample!(dev::Device, static::Bool, slots::Vector{Int32}, rows::Vector{Int32}, origin::Integer)
    check(dev, ccall((:md_sq_sample, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Int32}, Cint, Cint),
                     dev.h, static ? 1 : 0, slots, rows, length(slots), origin))
end
function sq_act!(dev::Device, static::Bool, ev)
    smp, org = ev === nothing ? (Tuple{Int,Int}[], -1) : ev
    sq_sample!(dev, static, Int32[a for (a, _) in smp], Int32[b for (_, b) in smp], org)
end
"rho(q) of the last sampled frame (rho = sum exp(+i q.x)); waits"
function sq_rho(dev::Device, nvec::Int)
    out = zeros(2, nvec)
    check(dev, ccall((:md_sq_rho, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), dev.h, out))
    return [complex(out[1, v], out[2, v]) for v in 1:nvec]
end
sq_reset!(dev::Device) = check(dev, ccall((:md_sq_reset, LIB), Cint, (Ptr{Cvoid},), dev.h))
function sq_collect!(dev::Device, sq::StructureFactor, dt)
    nvec = length(sq.qvec); nl = length(sq.lags)
    nst = Ref{Int64}(0); s2 = zeros(nvec); ns = zeros(Int64, max(nl, 1)); corr = zeros(nvec, max(nl, 1))
    check(dev, ccall((:md_sq_read, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
                     dev.h, nst, s2, ns, corr))
    sq.nstatic += nst[]; sq.s2 .+= s2
    if nl > 0
        sq.nsamples .+= ns[1:nl]; sq.corr .+= corr[:, 1:nl]
    end
    sq.n_particles = dev.n; sq.dt = dt
    return sq
end

_sq_binned(sq::StructureFactor, v) = [sum(v[sq.bin .== k]) / sq.nvectors[k] for k in eachindex(sq.q)]
"S(q) per |q| bin: sum over the bin's vectors of s2_v / (nstatic N M_bin)"
sofq(sq::StructureFactor) = sq.nstatic == 0 ? fill(NaN, length(sq.q)) : _sq_binned(sq, sq.s2 ./ (sq.nstatic * sq.n_particles))
"F(q,t): nlags x nbins, sum over the bin's vectors of corr_kv / (ns_k N M_bin); NaN where a lag has no sample"
function fqt(sq::StructureFactor)
    out = fill(NaN, length(sq.lags), length(sq.q))
    for k in eachindex(sq.lags)
        sq.nsamples[k] > 0 && (out[k, :] = _sq_binned(sq, sq.corr[:, k] ./ (sq.nsamples[k] * sq.n_particles)))
    end
    return out
end
"F(q,t) / S(q)"
fqt_normalised(sq::StructureFactor) = fqt(sq) ./ sofq(sq)'

function write_sq(path, sq::StructureFactor)
    s = sofq(sq)
    open(path, "w") do io
        println(io, "# q S(q) nvectors nsamples")
        for b in eachindex(sq.q)
            @printf(io, "%.6f %.6e %d %d\n", sq.q[b], s[b], sq.nvectors[b], sq.nstatic)
        end
    end
end

function write_fqt(path, sq::StructureFactor; dt=sq.dt)
    f = fqt(sq); fn = fqt_normalised(sq)
    open(path, "w") do io
        println(io, "# lag time q F F/S nsamples")
        first = true
        for (k, l) in enumerate(sq.lags)
            sq.nsamples[k] > 0 || continue
            first || println(io)
            first = false
            for b in eachindex(sq.q)
                @printf(io, "%d %.6e %.6f %.6e %.6e %d\n", l, l * dt, sq.q[b], f[k, b], fn[k, b], sq.nsamples[k])
            end
        end
    end
end

"compute_sq(state, params, q_max; dq, max_per_bin, seed): one device sample of S(q) of state's positions"
function compute_sq(state::SimulationState, params::Parameters, q_max; dq=nothing, max_per_bin::Int=16, seed::Int=0)
    sq = StructureFactor(q_max; dq=dq, max_per_bin=max_per_bin, seed=seed)
    dev = state.system.device
    X = pack(state.system.positions, state.dimension)
    check(dev, ccall((:md_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                     dev.h, X, C_NULL, C_NULL, state.images, C_NULL))
    sq_setup!(dev, sq, state.unitcell)
    sq_sample!(dev, true, Int32[], Int32[], -1)
    return sq_collect!(dev, sq, params.dt)
end

# ---- currents, C_L / C_T(q,t) and the VACF, sampled on the device (md_cur_*; normalisation and file formats as analysis.py's
# CurrentCorrelations)
"""
CurrentCorrelations(q_max; dq, max_per_bin=16, seed=0, lags, origin_every, vacf=true): the longitudinal and transverse
current correlations C_L(q,t), C_T(q,t) of j_a(q) = sum_i v_i,a exp(+i q.x_i) on select_wave_vectors' vectors (directions
e = q_n / |q_n|) and, with vacf, Z(t) = <v_i(t0+t).v_i(t0)>, on SelfDynamics' schedule (default: the log-time schedule;
explicit lags need origin_every, at most 64 slots; samples before the new origin); the equal-time sample is taken at the
stops that store an origin.  q_max=nothing samples the VACF only.  Not available with Brownian dynamics.
"""
mutable struct CurrentCorrelations
    q_max::Union{Nothing,Float64}
    dq::Union{Nothing,Float64}
    max_per_bin::Int
    seed::Int
    with_vacf::Bool
    sched::SelfDynamics                  # the schedule (lags, origin_every, nslots) is SelfDynamics' own
    lags::Vector{Int}
    nslots::Int
    unitcell::Union{Nothing,Matrix{Float64}}
    n::Matrix{Int32}                     # d x nvec
    e::Matrix{Float64}                   # d x nvec
    qvec::Vector{Float64}
    bin::Vector{Int}                     # per vector: index into q
    q::Vector{Float64}                   # mean |q| of a bin
    nvectors::Vector{Int}
    nstatic::Int64
    s_tot::Vector{Float64}
    s_long::Vector{Float64}
    nsamples::Vector{Int64}
    c_tot::Matrix{Float64}               # nvec x nlags
    c_long::Matrix{Float64}              # nvec x nlags
    z::Vector{Float64}                   # per lag
    z0::Float64
    n_particles::Int
    dimension::Int
    dt::Float64
end
function CurrentCorrelations(q_max; dq=nothing, max_per_bin::Int=16, seed::Int=0, lags=nothing, origin_every=nothing,
                             vacf::Bool=true)
    (q_max === nothing || (q_max > 0 && isfinite(q_max))) || error("q_max must be finite and > 0 (or nothing for the VACF only)")
    (q_max !== nothing || dq === nothing) || error("dq needs q_max")
    (q_max !== nothing || vacf) || error("q_max=nothing with vacf=false leaves nothing to sample")
    (dq === nothing || (dq > 0 && isfinite(dq))) || error("dq must be finite and > 0")
    max_per_bin >= 1 || error("max_per_bin must be >= 1")
    sched = SelfDynamics(; q=Float64[], lags=lags, origin_every=origin_every)
    lv = copy(sched.lags)
    return CurrentCorrelations(q_max === nothing ? nothing : Float64(q_max), dq === nothing ? nothing : Float64(dq),
                               max_per_bin, seed, vacf, sched, lv, sched.nslots, nothing, zeros(Int32, 0, 0), zeros(0, 0),
                               Float64[], Int[], Float64[], Int[], 0, Float64[], Float64[], zeros(Int64, length(lv)),
                               zeros(0, length(lv)), zeros(0, length(lv)), zeros(length(lv)), 0.0, 0, 3, 1.0)
end
function reset!(cc::CurrentCorrelations)
    cc.unitcell = nothing; cc.nstatic = 0; cc.nsamples .= 0; cc.z .= 0.0; cc.z0 = 0.0
    cc.n = zeros(Int32, 0, 0); cc.e = zeros(0, 0); cc.qvec = Float64[]; cc.s_tot = Float64[]; cc.s_long = Float64[]
    cc.c_tot = zeros(0, length(cc.lags)); cc.c_long = zeros(0, length(cc.lags))
    return cc
end
cur_schedule(cc::CurrentCorrelations, T::Int) = dyn_schedule(cc.sched, T)

function cur_setup!(dev::Device, cc::CurrentCorrelations, unitcell)
    U = Matrix{Float64}(unitcell)
    if cc.q_max !== nothing
        if cc.unitcell === nothing
            n, q, b = select_wave_vectors(U, cc.q_max; dq=cc.dq, max_per_bin=cc.max_per_bin, seed=cc.seed)
            ub = sort(unique(b))
            qc = 2π .* (inv(U)' * Float64.(n))                                     # the Cartesian q_n, d x nvec
            cc.unitcell = U; cc.n = n; cc.qvec = q; cc.bin = [searchsortedfirst(ub, x) for x in b]
            cc.e = qc ./ [norm(qc[:, v]) for v in 1:size(qc, 2)]'
            cc.nvectors = [count(==(k), cc.bin) for k in eachindex(ub)]
            cc.q = [sum(q[cc.bin .== k]) / cc.nvectors[k] for k in eachindex(ub)]
            cc.s_tot = zeros(length(q)); cc.s_long = zeros(length(q))
            cc.c_tot = zeros(length(q), length(cc.lags)); cc.c_long = zeros(length(q), length(cc.lags))
        else
            cc.unitcell == U || error("the unit cell differs from the one the wave vectors were selected for; reset! first")
        end
    end
    nvec = size(cc.n, 2)
    check(dev, ccall((:md_cur_setup, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Cint, Cint, Cint, Cint),
                     dev.h, nvec > 0 ? cc.n : C_NULL, nvec > 0 ? cc.e : C_NULL, nvec, cc.nslots, length(cc.lags),
                     cc.with_vacf ? 1 : 0))
end
"j of the current frame once; then the static sample, the correlations (slot, row), the origin store (-1: none)"
function cur_sample!(dev::Device, static::Bool, slots::Vector{Int32}, rows::Vector{Int32}, origin::Integer)
    check(dev, ccall((:md_cur_sample, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Int32}, Cint, Cint),
                     dev.h, static ? 1 : 0, slots, rows, length(slots), origin))
end
"the work at one stop: the static sample exactly where an origin is stored"
function cur_act!(dev::Device, ev)
    smp, org = ev
    cur_sample!(dev, org >= 0, Int32[a for (a, _) in smp], Int32[b for (_, b) in smp], org)
end
"j_a(q) of the last sampled frame, nvec x d (j = sum v exp(+i q.x)); waits"
function cur_last(dev::Device, nvec::Int, d::Int)
    out = zeros(2, d, max(nvec, 1))
    check(dev, ccall((:md_cur_last, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), dev.h, out))
    return [complex(out[1, a, v], out[2, a, v]) for v in 1:nvec, a in 1:d]
end
cur_reset!(dev::Device) = check(dev, ccall((:md_cur_reset, LIB), Cint, (Ptr{Cvoid},), dev.h))
function cur_collect!(dev::Device, cc::CurrentCorrelations, d, dt)
    nvec = length(cc.qvec); nl = length(cc.lags)
    nst = Ref{Int64}(0); s_tot = zeros(max(nvec, 1)); s_long = zeros(max(nvec, 1)); ns = zeros(Int64, max(nl, 1))
    c_tot = zeros(max(nvec, 1), max(nl, 1)); c_long = zeros(max(nvec, 1), max(nl, 1)); z = zeros(nl + 1)
    check(dev, ccall((:md_cur_read, LIB), Cint,
                     (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     dev.h, nst, s_tot, s_long, ns, c_tot, c_long, cc.with_vacf ? z : C_NULL))
    cc.nstatic += nst[]; cc.nsamples .+= ns[1:nl]
    if nvec > 0
        cc.s_tot .+= s_tot; cc.s_long .+= s_long; cc.c_tot .+= c_tot[:, 1:nl]; cc.c_long .+= c_long[:, 1:nl]
    end
    if cc.with_vacf
        cc.z .+= z[1:nl]; cc.z0 += z[nl + 1]
    end
    cc.n_particles = dev.n; cc.dimension = d; cc.dt = dt
    return cc
end

_cur_binned(cc::CurrentCorrelations, v) = [sum(v[cc.bin .== k]) / cc.nvectors[k] for k in eachindex(cc.q)]
function _cur_lags(cc::CurrentCorrelations, per_vector)
    out = fill(NaN, length(cc.lags), length(cc.q))
    for k in eachindex(cc.lags)
        cc.nsamples[k] > 0 && (out[k, :] = _cur_binned(cc, per_vector(k) ./ (cc.nsamples[k] * cc.n_particles)))
    end
    return out
end
"C_L(q,t): nlags x nbins, the bin mean of c_long / (ns N); NaN where a lag has no sample"
current_cl(cc::CurrentCorrelations) = _cur_lags(cc, k -> cc.c_long[:, k])
"C_T(q,t): nlags x nbins, the bin mean of (c_tot - c_long) / ((d-1) ns N)"
current_ct(cc::CurrentCorrelations) = _cur_lags(cc, k -> (cc.c_tot[:, k] .- cc.c_long[:, k]) ./ (cc.dimension - 1))
"C_L(q,0) per |q| bin from the static sums"
current_cl0(cc::CurrentCorrelations) = cc.nstatic == 0 ? fill(NaN, length(cc.q)) :
    _cur_binned(cc, cc.s_long ./ (cc.nstatic * cc.n_particles))
"C_T(q,0) per |q| bin from the static sums"
current_ct0(cc::CurrentCorrelations) = cc.nstatic == 0 ? fill(NaN, length(cc.q)) :
    _cur_binned(cc, (cc.s_tot .- cc.s_long) ./ ((cc.dimension - 1) * cc.nstatic * cc.n_particles))
"Z(t) per lag: z / (ns N); NaN where a lag has no sample"
vacf(cc::CurrentCorrelations) = [cc.nsamples[k] > 0 ? cc.z[k] / (cc.nsamples[k] * cc.n_particles) : NaN for k in eachindex(cc.lags)]
"Z(0) from the static samples"
vacf0(cc::CurrentCorrelations) = cc.nstatic > 0 ? cc.z0 / (cc.nstatic * cc.n_particles) : NaN

function write_currents(path, cc::CurrentCorrelations; dt=cc.dt)
    cl = current_cl(cc); ct = current_ct(cc); cl0 = current_cl0(cc); ct0 = current_ct0(cc)
    open(path, "w") do io
        println(io, "# lag time q C_L C_T nsamples")
        first = true
        if cc.nstatic > 0
            first = false
            for b in eachindex(cc.q)
                @printf(io, "%d %.6e %.6f %.6e %.6e %d\n", 0, 0.0, cc.q[b], cl0[b], ct0[b], cc.nstatic)
            end
        end
        for (k, l) in enumerate(cc.lags)
            cc.nsamples[k] > 0 || continue
            first || println(io)
            first = false
            for b in eachindex(cc.q)
                @printf(io, "%d %.6e %.6f %.6e %.6e %d\n", l, l * dt, cc.q[b], cl[k, b], ct[k, b], cc.nsamples[k])
            end
        end
    end
end

function write_vacf(path, cc::CurrentCorrelations; dt=cc.dt)
    z = vacf(cc); z0 = vacf0(cc)
    open(path, "w") do io
        println(io, "# lag time Z Z/Z(0) nsamples")
        cc.nstatic > 0 && @printf(io, "%d %.6e %.6e %.6e %d\n", 0, 0.0, z0, 1.0, cc.nstatic)
        for (k, l) in enumerate(cc.lags)
            cc.nsamples[k] > 0 && @printf(io, "%d %.6e %.6e %.6e %d\n", l, l * dt, z[k], z[k] / z0, cc.nsamples[k])
        end
    end
end

# ---- four-point dynamics, sampled on the device (md_chi4_*; normalisation and file formats as analysis.py's FourPoint) --
"""
FourPoint(a; q_max=nothing, dq=nothing, max_per_bin=16, seed=0, lags=nothing, origin_every=nothing): the self overlap
Q(t0, t) = sum_i w_i, w_i = 1 iff particle i moved less than a (strict), its variance chi4(t) = (<Q^2> - <Q>^2) / N and
S4(q, t) = <|W(q)|^2> / N, W(q) = sum_i w_i exp(+i q.x_i(t0)), on select_wave_vectors' vectors of the cell first used on
(at most 4096; q_max=nothing: chi4 only), accumulated across run_simulation! calls until reset!.  The schedule is
SelfDynamics' own (log-time by default; samples before the new origin at a shared step).  chi4 as measured is the
fixed-N variance in the ensemble of the run: NVE, NVT and Brownian runs each miss the contributions of the quantities they
hold fixed; S4(q -> 0, t) of the same run is the estimate without that loss.  The overlap is the self overlap; a
cage-relative variant for 2-D is not provided.
"""
mutable struct FourPoint
    a::Float64
    q_max::Union{Nothing,Float64}
    dq::Union{Nothing,Float64}
    max_per_bin::Int
    seed::Int
    sched::SelfDynamics                  # lags, origin_every, nslots: the schedule is SelfDynamics' own
    nsamples::Vector{Int64}
    sum_q::Vector{BigInt}                # per lag: sum Q and sum Q^2, exact
    sum_q2::Vector{BigInt}
    unitcell::Union{Nothing,Matrix{Float64}}
    n::Matrix{Int32}                     # d x nvec
    qvec::Vector{Float64}
    bin::Vector{Int}                     # per vector: index into q
    q::Vector{Float64}                   # mean |q| of a bin
    nvectors::Vector{Int}
    sum_s4::Matrix{Float64}              # nvec x nlags: sum |W|^2
    n_particles::Int
    dt::Float64
end
function FourPoint(a; q_max=nothing, dq=nothing, max_per_bin::Int=16, seed::Int=0, lags=nothing, origin_every=nothing)
    (a > 0 && isfinite(a)) || error("a must be finite and > 0")
    (q_max === nothing || (q_max > 0 && isfinite(q_max))) || error("q_max must be finite and > 0 (or nothing for chi4 only)")
    (dq === nothing || q_max !== nothing) || error("dq needs q_max")
    (dq === nothing || (dq > 0 && isfinite(dq))) || error("dq must be finite and > 0")
    max_per_bin >= 1 || error("max_per_bin must be >= 1")
    sched = SelfDynamics(; q=Float64[], lags=lags, origin_every=origin_every)
    nl = length(sched.lags)
    return FourPoint(Float64(a), q_max === nothing ? nothing : Float64(q_max), dq === nothing ? nothing : Float64(dq),
                     max_per_bin, seed, sched, zeros(Int64, nl), zeros(BigInt, nl), zeros(BigInt, nl), nothing,
                     zeros(Int32, 0, 0), Float64[], Int[], Float64[], Int[], zeros(0, nl), 0, 1.0)
end
function reset!(fp::FourPoint)
    fp.nsamples .= 0; fp.sum_q .= 0; fp.sum_q2 .= 0
    fp.unitcell = nothing; fp.n = zeros(Int32, 0, 0); fp.qvec = Float64[]; fp.sum_s4 = zeros(0, length(fp.sched.lags))
    return fp
end
chi4_schedule(fp::FourPoint, T::Int) = dyn_schedule(fp.sched, T)

function chi4_setup!(dev::Device, fp::FourPoint, unitcell)
    if fp.q_max !== nothing
        U = Matrix{Float64}(unitcell)
        if fp.unitcell === nothing
            n, q, b = select_wave_vectors(U, fp.q_max; dq=fp.dq, max_per_bin=fp.max_per_bin, seed=fp.seed)
            size(n, 2) <= 4096 || error("$(size(n, 2)) wave vectors selected; FourPoint takes at most 4096")
            ub = sort(unique(b))
            fp.unitcell = U; fp.n = n; fp.qvec = q; fp.bin = [searchsortedfirst(ub, x) for x in b]
            fp.nvectors = [count(==(k), fp.bin) for k in eachindex(ub)]
            fp.q = [sum(q[fp.bin .== k]) / fp.nvectors[k] for k in eachindex(ub)]
            fp.sum_s4 = zeros(length(q), length(fp.sched.lags))
        else
            fp.unitcell == U || error("the unit cell differs from the one the wave vectors were selected for; reset! first")
        end
    end
    nvec = length(fp.qvec)
    check(dev, ccall((:md_chi4_setup, LIB), Cint, (Ptr{Cvoid}, Float64, Ptr{Int32}, Cint, Cint, Cint),
                     dev.h, fp.a, fp.n, nvec, fp.sched.nslots, length(fp.sched.lags)))
end
chi4_origin!(dev::Device, slot::Integer) = check(dev, ccall((:md_chi4_origin, LIB), Cint, (Ptr{Cvoid}, Cint), dev.h, slot))
function chi4_sample!(dev::Device, slots::Vector{Int32}, rows::Vector{Int32})
    check(dev, ccall((:md_chi4_sample, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Cint), dev.h, slots, rows,
                     length(slots)))
end
chi4_reset!(dev::Device) = check(dev, ccall((:md_chi4_reset, LIB), Cint, (Ptr{Cvoid},), dev.h))
"Q, W (complex, per vector) and the slow mask (one byte per particle id) of the last (slot, row) of the last chi4_sample! call"
function chi4_last(dev::Device, nvec::Int)
    q = Ref{Int64}(0); w = zeros(2, max(nvec, 1)); slow = zeros(UInt8, dev.n)
    check(dev, ccall((:md_chi4_last, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Cvoid}), dev.h, q, w, slow))
    return q[], [complex(w[1, v], w[2, v]) for v in 1:nvec], slow
end
function chi4_act!(dev::Device, ev)
    smp, org = ev
    isempty(smp) || chi4_sample!(dev, Int32[a for (a, _) in smp], Int32[b for (_, b) in smp])
    org >= 0 && chi4_origin!(dev, org)
end
function chi4_collect!(dev::Device, fp::FourPoint, dt)
    nl = length(fp.sched.lags); nvec = length(fp.qvec)
    ns = zeros(Int64, nl); sq = zeros(Int64, nl); sq2 = zeros(Int64, nl); s4 = zeros(max(nvec, 1), nl)
    check(dev, ccall((:md_chi4_read, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                     dev.h, ns, sq, sq2, s4))
    fp.nsamples .+= ns; fp.sum_q .+= sq; fp.sum_q2 .+= sq2
    nvec > 0 && (fp.sum_s4 .+= s4)
    fp.n_particles = dev.n; fp.dt = dt
    return fp
end

"<Q> / N per lag; NaN where a lag has no sample"
overlap(fp::FourPoint) = [fp.nsamples[k] > 0 ? Float64(fp.sum_q[k] // (BigInt(fp.nsamples[k]) * fp.n_particles)) : NaN
                          for k in eachindex(fp.nsamples)]
"chi4 per lag: (ns sum Q^2 - (sum Q)^2) / (ns^2 N), the numerator formed in integers"
chi4(fp::FourPoint) = [fp.nsamples[k] > 0 ?
                       Float64((fp.nsamples[k] * fp.sum_q2[k] - fp.sum_q[k]^2) // (BigInt(fp.nsamples[k])^2 * fp.n_particles)) :
                       NaN for k in eachindex(fp.nsamples)]
"S4(q_v, t): nlags x nvec, sum |W|^2 / (ns N); NaN where a lag has no sample"
s4_vectors(fp::FourPoint) = [fp.nsamples[k] > 0 ? fp.sum_s4[v, k] / (fp.nsamples[k] * fp.n_particles) : NaN
                             for k in eachindex(fp.nsamples), v in eachindex(fp.qvec)]
"S4(q, t): nlags x nbins, the mean of s4_vectors over the vectors of a |q| bin"
function s4(fp::FourPoint)
    sv = s4_vectors(fp)
    return [sum(sv[k, fp.bin .== b]) / fp.nvectors[b] for k in eachindex(fp.nsamples), b in eachindex(fp.q)]
end

function write_chi4(path, fp::FourPoint; dt=fp.dt)
    ov = overlap(fp); c4 = chi4(fp)
    open(path, "w") do io
        println(io, "# lag time Q/N chi4 nsamples")
        for (k, l) in enumerate(fp.sched.lags)
            fp.nsamples[k] > 0 || continue
            @printf(io, "%d %.6e %.6e %.6e %d\n", l, l * dt, ov[k], c4[k], fp.nsamples[k])
        end
    end
end

function write_s4(path, fp::FourPoint; dt=fp.dt)
    s = s4(fp)
    open(path, "w") do io
        println(io, "# lag time q S4 nvectors nsamples")
        first = true
        for (k, l) in enumerate(fp.sched.lags)
            fp.nsamples[k] > 0 || continue
            first || println(io)
            first = false
            for b in eachindex(fp.q)
                @printf(io, "%d %.6e %.6f %.6e %d %d\n", l, l * dt, fp.q[b], s[k, b], fp.nvectors[b], fp.nsamples[k])
            end
        end
    end
end

# ---- marked pair correlations, sampled on the device (md_mpc_*; device.py's mpc_* calls) -----------------------------
const MD_MPC_BOO, MD_MPC_USER = 0, 1
"the bond-order sampler's last frame as marks (G_l(r), g6(r)): nc, weights and tmax come from its setup"
function mpc_setup!(dev::Device, r_max, nbins::Integer)
    check(dev, ccall((:md_mpc_setup, LIB), Cint, (Ptr{Cvoid}, Cint, Float64, Cint, Cint, Ptr{Float64}, Float64),
                     dev.h, MD_MPC_BOO, r_max, nbins, 0, C_NULL, 0.0))
end
"user marks: length(weights) = NC in 1..3 components per particle, tmax >= |t| of every term (rounded up to a power of two)"
function mpc_setup!(dev::Device, r_max, nbins::Integer, weights::Vector{Float64}, tmax)
    check(dev, ccall((:md_mpc_setup, LIB), Cint, (Ptr{Cvoid}, Cint, Float64, Cint, Cint, Ptr{Float64}, Float64),
                     dev.h, MD_MPC_USER, r_max, nbins, length(weights), weights, tmax))
end
"marks: NC x N (component c of particle i at [c, i]), in particle order; kept until replaced"
mpc_marks!(dev::Device, marks::Matrix{Float64}) =
    check(dev, ccall((:md_mpc_marks, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), dev.h, marks))
mpc_sample!(dev::Device) = check(dev, ccall((:md_mpc_sample, LIB), Cint, (Ptr{Cvoid},), dev.h))
mpc_reset!(dev::Device) = check(dev, ccall((:md_mpc_reset, LIB), Cint, (Ptr{Cvoid},), dev.h))
"(cnt, sum, self) of the last sample: the integers of the exactness contract; waits"
function mpc_last(dev::Device, nbins::Integer)
    cnt = zeros(Int64, nbins); sum = zeros(Int64, nbins); self = Ref{Int64}(0)
    check(dev, ccall((:md_mpc_last, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), dev.h, cnt, sum, self))
    return cnt, sum, self[]
end
"(nsamples, acc_cnt, acc_sum, acc_self, tmax, range_error) since setup / reset; sum * tmax * 2^-31 / cnt is the correlation"
function mpc_read(dev::Device, nbins::Integer)
    ns = Ref{Int64}(0); cnt = zeros(Int64, nbins); sum = zeros(nbins); self = Ref{Float64}(0.0)
    tmax = Ref{Float64}(0.0); err = Ref{Int32}(0)
    check(dev, ccall((:md_mpc_read, LIB), Cint,
                     (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                     dev.h, ns, cnt, sum, self, tmax, err))
    return ns[], cnt, sum, self[], tmax[], err[]
end

# ---- swap Monte Carlo on the device (md_swap_*; device.py's swap_* calls) ---------------------------------------------
"fraction in (0, 1]; max_diameter_difference <= 0: no filter; seed keys the Philox stream"
swap_setup!(dev::Device, fraction, max_diameter_difference, seed::Integer) =
    check(dev, ccall((:md_swap_setup, LIB), Cint, (Ptr{Cvoid}, Float64, Float64, UInt64),
                     dev.h, fraction, max_diameter_difference, seed))
"rounds first_round .. first_round + nrounds - 1, then a force refresh: (counts[6], decided, du_accepted, U, W); waits"
function swap_rounds!(dev::Device, nrounds::Integer, ktemp, first_round::Integer = 0)
    counts = zeros(Int64, 6); dec = Ref{Int64}(0)
    du = Ref{Float64}(0.0); u = Ref{Float64}(0.0); w = Ref{Float64}(0.0)
    check(dev, ccall((:md_swap_rounds, LIB), Cint,
                     (Ptr{Cvoid}, Int64, Float64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     dev.h, nrounds, ktemp, first_round, counts, dec, du, u, w))
    return counts, dec[], du[], u[], w[]
end
"(partner, status, du) of the last round, by particle (0-based partner, -1: did not propose); waits"
function swap_last(dev::Device, n::Integer)
    partner = zeros(Int32, n); status = zeros(Int32, n); du = zeros(n)
    check(dev, ccall((:md_swap_last, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
                     dev.h, partner, status, du))
    return partner, status, du
end
"the current diameters, in particle order; waits"
function diameters(dev::Device, n::Integer)
    d = zeros(n)
    check(dev, ccall((:md_diameters, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), dev.h, d))
    return d
end

# ---- output: src/io.jl ---------------------------------------------------------------------------------------------
function generate_log_times(; max_iter::Int=10000, logn::Int=40, logbase::Float64=1.35, save::Bool=true)   # src/io.jl:17-36
    dtime = Int[]
    maxlog = floor(Int, logbase^logn)
    for j in 0:max_iter, i in 0:logn
        push!(dtime, floor(Int, j * maxlog + logbase^i))
    end
    logs = sort(unique(dtime))
    save || return logs
    open("new-log-times.txt", "w") do file                                          # src/io.jl:1-15 (in the CWD, as the reference)
        write(file, "#maxsnap=$logn,base=$logbase\n")
        for l in logs; write(file, "$l\n"); end
    end
    return logs
end

"extended XYZ, src/io.jl:42-70 (X: d x N matrix; \"%lf\" prints 6 decimals)"
function write_to_file(filepath, step, unitcell, n_particles, X::AbstractMatrix, diameters, dimension; mode="a")
    open(filepath, mode) do io
        println(io, n_particles)
        flat = join([string(unitcell[i, j]) for i in 1:dimension, j in 1:dimension], " ")
        @printf(io, "Lattice=\"%s\" Properties=type:I:1:id:I:1:radius:R:1:pos:R:%d Time=%.6g\n", flat, dimension, step)
        for i in 1:n_particles
            @printf(io, "%d %d %f", 1, i, diameters[i] / 2.0)
            for d in 1:dimension; @printf(io, " %f", X[d, i]); end
            @printf(io, "\n")
        end
    end
    return nothing
end

"LAMMPS dump with wrapped and unwrapped coordinates, src/io.jl:96-170 (id = i, type = 1, radius = sigma/2)"
function write_to_file_lammps(filepath, step, unitcell, n_particles, X::AbstractMatrix, IM::AbstractMatrix, diameters,
                              dimension; mode="w")
    open(filepath, mode) do io
        @printf(io, "ITEM: TIMESTEP\n%d\n", step)
        @printf(io, "ITEM: NUMBER OF ATOMS\n%d\n", n_particles)
        boxmat = zeros(3, 3); boxmat[1:dimension, 1:dimension] .= unitcell
        if dimension == 2
            @printf(io, "ITEM: BOX BOUNDS xy pp pp\n")
            @printf(io, "%f %f %f\n", 0.0, norm(boxmat[:, 1]), boxmat[1, 2])
            @printf(io, "%f %f 0.0\n", 0.0, norm(boxmat[:, 2]))
            @printf(io, "%f %f 0.0\n", 0.0, 1.0)
            @printf(io, "ITEM: ATOMS id type radius x y xu yu\n")
        elseif dimension == 3
            @printf(io, "ITEM: BOX BOUNDS xy xz yz pp pp pp\n")
            @printf(io, "%f %f %f\n", 0.0, norm(boxmat[:, 1]), boxmat[1, 2])
            @printf(io, "%f %f %f\n", 0.0, norm(boxmat[:, 2]), boxmat[2, 3])
            @printf(io, "%f %f %f\n", 0.0, norm(boxmat[:, 3]), boxmat[1, 3])
            @printf(io, "ITEM: ATOMS id type radius x y z xu yu zu\n")
        else
            error("Unsupported dimension: $dimension")
        end
        for i in 1:n_particles
            uw = X[:, i] .+ unitcell * IM[:, i]                                       # unwrapped: src/io.jl:77-85
            if dimension == 2
                @printf(io, "%d %d %f %f %f %f %f\n", i, 1, diameters[i] / 2.0, X[1, i], X[2, i], uw[1], uw[2])
            else
                @printf(io, "%d %d %f %f %f %f %f %f %f\n", i, 1, diameters[i] / 2.0, X[1, i], X[2, i], X[3, i],
                        uw[1], uw[2], uw[3])
            end
        end
    end
    return nothing
end

function compress_zstd(filepath)                                                     # src/io.jl:207-223
    open(filepath, "r") do infile
        open(CodecZstd.ZstdCompressorStream, filepath * ".zst", "w") do outfile
            write(outfile, read(infile))
        end
    end
    rm(filepath)
    return nothing
end

function open_files(pathname, traj_name, thermo_name)                                # src/io.jl:225-239
    files = (joinpath(pathname, traj_name), joinpath(pathname, thermo_name))
    for f in files; isfile(f) && rm(f); end
    return files
end

"""
run_simulation!(state, params, ensemble, total_steps, frequency, pathname; traj_name, thermo_name, compress, log_times, rdf)
-- src/simulation.jl:40-178 (NVE / NVT) and :181-308 (Brownian).  Mutates `state`, returns nothing.  The step loop
runs device-resident inside libmdhip; this driver cuts the run into segments that end on the reference's output
steps (step % frequency == 0, 0-based), draws the thermostat's random numbers on the host in the reference's
order, and writes the thermo line, the LAMMPS frames, the log-spaced snapshots and final.xyz.  With rdf a
RadialDistribution, g(r) is sampled on the device at every rdf.every-th output step and written to pathname/rdf.txt.
With sq a StructureFactor, S(q) is sampled the same way (pathname/sq.txt) and, if it is dynamic, the coherent F(q,t) on its
schedule (pathname/fqt.txt).  With cage a CageDynamics, the cage-relative MSD, alpha2, F_s(q,t) and the bond-breaking
correlation are sampled on SelfDynamics' schedule (pathname/cage.txt).  With four_point a FourPoint, the self overlap,
chi4(t) and -- if it has wave vectors -- S4(q,t) are sampled on SelfDynamics' schedule (pathname/chi4.txt, pathname/s4.txt).
With currents a CurrentCorrelations, C_L(q,t), C_T(q,t) and -- with vacf -- Z(t) are sampled on SelfDynamics' schedule
(pathname/currents.txt, pathname/vacf.txt); not with Brownian dynamics.
"""
function run_simulation!(state::SimulationState, params::Parameters, ensemble::Ensemble, total_steps::Int,
                         frequency::Int, pathname::String; traj_name::String="trajectory.xyz",
                         thermo_name::String="thermo.txt", compress::Bool=false, log_times::Bool=false,
                         rdf::Union{Nothing,RadialDistribution}=nothing,
                         dynamics::Union{Nothing,SelfDynamics}=nothing,
                         sq::Union{Nothing,StructureFactor}=nothing,
                         currents::Union{Nothing,CurrentCorrelations}=nothing,
                         cage::Union{Nothing,CageDynamics}=nothing,
                         four_point::Union{Nothing,FourPoint}=nothing)
    dev = state.system.device; d = state.dimension; n = params.n_particles
    brownian = ensemble isa Brownian
    (currents === nothing || !brownian) || error("currents is not available with Brownian dynamics (no velocities)")
    configure!(dev, params.potential)
    upload!(dev, state; velocities=!brownian)
    rdf === nothing || rdf_setup!(dev, rdf)
    # the dynamics schedule restarts at step 0 in every call; its stops are added to the output steps
    dyn_stops, dyn_events = dynamics === nothing ? (Int[], nothing) : dyn_schedule(dynamics, total_steps)
    dynamics === nothing || dyn_setup!(dev, dynamics)
    dyn_i = 1
    # the structure factor: static samples at every sq.every-th output step, the dynamic stops as SelfDynamics' are
    sq_stops, sq_events = sq === nothing ? (Int[], nothing) : sq_schedule(sq, total_steps)
    sq === nothing || sq_setup!(dev, sq, state.unitcell)
    sq_i = 1
    # the currents: SelfDynamics' stops; their device calls come after sq's at a shared step
    cur_stops, cur_events = currents === nothing ? (Int[], nothing) : cur_schedule(currents, total_steps)
    currents === nothing || cur_setup!(dev, currents, state.unitcell)
    cur_i = 1
    # cage-relative dynamics: SelfDynamics' stops; its device calls come after every other sampler's at a shared step
    cage_stops, cage_events = cage === nothing ? (Int[], nothing) : cage_schedule(cage, total_steps)
    cage === nothing || cage_setup!(dev, cage)
    cage_i = 1
    # four-point dynamics: SelfDynamics' stops; its device calls come last at a shared step, after cage's
    fp_stops, fp_events = four_point === nothing ? (Int[], nothing) : chi4_schedule(four_point, total_steps)
    four_point === nothing || chi4_setup!(dev, four_point, state.unitcell)
    fp_i = 1
    trajectory_file, thermo_file = open_files(pathname, traj_name, thermo_name)
    open(io -> println(io, "# Step Energy Temperature Pressure"), thermo_file, "a")
    volume = abs(det(state.unitcell))                                                # src/simulation.jl:7-9
    nvt = ensemble isa NVT
    # Brownian method: the device's noise stream is keyed by one draw of state.rng; the virial is sampled every 10th
    # step and averaged at the output steps (src/simulation.jl:253-266)
    brown_seed = brownian ? rand(state.rng, UInt64) >> 1 : UInt64(0)
    vir_sum = 0.0; vir_cnt = 0.0
    snapshot_times = log_times ? vcat(0, generate_log_times()) : Int[]                # src/simulation.jl:80-87
    snap_i = 1
    step = 0
    uwk = zeros(3); bout = zeros(4)
    # A frame is exported asynchronously (snapshot_begin) and collected after the NEXT segment has run: its device-to-host
    # copy overlaps that segment.  `pending` = the files the frame in flight goes to: (path, step, mode).
    pending = Tuple{String,Int,String}[]
    function collect_frame!()
        isempty(pending) && return
        X, IM = snapshot_end(dev)
        for (path, at, mode) in pending
            write_to_file_lammps(path, at, state.unitcell, n, X, IM, state.diameters, d; mode=mode)
        end
        empty!(pending)
    end
    while step < total_steps
        next_out = mod(step, frequency) == 0 ? step : (step ÷ frequency + 1) * frequency
        if log_times
            while snap_i <= length(snapshot_times) && snapshot_times[snap_i] < step; snap_i += 1; end
            snap_i <= length(snapshot_times) && (next_out = min(next_out, snapshot_times[snap_i]))
        end
        while dyn_i <= length(dyn_stops) && dyn_stops[dyn_i] < step; dyn_i += 1; end
        dyn_i <= length(dyn_stops) && (next_out = min(next_out, dyn_stops[dyn_i]))
        while sq_i <= length(sq_stops) && sq_stops[sq_i] < step; sq_i += 1; end
        sq_i <= length(sq_stops) && (next_out = min(next_out, sq_stops[sq_i]))
        while cur_i <= length(cur_stops) && cur_stops[cur_i] < step; cur_i += 1; end
        cur_i <= length(cur_stops) && (next_out = min(next_out, cur_stops[cur_i]))
        while cage_i <= length(cage_stops) && cage_stops[cage_i] < step; cage_i += 1; end
        cage_i <= length(cage_stops) && (next_out = min(next_out, cage_stops[cage_i]))
        while fp_i <= length(fp_stops) && fp_stops[fp_i] < step; fp_i += 1; end
        fp_i <= length(fp_stops) && (next_out = min(next_out, fp_stops[fp_i]))
        last = min(next_out, total_steps - 1)
        ns = last - step + 1
        if brownian
            rc = @ccall gc_safe=true LIB.md_run_brownian(dev.h::Ptr{Cvoid}, ns::Int64, params.dt::Float64,
                              ensemble.ktemp::Float64, brown_seed::UInt64, step::Int64, 10::Int64, bout::Ptr{Float64})::Cint
            check(dev, rc)
            uwk[1] = bout[1]; uwk[2] = bout[2]; uwk[3] = 0.0
            vir_sum += bout[3]; vir_cnt += bout[4]
        else
            kt = nvt ? Float64[ensemble.ktemp(s + 1) for s in step:last] : Float64[]   # step+1: src/simulation.jl:108
            r1 = zeros(nvt ? ns : 0); r2 = zeros(nvt ? ns : 0)
            if nvt
                for s in 1:ns
                    r1[s] = randn(state.rng)                                       # draw order: src/thermostat.jl:32-33
                    r2[s] = sum_noises(state.nf - 1, state.rng)
                end
            end
            # long-running and allocation-free on the Julia side: safe to run GC-safe
            rc = @ccall gc_safe=true LIB.md_run(dev.h::Ptr{Cvoid}, ns::Int64, params.dt::Float64, (nvt ? 1 : 0)::Cint,
                              (nvt ? ensemble.tau : 0.0)::Float64, state.nf::Float64, kt::Ptr{Float64}, r1::Ptr{Float64},
                              r2::Ptr{Float64}, uwk::Ptr{Float64})::Cint
            check(dev, rc)
        end
        collect_frame!()                 # the frame exported before this segment
        step = last + 1
        if mod(last, frequency) == 0                                               # src/simulation.jl:118-136
            if brownian
                T = ensemble.ktemp                                                 # src/simulation.jl:259-266
                e = uwk[1] / n
                P = vir_sum / (d * max(vir_cnt, 1.0) * volume) + params.ρ * ensemble.ktemp
                vir_sum = 0.0; vir_cnt = 0.0
            else
                T = 2.0 * uwk[3] / state.nf
                e = (uwk[1] + energy_lrc(params.potential, n, volume)) / n         # :120-124
                P = uwk[2] / (d * volume) + params.ρ * T + pressure_lrc(params.potential, n, volume)   # :128-131
            end
            open(io -> @printf(io, "%d %.6f %.6f %.6f\n", last, e, T, P), thermo_file, "a")
            state.system.energy_and_forces.energy = uwk[1]; state.system.energy_and_forces.virial = uwk[2]
            push!(pending, (trajectory_file, last, "a"))                           # src/simulation.jl:139-151
        end
        if rdf !== nothing && mod(last, frequency) == 0 && mod(last ÷ frequency, rdf.every) == 0
            rdf_sample!(dev)                         # only where the loop stops anyway: no extra segment cut
        end
        if dyn_i <= length(dyn_stops) && dyn_stops[dyn_i] == last
            dyn_act!(dev, dyn_events[last])          # the samples, then the new origin
            dyn_i += 1
        end
        if sq !== nothing
            sq_static = mod(last, frequency) == 0 && mod(last ÷ frequency, sq.every) == 0
            sq_ev = nothing
            if sq_i <= length(sq_stops) && sq_stops[sq_i] == last
                sq_ev = sq_events[last]; sq_i += 1
            end
            (sq_static || sq_ev !== nothing) && sq_act!(dev, sq_static, sq_ev)   # rho once: static, samples, origin
        end
        if cur_i <= length(cur_stops) && cur_stops[cur_i] == last
            cur_act!(dev, cur_events[last])          # j once: static (at an origin stop), samples, origin
            cur_i += 1
        end
        if cage_i <= length(cage_stops) && cage_stops[cage_i] == last
            cage_act!(dev, cage_events[last])        # the samples, then the new origin and its neighbour table
            cage_i += 1
        end
        if fp_i <= length(fp_stops) && fp_stops[fp_i] == last
            chi4_act!(dev, fp_events[last])          # the samples, then the new origin
            fp_i += 1
        end
        if log_times && snap_i <= length(snapshot_times) && snapshot_times[snap_i] == last   # :153-171
            push!(pending, (joinpath(pathname, "snapshot.$(last)"), last, "w"))
            snap_i += 1
        end
        isempty(pending) || snapshot_begin(dev)      # gather + copy to pinned memory: overlaps the next segment
    end
    collect_frame!()
    X, V, F, IM = download(dev)
    unpack!(state.system.positions, X); unpack!(state.system.energy_and_forces.forces, F)
    brownian || (state.velocities = [V[:, i] for i in 1:n])
    state.images .= IM
    # finalize_simulation!: src/simulation.jl:11-36
    write_to_file(joinpath(pathname, "final.xyz"), total_steps, state.unitcell, n, X, state.diameters, d; mode="w")
    if rdf !== nothing
        rdf_collect!(dev, rdf, state.unitcell)
        write_rdf(joinpath(pathname, "rdf.txt"), rdf)
    end
    if dynamics !== nothing
        dyn_collect!(dev, dynamics, d, params.dt)
        write_dynamics(joinpath(pathname, "dynamics.txt"), dynamics)
        dynamics.nbins > 0 && write_van_hove(joinpath(pathname, "vanhove.txt"), dynamics)
    end
    if sq !== nothing
        sq_collect!(dev, sq, params.dt)
        write_sq(joinpath(pathname, "sq.txt"), sq)
        sq.dynamic && write_fqt(joinpath(pathname, "fqt.txt"), sq)
    end
    if currents !== nothing
        cur_collect!(dev, currents, d, params.dt)
        isempty(currents.qvec) || write_currents(joinpath(pathname, "currents.txt"), currents)
        currents.with_vacf && write_vacf(joinpath(pathname, "vacf.txt"), currents)
    end
    if cage !== nothing
        cage_collect!(dev, cage, d, params.dt)
        write_cage(joinpath(pathname, "cage.txt"), cage)
    end
    if four_point !== nothing
        chi4_collect!(dev, four_point, params.dt)
        write_chi4(joinpath(pathname, "chi4.txt"), four_point)
        isempty(four_point.qvec) || write_s4(joinpath(pathname, "s4.txt"), four_point)
    end
    compress && isfile(trajectory_file) && compress_zstd(trajectory_file)
    return nothing
end

# ---- fire_minimize!: src/minimize.jl:31-135 (same keywords and defaults; returns (energy, true) or nothing) ----
function fire_minimize!(state::SimulationState, params::Parameters; dimension::Int=2, max_steps::Int=10000,
                        tol::Float64=1e-6, dt_initial::Float64=0.01, dt_max::Float64=0.1, alpha0::Float64=0.1,
                        f_inc::Float64=1.2, f_dec::Float64=0.2, Nmin::Int=5)
    dev = state.system.device; d = state.dimension; n = params.n_particles
    configure!(dev, params.potential)
    X = pack(state.system.positions, d); F = pack(state.system.energy_and_forces.forces, d)
    check(dev, ccall((:md_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                     dev.h, X, C_NULL, F, state.images, state.diameters))
    steps = Ref{Int64}(0); conv = Ref{Cint}(0); energy = Ref{Float64}(0.0); frms = Ref{Float64}(0.0)
    rc = @ccall gc_safe=true LIB.md_fire_minimize(dev.h::Ptr{Cvoid}, max_steps::Int64, tol::Float64, dt_initial::Float64,
                      dt_max::Float64, alpha0::Float64, f_inc::Float64, f_dec::Float64, Nmin::Cint, steps::Ptr{Int64},
                      conv::Ptr{Cint}, energy::Ptr{Float64}, frms::Ptr{Float64})::Cint
    check(dev, rc)
    check(dev, ccall((:md_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                     dev.h, X, C_NULL, F, state.images))
    unpack!(state.system.positions, X); unpack!(state.system.energy_and_forces.forces, F)
    state.system.energy_and_forces.energy = energy[]
    conv[] != 0 && return energy[], true
    @warn "FIRE did not converge after $(max_steps) steps; final F_norm = $(frms[])"
    return nothing
end

"minimize!(state, params, pathname, dimension; method=:FIRE, save_config=\"minimized.xyz\", kwargs...): src/minimize.jl:166-197"
function minimize!(state::SimulationState, params::Parameters, pathname::String, dimension::Int; method::Symbol=:FIRE,
                   save_config::String="minimized.xyz", kwargs...)
    if method == :FIRE
        fire_minimize!(state, params; dimension=dimension, kwargs...)
    else
        error("Unknown minimization method: $method")
    end
    X = pack(state.system.positions, state.dimension)
    write_to_file(joinpath(pathname, save_config), 0, state.unitcell, params.n_particles, X, state.diameters, dimension)
    return nothing
end

# ---- deformation of a live sample: md_set_cell, md_nonaffine_*, AQS (moleculardynamics/jl_amd/deformation.py) ----
# The unit cell has the lattice vectors in its columns; F acts from the left, U' = F U.  params is never touched: after a
# change of volume params.ρ is the caller's to keep consistent, the reference's own convention.
const MD_CELL_AFFINE = 0
const MD_CELL_LATTICE = 1

function simple_shear(d::Int, gamma::Real; plane=(1, 2))                           # axes are 1-based here
    F = Matrix{Float64}(I, d, d); F[plane[1], plane[2]] = gamma; return F
end
function pure_shear(d::Int, eps::Real; plane=(1, 2))
    1.0 + eps > 0.0 || error("eps must be > -1")
    F = Matrix{Float64}(I, d, d); F[plane[1], plane[1]] = 1.0 + eps; F[plane[2], plane[2]] = 1.0 / (1.0 + eps); return F
end
function volumetric(d::Int, eps::Real)
    1.0 + eps > 0.0 || error("eps must be > -1")
    return Matrix{Float64}(I, d, d) .* (1.0 + eps)
end

function device_set_cell!(state::SimulationState, U::AbstractMatrix, mode::Integer)
    dev = state.system.device
    box = Matrix{Float64}(U)
    check(dev, ccall((:md_set_cell, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), dev.h, box, mode))
    state.unitcell = box; state.system.unitcell = box
    return nothing
end

# ---- constant pressure: md_scale_cell (moleculardynamics/jl_amd/barostat.py, DESIGN.md section 26) ----
# The device call of stochastic cell rescaling.  run_simulation!'s barostat keyword exists in the Python driver only: the
# Julia run loop does not drive the coupling.
"""
    scale_cell!(state, mu, vscale=1.0) -> rows_kept

Scale the whole frame isotropically: cell and positions times mu, velocities times vscale, nothing wrapped; the Verlet rows
are kept with the skins they still leave (1) or retired (0).  Forces are those of the old cell until the next evaluation.
"""
function scale_cell!(state::SimulationState, mu::Real, vscale::Real=1.0)
    dev = state.system.device
    kept = Ref{Cint}(0)
    check(dev, ccall((:md_scale_cell, LIB), Cint, (Ptr{Cvoid}, Float64, Float64, Ptr{Cint}), dev.h, mu, vscale, kept))
    box = Float64(mu) .* Matrix{Float64}(state.unitcell)
    state.unitcell = box; state.system.unitcell = box
    return Int(kept[])
end

# ---- shear flow: md_deform_cell (moleculardynamics/jl_amd/deformation.py ShearFlow, DESIGN.md section 27) ----
# The device call of SLLOD in a deforming cell.  run_simulation!'s shear keyword exists in the Python driver only: the Julia
# run loop does not drive the flow.
"""
    deform_cell!(state, F, G=nothing) -> rows_kept

Map the whole frame by the deformation gradient F: the cell becomes F U, positions F x and, with G, velocities G v
(G = inv(F): peculiar velocities), nothing wrapped; the Verlet rows are kept with the skins they still leave (1) or retired
(0).  Forces are those of the old cell until the next evaluation.
"""
function deform_cell!(state::SimulationState, F::AbstractMatrix, G::Union{AbstractMatrix,Nothing}=nothing)
    dev = state.system.device
    kept = Ref{Cint}(0)
    Fr = Matrix{Float64}(permutedims(F))           # row-major for the C side
    Gr = G === nothing ? C_NULL : Matrix{Float64}(permutedims(G))
    check(dev, ccall((:md_deform_cell, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}), dev.h, Fr, Gr, kept))
    box = Matrix{Float64}(F) * Matrix{Float64}(state.unitcell)
    state.unitcell = box; state.system.unitcell = box
    return Int(kept[])
end

"(M0, M1, sig): the maps since the list build and the last prune (d x d) and the singular-value bounds s0, S0, s1, S1"
function deform_state(dev::Device)
    m0 = zeros(9); m1 = zeros(9); sig = zeros(4)
    check(dev, ccall((:md_deform_state, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), dev.h, m0, m1, sig))
    d = dev.dim
    return permutedims(reshape(m0, 3, 3))[1:d, 1:d], permutedims(reshape(m1, 3, 3))[1:d, 1:d], sig
end

"mark the frame the device holds: fractional coordinates and image counts by particle index"
nonaffine_mark!(dev::Device) = (check(dev, ccall((:md_nonaffine_mark, LIB), Cint, (Ptr{Cvoid},), dev.h)); nothing)

"(sums[8], u d x N or nothing): the displacement since the mark with the affine part taken out (md_nonaffine)"
function nonaffine(dev::Device; fields::Bool=false)
    sums = zeros(8)
    u = fields ? Matrix{Float64}(undef, dev.dim, dev.n) : nothing
    check(dev, ccall((:md_nonaffine, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), dev.h, sums, fields ? u : C_NULL))
    return sums, u
end

"set_unitcell!(state, params, unitcell; remap=:affine | :lattice, upload=true): see deformation.py set_unitcell"
function set_unitcell!(state::SimulationState, params::Parameters, unitcell::AbstractMatrix; remap::Symbol=:affine,
                       upload::Bool=true)
    remap in (:affine, :lattice) || error("remap must be :affine or :lattice")
    dev = state.system.device; d = state.dimension
    configure!(dev, params.potential)
    if upload
        X = pack(state.system.positions, d)
        check(dev, ccall((:md_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                         dev.h, X, C_NULL, C_NULL, state.images, state.diameters))
    end
    device_set_cell!(state, unitcell, remap == :affine ? MD_CELL_AFFINE : MD_CELL_LATTICE)
    X, _, _, IM = download(dev)
    unpack!(state.system.positions, X); state.images .= IM
    return nothing
end

deform!(state::SimulationState, params::Parameters, F::AbstractMatrix; upload::Bool=true) =
    set_unitcell!(state, params, F * state.unitcell; remap=:affine, upload=upload)

face_distances(U::AbstractMatrix) = (Ui = inv(U); [1.0 / norm(Ui[r, :]) for r in 1:size(U, 1)])

"(U * M, M): pairwise Gauss reduction of the columns of U; a step that would shrink a face distance is not taken"
function gauss_reduce(U::AbstractMatrix)
    d = size(U, 1); M = Matrix{Int64}(I, d, d); W = Matrix{Float64}(U)
    for _ in 1:64
        changed = false
        for a in 1:d, b in 1:d
            a == b && continue
            k = round(Int64, dot(W[:, b], W[:, a]) / dot(W[:, a], W[:, a]), RoundNearest)
            k == 0 && continue
            M2 = copy(M); M2[:, b] .-= k .* M2[:, a]
            W2 = Matrix{Float64}(U) * Float64.(M2)
            any(face_distances(W2) .< face_distances(W) .* (1.0 - 1e-12)) && continue
            M = M2; W = W2; changed = true
        end
        changed || break
    end
    return W, M
end

"reduce_cell!(state, params): the reduced cell of the same lattice, particles where they are; the integer matrix or nothing"
function reduce_cell!(state::SimulationState, params::Parameters; upload::Bool=true)
    W, M = gauss_reduce(state.unitcell)
    M == Matrix{Int64}(I, state.dimension, state.dimension) && return nothing
    set_unitcell!(state, params, W; remap=:lattice, upload=upload)
    return M
end

function aqs_columns(d::Int)
    comps = d == 3 ? ((1, 1), (2, 2), (3, 3), (1, 2), (1, 3), (2, 3)) : ((1, 1), (2, 2), (1, 2))
    return vcat(["step", "strain", "energy"], ["stress_" * "xyz"[a] * "xyz"[b] for (a, b) in comps],
                ["pressure", "fire_steps", "converged", "d2_nonaffine", "participation", "max_u", "flips"]), comps
end

"athermal_quasistatic_shear!(state, params, pathname, strain_step, nsteps; mode, plane, tol, reduce, mark, on_step,
max_steps, dt_initial, dt_max, alpha0, f_inc, f_dec, Nmin): deformation.py athermal_quasistatic_shear, the same aqs.txt.
The handle's pressure-tensor sampler is set up afresh (md_stress_setup, no lags): an earlier setup and its sums are discarded."
function athermal_quasistatic_shear!(state::SimulationState, params::Parameters, pathname::String, strain_step::Real,
                                     nsteps::Int; mode::Symbol=:simple, plane=(1, 2), tol::Float64=1e-9, reduce::Bool=true,
                                     mark::Symbol=:previous, on_step=nothing, max_steps::Int=10000,
                                     dt_initial::Float64=0.01, dt_max::Float64=0.1, alpha0::Float64=0.1,
                                     f_inc::Float64=1.2, f_dec::Float64=0.2, Nmin::Int=5)
    mark in (:previous, :start) || error("mark must be :previous or :start")
    mode in (:simple, :pure, :volumetric) || error("mode must be :simple, :pure or :volumetric")
    nsteps >= 1 || error("nsteps must be >= 1")
    tol > 0.0 || error("tol must be > 0")
    dev = state.system.device; d = state.dimension; n = params.n_particles
    F = mode == :simple ? simple_shear(d, strain_step; plane=plane) :
        mode == :pure ? pure_shear(d, strain_step; plane=plane) : volumetric(d, strain_step)
    configure!(dev, params.potential)
    X = pack(state.system.positions, d); Fo = pack(state.system.energy_and_forces.forces, d)
    check(dev, ccall((:md_upload, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                     dev.h, X, C_NULL, Fo, state.images, state.diameters))
    check(dev, ccall((:md_stress_setup, LIB), Cint, (Ptr{Cvoid}, Cint), dev.h, 0))
    names, comps = aqs_columns(d)
    nc = length(comps)
    rows = Vector{Vector{Float64}}()
    mark == :start && nonaffine_mark!(dev)
    kin = zeros(nc); vir = zeros(nc)
    eye = Matrix{Int64}(I, d, d)
    for k in 1:nsteps
        device_set_cell!(state, F * state.unitcell, MD_CELL_AFFINE)
        flips = 0
        if reduce
            W, M = gauss_reduce(state.unitcell)
            if M != eye
                device_set_cell!(state, W, MD_CELL_LATTICE); flips = 1
            end
        end
        mark == :previous && nonaffine_mark!(dev)
        steps = Ref{Int64}(0); conv = Ref{Cint}(0); energy = Ref{Float64}(0.0); frms = Ref{Float64}(0.0)
        rc = @ccall gc_safe=true LIB.md_fire_minimize(dev.h::Ptr{Cvoid}, max_steps::Int64, tol::Float64, dt_initial::Float64,
                          dt_max::Float64, alpha0::Float64, f_inc::Float64, f_dec::Float64, Nmin::Cint, steps::Ptr{Int64},
                          conv::Ptr{Cint}, energy::Ptr{Float64}, frms::Ptr{Float64})::Cint
        check(dev, rc)
        check(dev, ccall((:md_stress_sample, LIB), Cint, (Ptr{Cvoid},), dev.h))
        check(dev, ccall((:md_stress_tensor, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), dev.h, kin, vir))
        volume = abs(det(state.unitcell))
        stress = -vir ./ volume
        sums, _ = nonaffine(dev)
        s2 = sums[4]; s4 = sums[5]
        pressure = -sum(stress[i] for (i, (a, b)) in enumerate(comps) if a == b) / d
        row = vcat([k, k * strain_step, energy[] / n], stress,
                   [pressure, steps[], conv[] != 0 ? 1 : 0, s2 / n, s4 > 0.0 ? s2 * s2 / (n * s4) : 0.0, sqrt(sums[6]), flips])
        push!(rows, row)
        on_step === nothing || on_step(Dict(zip(names, row)))
    end
    X, _, Fd, IM = download(dev)
    unpack!(state.system.positions, X); unpack!(state.system.energy_and_forces.forces, Fd); state.images .= IM
    state.system.energy_and_forces.energy = rows[end][3] * n
    mkpath(pathname)
    ints = Set(["step", "fire_steps", "converged", "flips"])
    open(joinpath(pathname, "aqs.txt"), "w") do io
        println(io, "# " * join(names, " "))
        for row in rows
            println(io, join([nm in ints ? @sprintf("%d", Int(v)) : @sprintf("%.17g", v) for (nm, v) in zip(names, row)], " "))
        end
    end
    return Dict(nm => [row[i] for row in rows] for (i, nm) in enumerate(names))
end

end # module
