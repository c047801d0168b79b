# KlaraHIP.jl — Julia host side of libklara_hip.so: Klara's own sampler / tuner / range structs in, Klara's own
# BasicContMuvParameterNState out, the transition loop on an MI355X in between (include/klara_hip.h, INTEGRATION.md).
# Package layout: julia/KlaraHIP/{REQUIRE, src/KlaraHIP.jl, test/runtests.jl}; put julia/ on LOAD_PATH (or Pkg.clone the directory).
#
#     using Klara, KlaraHIP
#     plogtarget = GaussDiagTarget(2)                                     # README.md:23 `plogtarget(z) = -dot(z, z)` as a device target family
#     p      = HIPParameter(:p, logtarget=plogtarget)                     # README.md:30  BasicContMuvParameter(:p, logtarget=plogtarget)
#     model  = likelihood_model(p, false)                                 # README.md:35  unchanged: HIPParameter <: Klara.Parameter{Continuous, Multivariate}
#     job    = HIPMCJob(model, MH(ones(2)), BasicMCRange(nsteps=10000, burnin=1000), Dict(:p => [5.1, -0.9]))     # README.md:39-51 BasicMCJob(model, sampler, mcrange, v0)
#     run(job); chain = output(job); mean(chain); acceptance(chain)      # README.md:55-59 unchanged
#     reset(job); run(job)                                                # an independent replicate (BasicMCJob.jl:187-201)
#
# Many chains of one model — what the device is for — are the same call with `nchains` (v0's vector is every chain's start) or a D x N matrix of starts:
#     job    = HIPMCJob(model, MALA(0.9), BasicMCRange(nsteps=10000, burnin=1000), Dict(:p => randn(100, 65536));
#                       tuner=VanillaMCTuner(), outopts=Dict(:monitor => [:value], :diagnostics => [:accept]))
#     run(job); chain = output(job, 1); mean(chain); acceptance(chain)
#
# `run`, `reset` (Base generics Klara extends: src/Klara.jl:26-27) and `output` (Klara's own, exported at src/Klara.jl:232) are
# IMPORTED before the methods below are defined, so `run(job)`, `reset(job[, x])`, `output(job[, c])` on an HIPMCJob are methods
# of the same functions a Klara user already calls on a BasicMCJob (src/jobs/BasicMCJob.jl:187-201,212,279); HIPMCJob <: Klara.MCJob,
# so `run(jobs::Vector)` (src/jobs/jobs.jl:212) maps over HIP jobs too.  Everything else the example names is exported below.
#
# UNTESTED in the build image (no Julia there); tests/test_host_api.py checks mechanically what can be checked without it: the
# struct layout against the C header, the descriptor builder's argument order, the Klara field names each mapping reads
# (cited below), that only declared symbols are bound, that blocks / brackets balance, that every unqualified name of the example
# above and of INTEGRATION.md is exported here or by Klara, that every generic of Klara / Base this file adds methods to is imported
# first, and that nothing reaches through the caller's top-level module.  One file for Klara's own Julia 0.6
# (REQUIRE:1 — `Void`, `Array{T}(dims)`, `finalizer(obj, f)`) and for Julia >= 0.7 (`Cvoid`, `Array{T}(undef, dims)`,
# `finalizer(f, obj)`): the three differences are confined to the compatibility block below, everything else is common syntax.
module KlaraHIP
import Klara
import Klara: output, MCJob, MH, MALA, SMMALA, RAM, AM, MuvAMWG, HMC, SliceSampler, VanillaMCTuner, AcceptanceRateMCTuner, DualAveragingMCTuner, RobertsRosenthalMCTuner,
              BasicContMuvParameterState, BasicContMuvParameterNState, erf_rate_score, logistic_rate_score,
              Parameter, GenericModel, VariableState, VariableStateVector, DiffOptions
import Distributions
import Distributions: Continuous, Multivariate
import Base: run, reset, show
export HIPMCJob, HIPParameter, HIPTarget, GaussDiagTarget, GaussDenseTarget, LogisticTarget, HierNormalTarget, CustomTarget,
       chainvalue, chainmeans, chainacceptance, chainmcvar_bm, chainlzv, chainqzv, streamkey, launchmodes, shaderclock, check_custom_target,
       check_custom_target_softabs, SoftAbs, ramfactor, amstate, amwgstate, mhfactor, setmhfactor!,
       HIPComm, comm_unique_id, comm_info, gather_summaries, gather_moments, pooledmoments, gather_covariance, pooledcovariance, rhat, gather_rhat, pooledess, gather_ess,
       pooledhistogram, pooledquantiles, gather_histogram, Derived, derivedsums, derivedmoments, derivedrhat, derivedhistogram, derivedquantiles,
       gather_derived_moments, gather_derived_rhat, gather_derived_histogram, check_derived, KlaraDesc, klara_desc
const lib = "libklara_hip"            # klara.jl_amd/lib/libklara_hip.so on LD_LIBRARY_PATH

# ---------------------------------------------------------------- Julia 0.6 / >= 0.7 compatibility (the only version-dependent code)
@static if VERSION < v"0.7.0-"
    const Cvoid = Void
    newarray(::Type{T}, dims::Integer...) where {T} = Array{T}(dims...)
    on_finalize(obj, f) = finalizer(obj, f)
else
    newarray(::Type{T}, dims::Integer...) where {T} = Array{T}(undef, dims...)
    on_finalize(obj, f) = finalizer(f, obj)
end

# ---------------------------------------------------------------- constants of include/klara_hip.h
const KLARA_ABI_VERSION = UInt32(6)
const SAMPLER_MH, SAMPLER_MALA, SAMPLER_HMC, SAMPLER_SLICE = Int32(0), Int32(1), Int32(2), Int32(3)
const SAMPLER_SMMALA = Int32(4)      # SMMALA(driftstep) with transform = nothing or SoftAbs(a); the logistic target or a CustomTarget's tensor, D <= 8
const SAMPLER_RAM = Int32(6)         # RAM(S0; targetrate, γ): the logistic target or a CustomTarget's whole-vector closure, D <= 8 (5 is reserved)
const SAMPLER_AM = Int32(8)          # AM(C0; corescale, minorscale, c, t0): RAM's targets, D <= 8 (7 is reserved)
const SAMPLER_AMWG = Int32(10)       # MuvAMWG(σ) with RobertsRosenthalMCTuner: the logistic target up to 16 parameters or a CustomTarget's whole-vector closure, D <= 32 (9 is reserved)
const SAMPLER_MH_COV = Int32(12)     # MH(Σ::Matrix) with a Σ that is not diagonal: AMWG's targets, D <= 32, one factor for the job (11 is reserved)
const TARGET_GAUSS_DIAG, TARGET_GAUSS_DENSE, TARGET_LOGISTIC, TARGET_HIER_NORMAL, TARGET_CUSTOM = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4)
const TUNER_VANILLA, TUNER_ACCEPT_RATE, TUNER_DUAL_AVERAGING = Int32(0), Int32(1), Int32(2)
const TUNER_ROBERTS_ROSENTHAL = Int32(3)      # RobertsRosenthalMCTuner(targetrate, period): MuvAMWG only
const TUNE_PER_CHAIN, TUNE_POOLED = Int32(0), Int32(1)
const MON_ACCEPT, MON_HISTORY, MON_SUMMARIES, MON_HIST_LT, MON_HIST_GRAD, MON_HIST_LLLP = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
const MARG_MAX_BINS = 1024             # KLARA_MARG_MAX_BINS
const DERIVED_MAX_OUT = 64             # KLARA_DERIVED_MAX_OUT
const MON_COVARIANCE = 0x40            # KLARA_MON_COVARIANCE: the pooled D x D cross-products, accumulated while sampling (pooledcovariance)

# struct klara_desc — field order/types exactly as include/klara_hip.h
struct KlaraDesc
    struct_size::UInt32; abi_version::UInt32
    sampler::Int32; target::Int32; tuner::Int32; tuner_mode::Int32
    nchains::Int64; chain_offset::Int64; ndims::Int32; device::Int32
    mh_sigma::Ptr{Float64}; driftstep::Float64; leapstep::Float64
    nleaps::Int32; slice_stepout::Int32; slice_widths::Ptr{Float64}; amwg_logsigma0::Ptr{Float64}; mh_factor::Ptr{Float64}
    targetrate::Float64; score_k::Float64; period::Int32; verbose::Int32
    da_nadapt::Int64; da_eps0bar::Float64; da_h0bar::Float64; da_gamma::Float64; da_kappa::Float64
    da_t0::Int32; tuner_score::Int32
    nsteps::Int64; burnin::Int64; thinning::Int64
    gauss_w::Ptr{Float64}; gauss_mu::Ptr{Float64}; gauss_const::Float64; gauss_prec::Ptr{Float64}
    logit_X::Ptr{Float64}; logit_y::Ptr{Float64}; logit_ndata::Int32; nstreams::Int32; logit_lambda::Float64
    hier_Y::Ptr{Float64}; hier_xc::Ptr{Float64}; hier_nunits::Int32; hier_ntimes::Int32
    hier_prior_prec::Float64; hier_gamma_a::Float64; hier_gamma_b::Float64
    custom_src::Cstring; custom_data::Ptr{Float64}; custom_ndata::Int64; bm_batchlen::Int64
    hist_ring_cols::Int64; acov_maxlag::Int32; sparse_moves::Int32
    smmala_softabs::Float64
    am_C0::Ptr{Float64}; am_corescale::Float64; am_minorscale::Float64; am_c::Float64; am_t0::Int64
    ram_S0::Ptr{Float64}; ram_targetrate::Float64; ram_gamma::Float64
    marg_lo::Ptr{Float64}; marg_hi::Ptr{Float64}; marg_nbins::Int64
    seed::UInt64; monitor::UInt32; steps_per_launch::Int32
    derived_src::Cstring; derived_data::Ptr{Float64}; derived_ndata::Int64; derived_nout::Int64; derived_nbins::Int64
    derived_lo::Ptr{Float64}; derived_hi::Ptr{Float64}
    stream::Ptr{Cvoid}
end

# every field by keyword, defaults = "not used"; the positional call below must list the fields in struct order (checked by
# tests/test_host_api.py)
function klara_desc(; sampler=SAMPLER_MH, target=TARGET_GAUSS_DIAG, tuner=TUNER_VANILLA, tuner_mode=TUNE_PER_CHAIN,
                    nchains=1, chain_offset=0, ndims=1, device=0,
                    mh_sigma=Ptr{Float64}(C_NULL), driftstep=1.0, leapstep=0.1, nleaps=10, slice_stepout=1, slice_widths=Ptr{Float64}(C_NULL),
                    amwg_logsigma0=Ptr{Float64}(C_NULL), mh_factor=Ptr{Float64}(C_NULL),
                    targetrate=0.0, score_k=7.0, period=100, verbose=0,
                    da_nadapt=0, da_eps0bar=1.0, da_h0bar=0.0, da_gamma=0.05, da_kappa=0.75, da_t0=10, tuner_score=0,
                    nsteps=100, burnin=0, thinning=1,
                    gauss_w=Ptr{Float64}(C_NULL), gauss_mu=Ptr{Float64}(C_NULL), gauss_const=0.0, gauss_prec=Ptr{Float64}(C_NULL),
                    logit_X=Ptr{Float64}(C_NULL), logit_y=Ptr{Float64}(C_NULL), logit_ndata=0, nstreams=0, logit_lambda=100.0,
                    hier_Y=Ptr{Float64}(C_NULL), hier_xc=Ptr{Float64}(C_NULL), hier_nunits=0, hier_ntimes=0,
                    hier_prior_prec=1e-4, hier_gamma_a=1e-3, hier_gamma_b=1e-3,
                    custom_src=Cstring(C_NULL), custom_data=Ptr{Float64}(C_NULL), custom_ndata=0, bm_batchlen=0,
                    hist_ring_cols=0, acov_maxlag=0, sparse_moves=0, smmala_softabs=0.0,
                    am_C0=Ptr{Float64}(C_NULL), am_corescale=0.0, am_minorscale=0.0, am_c=0.0, am_t0=0,
                    ram_S0=Ptr{Float64}(C_NULL), ram_targetrate=0.0, ram_gamma=0.0,
                    marg_lo=Ptr{Float64}(C_NULL), marg_hi=Ptr{Float64}(C_NULL), marg_nbins=0,
                    seed=UInt64(0), monitor=UInt32(0), steps_per_launch=0,
                    derived_src=Cstring(C_NULL), derived_data=Ptr{Float64}(C_NULL), derived_ndata=0, derived_nout=0, derived_nbins=0,
                    derived_lo=Ptr{Float64}(C_NULL), derived_hi=Ptr{Float64}(C_NULL), stream=C_NULL)
    KlaraDesc(UInt32(sizeof(KlaraDesc)), KLARA_ABI_VERSION,
              sampler, target, tuner, tuner_mode,
              nchains, chain_offset, ndims, device,
              mh_sigma, driftstep, leapstep,
              nleaps, slice_stepout, slice_widths, amwg_logsigma0, mh_factor,
              targetrate, score_k, period, verbose,
              da_nadapt, da_eps0bar, da_h0bar, da_gamma, da_kappa,
              da_t0, tuner_score,
              nsteps, burnin, thinning,
              gauss_w, gauss_mu, gauss_const, gauss_prec,
              logit_X, logit_y, logit_ndata, nstreams, logit_lambda,
              hier_Y, hier_xc, hier_nunits, hier_ntimes,
              hier_prior_prec, hier_gamma_a, hier_gamma_b,
              custom_src, custom_data, custom_ndata, bm_batchlen,
              hist_ring_cols, acov_maxlag, sparse_moves, smmala_softabs,
              am_C0, am_corescale, am_minorscale, am_c, am_t0,
              ram_S0, ram_targetrate, ram_gamma,
              marg_lo, marg_hi, marg_nbins,
              seed, monitor, steps_per_launch,
              derived_src, derived_data, derived_ndata, derived_nout, derived_nbins,
              derived_lo, derived_hi, stream)
end

# Derived(nout, src; data, marginals): a function of the state, summarised on the device (klara_desc.derived_src ...; the reference's Transformation,
# src/variables/variables.jl:102-119, on the one-parameter job).  src is C text defining
#     KLARA_USER_FN void klara_user_derived(const double* x, int D, const double* data, long long ndata, double* out, int K);
# data its own block of doubles, marginals = (nbins, lo, hi) over the nout outputs (lo, hi scalars or nout values) for their pooled histograms.
struct Derived
    nout::Int; src::String; data::Vector{Float64}; marginals
end
Derived(nout::Integer, src::AbstractString; data=Float64[], marginals=nothing) = Derived(Int(nout), String(src), convert(Vector{Float64}, data), marginals)

# H -> softabs(H, a) (stats/metrics.jl:1-4) as a callable the device path can recognise: SMMALA(1.25, SoftAbs(1000.)) is Klara's own sampler — it
# runs on the CPU through Klara unchanged — and HIPMCJob maps it to klara_desc.smmala_softabs = a (an anonymous closure H -> softabs(H, a) cannot be
# recognised and stays refused)
struct SoftAbs <: Function; a::Float64; end
(s::SoftAbs)(H) = Klara.softabs(H, s.a)

check(st::Cint, what) = st == 0 || error(what, ": ", unsafe_string(ccall((:klara_strerror, lib), Cstring, (Cint,), st)))

# ---------------------------------------------------------------- device target families (klara_target)
# Julia closures cannot run on the GPU: the parameter's target is one of the enumerated families, or C text (CustomTarget) —
# the device form of BasicContMuvParameter(:p, logtarget=f, gradlogtarget=g) / (loglikelihood=..., logprior=...).
abstract type HIPTarget end
struct GaussDiagTarget <: HIPTarget          # lt = c - sum w_i (x_i - mu_i)^2 ; README.md:23 is GaussDiagTarget(D)
    ndims::Int; w::Vector{Float64}; mu::Vector{Float64}; c::Float64
end
GaussDiagTarget(D::Integer) = GaussDiagTarget(D, Float64[], Float64[], 0.0)
struct GaussDenseTarget <: HIPTarget         # lt = c - 1/2 (x-mu)' P (x-mu), P row-major D x D; mu empty = 0
    P::Matrix{Float64}; c::Float64; mu::Vector{Float64}
end
GaussDenseTarget(P::Matrix{Float64}, c::Float64=0.0) = GaussDenseTarget(P, c, Float64[])
struct LogisticTarget <: HIPTarget           # doc/examples/swiss/MALA/analytical.jl:11-18; X is ndata x D
    X::Matrix{Float64}; y::Vector{Float64}; lambda::Float64
end
struct HierNormalTarget <: HIPTarget         # BUGS "Rats" model on data/rats/*.csv (include/klara_hip.h KLARA_TARGET_HIER_NORMAL)
    Y::Matrix{Float64}; xc::Vector{Float64}; prior_prec::Float64; gamma_a::Float64; gamma_b::Float64
end
# diffopts=DiffOptions(mode=:forward[, order=2][, chunksize=n]) (Klara's own, autodiff/autodiff.jl:55-76): the source defines no gradient, only the generic
# klara_user_logtarget_ad (klara.jl_amd/csrc/klara_autodiff.h), and is differentiated on the device by forward-mode dual numbers; order = 2 also gives SMMALA
# its metric, minus the Hessian (autodiff/forward.jl:11-16).  Reverse mode needs tapes, which do not exist on the device.
function autodiff_source(src::AbstractString, diffopts::DiffOptions)
    diffopts.mode == :forward || error("DiffOptions(mode=:reverse): reverse-mode tapes do not exist on the device; use mode=:forward")
    head = string("#define KLARA_USER_AUTODIFF ", Int(diffopts.order), "\n")
    if diffopts.chunksize > 0
        head = string(head, "#define KLARA_USER_AUTODIFF_CHUNK ", Int(diffopts.chunksize), "\n")
    end
    string(head, src)
end
struct CustomTarget <: HIPTarget             # C text of klara_user_logtarget / klara_user_gradlogtarget (or the likelihood + prior form)
    ndims::Int; src::String; data::Vector{Float64}
    CustomTarget(ndims::Integer, src::AbstractString, data::Vector{Float64}=Float64[]; diffopts=nothing) =
        new(ndims, diffopts === nothing ? src : autodiff_source(src, diffopts), data)
end
ndims_of(t::GaussDiagTarget) = t.ndims
ndims_of(t::GaussDenseTarget) = size(t.P, 1)
ndims_of(t::LogisticTarget) = size(t.X, 2)
ndims_of(t::HierNormalTarget) = 2 * size(t.Y, 1) + 5
ndims_of(t::CustomTarget) = t.ndims

# The device form of BasicContMuvParameter (variables/parameters/BasicContMuvParameter.jl:3-28): a Klara.Parameter{Continuous, Multivariate}
# with the fields a GenericModel reads and writes — `key` (GenericModel.jl:44 `m.ofkey[v.key] = n`), `index` (assigned by
# likelihood_model(p, false): GenericModel.jl:110-113 `m.vertices[i].index = i`, hence mutable) and `states` (BasicContMuvParameter.jl:27) — and, in place
# of the closure fields, the device target family.  `likelihood_model(p, false)` (models/generators.jl:20) therefore works on it unchanged.
mutable struct HIPParameter <: Parameter{Continuous, Multivariate}
    key::Symbol
    index::Integer
    target::HIPTarget
    states::VariableStateVector
end
HIPParameter(key::Symbol, target::HIPTarget; index::Integer=0, states::VariableStateVector=VariableState[]) = HIPParameter(key, index, target, states)
# keyword form, mirroring BasicContMuvParameter(key; logtarget=...) (BasicContMuvParameter.jl:383-411): the "closure" is a device target
# (diffopts=DiffOptions(mode=:forward), as in doc/examples/swiss/MALA/forwarddiff.jl: the CustomTarget's text is the generic log-target alone)
with_diffopts(t::HIPTarget, diffopts) = diffopts === nothing ? t :
    isa(t, CustomTarget) ? CustomTarget(t.ndims, t.src, t.data, diffopts=diffopts) : error("HIPParameter: diffopts goes with a CustomTarget")
HIPParameter(key::Symbol; logtarget::HIPTarget=error("HIPParameter: logtarget=<a device target family, e.g. GaussDiagTarget(D)> is required"),
             diffopts=nothing, index::Integer=0, states::VariableStateVector=VariableState[]) = HIPParameter(key, index, with_diffopts(logtarget, diffopts), states)

# ---------------------------------------------------------------- the job
mutable struct HIPMCJob <: MCJob   # stands for N BasicMCJobs of one model (run(jobs::Vector) = map(run, jobs), jobs.jl:212)
    handle::Ptr{Cvoid}; nchains::Int; ndims::Int
    parameter::HIPParameter; sampler; tuner; range        # Klara's own MCSampler / MCTuner / BasicMCRange
    outopts::Dict{Symbol, Any}; monitor::UInt32
    keep::Vector{Any}                                      # host arrays the descriptor pointed at
end

rowmajor(A::Matrix{Float64}) = collect(transpose(A))       # Julia is column-major, the C ABI row-major

# the lower Cholesky factor L of a symmetric positive definite matrix, A = L L' (plain loops: the same text on every Julia version)
function lowerfactor(A::Matrix{Float64})
    n = size(A, 1)
    size(A, 2) == n || error("MH: the proposal covariance must be a square matrix")
    Lf = zeros(n, n)
    for j in 1:n
        s = A[j, j]
        for k in 1:j-1; s -= Lf[j, k]^2; end
        (s > 0 && isfinite(s)) || error("MH: the proposal covariance must be positive definite")
        Lf[j, j] = sqrt(s)
        for i in j+1:n
            a = A[i, j]
            for k in 1:j-1; a -= Lf[i, k] * Lf[j, k]; end
            Lf[i, j] = a / Lf[j, j]
        end
    end
    Lf
end

# Klara's structs -> klara_desc.  Field names read from Klara (file:line in /root/reference/src):
#   MALA.driftstep                         samplers/MALA.jl:61-70
#   SMMALA.driftstep, .transform (nothing or SoftAbs(a)) samplers/SMMALA.jl:127-137
#   RAM.S0, .targetrate, .γ                samplers/RAM.jl:94-111
#   AM.C0, .corescale, .minorscale, .c, .t0 samplers/AM.jl:131-136
#   HMC.leapstep, HMC.nleaps               samplers/HMC.jl:89-100
#   SliceSampler.widths, .stepout          samplers/SliceSampler.jl:22-34
#   MH.setproposal (sigma is inside the closure: MH(sigma) = MH(x -> MvNormal(x, sigma)))   samplers/MH.jl:46-66
#   VanillaMCTuner.period, .verbose        tuners/VanillaMCTuner.jl:6-17
#   AcceptanceRateMCTuner.targetrate, .score, .period, .verbose          tuners/AcceptanceRateMCTuner.jl:25-44
#   DualAveragingMCTuner.targetrate, .nadapt, .ε0bar, .h0bar, .γ, .t0, .κ, .period, .verbose   tuners/DualAveragingMCTuner.jl:54-93
#   BasicMCRange.burnin, .thinning, .nsteps, .postrange, .npoststeps     ranges/BasicMCRange.jl:7-36
# v0[key]: a D x N matrix of starts (column = chain), or one vector — BasicMCJob's form (README.md:47 `Dict(:p=>[5.1, -0.9])`) — that every one of
# `nchains` chains starts from
startmatrix(x::Matrix{Float64}, nchains::Integer) = x
function startmatrix(x::AbstractVector, nchains::Integer)
    X = newarray(Float64, length(x), Int(nchains))
    for j in 1:Int(nchains), i in 1:length(x)
        X[i, j] = x[i]
    end
    X
end
startmatrix(x, nchains::Integer) = convert(Matrix{Float64}, x)

# BasicMCJob(model, sampler, range, v0; tuner, outopts) (jobs/BasicMCJob.jl:140-185): the parameter is the model's first Parameter vertex
# (`pindex`, :144) and v0 is keyed by the variables' keys (:156-158)
function firstparameter(vs)               # BasicMCJob.jl:144 `findfirst(v -> isa(v, Parameter), model.vertices)` (findfirst's "none" differs between 0.6 and 0.7)
    for i in 1:length(vs)
        isa(vs[i], Parameter) && return i
    end
    error("the model has no Parameter vertex")
end
function HIPMCJob(model::GenericModel, sampler, mcrange, v0::Dict;
                  pindex::Integer=firstparameter(model.vertices), kwargs...)
    parameter = model.vertices[pindex]
    isa(parameter, HIPParameter) || error("the model's parameter must be a HIPParameter (a device target family), got $(typeof(parameter))")
    HIPMCJob(parameter, sampler, mcrange, v0; kwargs...)
end

function HIPMCJob(parameter::HIPParameter, sampler, mcrange, v0::Dict;
                  tuner=nothing, outopts::Dict=Dict{Symbol, Any}(), pooled::Bool=false, nchains::Integer=1,
                  seed::Integer=rand(UInt64), chain_offset::Integer=0, device::Integer=0, steps_per_launch::Integer=0,
                  summaries::Bool=true, bm_batchlen::Integer=0, covariance::Bool=false, marginals=nothing, derived=nothing)
    X0 = startmatrix(v0[parameter.key], nchains)                          # D x N: column = chain == N x D row-major
    D, N = size(X0)
    t = parameter.target
    D == ndims_of(t) || error("v0 has the wrong number of dimensions for the target")
    keep = Any[X0]
    kw = Dict{Symbol, Any}(:nchains => N, :ndims => D, :chain_offset => chain_offset, :device => device, :seed => UInt64(seed),
                           :steps_per_launch => steps_per_launch, :bm_batchlen => bm_batchlen,
                           :nsteps => mcrange.nsteps, :burnin => mcrange.burnin, :thinning => mcrange.thinning)
    # --- sampler
    if isa(sampler, SMMALA)                                 # samplers/SMMALA.jl:127-137; the metric is the target's (LogisticTarget, or a CustomTarget's tensor)
        tr = sampler.transform                              # nothing, or SoftAbs(a): softabs(G, a) of every metric on the device (CustomTarget only)
        (tr === nothing || isa(tr, SoftAbs)) || error("SMMALA: the only transform of the metric that runs on the device is SoftAbs(a), as in SMMALA(1.25, SoftAbs(1000.)); a closure cannot be recognised")
        kw[:sampler] = SAMPLER_SMMALA; kw[:driftstep] = Float64(sampler.driftstep)
        kw[:smmala_softabs] = tr === nothing ? 0.0 : tr.a
    elseif isa(sampler, RAM)                                # samplers/RAM.jl:94-111: the initial factor (lower triangular), target rate and exponent
        S0 = rowmajor(convert(Matrix{Float64}, sampler.S0)); push!(keep, S0)
        size(S0) == (D, D) || error("RAM: S0 must be D x D")
        kw[:sampler] = SAMPLER_RAM; kw[:ram_S0] = pointer(S0)
        kw[:ram_targetrate] = Float64(sampler.targetrate); kw[:ram_gamma] = Float64(sampler.γ)
    elseif isa(sampler, AM)                                 # samplers/AM.jl:131-136: the initial covariance (symmetric), the two scalings, the weight and t0
        C0 = rowmajor(convert(Matrix{Float64}, sampler.C0)); push!(keep, C0)
        size(C0) == (D, D) || error("AM: C0 must be D x D")
        kw[:sampler] = SAMPLER_AM; kw[:am_C0] = pointer(C0)
        kw[:am_corescale] = Float64(sampler.corescale); kw[:am_minorscale] = Float64(sampler.minorscale)
        kw[:am_c] = Float64(sampler.c); kw[:am_t0] = Int64(sampler.t0)
    elseif isa(sampler, MuvAMWG)                            # samplers/AMWG.jl:139-151: logσ0; the truncated proposals of finite bounds are not built (W5)
        all(isinf, sampler.lower) || error("MuvAMWG: a finite `lower` bound asks for the truncated-normal proposal (iterate/AMWG.jl:100-115), which is not built on the device")
        all(isinf, sampler.upper) || error("MuvAMWG: a finite `upper` bound asks for the truncated-normal proposal (iterate/AMWG.jl:100-115), which is not built on the device")
        ls0 = convert(Vector{Float64}, sampler.logσ0); push!(keep, ls0)
        length(ls0) == D || error("MuvAMWG: σ must have one entry per dimension")
        kw[:sampler] = SAMPLER_AMWG; kw[:amwg_logsigma0] = pointer(ls0)
    elseif isa(sampler, MALA)
        kw[:sampler] = SAMPLER_MALA; kw[:driftstep] = Float64(sampler.driftstep)
    elseif isa(sampler, HMC)
        kw[:sampler] = SAMPLER_HMC; kw[:leapstep] = Float64(sampler.leapstep); kw[:nleaps] = Int32(sampler.nleaps)
    elseif isa(sampler, SliceSampler)
        w = convert(Vector{Float64}, sampler.widths); push!(keep, w)
        length(w) == D || error("SliceSampler widths must have one entry per dimension")
        kw[:sampler] = SAMPLER_SLICE; kw[:slice_widths] = pointer(w); kw[:slice_stepout] = Int32(sampler.stepout)
    elseif isa(sampler, MH)
        (sampler.symmetric && sampler.normalised) || error("only the symmetric normalised random-walk MH(sigma) runs on the device (iterate/MH.jl:72-124)")
        prop = sampler.setproposal(BasicContMuvParameterState(zeros(D)))    # MvNormal(x, sigma) or MvNormal(x, Σ): its covariance says which (MH.jl:63-66)
        Sigma = convert(Matrix{Float64}, Distributions.cov(prop))
        if all(i == j || Sigma[i, j] == 0 for i in 1:D, j in 1:D)           # diagonal: MH(sigma), the variances give sigma
            sig = sqrt.(Distributions.var(prop)); push!(keep, sig)
            kw[:sampler] = SAMPLER_MH; kw[:mh_sigma] = pointer(sig)
        else                                                                # MH(Σ): the lower factor, Σ = L L'; off-diagonals are never dropped
            Lf = rowmajor(lowerfactor(Sigma)); push!(keep, Lf)
            kw[:sampler] = SAMPLER_MH_COV; kw[:mh_factor] = pointer(Lf)
        end
    else
        error("sampler $(typeof(sampler)) is not on the device path (MH with a vector or a matrix, RAM, AM, MuvAMWG, MALA, SMMALA, HMC, SliceSampler are)")
    end
    # --- tuner
    tn = tuner === nothing ? (isa(sampler, MuvAMWG) ? RobertsRosenthalMCTuner() : VanillaMCTuner()) : tuner
    isa(sampler, MuvAMWG) == isa(tn, RobertsRosenthalMCTuner) || error("MuvAMWG and RobertsRosenthalMCTuner go together, and with nothing else (AMWG.jl:165-170)")
    kw[:period] = Int32(tn.period); kw[:verbose] = Int32(tn.verbose)
    if isa(tn, VanillaMCTuner)
        kw[:tuner] = TUNER_VANILLA
    elseif isa(tn, AcceptanceRateMCTuner)
        kw[:tuner] = TUNER_ACCEPT_RATE; kw[:targetrate] = Float64(tn.targetrate)
        kw[:tuner_mode] = pooled ? TUNE_POOLED : TUNE_PER_CHAIN
        # tuner.score is a function: logistic_rate_score (k = 7) and erf_rate_score (k = 3) are the two Klara ships
        if tn.score === erf_rate_score
            kw[:tuner_score] = Int32(1); kw[:score_k] = 3.0
        elseif tn.score === logistic_rate_score
            kw[:tuner_score] = Int32(0); kw[:score_k] = 7.0
        else
            error("AcceptanceRateMCTuner score must be logistic_rate_score or erf_rate_score on the device")
        end
    elseif isa(tn, RobertsRosenthalMCTuner)                 # tuners/RobertsRosenthalMCTuner.jl:84-97: target rate and period; per chain and coordinate
        kw[:tuner] = TUNER_ROBERTS_ROSENTHAL; kw[:targetrate] = Float64(tn.targetrate)
    elseif isa(tn, DualAveragingMCTuner)
        isa(sampler, HMC) || error("DualAveragingMCTuner is wired into HMC only (HMC.jl:124-133)")
        kw[:tuner] = TUNER_DUAL_AVERAGING; kw[:targetrate] = Float64(tn.targetrate); kw[:da_nadapt] = Int64(tn.nadapt)
        kw[:da_eps0bar] = Float64(tn.ε0bar); kw[:da_h0bar] = Float64(tn.h0bar); kw[:da_gamma] = Float64(tn.γ)
        kw[:da_t0] = Int32(tn.t0); kw[:da_kappa] = Float64(tn.κ)
    else
        error("tuner $(typeof(tn)) is not on the device path")
    end
    # --- target
    if isa(t, GaussDiagTarget)
        kw[:target] = TARGET_GAUSS_DIAG; kw[:gauss_const] = t.c
        if !isempty(t.w); push!(keep, t.w); kw[:gauss_w] = pointer(t.w); end
        if !isempty(t.mu); push!(keep, t.mu); kw[:gauss_mu] = pointer(t.mu); end
    elseif isa(t, GaussDenseTarget)
        P = rowmajor(t.P); push!(keep, P)
        kw[:target] = TARGET_GAUSS_DENSE; kw[:gauss_prec] = pointer(P); kw[:gauss_const] = t.c
        if !isempty(t.mu); push!(keep, t.mu); kw[:gauss_mu] = pointer(t.mu); end
    elseif isa(t, LogisticTarget)
        X = rowmajor(t.X); push!(keep, X); push!(keep, t.y)
        kw[:target] = TARGET_LOGISTIC; kw[:logit_X] = pointer(X); kw[:logit_y] = pointer(t.y)
        kw[:logit_ndata] = Int32(size(t.X, 1)); kw[:logit_lambda] = t.lambda
    elseif isa(t, HierNormalTarget)
        Y = rowmajor(t.Y); push!(keep, Y); push!(keep, t.xc)
        kw[:target] = TARGET_HIER_NORMAL; kw[:hier_Y] = pointer(Y); kw[:hier_xc] = pointer(t.xc)
        kw[:hier_nunits] = Int32(size(t.Y, 1)); kw[:hier_ntimes] = Int32(size(t.Y, 2))
        kw[:hier_prior_prec] = t.prior_prec; kw[:hier_gamma_a] = t.gamma_a; kw[:hier_gamma_b] = t.gamma_b
    else
        push!(keep, t.src)
        kw[:target] = TARGET_CUSTOM; kw[:custom_src] = Base.unsafe_convert(Cstring, t.src)
        if !isempty(t.data); push!(keep, t.data); kw[:custom_data] = pointer(t.data); kw[:custom_ndata] = length(t.data); end
    end
    # --- outopts (jobs.jl:9-43): destination, monitor, diagnostics
    oo = Dict{Symbol, Any}(outopts)
    get!(oo, :destination, :nstate)
    if oo[:destination] != :none
        get!(oo, :monitor, [:value]); get!(oo, :diagnostics, Symbol[])
    end
    mon = UInt32(summaries ? MON_SUMMARIES : 0x00)
    if covariance; mon |= MON_COVARIANCE; end                             # D <= 256; the chains are the same bits with and without it
    if :accept in get(oo, :diagnostics, Symbol[]); mon |= MON_ACCEPT; end
    for m in get(oo, :monitor, Symbol[])
        m == :value && (mon |= MON_HISTORY)
        m == :logtarget && (mon |= MON_HIST_LT)
        m == :gradlogtarget && (mon |= MON_HIST_GRAD)
        (m == :loglikelihood || m == :logprior) && (mon |= MON_HIST_LLLP)
    end
    kw[:monitor] = mon
    if marginals !== nothing                                              # (nbins, lo, hi): the pooled marginal histograms; lo, hi scalars or D values
        nb, mlo, mhi = marginals
        vlo = isa(mlo, Number) ? fill(Float64(mlo), D) : convert(Vector{Float64}, mlo)
        vhi = isa(mhi, Number) ? fill(Float64(mhi), D) : convert(Vector{Float64}, mhi)
        (length(vlo) == D && length(vhi) == D) || error("marginals: lo and hi must be scalars or have one entry per dimension")
        push!(keep, vlo); push!(keep, vhi)
        kw[:marg_lo] = pointer(vlo); kw[:marg_hi] = pointer(vhi); kw[:marg_nbins] = Int64(nb)
        oo[:marginals] = (Int64(nb), vlo, vhi)
    end
    if derived !== nothing                                                # Derived(nout, src; data, marginals): a function of the state, summed per chain
        isa(derived, Derived) || error("derived= takes a Derived(nout, src; data, marginals)")
        push!(keep, derived.src); push!(keep, derived.data)
        kw[:derived_src] = Base.unsafe_convert(Cstring, derived.src); kw[:derived_nout] = Int64(derived.nout)
        if length(derived.data) > 0
            kw[:derived_data] = pointer(derived.data); kw[:derived_ndata] = Int64(length(derived.data))
        end
        dmarg = nothing
        if derived.marginals !== nothing
            dnb, dlo, dhi = derived.marginals
            wlo = isa(dlo, Number) ? fill(Float64(dlo), derived.nout) : convert(Vector{Float64}, dlo)
            whi = isa(dhi, Number) ? fill(Float64(dhi), derived.nout) : convert(Vector{Float64}, dhi)
            (length(wlo) == derived.nout && length(whi) == derived.nout) || error("derived marginals: lo and hi must be scalars or have one entry per output")
            push!(keep, wlo); push!(keep, whi)
            kw[:derived_lo] = pointer(wlo); kw[:derived_hi] = pointer(whi); kw[:derived_nbins] = Int64(dnb)
            dmarg = (Int64(dnb), wlo, whi)
        end
        oo[:derived] = (derived.nout, dmarg)
    end
    desc = klara_desc(; kw...)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:klara_create, lib), Cint, (Ref{KlaraDesc}, Ref{Ptr{Cvoid}}), desc, h), "klara_create")
    job = HIPMCJob(h[], N, D, parameter, sampler, tn, mcrange, oo, mon, keep)
    on_finalize(job, j -> ccall((:klara_destroy, lib), Cint, (Ptr{Cvoid},), j.handle))
    # initialize!(pstate, parameter, sampler, outopts): BasicMCJob.jl:73 (finiteness asserts on device)
    check(ccall((:klara_set_state, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), job.handle, X0), "klara_set_state")
    job
end

# raw form for callers that fill the descriptor themselves
function HIPMCJob(desc::KlaraDesc, X0::Matrix{Float64}, range)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:klara_create, lib), Cint, (Ref{KlaraDesc}, Ref{Ptr{Cvoid}}), desc, h), "klara_create")
    job = HIPMCJob(h[], size(X0, 2), size(X0, 1), HIPParameter(:p, GaussDiagTarget(size(X0, 1))), nothing, nothing, range,
                   Dict{Symbol, Any}(), desc.monitor, Any[X0])
    on_finalize(job, j -> ccall((:klara_destroy, lib), Cint, (Ptr{Cvoid},), j.handle))
    check(ccall((:klara_set_state, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), job.handle, X0), "klara_set_state")
    job
end

# ramfactor(job): (S, skipped) of a RAM job — S[:, :, c] is chain c's current lower-triangular factor (sstate.S of iterate/RAM.jl:129), skipped the
# number of factor updates the device left out because a pivot was not a finite positive number (0 in exact arithmetic)
function ramfactor(job::HIPMCJob)
    St = newarray(Float64, job.ndims, job.ndims, job.nchains)       # row-major D x D per chain == the transposes, column-major
    skipped = Ref{Clonglong}(0)
    check(ccall((:klara_get_ram_factor, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Clonglong}), job.handle, St, skipped), "klara_get_ram_factor")
    (permutedims(St, (2, 1, 3)), Int(skipped[]))
end

# run / reset: methods of Base.run / Base.reset — the generics Klara itself extends (src/Klara.jl:26-27; imported above)
run(job::HIPMCJob) =                                     # BasicMCJob.jl:212-244 for all chains
    check(ccall((:klara_run, lib), Cint, (Ptr{Cvoid}, Clonglong), job.handle, job.range.nsteps), "klara_run")

reset(job::HIPMCJob) =                                   # BasicMCJob.jl:187-195; the job moves to its next Philox key (klara_hip.h)
    check(ccall((:klara_reset, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), job.handle, C_NULL), "klara_reset")
reset(job::HIPMCJob, X::Matrix{Float64}) =               # BasicMCJob.jl:197-201 reset(job, x): new initial values (D x N, one column per chain)
    check(ccall((:klara_reset, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), job.handle, X), "klara_reset")
reset(job::HIPMCJob, x::AbstractVector) =                # README.md:68 `reset(job, [3.2, 9.4])`: every chain restarts from x
    reset(job, startmatrix(x, job.nchains))

function show(io::IO, job::HIPMCJob)                     # BasicMCJob.jl:281-295 prints parameter, model, sampler, tuner, range
    println(io, "HIPMCJob: ", job.nchains, " chains of ", job.ndims, " dimensions on libklara_hip")
    print(io, "  "); show(io, job.parameter.target)
    print(io, "\n  "); show(io, job.sampler)
    print(io, "\n  "); show(io, job.tuner)
    print(io, "\n  "); show(io, job.range)
end

# mhfactor(job): the lower factor L of an MH(Σ) job's proposal covariance as it stands, Σ = L L' (the job's own, or what setmhfactor! gave)
function mhfactor(job::HIPMCJob)
    Lt = newarray(Float64, job.ndims, job.ndims)                    # row-major D x D == the transpose, column-major
    check(ccall((:klara_get_mh_factor, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), job.handle, Lt), "klara_get_mh_factor")
    collect(transpose(Lt))
end

# setmhfactor!(job, L): a new lower factor for an MH(Σ) job, in effect from the next transition — an adaptation step, which belongs before the samples that
# are kept; reset(job) puts the job's own factor back
function setmhfactor!(job::HIPMCJob, Lf::Matrix{Float64})
    size(Lf) == (job.ndims, job.ndims) || error("setmhfactor!: the factor must be D x D")
    check(ccall((:klara_set_mh_factor, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), job.handle, rowmajor(Lf)), "klara_set_mh_factor")
    job
end

# amstate(job): (C, lastmean, secondlastmean, fallbacks) of an AM job — C[:, :, c] is chain c's current covariance (sstate.C of iterate/AM.jl:87-91),
# lastmean[:, c] and secondlastmean[:, c] its running means (:134-135), fallbacks the number of transitions at which corescale * C did not factor and the
# chain proposed from the stabilising component instead
function amstate(job::HIPMCJob)
    Cm = newarray(Float64, job.ndims, job.ndims, job.nchains)       # symmetric: row-major == column-major
    m = newarray(Float64, job.ndims, job.nchains)
    m2 = newarray(Float64, job.ndims, job.nchains)
    fallbacks = Ref{Clonglong}(0)
    check(ccall((:klara_get_am_state, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Clonglong}), job.handle, Cm, m, m2, fallbacks),
          "klara_get_am_state")
    (Cm, m, m2, Int(fallbacks[]))
end

# amwgstate(job): (logσ, accepted, naccept) of a MuvAMWG job — logσ[:, c] is chain c's current log proposal scales (tune.logσ of iterate/AMWG.jl:96),
# accepted[:, c] the accepted proposals of its current tuning window per coordinate (tune.accepted), naccept[:, c] those since the start state
function amwgstate(job::HIPMCJob)
    ls = newarray(Float64, job.ndims, job.nchains)                  # nchains x D row-major == D x nchains column-major
    acc = newarray(Int32, job.ndims, job.nchains)
    nacc = newarray(UInt64, job.ndims, job.nchains)
    check(ccall((:klara_get_amwg_state, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{UInt64}), job.handle, ls, acc, nacc), "klara_get_amwg_state")
    (ls, acc, nacc)
end

# value matrix of chain c exactly as BasicContMuvParameterNState.value (D x npoststeps)
function chainvalue(job::HIPMCJob, c::Integer)
    n = Ref{Clonglong}(0)
    ccall((:klara_get_chain, lib), Cint, (Ptr{Cvoid}, Clonglong, Ptr{Float64}, Clonglong, Ref{Clonglong}),
          job.handle, c - 1, C_NULL, 0, n)
    v = newarray(Float64, job.ndims, n[])
    check(ccall((:klara_get_chain, lib), Cint, (Ptr{Cvoid}, Clonglong, Ptr{Float64}, Clonglong, Ref{Clonglong}),
                job.handle, c - 1, v, n[], n), "klara_get_chain")
    v
end

# output(job, c): a method of Klara.output (imported above) — the BasicContMuvParameterNState of chain c (BasicMCJob.jl:279; nstates/ParameterNStates/
# BasicContMuvParameterNState.jl:23-61: fields value, loglikelihood, logprior, logtarget, gradloglikelihood, gradlogprior,
# gradlogtarget, ..., diagnosticvalues, size, monitor, n, diagnostickeys) filled from the device history
function output(job::HIPMCJob, c::Integer=1)
    n = job.range.npoststeps
    monitor = fill(false, 13)
    monitor[1] = (job.monitor & MON_HISTORY) != 0           # value
    monitor[2] = monitor[3] = (job.monitor & MON_HIST_LLLP) != 0   # loglikelihood, logprior
    monitor[4] = (job.monitor & MON_HIST_LT) != 0           # logtarget
    monitor[7] = (job.monitor & MON_HIST_GRAD) != 0         # gradlogtarget
    dkeys = (job.monitor & MON_ACCEPT) != 0 ? [:accept] : Symbol[]
    ns = BasicContMuvParameterNState(job.ndims, n, monitor, dkeys)
    if monitor[1]; ns.value = chainvalue(job, c); end
    nc = Ref{Clonglong}(0)
    if monitor[4] || monitor[7]
        check(ccall((:klara_get_chain_fields, lib), Cint, (Ptr{Cvoid}, Clonglong, Ptr{Float64}, Ptr{Float64}, Clonglong, Ref{Clonglong}),
                    job.handle, c - 1, monitor[4] ? ns.logtarget : C_NULL, monitor[7] ? ns.gradlogtarget : C_NULL, n, nc), "klara_get_chain_fields")
    end
    if monitor[2]
        check(ccall((:klara_get_chain_likelihood_prior, lib), Cint, (Ptr{Cvoid}, Clonglong, Ptr{Float64}, Ptr{Float64}, Clonglong, Ref{Clonglong}),
                    job.handle, c - 1, ns.loglikelihood, ns.logprior, n, nc), "klara_get_chain_likelihood_prior")
    end
    if !isempty(dkeys)                                      # diagnosticvalues[1, i] = accept flag of saved step i (iterate/MALA.jl:112-117)
        nst = Ref{Clonglong}(0)
        ccall((:klara_get_accept_mask, lib), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Clonglong, Ref{Clonglong}), job.handle, C_NULL, 0, nst)
        mask = newarray(UInt8, job.nchains, nst[])     # step-major rows of nchains bytes == column = step
        check(ccall((:klara_get_accept_mask, lib), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Clonglong, Ref{Clonglong}), job.handle, mask, nst[], nst), "klara_get_accept_mask")
        for (i, step) in enumerate(job.range.postrange)
            step <= nst[] && (ns.diagnosticvalues[1, i] = mask[c, step] != 0)
        end
    end
    ns
end

# mean(chain) for every chain from the on-device running sums (stats/mean.jl:7-11): D x N
function chainmeans(job::HIPMCJob)
    s = newarray(Float64, job.ndims, job.nchains); q = similar(s); n = Ref{Clonglong}(0)
    check(ccall((:klara_get_chain_sums, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{Clonglong}),
                job.handle, s, q, n), "klara_get_chain_sums")
    s ./ n[]
end
# acceptance rate of every chain over all transitions (stats/acceptance.jl:28-34 counts the saved steps' diagnostics)
function chainacceptance(job::HIPMCJob)
    a = newarray(UInt64, job.nchains); nst = Ref{UInt64}(0)
    check(ccall((:klara_get_accept_counts, lib), Cint, (Ptr{Cvoid}, Ptr{UInt64}, Ref{UInt64}), job.handle, a, nst), "klara_get_accept_counts")
    a ./ Float64(nst[])
end
# mcvar(chain, Val{:bm}) for every chain and dimension from the streaming batch means (bm_batchlen > 0): D x N, nbatches
function chainmcvar_bm(job::HIPMCJob)
    v = newarray(Float64, job.ndims, job.nchains); nb = Ref{Clonglong}(0)
    check(ccall((:klara_get_chain_bm, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Clonglong}), job.handle, v, nb), "klara_get_chain_bm")
    (v, nb[])
end
# Zero-variance control variates of EVERY chain on the device (klara_get_chain_zv; stats/variance/zv.jl:16-34, 50-80), from the stored value and
# gradlogtarget (outopts :monitor => [:value, :gradlogtarget]): (mean of chain + f a: D x N, its sample variance: D x N, coefficients, info).
# The coefficients come as the C ABI lays them out, a[i, k, c] = zv.jl's a[k, i] of chain c (D x K x N; pooled=true: one D x K matrix fitted to
# all chains' samples together); info[c] is 0, 1 (singular) or 2 (fewer than K + 2 samples) — such a chain's columns are NaN.
# Klara's own lzv / qzv are NOT redefined here: `lzv(output(job, c))` runs the reference's code on one chain's NState.
function chainzv(job::HIPMCJob, order::Integer, pooled::Bool)
    d = job.ndims
    k = order == 1 ? d : div(d * (d + 3), 2)
    a = pooled ? newarray(Float64, d, k) : newarray(Float64, d, k, job.nchains)
    m = newarray(Float64, d, job.nchains); v = similar(m); info = newarray(Int32, job.nchains); n = Ref{Clonglong}(0)
    check(ccall((:klara_get_chain_zv, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{Clonglong}),
                job.handle, order, pooled ? 1 : 0, a, m, v, info, n), "klara_get_chain_zv")
    (m, v, a, info)
end
function chainlzv(job::HIPMCJob; pooled=false)
    chainzv(job, 1, pooled)
end
function chainqzv(job::HIPMCJob; pooled=false)
    chainzv(job, 2, pooled)
end
# the Philox key the job draws from and the number of resets so far (klara_hip.h klara_reset)
function streamkey(job::HIPMCJob)
    k = Ref{UInt64}(0); e = Ref{UInt64}(0)
    check(ccall((:klara_stream_key, lib), Cint, (Ptr{Cvoid}, Ref{UInt64}, Ref{UInt64}), job.handle, k, e), "klara_stream_key")
    (k[], e[])
end

# how the launches were issued so far (klara_get_launch_modes): (4-lane kernel alone, 8-lane kernel alone, device-decided pair), and per
# chain partition the last decision (0: 4 lanes, 1: 8 lanes) and the accepted proposals of the launch that took it
function launchmodes(job::HIPMCJob)
    counts = newarray(Int64, 3); lastmode = newarray(Int32, 4); lastaccepted = newarray(Int64, 4)
    check(ccall((:klara_get_launch_modes, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}), job.handle, counts, lastmode, lastaccepted),
          "klara_get_launch_modes")
    (counts, lastmode, lastaccepted)
end

# shader clock (MHz) during the job's last launch of a pair-transposed kernel (an in-kernel probe, klara_get_shader_clock); 0.0 when unknown
function shaderclock(job::HIPMCJob)
    mhz = newarray(Float64, 1)
    check(ccall((:klara_get_shader_clock, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), job.handle, mhz), "klara_get_shader_clock")
    mhz[1]
end

# user-defined target: compile the closures' C text without a GPU; the compiler's message on failure
function check_custom_target(src::String, sampler::Integer, ndims::Integer)
    st = ccall((:klara_check_custom_target, lib), Cint, (Cstring, Cint, Cint), src, sampler, ndims)
    st == 0 || error(unsafe_string(ccall((:klara_compile_log, lib), Cstring, ())))
    true
end

# ... and for the SMMALA kernels with the softabs transform of the metric (SMMALA(h, SoftAbs(a)))
function check_custom_target_softabs(src::String, ndims::Integer)
    st = ccall((:klara_check_custom_target_softabs, lib), Cint, (Cstring, Cint), src, ndims)
    st == 0 || error(unsafe_string(ccall((:klara_compile_log, lib), Cstring, ())))
    true
end

# ---- multi-GPU: one process per GPU; the only exchange is the all-reduce of the pooled summaries (RCCL over xGMI)
mutable struct HIPComm; handle::Ptr{Cvoid}; end
function comm_unique_id()
    id = newarray(UInt8, 128)
    check(ccall((:klara_comm_unique_id, lib), Cint, (Ptr{UInt8},), id), "klara_comm_unique_id")
    id
end
function HIPComm(nranks::Integer, rank::Integer, id::Vector{UInt8}, device::Integer)
    c = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:klara_comm_init, lib), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Ptr{UInt8}, Cint), c, nranks, rank, id, device), "klara_comm_init")
    comm = HIPComm(c[])
    on_finalize(comm, x -> ccall((:klara_comm_destroy, lib), Cint, (Ptr{Cvoid},), x.handle))
    comm
end
# (ranks, this rank, device) as the communicator itself reports them (ncclCommCount / ncclCommUserRank)
function comm_info(comm::HIPComm)
    n = Ref{Cint}(0); r = Ref{Cint}(0); d = Ref{Cint}(0)
    check(ccall((:klara_comm_info, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cint}), comm.handle, n, r, d), "klara_comm_info")
    (Int(n[]), Int(r[]), Int(d[]))
end
# (sum x, sum x^2 per dimension over every chain of every GPU, accepted, transitions, saved samples, chains)
function gather_summaries(job::HIPMCJob, comm::HIPComm)
    s = newarray(Float64, job.ndims); q = similar(s)
    na = Ref{UInt64}(0); nt = Ref{UInt64}(0); ns = Ref{UInt64}(0); nc = Ref{UInt64}(0)
    check(ccall((:klara_gather_summaries, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{UInt64}, Ref{UInt64}, Ref{UInt64}, Ref{UInt64}),
                job.handle, comm.handle, s, q, na, nt, ns, nc), "klara_gather_summaries")
    (s, q, na[], nt[], ns[], nc[])
end
# The pooled posterior moments over every chain of every GPU without the cancellation of sumsq/n - mean^2 (klara_gather_moments:
# per-chain (n, mean, M2) on the device, Chan's merge over chains, blocks and ranks): (mean, var, nsamples, accepted, transitions, chains)
function gather_moments(job::HIPMCJob, comm::HIPComm)
    m = newarray(Float64, job.ndims); m2 = similar(m)
    ns = Ref{UInt64}(0); na = Ref{UInt64}(0); nt = Ref{UInt64}(0); nc = Ref{UInt64}(0)
    check(ccall((:klara_gather_moments, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{UInt64}, Ref{UInt64}, Ref{UInt64}, Ref{UInt64}),
                job.handle, comm.handle, m, m2, ns, na, nt, nc), "klara_gather_moments")
    (m, m2 ./ Float64(ns[]), ns[], na[], nt[], nc[])
end
# ... and of this job's chains alone (no communicator, no RCCL)
function pooledmoments(job::HIPMCJob)
    m = newarray(Float64, job.ndims); m2 = similar(m)
    ns = Ref{UInt64}(0); na = Ref{UInt64}(0); nt = Ref{UInt64}(0); nc = Ref{UInt64}(0)
    check(ccall((:klara_gather_moments, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{UInt64}, Ref{UInt64}, Ref{UInt64}, Ref{UInt64}),
                job.handle, C_NULL, m, m2, ns, na, nt, nc), "klara_gather_moments")
    (m, m2 ./ Float64(ns[]), ns[], na[], nt[], nc[])
end
# The pooled posterior covariance of a job built with covariance=true (klara_gather_covariance: M = sum (x - mean)(x - mean)' over all chains and saved
# steps, accumulated while sampling on the FP64 matrix cores; no history is stored): (mean, cov = M / (n - 1), nsamples, chains) over every chain of
# every GPU.  (Klara's own covariance! is the in-place sample covariance of ONE stored chain: another function.)
function gather_covariance(job::HIPMCJob, comm::HIPComm)
    m = newarray(Float64, job.ndims); m2 = newarray(Float64, job.ndims * job.ndims)
    ns = Ref{UInt64}(0); nc = Ref{UInt64}(0)
    check(ccall((:klara_gather_covariance, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{UInt64}, Ref{UInt64}),
                job.handle, comm.handle, m, m2, ns, nc), "klara_gather_covariance")
    (m, reshape(m2, job.ndims, job.ndims) ./ (Float64(ns[]) - 1.0), ns[], nc[])       # (symmetric: row-major == column-major)
end
# ... and of this job's chains alone (no communicator, no RCCL)
function pooledcovariance(job::HIPMCJob)
    m = newarray(Float64, job.ndims); m2 = newarray(Float64, job.ndims * job.ndims)
    ns = Ref{UInt64}(0); nc = Ref{UInt64}(0)
    check(ccall((:klara_gather_covariance, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{UInt64}, Ref{UInt64}),
                job.handle, C_NULL, m, m2, ns, nc), "klara_gather_covariance")
    (m, reshape(m2, job.ndims, job.ndims) ./ (Float64(ns[]) - 1.0), ns[], nc[])
end
# the (nbins, lo, hi) a job was built with, the documented edges, and the one call behind pooledhistogram / gather_histogram (comm: a communicator's handle or C_NULL)
function marginals_of(job::HIPMCJob)
    haskey(job.outopts, :marginals) || error("the job was built without marginals=(nbins, lo, hi)")
    job.outopts[:marginals]
end
function histogram_edges(nb, lo, hi)
    Float64[lo[d] + k * ((hi[d] - lo[d]) / nb) for k in 0:nb, d in 1:length(lo)]
end
function histogram_of(job::HIPMCJob, comm::Ptr{Cvoid})
    nb, lo, hi = marginals_of(job)
    counts = zeros(UInt64, nb + 2, job.ndims)
    ns = Ref{UInt64}(0); nc = Ref{UInt64}(0)
    check(ccall((:klara_gather_histogram, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt64}, Ref{UInt64}, Ref{UInt64}),
                job.handle, comm, counts, ns, nc), "klara_gather_histogram")
    (counts, histogram_edges(nb, lo, hi), ns[], nc[])
end
# The pooled marginal histograms of a job built with marginals=(nbins, lo, hi) (klara_gather_histogram): per dimension, the saved samples of all chains
# counted after every launch into nbins equal bins over [lo, hi) plus an underflow and an overflow slot; no history is stored.  (counts, edges, nsamples,
# chains): counts is (nbins + 2) x D (column d = dimension d: the C table's rows), edges (nbins + 1) x D with edges[k + 1, d] = lo[d] + k (hi[d] - lo[d]) / nbins
# — documentation: the index formula of include/klara_hip.h is the contract.  Over every chain of every GPU (the ranks' jobs built with the same marginals):
gather_histogram(job::HIPMCJob, comm::HIPComm) = histogram_of(job, comm.handle)
# ... and of this job's chains alone (no communicator, no RCCL)
pooledhistogram(job::HIPMCJob) = histogram_of(job, Ptr{Cvoid}(C_NULL))
# Quantiles from those counts (klara_histogram_quantiles, host code): length(probs) x D, probs in (0, 1]; -Inf / Inf where the order statistic lies outside
# [lo, hi) — a range chosen badly is never clipped silently —, NaN before the first saved sample
function pooledquantiles(job::HIPMCJob, probs)
    nb, lo, hi = marginals_of(job)
    quantiles_of(pooledhistogram(job)[1], nb, lo, hi, probs)
end
# ... the one call behind pooledquantiles and derivedquantiles: counts (nbins + 2) x W, lo and hi W each
function quantiles_of(counts::Matrix{UInt64}, nb, lo, hi, probs)
    W = size(counts, 2)
    p = convert(Vector{Float64}, collect(probs))
    out = newarray(Float64, length(p), W)
    check(ccall((:klara_histogram_quantiles, lib), Cint,
                (Ptr{UInt64}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                counts, Int32(W), Int64(nb), lo, hi, Int32(length(p)), p, out), "klara_histogram_quantiles")
    out
end
# ---- derived quantities: a job built with derived=Derived(nout, src; data, marginals).  (nout, marginals) of the job, then the calls; comm: a communicator's
# handle or C_NULL (this job's chains alone)
function derived_of(job::HIPMCJob)
    haskey(job.outopts, :derived) || error("the job was built without derived=Derived(nout, src)")
    job.outopts[:derived]
end
# (sum, sumsq, nsaved): every chain's running sums of the closure's outputs and of their squares, nout x nchains (column c = chain c: the C arrays' rows)
function derivedsums(job::HIPMCJob)
    K = derived_of(job)[1]
    s = newarray(Float64, K, job.nchains); q = similar(s); n = Ref{Int64}(0)
    check(ccall((:klara_get_derived_sums, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}), job.handle, s, q, n), "klara_get_derived_sums")
    (s, q, n[])
end
function derived_moments_of(job::HIPMCJob, comm::Ptr{Cvoid})
    K = derived_of(job)[1]
    m = newarray(Float64, K); m2 = similar(m); ns = Ref{UInt64}(0); nc = Ref{UInt64}(0)
    check(ccall((:klara_gather_derived_moments, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{UInt64}, Ref{UInt64}),
                job.handle, comm, m, m2, ns, nc), "klara_gather_derived_moments")
    (m, m2 ./ Float64(ns[]), ns[], nc[])
end
# (mean, var, nsamples, chains) of the outputs over every chain of every GPU (klara_gather_derived_moments: klara_gather_moments on the derived sums) ...
gather_derived_moments(job::HIPMCJob, comm::HIPComm) = derived_moments_of(job, comm.handle)
# ... and of this job's chains alone
derivedmoments(job::HIPMCJob) = derived_moments_of(job, Ptr{Cvoid}(C_NULL))
function derived_rhat_of(job::HIPMCJob, comm::Ptr{Cvoid})
    K = derived_of(job)[1]
    r = newarray(Float64, K); m = similar(r); w = similar(r); b = similar(r); nc = Ref{UInt64}(0); np = Ref{Int64}(0)
    check(ccall((:klara_gather_derived_rhat, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{UInt64}, Ref{Int64}),
                job.handle, comm, r, m, w, b, nc, np), "klara_gather_derived_rhat")
    (r, m, w, b, nc[], np[])
end
# R-hat of the outputs (the plain form of rhat): (rhat, mean of the chain means, wsum, bsum, chains, samples per chain)
gather_derived_rhat(job::HIPMCJob, comm::HIPComm) = derived_rhat_of(job, comm.handle)
derivedrhat(job::HIPMCJob) = derived_rhat_of(job, Ptr{Cvoid}(C_NULL))
function derived_marginals_of(job::HIPMCJob)
    dm = derived_of(job)[2]
    dm === nothing && error("the job's Derived was built without marginals=(nbins, lo, hi)")
    dm
end
function derived_histogram_of(job::HIPMCJob, comm::Ptr{Cvoid})
    K = derived_of(job)[1]
    nb, lo, hi = derived_marginals_of(job)
    counts = zeros(UInt64, nb + 2, K); ns = Ref{UInt64}(0); nc = Ref{UInt64}(0)
    check(ccall((:klara_gather_derived_histogram, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt64}, Ref{UInt64}, Ref{UInt64}),
                job.handle, comm, counts, ns, nc), "klara_gather_derived_histogram")
    (counts, histogram_edges(nb, lo, hi), ns[], nc[])
end
# the pooled histograms of the outputs, as pooledhistogram's of the coordinates: (counts (nbins + 2) x nout, edges, nsamples, chains)
gather_derived_histogram(job::HIPMCJob, comm::HIPComm) = derived_histogram_of(job, comm.handle)
derivedhistogram(job::HIPMCJob) = derived_histogram_of(job, Ptr{Cvoid}(C_NULL))
# quantiles of the outputs from those counts (klara_histogram_quantiles): length(probs) x nout
function derivedquantiles(job::HIPMCJob, probs)
    nb, lo, hi = derived_marginals_of(job)
    quantiles_of(derivedhistogram(job)[1], nb, lo, hi, probs)
end
# compile a derived-quantity closure for gfx950 as klara_create would, without a GPU; the compiler's log on failure
function check_derived(src::String, ndims::Integer, nout::Integer)
    st = ccall((:klara_check_derived, lib), Cint, (Cstring, Cint, Cint), src, ndims, nout)
    st == 0 || error(unsafe_string(ccall((:klara_compile_log, lib), Cstring, ())))
    true
end
# The Gelman–Rubin diagnostic over all chains (klara_gather_rhat; Klara has no counterpart: its job is one chain): (rhat, mean of the chain means, wsum =
# sum of the chains' M2, bsum = sum (chain mean - mean)^2, units, samples per unit).  split=false works from the running sums; split=true is the split
# form from the stored history — every chain cut into its halves [0, h) and [n - h, n), h = div(n, 2) — and the units are the half-chains.
function gather_rhat(job::HIPMCJob, comm::HIPComm; split::Bool=false)
    r = newarray(Float64, job.ndims); m = similar(r); w = similar(r); b = similar(r)
    nc = Ref{UInt64}(0); np = Ref{Int64}(0)
    check(ccall((:klara_gather_rhat, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{UInt64}, Ref{Int64}),
                job.handle, comm.handle, Int32(split), r, m, w, b, nc, np), "klara_gather_rhat")
    (r, m, w, b, nc[], np[])
end
# ... and of this job's chains alone (no communicator, no RCCL)
function rhat(job::HIPMCJob; split::Bool=false)
    r = newarray(Float64, job.ndims); m = similar(r); w = similar(r); b = similar(r)
    nc = Ref{UInt64}(0); np = Ref{Int64}(0)
    check(ccall((:klara_gather_rhat, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{UInt64}, Ref{Int64}),
                job.handle, C_NULL, Int32(split), r, m, w, b, nc, np), "klara_gather_rhat")
    (r, m, w, b, nc[], np[])
end
# The pooled (multi-chain) effective sample size over all chains (klara_gather_ess; Klara's ess is per chain, its job being one chain): the tuple
# (ess, tau, rho, mean, wsum, bsum, pairs, window_exhausted, nunits, nper, lags) — rho is ndims x (lags + 1); window_exhausted[d] says that the window
# ended before Geyer's rule did, so that ess[d] is an overestimate.  Without split and maxlag the autocovariances kept while sampling are used when the
# job has them (acov_maxlag > 0), the stored history otherwise; maxlag > 0 (<= 127) and split=true (every chain's two halves, as rhat's split form) work
# from the stored history.
const ESS_STREAMED = Int32(0); const ESS_HISTORY = Int32(1); const ESS_SPLIT = Int32(2)
function ess_call(job::HIPMCJob, comm, mode::Int32, maxlag::Integer)
    D = job.ndims
    e = newarray(Float64, D); t = similar(e); m = similar(e); w = similar(e); b = similar(e)
    rho = newarray(Float64, 128 * D); pairs = newarray(Int32, D)
    nu = Ref{UInt64}(0); np = Ref{Int64}(0); lg = Ref{Int32}(0)
    st = ccall((:klara_gather_ess, lib), Cint,
               (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32},
                Ref{UInt64}, Ref{Int64}, Ref{Int32}),
               job.handle, comm, mode, Int32(maxlag), e, t, rho, m, w, b, pairs, nu, np, lg)
    L = Int(lg[])
    r = permutedims(reshape(rho[1:D * (L + 1)], L + 1, D))             # (row-major ndims x (L + 1) on the C side)
    (st, (e, t, r, m, w, b, pairs, pairs .== (div(max(L - 1, 0), 2) + 1), nu[], np[], L))
end
function ess_modes(job::HIPMCJob, comm, split::Bool, maxlag::Integer)
    if !split && maxlag <= 0
        st, out = ess_call(job, comm, ESS_STREAMED, 0)
        st != 6 && (check(st, "klara_gather_ess"); return out)        # (KLARA_ERR_STATE: the job keeps no streamed autocovariances — every rank alike)
    end
    st, out = ess_call(job, comm, split ? ESS_SPLIT : ESS_HISTORY, maxlag)
    check(st, "klara_gather_ess")
    out
end
gather_ess(job::HIPMCJob, comm::HIPComm; split::Bool=false, maxlag::Integer=0) = ess_modes(job, comm.handle, split, maxlag)
# ... and of this job's chains alone (no communicator, no RCCL)
pooledess(job::HIPMCJob; split::Bool=false, maxlag::Integer=0) = ess_modes(job, C_NULL, split, maxlag)
end # module
