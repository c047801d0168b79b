/* klara_hip.h — C ABI of libklara_hip.so: the many-chain MCMC transition path of Klara.jl on MI355X.
 *
 * What this replaces.  Klara.jl has no FFI (it is 100 % Julia); the hot path sits behind Julia
 * multiple dispatch:
 *     run(job::BasicMCJob)                               src/jobs/BasicMCJob.jl:212-244
 *       iterate!(job, typeof(job.sampler), variate_form)  src/jobs/BasicMCJob.jl:224
 *         iterate!(::BasicMCJob, ::Type{MH|MALA|HMC|SliceSampler}, ::Type{Multivariate})
 *                                                         src/samplers/iterate/{MH,MALA,HMC,SliceSampler}.jl
 *         job.parameter.logtarget! / gradlogtarget! / uptogradlogtarget!
 *                                                         src/variables/parameters/BasicContMuvParameter.jl:174-279
 * One klara_handle stands for N independent BasicMCJobs (N chains of one model); klara_run() is the
 * `for i in 1:nsteps iterate!(...)` loop of BasicMCJob.jl:219-238 executed for all chains at once on
 * the GPU.  The Julia-side binding a maintainer would add is shown in INTEGRATION.md (ccall stubs).
 *
 * Conventions: plain C, caller-owned host buffers copied at the call, library-owned device buffers
 * inside the handle, every entry point returns klara_status (never aborts).  Matrices are row-major
 * (nchains x ndims): chain c's D-vector is contiguous — the transpose of Klara's per-chain
 * NState.value (ndims x nsaved, src/nstates/ParameterNStates/BasicContMuvParameterNState.jl:1-21);
 * klara_get_chain() returns one chain in Klara's own column-major layout.
 *
 * There is no CPU implementation behind this ABI: if no HIP device is present klara_create() fails
 * with KLARA_ERR_HIP.
 */
#ifndef KLARA_HIP_H
#define KLARA_HIP_H

#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define KLARA_ABI_VERSION 6   /* 6: Box-Muller angles at the centres of their 2^20 cells (version 5 used the left edges, which put mass 2^-19 of every
                                 normal on the coordinate axes), klara_selftest_transition_normals; same structs as 4 and 5, but a given seed draws
                                 different chains than a version-5 library.  5: one Philox block makes four normals, 44-bit accept uniform.
                                 4: klara_gather_moments, klara_desc.sparse_moves 0 = device-decided */
/* THE RANDOM STREAM IS FROZEN AT VERSION 6.  What a (seed, chain, transition) draws — the counter layout (detmath.h kd_stream_block), the
 * pair -> block-half map (kd_pair_block / kd_pair_half), the 44-bit radius / 20-bit centred angle Box-Muller (kd_normal_pair_w), the accept
 * uniform's slot ceil(D/2) and the slice sampler's slots (kd_slice_attempt_slot) — is pinned by known-answer values committed under
 * tests/golden/stream_kat.json (host build, device build and the independent NumPy restatement must all reproduce them), and the HIP
 * path is tied to the LITERAL Julia arithmetic and to the NumPy mirror on every accept decision at the BASELINE sizes
 * (tests/test_gpu_literal.py), with the joint law of a transition's normals tested in tests/test_stream_joint.py.  A change to the draw
 * schedule, to detmath.h's transforms or to the oracle's arithmetic needs those three green BEFORE and AFTER, and a new version number. */
/* klara_desc.steps_per_launch = 0 selects this many transitions per kernel launch (launches also end at the pooled tuner's
 * events and at batch boundaries of the streaming batch means, whichever comes first) */
#define KLARA_DEFAULT_STEPS_PER_LAUNCH 32
/* ... and for the slice-sampler jobs the free-running kernel serves (klara.jl_amd/csrc/klara_diagt_slice.h: the lanes run out of lockstep, a wavefront
 * waits for its slowest lane once per element slot and launch): diagonal Gaussian, 17 <= D <= 1024, untuned (VanillaMCTuner per chain, not verbose),
 * monitors among the accept diagnostics, the running sums, the value history (ring or not), the log-target history (with the values kept) and
 * the streaming autocovariances.  Ring planning and the cadence of the accept rows follow this length.  Every other slice job: 32. */
#define KLARA_DEFAULT_STEPS_PER_LAUNCH_SLICE 128
#define KLARA_LOGIT_MAX_LDS_DOUBLES 18432u   /* 144 KB of the 160 KB of LDS of a compute unit */

typedef enum klara_status {
    KLARA_OK = 0,
    KLARA_ERR_INVALID_ARG = 1,     /* mirrors the reference's @assert argument checks                */
    KLARA_ERR_NONFINITE_INIT = 2,  /* MH.jl:83 / MALA.jl:83-89 / HMC.jl:113-119: non-finite start     */
    KLARA_ERR_HIP = 3,             /* HIP runtime failure or no device                                */
    KLARA_ERR_NOMEM = 4,
    KLARA_ERR_UNSUPPORTED = 5,     /* valid Klara option that this build does not cover (see DESIGN)  */
    KLARA_ERR_STATE = 6,           /* call order (e.g. run before set_state)                          */
    KLARA_ERR_SLICE_STUCK = 7,     /* iterate/SliceSampler.jl:102 "Shrunk to current position ..." (or 16,383 step-out / shrink attempts): a chain that
                                      raised it stops at the state BEFORE the coordinate update that failed (its X and log-target belong together; the
                                      reference throws out of run(job) at that point), the job's other chains go on; reset the job */
    KLARA_ERR_COMPILE = 8          /* CUSTOM target: the user's source did not compile (klara_compile_log) */
} klara_status;

/* src/samplers/{MH,MALA,HMC,SliceSampler,SMMALA,RAM,AM,AMWG}.jl (MH twice: its vector and its matrix constructor) */
typedef enum klara_sampler {
    KLARA_SAMPLER_MH = 0,      /* MH(sigma): symmetric normal random walk, MH.jl:63-66            */
    KLARA_SAMPLER_MALA = 1,    /* MALA(driftstep), MALA.jl:61-70                                   */
    KLARA_SAMPLER_HMC = 2,     /* HMC(leapstep, nleaps), HMC.jl:89-100                             */
    KLARA_SAMPLER_SLICE = 3,   /* SliceSampler(widths, stepout), SliceSampler.jl:22-34             */
    /* SMMALA(driftstep) (transform = nothing; klara_desc.smmala_softabs for SMMALA(driftstep, H -> softabs(H, a))), SMMALA.jl:127-137: MALA with the position-dependent metric G(x) of the target —
     * for KLARA_TARGET_LOGISTIC with D <= 8 on the row-split kernels, G = X' diag(r (1 - r)) X + I / lambda
     * (doc/examples/swiss/SMMALA/analytical.jl:20-23).  Draws exactly what MALA draws (D normals and one accept uniform per
     * transition); C = L^-T with G = L L' in place of chol(inv(G))', and a proposal whose metric is not positive definite is
     * rejected.  Also KLARA_TARGET_CUSTOM in the plain whole-vector form with D <= 8, one chain per lane, whose source
     * defines KLARA_USER_FN void klara_user_tensorlogtarget(const double* x, int D, const double* data, long long ndata, double* G) (the
     * metric, row-major D x D; a source without it is KLARA_ERR_COMPILE).  Every other target (the likelihood + prior form and pair closures
     * included), and D >= 9, is KLARA_ERR_UNSUPPORTED. */
    KLARA_SAMPLER_SMMALA = 4,
    /* (5 is reserved: klara_create and klara_check_custom_target refuse it with KLARA_ERR_INVALID_ARG) */
    /* RAM(S0; targetrate, gamma), RAM.jl:94-111, iterate/RAM.jl:65-130 (Vihola 2012): the random walk x' = x + S z whose lower-triangular
     * factor S every chain adapts by itself — after EVERY transition, accepted or not, S <- chol(S (I + c z z') S')' with
     * c = min(1, D count^-gamma) (min(1, exp(ratio)) - targetrate) / (z . z).  Draws exactly what MH draws (D normals and one accept
     * uniform per transition) and needs no gradient.  KLARA_TARGET_LOGISTIC with D <= 8 (layout kinds 0 and 2) and KLARA_TARGET_CUSTOM
     * whole-vector closures (plain or likelihood + prior form) with D <= 8 at one chain per lane; every other target, pair closures,
     * more lanes per chain and D >= 9 are KLARA_ERR_UNSUPPORTED.  Only KLARA_TUNER_VANILLA (verbose or not: it counts as for MH);
     * another tuner is KLARA_ERR_UNSUPPORTED.  S lives on the device per chain (klara_get_ram_factor / klara_set_ram_factor);
     * klara_set_state and klara_reset put S = klara_desc.ram_S0 and restart the count.  DESIGN.md section 2, R1-R4. */
    KLARA_SAMPLER_RAM = 6,
    /* (7 is reserved like 5: klara_create and klara_check_custom_target refuse it with KLARA_ERR_INVALID_ARG) */
    /* AM(C0; corescale, minorscale, c, t0), AM.jl:131-154, iterate/AM.jl:77-152 (Haario, Saksman and Tamminen 2001 with the mixture proposal of
     * Roberts and Rosenthal 2009): every chain keeps the running mean of its states and a covariance C that starts at C0.  Up to transition t0
     * it proposes x' = x + sqrt(minorscale) z.  From transition t0 + 1 on (count = t + 1 > t0) it first brings C up to date from its state and the
     * last two running means (stats/covariance.jl:6-19, k = count - 2), then proposes from the mixture of N(x, corescale C), weight 1 - c, and
     * N(x, minorscale I), weight c.  Draws what MH draws (D normals and one accept uniform per transition); the component is chosen by a uniform
     * from the two unused words of the accept block, so the stream does not move.  Needs no gradient.  Scope and tuners as for
     * KLARA_SAMPLER_RAM: KLARA_TARGET_LOGISTIC with D <= 8 (layout kinds 0 and 2), KLARA_TARGET_CUSTOM whole-vector closures (plain or
     * likelihood + prior form) with D <= 8 at one chain per lane, KLARA_TUNER_VANILLA per chain; everything else is KLARA_ERR_UNSUPPORTED.
     * am_t0 = 1 is KLARA_ERR_UNSUPPORTED too: it makes k = 0 at the first update and divides by zero.  The proposal log-densities of
     * iterate/AM.jl:102-106 cancel and are not formed; where corescale C does not factor the chain proposes from the minor component and the
     * handle counts it (klara_get_am_state).  klara_set_state and klara_reset put C = am_C0, both means = the start value and restart the
     * count.  DESIGN.md section 2, A1-A5. */
    KLARA_SAMPLER_AM = 8,
    /* (9 is reserved like 5 and 7) */
    /* MuvAMWG(sigma) with RobertsRosenthalMCTuner(targetrate, period), samplers/AMWG.jl:139-151, iterate/AMWG.jl:82-171,
     * tuners/RobertsRosenthalMCTuner.jl (Roberts and Rosenthal 2009, section 3): adaptive Metropolis-within-Gibbs.  A transition is a sweep over
     * the D coordinates in order; coordinate i proposes x_i' = x_i + sqrt(exp(logsigma_i)) z_i with MH's i-th normal of the transition, evaluates
     * the log-target at the current state with coordinate i replaced, and accepts iff ratio > 0 || ratio > log(u_i), u_i from block slot
     * ceil(D/2) + (i >> 1) of the transition (words (x, y) for even i, (z, w) for odd i, 44 bits as the accept draw; u_0 is MH's accept draw, the
     * normals use only the slots below ceil(D/2): the stream does not move).  Every chain keeps logsigma[D] and a window count accepted[D]; when
     * count = t + 1 is a multiple of klara_desc.period, batch = count / period, delta = min(0.01, 1 / sqrt(batch)) and every coordinate moves
     * its logsigma_i by -delta where accepted_i / period < klara_desc.targetrate, by +delta otherwise, and clears accepted_i.  Adaptation never
     * stops.  Needs no gradient; D evaluations of the log-target per transition.  Only KLARA_TUNER_ROBERTS_ROSENTHAL per chain (any other tuner,
     * the pooled mode, and that tuner with any other sampler: KLARA_ERR_UNSUPPORTED; klara_desc.verbose changes nothing on the device).
     * KLARA_TARGET_LOGISTIC up to 16 parameters whose rows fit the LDS (layout kinds 0 and 2) and KLARA_TARGET_CUSTOM whole-vector closures
     * (plain, likelihood + prior, autodiff sources) with D <= 32 at one chain per lane; pair closures, staged closures, the Gaussian and
     * hierarchical families: KLARA_ERR_UNSUPPORTED.  The accept count and the accept mask record whether at least one coordinate moved;
     * klara_get_amwg_state / klara_get_amwg_accept_mask have the per-coordinate view.  klara_set_state and klara_reset put
     * logsigma = klara_desc.amwg_logsigma0, clear the counts and restart the schedule.  DESIGN.md section 2, W1-W6. */
    KLARA_SAMPLER_AMWG = 10,
    /* (11 is reserved like 5, 7 and 9) */
    /* MH(Σ::Matrix), samplers/MH.jl:63-66 (x -> MvNormal(x, Σ)) with iterate/MH.jl:72-124, symmetric normalised branch: random-walk Metropolis with a full
     * proposal covariance, one for the whole job.  With L the lower Cholesky factor of Σ (klara_desc.mh_factor) and z the D normals MH draws for the chain
     * and transition, the proposal is x' = x + L z, row i summed as w_i = L_i0 z_0, then w_i = w_i + L_ik z_k for k = 1 .. i ascending, each a separate
     * multiplication and addition; everything else is KLARA_SAMPLER_MH — the evaluation, ratio = lt' - lt, the accept test with MH's accept uniform from
     * its slot, the monitors; the stream does not move.  The proposal densities of a symmetric proposal cancel and are not formed.  The factor lives on the
     * device once per handle (klara_get_mh_factor / klara_set_mh_factor), not per chain.  Only KLARA_TUNER_VANILLA per chain (it counts when verbose, as
     * for MH; any other tuner and the pooled mode: KLARA_ERR_UNSUPPORTED).  KLARA_SAMPLER_AMWG's scope: KLARA_TARGET_LOGISTIC up to 16 parameters whose
     * rows fit the LDS (layout kinds 0 and 2, never the matrix cores) and KLARA_TARGET_CUSTOM whole-vector closures (plain, likelihood + prior, autodiff
     * sources) with D <= 32 at one chain per lane; pair closures, staged closures, the Gaussian and hierarchical families: KLARA_ERR_UNSUPPORTED.
     * klara_desc.mh_sigma is not read.  klara_reset puts klara_desc.mh_factor back; klara_set_state leaves the factor alone (it is the job's, not a
     * chain's).  DESIGN.md section 2, C1-C3. */
    KLARA_SAMPLER_MH_COV = 12
} klara_sampler;

/* Target families evaluated on device (stand-ins for the user closures of
 * BasicContMuvParameter.jl:383-411; arbitrary Julia closures cannot run on the GPU). */
typedef enum klara_target {
    /* lt = c - sum_i w_i (x_i - mu_i)^2 ; grad_i = -2 w_i (x_i - mu_i).
     * README.md:23,155 is w=1, mu=0, c=0; MvNormal(mu, sigma I) of test/BasicContMuvParameter.jl:39-56
     * is w = 1/(2 sigma^2), c = -D/2 log(2 pi) - D log sigma. */
    KLARA_TARGET_GAUSS_DIAG = 0,
    /* lt = c - 1/2 (x-mu)' P (x-mu) ; grad = -P (x-mu).  P = dense precision matrix (D x D).  D <= 128: FP64 matrix cores (all four
     * samplers; P in LDS); D = 129..256: all four stay on the matrix cores (P streamed from memory; HMC's momentum in LDS: 64 TFLOP/s
     * at D = 256); D = 257..1024 (round 6; refused before): all four samplers with the tile of 16 chains on a workgroup of 4 / 8 wavefronts that
     * deal the row tiles of P evenly (layout kind 6, klara_dense_split.h: HMC L = 10 at 56 .. 71 TFLOP/s); D > 1024 is KLARA_ERR_UNSUPPORTED. */
    KLARA_TARGET_GAUSS_DENSE = 1,
    /* Bayesian logistic regression of doc/examples/swiss/MALA/analytical.jl:11-18:
     * lt = dot(Xp, y) - sum(log(1+exp(Xp))) - 0.5 (p.p/lambda + D log(2 pi lambda)).  Up to 16 parameters: the data rows in LDS, dealt to 4 lanes
     * per chain; 17 .. 256 parameters (and 9 .. 16 with more rows than the LDS holds), every sampler: X p and X' (y - 1/(1+exp(-Xp))) of 16 chains
     * per wavefront on the FP64 matrix cores, X streamed from memory — any number of rows (round 6; layout kind 5).  (KLARA_LOGIT_NO_MFMA=1 in the
     * environment: the same closures through the run-time compiled path, as in rounds 1-5.)  257 .. 1024 parameters: that closure form, one chain
     * per lane with the vector in scratch (correct, slow; round 6 — refused before). */
    KLARA_TARGET_LOGISTIC = 2,
    /* Hierarchical normal growth-curve model for data/rats/{weight,age}.csv (BASELINE cfg 5).  The reference
     * ships the data but no model (doc/examples/rats/Gibbs.jl:1-7 is a stub), so the target is builder-defined:
     * the BUGS "Rats" model  Y_ij ~ N(alpha_i + beta_i xc_j, sigma_c^2),  alpha_i ~ N(alpha_c, sigma_a^2),
     * beta_i ~ N(beta_c, sigma_b^2),  alpha_c, beta_c ~ N(0, 1/prior_prec),  1/sigma_k^2 ~ Gamma(a, b),
     * sampled in theta = (alpha_1, beta_1, ..., alpha_R, beta_R, alpha_c, beta_c, log sigma_c, log sigma_a,
     * log sigma_b), D = 2R + 5 (65 for the 30 rats).  See DESIGN.md for the log-density. */
    KLARA_TARGET_HIER_NORMAL = 3,
    /* User-defined target — the device form of BasicContMuvParameter(:p, logtarget=f, gradlogtarget=g)
     * (BasicContMuvParameter.jl:174-201,264-279; uptogradlogtarget! = logtarget!; gradlogtarget!, :270-274).
     * klara_desc.custom_src is source text in the C subset accepted by hipcc and by a host C compiler; it defines
     *   KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata);
     *   KLARA_USER_FN void   klara_user_gradlogtarget(const double* x, int D, const double* data, long long ndata,
     *                                                 double* g);           (needed by MALA / HMC only)
     * and is compiled for gfx950 at klara_create (hiprtc) into the group-layout transition kernels (D <= 1024 — round 6: up to 64 lanes x 16 elements of the staged form; 256 before —; KLARA_D is predefined
     * to D so that loops unroll): up to D = 32 one chain per lane, the whole vector in the lane's registers; beyond, 4 .. 32 lanes per
     * chain — normals, sampler arithmetic and sums spread over them — and for an evaluation the closure reads the vector from the chain's
     * row of LDS, every lane of the chain evaluating it identically (KLARA_CUSTOM_LANES=1 in the environment keeps one chain per lane
     * at any D: the vector then lives in scratch, which only a closure far costlier than the sampler's own work repays).  kd_exp, kd_log,
     * kd_fma, kd_erf (klara.jl_amd/csrc/detmath.h) and IEEE + - * / sqrt give the same bits on host and device;
     * `data` is custom_data (custom_ndata doubles, copied to the device at create).
     * Likelihood + prior form (BasicContMuvParameter(:p, loglikelihood=..., logprior=..., gradloglikelihood=..., gradlogprior=...),
     * BasicContMuvParameter.jl:174-201): a source that starts with `#define KLARA_USER_LIKELIHOOD_PRIOR 1` defines
     * klara_user_loglikelihood, klara_user_logprior (and klara_user_gradloglikelihood, klara_user_gradlogprior for MALA / HMC)
     * instead; the library composes logtarget = loglikelihood + logprior and the gradients' elementwise sum
     * (klara.jl_amd/csrc/klara_custom_compose.h) and can keep both parts per saved step (KLARA_MON_HIST_LLLP).
     * Pair form, for targets that are a sum of terms of one or two neighbouring coordinates (every separable target, pairwise-coupled
     * ones, the README closure): a source that starts with `#define KLARA_USER_PAIR_TARGET 1` defines instead
     *   KLARA_USER_FN double klara_user_pair(double x0, double x1, int pair, int D, const double* data, long long ndata,
     *                                        double* g0, double* g1);
     * with logtarget(x) = sum over pairs P of klara_user_pair(x[2P], x[2P+1], P, ...) and (*g0, *g1) the pair's two partial derivatives
     * (for the half pair of an odd D, x1 is 0 and *g1 is ignored; the function is called for the real pairs only, 0 <= pair < ceil(D/2), so it may
     * index `data` by pair or by coordinate).  Such a job runs on the few-lanes-per-chain kernels of the diagonal
     * Gaussian (layout kind 3: 8 / 16 / 32 / 64 lanes per chain, 17 <= D <= 1024; MH, MALA, HMC with every tuner, the running sums and the
     * value / logtarget / gradlogtarget histories; klara_get_layout reports the summation order: a lane adds its pairs' terms in
     * ascending order, then the butterfly over the chain's lanes) instead of holding the whole vector in one lane: at D = 100 the
     * README closure runs at 3.5e9 transitions/s in this form and at 2.1e8 in the whole-vector form.  A pair-form job those kernels do
     * not serve — D < 17, or the slice sampler — is taken as a whole-vector closure whose logtarget is the sum of the pairs' terms,
     * pair 0 first (klara_custom_compose.h; D <= 1024).
     * Forward-mode autodiff (diffopts=DiffOptions(mode=:forward), src/autodiff/forward.jl, BasicContMuvParameter.jl:627-694): a source that starts
     * with `#define KLARA_USER_AUTODIFF 1` defines no gradient; its log-target is generic in its scalar type,
     *   template <class T, class V>
     *   KLARA_USER_FN T klara_user_logtarget_ad(const V& x, int D, const double* data, long long ndata);
     * (C++; x[i] yields a T; with KLARA_USER_LIKELIHOOD_PRIOR as well: klara_user_loglikelihood_ad and klara_user_logprior_ad), written with + - * /
     * and comparisons between T and double, sqrt, fabs, kd_fma, kd_exp, kd_log, kd_erf and kd_softplus_logistic_rows.  The library differentiates it
     * with dual numbers (klara.jl_amd/csrc/klara_autodiff.h): one chain per lane in sweeps of `#define KLARA_USER_AUTODIFF_CHUNK n` directions
     * (DiffOptions.chunksize; absent or 0: the library's choice), in the staged form every lane of a chain carrying the partials of its own elements.
     * MH and the slice sampler use the double instantiation only.  `#define KLARA_USER_AUTODIFF 2` also gives KLARA_SAMPLER_SMMALA its metric, the
     * upper triangle of MINUS the Hessian (forward.jl:11-16; the plain whole-vector form, D <= 8; with any other sampler 2 means 1).  Pair closures
     * with the marker, and second order outside SMMALA's limits, are refused (KLARA_ERR_UNSUPPORTED); a marker without its _ad function is
     * KLARA_ERR_COMPILE.  Reverse mode does not exist on the device. */
    KLARA_TARGET_CUSTOM = 4
} klara_target;

/* src/tuners/{VanillaMCTuner,AcceptanceRateMCTuner}.jl */
typedef enum klara_tuner {
    KLARA_TUNER_VANILLA = 0,
    KLARA_TUNER_ACCEPT_RATE = 1,
    /* DualAveragingMCTuner (src/tuners/DualAveragingMCTuner.jl:54-101), HMC only (HMC.jl:124-133): Nesterov dual
     * averaging of the leapfrog step during the first da_nadapt transitions, nleaps = max(1, round(lambda/step))
     * per transition (iterate/HMC.jl:142-144), step = eps_bar afterwards (iterate/HMC.jl:246-248).  Per chain. */
    KLARA_TUNER_DUAL_AVERAGING = 2,
    /* RobertsRosenthalMCTuner(targetrate = 0.44, period = 50) (src/tuners/RobertsRosenthalMCTuner.jl:84-101), KLARA_SAMPLER_AMWG only: every
     * `period` transitions a coordinate's log proposal scale moves by delta = min(0.01, batch^-1/2) towards the target rate (see
     * KLARA_SAMPLER_AMWG).  Reads klara_desc.targetrate (in (0, 1)) and klara_desc.period.  Per chain. */
    KLARA_TUNER_ROBERTS_ROSENTHAL = 3
} klara_tuner;

typedef enum klara_tuner_mode {
    KLARA_TUNE_PER_CHAIN = 0,   /* reference semantics: one BasicMCTune per job = per chain      */
    KLARA_TUNE_POOLED = 1       /* one tune state per GPU, rate pooled over the GPU's chains      */
} klara_tuner_mode;

/* monitor flags (jobs.jl:9-43 outopts :monitor / :diagnostics / :destination) */
#define KLARA_MON_ACCEPT    0x1u  /* keep the per-step accept diagnostics (u8 per step per chain)  */
#define KLARA_MON_HISTORY   0x2u  /* :destination=>:nstate — keep value at every postrange step    */
#define KLARA_MON_SUMMARIES 0x4u  /* accumulate sum x, sum x^2 over postrange steps on device      */
#define KLARA_MON_HIST_LT   0x8u  /* :monitor=>[:logtarget]: keep logtarget at every postrange step */
#define KLARA_MON_HIST_GRAD 0x10u /* :monitor=>[:gradlogtarget] (MALA/HMC only)                    */
#define KLARA_MON_HIST_LLLP 0x20u /* :monitor=>[:loglikelihood, :logprior]: the two parts of a likelihood + prior user target
                                     (KLARA_TARGET_CUSTOM whose source defines KLARA_USER_LIKELIHOOD_PRIOR) at every postrange step */
#define KLARA_MON_COVARIANCE 0x40u /* accumulate the pooled D x D cross-products of the saved samples of all chains while sampling, on the FP64 matrix
                                     cores (the covariance / correlations of the posterior; see the gather call below).  A consumer of the saved samples, as
                                     klara_desc.acov_maxlag is: the values are kept (a 32-column ring of its own when no value history was asked for), the
                                     job runs as one chain partition, and a job that cannot keep a value history is refused as with KLARA_MON_HISTORY.
                                     ndims > KLARA_COV_MAX_DIMS: KLARA_ERR_UNSUPPORTED.  The transition kernels never see the bit: the chains of a job are the
                                     same bits with and without it. */
#define KLARA_COV_MAX_DIMS 256
#define KLARA_DERIVED_MAX_OUT 64   /* outputs of a derived-quantity closure at most (klara_desc.derived_nout) */

typedef struct klara_desc {
    uint32_t struct_size;        /* = sizeof(klara_desc), ABI check                                  */
    uint32_t abi_version;        /* = KLARA_ABI_VERSION                                              */

    int32_t  sampler;            /* klara_sampler                                                    */
    int32_t  target;             /* klara_target                                                     */
    int32_t  tuner;              /* klara_tuner                                                      */
    int32_t  tuner_mode;         /* klara_tuner_mode                                                 */

    int64_t  nchains;            /* chains owned by this handle (this GPU's shard)                   */
    int64_t  chain_offset;       /* global id of local chain 0 (RNG subsequence = offset + local id) */
    int32_t  ndims;              /* D                                                                */
    int32_t  device;             /* HIP device ordinal                                               */

    /* sampler parameters */
    const double* mh_sigma;      /* MH: proposal std-devs, D doubles (MH.jl:63: MvNormal(x, sigma))   */
    double   driftstep;          /* MALA (MALA.jl:65: > 0), SMMALA (SMMALA.jl:132: > 0)               */
    double   leapstep;           /* HMC  (HMC.jl:94: > 0)                                            */
    int32_t  nleaps;             /* HMC  (HMC.jl:95: > 0)                                            */
    int32_t  slice_stepout;      /* SliceSampler.stepout                                             */
    const double* slice_widths;  /* SliceSampler.widths, D doubles (> 0, SliceSampler.jl:27)         */
    const double* amwg_logsigma0; /* MuvAMWG.logσ0, D doubles: the initial log proposal scales (the log of the constructor's σ, AMWG.jl:139-151; the
                                    proposal's standard deviation is sqrt(exp(logsigma)), iterate/AMWG.jl:96), all finite.  Required for
                                    KLARA_SAMPLER_AMWG; NULL for every other sampler (else KLARA_ERR_INVALID_ARG).  Copied at create.  (Beside the
                                    other samplers' vectors: the fields behind steps_per_launch and in front of stream are the derived quantities') */
    const double* mh_factor;     /* MH(Σ): the lower Cholesky factor L of the proposal covariance, Σ = L L', D x D row-major; only the lower triangle is
                                    read, every read entry finite and the diagonal positive (else KLARA_ERR_INVALID_ARG).  Required for
                                    KLARA_SAMPLER_MH_COV; NULL for every other sampler (else KLARA_ERR_INVALID_ARG).  Copied at create. */

    /* tuner (AcceptanceRateMCTuner.jl:38-44; VanillaMCTuner: only period/verbose are used) */
    double   targetrate;         /* in (0,1)                                                         */
    double   score_k;            /* steepness of logistic_rate_score (default 7)                     */
    int32_t  period;             /* > 0, default 100                                                 */
    int32_t  verbose;            /* counts proposals the way the reference's verbose tuners do      */
    /* DualAveragingMCTuner(targetrate, nadapt; e0bar=1, h0bar=0, gamma=0.05, t0=10, kappa=0.75) */
    int64_t  da_nadapt;          /* > 0                                                              */
    double   da_eps0bar;         /* > 0                                                              */
    double   da_h0bar;
    double   da_gamma;
    double   da_kappa;
    int32_t  da_t0;              /* > 0                                                              */
    int32_t  tuner_score;        /* AcceptanceRate score: 0 logistic_rate_score(x, score_k) (default k 7), 1 erf_rate_score(x, score_k) (default k 3) */

    /* range (BasicMCRange.jl:17-36) */
    int64_t  nsteps;
    int64_t  burnin;
    int64_t  thinning;

    /* target parameters (host pointers, copied at create) */
    const double* gauss_w;       /* DIAG: D weights (NULL = all 1)                                   */
    const double* gauss_mu;      /* DIAG/DENSE: D means (NULL = 0)                                   */
    double   gauss_const;        /* DIAG/DENSE: additive constant c                                  */
    const double* gauss_prec;    /* DENSE: D*D row-major precision matrix                            */
    const double* logit_X;       /* LOGISTIC: ndata x D row-major design matrix                      */
    const double* logit_y;       /* LOGISTIC: ndata outcomes                                         */
    int32_t  logit_ndata;        /* LOGISTIC: rows.  D <= 8: ndata * (E + 1) <= KLARA_LOGIT_MAX_LDS_DOUBLES, E = 2, 4 or 8 >= D (rows live in LDS);
                                    D = 9..16: the same kernels (E = 16) while the rows fit, the closure form beyond; D = 17..256: any number of
                                    rows (run-time compiled closure form, rows read from memory) */
    int32_t  nstreams;           /* internal HIP streams for independent chain partitions (pair-transposed layout only):
                                    0 = automatic (2 when a partition still fills the GPU), 1..4 = forced        */
    double   logit_lambda;       /* LOGISTIC: prior variance (v[1] of the example)                   */
    const double* hier_Y;        /* HIER_NORMAL: R x T row-major observations                        */
    const double* hier_xc;       /* HIER_NORMAL: T centred covariate values (age_j - 22 for rats)    */
    int32_t  hier_nunits;        /* R (D must equal 2R + 5)                                          */
    int32_t  hier_ntimes;        /* T (<= 16)                                                        */
    double   hier_prior_prec;    /* precision of the N(0, .) priors on alpha_c, beta_c               */
    double   hier_gamma_a;       /* Gamma(a, b) prior on the three precisions                        */
    double   hier_gamma_b;
    const char*   custom_src;    /* CUSTOM: NUL-terminated source text (see KLARA_TARGET_CUSTOM)     */
    const double* custom_data;   /* CUSTOM: read-only data block handed to the user functions, or NULL */
    int64_t  custom_ndata;       /* CUSTOM: doubles in custom_data                                   */
    int64_t  bm_batchlen;        /* > 0: streaming batch means over the saved samples (needs KLARA_MON_SUMMARIES):
                                    every bm_batchlen saved samples a batch of every (chain, dimension) series is closed on
                                    device; klara_get_chain_bm then gives mcvar(:bm) (mcvar.jl:35-41) with no stored history */

    int64_t  hist_ring_cols;     /* > 0: the history monitors (value / logtarget / gradlogtarget / loglikelihood, logprior) keep only
                                    the LAST hist_ring_cols saved steps (a ring): bounded memory for jobs that drain the samples as
                                    they go (the :iostream destination with :flush, jobs.jl:17-29).  0: every saved step is kept. */
    int32_t  acov_maxlag;        /* > 0: lagged cross-products of every (chain, dimension) series are accumulated while sampling
                                    (lags 0..acov_maxlag, at most 127: 3 (maxlag + 1) doubles per series), so that Geyer's initial monotone / positive sequence estimators
                                    (mcvar(:imse | :ipse, maxlag), mcvar.jl:75-105,137-158) need no stored history:
                                    klara_get_chain_acov_mcvar.  Uses a value ring of its own when no history monitor is on. */
    int32_t  sparse_moves;       /* how untuned MH / MALA jobs on the diagonal Gaussian (17 <= D <= 104) keep their running sums.  Two kernel
                                    families run such a job and produce the same bits (both sum in the 8-lane order klara_get_layout reports):
                                    4 lanes per chain, a moving chain's sums folded straight into memory (cheapest while chains move rarely:
                                    acceptance of a few per cent), and 8 lanes per chain with the sums of the chains that moved resident in
                                    registers (flat cost at any acceptance).  0 (default): the library decides launch by launch, on the device,
                                    from the accepted proposals of the previous launch (klara_get_launch_modes reports what ran); 1: always the
                                    4-lane kernels; 2: always the 8-lane kernels.  Results never depend on this field. */
    double   smmala_softabs;     /* SMMALA: 0 = no transform of the metric (SMMALA(driftstep), transform = nothing); a > 0: the metric of every chain, at the
                                    start state and at every proposal, is softabs(G, a) = Q diag(lambda ./ tanh(a lambda)) Q' (stats/metrics.jl:1-4), i.e.
                                    SMMALA(driftstep, H -> softabs(H, a)), formed on the device in the lane's registers (klara_softabs.h, DESIGN.md section 2
                                    T1-T5).  KLARA_TARGET_CUSTOM only (the plain whole-vector form, D <= 8: a klara_user_tensorlogtarget or
                                    KLARA_USER_AUTODIFF 2, whose minus-Hessian is indefinite wherever the target is not log-concave).
                                    KLARA_TARGET_LOGISTIC with a > 0 is KLARA_ERR_UNSUPPORTED: its metric X' diag(r (1 - r)) X + I / lambda is positive
                                    definite by construction and has no use for the transform.  Negative or non-finite, or a > 0 with another sampler:
                                    KLARA_ERR_INVALID_ARG. */
    const double* am_C0;         /* AM: the initial covariance, D x D row-major, symmetric; the upper triangle is read and must be finite (AM.jl:132).
                                    Required for KLARA_SAMPLER_AM; NULL for every other sampler (else KLARA_ERR_INVALID_ARG) */
    double   am_corescale;       /* AM: scaling of C in the core mixture component, > 0 (AM.jl:139); 0 for every other sampler */
    double   am_minorscale;      /* AM: variance of the stabilising component N(x, minorscale I), > 0 (AM.jl:140); 0 for every other sampler */
    double   am_c;               /* AM: weight of the stabilising component, in [0, 1) (AM.jl:141; 1 - c > 0, AM.jl:107-109); 0 for every other sampler */
    int64_t  am_t0;              /* AM: transitions before the adaptation starts, >= 2 (AM.jl:142; 1 is KLARA_ERR_UNSUPPORTED: k = count - 2 = 0 divides
                                    by zero at the first update, stats/covariance.jl:18); 0 for every other sampler */
    const double* ram_S0;        /* RAM: the initial factor, D x D row-major; the lower triangle is read and its diagonal must be > 0
                                    (RAM.jl:100).  Required for KLARA_SAMPLER_RAM; NULL for every other sampler (else KLARA_ERR_INVALID_ARG) */
    double   ram_targetrate;     /* RAM: target acceptance rate, in (0, 1) (RAM.jl:101); 0 for every other sampler */
    double   ram_gamma;          /* RAM: exponent of the step size eta = min(1, D count^-gamma), in (0.5, 1] (RAM.jl:102); 0 for every other sampler */
    const double* marg_lo;       /* pooled marginal histograms (klara_gather_histogram), switched on by marg_nbins > 0: the lower bounds, D doubles, copied at create */
    const double* marg_hi;       /* ... and the upper bounds, D doubles, lo[d] < hi[d], all finite.  Both NULL when marg_nbins = 0 (else KLARA_ERR_INVALID_ARG) */
    int64_t  marg_nbins;         /* 0: off (nothing changes); 1..KLARA_MARG_MAX_BINS: after every launch the saved samples of all chains are counted per dimension
                                    into marg_nbins equal bins over [lo[d], hi[d]) plus an underflow and an overflow slot (the rule is stated at
                                    klara_gather_histogram).  A consumer of the saved samples, as acov_maxlag and KLARA_MON_COVARIANCE are: the values are kept
                                    (a 32-column ring of its own when no value history was asked for), the job runs as one chain partition, and a job that cannot
                                    keep a value history is refused as with KLARA_MON_HISTORY.  Every sampler, target and ndims the library accepts.  The transition
                                    kernels never see the field: the chains of a job are the same bits with and without it. */

    uint64_t seed;               /* Philox key                                                       */
    uint32_t monitor;            /* KLARA_MON_* bits                                                 */
    int32_t  steps_per_launch;   /* transitions fused in one kernel launch (>=1; 0 = library default) */
    const char* derived_src;     /* derived quantities — a user function of the state, summarised on the device (the reference's Transformation,
                                    src/variables/variables.jl:102-119, on the one-parameter job): C text compiled for gfx950 at klara_create, for ANY target
                                    family, that defines
                                      KLARA_USER_FN void klara_user_derived(const double* x, int D, const double* data, long long ndata, double* out, int K);
                                    x: one saved sample (read-only), data: the closure's own block (derived_data), out: K = derived_nout doubles, all of which
                                    it must write.  KLARA_D and KLARA_K are defined before the text.  It may call the kd_* functions of detmath.h that need no table of
                                    their own in dynamic LDS (kd_exp, kd_exp_neg, kd_log, kd_log_u01, kd_log12, kd_erf, kd_sincos2pi, kd_softplus_logistic, kd_fma:
                                    every one but kd_sincos2pi_tab20 and the other readers of kd_screm_lds, a table in dynamic LDS that would alias the kernel's rows) and nothing
                                    else from the library, and must be a pure function of its arguments: the same text built by a host compiler with
                                    -ffp-contract=off then gives the same bits.  After every launch that saved m > 0 columns, for each chain c and saved step
                                    t in ascending t, y = klara_user_derived(x_ct):  dsum[c][k] = dsum[c][k] + y[k];  dsumsq[c][k] = dsumsq[c][k] + y[k] * y[k]
                                    (the product rounded, then added; no contraction).  A chain's sums depend on that chain only; the bits are the same
                                    however the steps are cut into launches; no floating-point atomics.  A non-finite y flows through as IEEE arithmetic.
                                    A consumer of the saved samples exactly as marg_nbins is (value ring, one chain partition, the status of
                                    KLARA_MON_HISTORY where a job cannot keep values); the transition kernels never see it: the chains of a job are the same
                                    bits with and without it.  klara_set_state and klara_reset clear the accumulators.  NULL exactly when derived_nout = 0
                                    (else KLARA_ERR_INVALID_ARG); a text that does not compile: KLARA_ERR_COMPILE (klara_compile_log, klara_check_derived).
                                    Read with klara_get_derived_sums and the klara_gather_derived_* calls.  Copied at create (klara.jl_amd/csrc/klara_derived.h) */
    const double* derived_data;  /* the closure's data block, derived_ndata doubles, copied to the device at create; NULL when derived_ndata = 0 */
    int64_t  derived_ndata;      /* >= 0; > 0 needs derived_data and derived_nout > 0 */
    int64_t  derived_nout;       /* K: 0 = off (nothing changes), 1..KLARA_DERIVED_MAX_OUT */
    int64_t  derived_nbins;      /* 0: no histograms of the outputs; 1..KLARA_MARG_MAX_BINS (needs derived_nout > 0): y is also staged as [column][chain][K] and
                                    counted by the marginals' kernel with the geometry of (nchains, K, derived_nbins) and the slot rule stated at
                                    klara_gather_histogram — a NaN output is counted in the overflow slot (klara_gather_derived_histogram) */
    const double* derived_lo;    /* the histograms' lower bounds, K doubles ... */
    const double* derived_hi;    /* ... and upper bounds, K doubles, all finite, lo[k] < hi[k].  Both NULL when derived_nbins = 0 (else KLARA_ERR_INVALID_ARG) */
    void*    stream;             /* hipStream_t to launch on, or NULL for a library-owned stream     */
} klara_desc;

typedef struct klara_handle klara_handle;

/* Lifetime.  klara_create validates the descriptor the way the Julia constructors do and uploads the
 * target data.  (BasicMCJob inner ctor, BasicMCJob.jl:24-104.) */
klara_status klara_create(const klara_desc* desc, klara_handle** out);
klara_status klara_destroy(klara_handle* h);

/* Initial values (v0 of BasicMCJob.jl:156-185), nchains x ndims row-major.  Evaluates the target and
 * (MALA/HMC) its gradient on device and applies the reference's finiteness asserts
 * (MH.jl:72-85, MALA.jl:76-90, HMC.jl:106-120, SliceSampler.jl:40-48).  Also (re)initialises the tuner
 * state (samplers.jl:29-45: accepted=proposed=0, totproposed=period) and the step counter. */
klara_status klara_set_state(klara_handle* h, const double* x_host);
/* Same, x0 ~ N(0, I) drawn on device from the handle's Philox stream (transition index -1). */
klara_status klara_init_state_normal(klara_handle* h);

/* The transition loop: nsteps calls of iterate! for every chain (BasicMCJob.jl:219-238), including the
 * tuning block and the save rule.  Synchronous w.r.t. the host on return. */
klara_status klara_run(klara_handle* h, int64_t nsteps);
/* Same, but returns immediately after enqueueing (for overlap / external event timing). */
klara_status klara_run_async(klara_handle* h, int64_t nsteps);
klara_status klara_synchronize(klara_handle* h);

/* reset(job[, x]) of BasicMCJob.jl:187-201: rewind sampler/tuner state and counters; x_host may be
 * NULL (keep the current values, re-evaluate the target).  In the reference the random generator keeps advancing across a
 * reset, so run -> reset -> run gives an independent replicate; here the transition index restarts at 0 and the job moves to a
 * fresh Philox key instead: after the k-th klara_reset the key is seed + k * KLARA_EPOCH_KEY_STRIDE (mod 2^64).
 * klara_set_state does not change the key: it replays the job from the given values. */
#define KLARA_EPOCH_KEY_STRIDE 0x9E3779B97F4A7C15ull
klara_status klara_reset(klara_handle* h, const double* x_host);
/* the Philox key the job currently draws from and the number of klara_reset calls so far (either pointer may be NULL) */
klara_status klara_stream_key(klara_handle* h, uint64_t* key, uint64_t* epoch);

/* Read-back.  Any pointer may be NULL. */
klara_status klara_get_state(klara_handle* h, double* x, double* logtarget, double* gradlogtarget);
/* accept diagnostics of the transitions run so far since set_state/reset: steps x nchains bytes,
 * step-major (requires KLARA_MON_ACCEPT).  *nsteps_out receives the number of recorded steps. */
klara_status klara_get_accept_mask(klara_handle* h, uint8_t* mask, int64_t capacity_steps,
                                   int64_t* nsteps_out);
/* the same for the transitions [first_step, first_step + nsteps) only (0-based, within the steps run so far): nsteps x nchains
 * bytes — what a sink that drains a long job chunk by chunk reads (diagnosticvalues of the newly saved steps,
 * BasicContParamIOStream.jl:152-159) instead of every row since the start. */
klara_status klara_get_accept_rows(klara_handle* h, int64_t first_step, int64_t nsteps, uint8_t* mask);
/* per-chain accepted-transition counts over all steps since set_state/reset */
klara_status klara_get_accept_counts(klara_handle* h, uint64_t* naccept, uint64_t* nsteps_out);
/* per-chain sums over saved (postrange) steps: sum[c*D+d], sumsq[c*D+d]; *nsaved_out = count */
klara_status klara_get_chain_sums(klara_handle* h, double* sum, double* sumsq, int64_t* nsaved_out);
/* sums pooled over this handle's chains (reduced on device): sum[D], sumsq[D], total accepted,
 * total transitions, saved samples per chain. */
klara_status klara_get_pooled_summaries(klara_handle* h, double* sum, double* sumsq,
                                        uint64_t* naccept, uint64_t* ntransitions,
                                        int64_t* nsaved_out);
/* ---- multi-GPU without a host framework (SURVEY section 8(b),(e)): one process (or thread) per GPU, chains sharded by
 * klara_desc.chain_offset, and ONE exchange: the all-reduce of the pooled chain summaries over RCCL / xGMI.  (The Python host
 * does the same through torch.distributed, klara.jl_amd/distributed.py.)  librccl.so is loaded on first use (dlopen), a
 * single-GPU user never touches it.  The 128-byte id is RCCL's ncclUniqueId: rank 0 creates it, the caller ships it to the
 * other ranks by whatever it has (file, socket, MPI, Julia Distributed). */
#define KLARA_COMM_ID_BYTES 128
typedef struct klara_comm klara_comm;
klara_status klara_comm_unique_id(uint8_t id[KLARA_COMM_ID_BYTES]);
klara_status klara_comm_init(klara_comm** out, int32_t nranks, int32_t rank, const uint8_t id[KLARA_COMM_ID_BYTES],
                             int32_t device);
/* ranks and this rank's index as the communicator reports them (ncclCommCount, ncclCommUserRank) and the device it was made on:
 * what a launcher checks after the id went round (bench.py's `rccl_ranks_seen`) */
klara_status klara_comm_info(klara_comm* comm, int32_t* nranks, int32_t* rank, int32_t* device);
klara_status klara_comm_destroy(klara_comm* comm);
/* Sum over all ranks of klara_get_pooled_summaries: sum[D], sumsq[D] (NULL unless KLARA_MON_SUMMARIES is on), accepted
 * transitions, transitions, saved samples (= saved steps x chains), chains.  Collective: every rank calls it. */
klara_status klara_gather_summaries(klara_handle* h, klara_comm* comm, double* sum, double* sumsq, uint64_t* naccept,
                                    uint64_t* ntransitions, uint64_t* nsamples, uint64_t* nchains);

/* The pooled posterior moments over every chain of every rank WITHOUT the cancellation of sumsq/n - mean^2 (which loses
 * mean^2/var digits: 4 at the rats model's alpha_c): mean[D], m2[D] = sum (x - mean)^2 per dimension over all saved samples
 * (variance = m2 / nsamples, Klara's var(chain) over the pooled chains), the counters as klara_gather_summaries.  Every chain's
 * running sums become (n, mean, M2) on the device with the one cancelling subtraction carried in double-double, then chains,
 * blocks and ranks are merged by Chan's update; across ranks that is three all-reduces (4 counters, D weighted means, D sums of
 * squares).  comm = NULL: this handle's chains only, no RCCL involved (what a host with its own transport — torch.distributed,
 * MPI.jl, Julia's Distributed — merges itself, klara.jl_amd/distributed.py allreduce_moments).  Requires KLARA_MON_SUMMARIES.
 * Collective when comm != NULL: every rank calls it. */
klara_status klara_gather_moments(klara_handle* h, klara_comm* comm, double* mean, double* m2, uint64_t* nsamples,
                                  uint64_t* naccept, uint64_t* ntransitions, uint64_t* nchains);

/* The pooled posterior covariance (requires KLARA_MON_COVARIANCE, else KLARA_ERR_STATE): over all chains c and all saved steps t, n = chains x saved steps,
 * mean[D] and m2[D x D] = sum (x - mean)(x - mean)', row-major, both triangles filled and bitwise symmetric — the D x D form of what klara_gather_moments
 * returns (its diagonal is that call's m2); the caller divides: cov = m2 / (n - 1).  Accumulated while sampling: after every launch the saved samples go
 * through v_mfma_f64_16x16x4_f64 as z = x - pivot (pivot = the first saved sample of local chain 0), slab of chains by slab, every element one fma chain
 * in the order (saved step, chain) — the same bits however the steps are cut into launches (klara.jl_amd/csrc/klara_cov.h).  This call
 * only reads the accumulators: m2 = S - T T' / n with the product's rounding carried.  comm = NULL: this handle's chains only; otherwise collective, the
 * ranks merged by Chan's update in three all-reduces (4 counters, D weighted means, D x D cross-products).  Any output pointer may be NULL.  Before the
 * first saved sample: zeros, as klara_gather_moments.  klara_set_state and klara_reset clear the accumulators. */
klara_status klara_gather_covariance(klara_handle* h, klara_comm* comm, double* mean, double* m2, uint64_t* nsamples, uint64_t* nchains);

/* The Gelman–Rubin diagnostic over all chains: do the chains agree with each other?  Per dimension, over m chains of n saved samples each with chain mean
 * mu_j and M2_j = sum_t (x_jt - mu_j)^2:
 *   wsum = sum_j M2_j,  mean = (1 / m) sum_j mu_j,  bsum = sum_j (mu_j - mean)^2,
 *   W = wsum / (m (n - 1)),  B / n = bsum / (m - 1),  var+ = (n - 1) / n W + B / n,  rhat = sqrt(var+ / W)
 * (Gelman & Rubin 1992; the reference has no counterpart: one BasicMCJob is one chain).  m < 2 or n < 2: NaN; otherwise plain IEEE division: wsum = 0 with
 * bsum > 0 gives +inf, both zero NaN; nothing is clamped.  split = 0 works from the running sums (requires KLARA_MON_SUMMARIES; no history needed): every
 * chain's (mu_j, M2_j) is formed as klara_gather_moments forms it, then (chains, mean of means, bsum) go through the same two-stage Chan reduction at unit
 * weight per chain and wsum through a plain sum — no floating-point atomics, the same bits for a given chain count.  split != 0 is the split form (BDA3
 * section 11.4) from the stored value history (requires KLARA_MON_HISTORY without a ring and at least 4 saved steps, else KLARA_ERR_STATE): with
 * h = floor(n / 2), every chain gives the two half-chains of samples [0, h) and [n - h, n) — an odd n drops the middle sample — and the formulas run
 * with m -> 2 m and n -> h; the history is read once.  rhat, mean, wsum, bsum: D each; *nchains and *nper are the units the formulas ran on (split: the
 * half-chains and h).  comm = NULL: this handle's chains only; otherwise collective over the ranks: (m_r, mean_r, bsum_r) merge as the samples, means and
 * m2 of klara_gather_moments do, wsum is one more sum — four all-reduces, entered by every rank whatever happens locally.  All ranks must hold the same
 * number of saved steps: if they do not, every rank returns KLARA_ERR_STATE.  Any output pointer may be NULL.  Before the first saved sample: NaN for rhat,
 * zeros for the other outputs, KLARA_OK.  The call only reads the job's state: a job that goes on after it produces the same bits as one that never called it. */
klara_status klara_gather_rhat(klara_handle* h, klara_comm* comm, int32_t split, double* rhat, double* mean, double* wsum, double* bsum,
                               uint64_t* nchains, int64_t* nper);

/* The pooled (multi-chain) effective sample size: how many independent draws are all the chains together worth?  The estimator of BDA3 section 11.5 /
 * Vehtari et al. 2021 on R-hat's decomposition.  Per dimension, over m units (chains, or half-chains cut as klara_gather_rhat's split form cuts them) of n
 * saved samples each, with unit mean mu_j and c_j(k) = sum_(t >= k) (x_jt - mu_j)(x_j,t-k - mu_j) (n times StatsBase's autocov(v, k), demean = true):
 *   csum[k] = sum_j c_j(k),  wsum = csum[0],  mean = (1 / m) sum_j mu_j,  bsum = sum_j (mu_j - mean)^2,
 *   W = wsum / (m (n - 1)),  var+ = (n - 1) / n W + bsum / (m - 1)   (m = 1: the between term is 0),
 *   rho[0] = 1,  rho[k] = 1 - (W - csum[k] / (m n)) / var+  for k = 1 .. L,  L = min(maxlag, n - 1),
 *   P_j = rho[2 j] + rho[2 j + 1], j = 0 .. (L - 1) / 2 (integer division): pair 0 is always summed; from j = 1 the sum stops at the first P_j <= 0 (the
 *   library's convention for Geyer's stop, as klara_get_chain_acov_mcvar); each summed pair enters as min(P_j, P'_(j-1)) (the monotone sequence);
 *   tau = -1 + 2 sum P'_j,  ess = m n / tau,  pairs = the number of pairs summed.
 * pairs == (L - 1) / 2 + 1 means the window ended before Geyer's rule did: ess is then an overestimate (widen the window).  Nothing is clamped (no cap on
 * ess, no floor on tau); plain IEEE division: var+ = 0 gives NaN.  n < 4: NaN for ess, tau and rho[1..].  When the chains disagree, bsum enters var+ and
 * every rho rises towards 1 - W / var+: the sum of the per-chain ESS values, whose autocovariances are each taken around the chain's own mean, cannot see that.
 * mode: */
#define KLARA_ESS_STREAMED 0   /* from the streamed autocovariances: needs klara_desc.acov_maxlag > 0, nothing else; maxlag must be 0 (it is acov_maxlag) */
#define KLARA_ESS_HISTORY  1   /* from the stored value history (KLARA_MON_HISTORY, no ring); maxlag 1..127, <= 0: min(127, n - 1) */
#define KLARA_ESS_SPLIT    2   /* as HISTORY over every chain's two halves, cut as klara_gather_rhat's split form cuts them (>= 8 saved steps) */
/* A wrong mode for the job's monitors (or a split of fewer than 8 saved steps): KLARA_ERR_STATE; an invalid mode or maxlag: KLARA_ERR_INVALID_ARG before any
 * HIP call.  The history modes build a temporary streamed state — 3 (L' + 1) nchains ndims doubles, L' the window asked for, twice that for the split form,
 * freed before the call returns — by feeding the stored columns through the kernels that a job with acov_maxlag runs after its launches; the result has
 * the bits of a job that had streamed them.  Outputs (any may be NULL): ess, tau, mean, wsum, bsum and pairs ndims each; rho ndims x (L + 1) row-major
 * (capacity ndims x 128 is always enough); *nunits = m, *nper = n, *lags_out = L.  The across-chain sums are two stages of fixed shape without
 * floating-point atomics: the bits depend on (nchains, ndims, L, n) and the samples only, not on how the steps were cut into launches.  comm = NULL: this
 * handle's chains only.  Otherwise collective: the ranks first agree on L (an integer maximum over (L, ~L)); then (m_r, mean_r, bsum_r) merge as for
 * klara_gather_rhat and wsum, csum are summed; every rank enters every reduction whatever happened locally.  Ranks holding different L or different n all
 * return KLARA_ERR_STATE.  Before the first saved sample: NaN and zeros, KLARA_OK.  The call only reads the job's state. */
klara_status klara_gather_ess(klara_handle* h, klara_comm* comm, int32_t mode, int32_t maxlag,
                              double* ess, double* tau, double* rho /* ndims x (L + 1), row-major */, double* mean, double* wsum, double* bsum,
                              int32_t* pairs, uint64_t* nunits, int64_t* nper, int32_t* lags_out /* L */);

/* The pooled marginal histograms (requires klara_desc.marg_nbins > 0, else KLARA_ERR_STATE): what credible intervals, medians and tail probabilities are
 * read from when the job is too large to keep its values.  With nbins = marg_nbins and, per dimension d, lo = marg_lo[d], hi = marg_hi[d] and
 * inv_w = nbins / (hi - lo) (formed once on the host, in double), a saved sample x of dimension d is counted in one of nbins + 2 slots:
 *   slot 0 (underflow)        if x < lo;
 *   slot nbins + 1 (overflow) if !(x < hi): x >= hi, +inf and NaN;
 *   slot 1 + min(nbins - 1, (int)floor((x - lo) * inv_w)) otherwise.
 * (x - lo) * inv_w is a subtraction followed by a multiplication: nothing in it can contract to an fma, on any layer.  This index formula is the contract;
 * the edges lo + k (hi - lo) / nbins that the bindings report are documentation and may differ from it by an ulp at a boundary.
 * counts is ndims x (nbins + 2) row-major, uint64, over all chains of the handle and all saved steps: integer sums, exact in any order — the same result for
 * every cut of the steps into launches.  *nsamples = chains x saved steps (= every row's total), *nchains = chains.  Counted after every launch from the value
 * ring (klara.jl_amd/csrc/klara_marg.h); this call only reads.  comm = NULL: this handle's chains only; otherwise collective: every rank calls it, on handles
 * of the same ndims (a rank that fails the argument and state checks above returns before the collectives, as with the other gather calls).  First an integer
 * maximum all-reduce over nbins and the bit patterns of lo and hi and their complements, which every rank enters and waits for: ranks whose (nbins, lo, hi)
 * differ then ALL return KLARA_ERR_STATE, before anything whose length depends on nbins is exchanged.  Otherwise the counts merge by one 64-bit integer sum
 * all-reduce.  Any output pointer may be NULL.  Before the first saved sample: zeros.  klara_set_state and klara_reset clear the counts. */
#define KLARA_MARG_MAX_BINS 1024
klara_status klara_gather_histogram(klara_handle* h, klara_comm* comm, uint64_t* counts, uint64_t* nsamples, uint64_t* nchains);

/* Quantiles from such counts: pure host code, no device — the one statement of the rule for C, Python and Julia callers.  counts is ndims x (nbins + 2) as
 * above, lo and hi ndims each, probs nprobs values in (0, 1], out ndims x nprobs row-major.  Per dimension, n = the row's total and w = (hi - lo) / nbins:
 *   k = max(1, ceil(p n));  b = the first slot whose cumulative count reaches k;
 *   b = 0: -inf;  b = nbins + 1: +inf;  otherwise  (lo + (b - 1) w) + w (k - cum_before) / count_b.
 * A range chosen badly shows up as infinities and as the two outer counts, never as a silently clipped number.  n = 0: NaN.
 * KLARA_ERR_INVALID_ARG for a NULL argument, ndims < 1, nbins outside 1..KLARA_MARG_MAX_BINS, nprobs < 1 or a p outside (0, 1]. */
klara_status klara_histogram_quantiles(const uint64_t* counts, int32_t ndims, int64_t nbins, const double* lo, const double* hi, int32_t nprobs,
                                       const double* probs, double* out);

/* ---- Derived quantities (klara_desc.derived_src / derived_nout = K > 0; a job without them: KLARA_ERR_STATE from the calls below).  Every pooled diagnostic
 * of the coordinates, applied to the K outputs of the user's klara_user_derived: the calls hand the per-chain sums dsum / dsumsq (klara_desc.derived_src) to
 * the very reductions klara_gather_moments, klara_gather_rhat (split = 0) and klara_gather_histogram run — the same kernels, the same between-rank merge —
 * with K where those have ndims.  No history of the derived values is kept: nothing that needs one (per-chain ESS, split R-hat, pooled ESS, covariance).
 * Before the first saved sample: zeros or NaN and KLARA_OK, as their counterparts.  The calls only read the job's state. */
/* the per-chain running sums: sum and sumsq nchains x K row-major (either may be NULL), *nsaved_out = saved steps consumed */
klara_status klara_get_derived_sums(klara_handle* h, double* sum, double* sumsq, int64_t* nsaved_out);
/* klara_gather_moments over the outputs: mean[K], m2[K] = sum (y - mean)^2 over all saved samples of all chains, *nsamples = chains x saved steps */
klara_status klara_gather_derived_moments(klara_handle* h, klara_comm* comm, double* mean, double* m2, uint64_t* nsamples, uint64_t* nchains);
/* klara_gather_rhat's plain (unsplit) form over the outputs: rhat, mean, wsum, bsum K each */
klara_status klara_gather_derived_rhat(klara_handle* h, klara_comm* comm, double* rhat, double* mean, double* wsum, double* bsum, uint64_t* nchains,
                                       int64_t* nper);
/* klara_gather_histogram over the outputs (needs derived_nbins > 0, else KLARA_ERR_STATE): counts K x (derived_nbins + 2), the slot rule stated there with
 * lo = derived_lo[k], hi = derived_hi[k]; klara_histogram_quantiles turns the table into quantiles.  With a communicator the ranks' (derived_nbins, lo, hi)
 * are compared first, as there. */
klara_status klara_gather_derived_histogram(klara_handle* h, klara_comm* comm, uint64_t* counts, uint64_t* nsamples, uint64_t* nchains);
/* Compile `src` as a derived-quantity closure for gfx950 exactly as klara_create would for ndims and nout outputs, without a handle and without a GPU.
 * KLARA_OK or KLARA_ERR_COMPILE (the log in klara_compile_log; a source without the function names klara_user_derived there); ndims outside 1..1024 or nout
 * outside 1..KLARA_DERIVED_MAX_OUT: KLARA_ERR_INVALID_ARG. */
klara_status klara_check_derived(const char* src, int32_t ndims, int32_t nout);
/* Self-test hook, no device needed: the geometry of the derived-quantity kernel for (nchains, ndims, nout) — a function of those three alone
 * (klara.jl_amd/csrc/klara_derived.h): chains per workgroup, doubles per LDS row, threads per workgroup, workgroups, LDS bytes.  Any output may be NULL.
 * KLARA_ERR_INVALID_ARG for nchains <= 0, ndims outside 1..1024, nout outside 1..KLARA_DERIVED_MAX_OUT. */
klara_status klara_selftest_derived_plan(int64_t nchains, int32_t ndims, int32_t nout, int32_t* chains_per_wg, int32_t* stride, int32_t* threads,
                                         int64_t* workgroups, int64_t* lds_bytes);
/* Self-test hook: the derived-quantity kernel on a caller's value history.  hist holds ncols (>= 1) saved steps of nchains x ndims values (column t at
 * hist + t * nchains * ndims); it is fed launch by launch through the launch function the job path uses — launch j brings splits[j] >= 0 saved steps, the
 * splits sum to ncols; a launch of more than 32 columns goes in pieces, as in a job — starting from zeroed accumulators.  sum, sumsq: nchains x nout, read
 * back as klara_get_derived_sums reads them; values (may be NULL; not NULL compiles the kernel with staging on): ncols x nchains x nout, the staged outputs.
 * data may be NULL when ndata = 0.  KLARA_ERR_INVALID_ARG (before any HIP call or compilation) for a NULL hist, splits, src, sum or sumsq, nchains <= 0,
 * ndims outside 1..1024, nout outside 1..KLARA_DERIVED_MAX_OUT, ncols < 1, ndata < 0 or data missing, a negative split or splits that do not sum to ncols. */
klara_status klara_selftest_derived(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t nsplits,
                                    const int64_t* splits, const char* src, int32_t nout, const double* data, int64_t ndata, double* sum, double* sumsq,
                                    double* values);

/* Memory-safety aid (tests only).  With KLARA_DEBUG_CANARY=1 in the environment every device array the library allocates lies between
 * two 4 KiB canaries of a signalling-NaN pattern; klara_destroy returns KLARA_ERR_STATE when a kernel of the job wrote into one, and this
 * call checks the canaries of everything alive: *nalloc = arrays checked, *ncorrupt = arrays whose canaries were damaged (they are
 * repaired, so a damage is reported once).  poke != 0 first stores 8 bytes right behind the largest live array — the proof that the
 * check fires.  KLARA_ERR_STATE when the canaries are not enabled. */
klara_status klara_selftest_canary(int32_t poke, int64_t* nalloc, int64_t* ncorrupt);

/* one chain of the stored history in Klara's NState layout: value[d + D*i], i = saved step
 * (BasicContMuvParameterNState.jl:89-119); requires KLARA_MON_HISTORY.  With klara_desc.hist_ring_cols > 0 the columns are the
 * last min(saved, hist_ring_cols) saved steps, oldest first, and *ncols_out is that count (klara_get_chain_fields and
 * klara_get_chain_likelihood_prior likewise); klara_saved_steps tells how many steps have been saved in all. */
klara_status klara_get_chain(klara_handle* h, int64_t local_chain, double* value, int64_t capacity_cols,
                             int64_t* ncols_out);
/* the other monitored NState fields of one chain (BasicContMuvParameterNState.jl:1-21): logtarget[i] (n values,
 * KLARA_MON_HIST_LT) and gradlogtarget[d + D*i] (KLARA_MON_HIST_GRAD); either pointer may be NULL. */
klara_status klara_get_chain_fields(klara_handle* h, int64_t local_chain, double* logtarget,
                                    double* gradlogtarget, int64_t capacity_cols, int64_t* ncols_out);
/* loglikelihood[i] and logprior[i] of one chain over the saved steps (KLARA_MON_HIST_LLLP); either pointer may be NULL */
klara_status klara_get_chain_likelihood_prior(klara_handle* h, int64_t local_chain, double* loglikelihood, double* logprior,
                                              int64_t capacity_cols, int64_t* ncols_out);
/* Monte Carlo variance of every (chain, dimension) series of the stored history, computed on device
 * (src/stats/variance/mcvar.jl): iid (:5), batch means with `batchlen` (:35-41), Geyer's initial monotone sequence
 * estimator up to `maxlag` (<= 0: n-1) (:75-105).  Each output is nchains x ndims or NULL; requires KLARA_MON_HISTORY.
 * ess = n * iid / imse and iact = imse / iid (src/stats/convergence/{ess,iact}.jl:3) follow on the host. */
klara_status klara_get_chain_mcvar(klara_handle* h, int64_t batchlen, int64_t maxlag, double* mcvar_iid,
                                   double* mcvar_bm, double* mcvar_imse);
/* Streaming form of mcvar(v, Val{:imse}, maxlag) / mcvar(v, Val{:ipse}, maxlag) (mcvar.jl:75-105, 137-158) for klara_desc.acov_maxlag > 0
 * (maxlag = acov_maxlag): the empirical autocovariances autocov(v, 0:maxlag) (StatsBase, demean = true) of every series are
 * formed exactly from the lagged cross-products, the first and the last maxlag samples and the total, all kept while sampling
 * (3 (maxlag + 1) doubles per series), then Geyer's truncation.  Each output is nchains x ndims or NULL.  Also available post hoc
 * from a stored history: klara_get_chain_mcvar (imse) and klara_get_chain_mcvar_ipse. */
klara_status klara_get_chain_acov_mcvar(klara_handle* h, double* mcvar_imse, double* mcvar_ipse, int64_t* nsamples_out);
/* Geyer's initial positive sequence estimator over the stored history (mcvar.jl:137-158), maxlag <= 0: n - 1 */
klara_status klara_get_chain_mcvar_ipse(klara_handle* h, int64_t maxlag, double* mcvar_ipse);
/* Zero-variance control variates lzv / qzv (src/stats/variance/zv.jl:9-84, Mira, Solgi & Imparato 2013) of EVERY chain over the stored
 * value and gradlogtarget histories (KLARA_MON_HISTORY | KLARA_MON_HIST_GRAD, no ring, >= 2 saved steps: else KLARA_ERR_STATE).
 * z = -gradlogtarget / 2; the control variates f are z (order 1, K = ndims) or z_i | 2 z_i x_i - 1 | x_i z_j + x_j z_i, i < j
 * (order 2, K = ndims (ndims + 3) / 2); the coefficients solve  S_ff a = -S_fx  with the centred cross-products of the chain
 * (zv.jl: a[:, i] = -inv(cov(f)) cov(f, x_i)) by Cholesky on the device; the corrected series is x + f a.  K > KLARA_ZV_MAX_TERMS:
 * KLARA_ERR_UNSUPPORTED.  pooled != 0: one coefficient matrix from the concatenation of all chains' samples of this handle; zv_mean and
 * zv_var stay per chain.  info: 0, 1 (a Cholesky pivot was not a positive finite number, e.g. a chain that never moved), 2 (fewer than
 * K + 2 samples); in both cases the chain's outputs are NaN and the call still returns KLARA_OK. */
#define KLARA_ZV_LINEAR 1
#define KLARA_ZV_QUADRATIC 2
#define KLARA_ZV_MAX_TERMS 128
klara_status klara_get_chain_zv(klara_handle* h, int32_t order, int32_t pooled,
                                double* coef,     /* per chain: nchains x K x D row-major, coef[c][k][i] = a[k, i]; pooled: K x D; may be NULL */
                                double* zv_mean,  /* nchains x D, may be NULL */
                                double* zv_var,   /* nchains x D, may be NULL */
                                int32_t* info,    /* nchains (pooled: every entry the same), may be NULL */
                                int64_t* nsamples_out);
/* chain + f * a of one chain in NState layout (D x n), zv.jl's first return value; coef NULL: the chain's own coefficients, else K x D given (e.g. the pooled ones) */
klara_status klara_get_chain_zv_series(klara_handle* h, int64_t local_chain, int32_t order, const double* coef,
                                       double* value, int64_t capacity_cols, int64_t* ncols_out);
/* lzv(s) / qzv(s) of ONE chain, both of zv.jl's return values from one fit: its own coefficients (coef: K x D row-major), info (0, 1, 2 as above) and
 * the corrected series (value: NState layout, D x n); each of coef, info, value may be NULL */
klara_status klara_get_chain_zv_one(klara_handle* h, int64_t local_chain, int32_t order, double* coef, int32_t* info,
                                    double* value, int64_t capacity_cols, int64_t* ncols_out);
/* Streaming form of mcvar(v, Val{:bm}) (src/stats/variance/mcvar.jl:35-41: batchlen * var(batch means) / (nbatches *
 * batchlen)) for klara_desc.bm_batchlen > 0: batch means are formed from the running sums at every batch boundary and
 * their mean / sum of squared deviations are updated in place (Welford), so no history is stored — 3 x nchains x ndims
 * doubles however long the run.  mcvar_bm is nchains x ndims (NaN while fewer than two batches are closed). */
klara_status klara_get_chain_bm(klara_handle* h, double* mcvar_bm, int64_t* nbatches_out);
/* saved (post-burn-in, thinned) steps so far */
klara_status klara_saved_steps(klara_handle* h, int64_t* nsaved_out);
/* tuner state per chain (tuners.jl:5-10). In pooled mode every chain reports the shared state. */
klara_status klara_get_tune(klara_handle* h, double* step, int64_t* accepted, int64_t* proposed,
                            int64_t* totproposed);
/* dual-averaging state per chain (DualAveragingMCTune: eps_bar, h_bar); KLARA_TUNER_DUAL_AVERAGING only */
klara_status klara_get_dual_averaging(klara_handle* h, double* epsbar, double* hbar);
/* KLARA_SAMPLER_RAM: the chains' current factors, nchains x D x D row-major, lower triangular with zeros above the diagonal, and the
 * number of factor updates skipped since klara_set_state / klara_reset because a pivot or z . z was not a finite positive number
 * (0 in exact arithmetic).  Either pointer may be NULL.  KLARA_ERR_INVALID_ARG on a handle of another sampler. */
klara_status klara_get_ram_factor(klara_handle* h, double* S, int64_t* skipped);
/* KLARA_SAMPLER_RAM: per-chain factors for a warm start (nchains x D x D row-major, the lower triangles are read); the transition
 * count is kept.  A diagonal entry that is not a finite positive number: KLARA_ERR_INVALID_ARG; before klara_set_state: KLARA_ERR_STATE. */
klara_status klara_set_ram_factor(klara_handle* h, const double* S);
/* KLARA_SAMPLER_AM: the chains' current covariances C (nchains x D x D row-major, full symmetric), running means lastmean and secondlastmean
 * (nchains x D each), and the number of transitions since klara_set_state / klara_reset at which corescale C did not factor and the chain
 * proposed from the minor component instead.  Any pointer may be NULL.  KLARA_ERR_INVALID_ARG on a handle of
 * another sampler. */
klara_status klara_get_am_state(klara_handle* h, double* C, double* lastmean, double* secondlastmean, int64_t* fallbacks);
/* KLARA_SAMPLER_AMWG: the chains' current log proposal scales (nchains x D), the accepted proposals of the current tuning window per coordinate
 * (nchains x D int32) and the accepted proposals per coordinate since klara_set_state / klara_reset (nchains x D uint64).  Any pointer may be NULL.
 * KLARA_ERR_INVALID_ARG on a handle of another sampler; before klara_set_state: KLARA_ERR_STATE. */
klara_status klara_get_amwg_state(klara_handle* h, double* logsigma, int32_t* accepted, uint64_t* naccept_coord);
/* KLARA_SAMPLER_AMWG: per-chain log proposal scales for a warm start (nchains x D, all finite, else KLARA_ERR_INVALID_ARG); the transition count,
 * the window counts and the schedule are kept.  Before klara_set_state: KLARA_ERR_STATE. */
klara_status klara_set_amwg_logsigma(klara_handle* h, const double* logsigma);
/* KLARA_SAMPLER_AMWG with KLARA_MON_ACCEPT: one uint32 per transition and chain, step-major like klara_get_accept_mask, bit i set where coordinate i
 * moved (D <= 32).  *nsteps_out receives the number of recorded steps.  Without the monitor: KLARA_ERR_STATE. */
klara_status klara_get_amwg_accept_mask(klara_handle* h, uint32_t* mask, int64_t capacity_steps, int64_t* nsteps_out);
/* KLARA_SAMPLER_MH_COV: the job's current proposal factor L, D x D row-major, lower triangular with zeros above the diagonal — what the descriptor or the
 * last klara_set_mh_factor gave.  KLARA_ERR_INVALID_ARG on a handle of another sampler. */
klara_status klara_get_mh_factor(klara_handle* h, double* L);
/* KLARA_SAMPLER_MH_COV: a new proposal factor (D x D row-major, the lower triangle is read: every entry finite, the diagonal positive, else
 * KLARA_ERR_INVALID_ARG), in effect from the next transition; the states, the transition count and the monitors are kept.  Like the other setters it
 * waits for the transitions a klara_run_async has queued before it writes.  Changing the proposal from the chains' own past is an adaptation step: the
 * samples that are kept belong behind it.  klara_reset puts klara_desc.mh_factor back. */
klara_status klara_set_mh_factor(klara_handle* h, const double* L);

/* Measurement: duration (ms, HIP events on the launch stream) and launch count of the transition
 * kernels enqueued by the last klara_run / klara_run_async (after synchronisation). */
klara_status klara_last_run_ms(klara_handle* h, double* kernel_ms, int64_t* nlaunches);

/* Raw device pointers of the state (for zero-copy consumers on the same device, e.g. a torch tensor
 * wrapper or an RCCL gather): x, logtarget, gradlogtarget.  Library keeps ownership. */
klara_status klara_device_ptrs(klara_handle* h, void** x, void** logtarget, void** gradlogtarget);

/* The lane layout the kernels use for this handle (needed by the CPU oracle to sum in the same
 * order): kind 0 = contiguous E elements per lane over G lanes; kind 1 = MFMA-transposed layout
 * (element i on lane-quarter i%4); kind 2 = logistic row split (every lane holds all E elements, the data
 * rows are dealt round-robin to `lanes_per_chain` lanes); kind 3 = pair-transposed layout of the diagonal Gaussian
 * (element pair P = i/2 on lane P % lanes_per_chain, elements_per_lane/2 pairs per lane; 8, 16, 32 or 64 lanes per chain for D <= 128 / 256 / 512 / 1024); kind 4 = hierarchical target
 * with few lanes per chain (unit r on lane r / (elements_per_lane/2), hyper block replicated); kind 5 = logistic regression on the matrix cores
 * (elements as in kind 1; data row r on lane-quarter r % 4: row sums are lane partials over ascending rows, then (q0 + q1) + (q2 + q3); X p and
 * X' (y - 1/(1+exp(-Xp))) are fma chains over ascending columns / rows); kind 6 = dense Gaussian beyond D = 256 on a workgroup of `lanes_per_chain`
 * WAVEFRONTS per tile of 16 chains (`elems_per_lane` = 16, 24 or 32: the elements of a lane's column a wavefront can own) (element i on lane-quarter i % 4 of the wavefront that owns row tile i / 16 — the ceil(D / 16) tiles dealt evenly,
 * consecutive tiles each, the first ceil(D/16) % W wavefronts one more —; lane partials in ascending order, (q0 + q1) + (q2 + q3) inside a wavefront, then
 * the wavefronts in ascending order).  See DESIGN.md section 3. */
klara_status klara_get_layout(klara_handle* h, int32_t* kind, int32_t* lanes_per_chain,
                              int32_t* elems_per_lane);

/* Registers, scratch and static LDS of the transition kernel this handle launches for a launch of `nsteps` transitions (1 selects the
 * one-transition-per-launch instantiation where one exists), read from the loaded code object — no launch happens.  which = 0: the
 * kernel a launch runs (for jobs that two kernel families can run, see klara_desc.sparse_moves: the 4-lane one), 1: the 8-lane
 * sibling of such jobs (the same kernel as 0 otherwise).  bench.py checks the committed PMC summaries against these values, so that
 * counters collected on an older build of a kernel are not silently combined with timings of the current one. */
/* Shader clock (MHz) the device ran at during the handle's last launch of a pair-transposed kernel (layout kind 3): one workgroup in
 * the middle of the grid stores the shader-cycle counter and the constant-rate wall clock when it starts and when it ends; 0 when the
 * handle runs other kernels or has not launched yet.  An MI355X clocks between ~1.9 and 2.4 GHz depending on the power the instruction
 * mix draws: a kernel's issue-cycle budget (bench.py roofline) is only comparable with elapsed time at the clock that was actually
 * running.  Synchronises the handle's streams. */
klara_status klara_get_shader_clock(klara_handle* h, double* mhz);
klara_status klara_get_kernel_attributes(klara_handle* h, int32_t which, int32_t nsteps, int32_t* vgprs, int32_t* scratch_bytes,
                                         int32_t* static_lds_bytes);

/* How the launches of this handle were issued so far (layout kind 3 jobs that both kernel families can run, see
 * klara_desc.sparse_moves; zeros otherwise): counts[0] = launches issued as the 4-lane kernel alone, counts[1] = as the 8-lane
 * kernel alone, counts[2] = as a device-decided pair; last_mode[j] / last_accepted[j] = decision (0: 4 lanes, 1: 8 lanes) and
 * accepted proposals the most recent completed launch of chain partition j < 4 left behind (-1 when not available).  Never
 * synchronises: the per-partition values are read from host-visible memory and may lag the device. */
klara_status klara_get_launch_modes(klara_handle* h, int64_t counts[3], int32_t last_mode[4], int64_t last_accepted[4]);

/* Self-test hook: writes nblocks Philox4x32-10 blocks produced by rocRAND's device engine
 * (rocrand_device::philox4x32_10_engine, seed/subsequence/offset = 4*first_block) into out[4*nblocks];
 * tests compare this with the library's own in-kernel generator and with the CPU oracle. */
klara_status klara_selftest_rocrand_blocks(int32_t device, uint64_t seed, uint64_t subsequence,
                                           uint64_t first_block, int32_t nblocks, uint32_t* out);
/* Self-test hook: evaluates the deterministic device math (log, exp, sincos2pi, normal pair) on n
 * inputs so tests can compare bits with the CPU build of the same header. op: 0 log, 1 exp,
 * 2 sin2pi, 3 cos2pi, 4 sqrt, 5 div (in[i] / in2[i]), 6 erf, 7 log_u01 (log of a positive normal number),
 * 8 sqrt of a Box-Muller radicand (positive normal numbers in [1e-16, 1e2]);
 * 13 / 14 sin / cos of the 20-bit Box-Muller angle with index in[i] (an integer in [0, 2^20)) through the LDS remainder table the transition kernels use,
 * 15 / 16 the same angle in the arithmetic form. */
klara_status klara_selftest_math(int32_t device, int32_t op, int64_t n, const double* in,
                                 const double* in2, double* out);

/* Self-test hook: the proposal normals exactly as the transition kernels draw them — kd_normal_pair_w on both halves of the stream block
 * (seed, chain first_chain + i, transition t, slot 0), i.e. the pair indices 0 and 8 of a transition — counted on the device: counts[k] = number of the
 * 4 * nchains * ntransitions normals with |z| > thr[k] (nthr <= 8); moments (may be NULL) = sum z, sum z^2, sum z^4, max |z|.
 * Tests compare the counts with the CPU build of the same generator (exactly) and with the normal tail mass (statistically). */
klara_status klara_selftest_normal_tail(int32_t device, uint64_t seed, uint64_t first_chain, int64_t nchains,
                                        int64_t ntransitions, int32_t nthr, const double* thr, uint64_t* counts,
                                        double* moments);

/* Self-test hook: the D proposal normals of transition `transition` of chains first_chain .. first_chain + nchains - 1 exactly as the samplers draw
 * them (kd_normal_pair_at: element pair p <- half (p >> 3) & 1 of block slot (p & 7) + 8 (p >> 4)), z[nchains x ndims] row-major, and the
 * transition's accept uniform (block slot ceil(ndims / 2)), accept_u[nchains] (may be NULL).  The joint-law tests of the stream — chi-square of
 * a transition's sum z^2, independence of the two pairs that share a block and of a pair's radius and angle bits — run on this output, and
 * the CPU build of the same generator (oracle ko_transition_normals) must return the same bits. */
klara_status klara_selftest_transition_normals(int32_t device, uint64_t seed, uint64_t first_chain, int64_t nchains,
                                               uint64_t transition, int32_t ndims, double* z, double* accept_u);

/* Self-test hook: D(16x16) = A(16x4) * B(4x16) + C(16x16), all row-major, through ONE
 * v_mfma_f64_16x16x4_f64 — pins the instruction's accumulation order for the dense-target parity. */
klara_status klara_selftest_mfma_f64(int32_t device, const double* A, const double* B, const double* C,
                                     double* D);

/* One v_mfma_f64_4x4x4_4b with raw per-lane operands (64 doubles each): A_b[i][k] on lane 16k + 4b + i, B_b[k][j] on
 * lane 16k + 4b + j, C/D_b[i][j] on lane 16i + 4b + j.  Pins the lane layout and the accumulation order the dense
 * kernel's 4-row tail tile relies on (klara_dense.h). */
klara_status klara_selftest_mfma_f64_4x4x4(int32_t device, const double* A, const double* B, const double* C,
                                           double* D);

/* Self-test hook: the chain statistics kernels on a caller's series.  hist holds ncols (>= 2) saved steps of nchains x ndims series as the device keeps a
 * value history (column t at hist + t * nchains * ndims).  Post-hoc estimators over the whole history (what klara_get_chain_mcvar / _ipse run) with lag
 * window maxlag (1..127) and batch length batchlen: iid, bm, imse, ipse; and the streaming autocovariance path (what a job with klara_desc.acov_maxlag =
 * maxlag runs after every launch, then klara_get_chain_acov_mcvar) fed launch by launch — launch j brings splits[j] saved steps, the splits sum to ncols:
 * stream_imse, stream_ipse.  Every output is nchains x ndims and may be NULL.  Tests compare them with exact rational arithmetic. */
klara_status klara_selftest_chain_stats(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t maxlag,
                                        int64_t batchlen, int32_t nsplits, const int64_t* splits, double* iid, double* bm, double* imse,
                                        double* ipse, double* stream_imse, double* stream_ipse);

/* Self-test hook: the across-chain reductions on a caller's per-chain running sums, through the launch functions klara_get_pooled_summaries and
 * klara_gather_moments use.  sum, sumsq and X are nchains x ndims (ndims 1..1024), held and naccept nchains: chain c's sums over its nsaved (>= 0) saved
 * steps are sum + held x and sumsq + held x^2 (held = 0: as stored).
 * (a) over all chains: pooled_sum, pooled_sumsq (ndims each; with_sums = 0 leaves the device's sum slots untouched: they start as the values these two
 * arrays hold on entry and are handed back as they are), accept_total, and the pooled moments mean, m2 (ndims each).
 * (b) the chains cut into nranks shards, rank r owning [bounds[r], bounds[r + 1]) with 0 = bounds[0] < ... < bounds[nranks] = nchains: every shard's
 * moments staged as klara_gather_moments stages them, then that call's own between-rank merge — the one sequence the communicator path runs, over one
 * staging buffer per simulated rank — with each all-reduce replaced by a host sum over the ranks in ascending order starting from zero, written back to
 * every rank; read from rank 0: ranks_mean, ranks_m2 (ndims each), ranks_counters[3] = accept total, saved samples, chains.
 * Every output may be NULL.  KLARA_ERR_INVALID_ARG (before any launch) for a NULL input, nchains <= 0, ndims outside 1..1024, nsaved < 0 or bad bounds.
 * Tests compare the outputs bit for bit with a restatement of the order of operations and with exact rational arithmetic. */
klara_status klara_selftest_pooled(int32_t device, int64_t nchains, int32_t ndims, int64_t nsaved, const double* sum, const double* sumsq,
                                   const double* X, const int64_t* held, const uint64_t* naccept, int32_t nranks, const int64_t* bounds,
                                   int32_t with_sums, double* pooled_sum, double* pooled_sumsq, uint64_t* accept_total, double* mean, double* m2,
                                   double* ranks_mean, double* ranks_m2, uint64_t* ranks_counters);

/* Self-test hook: the pooled covariance kernels on a caller's value history.  hist holds ncols (>= 1) saved steps of nchains x ndims values as the device
 * keeps a value history (column t at hist + t * nchains * ndims), ndims 1..KLARA_COV_MAX_DIMS; it is fed launch by launch through the launch functions the
 * job path uses — launch j brings splits[j] saved steps (0..32 each), the splits sum to ncols — then finalized as klara_gather_covariance does:
 * (a) over all chains: mean (ndims), m2 (ndims x ndims).
 * (b) the chains cut into nranks shards, rank r owning [bounds[r], bounds[r + 1]) with 0 = bounds[0] < ... < bounds[nranks] = nchains: every shard accumulated
 * and finalized on its own (its pivot is its own first chain's first sample), then klara_gather_covariance's own between-rank merge (the same sequence, in
 * its ndims x ndims form) with each all-reduce replaced by a host sum over the ranks in ascending order starting from zero, written back to every rank;
 * read from rank 0: ranks_mean (ndims), ranks_m2 (ndims x ndims), ranks_counters[2] = saved samples, chains.
 * Every output may be NULL.  KLARA_ERR_INVALID_ARG (before any launch) for a NULL input, nchains <= 0, ndims outside 1..KLARA_COV_MAX_DIMS, ncols < 1, a
 * split outside 0..32, splits that do not sum to ncols or bad bounds. */
klara_status klara_selftest_covariance(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t nsplits,
                                       const int64_t* splits, int32_t nranks, const int64_t* bounds, double* mean, double* m2, double* ranks_mean,
                                       double* ranks_m2, uint64_t* ranks_counters);

/* Self-test hook: the marginal histogram kernel on a caller's value history.  hist holds ncols (>= 1) saved steps of nchains x ndims values as the device
 * keeps a value history (column t at hist + t * nchains * ndims), ndims 1..1024; it is fed launch by launch through the launch function the job path uses —
 * launch j brings splits[j] saved steps (0..32 each), the splits sum to ncols — and the table is read back as klara_gather_histogram reads it: counts,
 * ndims x (nbins + 2).  KLARA_ERR_INVALID_ARG (before any HIP call) for a NULL argument, nchains <= 0, ndims outside 1..1024, ncols < 1, nbins outside
 * 1..KLARA_MARG_MAX_BINS, a bound that is not finite, lo >= hi, a split outside 0..32 or splits that do not sum to ncols. */
klara_status klara_selftest_marginals(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t nsplits,
                                      const int64_t* splits, int64_t nbins, const double* lo, const double* hi, uint64_t* counts);

/* Self-test hook, no device needed: the agreement step of klara_gather_histogram over simulated ranks.  Rank r holds nbins[r], lo[r * ndims ..] and
 * hi[r * ndims ..]; every rank's words are formed as that call stages them, the maximum all-reduce is replaced by a host maximum over the ranks, and the
 * verdict every rank reaches is returned: KLARA_OK when all ranks hold the same (nbins, lo, hi) bit for bit, KLARA_ERR_STATE otherwise (-0.0 and 0.0 differ).
 * KLARA_ERR_INVALID_ARG for a NULL argument, nranks < 1 or ndims outside 1..1024. */
klara_status klara_selftest_histogram_ranks(int32_t nranks, int32_t ndims, const int64_t* nbins, const double* lo, const double* hi);

/* Self-test hook: the R-hat kernels on a caller's data, through the launch functions klara_gather_rhat uses.  Unsplit: the per-chain running sums sum,
 * sumsq, X (nchains x ndims, ndims 1..1024) and held (nchains) over nsaved (>= 1) saved steps, as for klara_selftest_pooled; all four NULL: skipped.
 * Split: hist, ncols (>= 2) saved steps of nchains x ndims values (column t at hist + t * nchains * ndims); NULL: skipped.  For each of the two:
 * (a) over all chains; (b) the chains cut into nranks shards, rank r owning [bounds[r], bounds[r + 1]) with 0 = bounds[0] < ... < bounds[nranks] = nchains,
 * every shard staged as klara_gather_rhat stages it, then that call's own between-rank merge with each all-reduce replaced by a host sum over the ranks in
 * ascending order starting from zero.  out, ranks_out (unsplit (a), (b)) and split_out, split_ranks_out: 4 x ndims doubles each, rhat | mean | wsum | bsum;
 * counters[8]: (units, samples per unit) of the four in that order.  Every output may be NULL.  KLARA_ERR_INVALID_ARG (before any launch) for neither
 * input, an incomplete set of sums, nchains <= 0, ndims outside 1..1024, nsaved < 1, ncols < 2 or bad bounds. */
klara_status klara_selftest_rhat(int32_t device, int64_t nchains, int32_t ndims, int64_t nsaved, const double* sum, const double* sumsq,
                                 const double* X, const int64_t* held, int64_t ncols, const double* hist, int32_t nranks, const int64_t* bounds,
                                 double* out, double* ranks_out, double* split_out, double* split_ranks_out, uint64_t* counters);

/* Self-test hook: the pooled effective sample size on a caller's value history hist (ncols >= 2 saved steps of nchains x ndims values, column t at
 * hist + t * nchains * ndims; ndims 1..1024), window maxlag (1..127), through the launch functions and the host estimator klara_gather_ess uses.  Three
 * paths: the streamed state fed launch by launch (nsplits launches of splits[i] >= 0 saved steps, summing to ncols, as klara_selftest_chain_stats), the
 * history mode, and the split mode (skipped when ncols < 8); each (a) over all chains and (b) cut into nranks shards by bounds (as klara_selftest_rhat),
 * merged with every all-reduce replaced by a host sum in ascending rank order.  Slot s = 2 * path + (b): out + s * 5 * ndims: ess | tau | mean | wsum | bsum;
 * rho and csum + s * ndims * (maxlag + 1): ndims x (L + 1) row-major; pairs + s * ndims; counters + 3 * s: units, samples per unit, L.  Every output may be
 * NULL.  KLARA_ERR_INVALID_ARG (before any launch) for a NULL input, nchains <= 0, ndims outside 1..1024, ncols < 2, maxlag outside 1..127, splits that do
 * not sum to ncols or bad bounds. */
klara_status klara_selftest_ess(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t maxlag, int32_t nsplits,
                                const int64_t* splits, int32_t nranks, const int64_t* bounds, double* out, double* rho, double* csum, int32_t* pairs,
                                uint64_t* counters);

/* Self-test hook, no device needed: the verdict of a collective klara_gather_ess over simulated ranks holding units[r] units of n[r] samples and windows
 * lags[r] (0..127): KLARA_OK when all ranks hold the same (n, L), KLARA_ERR_STATE otherwise — L by the maximum over (L, ~L), n by the counters' check. */
klara_status klara_selftest_ess_ranks(int32_t nranks, const int64_t* units, const int64_t* n, const int32_t* lags);

/* Self-test hook, no device needed: the launches a sequence of klara_run calls of the given lengths issues on a fresh job of
 * this descriptor — transitions per launch k[i], the save-rule bookkeeping handed to the kernels (columns already saved,
 * thinning phase of the launch's first post-burn-in transition) and flags (bit 0: a pooled tuner update follows, bit 1: a batch
 * of the streaming batch means closes, bit 2: last launch of its klara_run call).  Launches end after steps_per_launch
 * transitions, at the pooled tuner's events (tuners.jl:27-32) and at batch boundaries, whichever comes first. */
klara_status klara_selftest_plan(const klara_desc* desc, int32_t nruns, const int64_t* run_lengths, int64_t capacity, int64_t* k,
                                 int64_t* save_col0, int32_t* save_phase0, int32_t* flags, int64_t* nlaunches);

/* CUSTOM target: compile `src` for gfx950 exactly as klara_create would for this sampler and dimension, without creating
 * a handle and without needing a GPU (a user checks a closure before submitting a job).  KLARA_OK or KLARA_ERR_COMPILE. */
klara_status klara_check_custom_target(const char* src, int32_t sampler, int32_t ndims);
/* The same for the SMMALA kernels with the softabs transform of the metric (klara_desc.smmala_softabs > 0): the variant klara_create compiles
 * for such a job.  ndims >= 9 is KLARA_ERR_UNSUPPORTED; a source without a metric (klara_user_tensorlogtarget or KLARA_USER_AUTODIFF 2)
 * KLARA_ERR_COMPILE. */
klara_status klara_check_custom_target_softabs(const char* src, int32_t ndims);
/* Compiler output of the calling thread's last klara_create / klara_check_custom_target that compiled a CUSTOM target
 * ("" if none); valid until the thread's next such call. */
const char* klara_compile_log(void);

const char* klara_strerror(klara_status s);
int32_t klara_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KLARA_HIP_H */
