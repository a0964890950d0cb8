/* colnde.h — C ABI of the MI355X-native NDE column-model hot path.
 *
 * The reference (CliMA/ClimateParameterizations.jl, pure Julia) has no FFI for this path: it is reached
 * through Julia closures handed to ODEProblem / OptimizationFunction / Flux.train!.  Each entry
 * point below names the reference closure it replaces (paths relative to /root/reference); INTEGRATION.md
 * shows the `ccall` stubs that give them the reference's names and arities.
 *
 * Conventions: every call returns 0 on success, non-zero on error with colnde_last_error() holding a
 * thread-local message; no exceptions cross the boundary.  One handle = one GPU = one host thread at a
 * time.  Host pointers are borrowed for the duration of the call; device memory is owned by the handle.
 * All arrays are float32, C order.  `weights` is in Flux.destructure order — per net, per Dense layer,
 * column-major vec(W[out x in]) then b — nets concatenated uw; vw; wT
 * (wind_mixing/src/NDE_training.jl:11-21,37).  There is NO CPU fallback: without a visible gfx950 device
 * colnde_create fails.
 */
#ifndef COLNDE_H
#define COLNDE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COLNDE_VERSION 106
#define COLNDE_MAX_LAYERS 8

enum { COLNDE_MODEL_WIND_MIXING = 0,        /* NDE / NDE!: wind_mixing/src/NDE_training.jl:56-165 */
       COLNDE_MODEL_FREE_CONVECTION = 1,    /* FreeConvectionNDE: free_convection/src/free_convection_nde.jl:29-38 */
       COLNDE_MODEL_CONV_ADJ_NDE = 2 };     /* ConvectiveAdjustmentNDE: free_convection/src/convective_adjustment_nde.jl:33-48 */

enum { COLNDE_ACT_IDENTITY = 0, COLNDE_ACT_RELU = 1, COLNDE_ACT_MISH = 2, COLNDE_ACT_SWISH = 3,
       COLNDE_ACT_TANH = 4, COLNDE_ACT_LEAKYRELU = 5 };

enum { COLNDE_ENGINE_AUTO = 0,      /* regtile when the configuration is one it is built for and there are > 8,192 columns, fc32 for its shape, else tile16 (with the net-split kernels where the shape is regtile's) */
       COLNDE_ENGINE_GENERIC = 1,   /* tile16: 16-column MFMA tiles staged through LDS, any layer sizes / model.  Networks whose per-tile activation rows exceed
                                       the CU's 160 KB of LDS — the reference's WIDE wind-mixing architectures, 3 x Chain(Dense(96,400,σ), Dense(400,400,σ),
                                       Dense(400,31)) of wind_mixing/train_NDE.jl:101-102 and train_NDE_args.jl:150-166 (their rows alone are 160 KB) — run
                                       with that one array in a per-workgroup slab of global memory (L2-resident) and the taped weight-gradient path
                                       (colnde_describe: "activation_rows=global_memory"); 3 x (96-400-31) fits the LDS.  Which pipe: for the networks with rows in
                                       global memory the dense chains of the forward and the taped adjoint AND the tape GEMM (dW) follow matrix_arithmetic
                                       (BF16X3_EXACT: pre-split weight planes, v_mfma_f32_16x16x32_bf16; colnde_plan info[7] bits 1-3); every other
                                       tile16 shape runs f32-MFMA forward / adjoint kernels under either arithmetic and only its tape GEMM follows it.
                                       4,096 columns x 32 steps of 3 x (96-400-400-31 swish), fwd + adjoint: 41 ms = 48 algorithmic TFLOP/s
                                       (52 ms under F32_MFMA; profiles/r05_wide_networks.log — bound by the weight stream from L2, not by the pipe). */
       COLNDE_ENGINE_MFMA = 2,      /* regtile: 32 columns per wavefront resident in registers (static 96-50-20-31 wind-mixing
                                       shape; colnde_create fails if the configuration is not covered) */
       COLNDE_ENGINE_FC32 = 3 };    /* fc32: 32-column v_mfma_f32_32x32x2_f32 tiles (16-column v_mfma_f32_16x16x4_f32 tiles up to 4,096 columns)
                                       with compile-time shapes for FreeConvectionNDE (RK4) and ConvectiveAdjustmentNDE (RK4, RKC2) with the
                                       reference's network Dense(Nz,4Nz,relu), Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1)
                                       (free_convection/train_free_convection_nde.jl:119-121), Nz = 32 | 64; AUTO picks it for that
                                       shape; colnde_create fails if it is requested for anything else */

enum { COLNDE_STEPPER_RK4 = 0,      /* classical RK4, `substeps` per save interval (what the bench measures) */
       COLNDE_STEPPER_RKC2 = 1 };   /* stabilised second-order Runge-Kutta-Chebyshev for the stiff variants: `substeps` steps per
                                       save interval of `rkc_stages` stages each (tile16; the net-split latency kernels; fc32 for
                                       ConvectiveAdjustmentNDE).  Stands where the reference uses ROCK4 (wind_mixing/train_NDE.jl:143,
                                       free_convection/test_free_convection_nde.jl:32-35).
                                       GRADIENT CAVEAT: for the models with a convective-adjustment switch (min(0, K dT/dz):
                                       ConvectiveAdjustmentNDE, the wind-mixing `convective_adjustment` branch) the RKC2 gradient is
                                       NOT the exact discrete adjoint — that one is unbounded, the stage Jacobians of one step
                                       differing in their switch patterns — but the pullback with ONE switch pattern per step (that
                                       of the last stage input).  It converges to the sub-stepped RK4 gradient as the step shrinks
                                       (6.5 % / cosine 0.998 at 8 steps per save interval of the 64-level model, 2 % at 16)
                                       and is exact for smooth closures (the Richardson-number branch).  colnde_plan reports it
                                       (info[7] bit 0). */

/* How the Float32 `Dense` products of the reference (W*x, NDE_training.jl:94-96; their transposes and outer products in the gradient) are
 * evaluated on the matrix pipe.  Both are f32 arithmetic: f32 operands, f32 accumulation, no operand rounded.
 *   BF16X3_EXACT (default, = 0): every f32 operand is split EXACTLY into three bf16 parts (x = x_h + x_m + x_l by truncation; 3 x 8 = 24
 *     significant bits) and a product is the six part-products down to 2^-16 on v_mfma_f32_*_bf16 with f32 accumulation; the three dropped
 *     part-products are below 2^-23 |a b| together — one f32 rounding of the product, which an f32 FMA chain commits at every step anyway
 *     (measured: profiles/r03ze_split_error_probe.txt).  Inf/NaN operands give NaN (Inf - Inf in the split), which the solve calls report
 *     as a non-finite loss.  A NaN pre-activation gives a NaN activation for all five activations of the wind-mixing and generic kernels, tanh and
 *     relu included (Flux's own behaviour); the relu of the fc32 free-convection kernels answers 0 to it (DESIGN, "A NaN member").  Subnormals are not flushed (bf16 inputs, f32 results: measured, profiles/r04_split_edge_probe.txt), but the part of an
 *     operand below 2^-133, the smallest bf16 subnormal, is dropped: operands are exact for |x| >= 2^-110 and carry an ABSOLUTE error below 2^-133
 *     (9e-41) under that — F32_MFMA keeps full relative precision down to FLT_MIN.
 *     Used where a split kernel exists (colnde_plan info[7] says which kernels ran on it); the other kernels run F32_MFMA.
 *   F32_MFMA (= 1): v_mfma_f32_32x32x2_f32 / 16x16x4_f32 throughout (bitwise an fmaf chain; 1/16 of the bf16 pipe's rate).
 * Test overrides (read when the arithmetic is resolved: colnde_create, colnde_set_matrix_arithmetic): COLNDE_FWD_SPLIT / COLNDE_ADJ_SPLIT /
 * COLNDE_DW_SPLIT = 0 | 1 force the forward-solve / adjoint / weight-gradient-GEMM kernels individually. */
enum { COLNDE_MATRIX_BF16X3_EXACT = 0, COLNDE_MATRIX_F32_MFMA = 1 };

/* Mirrors the `constants`, `scalings`, `conditions` NamedTuples of prepare_parameters_NDE_training
 * (wind_mixing/src/NDE_training.jl:1-44, :205-207) and the parameter tail of the free-convection NDEs
 * (free_convection/src/free_convection_nde.jl:49-62). */
typedef struct colnde_config {
    int32_t model;                               /* COLNDE_MODEL_* */
    int32_t Nz;                                  /* cells per column; state = 3*Nz (wind mixing) or Nz */
    int32_t n_layers;                            /* Dense layers per net */
    int32_t layer_sizes[COLNDE_MAX_LAYERS + 1];  /* in, h1, ..., out (= Nz-1 interior faces) */
    int32_t activations[COLNDE_MAX_LAYERS];      /* COLNDE_ACT_* per layer */
    int32_t modified_pacanowski_philander;       /* conditions.* */
    int32_t convective_adjustment;
    int32_t zero_weights;
    int32_t smooth_NN;
    int32_t smooth_Ri;
    int32_t diurnal;                             /* bcs[5] then holds Q^b; wT_top(t) as NDE_training.jl:73 */
    int32_t train_gradient;
    int32_t inplace_variant;                     /* NDE! arithmetic of training_postprocessing.jl:105-153 */
    float H, tau, f, g, alpha, nu0, nu_minus, Ric, dRi, Pr, kappa, eps;
    float mu[6];                                 /* scalings u, v, T, uw, vw, wT */
    float sigma[6];
    float ca_K;                                  /* convective_adjustment_nde.jl:43 (10) */
    int32_t n_save;                              /* number of `saveat` times, >= 2 */
    int32_t substeps;                            /* steps per save interval (RK4; RKC2: steps of rkc_stages stages); 0 = chosen from `reltol` by the first solve
                                                    call of the handle (colnde_choose_substeps), then kept */
    const float* save_times;                     /* [n_save] nondimensional t_train ./ tau (borrowed during create) */
    int32_t n_columns;                           /* columns (simulations) held by this handle */
    int32_t device;                              /* HIP device ordinal */
    int32_t engine;                              /* COLNDE_ENGINE_* */
    int32_t stepper;                             /* COLNDE_STEPPER_* (0 = RK4) */
    int32_t rkc_stages;                          /* RKC2: stages per step, 2..256; 0 = automatic (colnde_rkc_stages) */
    int32_t matrix_arithmetic;                   /* COLNDE_MATRIX_* (0 = exact three-way bf16 split where a split kernel exists) */
    float reltol;                                /* the tolerance the reference hands its adaptive integrator (solve(...; reltol=1f-3): NDE_training.jl:291;
                                                    1e-4: free_convection/src/solve.jl:4); 0 = 1e-3.  Used when substeps = 0 and by colnde_choose_substeps:
                                                    see colnde_error_estimate for the norm */
} colnde_config;

typedef struct colnde_handle colnde_handle;

const char* colnde_last_error(void);
int colnde_version(void);

/* Least `substeps` for which the classical-RK4 step stays inside its stability region (|lambda dt| <= 2.785) for the stiffest
 * diffusive mode the configuration can switch on: lambda = -4 D Nz^2 with D = tau (nu0 + nu_minus) max(1, 1/Pr) / H^2
 * (Richardson closure), tau kappa / H^2 (convective-adjustment branches) or (sigma_wT/sigma_T)(tau/H) ca_K
 * (ConvectiveAdjustmentNDE).  The reference sidesteps this with ROCK4 (wind_mixing/train_NDE.jl:143).  colnde_forward / _loss /
 * _loss_grad refuse a configuration below it (instead of returning a blown-up solve with rc = 0) unless
 * COLNDE_ALLOW_UNSTABLE_DT=1; colnde_rhs is not affected.  Returns -1 on an invalid configuration.  No GPU needed. */
int  colnde_min_substeps(const colnde_config* cfg);

/* Stage count an RKC2 configuration runs with: cfg->rkc_stages when given, else the least s >= 2 whose real stability interval
 * beta(s) ~ 0.653 s^2 (damping 2/13), used to 90 %, covers lambda dt of the same stiffest mode.  A given stage count that does
 * not cover it is refused by the solve calls like an unstable RK4 step.  Returns -1 on an invalid configuration. */
int  colnde_rkc_stages(const colnde_config* cfg);

int  colnde_create(const colnde_config* cfg, colnde_handle** out);
void colnde_destroy(colnde_handle* h);
int  colnde_n_params(const colnde_handle* h);
int  colnde_engine(const colnde_handle* h);                  /* engine actually selected */
/* The stream every later call of the handle enqueues on (default: the null stream).  A handle keeps device state from one call to the next that it
 * wrote in stream order without synchronising — the problem of colnde_set_problem_dev, packed operand images, tapes, coefficient tables — so a call with
 * ANOTHER stream first synchronises the stream in use (which must still exist) and returns its error; what the handle did there is then complete before
 * anything is enqueued on the new stream.  The caller's own buffers stay the caller's to order.  A call with the stream already in use costs nothing
 * (a front-end may issue one per call). */
int  colnde_set_stream(colnde_handle* h, void* hip_stream);
/* Switch the matrix arithmetic of an existing handle (COLNDE_MATRIX_*): tapes and results layout do not depend on it, so the same
 * handle can run both for an A/B on identical inputs.  A dW GEMM already planned takes the slice count a fresh handle of the new arithmetic plans (the
 * partial-gradient slab is replaced after the stream has drained), so the results are that handle's bit for bit; if the slab cannot be allocated the call
 * fails and the previous arithmetic and plan stay in force.  colnde_matrix_arithmetic returns the configured value. */
int  colnde_set_matrix_arithmetic(colnde_handle* h, int matrix_arithmetic);
int  colnde_matrix_arithmetic(const colnde_handle* h);
/* Global column count when columns are sharded over ranks: losses and gradients are normalised by it so
 * that a SUM all-reduce of the per-rank results is the global mean (NDE_training.jl:312-317). */
int  colnde_set_global_columns(colnde_handle* h, int64_t n_columns_total);

/* x0 [n_col][n_state], bcs [n_col][n_bc] (wind mixing: uw_b,uw_t,vw_b,vw_t,wT_b,wT_t — the tail of `p`,
 * NDE_training.jl:60; free convection: bottom, top — free_convection_nde.jl:31), truth
 * [n_col][n_save][n_state] or NULL.  Replaces uvT₀s / BCs / uvT_trains (NDE_training.jl:220-243). */
int colnde_set_problem(colnde_handle* h, const float* x0, const float* bcs, const float* truth);

/* One RHS evaluation for n_columns columns — NDE(x,p,t) (NDE_training.jl:56-81), NDE!(dx,x,p,t)
 * (training_postprocessing.jl:131-153), ∂T∂t(T,p,t) (free_convection_nde.jl:29-38). */
int colnde_rhs(colnde_handle* h, const float* x, const float* weights, const float* bcs, float t,
               float* dx, int n_columns);

/* solve(prob, alg; p=[weights;BCs], saveat=t_train) — NDE_training.jl:291,403; training_postprocessing.jl:157;
 * free_convection/src/solve.jl:1-6.  sol [n_col][n_save][n_state] (NULL: keep on device only). */
int colnde_forward(colnde_handle* h, const float* weights, float* sol);

/* ---- what `reltol` means here.  The reference integrates with an ADAPTIVE stepper (solve(prob, ROCK4(); reltol=1f-3, saveat=...): wind_mixing/src/
 * NDE_training.jl:291,304,403; reltol=1e-4: free_convection/src/solve.jl:4); this path steps at a fixed `substeps` per save interval, and the tolerance is
 * enforced a posteriori.  colnde_error_estimate: one more forward solve at 2 x substeps and Richardson's estimate of the error of the solve at `substeps`,
 *   e = (u_S - u_2S) 2^p / (2^p - 1),   *max_rel_err = max over columns and save points of rms_i(e_i / (abstol / reltol + |u_i|))
 * (rms over the state's components) — the integrator's accept test rms(err / (abstol + reltol |u|)) <= 1 with OrdinaryDiffEq's default abstol = 1e-6,
 * divided through by reltol, applied to the whole save interval instead of one adaptive step; +inf when a solve is not finite.  The floor
 * abstol / reltol follows the tolerance in force (cfg.reltol for colnde_error_estimate, the argument for colnde_choose_substeps): 1e-3 at wind mixing's
 * reltol = 1e-3, 1e-2 at free convection's 1e-4.  p is the order the RIGHT-HAND SIDE lets the stepper reach: 4 (RK4) and 2 (RKC2) for smooth closures,
 * 1 (factor 2) for the switching ones — ConvectiveAdjustmentNDE's min(0, K dT/dz) and the wind-mixing convective-adjustment branch converge at about
 * first order through their kinks whatever the stepper (measured: profiles/r05_rkc2_conditioning.json).  colnde_choose_substeps: the least
 * power-of-two sub-step count, not below colnde_min_substeps, whose estimate is <= reltol (reltol <= 0: cfg.reltol); the handle keeps it (call it before
 * the first colnde_loss_grad: the sub-step count sizes the tapes).  A handle created with substeps = 0 does this by itself in its first solve call, with
 * the weights of that call; later calls reuse the count (a training loop re-checks with colnde_error_estimate when it wants to).  colnde_substeps: the
 * count in use.  The stability bound alone (colnde_min_substeps) knows only the closure's diffusion; a trained net's Jacobian shows up here.
 * float32 solves resolve about 1e-4 in this norm (it divides by 1e-3 + |u|; round-off grows with the step count): a tolerance below that floor is
 * refused by colnde_choose_substeps with the floor it found, and the reference's 1e-3 / 1e-4 sit at or above it. */
int colnde_error_estimate(colnde_handle* h, const float* weights, float* max_rel_err);
int colnde_error_estimate_dev(colnde_handle* h, const float* d_weights, float* max_rel_err /* host */);
int colnde_choose_substeps(colnde_handle* h, const float* weights, float reltol, int* substeps /* nullable */, float* estimate /* nullable */);
int colnde_substeps(const colnde_handle* h);
/* Impose a sub-step count.  The column-sharded recipe (one handle per GPU, colnde_set_global_columns): substeps = 0 would let every rank choose from its own
 * columns — the SUM-all-reduced gradient would mix discretisations and the tapes would differ per rank — so a handle that knows it holds a shard REFUSES the
 * automatic choice; instead every rank calls colnde_choose_substeps, the host takes the MAX over ranks (one MAX all-reduce of one integer) and every rank
 * calls colnde_set_substeps with it.  Refused once the gradient path has sized its tapes, and outside the stability bound (colnde_min_substeps).  With the
 * RKC2 stepper and rkc_stages = 0 the stage count follows the new step (the least s with 0.9 beta(s) >= lambda dt), as it does inside
 * colnde_choose_substeps / colnde_error_estimate.  Float32 and the stage count: at a FIXED step, 17 ... 136 stages stand equally far from float64 (the
 * increment-form recurrence is internally stable); what separates float32 from float64 on ConvectiveAdjustmentNDE is the switch, and it shrinks with the
 * STEP, not the stage count — see the table in DESIGN section 2 (tools/rkc_conditioning.py). */
int colnde_set_substeps(colnde_handle* h, int substeps);

/* ---- a step SCHEDULE: the fixed-step form of the adaptive stepper's uneven steps.  One `substeps` serves the whole time axis, so every save interval pays
 * for the most demanding one: the stability bound follows the LONGEST interval, colnde_choose_substeps the worst.  A schedule is n_save - 1 positive counts
 * S_n, the RK4 steps of save interval n — the same for all columns and all members; interval n is stepped with dt_n = (t[n+1] - t[n]) / S_n.  Tapes, slab
 * rows and dW records are sized by the total, sum of S_n.  A handle without a schedule behaves, bit for bit, as it always did, and a schedule whose counts
 * all equal c gives the bits of substeps = c.
 * colnde_schedule_min (no GPU): counts[n_save - 1] = the stability bound of each interval's own length — colnde_min_substeps of the two-point configuration
 *   of that interval (RK4 only).
 * colnde_set_schedule: impose counts[n_save - 1]; NULL clears the schedule (cfg.substeps everywhere again).  Covers the handles whose solves run on the
 *   four-wave net-split kernels (rt16sh_forward_kernel / rt16sh_adjoint_kernel): single wind-mixing handles of the net-split shape under engine AUTO with at
 *   most 8,192 columns, and colnde_create_ensemble handles.  Refused, each with its reason and before any device work: once a single handle's tapes are
 *   planned (the first colnde_loss_grad; an ensemble's tapes, planned at creation, are planned again for the new total, and a total that does not fit is
 *   refused with the old schedule kept); a count below colnde_schedule_min (of an ensemble: below any model's; COLNDE_ALLOW_UNSTABLE_DT=1 overrides), below 1
 *   or above 4096; RKC2 (its stage table depends on dt); regtile (more than 8,192 columns or engine = regtile), tile16 shapes (wide networks, smoothing,
 *   inplace_variant), fc32, conv, closure and free-convection ensemble handles; COLNDE_T16_{FWD,ADJ}_HELPER=0, COLNDE_T16_{FWD,ADJ}_SPLIT=0,
 *   COLNDE_T16_ZTAPE=0, COLNDE_T16_DWTAPE=0.  Clears a pending substeps = 0.  colnde_set_substeps and a successful colnde_choose_substeps on a handle with a
 *   schedule CLEAR the schedule: one count for every interval is what they set.  colnde_error_estimate on such a handle estimates the schedule (against every
 *   interval doubled).
 * colnde_schedule: writes the counts in force (counts nullable; cfg.substeps each without a schedule) and returns their total (-1: null handle).
 * colnde_choose_schedule (single handles; refused on a column shard and once the tapes are planned, as colnde_choose_substeps): starts from
 *   colnde_schedule_min rounded up to powers of two; each round solves at S and at 2 S (every interval doubled) and forms E[n], colnde_error_estimate's norm
 *   at save point n alone (max over columns); stops when max E <= reltol (0: cfg.reltol); otherwise doubles every interval whose own addition
 *   d[n] = max(0, E[n] - E[n-1]) is at least half the largest.  Fails on a non-finite estimate, when max E fell by less than a fifth after a round (the
 *   float32 round-off floor, as colnde_choose_substeps), and when the intervals that carry the error are at 4096 (too stiff).  On success the handle keeps the
 *   schedule; counts / estimate (nullable) receive it and max E. */
int colnde_schedule_min(const colnde_config* cfg, int* counts /* [n_save - 1] */);
int colnde_set_schedule(colnde_handle* h, const int* counts /* [n_save - 1]; NULL clears */);
int colnde_schedule(const colnde_handle* h, int* counts /* [n_save - 1], nullable */);
int colnde_choose_schedule(colnde_handle* h, const float* weights, float reltol, int* counts /* nullable */, float* estimate /* nullable */);

/* predict_flux(uvT, BCs, ...) (wind_mixing/src/NDE_training.jl:83-147; exported at wind_mixing/src/WindMixing.jl:6): the face fluxes whose divergence the
 * RHS takes — uw, vw, wT on the Nz + 1 faces, NN output minus the closure's diffusive flux (MPP) or convective-adjustment flux, boundary faces as the
 * conditions say — for n_columns states: flux [n_col][3][Nz + 1], scaled units.  T-only models: flux [n_col][1][Nz + 1] = [bottom; NN(T); top]
 * (free_convection_nde.jl:33) minus min(0, K dT/dz) for ConvectiveAdjustmentNDE — the wT that the dataset-level solve_nde re-evaluates per saved step
 * (free_convection/src/solve.jl:32-46).  Same arguments as colnde_rhs. */
int colnde_flux(colnde_handle* h, const float* x, const float* weights, const float* bcs, float t, float* flux, int n_columns);
int colnde_flux_dev(colnde_handle* h, const float* d_x, const float* d_weights, const float* d_bcs, float t, float* d_flux, int n_columns);

/* loss_per_tstep(a, b) (wind_mixing/src/loss.jl:44-46) on the six profile matrices of every simulation, as NDE_profile calls it
 * (training_postprocessing.jl:311-316): out [n_col][6][n_save], term order u, v, T, dudz, dvdz, dTdz; entry = mse over the Nz levels (gradient terms:
 * over the Nz + 1 faces, the two zero boundary rows included) of solve(weights) against the truth at that save point, UNSCALED by the loss scalings.
 * T-only models fill terms 2 and 5. */
int colnde_loss_per_tstep(colnde_handle* h, const float* weights, float* out);
int colnde_loss_per_tstep_dev(colnde_handle* h, const float* d_weights, float* d_out);

/* loss_NDE / loss_gradient_NDE value (NDE_training.jl:290-323), nde_loss (training.jl:55-62).
 * scalings[6] = loss_scalings (u,v,T,dudz,dvdz,dTdz); terms[6] = scaled losses; total = their sum. */
int colnde_loss(colnde_handle* h, const float* weights, const float scalings[6], float terms[6], float* total);

/* Value and d(total)/d(weights): replaces Zygote through the sensitivity solve
 * (OptimizationFunction(loss_gradient_NDE, AutoZygote()), NDE_training.jl:327-333; Flux.train!, training.jl:71). */
int colnde_loss_grad(colnde_handle* h, const float* weights, const float scalings[6], float terms[6],
                     float* total, float* grad);

/* compute_neural_network_forcing! (free_convection/double_gyre_nn.jl:149-168): T [n_col][Nz] model units,
 * top_flux [n_col]; out [n_col][Nz] = -dz(wT) on cell centres with dz = Lz/Nz. */
int colnde_infer_forcing(colnde_handle* h, const float* weights, const float* T, const float* top_flux,
                         float Lz, float* out, int n_columns);
/* The same evaluation with the reference's storage convention: compute_neural_network_forcing! fills params.∂z_wT_NN with +dz(wT)
 * (double_gyre_nn.jl:165) and the forcing function negates it (:135).  out [n_col][Nz] = +dz(wT); colnde_infer_forcing returns the forcing itself. */
int colnde_infer_dz_wT(colnde_handle* h, const float* weights, const float* T, const float* top_flux,
                       float Lz, float* out, int n_columns);

/* ---- device-pointer twins: every pointer is device memory on cfg.device; work is enqueued on the
 * handle's stream and NOT synchronised — except where a call has to replace a buffer of the handle, which it does only after the stream has
 * drained: the first solve and the first gradient of a handle (tapes, plans and tables are made then), and a call on more columns than any call
 * before it (scratch and, for the wide networks, the activation rows grow).  d_out of loss_grad_dev has n_params + 8 floats:
 * [grad(n_params); scaled terms(6); total; 0] — the buffer a caller all-reduces (RCCL) when sharded. */
int colnde_set_problem_dev(colnde_handle* h, const float* d_x0, const float* d_bcs, const float* d_truth);
int colnde_rhs_dev(colnde_handle* h, const float* d_x, const float* d_weights, const float* d_bcs, float t,
                   float* d_dx, int n_columns);
int colnde_forward_dev(colnde_handle* h, const float* d_weights, float* d_sol);
int colnde_loss_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out8);
int colnde_loss_grad_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out);
int colnde_infer_forcing_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux,
                             float Lz, float* d_out, int n_columns);
int colnde_infer_dz_wT_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux,
                           float Lz, float* d_out, int n_columns);

/* ---- the steps either side of the hot path --------------------------------------------------------
 *
 * convective_adjustment!(model, Δt, K) — free_convection/double_gyre_nn.jl:27-62 (every (i,j) column of the 3-D model),
 * 1-D twin free_convection/src/oceananigans_nn.jl:13-40: κ_k = K where the centred ∂T/∂z of cell k is negative, 0 elsewhere,
 * then one backward-Euler step T' = L \ T with lower_k = -cκ_k, diag_k = 1 + c(κ_k + κ_{k+1}) (last row 1 + cκ_Nz),
 * upper_k = -cκ_{k+1}, c = Δt/Δz².  T, out: [n_col][Nz] (k = 0 deepest; out may alias T).  halo_bottom / halo_top: [n_col] values
 * of the halo cells below k = 0 / above k = Nz-1 as the ocean model filled them for the field's boundary conditions, or NULL for
 * the zero-gradient fill (nearest interior value).  Nz is the handle's. */
int colnde_convective_adjustment(colnde_handle* h, const float* T, const float* halo_bottom, const float* halo_top, float dt,
                                 float dz, float K, float* out, int n_columns);
int colnde_convective_adjustment_dev(colnde_handle* h, const float* d_T, const float* d_halo_bottom, const float* d_halo_top,
                                     float dt, float dz, float K, float* d_out, int n_columns);

/* modified_pacanowski_philander!(model, constants, Δt, p, convective_adjustment) — wind_mixing/src/NDE_oceananigans.jl:61-101, the implicit
 * diffusion step of the 1-D Oceananigans embedding of the wind-mixing NN (called every time step at :376,:402), with the face
 * diffusivities of modified_pacanowski_philander_diffusivity (:17-58):
 *   Ri_k  = ∂z b / ((∂z u)² + (∂z v)²) on faces, b = gαT (Oceanostics 0.3.2 richardson_number_ccf!, wind_mixing/Manifest.toml:1279)
 *   ν_k   = ν₀ + ν₋ tanh_step((Ri_k − Riᶜ)/ΔRi) on interior faces, 0 on the bottom face;  ν_T = ν/Pr, or under convective_adjustment
 *           Ri_k > 0 ? ν_k/Pr : 1 on every face (the bottom face sees the halo cells; NaN > 0 is false, as in Julia)
 *   u′ = L_ν \ u, v′ = L_ν \ v, T′ = L_νT \ T (backward Euler, the Tridiagonal of :69-83, c = Δt/Δz²), then T′[bottom] = T[bottom] (:94).
 * u, v, T and the outputs: [n_col][Nz] in the ocean model's units, k = 0 deepest; an output may alias its own input.  halo_bottom:
 * [3][n_col] = the u, v, T halo cells below k = 0 as the ocean model filled them for the fields' boundary conditions (only the
 * convective-adjustment switch of the bottom face reads them), or NULL for the zero-gradient fill.  params = {ν₀, ν₋, ΔRi, Riᶜ, Pr, α, g}
 * (the reference's `p` dictionary and `constants`).  Nz is the handle's (any model kind). */
int colnde_implicit_diffusion(colnde_handle* h, const float* u, const float* v, const float* T, const float* halo_bottom, float dt,
                              float dz, const float params[7], int convective_adjustment, float* u_out, float* v_out, float* T_out,
                              int n_columns);
int colnde_implicit_diffusion_dev(colnde_handle* h, const float* d_u, const float* d_v, const float* d_T, const float* d_halo_bottom,
                                  float dt, float dz, const float params[7], int convective_adjustment, float* d_u_out, float* d_v_out,
                                  float* d_T_out, int n_columns);

/* NN_uw_forcing / NN_vw_forcing / NN_wT_forcing (wind_mixing/src/NDE_oceananigans.jl:288-329) as progress_neural_network stores them every
 * iteration of the 1-D embedding (:393-400): the three trained flux networks on an ocean column's u, v, T.  Per column, with
 * x = [(u−μ_u)/σ_u; (v−μ_v)/σ_v; (T−μ_T)/σ_T] and y = net_k(x) (Nz−1 values):
 *   uw, vw (:288-304): a = σ y + μ, interior faces a .− (σ a[1] + μ) — the reference applies inv(scaling) a SECOND time to the already
 *           unscaled first element (`uw .- inv(uw_scaling).(uw[1])`, sic); this is NOT the inv(scaling)(0) of training and is mirrored as written;
 *   wT (:315-329): interior faces σ_wT (y .− y[1]), so the first interior face is exactly 0;
 *   faces [0; interior; top_flux] (:220-224), output in cell k = (F[k+1] − F[k])/Δz (:193-218), Δz = Lz/Nz.
 * u, v, T: [n_col][Nz] in the ocean model's units, k = 0 deepest (as colnde_implicit_diffusion); top_flux: [3][n_col] = uw, vw, wT at the
 * top face in physical units (a diurnal wT_flux(t), :323-329, is passed as its value at t); outputs each [n_col][Nz] = +∂z(flux) — the
 * forcing is its negative (:333, :338, :343) — and may alias nothing.  n_columns is independent of the handle's own column count.  All
 * state and output arrays 16-byte aligned.  No smoothing filter and none of the training `conditions` enter: a handle with smooth_NN is
 * refused, the other flags do not matter.  Single-model wind-mixing handles with Nz = 32 and three 96-50-20-31 networks (any hidden
 * activation, identity output) only; anything else is refused with the reason.  The dense chains run on the f32 matrix pipe under either
 * matrix_arithmetic (colnde_describe: wm_infer=f32); timed under colnde_kernel_time slot 4. */
int colnde_wm_infer_dz_flux_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T,
                                const float* d_top_flux, float Lz, float* d_dz_uw, float* d_dz_vw, float* d_dz_wT, int n_columns);
int colnde_wm_infer_dz_flux(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T, const float* top_flux,
                            float Lz, float* dz_uw, float* dz_vw, float* dz_wT, int n_columns);   /* host arrays; synchronises */

/* progress_neural_network (wind_mixing/src/NDE_oceananigans.jl:380-405) in one launch: the three ∂z arrays above from the state AS GIVEN,
 * then modified_pacanowski_philander! (:61-101; colnde_implicit_diffusion with dz = Lz/Nz) on that state.  halo_bottom, params and
 * convective_adjustment as colnde_implicit_diffusion; u_out, v_out, T_out may each alias its own input, the ∂z arrays nothing. */
int colnde_wm_embedded_step_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T,
                                const float* d_top_flux, const float* d_halo_bottom, float Lz, float dt, const float params[7],
                                int convective_adjustment, float* d_dz_uw, float* d_dz_vw, float* d_dz_wT, float* d_u_out, float* d_v_out,
                                float* d_T_out, int n_columns);
int colnde_wm_embedded_step(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T, const float* top_flux,
                            const float* halo_bottom, float Lz, float dt, const float params[7], int convective_adjustment, float* dz_uw,
                            float* dz_vw, float* dz_wT, float* u_out, float* v_out, float* T_out, int n_columns);

/* What the wind-mixing embedding saves with every state: the TOTAL fluxes uw, vw, wT on the Nz+1 faces (face 0 the bottom), read back as `uw`, `vw`,
 * `wT` by solve_oceananigans_modified_pacanowski_philander_nn and the comparison scripts.  Per column, on u, v, T [Nz] AS GIVEN (ocean units,
 * k = 0 deepest), dz = Lz/Nz:
 *   gradients  g_φ[f] = (φ[f] − φ[f−1])/dz on the Nz+1 faces ((Center, Center, Face) ∂z; :159, :232); the two end faces read the halo cells:
 *              halo_bottom [3][n_col] (u, v, T below k = 0, as colnde_implicit_diffusion) and halo_top [3][n_col] (above k = Nz−1), either NULL =
 *              the zero-gradient fill;
 *   diffusivities of modified_pacanowski_philander_diffusivity (:17-58), exactly those of colnde_implicit_diffusion: ν[f] = ν₀ + ν₋ tanh_step((Ri_f −
 *              Riᶜ)/ΔRi) on faces 1..Nz−1, 0 on both end faces; νT = ν/Pr, or under convective_adjustment Ri_f > 0 ? ν/Pr : 1 on EVERY face, the
 *              ends included (their Ri from the halo cells; with the fill it is 0/0 = NaN and `NaN > 0` is false, as in Julia: νT = 1);
 *   colnde_wm_diagnose_flux — diagnose_NN_flux_uw / _vw / _wT (wind_mixing/src/NDE_oceananigans.jl:226-286): NN faces F = [0; inv(scaling).(y) .−
 *              inv(scaling)(0); top_flux] (:235, :253, :274-276 with enforce_fluxes_* :220-224), y the net's 31 outputs on the scaled [u; v; T] as
 *              colnde_wm_infer_dz_flux evaluates them, each operation of (σ y + μ) − (σ·0 + μ) rounded to float32 — NOT the forcing chain's
 *              convention, which subtracts inv(scaling) of the already unscaled first element (:292, :301), so the ∂z arrays do not integrate to
 *              these faces;  uw = F_uw − ν g_u,  vw = F_vw − ν g_v,  wT = F_wT − νT g_T;
 *   colnde_mpp_diagnose_flux — diagnose_baseline_flux_uw / _vw / _wT (:157-191), the diffusivity-only model: uw = −ν g_u, vw = −ν g_v, wT = −νT g_T,
 *              then the top face REPLACED by top_flux (`uw[end] = uw_flux`), so no halo above is read and the call has no halo_top.  No networks:
 *              any handle kind, every Nz colnde_implicit_diffusion accepts (the handle's Nz), dz given; 16-byte alignment is used when present,
 *              not required;
 *   colnde_wm_embedded_step_flux — colnde_wm_embedded_step and colnde_wm_diagnose_flux of the SAME state as given in one call: the ∂z arrays and
 *              u′, v′, T′ are the bits of colnde_wm_embedded_step_dev, the faces the bits of colnde_wm_diagnose_flux_dev.  One launch that reads
 *              the state once (measured against the two launches in DESIGN §4j and kept).
 * u, v, T, the ∂z arrays, u_out, v_out, T_out: [n_col][Nz]; top_flux, halo_bottom, halo_top: [3][n_col]; uw, vw, wT: [n_col][Nz+1]; params = {nu0,
 * nu_minus, dRi, Ric, Pr, alpha, g}.  The wm calls need every state and output base pointer 16-byte aligned (a row of Nz+1 floats is not: only
 * the base).  u_out, v_out, T_out may each alias its own input; the ∂z arrays and the faces alias nothing.  n_columns is independent of the handle's
 * own column count.  The wm calls refuse, with the reason in colnde_last_error, what colnde_wm_infer_dz_flux refuses: anything but a single-model
 * wind-mixing handle with Nz = 32 and three 96-50-20-31 networks, and a handle with smooth_NN; also a misaligned pointer.  They run on the f32
 * matrix pipe under either matrix_arithmetic (colnde_describe: wm_infer=f32).  All six are timed under colnde_kernel_time slot 10. */
int colnde_wm_diagnose_flux_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T, const float* d_top_flux,
                                const float* d_halo_bottom /* nullable */, const float* d_halo_top /* nullable */, float Lz, const float params[7],
                                int convective_adjustment, float* d_uw, float* d_vw, float* d_wT, int n_columns);
int colnde_wm_diagnose_flux(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T, const float* top_flux,
                            const float* halo_bottom, const float* halo_top, float Lz, const float params[7], int convective_adjustment, float* uw,
                            float* vw, float* wT, int n_columns);   /* host arrays; synchronises */
int colnde_wm_embedded_step_flux_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T,
                                     const float* d_top_flux, const float* d_halo_bottom, const float* d_halo_top, float Lz, float dt,
                                     const float params[7], int convective_adjustment, float* d_dz_uw, float* d_dz_vw, float* d_dz_wT, float* d_u_out,
                                     float* d_v_out, float* d_T_out, float* d_uw, float* d_vw, float* d_wT, int n_columns);
int colnde_wm_embedded_step_flux(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T, const float* top_flux,
                                 const float* halo_bottom, const float* halo_top, float Lz, float dt, const float params[7], int convective_adjustment,
                                 float* dz_uw, float* dz_vw, float* dz_wT, float* u_out, float* v_out, float* T_out, float* uw, float* vw, float* wT,
                                 int n_columns);   /* host arrays; synchronises */
int colnde_mpp_diagnose_flux_dev(colnde_handle* h, const float* d_u, const float* d_v, const float* d_T, const float* d_top_flux,
                                 const float* d_halo_bottom /* nullable */, float dz, const float params[7], int convective_adjustment, float* d_uw,
                                 float* d_vw, float* d_wT, int n_columns);
int colnde_mpp_diagnose_flux(colnde_handle* h, const float* u, const float* v, const float* T, const float* top_flux, const float* halo_bottom, float dz,
                             const float params[7], int convective_adjustment, float* uw, float* vw, float* wT, int n_columns);   /* host arrays */

/* The free-convection embedding's per-iteration work and its diagnosed flux (free_convection/src/oceananigans_nn.jl; the same over 96 x 96 columns
 * in free_convection/double_gyre_nn.jl:211-234), per column, on T [Nz] AS GIVEN (k = 0 deepest, the units colnde_infer_dz_wT takes), dz = Lz/Nz,
 * c = dt/dz²:
 *   1. forcing (progress_neural_network :159-160 with neural_network_forcing :120-126): y = NN((T̃−μ_T)/σ_T) as colnde_infer_dz_wT evaluates it
 *      (Nz−1 values), faces F = [0; σ_wT y + μ_wT; top_flux] (:95), stored ∂z_wT_NN[k] = (F[k+1] − F[k])/dz (:86-93) — BEFORE the adjustment;
 *   2. convective_adjustment!(model, Δt, K) (:162, :13-40): exactly colnde_convective_adjustment above — κ_k = K where the centred ∂T/∂z of cell k
 *      is negative, 0 elsewhere, halo cells as given or, NULL, the zero-gradient fill, one backward-Euler step T′ = L \ T;
 *   3. diagnose_wT_NN (:100-118): g_f = ∂T/∂z on the Nz+1 faces (:107; the end faces from the halo cells, same NULL rule), κ_f = g_f < 0 ? K : 0
 *      (:110-113; NaN < 0 is false, as in Julia), wT_faces = F − κ_f g_f (:115-117), F the faces of 1.
 * colnde_fc_embedded_step: 1 and 2 (progress_neural_network, :153-165) and, when wT_faces is not NULL, 3 of the state as given, in ONE launch that
 * reads T once; colnde_fc_diagnose_wT: 3 alone.  T, dz_wT, T_out: [n_col][Nz]; top_flux, halo_bottom, halo_top: [n_col]; wT_faces: [n_col][Nz+1].
 * T, dz_wT, T_out and wT_faces 16-byte aligned.  T_out may alias T; no other aliasing.  n_columns is independent of the handle's own column
 * count.  The ∂z_wT_NN bits are colnde_infer_dz_wT_dev's and the T′ bits colnde_convective_adjustment_dev's (the same device code).  Refused, with
 * the reason in colnde_last_error: wind-mixing, ensemble and closure handles, networks other than the fc32 shape Dense(Nz,4Nz,relu),
 * Dense(4Nz,4Nz,relu), Dense(4Nz,Nz−1), networks with activation rows in global memory, Nz other than 32 or 64; the handle's engine and stepper do
 * not matter.  The dense chains run on the f32 matrix pipe under either matrix_arithmetic (colnde_describe: fc_embed=f32); timed under
 * colnde_kernel_time slot 9.  Launches: colnde_fc_diagnose_wT one; colnde_fc_embedded_step one when wT_faces is given and, when it is NULL,
 * the two of colnde_infer_dz_wT_dev and colnde_convective_adjustment_dev (slots 4 and 6) — measured faster than the fused kernel from 65,536
 * columns on (COLNDE_FC_EMBED_FUSED=1 forces the fused kernel); the results are the same bits either way. */
int colnde_fc_embedded_step_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux, const float* d_halo_bottom,
                                const float* d_halo_top, float Lz, float dt, float K, float* d_dz_wT, float* d_T_out, float* d_wT_faces /* nullable */,
                                int n_columns);
int colnde_fc_embedded_step(colnde_handle* h, const float* weights, const float* T, const float* top_flux, const float* halo_bottom,
                            const float* halo_top, float Lz, float dt, float K, float* dz_wT, float* T_out, float* wT_faces /* nullable */,
                            int n_columns);   /* host arrays; synchronises */
int colnde_fc_diagnose_wT_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux, const float* d_halo_bottom,
                              const float* d_halo_top, float Lz, float K, float* d_wT_faces, int n_columns);
int colnde_fc_diagnose_wT(colnde_handle* h, const float* weights, const float* T, const float* top_flux, const float* halo_bottom,
                          const float* halo_top, float Lz, float K, float* wT_faces, int n_columns);   /* host arrays; synchronises */

/* Flux.Optimise.ADAM apply! + update! (Flux 0.11.6 src/optimise/optimisers.jl; used at wind_mixing/src/NDE_training.jl:340-372,
 * free_convection/src/training.jl:71) on device vectors of n floats: m ← β₁m + (1-β₁)g, v ← β₂v + (1-β₂)g²,
 * w ← w - η·m/(1-β₁ᵗ)/(√(v/(1-β₂ᵗ)) + ϵ).  beta1_t / beta2_t are the running powers the optimiser state carries (β₁, β₂ on the
 * first call; the caller multiplies them by β after each call, as Flux does).  Enqueued on the handle's stream. */
int colnde_adam_step_dev(colnde_handle* h, float* d_weights, const float* d_grad, float* d_m, float* d_v, float eta, float beta1,
                         float beta2, float eps, float beta1_t, float beta2_t, int n);

/* Flux-MLP pre-training: one pass of `Flux.train!(NN_loss, Flux.params(NN), training_data, opt)` — `train_NN`,
 * wind_mixing/src/NN_training.jl:207-249 with the flux closures predict_uw / predict_vw / predict_wT (:25-169); T -> wT pre-training of
 * free_convection/train_free_convection_nde.jl:186-216 — i.e. ONE Flux-ADAM update per sample, in the order given:
 *   NN_flux = face vector of net `flux_type` (0 = uw, 1 = vw, 2 = wT; T-only models: 2) for the sample's profile and BCs, as the
 *             handle's conditions say (MPP / convective adjustment / zero_weights; the smoothing options are not covered);
 *   loss    = mse(NN_flux, flux) + gradient_scaling * mse(D^c flux, D^c NN_flux).
 * d_theta / d_m / d_v: the handle's full weight vector and its ADAM moments (n_params floats).  Only the block of the net trained is
 * read or written, in all three: the blocks of the other nets keep their bits in d_theta, d_m and d_v.
 * d_profiles [n][n_state], d_bcs [n][n_bc], d_flux [n][Nz+1] scaled fluxes on faces, d_order [n] sample order (NULL: 0..n-1; an index may
 * repeat: the sample is then visited again, with the weights its earlier visits left);
 * beta_t[2]: the optimiser's running powers (host, doubles; updated in place, so a pass may be split into several calls that carry d_m,
 * d_v and beta_t along: same bits as the one call).
 * update = 0: d_theta is not written, d_m / d_v are not read (either may be NULL), beta_t is not advanced, and *mean_loss = mean loss at
 * the given weights (`total_loss(training_data)`, :234-236).  update != 0: *mean_loss = mean over the pass of each sample's loss just
 * BEFORE its own update (the weights as the samples ahead of it in the order left them).
 * Refused (non-zero, colnde_last_error says why; nothing is written): the smoothing options, inplace_variant, a flux_type other than 2 on a
 * T-only model, update != 0 without moments, beta_t >= 1, n_samples < 1, ensemble and closure handles, and a network whose activations do
 * not fit the one workgroup's LDS (the message states the bytes needed).
 * Synchronises the handle's stream. */
int colnde_pretrain_flux_dev(colnde_handle* h, int flux_type, float* d_theta, float* d_m, float* d_v, const float* d_profiles,
                             const float* d_bcs, const float* d_flux, const int32_t* d_order, int n_samples, float gradient_scaling,
                             float eta, float beta1, float beta2, float eps, double beta_t[2], int update, float* mean_loss);

/* Data preparation on device (wind_mixing/src/data_containers.jl:343-427).  d_in [n_rows][N] -> d_out [n_rows][n], one row per
 * profile.  location 0 = Center: coarse_grain(Φ, n, Center) (src/DataWrangling/coarse_graining.jl:8-16), block means, n divides N;
 * location 1 = Face: coarse_grain_linear_interpolation(Φ, n, Face) (:47-62), end points kept (the form data_containers.jl:357 uses). */
int colnde_coarse_grain_dev(colnde_handle* h, const float* d_in, int n_rows, int N, int n, int location, float* d_out);
/* ZeroMeanUnitVarianceScaling(data) (src/DataWrangling/feature_scaling.jl:17-20): d_mu_sigma[0] = mean, [1] = std (n-1 denominator)
 * of `count` device floats; colnde_scale_dev applies scale(x, s) = (x - μ)/σ (:22) with μ, σ read from device memory. */
int colnde_zscore_stats_dev(colnde_handle* h, const float* d_x, int64_t count, float* d_mu_sigma);
int colnde_scale_dev(colnde_handle* h, const float* d_x, int64_t count, const float* d_mu_sigma, float* d_out);

/* ---- multi-GPU: the path's one exchange step, over RCCL (xGMI inside a node) -----------------------------------
 * One process per GPU, columns sharded over the ranks (each handle normalises by colnde_set_global_columns); per optimiser
 * iteration every rank SUM-all-reduces its result buffer [grad(n_params); 6 terms; total; 0] and then applies the identical
 * ADAM step.  The reference has no distributed code: nothing is replaced here, the reference's serial comprehension over
 * simulations (NDE_training.jl:291,304) is what gets sharded.  RCCL is bound lazily (dlopen): these calls fail with a message
 * on a box without it.  Bootstrap: rank 0 calls colnde_comm_unique_id and hands the 128 bytes to every rank through any host
 * channel (MPI, a file, a TCP store); every rank then calls colnde_comm_create, which returns once all ranks have joined. */
typedef struct colnde_comm colnde_comm;
int  colnde_comm_unique_id(void* out128);
int  colnde_comm_create(int rank, int nranks, const void* unique_id128, int device, colnde_comm** out);
void colnde_comm_destroy(colnde_comm* c);
int  colnde_comm_rank(const colnde_comm* c);
int  colnde_comm_size(const colnde_comm* c);
/* in-place all-reduce of n device floats, enqueued on hip_stream (not synchronised); op 0 = sum, 1 = max */
int  colnde_comm_allreduce_dev(colnde_comm* c, float* d_buf, int64_t n, int op, void* hip_stream);
/* the result buffer of colnde_loss_grad_dev (n_params + 8 floats), summed over the communicator on the handle's stream */
int  colnde_allreduce_result_dev(colnde_handle* h, colnde_comm* comm, float* d_out);

/* How the handle runs its gradient path (filled in by the first colnde_loss_grad[_dev]; zeros before that):
 * info[0] engine (COLNDE_ENGINE_*), [1] columns per block of the gradient path (the tapes hold one block), [2] number of blocks, [3] regtile: layer-1
 * pre-activations taped (1) or recomputed (0); fc32: number of time segments the tapes are cut into (0: they hold the whole axis), [4] tile16: weight gradients taped (1) or accumulated in registers (0),
 * [5] tile16 taped mode: K-slices of the dW GEMM, [6] fc32: the filter length c of a conv handle (colnde_create_conv; 0 otherwise); tile16: net-split kernels of the latency points (per 16-column tile one wavefront per flux net
 * plus a helper wavefront): bit 0 = forward solve, bit 1 = adjoint, bit 2 = with the rich tape (activations, their derivatives and the physics-pullback
 * coefficients taped by the forward kernel: blocks of at most 2,048 columns), [7] bit 0 = the gradient is the one-switch-pattern
 * RKC2 pullback, an approximation of the discrete adjoint (see COLNDE_STEPPER_RKC2); 0 = exact discrete adjoint of the stepper;
 * bits 1, 2, 3 = the forward-solve / adjoint / weight-gradient kernels of the handle's engine run BF16X3_EXACT (a cleared bit: F32_MFMA — the
 * configured arithmetic, a test override, or no split kernel for this engine and shape). */
int colnde_plan(const colnde_handle* h, int info[8]);

/* The same, spelled out, plus every tuning switch the library honours: one text line
 *   "engine=regtile stepper=rk4 substeps=2 matrix_arithmetic=bf16x3_exact forward=bf16x3 adjoint=bf16x3 dw=bf16x3 block=32768x1 ... | env COLNDE_RT_BLOCK=8192 ..."
 * The part after "| env" lists each COLNDE_* environment variable that is SET in this process and that the library reads (INTEGRATION.md has the
 * table): they are tuning and test aids, read when the handle is created or when it plans its tapes, never per call — and this is where a caller sees
 * that one of them shaped the handle.  buf may be NULL; returns the number of bytes the full line needs (including the terminating 0), or -1. */
int colnde_describe(const colnde_handle* h, char* buf, int capacity);

/* ---- ensembles: K models of ONE architecture trained side by side on one GPU ----------------------------------------------------------------------
 * The reference's production driver is a sweep: wind_mixing/train_NDE_args.jl takes the activation (ARGS[1]), the ADAM rate (ARGS[2], :143) and the
 * Pacanowski-Philander constants (ARGS[3], the train_parameters Dict at :175) on its command line and trains ONE model per process, at the small shape of
 * wind_mixing/train_NDE.jl:138-141 (8 to 18 simulations).  An ensemble handle holds K such models of one architecture (cfg) on the same columns, each
 * with its own weights, its own five constants and its own ADAM rate; every kernel of a training iteration runs once for all K models (model index in
 * the launch grid).  Shared by all models: the problem (colnde_set_problem[_dev]: x0, bcs, truth), the loss scalings and the sub-step count.
 * Accepted: the configurations on which engine AUTO runs the four-wave net-split kernels — Nz = 32, three 96-50-20-31 nets, training RHS, no smoothing,
 * RK4 or RKC2, engine AUTO, substeps >= 1, at most 8,192 columns per model; everything else (free convection / fc32, wide networks, inplace_variant,
 * a forced engine, substeps = 0) is refused with the reason.  The shared sub-step count must meet colnde_min_substeps for EVERY model's constants
 * (COLNDE_ALLOW_UNSTABLE_DT=1 overrides); RKC2 with rkc_stages = 0 runs the largest automatic stage count over the models.  The tapes of all models are
 * allocated at creation: a handle whose tapes do not fit is refused with the bytes it needs.  Handle-level calls that accept an ensemble: set_problem[_dev],
 * set_stream, set_matrix_arithmetic, set_profiling / kernel_time / reset_kernel_times, plan, describe (adds models=K and the bytes per model), n_params,
 * destroy.  Every call that takes ONE weight vector refuses an ensemble handle. */

/* Create: physics [n_models][5] = nu0, nu_minus, dRi, Ric, Pr per model (mpp_parameters order; the train_parameters of train_NDE_args.jl:175), host
 * memory; NULL = cfg's constants for every model.  A physics array needs modified_pacanowski_philander = 1. */
int colnde_create_ensemble(const colnde_config* cfg, int n_models, const float* physics, colnde_handle** out);
/* ---- tile ensembles: K wind-mixing models of ANY tile16 architecture side by side ----------------------------------------------------------------------
 * colnde_create_ensemble covers the net-split shape.  The reference sweeps its wider nets the same way (wind_mixing/train_NDE.jl:97-102,
 * train_NDE_args.jl:150-166: Dense(96,400)-Dense(400,400)-Dense(400,31), 96-32-400-31, 96-400-31, one model per process at 8 to 18 simulations).  A tile
 * ensemble runs the tile16 engine's own kernels with the model index in the launch grid; the launch geometry is the one a single handle of n_columns
 * columns runs, so row k of every result is, bit for bit, what a colnde_create handle with engine = COLNDE_ENGINE_GENERIC computes for model k's weights
 * and constants.  physics as for colnde_create_ensemble.
 * Accepted: the wind-mixing model on the training RHS; engine AUTO or GENERIC; any layer sizes and activations colnde_create accepts on tile16 (the
 * 96-50-20-31 shape included: it then runs tile16's kernels, not the net-split pair); RK4 or RKC2; substeps >= 1; at most 4,096 columns per model; the
 * modified Pacanowski-Philander, convective-adjustment or plain branches, diurnal forcing, smoothing; 16 x 3 Nz <= 2,048 (the 1,024-thread taped adjoint;
 * a single handle runs taller grids on 512-thread kernels, which have no model index).
 * Refused at creation, each with its reason and before any device work: free-convection models (colnde_create_fc_ensemble), inplace_variant, engine
 * MFMA / FC32, substeps = 0, a step below any model's colnde_min_substeps, n_models outside 1..65535, more than 4,096 columns, a network the taped adjoint
 * cannot run, COLNDE_T16_DWTAPE=0, COLNDE_T16_ZTAPE=0, COLNDE_T16_BLOCK, COLNDE_T16_TAPE_THREADS=512, COLNDE_T16_FWD_SPLIT=1, a physics array without
 * the closure, non-finite physics, dRi <= 0, Pr <= 0; and, once the device is known, tapes that do not fit (with the bytes).
 * Served: colnde_ensemble_forward_dev, _loss_dev, _loss_grad_dev, _loss_grad, _adam_step_dev, _set_physics, colnde_n_models, set_problem[_dev],
 * set_stream, set_matrix_arithmetic, profiling, plan, n_params, destroy, describe (models=K, tile_ensemble=1, the bytes per model).
 * Refused, each naming itself (their kernels read a 96-50-20-31 image or a net-split tape): colnde_ensemble_set_member_loss and the member-loss calls,
 * colnde_set_schedule / colnde_choose_schedule, colnde_ensemble_wm_embedded[_dev], colnde_ensemble_profile[_dev], colnde_ensemble_pretrain_wm_flux_dev,
 * and every single-model call.  The member loss on the tile engine is left out on purpose: tile16's adjoint has no column-weight path yet. */
int colnde_create_tile_ensemble(const colnde_config* cfg, int n_models, const float* physics /* [K][5] or NULL */, colnde_handle** out);
/* number of models: 1 for colnde_create handles, K for an ensemble */
int colnde_n_models(const colnde_handle* h);
/* new constants for every model (host [n_models][5]), checked against the stability bound like colnde_create_ensemble */
int colnde_ensemble_set_physics(colnde_handle* h, const float* physics);
/* solve(...) of every model (NDE_training.jl:291,403): d_weights [K][n_params], d_sol [K][n_col][n_save][n_state]; device memory, handle's stream */
int colnde_ensemble_forward_dev(colnde_handle* h, const float* d_weights, float* d_sol);
/* loss_NDE (NDE_training.jl:290-323) of every model: d_out8 [K][8] = [scaled terms(6); total; 0] per model */
int colnde_ensemble_loss_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out8);
/* loss_gradient_NDE of every model (NDE_training.jl:327-333): d_out [K][n_params + 8], each row exactly what colnde_loss_grad_dev writes for one model.
 * A model whose solve leaves the stable regime gets a non-finite row; the other rows are unaffected. */
int colnde_ensemble_loss_grad_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out);
/* the same with host arrays: weights [K][n_params], out [K][n_params + 8]; synchronises the stream */
int colnde_ensemble_loss_grad(colnde_handle* h, const float* weights, const float scalings[6], float* out);
/* ---- ensembles: the error estimate member by member, and one step schedule chosen for all K -----------------------------------------------------------
 * The members of a sweep differ in what decides the step — nu0, nu_minus, dRi, Ric, Pr and the weights — and the reference gives every run its own
 * adaptive ROCK4 at reltol = 1e-3 (1e-4 for free convection); an ensemble steps all K by one count or one schedule.
 * colnde_ensemble_error_estimate[_dev]: estimates [K][n_save] (HOST in both forms), estimates[k][n] = colnde_error_estimate's number for member k at save
 *   point n alone (the maximum over the columns; the same Richardson factor and the same floor 1e-6 / cfg.reltol).  Two tape-less solves of all K members
 *   on the handle's stream — under the counts in force (the schedule if one is set, else cfg.substeps everywhere) and with every interval doubled — into
 *   scratch, one kernel, one device-to-host copy, one synchronisation (RKC2 with rkc_stages = 0 excepted: the doubled solve and the restoration each upload
 *   a stage table and wait for it, as in colnde_error_estimate).  estimates[k][0] = 0 (both solves hold x0 there); a member whose solve is not finite
 *   has +inf in its own row and no other.  The handle computes afterwards what it computed before: schedule, its device copy, cfg.substeps, the RKC2 stage
 *   table and the tapes are untouched, on failure too.  Under RKC2 with rkc_stages = 0 the doubled solve runs the stage count its own step needs (the
 *   largest over the members, as at creation).  Serves colnde_create_ensemble (RK4, RKC2, with or without a schedule), colnde_create_tile_ensemble and
 *   colnde_create_fc_ensemble handles.  Refused before any device work, each naming the call: null arguments, a single handle (colnde_error_estimate),
 *   a closure handle, a conv ensemble, no problem set, a column shard (colnde_set_global_columns above the handle's own count).
 * colnde_ensemble_choose_schedule (the handles colnde_set_schedule accepts among ensembles: colnde_create_ensemble under RK4; colnde_set_schedule's refusals
 *   with their words, and those above): colnde_choose_schedule's greedy run with E[n] = the maximum over the members.  From the stability minima of the
 *   members' constants (the largest per interval) rounded up to powers of two; each round solves at S and 2 S for all K at once.  On success the handle
 *   keeps the schedule exactly as after colnde_set_schedule (the tapes planned again; a total that does not fit is refused with the bytes, the previous
 *   schedule and tapes kept); counts [n_save - 1] (nullable) receives it, estimates [K] (HOST, nullable) every member's own maximum over the save points
 *   at it — the member that drives the schedule is the largest.  reltol = 0: cfg.reltol.  Failures keep the previous schedule: a member whose solve is
 *   not finite (named), the float32 round-off floor and "too stiff" in colnde_choose_schedule's words. */
int colnde_ensemble_error_estimate_dev(colnde_handle* h, const float* d_weights /* [K][n_params] */, float* estimates /* HOST [K][n_save] */);
int colnde_ensemble_error_estimate(colnde_handle* h, const float* weights /* host [K][n_params] */, float* estimates /* [K][n_save] */);
int colnde_ensemble_choose_schedule(colnde_handle* h, const float* weights /* host [K][n_params] */, float reltol, int* counts /* [n_save - 1], nullable */,
                                    float* estimates /* [K], nullable */);
/* ---- the member loss: every member its own loss scalings and its own training simulations --------------------------------------------------------------
 * In the reference the loss is per run in two ways.  determine_loss_scalings (wind_mixing/src/NDE_training.jl:256-288) solves once with the run's own
 * initial weights and constants and feeds the six unscaled terms to calculate_loss_scalings (loss.jl:11-31), so two runs of a sweep train under different
 * scalings; and --training-simulations (free_convection/train_free_convection_nde.jl:60-66; N_sims of train_NDE_args.jl) trains a run on some of the
 * simulations and judges it on the rest.  Under a member loss, member k is differentiated under
 *     loss_k = sum_q s[k][q] * sum_c w[k][c] * (term q of column c) / sum_c w[k][c]
 * scalings [K][6] (host; NULL: every scaling 1) and column_weights [K][n_col] (host; NULL: every column 1; a 0/1 row is a training set, fractions weigh
 * simulations).  Both NULL clears the member loss.  The K weight rows are formed on the host in double, by the expression colnde_loss* use with
 * sum_c w[k][c] (summed in double) in the column count's place; the arrays are uploaded in stream order on the handle's stream and the upload is complete
 * when the call returns (the caller's arrays are not kept).  Refused before any device work, with the reason in colnde_last_error: a handle that is not
 * an ensemble (closure handles included), an entry that is negative or not finite, a member whose column weights sum to 0, a handle whose global column
 * count differs from its own (the normaliser would be a global sum).  Free-convection and conv ensembles take the same calls; as with scalings[6], only
 * scalings[k][2] is read.  colnde_describe reports member_loss=scalings|columns|scalings+columns while one is set; without one there is no such key and the line is what it was.  The shared-scalings calls above ignore a member loss
 * that has been set.  With per-member scalings alone, row k is bit for bit the row of the shared call given scalings[k]; all-ones weights give the bits
 * of column_weights = NULL.  The judge (colnde_ensemble_column_loss_dev, colnde_ensemble_profile) stays unweighted. */
int colnde_ensemble_set_member_loss(colnde_handle* h, const float* scalings /* host [K][6], or NULL */, const float* column_weights /* host [K][n_col], or NULL */);
/* colnde_ensemble_loss_dev / _loss_grad_dev / _loss_grad under the member loss that was set (refused when none is): the same layouts */
int colnde_ensemble_member_loss_dev(colnde_handle* h, const float* d_weights, float* d_out8 /* [K][8] */);
int colnde_ensemble_member_loss_grad_dev(colnde_handle* h, const float* d_weights, float* d_out /* [K][n_params + 8] */);
int colnde_ensemble_member_loss_grad(colnde_handle* h, const float* weights, float* out);
/* Flux.Optimise.ADAM (as colnde_adam_step_dev; NDE_training.jl:340-372) for every model: d_weights, d_m, d_v [K][n_params], the gradient read as the first
 * n_params floats of each [n_params + 8] row of d_result (the buffer of colnde_ensemble_loss_grad_dev), d_eta [K] per-model rates (train_NDE_args.jl:143) */
int colnde_ensemble_adam_step_dev(colnde_handle* h, float* d_weights, const float* d_result, float* d_m, float* d_v, const float* d_eta,
                                  float beta1, float beta2, float eps, float beta1_t, float beta2_t);

/* ---- free-convection ensembles: K networks of the fc32 shape on the same simulations ---------------------------------------------------------------
 * The reference trains the free-convection NDE on 3 to 9 simulations (free_convection/train_free_convection_nde.jl, --training-simulations), sweeps that
 * driver over seeds, optimiser rates and `--spatial_causality soft`, and judges a run by re-solving the network of EVERY epoch on every simulation
 * (compute_nde_solution_history, free_convection/src/testing.jl:1-32).  A free-convection ensemble handle holds K networks Dense(Nz,4Nz,relu),
 * Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1), Nz = 32 or 64, of FreeConvectionNDE (RK4) or ConvectiveAdjustmentNDE (RK4, RKC2) on the same columns; the 16-column
 * fc32 kernels carry the model index in the launch grid.  Shared: x0, the [bottom, top] fluxes, truth, the save times, the sub-step count, the RKC2 table.
 * Owned by a model: operand images, biases, solution, tapes, lambda between time segments, slab rows.
 * It is accepted by colnde_ensemble_forward_dev, _loss_dev, _loss_grad_dev, _loss_grad and _adam_step_dev with their layouts ([K][n_params] weights,
 * [K][n_params + 8] result rows), and by the handle-level calls a wind-mixing ensemble accepts (describe adds models=K, the bytes per model and
 * time_segments).  Row k of every result holds the bits a colnde_create handle computes for model k's weights, under either matrix arithmetic (and the same
 * COLNDE_FC_SEG: the segment count orders the gradient's sums).  colnde_ensemble_set_physics (no constants to vary), colnde_ensemble_wm_embedded, colnde_ensemble_profile and every
 * single-model call refuse it; colnde_ensemble_fc_embedded (below) takes its K networks into the embedding.
 * Refused at creation, before any device work, each with its reason: a wind-mixing model, another network shape or Nz, an engine other than AUTO or FC32,
 * substeps = 0, substeps < colnde_min_substeps, n_models outside 1..65535, more than 4,096 columns per model (above it a single handle runs 32-column
 * tiles), COLNDE_FC=0, COLNDE_FC_CW=32, COLNDE_FC_BLOCK.  Then "no HIP device ... no CPU fallback", and tapes that do not fit, with the bytes needed: all K
 * models' tapes are planned here on a per-model budget of (free memory - 3 GB) / K, the whole time axis when it fits, time segments otherwise. */
int colnde_create_fc_ensemble(const colnde_config* cfg, int n_models, colnde_handle** out);
/* out[k][c][n] = mean over the Nz levels of (sol[k][c][n][:] - truth[c][n][:])^2, scaled units:
 * Flux.mse(true, nde, agg = x -> mean(x, dims=1)) of testing.jl:83 for every model and simulation (plot_epoch_loss, animate_nde_loss: testing.jl:34-105).
 * d_sol: [K][n_col][n_save][Nz], the layout of colnde_ensemble_forward_dev.  Fixed-order sums: bit-reproducible. */
int colnde_ensemble_column_loss_dev(colnde_handle* h, const float* d_sol, float* d_out /* [K][n_col][n_save] */);
/* result[k][n_params + 6] += c_k * sum_{r < q} W1_k[r, q]^2 ;  result[k][index of W1[r, q]] += 2 c_k W1_k[r, q]
 * W1 = the first Dense weight (4Nz x Nz, column-major as Flux.destructure lays it out; a conv ensemble: 4Nz x (Nz-c+1) at offset c + 1), r < q the mask of
 * train_free_convection_nde.jl:193; c_k = 1 is the reference's penalty, 0 leaves row k's bits alone.
 * d_result: the buffer of colnde_ensemble_loss_grad_dev, updated in place. */
int colnde_ensemble_causal_penalty_dev(colnde_handle* h, const float* d_weights, const float* d_coeff /* [K] */, float* d_result);
/* T -> wT pre-training of all K networks of a free-convection ensemble in ONE launch: one pass of `Flux.train!(loss, ps, data, opt)` per model —
 * free_convection/train_free_convection_nde.jl:182-216, one optimiser update per sample in the order given, loss = mse([bottom; NN(T); top], wT)
 * + c_k sum(abs2, W1[mask]) (--spatial_causality soft, :186-197; mask r < q as colnde_ensemble_causal_penalty_dev).  One workgroup per model
 * (blockIdx.x = model); model k reads and writes only row k of d_theta / d_m / d_v ([K][n_params], the ensemble's layout) and reads row k of d_order,
 * d_eta and d_coeff; the samples d_T [n][Nz], d_bcs [n][2] = bottom, top and d_flux [n][Nz+1] (scaled) are shared.
 * Handles: colnde_create_fc_ensemble (the plain network) and colnde_create_conv_ensemble (theta = [w (c); b; vec(W1) 4Nz x (Nz-c+1); b1; ...]; K = 1 is
 * the single --conv run), any K >= 1 — the same handle then trains the NDE.
 * optimiser 0 = Flux ADAM (d_m, d_v, beta_t as colnde_pretrain_flux_dev), 1 = Descent: theta -= eta_k g, d_m / d_v not touched (may be NULL), beta_t
 * not advanced.  d_order NULL: 0..n-1 for every model; an index may repeat.  d_coeff NULL: no penalty.
 * update = 0: nothing on the device is written and mean_loss[k] = the mean loss at the given weights, the penalty included (the driver's nn_callback);
 * update != 0: mean_loss[k] = the mean of each sample's loss just before its own update; beta_t advances by n_samples steps (ADAM).  mean_loss: HOST, [K].
 * A plain ensemble under ADAM with c_k = 0: row k of d_theta, d_m, d_v and mean_loss[k] hold the bits colnde_pretrain_flux_dev computes on a
 * colnde_create handle for model k's weights with gradient_scaling = 0 and the same order (the two kernels share one per-sample body).
 * Refused before any launch, each with its reason and this call's name: a null handle or null pointers, a wind-mixing ensemble, single-model and closure
 * handles, an optimiser outside {0, 1}, ADAM with update but without moments, beta_t >= 1 under ADAM, n_samples < 1.  Synchronises the handle's stream. */
int colnde_ensemble_pretrain_flux_dev(colnde_handle* h, float* d_theta, float* d_m, float* d_v, const float* d_T, const float* d_bcs, const float* d_flux,
                                      const int32_t* d_order, int n_samples, const float* d_coeff, int optimiser, const float* d_eta, float beta1,
                                      float beta2, float eps, double beta_t[2], int update, float* mean_loss);
/* train_NN (wind_mixing/src/NN_training.jl:207-249) for the K x 3 flux networks of a wind-mixing ensemble in ONE launch: per (model k, net j) one pass of
 * `Flux.train!(NN_loss, Flux.params(NN), training_data, opt)` with the semantics of colnde_pretrain_flux_dev — Flux ADAM, one update per sample in the
 * order given, loss = mse + gradient_scaling * mse of the centred differences — and with MODEL k's closure constants (nu0, nu_minus, dRi, Ric, Pr of
 * colnde_create_ensemble / colnde_ensemble_set_physics) in the weight-independent part of the face flux.  The conditions (modified Pacanowski-Philander,
 * convective adjustment, zero_weights) are the handle's.  One workgroup per chain (blockIdx.x = model, blockIdx.y = net); chain (k, j) reads and writes only
 * floats [k P + j net_size, k P + (j + 1) net_size) of d_theta / d_m / d_v ([K][P], the ensemble's layout) and reads row (k, j) of d_order and d_eta; the
 * samples d_profiles, d_bcs and the three nets' fluxes d_flux (scaled, on the faces) are shared.
 * nets: bit j set = train net j (0 = uw, 1 = vw, 2 = wT), 1..7; the blocks of the other nets keep their bits and their mean_loss entries are 0.
 * d_order NULL: 0..n-1 for every chain; an index may repeat.
 * update = 0: nothing on the device is written, beta_t does not advance and mean_loss[k][j] = the mean loss at the given weights (d_m, d_v, d_eta may be
 * NULL); update != 0: mean_loss[k][j] = the mean of each sample's loss just before its own update, and beta_t advances by n_samples steps, once (every
 * selected chain takes the same number of steps).
 * Block (k, j) of d_theta, d_m, d_v, mean_loss[k][j] and beta_t hold the bits colnde_pretrain_flux_dev computes on a colnde_create handle whose config
 * carries model k's five constants, with flux_type = j, rate d_eta[k][j] and the same samples and order (the two kernels share one per-sample body).
 * Refused before any launch, each with its reason and this call's name: a null handle or null pointers, a free-convection or conv ensemble
 * (colnde_ensemble_pretrain_flux_dev), single-model and closure handles, nets outside 1..7, update without moments or rates, beta_t >= 1, n_samples < 1.
 * Runs on the handle's stream and synchronises it. */
int colnde_ensemble_pretrain_wm_flux_dev(colnde_handle* h, int nets /* bit j: train net j */, float* d_theta, float* d_m, float* d_v,
                                         const float* d_profiles /* [n][96] */, const float* d_bcs /* [n][6] */, const float* d_flux /* [3][n][33] scaled, faces */,
                                         const int32_t* d_order /* [K][3][n] or NULL */, int n_samples, float gradient_scaling, const float* d_eta /* [K][3] */,
                                         float beta1, float beta2, float eps, double beta_t[2], int update, float* mean_loss /* HOST [K][3] */);

/* All K models of an ensemble in the embedding ocean column at once — one iteration of progress_neural_network (wind_mixing/src/NDE_oceananigans.jl:380-405) and / or
 * the saved-state diagnoses diagnose_NN_flux_uw / _vw / _wT (:226-286) for every model, each on its OWN column state with its own weights and its own constants: how
 * NDE_profile_oceananigans / solve_oceananigans_modified_pacanowski_philander_nn judge the members of a sweep.  One launch for all K.
 *   d_weights [K][n_params] (the ensemble's layout); u, v, T and every [..][Nz] output [K][n_col][32]; the faces [K][n_col][33]; top_flux [3][n_col], SHARED by the
 *   models (they are driven by the same surface fluxes, as the ensemble shares bcs); halo_bottom, halo_top [K][3][n_col] or NULL; params HOST memory [K][7] =
 *   {nu0, nu_minus, dRi, Ric, Pr, alpha, g} per model, or NULL: the handle's current per-model physics (colnde_create_ensemble / colnde_ensemble_set_physics)
 *   followed by cfg.alpha, cfg.g.
 *   The ∂z arrays are always written.  d_u_out, d_v_out, d_T_out: all three given — the implicit step is taken, dt > 0 required, each may alias its own input —
 *   or all three NULL (no step, dt ignored).  d_uw, d_vw, d_wT: all three given — the face diagnosis of the state AS GIVEN — or all three NULL.
 * Row k of every output is, bit for bit, what the single-model call of the same output groups (colnde_wm_embedded_step_flux, colnde_wm_diagnose_flux,
 * colnde_wm_embedded_step, colnde_wm_infer_dz_flux) writes for model k's weights, state, halos and params.  Accepts an ensemble handle; a single-model handle is
 * K = 1.  Refuses, with the reason in colnde_last_error, what those calls refuse (shape, smooth_NN, null, the 16-byte alignment of every state and output BASE
 * pointer, dRi != 0, Pr > 0) and a closure handle, a half-given output group, dt <= 0 with a step.  Timed under colnde_kernel_time slot 10.
 * COLNDE_WM_ENS_GRID=<n> (a test override) caps the workgroups of this launch and of no other.
 * Networks of ANY trained architecture: a single (non-ensemble) wind-mixing handle at Nz = 32 whose three nets have layer sizes 96-h1-...-31 — whatever the
 *   hidden widths, the number of layers (up to COLNDE_MAX_LAYERS) and the per-layer activations colnde_create accepts — is served too, as K = 1, by a kernel of its
 *   own (csrc/engine_wm_embed_any.hip; colnde_describe: wm_embed=generic_f32): the same arithmetic and the same output groups in one launch, the
 *   weights read in place from d_weights, the f32 matrix pipe under either matrix_arithmetic.  This is the one embedding call that deploys 3 x 96-400-400-31 or
 *   3 x 96-400-31 (train_NDE.jl:97-103, train_NN_args.jl:101-103); the four single-model calls above keep to 96-50-20-31 and say so.  A shape whose activation
 *   rows do not fit a workgroup's 160 KiB of LDS is refused before any device work, with the bytes it needs (hidden widths up to 600 fit; 96-2048-2048-31 does
 *   not).  An ensemble of such networks is trained by colnde_create_tile_ensemble, whose handles this call refuses (it deploys
 *   single handles and colnde_create_ensemble's).  COLNDE_WM_GENERIC=1 (a test switch, read per call) sends a single handle
 *   of the 96-50-20-31 shape to that kernel as well; without it that shape runs the persistent kernel, single or ensemble, with the bits it always had. */
int colnde_ensemble_wm_embedded_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T,
        const float* d_top_flux, const float* d_halo_bottom, const float* d_halo_top, float Lz, float dt, const float* params,
        int convective_adjustment, float* d_dz_uw, float* d_dz_vw, float* d_dz_wT, float* d_u_out, float* d_v_out, float* d_T_out,
        float* d_uw, float* d_vw, float* d_wT, int n_columns);
/* the same with host arrays (no alignment rule); synchronises the stream */
int colnde_ensemble_wm_embedded(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T,
        const float* top_flux, const float* halo_bottom, const float* halo_top, float Lz, float dt, const float* params,
        int convective_adjustment, float* dz_uw, float* dz_vw, float* dz_wT, float* u_out, float* v_out, float* T_out,
        float* uw, float* vw, float* wT, int n_columns);

/* Judging the K members of a wind-mixing sweep — what NDE_profile (wind_mixing/src/training_postprocessing.jl:250-632) evaluates on the saved states of a solve,
 * for all K models at once.  The call solves nothing: d_sol [K][n_col][n_save][96] holds the states to diagnose in scaled units — the output of
 * colnde_ensemble_forward_dev, or of any other solve (the reference's solve_NDE_mutating :302: inplace_variant single handles, uploaded).
 *   d_uw, d_vw, d_wT [K][n_col][n_save][33], scaled units: predict_flux (NDE_training.jl:83-147) on state n of simulation c of model k (test_uw, test_vw, test_wT,
 *       :404-423) with the simulation's boundary fluxes from colnde_set_problem and, in the diurnal case, the top temperature flux at the frame's time — the training
 *       RHS in its three branches (the Pacanowski-Philander closure with eps on the gradients; convective adjustment; neither).  One launch of wm_profile_ens_kernel
 *       (f32 matrix pipe under either matrix_arithmetic; colnde_describe: wm_profile=f32).
 *   d_Ri [K][n_col][n_save][33]: local_richardson on D_face u, v, T WITHOUT eps, as :430 calls it.  D_face's first and last rows are zero, so the two boundary faces
 *       are 0 / 0 = NaN in the reference; they are NaN here (not repaired).
 *   d_losses [K][n_col][6][n_save]: loss_per_tstep (:310-317) of each member against the shared truth: row k holds the bits colnde_loss_per_tstep_dev writes on a
 *       single handle for the same solution.
 *   physics: HOST memory [K][5] = {nu0, nu_minus, dRi, Ric, Pr} per model for THIS call only, or NULL: the handle's.  Rows with nu0 = nu_minus = 0 give the networks'
 *       own share of the flux (constants_NN_only, :286, :474-495).  Nothing is integrated, so there is no stability check; dRi > 0, Pr > 0 and finiteness are checked.
 *       The closure-only set (:326-352, :433-472) is the same call with all-zero weights on the closure-only solve.
 * The flux outputs are all three given or all three NULL; d_Ri and d_losses may each be NULL; at least one output group is required; d_losses needs truth.
 * Accepts a wind-mixing ensemble handle, K >= 1.  Refused before any launch, each with its reason in colnde_last_error: free-convection and conv ensembles, closure and
 * single-model handles, null handle / weights / sol, a half-given flux group, no outputs, d_losses without truth, base pointers that are not 16-byte aligned (_dev
 * only; a model's rows need no alignment of their own), a call before colnde_set_problem, a physics array without the closure.  A model whose states are not finite
 * gets non-finite rows; the other models' rows are unaffected.  The flux / Ri launch is timed under colnde_kernel_time slot 11 (the losses under slot 2).
 * COLNDE_WM_PROFILE_GRID=<n> (a test override) caps the workgroups of this launch and of no other. */
int colnde_ensemble_profile_dev(colnde_handle* h, const float* d_weights, const float* d_sol, const float* physics, float* d_uw, float* d_vw, float* d_wT,
        float* d_Ri, float* d_losses);
/* the same with host arrays (no alignment rule); synchronises the stream */
int colnde_ensemble_profile(colnde_handle* h, const float* weights, const float* sol, const float* physics, float* uw, float* vw, float* wT,
        float* Ri, float* losses);

/* ---- the free-convection driver's --conv network (train_free_convection_nde.jl:50-53, 110-122) ----------------------------------------------------------
 * With --conv c > 1 the reference trains
 *     Chain(reshape, Conv((c, 1), 1 => 1, relu), reshape, Dense(Nz-c+1, 4Nz, relu), Dense(4Nz, 4Nz, relu), Dense(4Nz, Nz-1))
 * A conv handle runs FreeConvectionNDE (RK4) and ConvectiveAdjustmentNDE (RK4, RKC2) with that network on the fc32 engine's 16-column kernels, Nz = 32 | 64,
 * either matrix arithmetic.  The filter is applied inside the kernels where the stage input is written to LDS; the dense chain is the plain network's with
 * W1 padded by zero columns, so the operand images, the weight-gradient GEMM and the reductions are unchanged.
 *   Arithmetic (x the stage input, level 1 = bottom; M = Nz - c + 1; NNlib's conv flips the kernel):
 *       y[i] = relu(b + sum_{k=1..c} w[k] x[i + c - k]),  i = 1..M;     y feeds Dense(M, 4Nz, relu); the physics reads x.
 *   Parameter vector (Flux.params order; colnde_n_params):
 *       theta = [w (c); b (1); vec(W1) (4Nz x M, column-major); b1; vec(W2); b2; vec(W3); b3]
 * cfg is the PLAIN fc32 configuration — layer_sizes = (Nz, 4Nz, 4Nz, Nz-1), relu, relu, identity — and conv_filter = c says that the first Dense takes M
 * inputs behind a c-tap filter.  Calls that work on a conv handle: set_problem[_dev], forward[_dev], loss[_dev], loss_grad[_dev] (n_params gradient floats,
 * the filter's c + 1 first, then the 8 loss slots), loss_per_tstep[_dev], adam_step_dev, set_stream, set_substeps / substeps, set_matrix_arithmetic /
 * matrix_arithmetic, n_params, engine, conv_filter, plan (info[6] = c), describe ("conv=c"), profiling and kernel times (the filter-gradient kernel is timed
 * with the dW GEMM, slot 5), destroy; the array utilities that read no network (coarse_grain, zscore_stats, scale, convective_adjustment, implicit_diffusion,
 * mpp_diagnose_flux); colnde_ensemble_fc_embedded[_dev] (below: the network in the embedding, K = 1).  Every other call refuses a conv handle with a sentence naming the call: rhs, flux, error_estimate, choose_substeps, infer_*, the embedded
 * steps and diagnoses, pretrain_flux, set_global_columns and allreduce_result (multi-GPU results), the ensemble and closure calls (K conv networks side by
 * side: colnde_create_conv_ensemble, below).
 * Refused here, before any device work, each with its reason: conv_filter outside 2..8, a wind-mixing model, another network shape or Nz, an engine other than
 * AUTO or FC32, FreeConvectionNDE under RKC2, substeps = 0, substeps < colnde_min_substeps, more than 4,096 columns, COLNDE_FC=0, COLNDE_FC_CW=32,
 * COLNDE_FC_BLOCK.  Then "no HIP device ... no CPU fallback".  The tapes are planned by the first colnde_loss_grad (colnde_set_substeps works until then); tapes
 * that do not fit are refused there with the bytes needed. */
int colnde_create_conv(const colnde_config* cfg, int conv_filter, colnde_handle** out);
/* c of a conv handle or conv ensemble, 0 for every other handle (-1: null) */
int colnde_conv_filter(const colnde_handle* h);
/* ---- conv ensembles: K --conv networks of ONE filter length on the same simulations ---------------------------------------------------------------------
 * The sweep of train_free_convection_nde.jl (seed, optimiser rate, --spatial_causality) with --conv c among the swept architectures: the product of
 * colnde_create_fc_ensemble and colnde_create_conv.  cfg is the plain fc32 configuration, as for colnde_create_conv; model k's parameter vector has that
 * handle's layout, [w (c); b; vec(W1) 4Nz x M; b1; ...], colnde_n_params floats, the K vectors back to back.  Every kernel of a training iteration is
 * launched once for all K: the 16-column forward and adjoint kernels carry the model index in the launch grid and the filter (third entry points), the
 * padding, filter-gradient and fold kernels take the models in grid.y.  Row k of every result holds the bits a colnde_create_conv handle computes for
 * model k's weights, under either matrix arithmetic (and the same COLNDE_FC_SEG).
 * Accepted by colnde_ensemble_forward_dev, _loss_dev, _loss_grad_dev, _loss_grad, _adam_step_dev (over K x n_params), _column_loss_dev and
 * _causal_penalty_dev — there W1 is the first Dense weight of the conv chain, 4Nz x M at offset c + 1 of the model's vector, mask r < q
 * (ps[dense_layer_params_idx], train_free_convection_nde.jl:189-195) — and by the handle-level calls a free-convection ensemble accepts: n_params (the conv
 * count), conv_filter (c), n_models (K), plan (info[6] = c), describe ("models=K", "conv=c", the bytes per model, time_segments).  Everything a free-convection
 * ensemble or a conv handle refuses is refused, with a sentence naming the call.
 * Refused at creation, before any device work, each with its reason: what colnde_create_conv refuses and what colnde_create_fc_ensemble refuses (in those
 * creators' words).  Then "no HIP device ... no CPU fallback", and tapes that do not fit, with the bytes needed: all K models' tapes — the conv tape in the
 * bytes per column and save interval, the filter slab and the padded vectors in the bytes per model — are planned here as colnde_create_fc_ensemble plans
 * them. */
int colnde_create_conv_ensemble(const colnde_config* cfg, int conv_filter, int n_models, colnde_handle** out);

/* ---- the K networks of a free-convection ensemble in the embedding ocean column at once ------------------------------------------------------------------
 * What free_convection/test_free_convection_nde.jl:118-122 does with each trained network (oceananigans_convective_adjustment_nn, src/oceananigans_nn.jl:42-198):
 * per iteration progress_neural_network (:153-165), with every saved state diagnose_wT_NN (:100-118) — for every member of a sweep in ONE launch,
 * each member on its OWN column state with its own weights.  The one embedding call that accepts --conv networks.
 *   Handles: a colnde_create_fc_ensemble handle, a colnde_create_conv_ensemble handle, or a single free-convection handle as K = 1 — colnde_create or
 *   colnde_create_conv: this is how one trained --conv network is deployed (colnde_fc_embedded_step, colnde_fc_diagnose_wT and colnde_infer_* keep refusing
 *   ensembles and conv handles).  Shapes: Nz = 32 | 64 with Dense(Nz,4Nz,relu), Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1) behind the optional filter, whatever engine
 *   or stepper the handle trains with.
 *   d_weights [K][colnde_n_params] (the handle's layout; a conv member's vector leads with its filter), or NULL: the operand images the previous call on this
 *   handle packed are used again — an embedding calls with fixed weights hundreds of times, and packing K images per call rivals the kernel at these sizes.
 *   NULL on a handle that has never been given weights is an error.  The images are this call's own (tile width 16): training calls in between do not touch them.
 *   d_T [K][n_col][Nz], k = 0 deepest, the units colnde_infer_dz_wT takes; d_top_flux [n_col], SHARED by the members (they are driven by the same simulations);
 *   d_halo_bottom, d_halo_top [K][n_col] or NULL (the nearest interior value: zero-gradient fill).
 *   d_dz_wT and d_T_out [K][n_col][Nz] are one output group — both given: the forcing of T AS GIVEN, then convective_adjustment!(model, dt, K_ca), dt > 0
 *   required, d_T_out may be d_T — or both NULL (no step, dt ignored).  d_wT_faces [K][n_col][Nz+1] or NULL: diagnose_wT_NN of the state AS GIVEN.
 * Per member the arithmetic is colnde_fc_embedded_step's and colnde_fc_diagnose_wT's (above).  A conv member's filter sits in front of the dense chain exactly as in
 * training — y[i] = relu(b + sum_d w[c-1-d] x~[i+d]) (0-based) on the SCALED input x~ for i < M = Nz - c + 1, zero above, W1 padded with zero columns — and the
 * adjustment and the face gradients read the unfiltered T.  Row k of a plain ensemble is, bit for bit, what the single-model calls write for member k (at tile
 * width 16, their default up to 4,096 columns); row k of a conv ensemble is what this call writes on a colnde_create_conv handle with member k's vector.  The
 * matrix pipe is f32 MFMA under either matrix_arithmetic ("fc_embed=f32" in colnde_describe).  More than 4,096 columns per member run correctly, on the same
 * 16-column tiles.
 * Alignment: only the BASE pointers d_T, d_dz_wT, d_T_out and d_wT_faces must be 16-byte aligned.  Member k's wT_faces start k n_col (Nz + 1) floats in — not
 * a multiple of four for every n_col — and the kernel stores faces one float at a time; a member's T, dz_wT and T_out start a multiple of Nz floats in.
 * Refused, each with this call's name and the reason in colnde_last_error: a null handle, a wind-mixing or closure handle, a free-convection shape outside the
 * above, a half-given step group, neither output group given, a step with dt <= 0, K_ca < 0, n_columns < 1 or Lz <= 0, misaligned base pointers, NULL weights
 * on the first call.  Timed under colnde_kernel_time slot 9 (the launch alone; the pack is not in it).  Handle's stream, not synchronised. */
int colnde_ensemble_fc_embedded_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux, const float* d_halo_bottom,
        const float* d_halo_top, float Lz, float dt, float K_ca, float* d_dz_wT, float* d_T_out, float* d_wT_faces, int n_columns);
/* the same with host arrays (no alignment rule; the step runs in place on the uploaded T block); synchronises the stream */
int colnde_ensemble_fc_embedded(colnde_handle* h, const float* weights, const float* T, const float* top_flux, const float* halo_bottom,
        const float* halo_top, float Lz, float dt, float K_ca, float* dz_wT, float* T_out, float* wT_faces, int n_columns);

/* ---- closure-only model: fitting the five Pacanowski-Philander constants before any network is trained ------------------------------------------------
 * optimise_modified_pacanowski_philander (wind_mixing/src/diffusivity_parameter_optimisation.jl:35-231; drivers wind_mixing/optimise_modified_pacanowski_philander.jl
 * and ..._args.jl) integrates the column ODE WITHOUT the MLPs — DE(x, p, t), :1-33: eps on all three face gradients, nu on interior faces only, boundary faces
 * -(BC - scaling(0)), nu/Pr for T, Coriolis terms — and differentiates the six-term loss (loss_mpp, :150-163) with respect to nu0, nu_minus, dRi, Ric, Pr; the
 * fitted constants are the train_parameters of train_NDE_args.jl:175.  That is the wind-mixing RHS with modified_pacanowski_philander = zero_weights = 1 and every
 * network output zero.  A closure handle is a handle kind of its own: K constant sets on the same columns, every kernel launched once for all K (classical RK4,
 * `substeps` per save interval, float32; a wavefront per (set, column), a lane per level; exact discrete adjoint from a tape of step-start states; fixed-order
 * reductions — two launches on the same inputs give the same bits, and row k of a K-set launch equals a one-set launch of set k).
 * Handle-level calls that accept a closure handle: set_problem[_dev], set_stream, set_global_columns, set_profiling / kernel_time (which = 0, 1, 2) /
 * reset_kernel_times, describe ("engine=closure sets=K ... tape_bytes=..."), n_params (5), n_models (K), destroy, and colnde_adam_step_dev (any device vector).
 * Every call that takes a weight vector refuses a closure handle. */

/* The stability bound of colnde_min_substeps for these five constants (params = nu0, nu_minus, dRi, Ric, Pr): D = tau (nu0 + nu_minus) max(1, 1/Pr) / H^2,
 * whatever cfg's own constants and network fields say.  Returns -1 on an invalid configuration or a non-positive dRi or Pr.  No GPU needed. */
int colnde_closure_min_substeps(const colnde_config* cfg, const float params[5]);
/* Create: cfg.model = wind mixing with modified_pacanowski_philander = 1, 4 <= Nz <= 64; layer_sizes, n_layers and activations are ignored, and so are cfg's own
 * five constants (every solve call brings its sets).  Refused, each with its reason: convective_adjustment, smooth_NN, smooth_Ri, diurnal, inplace_variant, RKC2,
 * substeps = 0, a forced engine.  The tape (n_sets x n_columns x (n_save - 1) x substeps x 3 Nz floats) is allocated here: a handle that does not fit is refused
 * with the bytes it needs. */
int colnde_create_closure(const colnde_config* cfg, int n_sets, colnde_handle** out);
/* solve(ODEProblem(DE, ...)) of every set (diffusivity_parameter_optimisation.jl:165-170): d_params [K][5] = nu0, nu_minus, dRi, Ric, Pr per set,
 * d_sol [K][n_col][n_save][3 Nz] (NULL: keep in the handle); device memory, handle's stream, not synchronised */
int colnde_closure_forward_dev(colnde_handle* h, const float* d_params, float* d_sol);
/* loss_mpp of every set (:150-163): d_out8 [K][8] = [scaled terms(6); total; 0] */
int colnde_closure_loss_dev(colnde_handle* h, const float* d_params, const float scalings[6], float* d_out8);
/* ... and its gradient with respect to the five constants (replaces the AD of OptimizationFunction(loss_mpp, ...), :192-197): d_out [K][13], each row
 * [dL/dnu0, dL/dnu_minus, dL/ddRi, dL/dRic, dL/dPr; 6 scaled terms; total; 0] — the n_params + 8 layout of colnde_loss_grad_dev, normalised by the global
 * column count in the same way, so a sharded caller all-reduces it unchanged.  The _dev calls cannot see the values: a set that leaves the stable regime
 * yields a non-finite row and leaves every other row untouched. */
int colnde_closure_loss_grad_dev(colnde_handle* h, const float* d_params, const float scalings[6], float* d_out);
/* the same with host arrays (params [K][5], sol / out as above); they check every set against colnde_closure_min_substeps and refuse, naming the set,
 * unless COLNDE_ALLOW_UNSTABLE_DT=1; synchronise the stream */
int colnde_closure_forward(colnde_handle* h, const float* params, float* sol);
int colnde_closure_loss_grad(colnde_handle* h, const float* params, const float scalings[6], float* out);

/* ---- measurement: HIP-event timing of the handle's kernels on its stream.
 * which: 0 = forward solve kernel, 1 = adjoint kernel, 2 = gradient reduce, 3 = rhs, 4 = inference,
 * 5 = streaming dW1 GEMM (regtile engine only), 6 = convective adjustment, 7 = ADAM step, 8 = implicit diffusion,
 * 9 = free-convection embedded step / diagnose_wT (colnde_ensemble_fc_embedded too), 10 = wind-mixing flux diagnoses (colnde_wm_diagnose_flux, colnde_wm_embedded_step_flux,
 * colnde_mpp_diagnose_flux, colnde_ensemble_wm_embedded), 11 = the flux / Richardson-number launch of colnde_ensemble_profile.
 * Returns accumulated milliseconds and launch count since the last reset (synchronises the stream). */
int colnde_set_profiling(colnde_handle* h, int enabled);
int colnde_kernel_time(colnde_handle* h, int which, float* ms_total, int* n_launches);
int colnde_reset_kernel_times(colnde_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* COLNDE_H */
