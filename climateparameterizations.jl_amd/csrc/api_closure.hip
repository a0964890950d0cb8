// api_closure.hip — the closure-only model: colnde_create_closure and the colnde_closure_* entry points.
#include "api_internal.h"

// ---- closure-only model: calibrating the five Pacanowski-Philander constants (colnde_create_closure) ------------------------------------------------
// The reference fits nu0, nu_minus, dRi, Ric, Pr to the LES profiles before any network is trained (optimise_modified_pacanowski_philander,
// wind_mixing/src/diffusivity_parameter_optimisation.jl:35-231): the same column ODE without the MLPs (DE, :1-33), the same six-term loss (:150-163).
// A closure handle holds K constant sets on the same columns; every kernel (engine_closure.hip) runs once for all K.

// cfg as the closure model reads it: wind mixing, MPP, one placeholder Dense layer so that validate() has a network to look at
static colnde_config closure_config(const colnde_config* cfg, const float* params) {
    colnde_config c = *cfg;
    c.n_layers = 1;
    c.layer_sizes[0] = 3 * c.Nz;
    c.layer_sizes[1] = c.Nz - 1;
    c.activations[0] = COLNDE_ACT_IDENTITY;
    if (params) { c.nu0 = params[0]; c.nu_minus = params[1]; c.dRi = params[2]; c.Ric = params[3]; c.Pr = params[4]; }
    return c;
}

static int closure_refusals(const colnde_config* cfg) {
    if (!cfg) return fail("null config");
    if (cfg->model != COLNDE_MODEL_WIND_MIXING) return fail("the closure model is the wind-mixing column without networks: model = %d is refused", cfg->model);
    if (!cfg->modified_pacanowski_philander) return fail("the closure model IS the modified Pacanowski-Philander closure: modified_pacanowski_philander must be 1");
    if (cfg->convective_adjustment) return fail("closure model: convective_adjustment is not part of DE (diffusivity_parameter_optimisation.jl:1-33)");
    if (cfg->smooth_NN) return fail("closure model: smooth_NN filters network outputs, and there are none");
    if (cfg->smooth_Ri) return fail("closure model: smooth_Ri is not part of DE (diffusivity_parameter_optimisation.jl:1-33)");
    if (cfg->diurnal) return fail("closure model: diurnal forcing is not supported (DE takes constant boundary fluxes)");
    if (cfg->inplace_variant) return fail("closure model: inplace_variant (the NDE! evaluation arithmetic) is not supported");
    if (cfg->stepper != COLNDE_STEPPER_RK4) return fail("closure model: classical RK4 only (RKC2 is not supported)");
    if (cfg->substeps == 0) return fail("closure model: substeps = 0 (chosen from reltol) is not supported: the tape is sized at creation — pass substeps >= "
                                        "colnde_closure_min_substeps of the constants you start from");
    if (cfg->engine != COLNDE_ENGINE_AUTO) return fail("closure model: engine forced to %d, but the closure kernels are an engine of their own (use COLNDE_ENGINE_AUTO)", cfg->engine);
    if (cfg->Nz > CLOSURE_MAX_NZ) return fail("closure model: Nz = %d outside 4..%d (a lane per level)", cfg->Nz, CLOSURE_MAX_NZ);
    return 0;
}

extern "C" int colnde_closure_min_substeps(const colnde_config* cfg, const float params[5]) {
    if (!cfg || !params) { fail("null argument"); return -1; }
    for (int q = 0; q < 5; q++)
        if (!std::isfinite(params[q])) { fail("params[%d] = %g is not finite", q, params[q]); return -1; }
    if (!(params[2] > 0.0f) || !(params[4] > 0.0f)) { fail("dRi = %g and Pr = %g must be > 0", params[2], params[4]); return -1; }
    colnde_config c = closure_config(cfg, params);
    c.model = COLNDE_MODEL_WIND_MIXING;
    c.modified_pacanowski_philander = 1;
    c.convective_adjustment = 0;
    c.inplace_variant = 0;
    c.stepper = COLNDE_STEPPER_RK4;
    return colnde_min_substeps(&c);
}

extern "C" int colnde_create_closure(const colnde_config* cfg, int n_sets, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (closure_refusals(cfg)) return 1;
    const colnde_config cc = closure_config(cfg, nullptr);
    if (validate(&cc)) return 1;
    if (n_sets < 1) return fail("n_sets = %d must be >= 1", n_sets);
    if (open_device(cc.device)) return 1;
    colnde_handle* h = new (std::nothrow) colnde_handle();
    if (!h) return fail("out of host memory");
    h->cfg = cc;
    h->save_times.assign(cc.save_times, cc.save_times + cc.n_save);
    h->cfg.save_times = h->save_times.data();
    h->device = cc.device;
    h->n_col = cc.n_columns;
    h->n_col_total = cc.n_columns;
    h->closure = true;
    h->n_models = n_sets;
    PackInfo pk;
    build_model(&cc, &h->m, &pk);            // scalings and the physics prefactors; the network fields are not used
    h->m.n_params = CLOSURE_N_PARAMS;
    h->m.n_nets = 0;
    h->m.nst = 4;
    ClosureModel& cm = h->cm;
    cm.Nz = cc.Nz; cm.n_save = cc.n_save; cm.substeps = cc.substeps; cm.n_col = cc.n_columns; cm.n_sets = n_sets;
    for (int k = 0; k < 3; k++) { cm.cs[k] = h->m.cs[k]; cm.A[k] = h->m.A[k]; cm.s0[k] = h->m.s0[k]; }
    cm.B = h->m.B; cm.cor_u = h->m.cor_u; cm.cor_v = h->m.cor_v; cm.sig_u = h->m.sig_u; cm.sig_v = h->m.sig_v; cm.mu_u = h->m.mu_u; cm.mu_v = h->m.mu_v;
    cm.eps = h->m.eps;
    // the tape of all sets, the solutions and the partial rows are allocated here: a handle that does not fit is refused with the bytes it needs
    const size_t K = (size_t)n_sets, ns = (size_t)h->m.ns;
    const size_t b_tape = K * closure_tape_floats(cm) * sizeof(float), b_sol = K * h->n_col * cc.n_save * ns * sizeof(float),
                 b_rows = K * h->n_col * CLOSURE_ROW * sizeof(float), b_small = K * (CLOSURE_N_PARAMS + CLOSURE_N_PARAMS + 8) * sizeof(float),
                 b_problem = (size_t)h->n_col * (ns * (1 + cc.n_save) + 6) * sizeof(float);
    const size_t need = b_tape + b_sol + b_rows + b_small + b_problem;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { colnde_destroy(h); return fail("hipMemGetInfo failed"); }
    const size_t margin = (size_t)1 << 30;
    if (need + margin > free_b) {
        colnde_destroy(h);
        return fail("a closure handle of %d sets x %d columns needs %zu bytes of device memory (%zu of them the step-start tape: %d save intervals x %d substeps x "
                    "%zu floats per column and set); %zu bytes are free (1 GB kept in reserve): use fewer sets per handle",
                    n_sets, cc.n_columns, need, b_tape, cc.n_save - 1, cc.substeps, ns, free_b);
    }
    h->cl_tape_bytes = b_tape;
    DevPool& mem = h->mem;
    hipError_t e = mem.alloc(&h->d_cl_tape, b_tape / sizeof(float));
    if (e == hipSuccess) e = mem.alloc(&h->d_sol, b_sol / sizeof(float));
    if (e == hipSuccess) e = mem.alloc(&h->d_cl_rows, b_rows / sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->d_cl_rows, 0, b_rows);
    if (e == hipSuccess) e = mem.alloc(&h->d_cl_params, K * CLOSURE_N_PARAMS);
    if (e == hipSuccess) e = mem.alloc(&h->d_out, K * (CLOSURE_N_PARAMS + 8));
    if (e == hipSuccess) e = mem.alloc(&h->d_x0, (size_t)h->n_col * ns);
    if (e == hipSuccess) e = mem.alloc(&h->d_bcs, (size_t)h->n_col * 6);
    if (e == hipSuccess) e = mem.alloc(&h->d_times, (size_t)cc.n_save);
    if (e == hipSuccess) e = hipMemcpy(h->d_times, h->save_times.data(), sizeof(float) * cc.n_save, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        colnde_destroy(h);
        return fail("allocating the closure handle's buffers (%zu bytes, %zu of them tape) failed: %s", need, b_tape, hipGetErrorString(e));
    }
    *out = h;
    return 0;
}

static int closure_only(const colnde_handle* h) {
    if (!h) return fail("null handle");
    if (h->conv.c) return fail("colnde_closure_* take the handles of colnde_create_closure: this is a colnde_create_conv handle (conv=%d)", h->conv.c);
    if (!h->closure) return fail("not a closure handle: colnde_closure_* take the handles of colnde_create_closure");
    return 0;
}

// host-side stability check of every set (the _dev calls cannot see the values)
static int closure_check_sets(const colnde_handle* h, const float* params) {
    const bool allow = allow_unstable();
    for (int k = 0; k < h->n_models; k++) {
        const float* r = params + (size_t)CLOSURE_N_PARAMS * k;
        const int ms = colnde_closure_min_substeps(&h->cfg, r);
        if (ms < 0) return fail("set %d: %s", k, std::string(colnde_last_error()).c_str());
        if (h->cfg.substeps < ms && !allow)
            return fail("set %d (nu0 = %g, nu_minus = %g, Pr = %g) needs substeps >= %d for a stable RK4 step (colnde_closure_min_substeps), but the handle runs "
                        "substeps = %d (COLNDE_ALLOW_UNSTABLE_DT=1 overrides)", k, r[0], r[1], r[4], ms, h->cfg.substeps);
    }
    return 0;
}

static int closure_forward_impl(colnde_handle* h, const float* d_params, float* d_sol, bool with_tape, bool with_loss) {
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    Timed tm(h, K_FORWARD);
    hipError_t e = closure_launch_forward(h->cm, d_params, h->d_x0, h->d_bcs, h->d_times, d_sol, with_tape ? h->d_cl_tape : nullptr,
                                          with_loss ? h->d_truth : nullptr, with_loss ? h->d_cl_rows : nullptr, h->stream);
    if (e != hipSuccess) return fail("closure forward launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_closure_forward_dev(colnde_handle* h, const float* d_params, float* d_sol) {
    if (closure_only(h)) return 1;
    if (!d_params) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    return closure_forward_impl(h, d_params, d_sol ? d_sol : h->d_sol, false, false);
}

extern "C" int colnde_closure_loss_dev(colnde_handle* h, const float* d_params, const float scalings[6], float* d_out8) {
    if (closure_only(h)) return 1;
    if (!d_params || !scalings || !d_out8) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    if (closure_forward_impl(h, d_params, h->d_sol, false, true)) return 1;
    Timed tm(h, K_REDUCE);
    hipError_t e = closure_launch_reduce(h->cm, h->d_cl_rows, lw, false, d_out8, h->stream);
    if (e != hipSuccess) return fail("closure reduce launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_closure_loss_grad_dev(colnde_handle* h, const float* d_params, const float scalings[6], float* d_out) {
    if (closure_only(h)) return 1;
    if (!d_params || !scalings || !d_out) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    if (closure_forward_impl(h, d_params, h->d_sol, true, true)) return 1;
    {
        Timed tm(h, K_ADJOINT);
        hipError_t e = closure_launch_adjoint(h->cm, d_params, h->d_bcs, h->d_times, h->d_sol, h->d_truth, h->d_cl_tape, lw, h->d_cl_rows, h->stream);
        if (e != hipSuccess) return fail("closure adjoint launch failed: %s", hipGetErrorString(e));
    }
    Timed tm(h, K_REDUCE);
    hipError_t e = closure_launch_reduce(h->cm, h->d_cl_rows, lw, true, d_out, h->stream);
    if (e != hipSuccess) return fail("closure reduce launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_closure_forward(colnde_handle* h, const float* params, float* sol) {
    if (closure_only(h)) return 1;
    if (!params) return fail("null pointer argument");
    if (closure_check_sets(h, params)) return 1;
    HIPCHK(hipSetDevice(h->device));
    const size_t K = (size_t)h->n_models;
    HIPCHK(hipMemcpyAsync(h->d_cl_params, params, sizeof(float) * K * CLOSURE_N_PARAMS, hipMemcpyHostToDevice, h->stream));
    if (closure_forward_impl(h, h->d_cl_params, h->d_sol, false, false)) return 1;
    if (sol)
        HIPCHK(hipMemcpyAsync(sol, h->d_sol, sizeof(float) * K * h->n_col * h->cfg.n_save * h->m.ns, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int colnde_closure_loss_grad(colnde_handle* h, const float* params, const float scalings[6], float* out) {
    if (closure_only(h)) return 1;
    if (!params || !scalings || !out) return fail("null pointer argument");
    if (closure_check_sets(h, params)) return 1;
    HIPCHK(hipSetDevice(h->device));
    const size_t K = (size_t)h->n_models;
    HIPCHK(hipMemcpyAsync(h->d_cl_params, params, sizeof(float) * K * CLOSURE_N_PARAMS, hipMemcpyHostToDevice, h->stream));
    if (colnde_closure_loss_grad_dev(h, h->d_cl_params, scalings, h->d_out)) return 1;
    HIPCHK(hipMemcpyAsync(out, h->d_out, sizeof(float) * K * (CLOSURE_N_PARAMS + 8), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
