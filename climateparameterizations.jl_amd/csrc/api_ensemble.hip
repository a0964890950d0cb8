// api_ensemble.hip — handles built on colnde_create: wind-mixing and free-convection ensembles, the conv network and its ensembles; the colnde_ensemble_* entry points.
#include "api_internal.h"
#include "tape_plan.h"

// ---- ensembles: K models of one architecture side by side (colnde_create_ensemble) ---------------------------------------------------------------
// The reference's sweep (wind_mixing/train_NDE_args.jl: activation, ADAM rate and Pacanowski-Philander constants per process) trains many small
// models of ONE architecture on the same simulations.  Here every kernel of a training iteration runs once for all K models with the model index in
// blockIdx.y: the net-split pair (rt16sh_*), the weight packers, tile16's dW GEMM, the loss and gradient reductions and the ADAM step.  A model owns
// its packed weights, solution, tapes and slab rows (RtEns strides) and its closure constants (RtPhys); x0, bcs and truth are shared.

// the configuration of model k: cfg with row k of physics ([K][5]: nu0, nu_minus, dRi, Ric, Pr)
colnde_config model_config(const colnde_config* cfg, const float* physics, int k) {
    colnde_config c = *cfg;
    if (physics) {
        const float* r = physics + (size_t)5 * k;
        c.nu0 = r[0]; c.nu_minus = r[1]; c.dRi = r[2]; c.Ric = r[3]; c.Pr = r[4];
    }
    return c;
}

// The shared sub-step count against every model's stability bound; RKC2 with automatic stages: the largest stage count any model needs.
// *min_sub / *stages: the ensemble's bound and stage count (stages = 0 for RK4).
static int ens_stability(const colnde_config* cfg, int K, const float* physics, int* min_sub, int* stages) {
    *min_sub = 1;
    *stages = 0;
    for (int k = 0; k < K; k++) {
        const colnde_config c = model_config(cfg, physics, k);
        if (physics) {
            const float* r = physics + (size_t)5 * k;
            for (int q = 0; q < 5; q++)
                if (!std::isfinite(r[q])) return fail("physics[%d][%d] = %g is not finite", k, q, r[q]);
            if (!(c.dRi > 0.0f) || !(c.Pr > 0.0f)) return fail("physics[%d]: dRi = %g and Pr = %g must be > 0", k, c.dRi, c.Pr);
        }
        const int ms = colnde_min_substeps(&c);
        if (ms < 0) return 1;
        *min_sub = std::max(*min_sub, ms);
        if (cfg->stepper == COLNDE_STEPPER_RKC2 && !cfg->rkc_stages) *stages = std::max(*stages, colnde_rkc_stages(&c));
        if (cfg->substeps < ms && !allow_unstable())
            return fail("model %d (nu0 = %g, nu_minus = %g, Pr = %g) needs substeps >= %d for a stable step (colnde_min_substeps; lambda = -%.4g), but the "
                        "ensemble shares substeps = %d (COLNDE_ALLOW_UNSTABLE_DT=1 overrides)", k, c.nu0, c.nu_minus, c.Pr, ms, stiff_lambda(&c), cfg->substeps);
    }
    return 0;
}

static int ens_upload_physics(colnde_handle* h, const float* physics) {
    std::vector<RtPhys> ph((size_t)h->n_models);
    for (int k = 0; k < h->n_models; k++) {
        const colnde_config c = model_config(&h->cfg, physics, k);
        ph[k] = closure_constants(c.nu0, c.nu_minus, c.dRi, c.Ric, c.Pr);
        // tile16's physics also reads dRi and Pr themselves (build_model: m->dRi = c->dRi, m->Pr = c->Pr): a tile ensemble's table carries them in the pads
        if (h->tile_ens) { ph[k].pad0 = c.dRi; ph[k].pad1 = c.Pr; }
    }
    // (kernels in flight on the stream may still read the previous table: the copy is ordered on the stream and completed before returning)
    HIPCHK(hipMemcpyAsync(h->d_phys, ph.data(), ph.size() * sizeof(RtPhys), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->phys_host.swap(ph);
    if (physics) h->phys_raw.assign(physics, physics + (size_t)5 * h->n_models);
    else h->phys_raw.clear();
    return 0;
}

// The tapes of all K models, planned once at creation: tile16's taped-dW formats for ONE block of all columns per model (the net-split pair has no
// column-block loop across models), the rich tape by tape_plan.h's plan_t16_ens_tapes.  Refused with the bytes it needs when it does not fit.
static int ens_plan_tapes(colnde_handle* h) {
    const DevModel& m = h->m;
    const int K = h->n_models;
    const size_t n_rec = sched_records((size_t)h->n_tiles, total_steps(h), m.nst);
    const size_t R = dwtape_row_floats(m), P8 = (size_t)m.n_params + 8;
    h->blk.block = h->n_tiles * CT;
    h->blk.nblocks = 1;
    build_dw_plan(h, n_rec);                                 // the slice count a single handle of this size plans: same reduction order (and h->blk.rows, ens.slab)
    const size_t f_tape = n_rec * CT * m.ns, f_dw = n_rec * CT * R, f_rich = n_rec * rt_split_rich_record_floats(),
                 f_plain = n_rec * CT * t16_ztape_col_floats(m), f_sol = (size_t)h->n_col * h->cfg.n_save * m.ns, f_img = RT_IMG_STRIDE;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t budget = hbm_budget(free_b, ((size_t)3 << 30) + (size_t)K * (P8 * 2 + 256 * 8) * sizeof(float));
    auto per_model = [&](size_t f_z) { return (f_tape + f_dw + f_z + h->ens.slab + f_sol + f_img) * sizeof(float); };
    const T16EnsTapes plan = plan_t16_ens_tapes(K, h->n_tiles, per_model(f_rich), per_model(f_plain), budget, env_flag(ENV_T16_SPLIT_RICH));
    const size_t need = plan.bytes_per_model;
    if (plan.refused)
        return fail("an ensemble of %d models needs %zu bytes of device memory for its tapes, slab rows and solutions (%zu per model, %s tape, "
                    "%d substeps x %d stages x %d save intervals); %zu bytes are free (3 GB kept in reserve): use fewer models per handle",
                    K, (size_t)K * need, need, plan.rich ? "rich" : "plain", h->cfg.substeps, m.nst, h->cfg.n_save - 1, free_b);
    const size_t mark = h->mem.mark();
    int at = 0;
    hipError_t e = t16_alloc_tapes(h, (size_t)K, n_rec, &at);
    if (e == hipSuccess) e = t16_alloc_ztape(h, (size_t)K, n_rec, plan.rich);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->mem.rollback(mark);
        return fail("allocating the ensemble's tapes (%zu bytes, %zu per model) failed: %s", (size_t)K * need, need, hipGetErrorString(e));
    }
    h->t16_dwtape = 1;
    h->split_rich = plan.rich;
    h->ens.wimg = f_img;
    h->ens.sol = f_sol;
    h->ens.tape = f_tape;
    h->ens.ztape = plan.rich ? f_rich : f_plain;
    h->ens.dwtape = f_dw;
    h->ens.n_models = K;
    h->ens.phys = h->d_phys;
    h->ens_model_bytes = need;
    return 0;
}

// colnde_set_schedule on an ensemble: its tapes were sized at creation for (n_save - 1) x substeps steps, so they are planned again for the total in force
int ens_replan_tapes(colnde_handle* h) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->mem.release(&h->d_dwtape);
    h->mem.release(&h->d_tape);
    h->mem.release(&h->d_t16_ztape);
    h->mem.release(&h->d_slab);
    h->mem.release(&h->d_macros);
    h->mem.release(&h->d_split_macros);
    h->t16_dwtape = -1;
    return ens_plan_tapes(h);
}

extern "C" int colnde_create_ensemble(const colnde_config* cfg, int n_models, const float* physics, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (validate(cfg)) return 1;
    if (n_models < 1 || n_models > 65535) return fail("n_models = %d outside 1..65535", n_models);
    // only the configurations on which AUTO runs the four-wave net-split pair: those kernels carry the model index
    if (cfg->model != COLNDE_MODEL_WIND_MIXING)
        return fail("ensembles cover the wind-mixing NDE on the net-split kernels: the free-convection models (fc32 / tile16) run one handle per model");
    if (cfg->inplace_variant) return fail("ensembles train on the training RHS: inplace_variant (the NDE! evaluation RHS) is not supported");
    if (cfg->engine != COLNDE_ENGINE_AUTO)
        return fail("ensembles run the net-split kernels engine AUTO selects: engine forced to %d is not supported (those engines have no model index)", cfg->engine);
    if (cfg->substeps == 0)
        return fail("substeps = 0 (chosen from reltol by the first solve) is not supported: the models share one sub-step count, and the tapes are sized at "
                    "creation — choose it with a single handle (colnde_choose_substeps) and pass it");
    if (cfg->n_columns > 8192)
        return fail("%d columns per model: ensembles cover the net-split range (at most 8,192 columns per model); above it regtile runs one handle per model",
                    cfg->n_columns);
    {
        DevModel dm;
        PackInfo pk;
        build_model(cfg, &dm, &pk);
        if (!rt_supported(dm))
            return fail("ensembles cover the net-split shape only (Nz = 32, three 96-50-20-31 nets, one hidden activation, training RHS, no smoothing): "
                        "wide networks and other architectures run one handle per model");
    }
    if (physics && !cfg->modified_pacanowski_philander)
        return fail("a physics array needs modified_pacanowski_philander = 1: without the Richardson-number closure the five constants are unused (pass NULL)");
    // the environment switches that send a single handle down paths without a model index
    for (EnvSwitch sw : {ENV_T16_FWD_HELPER, ENV_T16_ADJ_HELPER, ENV_T16_FWD_SPLIT, ENV_T16_ADJ_SPLIT, ENV_T16_ZTAPE, ENV_T16_DWTAPE}) {
        const char* e = env_get(sw);
        if (e && *e && atoi(e) == 0)
            return fail("%s=0 selects kernels without a model index (the three-wave or tile16 kernels, or no delta / pre-activation tape): ensembles refuse it", env_name(sw));
    }
    if (env_get(ENV_T16_BLOCK)) return fail("COLNDE_T16_BLOCK: ensembles hold one block of columns per model (the column-block loop has no model index)");
    int min_sub = 1, stages = 0;
    if (ens_stability(cfg, n_models, physics, &min_sub, &stages)) return 1;
    colnde_handle* h = nullptr;
    if (colnde_create(cfg, &h)) return 1;
    if (h->use_rt || h->use_fc || h->ag_rows || !h->fwd_split || !h->adj_split || !h->fwd_helper || !h->adj_helper) {
        colnde_destroy(h);
        return fail("this configuration does not run the four-wave net-split pair under engine AUTO: ensembles refuse it");
    }
    h->ensemble = true;
    h->n_models = n_models;
    h->min_substeps = min_sub;
    if (stages > 0 && stages != h->m.nst) {
        h->ens_rkc_stages = stages;
        if (refresh_rkc(h)) { colnde_destroy(h); return 1; }
    } else if (stages > 0) {
        h->ens_rkc_stages = stages;
    }
    const size_t K = (size_t)n_models, P = (size_t)h->m.n_params;
    DevPool& mem = h->mem;
    if (mem.resize(&h->d_w, K * P) || mem.resize(&h->d_out, K * (P + 8)) || mem.resize(&h->d_partial, K * 256 * 8) ||
        mem.resize(&h->d_sol, K * h->n_col * h->cfg.n_save * h->m.ns) || mem.resize(&h->d_wimg, K * RT_IMG_STRIDE) || mem.alloc(&h->d_phys, K)) {
        colnde_destroy(h);
        return fail("allocating the ensemble's per-model buffers (%d models) failed", n_models);
    }
    if (ens_upload_physics(h, physics) || ens_plan_tapes(h)) { colnde_destroy(h); return 1; }
    *out = h;
    return 0;
}

// ---- tile ensembles (colnde_create_tile_ensemble): K wind-mixing models of ANY tile16 architecture side by side ------------------------------------
// The reference's wide nets (wind_mixing/train_NDE.jl:97-102, train_NDE_args.jl:150-166: 96-400-400-31, 96-32-400-31, 96-400-31) are swept like the small
// one, one model per process at 8-18 simulations: one 16-column workgroup each.  Here tile16's own kernels carry the model index in blockIdx.y
// (pack_weights_ens_kernel, pack_planes_ens_kernel, forward_ens_kernel, adjoint_ens_kernel; T16Ens strides); the dW GEMM, the loss and gradient
// reductions and the ADAM step already do.  The launch geometry — weights in LDS or streamed, rows in LDS or in global memory, the taped adjoint's
// form, the dW slice count — is decided from ONE model's tiles, so that row k of every result is, bit for bit, what a colnde_create handle with
// engine GENERIC computes for model k's weights and constants.

// Decided from the configuration and the environment alone, before any device work
static int tile_ens_refusals(const colnde_config* cfg, int n_models, const float* physics) {
    const size_t lds_cap = 160 * 1024;
    if (n_models < 1 || n_models > 65535) return fail("n_models = %d outside 1..65535", n_models);
    if (cfg->model != COLNDE_MODEL_WIND_MIXING)
        return fail("colnde_create_tile_ensemble covers the wind-mixing NDE: the free-convection models train side by side through colnde_create_fc_ensemble");
    if (cfg->inplace_variant) return fail("tile ensembles train on the training RHS: inplace_variant (the NDE! evaluation RHS) is not supported");
    if (cfg->engine != COLNDE_ENGINE_AUTO && cfg->engine != COLNDE_ENGINE_GENERIC)
        return fail("tile ensembles run the tile16 kernels (engine AUTO or GENERIC): engine forced to %d is not supported (regtile and fc32 have no such entry points)", cfg->engine);
    if (cfg->substeps == 0)
        return fail("substeps = 0 (chosen from reltol by the first solve) is not supported: the models share one sub-step count, and the tapes are sized at "
                    "creation — choose it with a single handle (colnde_choose_substeps) and pass it");
    if (cfg->n_columns > 4096)
        return fail("%d columns per model: tile ensembles cover at most 4,096 columns per model (256 tiles: the regime of the 1,024-thread kernels a single handle "
                    "runs there); above it one handle per model", cfg->n_columns);
    for (EnvSwitch sw : {ENV_T16_DWTAPE, ENV_T16_ZTAPE}) {
        const char* e = env_get(sw);
        if (e && atoi(e) == 0) return fail("%s=0 leaves no delta / pre-activation tape: tile ensembles run the taped adjoint only and refuse it", env_name(sw));
    }
    if (env_get(ENV_T16_BLOCK)) return fail("COLNDE_T16_BLOCK: tile ensembles hold one block of columns per model (the column-block loop has no model index)");
    {
        const char* e = env_get(ENV_T16_TAPE_THREADS);
        if (e && atoi(e) != 1024) return fail("COLNDE_T16_TAPE_THREADS=%s selects the 512-thread taped adjoint, which has no model index: tile ensembles refuse it", e);
        e = env_get(ENV_T16_FWD_SPLIT);
        if (e && atoi(e) != 0) return fail("COLNDE_T16_FWD_SPLIT=%s selects the net-split kernels: tile ensembles run tile16's own (colnde_create_ensemble runs those)", e);
    }
    if (physics && !cfg->modified_pacanowski_philander)
        return fail("a physics array needs modified_pacanowski_philander = 1: without the Richardson-number closure the five constants are unused (pass NULL)");
    DevModel dm;
    PackInfo pk;
    build_model(cfg, &dm, &pk);
    const size_t lds_fwd = lds_floats_forward(dm) * sizeof(float), lds_fwd_ag = lds_floats_forward_ag(dm) * sizeof(float);
    const bool ag_rows = lds_fwd > lds_cap;
    if (ag_rows && lds_fwd_ag > lds_cap)
        return fail("network too large for the tile engine: forward needs %zu B of LDS (> %zu), %zu B even with the activation rows in global memory", lds_fwd, lds_cap, lds_fwd_ag);
    // the single handle's decision (tape_plan.h) on a card with room for everything: what remains is whether the taped adjoint can run this network at all
    const size_t lds_ag = (MODEL_FLOATS + lds_floats_adjoint_ag(dm)) * sizeof(float);
    const T16Tapes plan = plan_t16_tapes({(cfg->n_columns + CT - 1) / CT * CT, CT, dm.ns, dm.n_bias, ag_rows, false, (MODEL_FLOATS + lds_floats_adjoint(dm)) * sizeof(float),
                                          (MODEL_FLOATS + lds_floats_adjoint_noA(dm)) * sizeof(float), lds_ag, 1, 1, (size_t)1 << 40, FLAG_UNSET, FLAG_UNSET, FLAG_OFF, 0});
    if (plan.status == T16_PLAN_REFUSED_TOO_LARGE)
        return fail("network too large for the taped adjoint with rows in global memory (%d biases, %zu B of LDS): no gradient path, no tile ensemble", dm.n_bias, lds_ag);
    if (plan.status != T16_PLAN_TAPED)
        return fail("the taped adjoint cannot run this network (16 x %d state values per tile against 3,072, or %zu B of LDS without the activation array against %zu): "
                    "tile ensembles have no in-register adjoint", dm.ns, (MODEL_FLOATS + lds_floats_adjoint_noA(dm)) * sizeof(float), lds_cap);
    if (CT * dm.ns > 2 * 1024 || dm.n_bias > 4 * 1024)
        return fail("Nz = %d (%d biases): tile ensembles run the 1,024-thread taped adjoint, which holds 16 x ns <= 2,048 state values and 4,096 biases per tile; a "
                    "single handle runs this network on the 512-thread kernels, which have no model index", cfg->Nz, dm.n_bias);
    return 0;
}

// the K models' weight images (and, with the rows in global memory under the split arithmetic, plane images) in one launch each
static int tile_ens_pack(colnde_handle* h, const float* d_weights, const T16Ens& en) {
    hipError_t e = launch_pack_ens(h->m, h->pk, d_weights, h->d_wf, h->d_wb, en, h->stream);
    if (e != hipSuccess) return fail("tile ensemble pack_weights launch failed: %s", hipGetErrorString(e));
    if (h->d_sf && (h->m.sf || h->m.sb)) {
        e = launch_pack_planes_ens(h->m, d_weights, h->d_sf, h->d_sb, en, h->stream);
        if (e != hipSuccess) return fail("tile ensemble pack_planes launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

static T16Ens tile_ens_strides(const colnde_handle* h) {
    T16Ens en = h->tens;
    en.phys = h->d_phys;
    en.slab = h->ens.slab;            // (follows the dW slice count: dw_slab_rows, replan_dw_slices)
    return en;
}

static int tile_ens_forward(colnde_handle* h, const float* d_weights, float* d_sol, bool with_tape) {
    const T16Ens en = tile_ens_strides(h);
    // every (model, tile) workgroup its own rows of m.ag: K x tiles slabs, sized and zero-filled at creation
    if (h->ag_rows && h->ag_tiles < (size_t)h->n_models * h->n_tiles) return fail("the activation rows hold %zu tiles, the ensemble needs %zu", h->ag_tiles, (size_t)h->n_models * h->n_tiles);
    if (tile_ens_pack(h, d_weights, en)) return 1;
    Timed tm(h, K_FORWARD);
    const hipError_t e = launch_forward_ens(h->m, h->pk, d_weights, h->d_wf, h->d_x0, h->d_bcs, h->d_times, h->cfg.n_save, h->cfg.substeps, d_sol,
                                            with_tape ? h->d_tape : nullptr, h->n_col, h->fwd_threads, h->fwd_wlds, h->lds_fwd_solve, en, h->stream,
                                            with_tape ? h->d_t16_ztape : nullptr);
    if (e != hipSuccess) return fail("tile ensemble forward launch failed: %s", hipGetErrorString(e));
    return 0;
}

static size_t tile_ens_adjoint_lds(const colnde_handle* h) {
    return (MODEL_FLOATS + (h->ag_rows ? lds_floats_adjoint_ag(h->m) : lds_floats_adjoint_noA(h->m))) * sizeof(float);
}

static int tile_ens_loss_grad(colnde_handle* h, const float* d_weights, const float* scalings, float* d_out) {
    const int K = h->n_models, stride = h->m.n_params + 8;
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    HIPCHK(hipMemsetAsync(h->d_slab, 0, (size_t)K * h->ens.slab * sizeof(float), h->stream));
    if (tile_ens_forward(h, d_weights, h->d_sol, true)) return 1;
    const T16Ens en = tile_ens_strides(h);
    hipError_t e;
    {
        Timed tm(h, K_ADJOINT);
        e = launch_adjoint_ens(h->m, h->pk, d_weights, h->d_wf, h->d_wb, h->d_bias_zoff, h->d_bias_goff, h->d_bcs, h->d_times, h->cfg.n_save, h->cfg.substeps, h->d_sol,
                               h->d_truth, h->d_tape, lw, h->d_slab, h->n_col, tile_ens_adjoint_lds(h), en, h->stream, h->d_dwtape, h->d_t16_ztape);
        if (e != hipSuccess) return fail("tile ensemble adjoint launch failed: %s", hipGetErrorString(e));
    }
    {
        Timed tm(h, K_DW1);
        e = dw_launch(h, (size_t)h->n_tiles * total_steps(h) * h->m.nst, h->d_slab + (size_t)h->n_tiles * stride, K, en.dwtape, en.slab);
        if (e != hipSuccess) return fail("tile ensemble dW GEMM launch failed: %s", hipGetErrorString(e));
    }
    {
        Timed tm(h, K_REDUCE);
        e = launch_reduce(h->d_slab, h->blk.rows, h->m.n_params, stride, lw, d_out, h->stream, K, en.slab, stride);
        if (e != hipSuccess) return fail("tile ensemble reduce launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

// One block of all columns per model, planned once at creation (tape_plan.h: plan_t16_tile_ens); the dW slice count is the one a single handle of this
// size plans (build_dw_plan): the same reduction order, and with it the bits
static int tile_ens_plan_tapes(colnde_handle* h) {
    const DevModel& m = h->m;
    const int K = h->n_models, n_steps = total_steps(h);
    const size_t n_rec = (size_t)h->n_tiles * n_steps * m.nst;
    h->blk.block = h->n_tiles * CT;
    h->blk.nblocks = 1;
    build_dw_plan(h, n_rec);                                 // (and h->blk.rows, ens.slab)
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t img = ((size_t)h->pk.pf_net + h->pk.pb_net) * m.n_nets, planes = h->ag_rows ? ((size_t)m.sf_net + m.sb_net) * m.n_nets * 4 : 0;
    const T16TileEns plan = plan_t16_tile_ens({K, h->n_tiles, n_steps, m.nst, m.ns, m.n_params, h->n_col, h->cfg.n_save, h->blk.rows, dwtape_row_floats(m),
                                               t16_ztape_col_floats(m), img, planes, h->ag_rows ? ag_floats_per_tile(m) : 0, free_b});
    if (plan.refused)
        return fail("a tile ensemble of %d models needs %zu bytes of device memory for its tapes, slab rows, solutions, weight images and activation rows (%zu per "
                    "model: %d substeps x %d stages x %d save intervals); %zu bytes are free (3 GB kept in reserve, %zu per model): use fewer models per handle",
                    K, (size_t)K * plan.bytes_per_model, plan.bytes_per_model, h->cfg.substeps, m.nst, h->cfg.n_save - 1, free_b, plan.share);
    const size_t mark = h->mem.mark();
    int at = 0;
    hipError_t e = t16_alloc_tapes(h, (size_t)K, n_rec, &at);
    if (e == hipSuccess) e = t16_alloc_ztape(h, (size_t)K, n_rec, false);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->mem.rollback(mark);
        return fail("allocating the tile ensemble's tapes (%zu bytes, %zu per model) failed: %s", (size_t)K * plan.bytes_per_model, plan.bytes_per_model, hipGetErrorString(e));
    }
    h->t16_dwtape = 1;
    h->tens.tape = n_rec * CT * m.ns;
    h->tens.dwtape = n_rec * CT * dwtape_row_floats(m);
    h->tens.ztape = n_rec * CT * t16_ztape_col_floats(m);
    h->ens_model_bytes = plan.bytes_per_model;
    return 0;
}

extern "C" int colnde_create_tile_ensemble(const colnde_config* cfg, int n_models, const float* physics, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (validate(cfg)) return 1;
    if (tile_ens_refusals(cfg, n_models, physics)) return 1;
    int min_sub = 1, stages = 0;
    if (ens_stability(cfg, n_models, physics, &min_sub, &stages)) return 1;
    // tile16's own kernels, as a single handle runs them under engine GENERIC (AUTO would send the 96-50-20-31 shape to the net-split pair)
    colnde_config c = *cfg;
    c.engine = COLNDE_ENGINE_GENERIC;
    colnde_handle* h = nullptr;
    if (colnde_create(&c, &h)) return 1;
    const size_t lds_cap = 160 * 1024;
    if (h->use_rt || h->use_fc || h->fwd_split || h->adj_split || !forward_ens_has(h->fwd_wlds, h->fwd_threads, h->ag_rows)) {
        const int th = h->fwd_threads, wl = h->fwd_wlds;
        colnde_destroy(h);
        return fail("this configuration's forward solve (weights in LDS: %d, %d threads; COLNDE_FWD_WLDS / COLNDE_FWD_THREADS) has no tile-ensemble entry point", wl, th);
    }
    if (h->lds_fwd_solve + t16_ens_forward_lds_extra() > lds_cap || !adjoint_ens_has(h->m, h->n_tiles, tile_ens_adjoint_lds(h))) {
        const size_t need = h->lds_fwd_solve + t16_ens_forward_lds_extra();
        colnde_destroy(h);
        return fail("the ensemble kernels keep the model description in LDS beside the tile: %zu B against %zu (or the taped adjoint of this network has no 1,024-thread "
                    "form): one handle per model", need, lds_cap);
    }
    h->ensemble = true;
    h->tile_ens = true;
    h->n_models = n_models;
    h->min_substeps = min_sub;
    if (stages > 0 && stages != h->m.nst) {
        h->ens_rkc_stages = stages;
        if (refresh_rkc(h)) { colnde_destroy(h); return 1; }
    } else if (stages > 0) {
        h->ens_rkc_stages = stages;
    }
    const size_t K = (size_t)n_models, P = (size_t)h->m.n_params;
    T16Ens& en = h->tens;
    en.n_models = n_models;
    en.w = P;
    en.wf = (size_t)h->pk.pf_net * h->m.n_nets;
    en.wb = (size_t)h->pk.pb_net * h->m.n_nets;
    en.sf = h->ag_rows ? (size_t)h->m.sf_net * h->m.n_nets * 4 : 0;
    en.sb = h->ag_rows ? (size_t)h->m.sb_net * h->m.n_nets * 4 : 0;
    en.sol = (size_t)h->n_col * h->cfg.n_save * h->m.ns;
    h->ens.sol = en.sol;
    h->ens.n_models = n_models;
    DevPool& mem = h->mem;
    if (mem.resize(&h->d_w, K * P) || mem.resize(&h->d_out, K * (P + 8)) || mem.resize(&h->d_partial, K * 256 * 8) || mem.resize(&h->d_sol, K * en.sol) ||
        mem.resize(&h->d_wf, K * en.wf) || mem.resize(&h->d_wb, K * en.wb) || mem.alloc(&h->d_phys, K) ||
        (h->ag_rows && (mem.resize(&h->d_sf, K * en.sf) || mem.resize(&h->d_sb, K * en.sb)))) {
        colnde_destroy(h);
        return fail("allocating the tile ensemble's per-model buffers (%d models) failed", n_models);
    }
    resolve_arithmetic(h);                                   // (m.sf / m.sb: the plane images just re-allocated)
    // K x tiles slabs of activation rows, zero-filled in stream order: no two (model, tile) workgroups share one
    if (ensure_ag(h, K * (size_t)h->n_tiles)) { colnde_destroy(h); return 1; }
    if (ens_upload_physics(h, physics) || tile_ens_plan_tapes(h)) { colnde_destroy(h); return 1; }
    *out = h;
    return 0;
}

extern "C" int colnde_n_models(const colnde_handle* h) { return h ? h->n_models : -1; }

// ---- free-convection ensembles (colnde_create_fc_ensemble) ------------------------------------------------------------------------------------------
// The reference trains the free-convection NDE on 3 to 9 simulations (train_free_convection_nde.jl, --training-simulations): one 16-column workgroup.  Its
// sweep (one process per seed / optimiser rate / penalty setting) and the judging of a run (compute_nde_solution_history, testing.jl:1-32: the network of
// EVERY epoch re-solved on every simulation) are both "many networks, same few columns".  Here the 16-column fc32 kernels carry the model index in
// blockIdx.y (FcEns: the strides of what a model owns), tile16's dW GEMM, the reductions and the ADAM step already do; row k of every result is, bit for
// bit, what a colnde_create handle computes for model k's weights (under the same COLNDE_FC_SEG: the segment count orders the gradient's sums).

// Decided from the configuration and the environment alone, before any device work
static int fc_ens_refusals(const colnde_config* cfg, int n_models) {
    if (n_models < 1 || n_models > 65535) return fail("n_models = %d outside 1..65535", n_models);
    if (cfg->model == COLNDE_MODEL_WIND_MIXING)
        return fail("colnde_create_fc_ensemble covers the free-convection models (FreeConvectionNDE, ConvectiveAdjustmentNDE): a wind-mixing ensemble is colnde_create_ensemble's");
    if (cfg->engine != COLNDE_ENGINE_AUTO && cfg->engine != COLNDE_ENGINE_FC32)
        return fail("free-convection ensembles run the fc32 kernels (engine AUTO or FC32): engine forced to %d has no model index", cfg->engine);
    {
        DevModel dm;
        PackInfo pk;
        build_model(cfg, &dm, &pk);
        if (!fc_supported(dm, cfg->stepper))
            return fail("free-convection ensembles cover the fc32 shape only: FreeConvectionNDE (RK4) or ConvectiveAdjustmentNDE (RK4, RKC2) with Dense(Nz,4Nz,relu), "
                        "Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1), Nz = 32 or 64 (Nz = %d, %d layers here); other networks run one handle per model", cfg->Nz, cfg->n_layers);
    }
    if (cfg->substeps == 0)
        return fail("substeps = 0 (chosen from reltol by the first solve) is not supported: the models share one sub-step count, and the tapes are sized at "
                    "creation — choose it with a single handle (colnde_choose_substeps) and pass it");
    if (refuse_unstable_substeps(cfg)) return 1;
    if (cfg->n_columns > 4096)
        return fail("%d columns per model: free-convection ensembles cover the 16-column tiles (at most 4,096 columns per model, fc_tile_width); above it the 32-column "
                    "kernels run one handle per model", cfg->n_columns);
    // the switches that send a single handle to kernels without a model index
    {
        const char* e = env_get(ENV_FC);
        if (e && *e && atoi(e) == 0) return fail("COLNDE_FC=0 sends free convection to the tile16 engine, which has no model index here: free-convection ensembles refuse it");
        e = env_get(ENV_FC_CW);
        if (e && atoi(e) == 32) return fail("COLNDE_FC_CW=32 selects the 32-column kernels, which have no model index: free-convection ensembles refuse it");
        if (env_get(ENV_FC_BLOCK)) return fail("COLNDE_FC_BLOCK: free-convection ensembles hold one block of columns per model (the column-block loop has no model index)");
    }
    return 0;
}

// ---- the --conv network (train_free_convection_nde.jl:110-122): a handle of its own on the 16-column fc32 kernels -------------------------------------
// Decided from the configuration and the environment alone, before any device work
static int conv_refusals(const colnde_config* cfg, int c) {
    if (c < 2 || c > FC_CONV_MAX)
        return fail("conv_filter = %d outside 2..%d (the reference builds the plain three-Dense chain for --conv <= 1: colnde_create; the taps are an unrolled loop of %d)", c,
                    FC_CONV_MAX, FC_CONV_MAX);
    if (cfg->model == COLNDE_MODEL_WIND_MIXING)
        return fail("colnde_create_conv covers the free-convection models (FreeConvectionNDE, ConvectiveAdjustmentNDE): the wind-mixing driver has no --conv network");
    {
        DevModel dm;
        PackInfo pk;
        build_model(cfg, &dm, &pk);
        if (!fc_supported(dm, COLNDE_STEPPER_RK4))
            return fail("colnde_create_conv takes the plain fc32 configuration, layer_sizes = (Nz, 4Nz, 4Nz, Nz-1) with relu, relu, identity and Nz = 32 or 64 (Nz = %d, %d "
                        "layers here): conv_filter says that the first Dense takes Nz - c + 1 inputs behind the filter", cfg->Nz, cfg->n_layers);
    }
    if (cfg->engine != COLNDE_ENGINE_AUTO && cfg->engine != COLNDE_ENGINE_FC32)
        return fail("the conv network runs the fc32 kernels (engine AUTO or FC32): engine forced to %d has no filter", cfg->engine);
    if (cfg->model == COLNDE_MODEL_FREE_CONVECTION && cfg->stepper == COLNDE_STEPPER_RKC2)
        return fail("FreeConvectionNDE under RKC2: fc32 has no such kernel (RKC2 covers ConvectiveAdjustmentNDE; FreeConvectionNDE runs RK4)");
    if (cfg->substeps == 0)
        return fail("substeps = 0 (chosen from reltol by the first solve) is not supported on a conv handle: the error estimate does not cover the filter — choose the count "
                    "and pass it");
    if (refuse_unstable_substeps(cfg)) return 1;
    if (cfg->n_columns > 4096)
        return fail("%d columns: the conv network covers the 16-column tiles (at most 4,096 columns, fc_tile_width); the 32-column kernels have no filter", cfg->n_columns);
    {
        const char* e = env_get(ENV_FC);
        if (e && *e && atoi(e) == 0) return fail("COLNDE_FC=0 sends free convection to the tile16 engine, which has no filter: conv handles refuse it");
        e = env_get(ENV_FC_CW);
        if (e && atoi(e) == 32) return fail("COLNDE_FC_CW=32 selects the 32-column kernels, which have no filter: conv handles refuse it");
        if (env_get(ENV_FC_BLOCK)) return fail("COLNDE_FC_BLOCK: conv handles hold one block of columns (at most 4,096)");
    }
    return 0;
}

// Puts the c-tap filter in front of a plain fc32 handle: the user's layout, and the padded weight vector and gradient row of each of K models
static hipError_t conv_attach(colnde_handle* h, int conv_filter, size_t K) {
    const DevModel& m = h->m;
    const int H = 4 * m.Nz, M = m.Nz - conv_filter + 1;
    h->conv.w1_end = m.w_off[0] + H * M;
    h->conv.n_zero = H * (conv_filter - 1);
    h->conv.n_params = conv_filter + 1 + m.n_params - h->conv.n_zero;
    hipError_t e = m.w_off[0] == 0 ? h->mem.alloc(&h->conv.d_wpad, K * (size_t)m.n_params) : hipErrorInvalidValue;
    if (e == hipSuccess) e = h->mem.alloc(&h->conv.d_gpad, K * ((size_t)m.n_params + 8));
    if (e == hipSuccess) h->conv.c = conv_filter;
    return e;
}

extern "C" int colnde_create_conv(const colnde_config* cfg, int conv_filter, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (validate(cfg)) return 1;
    if (conv_refusals(cfg, conv_filter)) return 1;
    colnde_handle* h = nullptr;
    if (colnde_create(cfg, &h)) return 1;
    if (!h->use_fc || h->fc_cw != 16) {
        colnde_destroy(h);
        return fail("colnde_create_conv: the configuration did not select the 16-column fc32 kernels");
    }
    const hipError_t e = conv_attach(h, conv_filter, 1);
    if (e != hipSuccess) {
        colnde_destroy(h);
        return fail("colnde_create_conv: allocating the padded weight and gradient vectors failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return 0;
}

// conv_filter = 0: K plain networks (colnde_create_fc_ensemble); c = 2..8: K --conv networks of that filter length (colnde_create_conv_ensemble), whose
// refusals are the union of the two creators', each in its own words
static int create_fc_ensemble(const colnde_config* cfg, int conv_filter, int n_models, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (validate(cfg)) return 1;
    if (conv_filter && conv_refusals(cfg, conv_filter)) return 1;
    if (fc_ens_refusals(cfg, n_models)) return 1;
    colnde_handle* h = nullptr;
    if (colnde_create(cfg, &h)) return 1;
    if (!h->use_fc || h->fc_cw != 16 || !fc_split_supported(16)) {
        colnde_destroy(h);
        return fail("this configuration does not run the 16-column fc32 kernels: free-convection ensembles refuse it");
    }
    h->ensemble = true;
    h->n_models = n_models;
    if (conv_filter) {
        const hipError_t ec = conv_attach(h, conv_filter, (size_t)n_models);
        if (ec != hipSuccess) {
            colnde_destroy(h);
            return fail("colnde_create_conv_ensemble: allocating the padded weight and gradient vectors of %d models failed: %s", n_models, hipGetErrorString(ec));
        }
    }
    // P: the floats of a model's vector as the caller passes it (d_w, d_out); the kernels pack the plain network's (en.w), padded behind a filter
    const size_t K = (size_t)n_models, P = (size_t)user_params(h);
    const int Nz = h->m.Nz;
    FcEns& en = h->fens;
    en.n_models = n_models;
    en.w = (size_t)h->m.n_params;
    en.img = fc_image_floats(Nz);
    en.simg = fc_split_image_words(Nz);
    en.bias = (fc_bias_floats(Nz) + 3) / 4 * 4;
    en.sol = (size_t)h->n_col * h->cfg.n_save * h->m.ns;
    h->ens.sol = en.sol;
    h->ens.n_models = n_models;
    DevPool& mem = h->mem;
    if (mem.resize(&h->d_w, K * P) || mem.resize(&h->d_out, K * (P + 8)) || mem.resize(&h->d_partial, K * 256 * 8) || mem.resize(&h->d_sol, K * en.sol) ||
        mem.resize(&h->d_fc_imgf, K * en.img) || mem.resize(&h->d_fc_imgb, K * en.img) || mem.resize(&h->d_fc_bias, K * en.bias) ||
        mem.resize(&h->d_fc_simgf, K * en.simg) || mem.resize(&h->d_fc_simgb, K * en.simg)) {
        colnde_destroy(h);
        return fail("allocating the free-convection ensemble's per-model buffers (%d models) failed", n_models);
    }
    if (fc_plan_tapes(h)) { colnde_destroy(h); return 1; }
    h->ens_model_bytes += (2 * en.img + en.bias + en.sol) * sizeof(float) + 2 * en.simg * sizeof(unsigned int);
    *out = h;
    return 0;
}

extern "C" int colnde_create_fc_ensemble(const colnde_config* cfg, int n_models, colnde_handle** out) { return create_fc_ensemble(cfg, 0, n_models, out); }

// ---- conv ensembles (colnde_create_conv_ensemble): K --conv networks of one filter length side by side ------------------------------------------------
// The product of the two handles above: the 16-column kernels' third entry points (fc_forward_conv_ens_kernel, fc_adjoint_conv_ens_kernel) carry the model
// index AND the filter; the pad, filter-gradient and fold kernels take K models in grid.y.  Row k of every result is, bit for bit, what a
// colnde_create_conv handle computes for model k's weights: the same records, slices, slab rows and orders of summation, at a stride.
extern "C" int colnde_create_conv_ensemble(const colnde_config* cfg, int conv_filter, int n_models, colnde_handle** out) {
    if (out) *out = nullptr;
    if (conv_filter == 0) return fail("conv_filter = 0 outside 2..%d: K plain networks are colnde_create_fc_ensemble's", FC_CONV_MAX);
    return create_fc_ensemble(cfg, conv_filter, n_models, out);
}

static int ensemble_only(const colnde_handle* h) {
    if (!h) return fail("null handle");
    if (h->closure) return fail("colnde_ensemble_* take weight vectors, but this is a closure handle (no networks): use colnde_closure_* (include/colnde.h)");
    if (h->conv.c && !h->ensemble) return fail("colnde_ensemble_* do not cover the convolutional first layer of a colnde_create_conv handle (conv=%d): ensembles of conv networks are out of scope", h->conv.c);
    if (!h->ensemble) return fail("not an ensemble handle: colnde_ensemble_* take the handles of colnde_create_ensemble (colnde_create: the single-model calls)");
    return 0;
}

static int fc_ensemble_only(const colnde_handle* h, const char* fn) {
    if (ensemble_only(h)) return 1;
    if (!h->use_fc) return fail("%s takes the handles of colnde_create_fc_ensemble: this ensemble holds wind-mixing models", fn);
    return 0;
}

extern "C" int colnde_ensemble_column_loss_dev(colnde_handle* h, const float* d_sol, float* d_out) {
    if (fc_ensemble_only(h, __func__)) return 1;
    if (!d_sol || !d_out) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_REDUCE);
    hipError_t e = launch_column_loss(d_sol, h->d_truth, h->m.Nz, (long)h->n_col * h->cfg.n_save, h->n_models, d_out, h->stream);
    if (e != hipSuccess) return fail("column loss launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_ensemble_causal_penalty_dev(colnde_handle* h, const float* d_weights, const float* d_coeff, float* d_result) {
    if (fc_ensemble_only(h, __func__)) return 1;
    if (!d_weights || !d_coeff || !d_result) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_REDUCE);
    // the first Dense weight as the caller's vector holds it: 4Nz x Nz at its offset, or — behind a filter — 4Nz x (Nz - c + 1) at c + 1
    const int c = h->conv.c;
    hipError_t e = launch_causal_penalty(d_weights, d_coeff, d_result, 4 * h->m.Nz, c ? h->m.Nz - c + 1 : h->m.Nz, c ? c + 1 : h->m.w_off[0], user_params(h), h->n_models,
                                         h->stream);
    if (e != hipSuccess) return fail("causal penalty launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_ensemble_set_physics(colnde_handle* h, const float* physics) {
    if (ensemble_only(h)) return 1;
    if (h->use_fc)
        return fail("colnde_ensemble_set_physics: a free-convection ensemble has no closure constants to vary (its models differ in their weights and ADAM rates only)");
    if (!physics) return fail("null physics array");
    if (!h->cfg.modified_pacanowski_philander)
        return fail("a physics array needs modified_pacanowski_philander = 1: without the Richardson-number closure the five constants are unused");
    HIPCHK(hipSetDevice(h->device));
    int min_sub = 1, stages = 0;
    if (ens_stability(&h->cfg, h->n_models, physics, &min_sub, &stages)) return 1;
    // the tapes hold the stage count planned at creation
    if (stages > h->m.nst)
        return fail("the new constants need %d RKC2 stages per step, the ensemble's tapes were planned for %d: create a new ensemble", stages, h->m.nst);
    if (ens_upload_physics(h, physics)) return 1;
    h->min_substeps = min_sub;
    return 0;
}

// forward solve of all K models (with_tape: into the ensemble's tapes)
static int ens_forward(colnde_handle* h, const float* d_weights, float* d_sol, bool with_tape) {
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    if (check_stability(h)) return 1;
    if (h->use_fc) return fc_pack(h, d_weights) ? 1 : fc_forward_range(h, d_sol, false, 0, h->n_col);
    if (h->tile_ens) return tile_ens_forward(h, d_weights, d_sol, with_tape);
    RtEns ens = h->ens;
    ens.sol = (size_t)h->n_col * h->cfg.n_save * h->m.ns;
    Timed tm(h, K_FORWARD);
    hipError_t e = rt_launch_pack(h->m, d_weights, h->d_wimg, h->stream, h->n_models);
    if (e == hipSuccess)
        e = rt_launch_forward_split(h->m, h->d_wimg, h->d_x0, h->d_bcs, h->d_times, h->cfg.n_save, h->cfg.substeps, d_sol,
                                    with_tape ? h->d_tape : nullptr, with_tape ? h->d_t16_ztape : nullptr, h->n_col, with_tape && h->split_rich,
                                    true, h->sp_fwd, h->stream, ens, sched_dev(h), total_steps(h));
    if (e != hipSuccess) return fail("ensemble forward launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_ensemble_forward_dev(colnde_handle* h, const float* d_weights, float* d_sol) {
    if (ensemble_only(h)) return 1;
    if (!d_weights || !d_sol) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    return ens_forward(h, d_weights, d_sol, false);
}

// ---- the member loss (colnde_ensemble_set_member_loss; member_loss.h) -------------------------------------------------------------------
// Member k's loss is  Σ_q s[k][q] · Σ_c w[k][c] · (term q of column c) / Σ_c w[k][c] : its own six scalings — determine_loss_scalings per run
// (wind_mixing/src/NDE_training.jl:256-288, calculate_loss_scalings: loss.jl:11-31) — and its own column weights, a 0/1 mask being the run's training
// simulations (train_free_convection_nde.jl:60-66).  Validation and the K LossWeights rows are member_loss.h's, pure host arithmetic; the rows and the
// K x n_col weights (ones where none were given) live in two buffers of the handle's pool, uploaded in stream order and complete on return, as
// colnde_set_schedule uploads its counts.  The shared-scalings entry points never read them.
extern "C" int colnde_ensemble_set_member_loss(colnde_handle* h, const float* scalings, const float* column_weights) {
    NOT_A_TILE_ENSEMBLE(h);               // (tile16's adjoint has no column-weight path)
    if (ensemble_only(h)) return 1;
    if (!scalings && !column_weights) {           // clears it (the buffers stay with the handle)
        h->ml_scalings = h->ml_columns = false;
        return 0;
    }
    const int K = h->n_models, nc = h->n_col;
    int bk = 0, bi = 0;
    switch (member_loss_validate(scalings, column_weights, K, nc, (long long)h->n_col_total, &bk, &bi)) {
        case MEMBER_LOSS_OK: break;
        case MEMBER_LOSS_GLOBAL_COLUMNS:
            return fail("a member loss normalises by the sum of a member's column weights over THIS handle's %d columns, but the handle is a shard of %lld "
                        "(colnde_set_global_columns): the normaliser would be a global sum", nc, (long long)h->n_col_total);
        case MEMBER_LOSS_BAD_SCALING:
            return fail("scalings[%d][%d] = %g: a loss scaling must be finite and >= 0", bk, bi, (double)scalings[(size_t)bk * 6 + bi]);
        case MEMBER_LOSS_BAD_WEIGHT:
            return fail("column_weights[%d][%d] = %g: a column weight must be finite and >= 0", bk, bi, (double)column_weights[(size_t)bk * nc + bi]);
        case MEMBER_LOSS_EMPTY_MEMBER:
            return fail("member %d's column weights sum to 0: it would train on no column (every member needs at least one column of positive weight)", bk);
    }
    HIPCHK(hipSetDevice(h->device));
    std::vector<LossWeights> lw((size_t)K);
    std::vector<float> cw((size_t)K * nc, 1.0f);
    const float ones[6] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
    const bool wm = h->m.model == COLNDE_MODEL_WIND_MIXING;
    for (int k = 0; k < K; k++) {
        const float* w = column_weights ? column_weights + (size_t)k * nc : nullptr;
        member_loss_weights(scalings ? scalings + (size_t)k * 6 : ones, member_weight_sum(w, nc), h->cfg.n_save, h->m.Nz, wm, lw[k].w);
        if (w) std::copy(w, w + nc, cw.begin() + (size_t)k * nc);
    }
    const size_t mark = h->mem.mark();
    if ((!h->d_ml_lw && h->mem.alloc(&h->d_ml_lw, (size_t)K) != hipSuccess) || (!h->d_ml_cw && h->mem.alloc(&h->d_ml_cw, (size_t)K * nc) != hipSuccess)) {
        h->mem.rollback(mark);
        h->ml_scalings = h->ml_columns = false;
        return fail("allocating the member loss (%d models x %d columns) failed", K, nc);
    }
    // in stream order on the handle's stream and complete on return: the caller's arrays are not kept, and a gradient queued earlier has read the old ones
    if (hipMemcpyAsync(h->d_ml_lw, lw.data(), (size_t)K * sizeof(LossWeights), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(h->d_ml_cw, cw.data(), (size_t)K * nc * sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
        (void)hipGetLastError();
        h->ml_scalings = h->ml_columns = false;
        return fail("uploading the member loss failed");
    }
    h->ml_scalings = scalings != nullptr;
    h->ml_columns = column_weights != nullptr;
    return 0;
}

// the member entry points: refused, before any device work, when no member loss is set
static int member_loss_only(const colnde_handle* h, const char* fn) {
    if (ensemble_only(h)) return 1;
    if (!(h->ml_scalings || h->ml_columns) || !h->d_ml_lw || !h->d_ml_cw)
        return fail("%s: no member loss is set — colnde_ensemble_set_member_loss first (colnde_ensemble_loss* take one scalings[6] for all members)", fn);
    return 0;
}

// scalings != nullptr: the shared loss, one scalings[6] for all K; nullptr: the member loss that was set
static int ens_loss(colnde_handle* h, const float* d_weights, const float* scalings, float* d_out8) {
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    if (ens_forward(h, d_weights, h->d_sol, false)) return 1;
    const int nblk = 256;
    hipError_t e;
    if (scalings) {
        LossWeights lw;
        loss_weights(h, scalings, &lw);
        e = launch_loss(h->m, h->d_sol, h->d_truth, h->cfg.n_save, h->n_col, h->d_partial, nblk, h->stream, h->n_models, h->ens.sol);
        if (e == hipSuccess) e = launch_reduce(h->d_partial, nblk, 0, 8, lw, d_out8, h->stream, h->n_models, (size_t)nblk * 8, 8);
    } else {
        e = launch_loss_member(h->m, h->d_sol, h->d_truth, h->cfg.n_save, h->n_col, h->d_partial, nblk, h->stream, h->n_models, h->ens.sol, h->d_ml_cw);
        if (e == hipSuccess) e = launch_reduce_member(h->d_partial, nblk, 0, 8, h->d_ml_lw, d_out8, h->stream, h->n_models, (size_t)nblk * 8, 8);
    }
    if (e != hipSuccess) return fail("ensemble loss launch failed: %s", hipGetErrorString(e));
    return 0;
}

static int ens_loss_grad(colnde_handle* h, const float* d_weights, const float* scalings, float* d_out) {
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    if (h->use_fc) {                 // fc32: the single handle's gradient path with the models' strides (api_grad.hip)
        if (!h->have_problem) return fail("colnde_set_problem has not been called");
        return check_stability(h) ? 1 : fc_loss_grad(h, d_weights, scalings, d_out);
    }
    if (h->tile_ens) {               // tile16's own kernels with the models' strides (the member loss is refused before this point)
        if (!h->have_problem) return fail("colnde_set_problem has not been called");
        if (!scalings) return fail("a tile ensemble has no member loss");
        return check_stability(h) ? 1 : tile_ens_loss_grad(h, d_weights, scalings, d_out);
    }
    const int K = h->n_models, stride = h->m.n_params + 8;
    LossWeights lw = {};
    if (scalings) loss_weights(h, scalings, &lw);
    HIPCHK(hipMemsetAsync(h->d_slab, 0, (size_t)K * h->ens.slab * sizeof(float), h->stream));
    if (ens_forward(h, d_weights, h->d_sol, true)) return 1;
    hipError_t e;
    {
        Timed tm(h, K_ADJOINT);
        e = rt_launch_adjoint_split(h->m, h->d_wimg, h->d_times, h->cfg.n_save, h->cfg.substeps, h->d_sol, h->d_truth, h->d_tape, h->d_t16_ztape, lw,
                                    h->d_slab, h->n_col, h->d_dwtape, h->split_rich, true, h->sp_adj, h->stream, h->ens, sched_dev(h), total_steps(h),
                                    scalings ? nullptr : h->d_ml_lw, scalings ? nullptr : h->d_ml_cw);
        if (e != hipSuccess) return fail("ensemble adjoint launch failed: %s", hipGetErrorString(e));
    }
    {
        Timed tm(h, K_DW1);
        const size_t n_rec = sched_records((size_t)h->n_tiles, total_steps(h), h->m.nst);
        e = dw_launch(h, n_rec, h->d_slab + (size_t)h->n_tiles * stride, K, h->ens.dwtape, h->ens.slab);
        if (e != hipSuccess) return fail("ensemble dW GEMM launch failed: %s", hipGetErrorString(e));
    }
    {
        Timed tm(h, K_REDUCE);
        e = scalings ? launch_reduce(h->d_slab, h->blk.rows, h->m.n_params, stride, lw, d_out, h->stream, K, h->ens.slab, stride)
                     : launch_reduce_member(h->d_slab, h->blk.rows, h->m.n_params, stride, h->d_ml_lw, d_out, h->stream, K, h->ens.slab, stride);
        if (e != hipSuccess) return fail("ensemble reduce launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

static int ens_loss_grad_host(colnde_handle* h, const float* weights, const float* scalings, float* out) {
    HIPCHK(hipSetDevice(h->device));
    const size_t K = (size_t)h->n_models, P = (size_t)user_params(h);
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * K * P, hipMemcpyHostToDevice, h->stream));
    if (ens_loss_grad(h, h->d_w, scalings, h->d_out)) return 1;
    HIPCHK(hipMemcpyAsync(out, h->d_out, sizeof(float) * K * (P + 8), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int colnde_ensemble_loss_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out8) {
    if (ensemble_only(h)) return 1;
    if (!d_weights || !scalings || !d_out8) return fail("null pointer argument");
    return ens_loss(h, d_weights, scalings, d_out8);
}

extern "C" int colnde_ensemble_loss_grad_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out) {
    if (ensemble_only(h)) return 1;
    if (!d_weights || !scalings || !d_out) return fail("null pointer argument");
    return ens_loss_grad(h, d_weights, scalings, d_out);
}

extern "C" int colnde_ensemble_loss_grad(colnde_handle* h, const float* weights, const float scalings[6], float* out) {
    if (ensemble_only(h)) return 1;
    if (!weights || !scalings || !out) return fail("null pointer argument");
    return ens_loss_grad_host(h, weights, scalings, out);
}

extern "C" int colnde_ensemble_member_loss_dev(colnde_handle* h, const float* d_weights, float* d_out8) {
    NOT_A_TILE_ENSEMBLE(h);
    if (member_loss_only(h, __func__)) return 1;
    if (!d_weights || !d_out8) return fail("null pointer argument");
    return ens_loss(h, d_weights, nullptr, d_out8);
}

extern "C" int colnde_ensemble_member_loss_grad_dev(colnde_handle* h, const float* d_weights, float* d_out) {
    NOT_A_TILE_ENSEMBLE(h);
    if (member_loss_only(h, __func__)) return 1;
    if (!d_weights || !d_out) return fail("null pointer argument");
    return ens_loss_grad(h, d_weights, nullptr, d_out);
}

extern "C" int colnde_ensemble_member_loss_grad(colnde_handle* h, const float* weights, float* out) {
    NOT_A_TILE_ENSEMBLE(h);
    if (member_loss_only(h, __func__)) return 1;
    if (!weights || !out) return fail("null pointer argument");
    return ens_loss_grad_host(h, weights, nullptr, out);
}

extern "C" int colnde_ensemble_adam_step_dev(colnde_handle* h, float* d_weights, const float* d_result, float* d_m, float* d_v, const float* d_eta,
                                             float beta1, float beta2, float eps, float beta1_t, float beta2_t) {
    if (ensemble_only(h)) return 1;
    if (!d_weights || !d_result || !d_m || !d_v || !d_eta) return fail("null pointer argument");
    if (!(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f)) return fail("0 <= beta < 1 required");
    if (!(beta1_t < 1.0f && beta2_t < 1.0f)) return fail("running powers beta^t must be < 1");
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_ADAM);
    const int np = user_params(h);
    hipError_t e = launch_adam_ensemble(d_weights, d_result, np + 8, d_m, d_v, d_eta, beta1, beta2, eps, beta1_t, beta2_t, np, h->n_models, h->stream);
    if (e != hipSuccess) return fail("ensemble ADAM launch failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- T -> wT pre-training of all K networks in one launch (engine_fc_pretrain.hip; train_free_convection_nde.jl:182-216) -----------------------------
// Semantics of colnde_pretrain_flux_dev, per model: the K sums of the per-sample losses come back in one copy and the means are formed here with the
// single call's expression.
extern "C" int colnde_ensemble_pretrain_flux_dev(colnde_handle* h, float* d_theta, float* d_m, float* d_v, const float* d_T, const float* d_bcs,
                                                 const float* d_flux, const int32_t* d_order, int n_samples, const float* d_coeff, int optimiser,
                                                 const float* d_eta, float beta1, float beta2, float eps, double beta_t[2], int update, float* mean_loss) {
    if (!h) return fail("%s: null handle", __func__);
    if (h->closure) return fail("%s takes the weight vectors of a free-convection ensemble, but this is a closure handle (no networks)", __func__);
    if (!h->ensemble)
        return fail("%s takes the handles of colnde_create_fc_ensemble / colnde_create_conv_ensemble (K = 1 for one network): this is a single-model handle "
                    "(colnde_pretrain_flux_dev pre-trains a plain single model)", __func__);
    if (!h->use_fc) return fail("%s covers the free-convection ensembles: this ensemble holds wind-mixing models (no T -> wT pre-training)", __func__);
    if (!d_theta || !d_T || !d_bcs || !d_flux || !beta_t || !mean_loss) return fail("%s: null pointer argument", __func__);
    if (optimiser != FCP_ADAM && optimiser != FCP_DESCENT) return fail("%s: optimiser = %d outside {0 = ADAM, 1 = Descent}", __func__, optimiser);
    if (n_samples < 1) return fail("%s: n_samples must be >= 1", __func__);
    const bool adam = optimiser == FCP_ADAM;
    if (update && !d_eta) return fail("%s: the rates d_eta [K] are needed when update != 0", __func__);
    if (update && adam && (!d_m || !d_v)) return fail("%s: the ADAM moments are needed when update != 0 under optimiser 0", __func__);
    if (adam && !(beta_t[0] < 1.0 && beta_t[1] < 1.0)) return fail("%s: running powers beta^t must be < 1", __func__);
    const int K = h->n_models;
    const DevModel dense = fc_pretrain_dense_model(h->m, h->conv.c);
    if (dense.n_params != user_params(h)) return fail("%s: parameter layout mismatch (%d vs %d)", __func__, dense.n_params, user_params(h));
    if (fc_pretrain_lds_bytes(dense, h->conv.c) > PRETRAIN_LDS_CAP)
        return fail("%s: network too large, a workgroup needs %zu B of LDS (> %zu)", __func__, fc_pretrain_lds_bytes(dense, h->conv.c), PRETRAIN_LDS_CAP);
    HIPCHK(hipSetDevice(h->device));
    DevScratch sc(h->stream);
    const size_t loss_bytes = ((size_t)K * sizeof(float) + 15) / 16 * 16;
    HIPCHK(sc.alloc(loss_bytes + 2 * sizeof(double)));
    float* d_loss = sc.p;
    double* d_bt = reinterpret_cast<double*>(reinterpret_cast<char*>(d_loss) + loss_bytes);
    hipError_t e = launch_fc_pretrain_ens(dense, h->conv.c, K, d_theta, adam ? d_m : nullptr, adam ? d_v : nullptr, d_T, d_bcs, d_flux, d_order, n_samples, d_coeff,
                                          optimiser, d_eta, beta1, beta2, eps, beta_t[0], beta_t[1], update, d_loss, d_bt, h->stream);
    std::vector<float> loss((size_t)K, 0.0f);
    double bt[2] = {beta_t[0], beta_t[1]};
    if (e == hipSuccess) e = hipMemcpyAsync(loss.data(), d_loss, (size_t)K * sizeof(float), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(bt, d_bt, sizeof(bt), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail("%s failed: %s", __func__, hipGetErrorString(e));
    for (int k = 0; k < K; k++) mean_loss[k] = loss[k] / (float)n_samples;
    if (update && adam) { beta_t[0] = bt[0]; beta_t[1] = bt[1]; }
    return 0;
}

// ---- train_NN for the K x 3 flux networks of a wind-mixing ensemble in one launch (engine_wm_pretrain.hip; wind_mixing/src/NN_training.jl:207-249) ----
// Semantics of colnde_pretrain_flux_dev per (model, net), with model k's closure constants (h->d_phys): the K x 3 sums of the per-sample losses come
// back in one copy and the means are formed here with the single call's expression.
extern "C" int colnde_ensemble_pretrain_wm_flux_dev(colnde_handle* h, int nets, float* d_theta, float* d_m, float* d_v, const float* d_profiles,
                                                    const float* d_bcs, const float* d_flux, const int32_t* d_order, int n_samples, float gradient_scaling,
                                                    const float* d_eta, float beta1, float beta2, float eps, double beta_t[2], int update, float* mean_loss) {
    if (!h) return fail("%s: null handle", __func__);
    NOT_A_TILE_ENSEMBLE(h);
    if (h->closure) return fail("%s takes the weight vectors of a wind-mixing ensemble, but this is a closure handle (no networks)", __func__);
    if (!h->ensemble)
        return fail("%s takes the handles of colnde_create_ensemble (K = 1 for one model): this is a single-model handle "
                    "(colnde_pretrain_flux_dev pre-trains one net of a single model)", __func__);
    if (h->use_fc)
        return fail("%s covers the wind-mixing ensembles: this ensemble holds free-convection networks (colnde_ensemble_pretrain_flux_dev pre-trains "
                    "those on T -> wT)", __func__);
    if (!d_theta || !d_profiles || !d_bcs || !d_flux || !beta_t || !mean_loss) return fail("%s: null pointer argument", __func__);
    if (nets < 1 || nets > 7) return fail("%s: nets = %d outside 1..7 (bit 0 = uw, bit 1 = vw, bit 2 = wT)", __func__, nets);
    if (update && !d_eta) return fail("%s: the rates d_eta [K][3] are needed when update != 0", __func__);
    if (update && (!d_m || !d_v)) return fail("%s: the ADAM moments are needed when update != 0", __func__);
    if (!(beta_t[0] < 1.0 && beta_t[1] < 1.0)) return fail("%s: running powers beta^t must be < 1", __func__);
    if (n_samples < 1) return fail("%s: n_samples must be >= 1", __func__);
    if (wm_pretrain_lds_bytes(h->m, update) > PRETRAIN_LDS_CAP)
        return fail("%s: network too large, a workgroup needs %zu B of LDS (> %zu)", __func__, wm_pretrain_lds_bytes(h->m, update), PRETRAIN_LDS_CAP);
    const int K = h->n_models, C = 3 * K;
    HIPCHK(hipSetDevice(h->device));
    DevScratch sc(h->stream);
    const size_t loss_bytes = ((size_t)C * sizeof(float) + 15) / 16 * 16;
    HIPCHK(sc.alloc(loss_bytes + 2 * sizeof(double)));
    float* d_loss = sc.p;
    double* d_bt = reinterpret_cast<double*>(reinterpret_cast<char*>(d_loss) + loss_bytes);
    hipError_t e = launch_wm_pretrain_ens(h->m, K, nets, h->d_phys, d_theta, update ? d_m : nullptr, update ? d_v : nullptr, d_profiles, d_bcs, d_flux, d_order,
                                          n_samples, gradient_scaling, d_eta, beta1, beta2, eps, beta_t[0], beta_t[1], update, d_loss, d_bt, h->stream);
    std::vector<float> loss((size_t)C, 0.0f);
    double bt[2] = {beta_t[0], beta_t[1]};
    if (e == hipSuccess) e = hipMemcpyAsync(loss.data(), d_loss, (size_t)C * sizeof(float), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && update) e = hipMemcpyAsync(bt, d_bt, sizeof(bt), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail("%s failed: %s", __func__, hipGetErrorString(e));
    for (int c = 0; c < C; c++) mean_loss[c] = ((nets >> (c % 3)) & 1) ? loss[c] / (float)n_samples : 0.0f;
    if (update) { beta_t[0] = bt[0]; beta_t[1] = bt[1]; }
    return 0;
}
