// api_grad.hip — loss and gradient of a single handle: the tape planners of the three engines (fc32's serves its ensembles too) and colnde_loss_grad[_dev].
#include "api_internal.h"
#include "tape_plan.h"
#include "dw_plan.h"

// Sizes the regtile engine's tapes.  They hold ONE block of columns; a problem whose tapes exceed the free HBM (many columns, or a
// long horizon: 1,153 frames need 4x the bytes per column of the 2-day suite) runs its gradient path block after block into the same
// buffers.  COLNDE_RT_BLOCK=<columns> forces a block size (testing aid).  The decision is tape_plan.h's plan_rt_tapes.
static int rt_plan_tapes(colnde_handle* h) {
    if (h->d_rt_tape) return 0;
    const int n_steps = (h->cfg.n_save - 1) * h->cfg.substeps;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t per_col_x = (size_t)n_steps * 4 * 96 * sizeof(float), per_col_2 = (size_t)n_steps * 4 * ((21 * 256) / 32) * sizeof(float);
    const size_t per_col_z = rt_tapez_floats(32, n_steps) / 32 * sizeof(float);      // (twice per_col_2 in the A/B build that tapes activation pairs)
    const int n32 = ((h->n_col + 31) / 32) * 32;
    const RtTapes plan = plan_rt_tapes(n32, per_col_x, per_col_2, per_col_z, hbm_budget(free_b, (size_t)2 << 30), !h->rt_fwd32 && env_flag(ENV_RT_ZTAPE) != FLAG_OFF,
                                       env_int(ENV_RT_BLOCK, 0));
    const int block = plan.block;
    if (block == 0) return fail("the stage tapes of even 1,024 columns (%zu bytes per column) do not fit in %zu free bytes of HBM",
                                per_col_x + per_col_2, free_b);
    const size_t n1 = rt_tape_floats(block, n_steps), n2 = rt_tape2_floats(block, n_steps);
    const size_t mark = h->mem.mark();
    hipError_t e = h->mem.alloc(&h->d_rt_tape, n1);
    if (e == hipSuccess) e = h->mem.alloc(&h->d_rt_tape2, n2);
    h->rt_ztape = plan.ztape;                    // the Z1 tape is optional: dropped when its allocation fails
    if (e == hipSuccess && plan.ztape && h->mem.alloc(&h->d_rt_tapez, rt_tapez_floats(block, n_steps)) != hipSuccess) h->rt_ztape = false;
    if (e != hipSuccess) {
        h->mem.rollback(mark);                   // leave no half-built state behind
        return fail("hipMalloc of the %zu-byte stage tapes failed: %s", (n1 + n2) * sizeof(float), hipGetErrorString(e));
    }
    h->blk.block = block;
    h->blk.nblocks = (n32 + block - 1) / block;
    return 0;
}

// The dW GEMM's plan for tapes of n_rec records: the block lists and passes of the network, the slice count of this size and arithmetic (dw_plan.h)
void build_dw_plan(colnde_handle* h, size_t n_rec) {
    dw_plan_blocks(h->m, h->dw);
    dw_plan_slices(h->dw, n_rec, dw_gemm_lds_fits((int)dwtape_row_floats(h->m), h->dw.n_macros), h->sp_dw);
    h->dw_n_rec = n_rec;
    dw_slab_rows(h);
}

// The slab rows that follow the plan's slice count: the adjoint's rows (one per tile, fc32: per tile and time segment), then the dW GEMM's (one per
// block, fc32: and segment, and slice); an ensemble's models lie that many rows apart.  The planners size d_slab by it and the setter below re-sizes it.
void dw_slab_rows(colnde_handle* h) {
    const int tiles = h->use_fc ? (h->n_col + 31) / 32 * 32 / h->fc_cw : h->n_tiles, nseg = h->use_fc ? h->fc_nseg : 1;
    h->blk.rows = (tiles + h->blk.nblocks * h->dw.slices) * nseg;
    h->fens.slab = h->ens.slab = (size_t)h->blk.rows * ((size_t)h->m.n_params + 8);      // (unused by a single handle: one model, no strides)
}

// colnde_set_matrix_arithmetic on a handle whose tapes are planned: the slice count was chosen for the arithmetic at plan time (dw_plan.h:
// dw_slice_count), and the kernel the new arithmetic runs may not take it (the L2-streaming f32 kernel: multiples of 8).  Leaves the handle with the
// count, slab rows and slab a fresh handle of the arithmetic now in h->sp_dw plans; a failure leaves the plan as it was.
int replan_dw_slices(colnde_handle* h) {
    if (!h->d_dwtape || !h->d_slab) return 0;
    const int slices = dw_slice_count(h->dw, h->dw_n_rec, h->dw.lds_fit, h->sp_dw), old = h->dw.slices;
    if (slices == old) return 0;
    const size_t P8 = (size_t)h->m.n_params + 8, K = (size_t)h->n_models;
    const size_t old_model = (size_t)h->blk.rows * P8;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));             // (launches in flight write the slab about to be freed)
    h->dw.slices = slices;
    dw_slab_rows(h);
    const size_t new_model = (size_t)h->blk.rows * P8;
    const hipError_t e = h->mem.replace(&h->d_slab, K * new_model);      // the new slab first: a failure keeps the old one
    if (e != hipSuccess) {
        h->dw.slices = old;
        dw_slab_rows(h);
        return fail("re-planning the dW GEMM for the new arithmetic: hipMalloc of the %zu-byte slab of %d slices failed (%s); the arithmetic and the plan "
                    "of %d slices stay in force", K * new_model * sizeof(float), slices, hipGetErrorString(e), old);
    }
    if (h->ensemble) h->ens_model_bytes = h->ens_model_bytes - old_model * sizeof(float) + new_model * sizeof(float);
    return 0;
}

hipError_t upload_dw_plan(colnde_handle* h) {
    const DwPlan& p = h->dw;
    hipError_t e = h->mem.alloc(&h->d_macros, p.macros.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_macros, p.macros.data(), p.macros.size() * sizeof(DwMacro), hipMemcpyHostToDevice);
    if (e == hipSuccess && p.split_ok) e = h->mem.alloc(&h->d_split_macros, p.split_macros.size());
    if (e == hipSuccess && p.split_ok) e = hipMemcpy(h->d_split_macros, p.split_macros.data(), p.split_macros.size() * sizeof(DwMacro), hipMemcpyHostToDevice);
    return e;
}

// The bf16-split kernel when the handle's weight-gradient arithmetic asks for it and the plan has passes, else the f32 kernels.
// (The slice count follows the arithmetic: replan_dw_slices.)
hipError_t dw_launch(colnde_handle* h, size_t n_records, float* slab_rows, int K, size_t tape_mstride, size_t slab_mstride) {
    const int R = (int)dwtape_row_floats(h->m), stride = h->m.n_params + 8;
    if (h->sp_dw && !h->dw.passes.empty())
        return launch_dw_gemm_split(h->d_dwtape, n_records, R, h->dw, h->d_split_macros, h->dw.slices, slab_rows, stride, h->stream, K, tape_mstride, slab_mstride);
    return launch_dw_gemm(h->d_dwtape, n_records, R, h->d_macros, h->dw.n_macros, h->dw.slices, slab_rows, stride, h->stream, K, tape_mstride, slab_mstride);
}

// fc32 gradient path: the records (forward: xs, a1, a2; adjoint: dz1, dz2, dz3) and the bit tapes.  When they do not fit in the free HBM for the
// whole problem there are two ways to cut it:
//   * column blocks (a multiple of the 32-column tile): forward -> adjoint -> dW GEMM block after block.  No extra work, but a block of fewer than
//     16,384 columns leaves CUs with one workgroup or none (the kernels get their speed from two per CU);
//   * time segments: ALL columns, the tapes hold `fc_seg` save intervals.  One tape-less forward pass first (it saves the state at every save
//     point, and tapes the last segment on its way), then, from the last segment to the first, a taped forward restarted from the saved state,
//     the adjoint over the segment (λ handed on through d_fc_lam) and the dW GEMM.  Costs (n_seg - 1)/n_seg of an extra forward solve, keeps every
//     CU at two workgroups.
// Blocks are used when they hold at least 16,384 columns (or everything), segments otherwise; COLNDE_FC_BLOCK=<columns> / COLNDE_FC_SEG=<intervals> force.
// An ensemble (h->ensemble, K = h->n_models; planned once, at creation): one block of all columns per model on a budget of (free memory - margin) / K,
// the whole time axis when it fits and time segments otherwise, the slice count a single handle of this size plans; refused with the bytes it needs
// when not even one save interval per segment fits.  The decision is tape_plan.h's plan_fc_tapes; what follows it is the same for both: K models'
// worth of every buffer, the models the FcEns / ConvBlock strides apart (a single handle's kernels get no strides).
int fc_plan_tapes(colnde_handle* h) {
    if (h->d_dwtape) return 0;
    const DevModel& m = h->m;
    const size_t K = (size_t)h->n_models;
    const int n_iv = h->cfg.n_save - 1, cw = h->fc_cw;
    const size_t R = dwtape_row_floats(m);
    if (R != fc_record_row_floats(m.Nz)) return fail("fc32: record layout mismatch (%zu vs %zu floats per column)", R, fc_record_row_floats(m.Nz));
    const bool ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE;
    const int conv = h->conv.c;
    const size_t per_col_iv = fc_tape_bytes_per_col_iv(h->cfg.substeps, m.nst, R, fc_mask_words(), cw, ca, conv ? fc_conv_tape_floats(m.Nz) : 0);
    const int n32 = (h->n_col + 31) / 32 * 32;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const char* es = env_get(ENV_FC_SEG);
    const FcTapes plan = plan_fc_tapes({n32, n_iv, cw, m.Nz, m.n_params, per_col_iv, free_b, h->ensemble, h->n_models,
                                        conv ? (size_t)FC_CONV_GRAD_MAX_SLICES * FC_CONV_GRAD_SLOTS : 0, env_int(ENV_FC_BLOCK, 0),
                                        es ? (atoi(es) >= 1 ? atoi(es) : -1) : 0});
    const int block = plan.block, seg = plan.seg;
    if (plan.status == FC_PLAN_NOTHING_FITS)
        return fail("fc32: the tapes of even one 32-column tile and one save interval (%zu bytes) do not fit in the free device memory", 32 * per_col_iv);
    if (plan.status == FC_PLAN_ENSEMBLE_REFUSED)
        return fail("a free-convection ensemble of %d models needs %zu bytes of device memory for its tapes and slab rows (%zu per model with %d save interval(s) per "
                    "time segment, %d substeps x %d stages); %zu bytes are free (3 GB kept in reserve): use fewer models per handle",
                    h->n_models, K * plan.model_bytes, plan.model_bytes, seg, h->cfg.substeps, m.nst, free_b);
    h->blk.block = block;
    h->blk.nblocks = (n32 + block - 1) / block;
    h->fc_seg = seg;
    h->fc_nseg = (n_iv + seg - 1) / seg;
    const size_t tiles_b = (size_t)block / cw;                                  // (block is a multiple of 32)
    const size_t stage_recs = (size_t)seg * h->cfg.substeps * m.nst;          // (tile, stage) records per tile held by the tapes
    const size_t n_rec = tiles_b * (cw / 16) * stage_recs;                     // records are tile16's: 16 columns each
    build_dw_plan(h, n_rec);                                                    // (and h->blk.rows, fens.slab: dw_slab_rows)
    FcEns& en = h->fens;
    en.dwtape = n_rec * CT * R;
    en.masks = tiles_b * stage_recs * fc_mask_words();
    en.swtape = ca ? tiles_b * stage_recs * fc_switch_words(cw) : 0;
    en.lam = (size_t)n32 * m.Nz;
    const size_t mark = h->mem.mark();
    hipError_t e = h->mem.alloc(&h->d_dwtape, K * en.dwtape);
    if (e == hipSuccess) e = h->mem.alloc(&h->d_fc_masks, K * en.masks);
    if (e == hipSuccess && ca) e = h->mem.alloc(&h->d_fc_switch, K * en.swtape);
    if (e == hipSuccess && h->fc_nseg > 1) e = h->mem.alloc(&h->d_fc_lam, K * en.lam);
    if (e == hipSuccess && conv) {                           // per model: the conv tape of the same records, and one single handle's filter slab
        h->conv.cslab_rows = h->blk.nblocks * h->fc_nseg * FC_CONV_GRAD_MAX_SLICES;
        h->conv.ctape_stride = n_rec * fc_conv_tape_floats(m.Nz);
        h->conv.cslab_stride = (size_t)h->conv.cslab_rows * FC_CONV_GRAD_SLOTS;
        e = h->mem.alloc(&h->conv.d_ctape, K * h->conv.ctape_stride);
        if (e == hipSuccess) e = h->mem.alloc(&h->conv.d_cslab, K * h->conv.cslab_stride);
    }
    if (e == hipSuccess) e = upload_dw_plan(h);
    if (e == hipSuccess && !h->d_slab) e = h->mem.alloc(&h->d_slab, K * en.slab);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->mem.rollback(mark);
        if (h->ensemble)
            return fail("allocating the free-convection ensemble's tapes (%zu bytes, %zu per model) failed: %s", K * plan.model_bytes, plan.model_bytes, hipGetErrorString(e));
        return fail("fc32: hipMalloc of the tapes (%zu bytes for %d columns x %d save intervals) failed: %s", (size_t)block * per_col_iv * seg, block, seg,
                    hipGetErrorString(e));
    }
    h->ens_model_bytes = (en.dwtape + en.slab + (h->fc_nseg > 1 ? en.lam : 0)) * sizeof(float) + en.masks * sizeof(unsigned int) + en.swtape * sizeof(unsigned long long);
    if (conv) h->ens_model_bytes += (h->conv.ctape_stride + h->conv.cslab_stride + 2 * (size_t)m.n_params + 8) * sizeof(float);
    return 0;
}

// The buffers of tile16's taped mode, K models' worth (n_rec records per model), inside the caller's mark / rollback bracket: the delta tape, the dW
// plan and the slab, then (*at = 1) the stage tape ...
hipError_t t16_alloc_tapes(colnde_handle* h, size_t K, size_t n_rec, int* at) {
    const DevModel& m = h->m;
    *at = 0;
    hipError_t e = h->mem.alloc(&h->d_dwtape, K * n_rec * CT * dwtape_row_floats(m));
    if (e == hipSuccess) e = upload_dw_plan(h);
    if (e == hipSuccess && !h->d_slab) e = h->mem.alloc(&h->d_slab, K * (size_t)h->blk.rows * (m.n_params + 8));
    if (e != hipSuccess) return e;
    *at = 1;
    return h->d_tape ? hipSuccess : h->mem.alloc(&h->d_tape, K * n_rec * CT * m.ns);
}
// ... and the net-split pair's rich tape, or the hidden pre-activations the forward kernel tapes for the adjoint
hipError_t t16_alloc_ztape(colnde_handle* h, size_t K, size_t n_rec, bool rich) {
    return h->mem.alloc(&h->d_t16_ztape, K * n_rec * (rich ? rt_split_rich_record_floats() : CT * t16_ztape_col_floats(h->m)));
}

// tile16, taped weight gradients: decide once per handle (tape_plan.h: plan_t16_tapes).  On when the tapes fit in the free HBM (the in-register
// adjoint_kernel geometries remain the fallback; 64-256-256-63's 384 gradient tiles spill there) — with the hidden pre-activations taped too, the
// 1,024-thread accumulator-free adjoint beats the in-register kernels at every size measured (8 columns: 53 vs 64 ms per iteration; 32-128-128-31: 162
// vs 198 ms).  COLNDE_T16_DWTAPE=1 / 0 forces it on / off, COLNDE_T16_BLOCK=<columns> a block size, COLNDE_T16_ZTAPE=0 disables the pre-activation tape.
static int t16_plan_dwtape(colnde_handle* h) {
    if (h->t16_dwtape >= 0) return 0;
    const DevModel& m = h->m;
    const int n_steps = total_steps(h), n16 = h->n_tiles * CT, ztape = env_flag(ENV_T16_ZTAPE);
    const size_t R = dwtape_row_floats(m);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t margin = ((size_t)3 << 30) + (size_t)h->n_tiles * (m.n_params + 8) * sizeof(float);
    // (the rich tape is 4x the pre-activation tape per column — 13,824 floats per 16-column record against 216 per column: part of the fit estimate)
    const size_t per_col = (size_t)n_steps * m.nst * (R + t16_ztape_col_floats(m) + m.ns) * sizeof(float);
    const size_t per_col_rich = (size_t)n_steps * m.nst * (R + rt_split_rich_record_floats() / CT + m.ns) * sizeof(float);
    const size_t lds_ag = (MODEL_FLOATS + lds_floats_adjoint_ag(m)) * sizeof(float);
    const T16Tapes plan = plan_t16_tapes({n16, CT, m.ns, m.n_bias, h->ag_rows, h->adj_split, (MODEL_FLOATS + lds_floats_adjoint(m)) * sizeof(float),
                                          (MODEL_FLOATS + lds_floats_adjoint_noA(m)) * sizeof(float), lds_ag, per_col, per_col_rich, hbm_budget(free_b, margin),
                                          env_flag(ENV_T16_DWTAPE), ztape, env_flag(ENV_T16_SPLIT_RICH), env_int(ENV_T16_BLOCK, 0)});
    switch (plan.status) {
    case T16_PLAN_REFUSED_OFF:
        return fail("COLNDE_T16_DWTAPE=0: this network's activation rows live in global memory, and only the taped-dW adjoint runs that way");
    case T16_PLAN_REFUSED_TOO_LARGE:
        return fail("network too large for the taped adjoint with rows in global memory (%d biases, %zu B of LDS)", m.n_bias, lds_ag);
    case T16_PLAN_REFUSED_NO_FIT:
        return fail("the delta tape of this network (%zu B per column) does not fit in HBM beside the solve", per_col);
    case T16_PLAN_IN_REGISTER:
        h->t16_dwtape = 0;
        return 0;
    case T16_PLAN_TAPED:
        break;
    }
    const size_t n_rec = (size_t)(plan.block / CT) * n_steps * m.nst;
    h->blk.block = plan.block;
    h->blk.nblocks = (n16 + plan.block - 1) / plan.block;
    build_dw_plan(h, n_rec);                                                    // (and h->blk.rows: dw_slab_rows)
    const size_t mark = h->mem.mark();
    int at = 0;
    const hipError_t e = t16_alloc_tapes(h, 1, n_rec, &at);
    if (e != hipSuccess) {                  // no delta tape (or no stage tape for the block): the in-register path follows
        (void)hipGetLastError();
        h->mem.rollback(mark);
        h->t16_dwtape = 0;
        if (h->ag_rows && at == 0) return fail("allocating the delta tape (%zu B) failed: %s", n_rec * CT * R * sizeof(float), hipGetErrorString(e));
        if (h->ag_rows) return fail("allocating the stage tape failed: %s", hipGetErrorString(e));
        return 0;
    }
    h->t16_dwtape = 1;
    // net-split kernels on a small block (<= 2,048 columns, where it pays: 64-step iteration with the four-wave kernels 2.36 vs 2.48 ms at 1,024
    // columns, 2.69 vs 2.77 at 2,048, 3.99 vs 3.53 at 4,096): the rich tape in place of the pre-activations
    if (plan.rich && t16_alloc_ztape(h, 1, n_rec, true) == hipSuccess) {
        h->split_rich = true;
        return 0;
    }
    if (ztape != FLAG_OFF) (void)t16_alloc_ztape(h, 1, n_rec, false);      // (optional: null when it fails)
    if ((h->ag_rows || plan.need_z) && !h->d_t16_ztape)
        return fail("this network's taped adjoint needs the pre-activation tape (COLNDE_T16_ZTAPE=0 or its allocation failed): no gradient path for it without one");
    return 0;
}

// regtile: the tapes hold one block of columns; forward -> adjoint -> dW1 block after block
static int rt_loss_grad(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out) {
    const int stride = h->m.n_params + 8;
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    if (rt_plan_tapes(h)) return 1;
    const int n_steps = (h->cfg.n_save - 1) * h->cfg.substeps;
    const int n_wt = rt_n_wtiles(h->n_col), n_dw = rt_dw1_waves(h->blk.block, n_steps);
    if (!h->d_rt_slab) {
        h->blk.rows = n_wt + h->blk.nblocks * n_dw;
        hipError_t e = h->mem.alloc(&h->d_rt_slab, (size_t)h->blk.rows * stride);
        if (e != hipSuccess) return fail("hipMalloc of the partial-gradient slab failed: %s", hipGetErrorString(e));
    }
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    hipError_t e = rt_launch_pack(h->m, d_weights, h->d_wimg, h->stream);
    if (e != hipSuccess) return fail("rt pack launch failed: %s", hipGetErrorString(e));
    HIPCHK(hipMemsetAsync(h->d_rt_slab, 0, (size_t)h->blk.rows * stride * sizeof(float), h->stream));
    const size_t ns = h->m.ns;
    for (int b = 0; b < h->blk.nblocks; b++) {
        const int c0 = b * h->blk.block, nc = std::min(h->blk.block, h->n_col - c0);
        if (nc <= 0) break;
        if (rt_forward_range(h, h->d_sol, true, c0, nc)) return 1;
        {
            Timed tm(h, K_ADJOINT);
            e = rt_launch_adjoint(h->m, h->d_wimg, h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times, h->cfg.n_save, h->cfg.substeps,
                                  h->d_sol + (size_t)c0 * h->cfg.n_save * ns, h->d_truth + (size_t)c0 * h->cfg.n_save * ns, h->d_rt_tape,
                                  h->d_rt_tape2, h->rt_ztape ? h->d_rt_tapez : nullptr, lw,
                                  h->d_rt_slab + (size_t)(c0 / 32) * stride, nc, h->sp_adj, h->stream);
            if (e != hipSuccess) return fail("rt adjoint launch failed: %s", hipGetErrorString(e));
        }
        {
            Timed tm(h, K_DW1);
            e = rt_launch_dw1(h->m, h->d_rt_tape, h->d_rt_tape2, nc, n_steps, h->d_rt_slab + ((size_t)n_wt + (size_t)b * n_dw) * stride,
                              h->sp_dw, h->stream);
            if (e != hipSuccess) return fail("rt dW1 launch failed: %s", hipGetErrorString(e));
        }
    }
    {
        Timed tm(h, K_REDUCE);
        e = launch_reduce(h->d_rt_slab, h->blk.rows, h->m.n_params, stride, lw, d_out, h->stream);
        if (e != hipSuccess) return fail("reduce launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

// fc32, for a single handle and for a free-convection ensemble alike (FcEns strides; the ensemble is the case of one column block): forward ->
// adjoint -> dW GEMM block after block, within a block segment by segment from the end of the time axis, λ handed on per model
int fc_loss_grad(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out) {
    const int stride = h->m.n_params + 8;
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    if (fc_plan_tapes(h)) return 1;
    // scalings == nullptr: the member loss of an ensemble — every model its own loss weight and column weights, read on the device (FcEns::member_*)
    const bool member = !scalings;
    if (member && !(h->ensemble && h->d_ml_lw && h->d_ml_cw)) return fail("no member loss is set: colnde_ensemble_set_member_loss first");
    LossWeights lw = {};
    if (!member) loss_weights(h, scalings, &lw);
    const size_t ns = h->m.ns;
    // an ensemble hands the kernels the strides of what a model owns (a single handle: one model, no strides) and its own words in the launch errors
    const int K = h->n_models;
    FcEns enm = h->fens;
    if (member) {
        enm.member_w = &h->d_ml_lw[0].w[2];
        enm.member_colw = h->d_ml_cw;
    }
    const FcEns* en = h->ensemble ? &enm : nullptr;
    const char* ens = h->ensemble ? "ensemble " : "";
    if (fc_pack(h, d_weights)) return 1;
    const FcConv cv = fc_conv_args(h);                                  // (after the plan: the conv tape exists)
    const FcConvEns ce = fc_conv_ens_args(h);
    const size_t cslab_model = (size_t)h->conv.cslab_rows * FC_CONV_GRAD_SLOTS;      // the filter slab of one model
    hipError_t e;
    HIPCHK(hipMemsetAsync(h->d_slab, 0, (size_t)K * h->blk.rows * stride * sizeof(float), h->stream));
    if (h->conv.c) HIPCHK(hipMemsetAsync(h->conv.d_cslab, 0, (size_t)K * cslab_model * sizeof(float), h->stream));
    const int cw = h->fc_cw;
    const int n_wg = (h->n_col + cw - 1) / cw, n_iv = h->cfg.n_save - 1, nseg = h->fc_nseg;
    const size_t gemm_rows0 = (size_t)n_wg * nseg;                      // slab: [tile][segment] adjoint rows, then [block][segment][slice] GEMM rows
    for (int b = 0; b < h->blk.nblocks; b++) {
        const int c0 = b * h->blk.block, nc = std::min(h->blk.block, h->n_col - c0);
        if (nc <= 0) break;
        const size_t tiles_b = ((size_t)nc + cw - 1) / cw;
        // time segments: the states at the save points first (tape-less), then segment by segment from the end of the axis
        // (that first pass tapes the LAST segment on its way, which is the first one the backward sweep needs)
        if (nseg > 1 && fc_forward_range(h, h->d_sol, true, c0, nc, 0, n_iv, (nseg - 1) * h->fc_seg)) return 1;
        for (int sg = nseg - 1; sg >= 0; sg--) {
            const int iv0 = sg * h->fc_seg, iv1 = std::min(n_iv, iv0 + h->fc_seg);
            if (!(nseg > 1 && sg == nseg - 1) && fc_forward_range(h, h->d_sol, true, c0, nc, iv0, iv1)) return 1;
            {
                Timed tm(h, K_ADJOINT);
                e = fc_launch_adjoint(h->m, h->fc_cw, h->d_fc_imgb, (h->sp_adj && fc_split_supported(h->fc_cw)) ? h->d_fc_simgb : nullptr, h->d_times, h->cfg.n_save, iv0, iv1, h->cfg.substeps, h->d_sol + (size_t)c0 * h->cfg.n_save * ns,
                                      h->d_truth + (size_t)c0 * h->cfg.n_save * ns, h->d_dwtape, h->d_fc_masks, h->d_fc_switch, lw.w[2],
                                      nseg > 1 ? h->d_fc_lam + (size_t)c0 * h->m.Nz : nullptr,
                                      h->d_slab + ((size_t)sg * n_wg + (size_t)(c0 / cw)) * stride, nc, h->stream, en, h->conv.c ? &cv : nullptr, &ce);
                if (e != hipSuccess) return fail("fc32 %sadjoint launch failed: %s", ens, hipGetErrorString(e));
            }
            {
                Timed tm(h, K_DW1);
                e = dw_launch(h, tiles_b * (cw / 16) * (size_t)(iv1 - iv0) * h->cfg.substeps * h->m.nst,
                              h->d_slab + (gemm_rows0 + ((size_t)b * nseg + sg) * h->dw.slices) * stride, K, h->fens.dwtape, h->fens.slab);
                if (e != hipSuccess) return fail("%sdW GEMM launch failed: %s", ens, hipGetErrorString(e));
                if (h->conv.c) {                                        // the filter's c + 1 entries (every model's), from the conv tape of the same records
                    e = launch_fc_conv_grad(h->conv.d_ctape, (long)(tiles_b * (size_t)(iv1 - iv0) * h->cfg.substeps * h->m.nst) * 16, h->m.Nz, h->conv.c,
                                            h->conv.d_cslab + ((size_t)b * nseg + sg) * FC_CONV_GRAD_MAX_SLICES * FC_CONV_GRAD_SLOTS, h->stream, K, h->conv.ctape_stride,
                                            h->conv.cslab_stride);
                    if (e != hipSuccess) return fail("conv filter gradient launch failed: %s", hipGetErrorString(e));
                }
            }
        }
    }
    {
        Timed tm(h, K_REDUCE);
        if (member) e = launch_reduce_member(h->d_slab, h->blk.rows, h->m.n_params, stride, h->d_ml_lw, h->conv.c ? h->conv.d_gpad : d_out, h->stream, K, h->fens.slab, stride);
        else e = launch_reduce(h->d_slab, h->blk.rows, h->m.n_params, stride, lw, h->conv.c ? h->conv.d_gpad : d_out, h->stream, K, h->fens.slab, h->ensemble ? stride : 0);
        if (e != hipSuccess) return fail("%sreduce launch failed: %s", ens, hipGetErrorString(e));
        if (h->conv.c) {                                                // the user's layout: filter entries in front, W1's padded columns dropped
            e = launch_fc_conv_fold(h->conv.d_gpad, h->conv.d_cslab, h->conv.cslab_rows, h->conv.c, h->conv.w1_end, h->conv.n_zero, h->conv.n_params + 8, d_out,
                                    h->stream, K, (size_t)stride, h->conv.cslab_stride);
            if (e != hipSuccess) return fail("conv gradient fold launch failed: %s", hipGetErrorString(e));
        }
    }
    return 0;
}

// tile16 with the delta tape: forward -> adjoint -> dW GEMM block after block
static int t16_taped_loss_grad(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out) {
    const int stride = h->m.n_params + 8;
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    const int n_steps = total_steps(h);
    const size_t ns = h->m.ns;
    if (!h->sched.empty() && !(h->adj_split && h->adj_helper && h->d_t16_ztape))
        return fail("a step schedule is set, but this gradient does not run on rt16sh_adjoint_kernel (no pre-activation or rich tape)");
    if (pack(h, d_weights)) return 1;
    HIPCHK(hipMemsetAsync(h->d_slab, 0, (size_t)h->blk.rows * stride * sizeof(float), h->stream));
    for (int b = 0; b < h->blk.nblocks; b++) {
        const int c0 = b * h->blk.block, nc = std::min(h->blk.block, h->n_col - c0);
        if (nc <= 0) break;
        const int tiles_b = (nc + CT - 1) / CT;
        if (t16_forward_range(h, d_weights, h->d_sol, true, c0, nc)) return 1;
        {
            Timed tm(h, K_ADJOINT);
            AdjointGeom g = {512, 1, 3, 0};
            hipError_t e;
            if (h->adj_split && h->d_t16_ztape)
                // the companion of the split forward: one wavefront per flux net (+ a helper) per tile, writing tile16's delta tape
                e = rt_launch_adjoint_split(h->m, h->d_wimg, h->d_times, h->cfg.n_save, h->cfg.substeps,
                                            h->d_sol + (size_t)c0 * h->cfg.n_save * ns, h->d_truth + (size_t)c0 * h->cfg.n_save * ns, h->d_tape,
                                            h->d_t16_ztape, lw, h->d_slab + (size_t)(c0 / CT) * stride, nc, h->d_dwtape, h->split_rich, h->adj_helper, h->sp_adj, h->stream,
                                            RtEns(), sched_dev(h), n_steps);
            else
            e = launch_adjoint(h->m, h->pk, d_weights, h->d_wf, h->d_wb, h->d_tiles, h->d_bias_zoff, h->d_bias_goff,
                                          h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times, h->cfg.n_save, h->cfg.substeps,
                                          h->d_sol + (size_t)c0 * h->cfg.n_save * ns, h->d_truth + (size_t)c0 * h->cfg.n_save * ns, h->d_tape,
                                          lw, h->d_slab + (size_t)(c0 / CT) * stride, nc, g,
                                          (MODEL_FLOATS + (h->ag_rows ? lds_floats_adjoint_ag(h->m) : (h->d_t16_ztape ? lds_floats_adjoint_noA(h->m) : lds_floats_adjoint(h->m)))) * sizeof(float),
                                          h->stream, h->d_dwtape, h->d_t16_ztape);
            if (e != hipSuccess) return fail("adjoint (taped dW) launch failed: %s", hipGetErrorString(e));
        }
        {
            Timed tm(h, K_DW1);
            hipError_t e = dw_launch(h, (size_t)tiles_b * n_steps * h->m.nst, h->d_slab + ((size_t)h->n_tiles + (size_t)b * h->dw.slices) * stride);
            if (e != hipSuccess) return fail("dW GEMM launch failed: %s", hipGetErrorString(e));
        }
    }
    {
        Timed tm(h, K_REDUCE);
        hipError_t e = launch_reduce(h->d_slab, h->blk.rows, h->m.n_params, stride, lw, d_out, h->stream);
        if (e != hipSuccess) return fail("reduce launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

// tile16 with the weight-gradient tiles in registers: the whole problem in one adjoint launch
static int t16_inreg_loss_grad(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out) {
    const int stride = h->m.n_params + 8;
    if (forward_impl(h, d_weights, h->d_sol, true)) return 1;
    if (!h->geo_ok)
        return fail("network too large for the tile engine's in-register adjoint (%d weight-gradient tiles, %zu B of LDS) and its "
                    "delta tape does not fit in HBM (or COLNDE_T16_DWTAPE=0)", h->m.n_tiles, h->lds_adj);
    if (!h->d_slab) {
        hipError_t e = h->mem.alloc(&h->d_slab, (size_t)h->n_tiles * stride);
        if (e != hipSuccess) return fail("hipMalloc of the partial-gradient slab failed: %s", hipGetErrorString(e));
    }
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    {
        Timed tm(h, K_ADJOINT);
        hipError_t e = launch_adjoint(h->m, h->pk, d_weights, h->d_wf, h->d_wb, h->d_tiles, h->d_bias_zoff, h->d_bias_goff,
                                      h->d_bcs, h->d_times, h->cfg.n_save, h->cfg.substeps, h->d_sol, h->d_truth, h->d_tape,
                                      lw, h->d_slab, h->n_col, h->geo, h->lds_adj, h->stream);
        if (e != hipSuccess) return fail("adjoint launch failed: %s", hipGetErrorString(e));
    }
    {
        Timed tm(h, K_REDUCE);
        hipError_t e = launch_reduce(h->d_slab, h->n_tiles, h->m.n_params, stride, lw, d_out, h->stream);
        if (e != hipSuccess) return fail("reduce launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

extern "C" int colnde_loss_grad_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!d_weights || !scalings || !d_out) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    if (h->m.inplace) return fail("the in-place NDE! variant is an evaluation RHS; gradients use the training RHS (inplace_variant = 0)");
    HIPCHK(hipSetDevice(h->device));
    if (h->auto_substeps) {
        if (!h->have_problem) return fail("colnde_set_problem has not been called");
        if (refuse_auto_on_a_shard(h)) return 1;
        h->auto_substeps = false;
        if (choose_substeps_impl(h, d_weights, h->cfg.reltol, nullptr, nullptr)) { h->auto_substeps = true; return 1; }
    }
    if (check_stability(h)) return 1;
    if (h->use_rt) return rt_loss_grad(h, d_weights, scalings, d_out);
    if (h->use_fc) return fc_loss_grad(h, d_weights, scalings, d_out);
    if (t16_plan_dwtape(h)) return 1;
    if (!h->sched.empty() && h->t16_dwtape != 1) return fail("a step schedule is set, but the delta tape of this problem was not planned: no gradient path runs it");
    return h->t16_dwtape == 1 ? t16_taped_loss_grad(h, d_weights, scalings, d_out) : t16_inreg_loss_grad(h, d_weights, scalings, d_out);
}

extern "C" int colnde_loss_grad(colnde_handle* h, const float* weights, const float scalings[6], float terms[6],
                                float* total, float* grad) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!weights || !scalings || !terms || !total || !grad) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    const int np = user_params(h);
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * np, hipMemcpyHostToDevice, h->stream));
    if (colnde_loss_grad_dev(h, h->d_w, scalings, h->d_out)) return 1;
    float o[8];
    HIPCHK(hipMemcpyAsync(grad, h->d_out, sizeof(float) * np, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(o, h->d_out + np, sizeof(o), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int q = 0; q < 6; q++) terms[q] = o[q];
    *total = o[6];
    if (!std::isfinite(o[6])) return fail("the loss is not finite (%g): the solve left the stable regime (time step, weights or inputs)", o[6]);
    return 0;
}
