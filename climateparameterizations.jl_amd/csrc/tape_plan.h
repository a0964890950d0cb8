// tape_plan.h — how many columns (and save intervals) of tape fit the free device memory: the arithmetic of the gradient paths' planners as pure
// functions.  No HIP: plain C++17, by value, so that tests/tape_plan_check.cpp runs every branch on the host (a nearly full card included).
#pragma once
#include <algorithm>
#include <cstddef>

inline size_t hbm_budget(size_t free_bytes, size_t margin_bytes) { return free_bytes > margin_bytes ? free_bytes - margin_bytes : 0; }

// Columns per pass of a gradient path whose tapes hold `fit` columns: everything when it fits, otherwise the problem cut into equal blocks of whole
// tiles — whole granules (rounds of the machine) from one granule up — and never more than fit.  0: not even one tile fits.
// (tile, granule): regtile (1024, 1024), fc32 (32, 8192), tile16 (16, 4096).
inline int plan_column_block(int n_padded, size_t fit_columns, int tile, int granule) {
    if (fit_columns >= (size_t)n_padded) return n_padded;
    if (fit_columns < (size_t)tile) return 0;
    const int nb = (int)(((size_t)n_padded + fit_columns - 1) / fit_columns);
    int block = ((n_padded + nb - 1) / nb + tile - 1) / tile * tile;
    if (block >= granule) block = (block + granule - 1) / granule * granule;
    while ((size_t)block > fit_columns) block -= block > granule ? granule : tile;
    return block;
}

// fc32: column blocks when they hold at least 16,384 columns (or everything), otherwise time segments of `seg` save intervals — of all columns, or of
// the largest column block one interval fits for.  per_col_iv: bytes of tape per column and save interval.  The partial-gradient slab grows with the
// number of segments ([tile][segment] + [block][segment][<= 512 slices] rows of n_params + 8 floats: 50 GB at 128 segments of the 64-level network): it
// must fit beside the tapes it is chosen for.  seg = 0 (or block < 32): not even one tile and one interval with its slab fit.
struct FcTapePlan { int block, seg; };
inline FcTapePlan plan_fc_block_seg(int n32, int n_iv, int cw, size_t per_col_iv, size_t budget, int n_params) {
    const size_t fit = budget / (per_col_iv * n_iv);                 // columns whose whole-axis tapes fit
    FcTapePlan p = {plan_column_block(n32, fit, 32, 8192), n_iv};
    if (fit >= (size_t)n32 || p.block >= 16384) return p;
    const size_t cols_iv = budget / per_col_iv / 32 * 32;            // columns whose ONE-interval tapes fit
    if (cols_iv < 32) return p;
    p.block = (int)std::min<size_t>((size_t)n32, cols_iv);
    if (p.block < n32 && p.block >= 8192) p.block = p.block / 8192 * 8192;
    p.seg = (int)std::min<size_t>((size_t)n_iv, budget / (per_col_iv * (size_t)p.block));
    auto over = [&](int sg) {
        const size_t nsg = ((size_t)n_iv + sg - 1) / sg, nblk = ((size_t)n32 + p.block - 1) / p.block;
        return per_col_iv * (size_t)p.block * sg + ((size_t)(n32 / cw) + nblk * 512) * nsg * (size_t)(n_params + 8) * sizeof(float) > budget;
    };
    while (p.seg > 1 && over(p.seg)) p.seg--;
    if (over(p.seg)) p.seg = 0;
    return p;
}

// A free-convection ensemble: one block of all columns per model on the model's share of the budget.  What a model owns beside the tapes: λ between
// segments and the slab rows ([tile][segment] + [segment][<= 512 slices] rows of n_params + 8 floats).
inline size_t fc_ens_model_bytes(int n32, int n_iv, int cw, int Nz, size_t per_col_iv, int n_params, int seg) {
    const size_t nsg = ((size_t)n_iv + seg - 1) / seg;
    return per_col_iv * (size_t)n32 * seg + ((size_t)(n32 / cw) + 512) * nsg * ((size_t)n_params + 8) * sizeof(float) + (size_t)n32 * Nz * sizeof(float);
}
inline int plan_fc_ens_seg(int n32, int n_iv, int cw, int Nz, size_t per_col_iv, size_t budget, int n_params) {
    int seg = n_iv;
    while (seg > 1 && fc_ens_model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg) > budget) seg--;
    return seg;
}

// A conv ensemble (colnde_create_conv_ensemble): per_col_iv carries the conv tape's bytes too; beside what fc_ens_model_bytes counts a model owns the filter
// slab (cslab_seg_floats floats per time segment), the padded weight vector (n_params floats) and the padded gradient row (n_params + 8).
inline size_t fc_conv_ens_model_bytes(int n32, int n_iv, int cw, int Nz, size_t per_col_iv, int n_params, int seg, size_t cslab_seg_floats) {
    const size_t nsg = ((size_t)n_iv + seg - 1) / seg;
    return fc_ens_model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg) + (nsg * cslab_seg_floats + 2 * (size_t)n_params + 8) * sizeof(float);
}
inline int plan_fc_conv_ens_seg(int n32, int n_iv, int cw, int Nz, size_t per_col_iv, size_t budget, int n_params, size_t cslab_seg_floats) {
    int seg = n_iv;
    while (seg > 1 && fc_conv_ens_model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg, cslab_seg_floats) > budget) seg--;
    return seg;
}

// ---- the planners' decisions: everything between reading the switches and the first allocation ----------------------------------------------------------
// Environment switches arrive parsed.  A flag: FLAG_UNSET, or atoi(value) != 0.  A forced block: atoi(value), 0 when unset (a value below one tile
// forces nothing).  Sizes that come from engine headers (record rows, mask words, LDS bytes of the adjoint variants) arrive as numbers.
enum { FLAG_UNSET = -1, FLAG_OFF = 0, FLAG_ON = 1 };

// fc32: bytes of tape per column and save interval — the record row, the relu bit masks of a cw-column tile, the switch pattern of
// ConvectiveAdjustmentNDE, the conv tape of a conv handle (conv_tape_floats_per_record: 0 without a filter)
inline size_t fc_tape_bytes_per_col_iv(int substeps, int nst, size_t row_floats, size_t mask_words, int cw, bool has_switch_tape, size_t conv_tape_floats_per_record) {
    return (size_t)substeps * nst * (row_floats * sizeof(float) + mask_words * sizeof(unsigned int) / cw + (has_switch_tape ? sizeof(unsigned long long) : 0) +
                                     conv_tape_floats_per_record / 16 * sizeof(float));
}

// fc32, a single handle and an ensemble of K models alike.  forced_seg: COLNDE_FC_SEG as a count, 0 when unset, -1 when set to no count (which
// still keeps a forced block from resetting seg to the whole axis).
enum FcPlanStatus { FC_PLAN_OK, FC_PLAN_NOTHING_FITS, FC_PLAN_ENSEMBLE_REFUSED };
struct FcTapesIn {
    int n32, n_iv, cw, Nz, n_params;
    size_t per_col_iv, free_bytes;
    bool ensemble;
    int K;                        // models (an ensemble may hold one)
    size_t cslab_seg_floats;      // a conv ensemble: floats of filter slab per time segment (0: no filter)
    int forced_block, forced_seg;
};
struct FcTapes { int block, seg; size_t model_bytes /* an ensemble: what one model needs */; FcPlanStatus status; };
inline FcTapes plan_fc_tapes(const FcTapesIn& in) {
    FcTapes p = {0, 0, 0, FC_PLAN_OK};
    if (!in.ensemble) {
        const size_t margin = ((size_t)3 << 30) + (size_t)(in.n32 / in.cw * 8 + 4096) * (in.n_params + 8) * sizeof(float) + (size_t)in.n32 * in.Nz * sizeof(float);
        const FcTapePlan bs = plan_fc_block_seg(in.n32, in.n_iv, in.cw, in.per_col_iv, hbm_budget(in.free_bytes, margin), in.n_params);
        p.block = bs.block;
        p.seg = bs.seg;
        if (in.forced_block >= 32) { p.block = std::min(in.n32, in.forced_block / 32 * 32); if (in.forced_seg == 0) p.seg = in.n_iv; }
        if (in.forced_seg >= 1) p.seg = std::min(in.n_iv, in.forced_seg);
        if (p.block < 32 || p.seg < 1) p.status = FC_PLAN_NOTHING_FITS;
        return p;
    }
    // one block of all columns per model (column blocks do not occur at <= 4,096 columns) on the model's share of the budget
    const size_t budget = hbm_budget(in.free_bytes, (size_t)3 << 30) / (size_t)in.K;
    const bool conv = in.cslab_seg_floats != 0;
    auto need = [&](int seg) {
        return conv ? fc_conv_ens_model_bytes(in.n32, in.n_iv, in.cw, in.Nz, in.per_col_iv, in.n_params, seg, in.cslab_seg_floats)
                    : fc_ens_model_bytes(in.n32, in.n_iv, in.cw, in.Nz, in.per_col_iv, in.n_params, seg);
    };
    p.block = in.n32;
    p.seg = conv ? plan_fc_conv_ens_seg(in.n32, in.n_iv, in.cw, in.Nz, in.per_col_iv, budget, in.n_params, in.cslab_seg_floats)
                 : plan_fc_ens_seg(in.n32, in.n_iv, in.cw, in.Nz, in.per_col_iv, budget, in.n_params);
    if (in.forced_seg >= 1) p.seg = std::min(in.n_iv, in.forced_seg);
    p.model_bytes = need(p.seg);
    if (p.model_bytes > budget) p.status = FC_PLAN_ENSEMBLE_REFUSED;
    return p;
}

// tile16 / net-split, a single handle: taped weight gradients on or off, which optional tape, the block.  On when the tapes fit; the in-register
// adjoint remains the fallback, except for a network whose activation rows live in global memory (ag_rows), where the taped adjoint with the Z tape is
// the ONLY gradient path (1,024 threads: n_bias <= 4 x 1,024) and every "off" is a refusal.
enum T16PlanStatus {
    T16_PLAN_TAPED,
    T16_PLAN_IN_REGISTER,         // no delta tape: the in-register path follows
    T16_PLAN_REFUSED_OFF,         // rows in global memory, and the delta tape is off (forced, or the tile state is too large)
    T16_PLAN_REFUSED_TOO_LARGE,   // rows in global memory, and the network exceeds the taped adjoint's limits
    T16_PLAN_REFUSED_NO_FIT       // rows in global memory, and not one tile of delta tape fits
};
struct T16TapesIn {
    int n16, tile /* columns per tile */, ns, n_bias;
    bool ag_rows, adj_split;
    size_t lds_adjoint, lds_adjoint_noA, lds_adjoint_ag;      // bytes of LDS of the taped adjoint's variants, the model's floats included
    size_t per_col, per_col_rich, budget;                     // bytes of tape per column with the pre-activation / the rich tape
    int dwtape, ztape, split_rich;                            // COLNDE_T16_DWTAPE, _ZTAPE, _SPLIT_RICH: flags
    int forced_block;                                         // COLNDE_T16_BLOCK
};
struct T16Tapes { bool need_z; int block; bool rich; T16PlanStatus status; };
inline T16Tapes plan_t16_tapes(const T16TapesIn& in) {
    const size_t lds_max = 160 * 1024;
    T16Tapes p = {false, 0, false, T16_PLAN_IN_REGISTER};
    bool want = in.dwtape != FLAG_OFF;
    if (want && (size_t)in.tile * in.ns > 6 * 512) want = false;
    // with the Z tape (the default) the taped adjoint's LDS holds no activation array; a network that fits only that way (3 x 96-400-31: 166 KB with the
    // array, 83 KB without) then NEEDS the Z tape
    if (want && !in.ag_rows && in.lds_adjoint > lds_max) {
        if (in.ztape != FLAG_OFF && in.lds_adjoint_noA <= lds_max && in.n_bias <= 4 * 512) p.need_z = true;
        else want = false;
    }
    if (in.ag_rows) {
        if (!want) { p.status = T16_PLAN_REFUSED_OFF; return p; }
        if (in.n_bias > 4 * 1024 || in.lds_adjoint_ag > lds_max) { p.status = T16_PLAN_REFUSED_TOO_LARGE; return p; }
    }
    if (want) {
        // ONE block of columns (whole rounds of 4,096 columns = one workgroup per CU when possible)
        p.block = plan_column_block(in.n16, in.budget / in.per_col, in.tile, 4096);
        if (in.forced_block >= in.tile) p.block = std::min(in.n16, in.forced_block / in.tile * in.tile);
        if (p.block <= 0) want = false;
        // The net-split pair's rich tape replaces the pre-activation tape and is 4x its size per column: by default on blocks of at most 2,048
        // columns (where it pays), forced on or off by COLNDE_T16_SPLIT_RICH.  It must fit WITH the other tapes: a forced one shrinks the block, an
        // automatic one is dropped.
        const bool rich_possible = in.adj_split && in.ztape != FLAG_OFF && in.split_rich != FLAG_OFF;
        p.rich = want && rich_possible && (in.split_rich == FLAG_ON || p.block <= 128 * in.tile);
        if (p.rich && (size_t)p.block * in.per_col_rich > in.budget) {
            const size_t fit_rich = in.budget / in.per_col_rich / in.tile * in.tile;
            if (in.split_rich == FLAG_ON && fit_rich >= (size_t)in.tile) p.block = (int)std::min<size_t>((size_t)p.block, fit_rich);
            else p.rich = false;
        }
    }
    if (!want) {
        p.block = 0;
        p.status = in.ag_rows ? T16_PLAN_REFUSED_NO_FIT : T16_PLAN_IN_REGISTER;
        return p;
    }
    p.status = T16_PLAN_TAPED;
    return p;
}

// A wind-mixing ensemble: one block of all columns per model.  The rich tape while the K models' tiles number at most 128 (2,048 columns in flight:
// the single handle's crossover counts concurrent tiles whoever owns them) unless COLNDE_T16_SPLIT_RICH says; an automatic one gives way to the plain
// tape when it does not fit, as for one handle.  per_model_*: bytes of a model's tapes, slab rows, solution and weight image with either tape.
struct T16EnsTapes { bool rich; size_t bytes_per_model; bool refused; };
inline T16EnsTapes plan_t16_ens_tapes(int K, int n_tiles, size_t per_model_rich, size_t per_model_plain, size_t budget, int split_rich) {
    const bool forced = split_rich != FLAG_UNSET;
    T16EnsTapes p = {forced ? split_rich == FLAG_ON : (size_t)K * n_tiles <= 128, 0, false};
    if (p.rich && !forced && (size_t)K * per_model_rich > budget) p.rich = false;
    p.bytes_per_model = p.rich ? per_model_rich : per_model_plain;
    p.refused = (size_t)K * p.bytes_per_model > budget;
    return p;
}

// A tile ensemble (colnde_create_tile_ensemble: K models of any tile16 architecture): one block of all columns per model on the model's share of
// (free memory - 3 GB).  tile16 has no time segments: what a model needs either fits its share or the ensemble is refused with the bytes.  A model
// owns, for its n_tiles x n_steps x nst records of 16 columns: the stage tape (ns floats per column), the delta tape (row_floats), the hidden
// pre-activation tape (ztape_col_floats); its slab rows (slab_rows — the adjoint's, one per tile, and the dW GEMM's, one per slice of the count a
// single handle of this size plans — of n_params + 8 floats); its solution; its two packed weight images (image_floats) and, with the rows in
// global memory, its bf16 plane images (plane_words) and n_tiles slabs of activation rows (ag_floats_per_tile; 0: rows in LDS).
struct T16TileEnsIn {
    int K, n_tiles, n_steps, nst, ns, n_params, n_col, n_save, slab_rows;
    size_t row_floats, ztape_col_floats, image_floats, plane_words, ag_floats_per_tile;
    size_t free_bytes;
};
struct T16TileEns { size_t records, bytes_per_model, share; bool refused; };
inline T16TileEns plan_t16_tile_ens(const T16TileEnsIn& in) {
    T16TileEns p = {(size_t)in.n_tiles * in.n_steps * in.nst, 0, 0, false};
    const size_t tile = 16;
    const size_t tapes = p.records * tile * ((size_t)in.ns + in.row_floats + in.ztape_col_floats);
    const size_t slab = (size_t)in.slab_rows * ((size_t)in.n_params + 8);
    const size_t sol = (size_t)in.n_col * in.n_save * in.ns;
    const size_t rows = (size_t)in.n_tiles * in.ag_floats_per_tile;
    p.bytes_per_model = (tapes + slab + sol + in.image_floats + rows) * sizeof(float) + in.plane_words * sizeof(unsigned int);
    p.share = hbm_budget(in.free_bytes, (size_t)3 << 30) / (size_t)(in.K > 0 ? in.K : 1);
    p.refused = p.bytes_per_model > p.share;
    return p;
}

// regtile: the block, with the Z1 tape when even 1,024 columns fit with it and without it otherwise; COLNDE_RT_BLOCK forces a size.  block = 0: the
// stage tapes of not even 1,024 columns fit.
struct RtTapes { int block; bool ztape; };
inline RtTapes plan_rt_tapes(int n32, size_t per_col_x, size_t per_col_2, size_t per_col_z, size_t budget, bool want_z, int forced_block) {
    RtTapes p = {0, want_z};
    for (int pass = 0; pass < 2 && p.block == 0; pass++) {
        p.block = plan_column_block(n32, budget / (per_col_x + per_col_2 + (p.ztape ? per_col_z : 0)), 1024, 1024);
        if (p.block == 0) p.ztape = false;       // not even 1,024 columns with the Z1 tape: try without it
    }
    if (forced_block >= 32) p.block = std::min(n32, forced_block / 32 * 32);
    return p;
}
