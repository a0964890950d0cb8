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
