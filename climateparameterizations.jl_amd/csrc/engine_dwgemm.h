// engine_dwgemm.h — the gradient tail every training path runs: the taped weight-gradient GEMM (tile16's taped adjoint, fc32 and its ensembles, the
// net-split pair and the wind-mixing ensembles write the same delta-tape records) and the fixed-order slab reduction (regtile's too).
#pragma once
#include <vector>
#include "colnde_dev.h"

struct LossWeights { float w[8]; };       // w[q] = loss_scaling[q] / (global element count of term q)

// the delta tape's records: floats per 16-column tile and stage
static inline int dwtape_ns4(const DevModel& m) { return (m.ns + 3) & ~3; }
static inline int dwtape_act4(const DevModel& m) { return (m.act_total + 3) & ~3; }
static inline size_t dwtape_row_floats(const DevModel& m) { return (size_t)dwtape_ns4(m) + (size_t)2 * m.n_nets * dwtape_act4(m); }

// dW GEMM on the bf16 pipe with exact three-way operand splitting (COLNDE_MATRIX_BF16X3_EXACT): the blocks are dealt to passes by layer so
// that a pass's operand features (split ONCE per record into LDS planes) and its accumulators fit one workgroup
struct DwSeg { int src, len, dst; };                                  // floats of a record row [src, src + len) -> compact features [dst, dst + len)
struct DwPassDesc { DwSeg seg[8]; int n_seg, Fc, m0, n_macros, maxm, nit; };

// The dW GEMM's whole plan, built on the host by dw_plan.h; the API uploads the two block lists into buffers the handle's pool owns.
struct DwPlan {
    std::vector<DwMacro> macros;          // the 64x64 blocks of every layer's weight matrix (the f32 kernels' work list)
    std::vector<DwMacro> split_macros;    // ... pass after pass with features in a pass's compact order (the split kernel's; DwPassDesc::m0 indexes it)
    std::vector<DwPassDesc> passes;       // empty: no split plan (split_ok false)
    int n_macros = 0, slices = 0;         // blocks of `macros`; K-slices of the records
    bool split_ok = false;                // the split plan exists
    bool lds_fit = false;                 // two records fit the LDS: the LDS-staged f32 kernel applies (dw_gemm_lds_fits when the plan was built)
};

bool dw_gemm_lds_fits(int row_floats, int n_macros);     // the LDS-staged dW kernel applies (else the L2-streaming one); reads COLNDE_T16_DWLDS
hipError_t dw_set_kernel_attributes(size_t max_lds_bytes);
// n_models > 1 (ensembles): grid.y = model, its records tape_mstride and its slab rows slab_mstride floats after the previous model's
hipError_t launch_dw_gemm(const float* dwtape, size_t n_records, int row_floats, const DwMacro* macros, int n_macros, int n_slices,
                          float* slab_rows, int slab_stride, hipStream_t stream, int n_models = 1, size_t tape_mstride = 0, size_t slab_mstride = 0);
// d_split_macros: the device copy of plan.split_macros
hipError_t launch_dw_gemm_split(const float* dwtape, size_t n_records, int row_floats, const DwPlan& plan, const DwMacro* d_split_macros, int n_slices,
                                float* slab_rows, int slab_stride, hipStream_t stream, int n_models = 1, size_t tape_mstride = 0, size_t slab_mstride = 0);
// n_models > 1 (ensembles): grid.y = model, slab slab_mstride and out out_mstride floats apart per model
hipError_t launch_reduce(const float* slab, int n_tiles, int n_params, int stride, const LossWeights& lw, float* out,
                         hipStream_t stream, int n_models = 1, size_t slab_mstride = 0, int out_mstride = 0);
// ... under a member loss (colnde_ensemble_set_member_loss): model k's six raw sums are scaled by its own lwk[k] (device, [n_models])
hipError_t launch_reduce_member(const float* slab, int n_tiles, int n_params, int stride, const LossWeights* lwk, float* out,
                                hipStream_t stream, int n_models, size_t slab_mstride, int out_mstride);
