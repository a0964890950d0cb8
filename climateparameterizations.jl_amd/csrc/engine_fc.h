// engine_fc.h — host interface of the 32-column free-convection engine (engine_fc.hip).
#pragma once
#include "colnde_dev.h"

// FreeConvectionNDE (classical RK4) or ConvectiveAdjustmentNDE (RK4 or the stabilised RKC2 stepper) with Dense(Nz,4Nz,relu) ->
// Dense(4Nz,4Nz,relu) -> Dense(4Nz,Nz-1), Nz = 32 | 64
bool fc_supported(const DevModel& m, int stepper);
size_t fc_image_floats(int Nz);          // floats of one A-operand image (forward and backward images have the same size)
size_t fc_bias_floats(int Nz);
size_t fc_record_row_floats(int Nz);     // = dwtape_row_floats(m): the records are tile16's delta-tape records
static inline size_t fc_mask_words() { return 512; }     // relu-derivative bits per 32-column tile and stage: [layer 2][wave 4][lane 64] dwords
static inline size_t fc_switch_words(int cw) { return (size_t)cw; }   // ConvectiveAdjustmentNDE: the switch pattern of a stage, one 64-bit word per column
hipError_t fc_set_kernel_attributes();
// cw = columns per workgroup tile (32: v_mfma_f32_32x32x2_f32, the throughput shape; 16: v_mfma_f32_16x16x4_f32, half the matrix work per stage for
// problems that cannot fill 32-column tiles on every CU); the operand images depend on it
int fc_tile_width(int n_col);
// simgf / simgb (fc_split_image_words(Nz) words each, or null): the operand images of COLNDE_MATRIX_BF16X3_EXACT — every weight split exactly into three
// bf16 planes, in each wave's stream order — packed beside the f32 images (fc_split_supported: tile width 32 -> engine_fc_split.hip's kernels, 16 -> the
// SPLIT instantiations of engine_fc.hip's; the two orders differ, the size does not)
size_t fc_split_image_words(int Nz);
bool fc_split_supported(int cw);
// Ensembles (colnde_create_fc_ensemble): K networks of the shape on the SAME columns, the model index in blockIdx.y of the 16-column kernels.  What a
// model owns lies at a fixed stride from model 0's, in elements of the array's type; x0 is 0 (the shared initial state) or `sol` (a time segment
// restarting from the model's own saved state).  x0 at iv_begin = 0, bcs, truth, the save times and the RKC2 table are shared.  Passed by value.
// member_w / member_colw (the adjoint kernel only; colnde_ensemble_set_member_loss): null, the loss enters through the scalar w_loss with every column
// weighted 1; given, model k's loss weight is member_w[8 k] (the temperature term of its LossWeights row) and column c enters with member_colw[k][c].
struct FcEns {
    size_t w = 0, img = 0, simg = 0, bias = 0, x0 = 0, sol = 0, dwtape = 0, masks = 0, swtape = 0, lam = 0, slab = 0;
    int n_models = 1;
    const float* member_w = nullptr;
    const float* member_colw = nullptr;
};
// The reference's --conv network (train_free_convection_nde.jl:110-122): Conv((c, 1), 1 => 1, relu) in front of the three Dense layers, on the 16-column
// kernels (colnde_create_conv).  The filter is applied where the stage input goes to LDS: y[i] = relu(b + sum_d w[c-1-d] x[i+d]) (NNlib's conv flips the
// kernel), i < M = Nz - c + 1, zero above; the dense chain runs on W1 padded with zero columns to 4Nz x Nz, so images, dW GEMM and reducers are the plain
// network's.  wb: the c taps and the bias, as they lead the user's parameter vector.  ctape [record][16 columns][2 Nz]: the stage input x (forward
// kernel) and the cotangent of the filter's pre-activation (adjoint kernel), record index as in the delta tape; fc_launch_conv_grad contracts the two.
// Passed by value to the CONV kernels only.
#define FC_CONV_MAX 8                    // taps: an unrolled loop in the kernels
struct FcConv {
    int c = 0;
    const float* wb = nullptr;
    float* ctape = nullptr;
};
static inline size_t fc_conv_tape_floats(int Nz) { return (size_t)16 * 2 * Nz; }       // per record (16-column tile and stage)
// A conv ensemble (colnde_create_conv_ensemble): what model k owns of the filter's lies at k strides from model 0's — the taps and bias at the head of
// its own parameter vector (wb floats apart: the conv parameter count) and its conv tape (ctape floats apart).  Passed by value to the CONV + ENS
// entry points only, beside FcConv (model 0's pointers) and FcEns: the argument blocks of the other entry points stay as they are.
struct FcConvEns {
    size_t wb = 0, ctape = 0;
};
// ens != null (cw = 16, both image kinds given): the images of all ens->n_models models, weights ens->w floats apart.  With imgb, simgf and simgb all
// null it is a forward-only pack: the f32 forward images and the biases (the embedded step's operands, engine_fc_embed.hip)
hipError_t fc_launch_pack(const DevModel& m, int cw, const float* w, float* imgf, float* imgb, float* bias, unsigned int* simgf, unsigned int* simgb,
                          hipStream_t stream, const FcEns* ens = nullptr);
// Save intervals [iv_begin, iv_end) from x0 (column stride x0_stride floats).  dwtape == nullptr: plain forward solve.  Otherwise, from interval
// tape_iv0 on (iv_begin <= tape_iv0 < iv_end; records numbered from its first step), the stage inputs
// and hidden activations go into the records [tile32][step of this launch][stage][cw/16 records of 16 columns][R], the relu bits into masks [..][512] and
// (ConvectiveAdjustmentNDE) the switch pattern into swtape [..][cw].  Stages per step: m.nst (4, or the RKC2 stage count when m.rkc is set).
// simgf != null (and cw == 32): the split kernels (v_mfma_f32_32x32x16_bf16 on exact three-way operand splits) instead of the f32-MFMA ones
hipError_t fc_launch_forward(const DevModel& m, int cw, const float* imgf, const unsigned int* simgf, const float* bias, const float* x0, size_t x0_stride,
                             const float* bcs, const float* save_times, int n_save, int iv_begin, int iv_end, int tape_iv0, int substeps, float* sol,
                             float* dwtape, unsigned int* masks, unsigned long long* swtape, int n_col, hipStream_t stream, const FcEns* ens = nullptr,
                             const FcConv* conv = nullptr, const FcConvEns* cens = nullptr);
// slab: one row of n_params + 8 floats per tile (bias gradients and the squared-error sum; the weight gradients are the dW GEMM's).
// lam_io [columns padded to 32][Nz]: carries λ between the time segments of a segmented gradient pass (null when one launch covers the axis).
hipError_t fc_launch_adjoint(const DevModel& m, int cw, const float* imgb, const unsigned int* simgb, const float* save_times, int n_save, int iv_begin, int iv_end,
                             int substeps,
                             const float* sol, const float* truth, float* dwtape, const unsigned int* masks, const unsigned long long* swtape,
                             float w_loss, float* lam_io, float* slab, int n_col, hipStream_t stream, const FcEns* ens = nullptr,
                             const FcConv* conv = nullptr, const FcConvEns* cens = nullptr);
// compute_neural_network_forcing! (double_gyre_nn.jl:149-168): T [n_col][Nz] model units, top_flux [n_col], out = -dz(wT) on cell centres
hipError_t fc_launch_infer(const DevModel& m, int cw, const float* imgf, const float* bias, const float* T, const float* top_flux, float inv_dz,
                           float* out, int n_col, hipStream_t stream);

// engine_fc_split.hip: the same kernels on v_mfma_f32_32x32x16_bf16 from exact three-way bf16 operand splits (COLNDE_MATRIX_BF16X3_EXACT; 32-column tiles):
// one wave per 32-row tile of a hidden layer, activations as bf16 planes in LDS, split once in the producing wave's epilogue.  Reached through the
// fc_launch_* calls above when the split images are handed over; tapes, slab rows and argument meaning are engine_fc.hip's.
hipError_t fcs_set_kernel_attributes();
hipError_t fcs_launch_pack(const DevModel& m, const float* w, unsigned int* simgf, unsigned int* simgb, hipStream_t stream);
hipError_t fcs_launch_forward(const DevModel& m, const unsigned int* simgf, const float* bias, const float* x0, size_t x0_stride, const float* bcs,
                              const float* save_times, int n_save, int iv_begin, int iv_end, int tape_iv0, int substeps, float* sol, float* dwtape,
                              unsigned int* masks, unsigned long long* swtape, int n_col, hipStream_t stream);
hipError_t fcs_launch_adjoint(const DevModel& m, const unsigned int* simgb, const float* save_times, int n_save, int iv_begin, int iv_end, int substeps,
                              const float* sol, const float* truth, float* dwtape, const unsigned int* masks, const unsigned long long* swtape,
                              float w_loss, float* lam_io, float* slab, int n_col, hipStream_t stream);
