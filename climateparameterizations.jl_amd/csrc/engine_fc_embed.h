// engine_fc_embed.h — the free-convection embedded step (engine_fc_embed.hip): what progress_neural_network does per ocean-model iteration
// (free_convection/src/oceananigans_nn.jl:153-165: the NN forcing of T as given, then convective_adjustment!) and diagnose_wT_NN (:100-118)
// in one launch, on fc32's operand images and tile widths.
#pragma once
#include "colnde_dev.h"
#include "engine_fc.h"                    // FC_CONV_MAX

struct FcEmbedArgs {
    const float *imgf, *bias;             // fc_launch_pack's forward image and biases for tile width cw
    int cw;                               // 32 | 16 (fc_tile_width)
    const float* T;                       // [n_col][Nz], k = 0 deepest, the units colnde_infer_dz_wT takes
    const float* top_flux;                // [n_col]
    const float *halo_bottom, *halo_top;  // [n_col] each, or null: the nearest interior value (zero-gradient fill)
    float Lz, dt, K;                      // dz = Lz/Nz, c = dt/dz²; dt is not read by the diagnosis-only mode
    float* dz_wT;                         // [n_col][Nz]     +∂z wT of T as given (step modes)
    float* T_out;                         // [n_col][Nz]     T′ (step modes); may be T
    float* wT_faces;                      // [n_col][Nz + 1] wT_NN − κ ∂T/∂z of T as given, or null
    int n_col;
    bool step;                            // true: forcing + adjustment (+ diagnosis when wT_faces); false: diagnosis only
};

// the network shapes of fc_supported (Nz = 32 | 64); T, dz_wT, T_out and wT_faces 16-byte aligned (hipErrorInvalidValue otherwise)
hipError_t fce_set_kernel_attributes();          // both kernel families
hipError_t launch_fc_embed(const DevModel& m, const FcEmbedArgs& a, hipStream_t stream);

// The K members of an ensemble at once (fce_ens_kernel: 16-column tiles, blockIdx.y = model).  Member k's arrays lie k strides from model 0's, in
// floats.  Passed by value to the kernel.
struct FceEns {
    size_t img = 0, bias = 0;             // operand image, biases (fc_image_floats, fc_bias_floats)
    size_t state = 0, halo = 0, faces = 0;   // T, dz_wT, T_out: n_col Nz; the halos: n_col; wT_faces: n_col (Nz + 1)
};
#define FCE_TAPS_FLOATS (FC_CONV_MAX + 1)  // per member: the taps in the kernel's order, then the bias
// `a` holds model 0's pointers (a.cw = 16; top_flux is shared); conv = 0: plain members, else the filter length, taps [n_models][FCE_TAPS_FLOATS]
// (launch_fce_taps).  Only the BASE pointers carry the 16-byte rule: a member's T, dz_wT and T_out start a multiple of Nz floats in, and the faces
// are stored one float at a time.
hipError_t launch_fc_embed_ens(const DevModel& m, const FcEmbedArgs& a, int n_models, int conv, const float* taps, hipStream_t stream);
// taps [n_models][FCE_TAPS_FLOATS] from the head of each member's parameter vector (w_stride floats apart)
hipError_t launch_fce_taps(const float* w, size_t w_stride, int conv, int n_models, float* taps, hipStream_t stream);
