// engine_fc_embed.h — the free-convection embedded step (engine_fc_embed.hip): what progress_neural_network does per ocean-model iteration
// (free_convection/src/oceananigans_nn.jl:153-165: the NN forcing of T as given, then convective_adjustment!) and diagnose_wT_NN (:100-118)
// in one launch, on fc32's operand images and tile widths.
#pragma once
#include "colnde_dev.h"

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
hipError_t fce_set_kernel_attributes();
hipError_t launch_fc_embed(const DevModel& m, const FcEmbedArgs& a, hipStream_t stream);
