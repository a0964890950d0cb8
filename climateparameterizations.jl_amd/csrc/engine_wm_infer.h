// engine_wm_infer.h — embedded inference of the trained wind-mixing NDE (wind_mixing/src/NDE_oceananigans.jl:288-329, :380-405):
// the three flux networks evaluated on an ocean column's u, v, T, optionally fused with the implicit diffusion step of that state and / or
// with the diagnosis of the total face fluxes diagnose_NN_flux_uw / _vw / _wT (:226-286).
#pragma once
#include <hip/hip_runtime.h>
#include "mpp_sweep.h"

// the one shape the kernels are built for: Nz = 32, three 96-50-20-31 networks (regtile's shape)
#define WM_NZ 32
#define WM_H1 50
#define WM_H2 20
#define WM_NET (96 * WM_H1 + WM_H1 + WM_H1 * WM_H2 + WM_H2 + WM_H2 * 31 + 31)   // 6521 parameters per net, Flux.destructure order

struct WmInferArgs {
    const float* weights;                 // [3 WM_NET] uw; vw; wT
    float mu[6], sigma[6];                // scalings u, v, T, uw, vw, wT
    int act1, act2;                       // COLNDE_ACT_* of the two hidden layers (identity on the output)
    const float *u, *v, *T;               // [n_col][32], physical units, k = 0 deepest
    const float* top_flux;                // [3][n_col]
    float Lz;
    float *dz_uw, *dz_vw, *dz_wT;         // [n_col][32]
    int n_col;
    // fused step only (fused = true): the diffusion step of the state as given; outputs may alias their own inputs
    bool fused;
    const float* halo_bottom;             // [3][n_col] or null
    MppParams mpp;
    float *u_out, *v_out, *T_out;
    // flux diagnosis (diag = true): uw, vw, wT [n_col][33] of the state as given; mpp (its step is not used unless fused) and halo_bottom as
    // above, halo_top [3][n_col] or null.  diag without fused writes no d/dz arrays (dz_* unused).
    bool diag;
    const float* halo_top;
    float *uw, *vw, *wT;
};

// every pointer of the state and the outputs must be 16-byte aligned (hipErrorInvalidValue otherwise)
hipError_t launch_wm_infer(const WmInferArgs& a, hipStream_t stream);
