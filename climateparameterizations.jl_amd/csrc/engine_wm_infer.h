// engine_wm_infer.h — embedded inference of the trained wind-mixing NDE (wind_mixing/src/NDE_oceananigans.jl:288-329, :380-405):
// the three flux networks evaluated on an ocean column's u, v, T, optionally fused with the implicit diffusion step of that state and / or
// with the diagnosis of the total face fluxes diagnose_NN_flux_uw / _vw / _wT (:226-286).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "mpp_sweep.h"

// the one shape the kernels are built for: Nz = 32, three 96-50-20-31 networks (regtile's shape)
#define WM_NZ 32
#define WM_H1 50
#define WM_H2 20
#define WM_NET (96 * WM_H1 + WM_H1 + WM_H1 * WM_H2 + WM_H2 + WM_H2 * 31 + 31)   // 6521 parameters per net, Flux.destructure order

// What one call of the embedding reads and writes, whichever kernel serves it (host only: the kernels take the members one by one).  The optional
// groups decide what is computed: u_out, v_out, T_out the fused diffusion step of the state as given (each may alias its own input), uw, vw, wT the
// diagnosis of the total face fluxes.  An ensemble's arrays carry a leading [K], top_flux excepted.
struct WmEmbedIO {
    const float *u, *v, *T;               // [n_col][32], physical units, k = 0 deepest
    const float* top_flux;                // [3][n_col]
    const float *halo_bottom, *halo_top;  // [3][n_col] or null; the step reads halo_bottom alone
    float Lz;
    float *dz_uw, *dz_vw, *dz_wT;         // [n_col][32]; the diagnosis without the step writes none (unused)
    float *u_out, *v_out, *T_out;         // [n_col][32]
    float *uw, *vw, *wT;                  // [n_col][33]
    int n_col;
    bool fused() const { return u_out != nullptr; }
    bool diag() const { return uw != nullptr; }
};
// the 16-byte rule of the state and the outputs a launch touches (an ensemble: of the base pointers); dz: the d/dz arrays are among them
inline bool wm_io_aligned(const WmEmbedIO& io, bool dz) {
    uintptr_t al = (uintptr_t)io.u | (uintptr_t)io.v | (uintptr_t)io.T;
    if (dz) al |= (uintptr_t)io.dz_uw | (uintptr_t)io.dz_vw | (uintptr_t)io.dz_wT;
    if (io.fused()) al |= (uintptr_t)io.u_out | (uintptr_t)io.v_out | (uintptr_t)io.T_out;
    if (io.diag()) al |= (uintptr_t)io.uw | (uintptr_t)io.vw | (uintptr_t)io.wT;
    return !(al & 15);
}

struct WmInferArgs {
    WmEmbedIO io;
    const float* weights;                 // [3 WM_NET] uw; vw; wT
    float mu[6], sigma[6];                // scalings u, v, T, uw, vw, wT
    int act1, act2;                       // COLNDE_ACT_* of the two hidden layers (identity on the output)
    MppParams mpp;                        // fused or diag (its step is not used unless fused)
};

// every pointer of the state and the outputs must be 16-byte aligned (hipErrorInvalidValue otherwise)
hipError_t launch_wm_infer(const WmInferArgs& a, hipStream_t stream);

// ---- the K models of an ensemble in ONE launch (wm_infer_ens_kernel): each model its own weights, state, halos and constants ----------------------
// The work list is model-major: item = model * n_groups + group, n_groups = ceil(n_col / 128) groups of four 32-column tiles per model, W = K n_groups
// items.  Workgroup b of `grid` walks the contiguous items [b W / grid, (b + 1) W / grid): below the grid size in models a model's groups are shared
// by several workgroups, above it a workgroup walks several models and re-copies the weight image at every model boundary.
inline int wm_ens_groups(int n_col) { return ((n_col + 31) / 32 + 3) / 4; }
__host__ __device__ inline void wm_ens_range(int b, int grid, long long W, long long* first, long long* last) {
    *first = (long long)b * W / grid;
    *last = (long long)(b + 1) * W / grid;
}
// workgroups of the launch: one per item up to one per CU, capped by grid_cap when it is positive (COLNDE_WM_ENS_GRID)
inline int wm_ens_grid(int n_models, int n_col, int n_cu, int grid_cap) {
    const long long W = (long long)n_models * wm_ens_groups(n_col);
    long long g = W < (long long)n_cu ? W : (long long)n_cu;
    if (grid_cap > 0 && g > grid_cap) g = grid_cap;
    return (int)(g < 1 ? 1 : g);
}

struct WmEnsArgs {
    WmEmbedIO io;                         // the d/dz arrays are always written
    int n_models;
    const float* weights;                 // [K][w_stride]: model k's [3 WM_NET] first in its row
    size_t w_stride;
    float mu[6], sigma[6];
    int act1, act2;
    const MppParams* mpp;                 // DEVICE array [K]
    int grid_cap;                         // > 0: at most this many workgroups
};

// every base pointer of the state and the outputs must be 16-byte aligned (hipErrorInvalidValue otherwise)
hipError_t launch_wm_infer_ens(const WmEnsArgs& a, hipStream_t stream);
