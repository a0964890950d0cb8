// engine_wm_profile.h — judging a wind-mixing sweep: what NDE_profile (wind_mixing/src/training_postprocessing.jl:250-632) evaluates on every saved
// state of a solve, for the K models of an ensemble in ONE launch (wm_profile_ens_kernel):
//   test_uw, test_vw, test_wT (:404-423): predict_flux (NDE_training.jl:83-147) on state n of simulation c with that simulation's boundary fluxes and,
//       in the diurnal case, the top temperature flux at t = save_times[n] — training RHS, no smoothing (what rt_supported admits), in the three
//       branches: the Pacanowski-Philander closure (eps = 1e-7 on the three gradients, nu / Pr on T, with zero_weights the boundary faces
//       BC - scaling(0)), convective adjustment (kappa min(0, dT/dz)), neither.  Scaled units, as predict_flux returns them.
//   test_Ri (:425-431): local_richardson on D_face u, v, T WITHOUT eps: Bz / S2, Bz = H g alpha sigma_T dT/dz, S2 = (sigma_u du/dz)^2 + (sigma_v dv/dz)^2.
//       D_face has zero first and last rows, so the two boundary faces are 0 / 0 = NaN in the reference; they are written as NaN here too, not repaired
//       (as the embedding's forcing chain keeps the reference's uw[1] quirk, engine_wm_infer.hip).
// The states are rows of sol [K][n_col][n_save][96] in scaled units (a solve's output: there is no input scaling), the constants of the closure are per
// model (RtPhys: rows with nu0 = nu_minus = 0 give the networks' own share of the flux, constants_NN_only :286, :474-495).
#pragma once
#include <hip/hip_runtime.h>
#include "colnde_dev.h"
#include "engine_netsplit.h"
#include "engine_wm_infer.h"

struct WmProfileArgs {
    DevModel m;                           // the handle's model: scalings, closure switches, diurnal forcing (rt_supported)
    int n_models;
    const float* weights;                 // [K][w_stride]: model k's [3 WM_NET] first in its row (unused without flux outputs)
    size_t w_stride;
    const float* sol;                     // [K][n_col][n_save][96], scaled units
    const float* bcs;                     // [n_col][6], shared by the models
    const float* save_times;              // [n_save]
    const RtPhys* phys;                   // DEVICE array [K]
    int n_col, n_save;
    float *uw, *vw, *wT;                  // [K][n_col][n_save][33]: all three or none
    float* Ri;                            // [K][n_col][n_save][33] or null
    int grid_cap;                         // > 0: at most this many workgroups (COLNDE_WM_PROFILE_GRID)
};

// the base pointers of sol and of the outputs must be 16-byte aligned (hipErrorInvalidValue otherwise); a model's rows need no alignment of their own
hipError_t launch_wm_profile_ens(const WmProfileArgs& a, hipStream_t stream);
