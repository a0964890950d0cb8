// engine_netsplit.h — the net-split kernels of the static wind-mixing shape: one wavefront per flux net (plus a helper wavefront) per 16-column tile,
// for problems too small for regtile's wave tiles (engine AUTO up to 8,192 columns) and for ensembles.  Weight images and their layout: engine_regtile.h.
#pragma once
#include "engine_regtile.h"

// Ensembles (colnde_create_ensemble): K models of this shape in ONE launch per kernel, the model index in blockIdx.y.  A model owns its packed
// weight image, solution, tapes and slab rows (per-model strides in floats below) and its Pacanowski-Philander constants; x0, bcs and truth are
// shared.  A single model launches with grid.y = 1 and phys = nullptr: the constants of DevModel, every offset zero.
struct RtPhys { float nu0, nu_minus, Ric, inv_dRi, inv_Pr, c_rib, pad0, pad1; };
struct RtEns {
    const RtPhys* phys = nullptr;        // [n_models] closure constants, or nullptr
    size_t wimg = 0, sol = 0, tape = 0, ztape = 0, dwtape = 0, slab = 0;
    int n_models = 1;
};

hipError_t rt_set_attributes_split();   // the dynamic-LDS limit of every kernel of this unit (beside rt_set_attributes)
// sched != nullptr (device, int[n_save - 1]; colnde_set_schedule): save interval n takes sched[n] RK4 steps instead of `substeps`, the tapes hold
// total_steps = their sum per tile — the four-wave RK4 kernels only (rt16sh_forward_sched_kernel / rt16sh_adjoint_sched_kernel), anything else is refused
hipError_t rt_launch_forward_split(const DevModel& m, const float* wimg, const float* x0, const float* bcs, const float* save_times,
                                   int n_save, int substeps, float* sol, float* t16_tape, float* t16_ztape, int n_col, bool rich, bool use_helper, bool want_split, hipStream_t stream,
                                   const RtEns& ens = RtEns(), const int* sched = nullptr, int total_steps = 0);
size_t rt_split_rich_record_floats();   // floats per (tile, step, stage) of the net-split kernels' rich tape (which then takes the place of t16_ztape)
// member_lw / member_colw (device, [n_models] and [n_models][n_col]; colnde_ensemble_set_member_loss): both given, lw is not read — model k is
// differentiated under member_lw[k] with column c weighted by member_colw[k][c] (rt16sh_adjoint_member_kernel and its scheduled twin: the four-wave
// kernels only)
hipError_t rt_launch_adjoint_split(const DevModel& m, const float* wimg, const float* save_times, int n_save, int substeps, const float* sol,
                                   const float* truth, const float* t16_tape, const float* t16_ztape, const LossWeights& lw, float* slab,
                                   int n_col, float* dwtape, bool rich, bool use_helper, bool want_split, hipStream_t stream,
                                   const RtEns& ens = RtEns(), const int* sched = nullptr, int total_steps = 0,
                                   const LossWeights* member_lw = nullptr, const float* member_colw = nullptr);
bool rt_adjoint_split_has_bf16(const DevModel& m, bool use_helper);   // the net-split adjoint has a split (bf16-pipe) kernel for this configuration
hipError_t rt_debug_read_stamps_split(unsigned long long* out16);   // diagnostic builds (-DCOLNDE_STAMPS): the phase stamps of this unit's kernels
