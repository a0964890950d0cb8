// engine_wm_pretrain.h — host interface of wm_pretrain_ens_kernel: `train_NN` (wind_mixing/src/NN_training.jl:207-249) for the K x 3 flux networks of a
// wind-mixing ensemble in one launch, one workgroup per (model, net) (colnde_ensemble_pretrain_wm_flux_dev).
#pragma once
#include "engine_tile16.h"     // DevModel, pretrain_lds_bytes, PRETRAIN_LDS_CAP
#include "engine_netsplit.h"   // RtPhys

// dynamic LDS of a workgroup: pretrain_kernel's carving, then the net's theta (update: and m, v), each padded to four floats.  (Defined beside the kernel: an
// experimental build of that unit — `make variant STEM=engine_wm_pretrain` — may keep the parameters elsewhere.)
size_t wm_pretrain_lds_bytes(const DevModel& m, int update);

hipError_t wmp_set_kernel_attributes(size_t max_lds_bytes);
// theta, mom, vel [K][3 net_size]; phys [K]; Y [3][n_samples][Nz + 1]; order [K][3][n_samples] or null; eta [K][3]; loss_out [K][3] sums of the per-sample
// losses (entries of nets outside the mask `nets` are not written); bt_out [2] the running powers after the pass
hipError_t launch_wm_pretrain_ens(const DevModel& m, int n_models, int nets, const RtPhys* phys, float* theta, float* mom, float* vel, const float* X,
                                  const float* BC, const float* Y, const int* order, int n_samples, float gs, const float* eta, float b1, float b2, float eps,
                                  double bt1, double bt2, int update, float* loss_out, double* bt_out, hipStream_t stream);
