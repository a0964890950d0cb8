// engine_fc_pretrain.h — host interface of fc_pretrain_ens_kernel: the T -> wT pre-training of train_free_convection_nde.jl:182-216 for all K networks of a
// free-convection ensemble in one launch, one workgroup per model (colnde_ensemble_pretrain_flux_dev).
#pragma once
#include "engine_tile16.h"   // DevModel, pretrain_lds_bytes, PRETRAIN_LDS_CAP

enum { FCP_ADAM = 0, FCP_DESCENT = 1 };

// The dense part of a model's vector as the kernel reads it.  conv = 0: the plain network `m` itself.  conv = c: the three Dense layers behind the c-tap
// filter inside the user's vector [w (c); b; vec(W1) 4Nz x M; b1; W2; b2; W3; b3], M = Nz - c + 1 — layer 0 takes M inputs at offset c + 1 and every later
// offset moves by (c + 1) - 4Nz (c - 1); ns stays Nz (the profile), n_params becomes the user's count.
static inline DevModel fc_pretrain_dense_model(const DevModel& m, int conv) {
    DevModel d = m;
    if (!conv) return d;
    const int H = m.sizes[1], M = m.Nz - conv + 1, shift = (conv + 1) - H * (conv - 1);
    d.sizes[0] = M;
    for (int l = 0; l < m.n_layers; l++) {
        d.w_off[l] = l == 0 ? conv + 1 : m.w_off[l] + shift;
        d.b_off[l] = m.b_off[l] + shift;
    }
    d.net_size = d.n_params = m.n_params + shift;
    return d;
}

// dynamic LDS: pretrain_kernel's carving of the dense part, plus the filter's M pre-activations, activations and deltas (each padded to four floats)
static inline size_t fc_pretrain_lds_bytes(const DevModel& dense, int conv) {
    const int M = conv ? dense.Nz - conv + 1 : 0;
    return pretrain_lds_bytes(dense) + (size_t)3 * ((M + 3) & ~3) * sizeof(float);
}

hipError_t fcp_set_kernel_attributes(size_t max_lds_bytes);
// theta, mom, vel [K][dense.n_params]; order [K][n_samples] or null; coeff, eta [K] (coeff null: no penalty); loss_out [K] sums of the per-sample losses;
// bt_out [2] the running powers after the pass (written under ADAM with update)
hipError_t launch_fc_pretrain_ens(const DevModel& dense, int conv, int n_models, float* theta, float* mom, float* vel, const float* X, const float* BC,
                                  const float* Y, const int* order, int n_samples, const float* coeff, int optimiser, const float* eta, float b1, float b2,
                                  float eps, double bt1, double bt2, int update, float* loss_out, double* bt_out, hipStream_t stream);
