// column_ops.h — the steps either side of the NDE hot path: the batched implicit convective-adjustment
// step of the ocean embeddings and the on-device ADAM update.
#pragma once
#include <hip/hip_runtime.h>

// T, out: [n_col][Nz] float32 (in place allowed), halo_bottom / halo_top: [n_col] or null.  2 <= Nz <= 128.
hipError_t launch_convective_adjustment(const float* T, const float* halo_bottom, const float* halo_top, float dt_over_dz2, float K,
                                        float* out, int Nz, int n_col, hipStream_t stream);
// modified_pacanowski_philander! (wind_mixing/src/NDE_oceananigans.jl:61-101): u, v, T and the outputs [n_col][Nz] (in place allowed field by
// field), halo_bottom [3][n_col] (u, v, T halo cells below k = 0) or null, params = {nu0, nu_minus, dRi, Ric, Pr, alpha, g}.  2 <= Nz <= 128.
hipError_t launch_mpp_diffusion(const float* u, const float* v, const float* T, const float* halo_bottom, float dt, float dz,
                                const float params[7], int convective_adjustment, float* uo, float* vo, float* To, int Nz, int n_col,
                                hipStream_t stream);
// diagnose_baseline_flux_uw / _vw / _wT (:157-191): uw, vw, wT [n_col][Nz+1] = −ν ∂z u, −ν ∂z v, −νT ∂z T on the faces, the top face replaced by
// top_flux [3][n_col]; halo_bottom, params as above.  The outputs alias nothing.  2 <= Nz <= 128.
hipError_t launch_mpp_diagnose_flux(const float* u, const float* v, const float* T, const float* top_flux, const float* halo_bottom, float dz,
                                    const float params[7], int convective_adjustment, float* uw, float* vw, float* wT, int Nz, int n_col,
                                    hipStream_t stream);
hipError_t launch_adam_step(float* w, const float* grad, float* m, float* v, float eta, float beta1, float beta2, float eps,
                            float beta1_t, float beta2_t, int n, hipStream_t stream);
hipError_t launch_adam_ensemble(float* w, const float* grad, int grad_stride, float* m, float* v, const float* eta, float beta1, float beta2,
                                float eps, float beta1_t, float beta2_t, int n, int n_models, hipStream_t stream);
// data preparation: rows are profiles ([n_rows][N] -> [n_rows][n]); face = 0: block means, 1: linear interpolation keeping the end points
hipError_t launch_coarse_grain(const float* in, int n_rows, int N, int n, int face, float* out, hipStream_t stream);
hipError_t launch_zscore_stats(const float* x, long count, float* out2 /* mu, sigma */, hipStream_t stream);
hipError_t launch_zscore_scale(const float* x, long count, const float* mu_sigma, float* out, hipStream_t stream);
// loss_per_tstep (wind_mixing/src/loss.jl:44-46) for the six profile terms of every column: sol, truth [n_col][n_save][n_var Nz] (n_var = 3 | 1),
// out [n_col][6][n_save] = mse over the Nz levels (terms u, v, T) and over the Nz + 1 faces of the finite-difference gradient, its two zero
// boundary rows included (terms dudz, dvdz, dTdz: loss.jl:9, NDE_training.jl:308-317); T-only models fill terms 2 and 5, the others are 0.
// n_models > 1: sol [K][n_col][n_save][n_var Nz] against the shared truth, out [K][n_col][6][n_save] (the model index in the launch grid; row k holds
// the bits of a K = 1 launch on model k's solution)
hipError_t launch_loss_per_tstep(const float* sol, const float* truth, int n_col, int n_save, int Nz, int n_var, float* out, hipStream_t stream, int n_models = 1);
// out[0] = max over the n_rows rows of rms_i((a_i - b_i) / (floor + |b_i|)) over the `row` floats of a row (+inf if any entry is not finite);
// partial: scratch of >= 1024 floats
hipError_t launch_rel_diff_max(const float* a, const float* b, long n_rows, int row, float floor, float* partial, float* out, hipStream_t stream);
// ... per save point: out[n] (n < n_save) = the maximum over the n_col columns of that norm of rows [column][n_save][row]
hipError_t launch_rel_diff_save_max(const float* a, const float* b, int n_col, int n_save, int row, float floor, float* out, hipStream_t stream);
// ... per member and save point: a, b [K][n_col][n_save][row] (colnde_ensemble_forward_dev's layout), out[k][n] (device, [K][n_save]); K in grid.y,
// at most 65,535; a non-finite entry makes its own (k, n) +inf and no other
hipError_t launch_rel_diff_member_save_max(const float* a, const float* b, int K, int n_col, int n_save, int row, float floor, float* out, hipStream_t stream);
// Free-convection ensembles.  out[k][c][n] = mean over Nz (32 | 64) levels of (sol[k][c][n][:] - truth[c][n][:])^2; rows_per_model = n_col * n_save
hipError_t launch_column_loss(const float* sol, const float* truth, int Nz, long rows_per_model, int n_models, float* out, hipStream_t stream);
// result[k][n_params + 6] += coeff[k] * sum_{r < q} W1_k[r, q]^2, result[k][index of W1[r, q]] += 2 coeff[k] W1_k[r, q] (W1: H x M at w1_off,
// column-major, M <= H — the plain network: 4 Nz x Nz; behind a c-tap filter: 4 Nz x (Nz - c + 1) at c + 1); w [K][n_params], result [K][n_params + 8];
// coeff[k] = 0 leaves row k untouched
hipError_t launch_causal_penalty(const float* w, const float* coeff, float* result, int H, int M, int w1_off, int n_params, int n_models, hipStream_t stream);
// The --conv network (colnde_create_conv; n_models > 1: a conv ensemble, model k's arrays at the given strides, in floats).  theta: the user's vector [w (c); b; W1 (4Nz x M); ...]; padded: the plain network's, W1 as 4Nz x Nz with
// n_zero = 4Nz (c - 1) zeros behind its w1_end = w1_off + 4Nz M entries.
hipError_t launch_fc_conv_pad(const float* theta, int c, int w1_end, int n_zero, int n_pad, float* padded, hipStream_t stream, int n_models = 1,
                              size_t theta_stride = 0);
// The filter's gradient from n_rows (record, column) rows of the conv tape ([x (Nz) | z̄ (Nz)], Nz = 32 | 64): fc_conv_grad_slices(n_rows) rows of
// FC_CONV_GRAD_SLOTS floats at slab_rows (slot d: d/dw[c - d], the last slot: d/db), every sum in a fixed order
#define FC_CONV_GRAD_SLOTS 9
#define FC_CONV_GRAD_MAX_SLICES 256
int fc_conv_grad_slices(long n_rows);
hipError_t launch_fc_conv_grad(const float* ctape, long n_rows, int Nz, int c, float* slab_rows, hipStream_t stream, int n_models = 1, size_t ctape_stride = 0,
                               size_t slab_stride = 0);
// out [n_out = user parameters + 8]: the filter entries summed over the n_rows rows of the filter slab, then gpad [padded + 8] without W1's padded columns
hipError_t launch_fc_conv_fold(const float* gpad, const float* cslab, int n_rows, int c, int w1_end, int n_zero, int n_out, float* out, hipStream_t stream,
                               int n_models = 1, size_t gpad_stride = 0, size_t cslab_stride = 0);
