// engine_closure.h — the closure-only column model: the modified Pacanowski-Philander closure without networks, K constant sets side by side.
// (DE(x, p, t) and its loss: wind_mixing/src/diffusivity_parameter_optimisation.jl:1-33, :150-163.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "engine_dwgemm.h"   // LossWeights

#define CLOSURE_N_PARAMS 5   // nu0, nu_minus, dRi, Ric, Pr (mpp_parameters order)
#define CLOSURE_ROW 16       // floats per (set, column) partial row: 5 sensitivities, 6 raw loss sums, padding
#define CLOSURE_MAX_NZ 64    // a lane per level

struct ClosureModel {
    int Nz, n_save, substeps, n_col, n_sets;
    float cs[3], A[3], s0[3], B, cor_u, cor_v, sig_u, sig_v, mu_u, mu_v, eps;
};

// floats of the step-start tape of ONE set: [n_col][n_steps][3 Nz]
size_t closure_tape_floats(const ClosureModel& m);

// Forward solve of every (set, column): sol [K][n_col][n_save][3 Nz].  tape (nullable): the state at the start of every RK4 step.
// truth + rows (nullable together): the six raw loss sums of every (set, column) into rows[..][5..10].
hipError_t closure_launch_forward(const ClosureModel& m, const float* params, const float* x0, const float* bcs, const float* times, float* sol,
                                  float* tape, const float* truth, float* rows, hipStream_t stream);
// Discrete adjoint of that solve: the five sensitivities of every (set, column) into rows[..][0..4].
hipError_t closure_launch_adjoint(const ClosureModel& m, const float* params, const float* bcs, const float* times, const float* sol,
                                  const float* truth, const float* tape, const LossWeights& lw, float* rows, hipStream_t stream);
// Fixed-order sum over the columns of each set.  with_grad: out [K][13] = [5 sensitivities; 6 scaled terms; total; 0]; else out [K][8].
hipError_t closure_launch_reduce(const ClosureModel& m, const float* rows, const LossWeights& lw, bool with_grad, float* out, hipStream_t stream);
