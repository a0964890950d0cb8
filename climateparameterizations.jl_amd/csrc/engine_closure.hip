// engine_closure.hip — the modified Pacanowski-Philander closure WITHOUT networks: forward solve, discrete adjoint with respect to the five
// constants (nu0, nu_minus, dRi, Ric, Pr) and the column reduction, for K constant sets side by side.  gfx950 only.
//
// Replaces DE(x, p, t) and loss_mpp of wind_mixing/src/diffusivity_parameter_optimisation.jl:1-33, :150-163: the wind-mixing RHS with
// modified_pacanowski_philander = zero_weights = 1 and all network outputs zero (oracle/nde_oracle.py Model.wm_rhs at theta = 0).
//
// Mapping: one wavefront per (set, column), a lane per level (Nz <= 64), four wavefronts per workgroup, the flat (set, column) index in the grid.
// There is no matrix product anywhere: a right-hand side is ~60 VALU operations per lane, and the only data that crosses lanes is the neighbour
// level of a face difference (state below) and of a flux divergence (face above).  Both are DPP wave shifts by one lane (no LDS, no ds_bpermute).
// Lane k owns cell k and face k (the face below it); face 0 is the bottom boundary, face Nz the top one (handled by lane Nz - 1).
//
// Tape: the forward kernel writes the state at the START of every RK4 step ([set][col][step][3 Nz]); the adjoint recomputes the four stage inputs
// of a step from it in registers (three more right-hand sides) rather than reading four taped stages: 3 Nz floats per step instead of 12 Nz,
// and the recomputation is cheaper than the loads it saves.
#include "engine_closure.h"

namespace {

constexpr int WPB = 4;   // wavefronts (= columns) per workgroup

// value of lane - 1 (0 into lane 0) / of lane + 1 (0 into lane 63): DPP wave_shr:1 / wave_shl:1, all 64 lanes must be active
__device__ __forceinline__ float lane_below(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float lane_above(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x130, 0xf, 0xf, true));
}

struct Col { float u, v, T; };
struct Phys { float nu0, nu_minus, inv_dRi, Ric, inv_Pr; };
struct Bcs { float b[3], t[3]; };   // bottom / top boundary fluxes minus scaling(0), per variable
// the closure on face k (zeros outside the interior faces): gradients, shear, Richardson number, y = (Ri - Ric) / dRi,
// e = exp(2 y), h = (1 - tanh y) / 2 = 1 / (1 + e), nu = nu0 + nu_minus h
struct Face { float gu, gv, gT, S2, Ri, y, e, h, nu; };

__device__ __forceinline__ Phys load_phys(const float* __restrict__ p) {
    Phys ph;
    ph.nu0 = p[0]; ph.nu_minus = p[1]; ph.inv_dRi = 1.0f / p[2]; ph.Ric = p[3]; ph.inv_Pr = 1.0f / p[4];
    return ph;
}

__device__ __forceinline__ Face closure_face(const ClosureModel& m, const Phys& ph, const Col& x, bool in) {
    Face g;
    const float Nzf = (float)m.Nz;
    const float ub = lane_below(x.u), vb = lane_below(x.v), Tb = lane_below(x.T);
    g.gu = in ? (x.u - ub) * Nzf : 0.0f;
    g.gv = in ? (x.v - vb) * Nzf : 0.0f;
    g.gT = in ? (x.T - Tb) * Nzf : 0.0f;
    const float a1 = m.sig_u * (g.gu + m.eps), a2 = m.sig_v * (g.gv + m.eps);
    g.S2 = a1 * a1 + a2 * a2;
    g.Ri = fast_div(m.B * (g.gT + m.eps), g.S2);               // local_richardson, NDE_training.jl:46-52
    g.y = (g.Ri - ph.Ric) * ph.inv_dRi;
    g.e = __expf(2.0f * fminf(fmaxf(g.y, -15.0f), 15.0f));
    g.h = __builtin_amdgcn_rcpf(1.0f + g.e);                    // tanh_step (:54) without the cancellation of 1 - tanh
    g.nu = ph.nu0 + ph.nu_minus * g.h;
    return g;
}

// DE(x, p, t): diffusivity_parameter_optimisation.jl:1-33
__device__ __forceinline__ Col closure_rhs(const ClosureModel& m, const Phys& ph, const Bcs& bc, const Col& x, int k) {
    const bool in = k >= 1 && k < m.Nz, bottom = k == 0, top = k == m.Nz - 1;
    const Face g = closure_face(m, ph, x, in);
    const float F0 = in ? -m.cs[0] * g.nu * g.gu : (bottom ? bc.b[0] : 0.0f);
    const float F1 = in ? -m.cs[1] * g.nu * g.gv : (bottom ? bc.b[1] : 0.0f);
    const float F2 = in ? -m.cs[2] * (g.nu * ph.inv_Pr) * g.gT : (bottom ? bc.b[2] : 0.0f);
    float U0 = lane_above(F0), U1 = lane_above(F1), U2 = lane_above(F2);
    if (top) { U0 = bc.t[0]; U1 = bc.t[1]; U2 = bc.t[2]; }
    Col d;
    d.u = -m.A[0] * (U0 - F0) + m.cor_u * (m.sig_v * x.v + m.mu_v);
    d.v = -m.A[1] * (U1 - F1) - m.cor_v * (m.sig_u * x.u + m.mu_u);
    d.T = -m.A[2] * (U2 - F2);
    if (k >= m.Nz) { d.u = 0.0f; d.v = 0.0f; d.T = 0.0f; }
    return d;
}

// Pullback of closure_rhs at x for the cotangent db of its result: returns the cotangent of x and adds this lane's share of the five parameter
// sensitivities to acc (oracle/nde_oracle.py Model.wm_rhs vjp, plus the parameter cotangents: nu-bar feeds nu0, nu_minus and, through
// y = (Ri - Ric) / dRi, Ric and dRi; the T flux feeds Pr).
__device__ __forceinline__ Col closure_vjp(const ClosureModel& m, const Phys& ph, const Col& x, const Col& db, int k, float acc[CLOSURE_N_PARAMS]) {
    const bool in = k >= 1 && k < m.Nz;
    const Face g = closure_face(m, ph, x, in);
    const float Nzf = (float)m.Nz;
    const float dub = lane_below(db.u), dvb = lane_below(db.v), dTb = lane_below(db.T);
    // D-bar = -F-bar on the interior faces, times the flux coefficients
    const float c0 = in ? -m.A[0] * (db.u - dub) * m.cs[0] : 0.0f;
    const float c1 = in ? -m.A[1] * (db.v - dvb) * m.cs[1] : 0.0f;
    const float c2 = in ? -m.A[2] * (db.T - dTb) * m.cs[2] * ph.inv_Pr : 0.0f;
    float gub = c0 * g.nu, gvb = c1 * g.nu, gTb = c2 * g.nu;
    const float nub = c0 * g.gu + c1 * g.gv + c2 * g.gT;
    // 1 - tanh^2 y = 4 e / (1 + e)^2 holds while e = exp(2 y): inside closure_face's clamp.  Beyond it e stays at exp(+-30) and the formula at
    // 3.7e-13 however large |y| grows, while y, Ri and 1 / S2 below are the unclamped values: a face at rest (u = v = 0: S2 = 2 (sigma eps)^2 =
    // 5e-17, |Ri| ~ 1e15) would put 3e3 on dRi-bar and 3e10 on the state cotangent where the derivative is 0.  There sech^2 |y| < 6e-12: the face
    // is saturated, Ri-bar is exactly 0 and none of its products is formed (0 * Inf included).
    const bool live = !(fabsf(g.y) >= 15.0f);                                      // (a NaN y stays live: it must reach the result)
    const float sech2 = 4.0f * g.e * g.h * g.h;
    const float rib = nub * (-0.5f * ph.nu_minus) * sech2 * ph.inv_dRi;           // Ri-bar
    if (in) {
        acc[0] += nub;
        acc[1] += nub * g.h;
        acc[4] -= c2 * g.nu * g.gT * ph.inv_Pr;
    }
    if (in && live) {
        acc[2] -= rib * g.y;
        acc[3] -= rib;
        gTb += fast_div(rib * m.B, g.S2);
        const float q = fast_div(rib * -g.Ri, g.S2) * 2.0f;
        gub += q * m.sig_u * m.sig_u * (g.gu + m.eps);
        gvb += q * m.sig_v * m.sig_v * (g.gv + m.eps);
    }
    const float gua = lane_above(gub), gva = lane_above(gvb), gTa = lane_above(gTb);   // (zero from lane Nz: not an interior face)
    Col xb;
    xb.u = Nzf * (gub - gua) - m.cor_v * m.sig_u * db.v;
    xb.v = Nzf * (gvb - gva) + m.cor_u * m.sig_v * db.u;
    xb.T = Nzf * (gTb - gTa);
    if (k >= m.Nz) { xb.u = 0.0f; xb.v = 0.0f; xb.T = 0.0f; }
    return xb;
}

__device__ __forceinline__ Col axpy(const Col& x, float a, const Col& k) { return Col{fmaf(a, k.u, x.u), fmaf(a, k.v, x.v), fmaf(a, k.T, x.T)}; }

__device__ __forceinline__ Col load_col(const float* __restrict__ p, int Nz, int k) {
    Col x{0.0f, 0.0f, 0.0f};
    if (k < Nz) { x.u = p[k]; x.v = p[Nz + k]; x.T = p[2 * Nz + k]; }
    return x;
}
__device__ __forceinline__ void store_col(float* __restrict__ p, int Nz, int k, const Col& x) {
    if (k < Nz) { p[k] = x.u; p[Nz + k] = x.v; p[2 * Nz + k] = x.T; }
}

__device__ __forceinline__ Bcs load_bcs(const ClosureModel& m, const float* __restrict__ bc) {
    Bcs b;
#pragma unroll
    for (int q = 0; q < 3; q++) { b.b[q] = bc[2 * q] - m.s0[q]; b.t[q] = bc[2 * q + 1] - m.s0[q]; }   // -(BC - scaling(0)) enters through the divergence
    return b;
}

// one save point of the loss: raw sums of squares of the profile and face-gradient differences (loss.jl:1-9), and, with INJECT, the
// cotangent the loss hands the state there (oracle _loss_injection)
template <bool INJECT>
__device__ __forceinline__ void loss_point(const ClosureModel& m, const Col& x, const Col& tr, int k, const LossWeights& lw, float sums[6], Col* lam) {
    const bool in = k >= 1 && k < m.Nz;
    const float Nzf = (float)m.Nz;
    const float d[3] = {x.u - tr.u, x.v - tr.v, x.T - tr.T};
    float inj[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const float db = lane_below(d[q]);
        const float g = in ? (d[q] - db) * Nzf : 0.0f;
        if (!INJECT) {
            sums[q] += d[q] * d[q];
            sums[3 + q] += g * g;
        } else {
            const float ga = lane_above(g);
            inj[q] = 2.0f * lw.w[q] * d[q] + 2.0f * lw.w[3 + q] * Nzf * (g - ga);
        }
    }
    if (INJECT && k < m.Nz) { lam->u += inj[0]; lam->v += inj[1]; lam->T += inj[2]; }
}

// sum over the 64 lanes in a fixed butterfly order: every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool TAPE, bool LOSS>
__global__ void __launch_bounds__(64 * WPB) closure_forward_kernel(ClosureModel m, const float* __restrict__ params, const float* __restrict__ x0,
                                                                   const float* __restrict__ bcs, const float* __restrict__ times,
                                                                   float* __restrict__ sol, float* __restrict__ tape,
                                                                   const float* __restrict__ truth, float* __restrict__ rows) {
    const int k = threadIdx.x & 63;
    const long item = (long)blockIdx.x * WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (item >= (long)m.n_sets * m.n_col) return;          // wave-uniform
    const int set = (int)(item / m.n_col), col = (int)(item - (long)set * m.n_col);
    const int Nz = m.Nz, ns = 3 * Nz;
    const Phys ph = load_phys(params + (size_t)set * CLOSURE_N_PARAMS);
    const Bcs bc = load_bcs(m, bcs + (size_t)col * 6);
    float* so = sol + (size_t)item * m.n_save * ns;
    const float* tr = LOSS ? truth + (size_t)col * m.n_save * ns : nullptr;
    float* tp = TAPE ? tape + (size_t)item * (m.n_save - 1) * m.substeps * ns : nullptr;
    const LossWeights lw0{};
    float sums[6] = {0, 0, 0, 0, 0, 0};
    Col x = load_col(x0 + (size_t)col * ns, Nz, k);
    store_col(so, Nz, k, x);
    if (LOSS) loss_point<false>(m, x, load_col(tr, Nz, k), k, lw0, sums, nullptr);
    for (int i = 1; i < m.n_save; i++) {
        const float dt = (times[i] - times[i - 1]) / (float)m.substeps;
        for (int s = 0; s < m.substeps; s++) {
            if (TAPE) { store_col(tp, Nz, k, x); tp += ns; }
            const Col k1 = closure_rhs(m, ph, bc, x, k);
            const Col k2 = closure_rhs(m, ph, bc, axpy(x, 0.5f * dt, k1), k);
            const Col k3 = closure_rhs(m, ph, bc, axpy(x, 0.5f * dt, k2), k);
            const Col k4 = closure_rhs(m, ph, bc, axpy(x, dt, k3), k);
            const float w = dt * (1.0f / 6.0f);
            x.u += w * (k1.u + 2.0f * k2.u + 2.0f * k3.u + k4.u);
            x.v += w * (k1.v + 2.0f * k2.v + 2.0f * k3.v + k4.v);
            x.T += w * (k1.T + 2.0f * k2.T + 2.0f * k3.T + k4.T);
        }
        store_col(so + (size_t)i * ns, Nz, k, x);
        if (LOSS) loss_point<false>(m, x, load_col(tr + (size_t)i * ns, Nz, k), k, lw0, sums, nullptr);
    }
    if (LOSS) {
        float tot[6];
#pragma unroll
        for (int q = 0; q < 6; q++) tot[q] = wave_sum(sums[q]);
        float* r = rows + (size_t)item * CLOSURE_ROW;
        if (k >= 5 && k < CLOSURE_ROW) {
            float v = 0.0f;
#pragma unroll
            for (int q = 0; q < 6; q++) if (k == 5 + q) v = tot[q];
            r[k] = v;
        }
    }
}

__global__ void __launch_bounds__(64 * WPB) closure_adjoint_kernel(ClosureModel m, const float* __restrict__ params, const float* __restrict__ bcs,
                                                                   const float* __restrict__ times, const float* __restrict__ sol,
                                                                   const float* __restrict__ truth, const float* __restrict__ tape, LossWeights lw,
                                                                   float* __restrict__ rows) {
    const int k = threadIdx.x & 63;
    const long item = (long)blockIdx.x * WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (item >= (long)m.n_sets * m.n_col) return;          // wave-uniform
    const int set = (int)(item / m.n_col), col = (int)(item - (long)set * m.n_col);
    const int Nz = m.Nz, ns = 3 * Nz;
    const Phys ph = load_phys(params + (size_t)set * CLOSURE_N_PARAMS);
    const Bcs bc = load_bcs(m, bcs + (size_t)col * 6);
    const float* so = sol + (size_t)item * m.n_save * ns;
    const float* tr = truth + (size_t)col * m.n_save * ns;
    const float* tp = tape + (size_t)item * (m.n_save - 1) * m.substeps * ns;
    float acc[CLOSURE_N_PARAMS] = {0, 0, 0, 0, 0};
    Col lam{0.0f, 0.0f, 0.0f};
    for (int i = m.n_save - 1; i >= 1; i--) {
        loss_point<true>(m, load_col(so + (size_t)i * ns, Nz, k), load_col(tr + (size_t)i * ns, Nz, k), k, lw, nullptr, &lam);
        const float dt = (times[i] - times[i - 1]) / (float)m.substeps;
        for (int s = m.substeps - 1; s >= 0; s--) {
            const Col x = load_col(tp + ((size_t)(i - 1) * m.substeps + s) * ns, Nz, k);
            const Col k1 = closure_rhs(m, ph, bc, x, k);
            const Col X2 = axpy(x, 0.5f * dt, k1);
            const Col k2 = closure_rhs(m, ph, bc, X2, k);
            const Col X3 = axpy(x, 0.5f * dt, k2);
            const Col k3 = closure_rhs(m, ph, bc, X3, k);
            const Col X4 = axpy(x, dt, k3);
            const float w6 = dt * (1.0f / 6.0f), w3 = dt * (1.0f / 3.0f);
            const Col k4b{w6 * lam.u, w6 * lam.v, w6 * lam.T};
            const Col x4b = closure_vjp(m, ph, X4, k4b, k, acc);
            const Col k3b{fmaf(dt, x4b.u, w3 * lam.u), fmaf(dt, x4b.v, w3 * lam.v), fmaf(dt, x4b.T, w3 * lam.T)};
            const Col x3b = closure_vjp(m, ph, X3, k3b, k, acc);
            const Col k2b{fmaf(0.5f * dt, x3b.u, w3 * lam.u), fmaf(0.5f * dt, x3b.v, w3 * lam.v), fmaf(0.5f * dt, x3b.T, w3 * lam.T)};
            const Col x2b = closure_vjp(m, ph, X2, k2b, k, acc);
            const Col k1b{fmaf(0.5f * dt, x2b.u, w6 * lam.u), fmaf(0.5f * dt, x2b.v, w6 * lam.v), fmaf(0.5f * dt, x2b.T, w6 * lam.T)};
            const Col x1b = closure_vjp(m, ph, x, k1b, k, acc);
            lam.u += (x1b.u + x2b.u) + (x3b.u + x4b.u);
            lam.v += (x1b.v + x2b.v) + (x3b.v + x4b.v);
            lam.T += (x1b.T + x2b.T) + (x3b.T + x4b.T);
        }
    }
    float tot[CLOSURE_N_PARAMS];
#pragma unroll
    for (int q = 0; q < CLOSURE_N_PARAMS; q++) tot[q] = wave_sum(acc[q]);
    float* r = rows + (size_t)item * CLOSURE_ROW;
    if (k < CLOSURE_N_PARAMS) {
        float v = 0.0f;
#pragma unroll
        for (int q = 0; q < CLOSURE_N_PARAMS; q++) if (k == q) v = tot[q];
        r[k] = v;
    }
}

// out[set] = sum over the set's columns of its rows, in an order that depends on the column count alone: four row lanes take columns
// c = ry, ry + 4, ..., and their partial sums are added as ((p0 + p1) + p2) + p3.  No atomics.
__global__ void __launch_bounds__(64) closure_reduce_kernel(ClosureModel m, const float* __restrict__ rows, LossWeights lw, int with_grad,
                                                            float* __restrict__ out) {
    const int set = blockIdx.x, px = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const float* r = rows + (size_t)set * m.n_col * CLOSURE_ROW;
    float s = 0.0f;
    for (int c = ry; c < m.n_col; c += 4) s += r[(size_t)c * CLOSURE_ROW + px];
    const float p0 = __shfl(s, px), p1 = __shfl(s, 16 + px), p2 = __shfl(s, 32 + px), p3 = __shfl(s, 48 + px);
    float tot = ((p0 + p1) + p2) + p3;
    if (px >= 5 && px < 11) tot *= lw.w[px - 5];
    float total = 0.0f;
#pragma unroll
    for (int q = 0; q < 6; q++) total += __shfl(tot, 5 + q);
    if (threadIdx.x < 16) {
        float* o = out + (size_t)set * (with_grad ? CLOSURE_N_PARAMS + 8 : 8);
        const int p = px;
        if (with_grad && p < 5) o[p] = tot;
        const int base = with_grad ? 0 : -5;
        if (p >= 5 && p < 11) o[base + p] = tot;
        if (p == 11) o[base + 11] = total;
        if (p == 12) o[base + 12] = 0.0f;
    }
}

}  // namespace

size_t closure_tape_floats(const ClosureModel& m) { return (size_t)m.n_col * (m.n_save - 1) * m.substeps * 3 * m.Nz; }

static unsigned closure_grid(const ClosureModel& m) { return (unsigned)(((long)m.n_sets * m.n_col + WPB - 1) / WPB); }

hipError_t closure_launch_forward(const ClosureModel& m, const float* params, const float* x0, const float* bcs, const float* times, float* sol,
                                  float* tape, const float* truth, float* rows, hipStream_t stream) {
    if (m.Nz < 4 || m.Nz > CLOSURE_MAX_NZ || (long)m.n_sets * m.n_col > 0x7fffffffL * WPB) return hipErrorInvalidValue;
    if ((truth == nullptr) != (rows == nullptr)) return hipErrorInvalidValue;
    const dim3 grid(closure_grid(m)), block(64 * WPB);
    auto k = tape ? (truth ? closure_forward_kernel<true, true> : closure_forward_kernel<true, false>)
                  : (truth ? closure_forward_kernel<false, true> : closure_forward_kernel<false, false>);
    hipLaunchKernelGGL(k, grid, block, 0, stream, m, params, x0, bcs, times, sol, tape, truth, rows);
    return hipGetLastError();
}

hipError_t closure_launch_adjoint(const ClosureModel& m, const float* params, const float* bcs, const float* times, const float* sol,
                                  const float* truth, const float* tape, const LossWeights& lw, float* rows, hipStream_t stream) {
    if (m.Nz < 4 || m.Nz > CLOSURE_MAX_NZ || !tape || !truth || !rows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(closure_adjoint_kernel, dim3(closure_grid(m)), dim3(64 * WPB), 0, stream, m, params, bcs, times, sol, truth, tape, lw, rows);
    return hipGetLastError();
}

hipError_t closure_launch_reduce(const ClosureModel& m, const float* rows, const LossWeights& lw, bool with_grad, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(closure_reduce_kernel, dim3(m.n_sets), dim3(64), 0, stream, m, rows, lw, with_grad ? 1 : 0, out);
    return hipGetLastError();
}
