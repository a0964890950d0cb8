// mpp_sweep.h — device code of one modified_pacanowski_philander! step of ONE column (wind_mixing/src/NDE_oceananigans.jl:61-101), shared by
// mpp_diffusion_kernel (column_ops.hip) and the fused embedded step (engine_wm_infer.hip): the face diffusivities and the two Thomas sweeps —
// and the same face diffusivities, unscaled, times the face gradients for the flux diagnoses (:157-191, :226-286) of both files.
#pragma once
#include <hip/hip_runtime.h>

struct MppParams { float nu0, nu_minus, inv_dRi, Ric, inv_Pr, galpha_dz, c; int ca; };

// {nu0, nu_minus, dRi, Ric, Pr, alpha, g} of the C ABI, the step and the spacing -> the constants the sweeps use
inline MppParams mpp_params(const float params[7], float dt, float dz, int convective_adjustment) {
    MppParams P;
    P.nu0 = params[0]; P.nu_minus = params[1]; P.inv_dRi = 1.0f / params[2]; P.Ric = params[3]; P.inv_Pr = 1.0f / params[4];
    P.galpha_dz = params[5] * params[6] * dz;       // ∂z b / ((∂z u)² + (∂z v)²) = gα ΔT Δz / (Δu² + Δv²)
    P.c = dt / (dz * dz);
    P.ca = convective_adjustment ? 1 : 0;
    return P;
}

// c·ν and c·νT of face k (1 <= k < Nz) from the level differences across it (du, dv, dT = upper − lower); c = P.c in the sweeps, 1 in the
// diagnoses (ν and νT themselves)
__device__ __forceinline__ void mpp_face(const MppParams& P, float c, float du, float dv, float dT, float& kv, float& kT) {
    const float Ri = P.galpha_dz * dT / (du * du + dv * dv);
    const float x = (Ri - P.Ric) * P.inv_dRi;
    const float nu = P.nu0 + P.nu_minus * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x));
    kv = c * nu;
    kT = P.ca ? (Ri > 0.0f ? kv * P.inv_Pr : c) : kv * P.inv_Pr;
}

// c·νT of an END face (ν = 0 there; :38, :45-55): under convective adjustment from the Richardson number the halo cell gives (absent:
// zero-gradient fill, 0/0 = NaN, `NaN > 0` false: νT = 1 — what the reference computes for a flux-bounded field)
__device__ __forceinline__ float mpp_end_face_kT(const MppParams& P, float c, float du, float dv, float dT) {
    if (!P.ca) return 0.0f;
    const float Ri = P.galpha_dz * dT / (du * du + dv * dv);
    return Ri > 0.0f ? 0.0f : c;
}

// ν ∂z u, ν ∂z v, νT ∂z T on one face, as diagnose_baseline_flux_* / diagnose_NN_flux_* form them (:162, :239, :257, :281): the face
// gradients (φ[f] − φ[f−1])/Δz of the (Center, Center, Face) ComputedFields times the diffusivities above.  end: one of the two end faces.
// Evaluated as written (no contraction): the product is rounded before the caller subtracts it.
__device__ __forceinline__ void mpp_face_nu_grad(const MppParams& P, float dz, bool end, float du, float dv, float dT, float& nu_gu, float& nu_gv,
                                                 float& nuT_gT) {
#pragma clang fp contract(off)
    float nu, nuT;
    mpp_face(P, 1.0f, du, dv, dT, nu, nuT);
    if (end) { nu = 0.0f; nuT = mpp_end_face_kT(P, 1.0f, du, dv, dT); }
    nu_gu = nu * (du / dz);
    nu_gv = nu * (dv / dz);
    nuT_gT = nuT * (dT / dz);
}

// One column in place: tu, tv, tT point at its NZ levels of u, v, T (k = 0 deepest; LDS rows in both callers), c = its index among the n_col
// columns of halo_bottom [3][n_col] (nullable).  The T system goes first: its sweep forms the face diffusivities from the still-unmodified
// u, v and keeps c·ν for the velocity sweep.
template <int NZ>
__device__ __forceinline__ void mpp_column_step(const MppParams& P, float* tu, float* tv, float* tT, const float* __restrict__ halo_bottom,
                                                size_t c, int n_col) {
    float kvs[NZ], cp[NZ];
    // face 0: ν = 0; νT from the halo cells (mpp_end_face_kT)
    float u_lo = tu[0], v_lo = tv[0], T_lo = tT[0];
    const float T_bottom = T_lo;
    float kT_k = 0.0f;
    kvs[0] = 0.0f;
    if (P.ca) {
        const float du = halo_bottom ? u_lo - halo_bottom[c] : 0.0f;
        const float dv = halo_bottom ? v_lo - halo_bottom[(size_t)n_col + c] : 0.0f;
        const float dT = halo_bottom ? T_lo - halo_bottom[2 * (size_t)n_col + c] : 0.0f;
        kT_k = mpp_end_face_kT(P, P.c, du, dv, dT);
    }
    // ---- T system, forming the faces one ahead of the elimination
    float xT = 0.0f;
#pragma unroll
    for (int k = 0; k < NZ; k++) {
        float kT_n = 0.0f;
        const float T_k = T_lo;
        if (k + 1 < NZ) {
            const float u_hi = tu[k + 1], v_hi = tv[k + 1], T_hi = tT[k + 1];
            mpp_face(P, P.c, u_hi - u_lo, v_hi - v_lo, T_hi - T_lo, kvs[k + 1], kT_n);
            u_lo = u_hi; v_lo = v_hi; T_lo = T_hi;
        }
        const float a = -kT_k, b = 1.0f + kT_k + kT_n;
        const float inv = 1.0f / (k == 0 ? b : b - a * cp[k - 1]);
        cp[k] = -kT_n * inv;
        xT = (k == 0 ? T_k : T_k - a * xT) * inv;
        tT[k] = xT;
        kT_k = kT_n;
    }
#pragma unroll
    for (int k = NZ - 2; k >= 0; k--) { xT = tT[k] - cp[k] * xT; tT[k] = xT; }
    tT[0] = T_bottom;
    // ---- velocity system, two right-hand sides
    float xu = 0.0f, xv = 0.0f;
#pragma unroll
    for (int k = 0; k < NZ; k++) {
        const float kn = k + 1 < NZ ? kvs[k + 1] : 0.0f;
        const float a = -kvs[k], b = 1.0f + kvs[k] + kn;
        const float inv = 1.0f / (k == 0 ? b : b - a * cp[k - 1]);
        cp[k] = -kn * inv;
        xu = (k == 0 ? tu[k] : tu[k] - a * xu) * inv;
        xv = (k == 0 ? tv[k] : tv[k] - a * xv) * inv;
        tu[k] = xu; tv[k] = xv;
    }
#pragma unroll
    for (int k = NZ - 2; k >= 0; k--) {
        xu = tu[k] - cp[k] * xu; tu[k] = xu;
        xv = tv[k] - cp[k] * xv; tv[k] = xv;
    }
}
