// column_ops.hip — gfx950 kernels for the steps either side of the NDE hot path.
#include "column_ops.h"
#include "mpp_sweep.h"

// ------------------------------------------------------------------------------------------------
// convective_adjustment!(model, Δt, K): free_convection/double_gyre_nn.jl:27-62 (3-D), free_convection/src/oceananigans_nn.jl:13-40
// (1-D).  Per column: the centred vertical gradient (zero-gradient halos) marks the statically unstable cells,
// κ_k = K there and 0 elsewhere, and T' = L \ T with the reference's tridiagonal
//     lower_k = -c κ_k (k >= 1),  diag_k = 1 + c (κ_k + κ_{k+1}) (k < Nz-1),  diag_{Nz-1} = 1 + c κ_{Nz-1},  upper_k = -c κ_{k+1},
// c = Δt/Δz².  L is strictly diagonally dominant by rows and columns, so the reference's pivoted LU (`Tridiagonal \`)
// never pivots and the Thomas recurrence below is the same elimination.
//
// HBM-bound (2·4·Nz bytes per column, ~8 flop per level).  A workgroup stages its columns through LDS with coalesced float4 traffic
// (rows padded to NZ+1 floats: conflict-free per-thread column walks), one thread solves one column.
// ------------------------------------------------------------------------------------------------
// Round 3: ONE WAVE per workgroup (64 columns, 8.4 KB of LDS at Nz = 32) instead of four — what took the three-field kernel below to 70 % of the
// HBM peak: many small workgroups per CU are in different phases, one's solve hides under the others' float4 traffic (256-thread workgroups: 4.6–4.9 TB/s).
template <int NZ>
__global__ void __launch_bounds__(64) convadj_kernel(const float* T, const float* __restrict__ halo_bottom,
                                                     const float* __restrict__ halo_top, float c, float K, float* out, int n_col) {
    extern __shared__ float cs_smem[];
    constexpr int LD = NZ + 1, Q = NZ / 4;
    const int lane = threadIdx.x;
    const int col0 = blockIdx.x * 64;
    const int ncol = min(64, n_col - col0);
    typedef float ca_f32x4 __attribute__((ext_vector_type(4)));
    const ca_f32x4* src = reinterpret_cast<const ca_f32x4*>(T + (size_t)col0 * NZ);
    if (ncol == 64) {
        ca_f32x4 r[Q];
#pragma unroll
        for (int i = 0; i < Q; i++) r[i] = __builtin_nontemporal_load(src + i * 64 + lane);
#pragma unroll
        for (int i = 0; i < Q; i++) {
            const int e = i * 64 + lane, cl = e / Q, k = (e % Q) * 4;
            float* d = cs_smem + cl * LD + k;
            d[0] = r[i].x; d[1] = r[i].y; d[2] = r[i].z; d[3] = r[i].w;
        }
    } else {
        for (int e = lane; e < ncol * Q; e += 64) {
            const ca_f32x4 v = src[e];
            const int cl = e / Q, k = (e % Q) * 4;
            float* d = cs_smem + cl * LD + k;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    }
    __syncthreads();
    if (lane < ncol) {
        float* t = cs_smem + lane * LD;
        const int ca_i = col0 + lane;
#include "convadj_sweep.inc"
    }
    __syncthreads();
    ca_f32x4* dst = reinterpret_cast<ca_f32x4*>(out + (size_t)col0 * NZ);
    if (ncol == 64) {
#pragma unroll
        for (int i = 0; i < Q; i++) {
            const int e = i * 64 + lane, cl = e / Q, k = (e % Q) * 4;
            const float* d = cs_smem + cl * LD + k;
            const ca_f32x4 q = {d[0], d[1], d[2], d[3]};
            __builtin_nontemporal_store(q, dst + e);
        }
    } else {
        for (int e = lane; e < ncol * Q; e += 64) {
            const int cl = e / Q, k = (e % Q) * 4;
            const float* d = cs_smem + cl * LD + k;
            const ca_f32x4 q = {d[0], d[1], d[2], d[3]};
            dst[e] = q;
        }
    }
}

// any Nz <= 128 (not a multiple of 4, unaligned pointers, or none of the instantiated sizes): one thread per column straight from HBM
// (T and out carry no __restrict__: out may be T itself, in place, as in convadj_kernel)
__global__ void __launch_bounds__(256) convadj_generic_kernel(const float* T, const float* __restrict__ halo_bottom,
                                                               const float* __restrict__ halo_top, float c, float K,
                                                               float* out, int Nz, int n_col) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= n_col) return;
    const float* t = T + (size_t)col * Nz;
    float* o = out + (size_t)col * Nz;
    float x[128], cp[128], kk[128];
    for (int k = 0; k < Nz; k++) x[k] = t[k];
    const float ck = c * K;
    const float below = halo_bottom ? halo_bottom[col] : x[0], above = halo_top ? halo_top[col] : x[Nz - 1];
    for (int k = 0; k < Nz; k++) kk[k] = ((k + 1 < Nz ? x[k + 1] : above) - (k > 0 ? x[k - 1] : below)) < 0.0f ? ck : 0.0f;
    float inv = 1.0f / (1.0f + kk[0] + (Nz > 1 ? kk[1] : 0.0f));
    cp[0] = (Nz > 1 ? -kk[1] : 0.0f) * inv;
    x[0] *= inv;
    for (int k = 1; k < Nz; k++) {
        const float a = -kk[k];
        const float b = 1.0f + kk[k] + (k < Nz - 1 ? kk[k + 1] : 0.0f);
        inv = 1.0f / (b - a * cp[k - 1]);
        cp[k] = (k < Nz - 1 ? -kk[k + 1] : 0.0f) * inv;
        x[k] = (x[k] - a * x[k - 1]) * inv;
    }
    for (int k = Nz - 2; k >= 0; k--) x[k] -= cp[k] * x[k + 1];
    for (int k = 0; k < Nz; k++) o[k] = x[k];
}

hipError_t launch_convective_adjustment(const float* T, const float* halo_bottom, const float* halo_top, float c, float K, float* out,
                                        int Nz, int n_col, hipStream_t stream) {
    if (Nz < 2 || Nz > 128 || n_col < 1) return hipErrorInvalidValue;
    const dim3 grid((n_col + 63) / 64), block(64);
#define CA_LAUNCH(N) hipLaunchKernelGGL(convadj_kernel<N>, grid, block, 64 * (N + 1) * sizeof(float), stream, T, halo_bottom, halo_top, c, K, out, n_col)
    const bool aligned = (((uintptr_t)T | (uintptr_t)out) & 15) == 0;
    if (aligned && Nz == 16) CA_LAUNCH(16);
    else if (aligned && Nz == 32) CA_LAUNCH(32);
    else if (aligned && Nz == 64) CA_LAUNCH(64);
    else hipLaunchKernelGGL(convadj_generic_kernel, dim3((n_col + 255) / 256), dim3(256), 0, stream, T, halo_bottom, halo_top, c, K, out, Nz, n_col);
#undef CA_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Flux.Optimise.ADAM `apply!` followed by `update!` (Flux 0.11.6, src/optimise/optimisers.jl; call sites
// wind_mixing/src/NDE_training.jl:340-372, free_convection/src/training.jl:71): one fused pass over the parameter vector.
// beta1_t / beta2_t are the running powers β₁ᵗ, β₂ᵗ the optimiser state carries (β on the first step).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, float eta, float b1, float b2, float eps, float c1, float c2,
                                                    int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    w[i] -= mi * c1 / (sqrtf(vi * c2) + eps) * eta;      // c1 = 1/(1-β₁ᵗ), c2 = 1/(1-β₂ᵗ)
}

hipError_t launch_adam_step(float* w, const float* grad, float* m, float* v, float eta, float beta1, float beta2, float eps,
                            float beta1_t, float beta2_t, int n, hipStream_t stream) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, w, grad, m, v, eta, beta1, beta2, eps,
                       1.0f / (1.0f - beta1_t), 1.0f / (1.0f - beta2_t), n);
    return hipGetLastError();
}

// The same update for an ensemble of K models in one launch (blockIdx.y = model): weights, moments [K][n], the gradient read at
// stride g_stride straight from the result buffer of colnde_ensemble_loss_grad_dev ([K][n + 8]: gradient first), eta[K] per model.
__global__ void __launch_bounds__(256) adam_ensemble_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, const float* __restrict__ eta, float b1, float b2, float eps,
                                                             float c1, float c2, int n, int g_stride) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t k = blockIdx.y, o = k * (size_t)n + i;
    const float gi = g[k * (size_t)g_stride + i];
    const float mi = b1 * m[o] + (1.0f - b1) * gi;
    const float vi = b2 * v[o] + (1.0f - b2) * gi * gi;
    m[o] = mi;
    v[o] = vi;
    w[o] -= mi * c1 / (sqrtf(vi * c2) + eps) * eta[k];
}

hipError_t launch_adam_ensemble(float* w, const float* grad, int grad_stride, float* m, float* v, const float* eta, float beta1, float beta2,
                                float eps, float beta1_t, float beta2_t, int n, int n_models, hipStream_t stream) {
    if (n < 1 || n_models < 1 || grad_stride < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_ensemble_kernel, dim3((n + 255) / 256, n_models), dim3(256), 0, stream, w, grad, m, v, eta, beta1, beta2, eps,
                       1.0f / (1.0f - beta1_t), 1.0f / (1.0f - beta2_t), n, grad_stride);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// data preparation: wind_mixing/src/data_containers.jl:343-427 coarse-grains every LES profile
// 128 -> 32 cells / 129 -> 33 faces and z-scores each variable before training.
// ------------------------------------------------------------------------------------------------
// coarse_grain(Φ, n, Center), src/DataWrangling/coarse_graining.jl:8-16: block means, Δ = N / n.
// coarse_grain_linear_interpolation(Φ, n, Face), :47-62: end points kept, interior point i (1-based) at position
// p = 1 + (i-1)(N-1)/(n-1): (⌊p⌋ + 1 - p) Φ[⌊p⌋] + (p - ⌊p⌋) Φ[⌊p⌋ + 1].  One thread per output value; rows are profiles.
__global__ void __launch_bounds__(256) coarse_grain_kernel(const float* __restrict__ in, int n_rows, int N, int n, int face,
                                                           float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)n_rows * n) return;
    const int row = (int)(idx / n), i = (int)(idx - (long)row * n);
    const float* src = in + (size_t)row * N;
    float v;
    if (!face) {
        const int d = N / n;
        float acc = 0.0f;
        for (int k = 0; k < d; k++) acc += src[i * d + k];
        v = acc / (float)d;
    } else if (i == 0) v = src[0];
    else if (i == n - 1) v = src[N - 1];
    else {
        const double p = 1.0 + (double)i * ((double)(N - 1) / (double)(n - 1));     // 1-based position, as the reference computes it
        const double fl = floor(p);
        const int k = (int)fl - 1;                                                    // 0-based index of Φ[⌊p⌋]
        v = (float)((fl + 1.0 - p) * (double)src[k] + (p - fl) * (double)src[k + 1 < N ? k + 1 : N - 1]);
    }
    out[idx] = v;
}

// ZeroMeanUnitVarianceScaling(data) (src/DataWrangling/feature_scaling.jl:17-20): μ = mean, σ = std (n - 1 in the denominator),
// accumulated in float64 by one workgroup in a fixed order (deterministic); out[0] = μ, out[1] = σ.
__global__ void __launch_bounds__(1024) zscore_stats_kernel(const float* __restrict__ x, long count, float* __restrict__ out2) {
    __shared__ double red[1024];
    double s = 0.0;
    for (long i = threadIdx.x; i < count; i += 1024) s += (double)x[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) { if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w]; __syncthreads(); }
    const double mu = red[0] / (double)count;
    __syncthreads();
    double q = 0.0;
    for (long i = threadIdx.x; i < count; i += 1024) { const double d = (double)x[i] - mu; q += d * d; }
    red[threadIdx.x] = q;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) { if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) { out2[0] = (float)mu; out2[1] = (float)sqrt(red[0] / (double)(count > 1 ? count - 1 : 1)); }
}

// scale(x, s) = (x - μ) / σ (feature_scaling.jl:22); μ, σ read from device memory (the output of zscore_stats_kernel)
__global__ void __launch_bounds__(256) zscore_scale_kernel(const float* __restrict__ x, long count, const float* __restrict__ mu_sigma,
                                                           float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = (x[i] - mu_sigma[0]) / mu_sigma[1];
}

hipError_t launch_coarse_grain(const float* in, int n_rows, int N, int n, int face, float* out, hipStream_t stream) {
    if (n_rows < 1 || N < 2 || n < 2 || n > N) return hipErrorInvalidValue;
    if (!face && N % n != 0) return hipErrorInvalidValue;
    const long total = (long)n_rows * n;
    hipLaunchKernelGGL(coarse_grain_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, n_rows, N, n, face, out);
    return hipGetLastError();
}

hipError_t launch_zscore_stats(const float* x, long count, float* out2, hipStream_t stream) {
    if (count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zscore_stats_kernel, dim3(1), dim3(1024), 0, stream, x, count, out2);
    return hipGetLastError();
}

hipError_t launch_zscore_scale(const float* x, long count, const float* mu_sigma, float* out, hipStream_t stream) {
    if (count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zscore_scale_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, x, count, mu_sigma, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// modified_pacanowski_philander!(model, constants, Δt, p, convective_adjustment): wind_mixing/src/NDE_oceananigans.jl:61-101, with
// the face diffusivities of modified_pacanowski_philander_diffusivity (:17-58).  Per column, one backward-Euler diffusion step of
// u, v (shared matrix) and T:
//     Ri_k = gα (T_k − T_{k−1}) Δz / ((u_k − u_{k−1})² + (v_k − v_{k−1})²)          (Oceanostics 0.3.2 richardson_number_ccf!, the
//            (Center, Center, Face) ratio ∂z b / ((∂z u)² + (∂z v)²) with b = gαT; third-party, pinned in wind_mixing/Manifest.toml:1279)
//     ν_k  = ν₀ + ν₋ tanh_step((Ri_k − Riᶜ)/ΔRi) on the interior faces, 0 on face 0 (:45-47);   tanh_step(x) = (1 − tanh x)/2
//     νT_k = convective_adjustment ? (Ri_k > 0 ? ν_k/Pr : 1) : ν_k/Pr  on EVERY face (:49-55; face 0 sees the halo cells)
//     lower_k = −c ν_k,  diag_k = 1 + c (ν_k + ν_{k+1}) (k < Nz−1),  diag_{Nz−1} = 1 + c ν_{Nz−1},  upper_k = −c ν_{k+1},  c = Δt/Δz²
//     u′ = L_ν \ u,  v′ = L_ν \ v,  T′ = L_νT \ T,  then T′_0 = T_0 (`T′[1] = T_bottom`, :94).
// The same strictly diagonally dominant tridiagonal as convadj_kernel: the Thomas recurrence is the reference's LU without pivoting.
// tanh_step is evaluated as 1/(1 + e^{2x}) (one v_exp + one v_rcp; exact limits 0 / 1 at Ri = ±∞, NaN stays NaN as in the reference,
// which a face with no shear AND no stratification produces: 0/0).
//
// HBM-bound: 2·3·4·Nz bytes per column (768 B at Nz = 32), ≈ 60 flop per level.  One WAVE per workgroup stages 64 columns of the three
// fields through LDS (rows padded to NZ+1: conflict-free column walks; 25 KB at Nz = 32, so six workgroups share a CU and one's solve
// hides under the others' float4 traffic); a lane solves one column in place in LDS with the elimination factors in registers.  The T
// system goes first: its sweep forms the face diffusivities from the still-unmodified u, v and keeps c·ν for the velocity sweep.
// ------------------------------------------------------------------------------------------------
typedef float co_f32x4 __attribute__((ext_vector_type(4)));
template <int NZ>
__global__ void __launch_bounds__(64) mpp_diffusion_kernel(const float* u, const float* v, const float* T,
                                                           const float* __restrict__ halo_bottom, MppParams P, float* uo, float* vo, float* To, int n_col) {
    extern __shared__ float cs_smem[];
    constexpr int LD = NZ + 1, Q = NZ / 4, FS = 64 * LD;
    const int lane = threadIdx.x;
    const int col0 = blockIdx.x * 64;
    const int ncol = min(64, n_col - col0);
    const float* srcs[3] = {u, v, T};
    float* dsts[3] = {uo, vo, To};
    if (ncol == 64) {
        co_f32x4 r[3][Q];
#pragma unroll
        for (int f = 0; f < 3; f++) {
            const co_f32x4* s = reinterpret_cast<const co_f32x4*>(srcs[f] + (size_t)col0 * NZ);
#pragma unroll
            for (int i = 0; i < Q; i++) r[f][i] = __builtin_nontemporal_load(s + i * 64 + lane);
        }
#pragma unroll
        for (int f = 0; f < 3; f++)
#pragma unroll
            for (int i = 0; i < Q; i++) {
                const int e = i * 64 + lane, cl = e / Q, k = (e % Q) * 4;
                float* d = cs_smem + f * FS + cl * LD + k;
                d[0] = r[f][i].x; d[1] = r[f][i].y; d[2] = r[f][i].z; d[3] = r[f][i].w;
            }
    } else {
        for (int f = 0; f < 3; f++) {
            const float4* s = reinterpret_cast<const float4*>(srcs[f] + (size_t)col0 * NZ);
            for (int e = lane; e < ncol * Q; e += 64) {
                const float4 q = s[e];
                const int cl = e / Q, k = (e % Q) * 4;
                float* d = cs_smem + f * FS + cl * LD + k;
                d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
            }
        }
    }
    __syncthreads();
    if (lane < ncol) {
        float* tu = cs_smem + lane * LD;
        mpp_column_step<NZ>(P, tu, tu + FS, tu + 2 * FS, halo_bottom, (size_t)col0 + lane, n_col);
    }
    __syncthreads();
    if (ncol == 64) {
#pragma unroll
        for (int f = 0; f < 3; f++) {
            co_f32x4* dd = reinterpret_cast<co_f32x4*>(dsts[f] + (size_t)col0 * NZ);
#pragma unroll
            for (int i = 0; i < Q; i++) {
                const int e = i * 64 + lane, cl = e / Q, k = (e % Q) * 4;
                const float* d = cs_smem + f * FS + cl * LD + k;
                const co_f32x4 q = {d[0], d[1], d[2], d[3]};
                __builtin_nontemporal_store(q, dd + e);
            }
        }
    } else {
        for (int f = 0; f < 3; f++) {
            float4* dd = reinterpret_cast<float4*>(dsts[f] + (size_t)col0 * NZ);
            for (int e = lane; e < ncol * Q; e += 64) {
                const int cl = e / Q, k = (e % Q) * 4;
                const float* d = cs_smem + f * FS + cl * LD + k;
                dd[e] = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
    }
}

// any 2 <= Nz <= 128 (not a multiple of 4, unaligned pointers, or none of the instantiated sizes): one thread per column from HBM
__global__ void __launch_bounds__(64) mpp_diffusion_generic_kernel(const float* u, const float* v, const float* T, const float* __restrict__ halo_bottom,
                                                                   MppParams P, float* uo, float* vo, float* To, int Nz, int n_col) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= n_col) return;
    const float* pu = u + (size_t)col * Nz;
    const float* pv = v + (size_t)col * Nz;
    const float* pT = T + (size_t)col * Nz;
    float kv[128], kT[128], cp[128], xa[128], xb[128];
    kv[0] = 0.0f;
    kT[0] = 0.0f;
    if (P.ca) {
        const float du = halo_bottom ? pu[0] - halo_bottom[col] : 0.0f;
        const float dv = halo_bottom ? pv[0] - halo_bottom[(size_t)n_col + col] : 0.0f;
        const float dT = halo_bottom ? pT[0] - halo_bottom[2 * (size_t)n_col + col] : 0.0f;
        const float Ri0 = P.galpha_dz * dT / (du * du + dv * dv);
        kT[0] = Ri0 > 0.0f ? 0.0f : P.c;
    }
    for (int k = 1; k < Nz; k++) mpp_face(P, P.c, pu[k] - pu[k - 1], pv[k] - pv[k - 1], pT[k] - pT[k - 1], kv[k], kT[k]);
    const float T_bottom = pT[0];
    // T
    for (int k = 0; k < Nz; k++) {
        const float kn = k + 1 < Nz ? kT[k + 1] : 0.0f;
        const float a = -kT[k], b = 1.0f + kT[k] + kn;
        const float inv = 1.0f / (k == 0 ? b : b - a * cp[k - 1]);
        cp[k] = -kn * inv;
        xa[k] = (k == 0 ? pT[k] : pT[k] - a * xa[k - 1]) * inv;
    }
    for (int k = Nz - 2; k >= 0; k--) xa[k] -= cp[k] * xa[k + 1];
    xa[0] = T_bottom;
    for (int k = 0; k < Nz; k++) To[(size_t)col * Nz + k] = xa[k];
    // u, v
    for (int k = 0; k < Nz; k++) {
        const float kn = k + 1 < Nz ? kv[k + 1] : 0.0f;
        const float a = -kv[k], b = 1.0f + kv[k] + kn;
        const float inv = 1.0f / (k == 0 ? b : b - a * cp[k - 1]);
        cp[k] = -kn * inv;
        xa[k] = (k == 0 ? pu[k] : pu[k] - a * xa[k - 1]) * inv;
        xb[k] = (k == 0 ? pv[k] : pv[k] - a * xb[k - 1]) * inv;
    }
    for (int k = Nz - 2; k >= 0; k--) { xa[k] -= cp[k] * xa[k + 1]; xb[k] -= cp[k] * xb[k + 1]; }
    for (int k = 0; k < Nz; k++) { uo[(size_t)col * Nz + k] = xa[k]; vo[(size_t)col * Nz + k] = xb[k]; }
}

hipError_t launch_mpp_diffusion(const float* u, const float* v, const float* T, const float* halo_bottom, float dt, float dz,
                                const float params[7], int convective_adjustment, float* uo, float* vo, float* To, int Nz, int n_col,
                                hipStream_t stream) {
    if (Nz < 2 || Nz > 128 || n_col < 1) return hipErrorInvalidValue;
    const MppParams P = mpp_params(params, dt, dz, convective_adjustment);
    const dim3 grid((n_col + 63) / 64), block(64);
    const bool aligned = (((uintptr_t)u | (uintptr_t)v | (uintptr_t)T | (uintptr_t)uo | (uintptr_t)vo | (uintptr_t)To) & 15) == 0;
    // in-place use is allowed field by field (uo == u etc.); any other overlap between the six arrays is the caller's error
#define MPP_LAUNCH(N) hipLaunchKernelGGL(mpp_diffusion_kernel<N>, grid, block, 3 * 64 * (N + 1) * sizeof(float), stream, u, v, T, halo_bottom, P, uo, vo, To, n_col)
    if (aligned && Nz == 16) MPP_LAUNCH(16);
    else if (aligned && Nz == 32) MPP_LAUNCH(32);
    else if (aligned && Nz == 64) MPP_LAUNCH(64);
    else hipLaunchKernelGGL(mpp_diffusion_generic_kernel, grid, block, 0, stream, u, v, T, halo_bottom, P, uo, vo, To, Nz, n_col);
#undef MPP_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// diagnose_baseline_flux_uw / _vw / _wT (wind_mixing/src/NDE_oceananigans.jl:157-191): what the diffusivity-only model saves with every state.
// Per column, on the Nz+1 faces (face 0 the bottom):  uw = −ν ∂z u,  vw = −ν ∂z v,  wT = −νT ∂z T  with the ν, νT of
// modified_pacanowski_philander_diffusivity above (mpp_sweep.h: the same face function as the step, c = 1) and the (Center, Center, Face)
// gradients (φ[f] − φ[f−1])/Δz — face 0 from the halo cells below (absent: zero-gradient fill) —, then the top face REPLACED by the given top
// flux (`uw[end] = uw_flux`, :163, :173, :185-187), so no halo above is read.
//
// HBM-bound: 3·4·Nz bytes in, 3·4·(Nz+1) out per column.  One wave per workgroup stages 64 columns of the three fields in LDS rows of Nz+1
// floats with coalesced loads; a lane walks its column upwards and overwrites slot k of each row with face k AFTER reading level k (the
// padding slot takes face Nz), which leaves in LDS the exact image of the workgroup's contiguous, 16-byte-aligned span of each output
// (64 (Nz+1) floats): it goes out as coalesced 16-byte pieces.  NZT = 0: Nz at run time (any 2 <= Nz <= 128).
// ------------------------------------------------------------------------------------------------
template <int NZT>
__global__ void __launch_bounds__(64) mpp_diagnose_flux_kernel(const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ T,
                                                               const float* __restrict__ top, const float* __restrict__ halo_bottom, MppParams P, float dz,
                                                               float* __restrict__ uw, float* __restrict__ vw, float* __restrict__ wT, int Nz_rt, int n_col,
                                                               int vec_in, int vec_out) {
    extern __shared__ __attribute__((aligned(16))) float dg_smem[];
    const int Nz = NZT ? NZT : Nz_rt, LD = Nz + 1, FS = 64 * LD;
    const int lane = threadIdx.x;
    const size_t col0 = (size_t)blockIdx.x * 64;
    const int ncol = (int)min((size_t)64, (size_t)n_col - col0);
    const float* srcs[3] = {u, v, T};
    float* dsts[3] = {uw, vw, wT};
    for (int f = 0; f < 3; f++) {
        const float* s = srcs[f] + col0 * Nz;
        float* d = dg_smem + f * FS;
        if (vec_in) {                               // Nz % 4 == 0: the four floats of a piece lie in one row
            for (int e = 4 * lane; e < ncol * Nz; e += 256) {
                const co_f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const co_f32x4*>(s + e));
                float* t = d + e + e / Nz;
                t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
            }
        } else {
            for (int e = lane; e < ncol * Nz; e += 64) d[e + e / Nz] = s[e];
        }
    }
    __syncthreads();
    if (lane < ncol) {
        const size_t col = col0 + lane;
        float* tu = dg_smem + lane * LD;
        float* tv = tu + FS;
        float* tT = tu + 2 * FS;
        float u_lo = tu[0], v_lo = tv[0], T_lo = tT[0];
        float a, b, c;
        mpp_face_nu_grad(P, dz, true, halo_bottom ? u_lo - halo_bottom[col] : 0.0f, halo_bottom ? v_lo - halo_bottom[(size_t)n_col + col] : 0.0f,
                         halo_bottom ? T_lo - halo_bottom[2 * (size_t)n_col + col] : 0.0f, a, b, c);
        tu[0] = -a; tv[0] = -b; tT[0] = -c;
#pragma unroll 8
        for (int k = 1; k < Nz; k++) {
            const float u_hi = tu[k], v_hi = tv[k], T_hi = tT[k];
            mpp_face_nu_grad(P, dz, false, u_hi - u_lo, v_hi - v_lo, T_hi - T_lo, a, b, c);
            tu[k] = -a; tv[k] = -b; tT[k] = -c;
            u_lo = u_hi; v_lo = v_hi; T_lo = T_hi;
        }
        tu[Nz] = top[col]; tv[Nz] = top[(size_t)n_col + col]; tT[Nz] = top[2 * (size_t)n_col + col];
    }
    __syncthreads();
    const int cnt = ncol * LD, nv = vec_out ? cnt / 4 : 0;
    for (int f = 0; f < 3; f++) {
        float* o = dsts[f] + col0 * LD;
        const float* d = dg_smem + f * FS;
        for (int i = lane; i < nv; i += 64) __builtin_nontemporal_store(*reinterpret_cast<const co_f32x4*>(d + 4 * i), reinterpret_cast<co_f32x4*>(o + 4 * i));
        for (int e = 4 * nv + lane; e < cnt; e += 64) o[e] = d[e];
    }
}

hipError_t launch_mpp_diagnose_flux(const float* u, const float* v, const float* T, const float* top_flux, const float* halo_bottom, float dz,
                                    const float params[7], int convective_adjustment, float* uw, float* vw, float* wT, int Nz, int n_col,
                                    hipStream_t stream) {
    if (Nz < 2 || Nz > 128 || n_col < 1) return hipErrorInvalidValue;
    const MppParams P = mpp_params(params, dz * dz, dz, convective_adjustment);          // (c = 1: the diagnosis takes no step)
    const dim3 grid((n_col + 63) / 64), block(64);
    const size_t lds = 3 * 64 * (size_t)(Nz + 1) * sizeof(float);
    const int vec_in = Nz % 4 == 0 && (((uintptr_t)u | (uintptr_t)v | (uintptr_t)T) & 15) == 0;
    const int vec_out = (((uintptr_t)uw | (uintptr_t)vw | (uintptr_t)wT) & 15) == 0;
#define DG_LAUNCH(N) hipLaunchKernelGGL(mpp_diagnose_flux_kernel<N>, grid, block, lds, stream, u, v, T, top_flux, halo_bottom, P, dz, uw, vw, wT, Nz, n_col, vec_in, vec_out)
    if (Nz == 16) DG_LAUNCH(16);
    else if (Nz == 32) DG_LAUNCH(32);
    else if (Nz == 64) DG_LAUNCH(64);
    else {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mpp_diagnose_flux_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        DG_LAUNCH(0);
    }
#undef DG_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// loss_per_tstep (wind_mixing/src/loss.jl:44-46; called on the six profile matrices of one simulation at training_postprocessing.jl:311-316)
// ------------------------------------------------------------------------------------------------
// blockIdx.y = model: its solution [n_col][n_save][n_var Nz] and its output [n_col][6][n_save] follow the previous model's; the truth is shared
__global__ void __launch_bounds__(256) loss_per_tstep_kernel(const float* __restrict__ sol, const float* __restrict__ truth, int n_col, int n_save, int Nz,
                                                             int n_var, float* __restrict__ out) {
    const long total = (long)n_col * n_save * n_var;
    sol += (size_t)blockIdx.y * total * Nz;
    out += (size_t)blockIdx.y * n_col * 6 * n_save;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const int v = (int)(it % n_var);
        const long cs = it / n_var;                        // column * n_save + save point
        const int sp = (int)(cs % n_save);
        const long c = cs / n_save;
        const float* a = sol + (cs * n_var + v) * Nz;
        const float* b = truth + (cs * n_var + v) * Nz;
        float sp2 = 0.0f, sg2 = 0.0f, prev = 0.0f;
        for (int k = 0; k < Nz; k++) {
            const float d = a[k] - b[k];
            sp2 += d * d;
            if (k > 0) { const float g = (d - prev) * (float)Nz; sg2 += g * g; }      // D^f: (x[k] - x[k-1]) Nz on the interior faces, 0 on the two end faces
            prev = d;
        }
        const int term = n_var == 3 ? v : 2;
        out[(c * 6 + term) * n_save + sp] = sp2 / (float)Nz;
        out[(c * 6 + 3 + term) * n_save + sp] = sg2 / (float)(Nz + 1);
    }
}

hipError_t launch_loss_per_tstep(const float* sol, const float* truth, int n_col, int n_save, int Nz, int n_var, float* out, hipStream_t stream, int n_models) {
    if (n_models < 1 || n_models > 65535) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n_models * n_col * 6 * n_save * sizeof(float), stream);
    if (e != hipSuccess) return e;
    const long total = (long)n_col * n_save * n_var;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(loss_per_tstep_kernel, dim3(blocks, n_models), dim3(256), 0, stream, sol, truth, n_col, n_save, Nz, n_var, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The adaptive integrator's error norm of a difference (the Richardson estimate of colnde_error_estimate): per state vector (row) the RMS over its
// components of (a_i - b_i) / (floor + |b_i|) — OrdinaryDiffEq's internalnorm of err / (abstol + reltol |u|), divided through by reltol —, then the
// maximum over the rows (columns x save points)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rel_diff_max_kernel(const float* __restrict__ a, const float* __restrict__ b, long n_rows, int row, float floor,
                                                           float* __restrict__ partial) {
    float mx = 0.0f;
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (long)gridDim.x * 256) {
        float s2 = 0.0f;
        for (int i = 0; i < row; i++) {
            const float q = (a[r * row + i] - b[r * row + i]) / (floor + fabsf(b[r * row + i]));
            s2 += q * q;
        }
        const float v = sqrtf(s2 / (float)row);
        mx = (v <= 3.0e38f) ? fmaxf(mx, v) : __int_as_float(0x7f800000);              // a NaN or Inf anywhere: +inf
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__global__ void __launch_bounds__(64) rel_diff_finish_kernel(const float* __restrict__ partial, int nb, float* __restrict__ out) {
    float mx = 0.0f;
    for (int i = threadIdx.x; i < nb; i += 64) mx = fmaxf(mx, partial[i]);
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off));
    if (threadIdx.x == 0) out[0] = mx;
}

hipError_t launch_rel_diff_max(const float* a, const float* b, long n_rows, int row, float floor, float* partial, float* out, hipStream_t stream) {
    const int blocks = (int)((n_rows + 255) / 256 < 1024 ? (n_rows + 255) / 256 : 1024);
    hipLaunchKernelGGL(rel_diff_max_kernel, dim3(blocks), dim3(256), 0, stream, a, b, n_rows, row, floor, partial);
    hipLaunchKernelGGL(rel_diff_finish_kernel, dim3(1), dim3(64), 0, stream, partial, blocks, out);
    return hipGetLastError();
}

// The same norm per save point (colnde_choose_schedule): out[n] = max over the columns of the row norm at save point n, rows [column][n_save][row].
// One workgroup per save point; a maximum, so the order of the reduction does not matter.
__global__ void __launch_bounds__(256) rel_diff_save_max_kernel(const float* __restrict__ a, const float* __restrict__ b, int n_col, int n_save, int row, float floor,
                                                                float* __restrict__ out) {
    const int n = blockIdx.x;
    float mx = 0.0f;
    for (int c = threadIdx.x; c < n_col; c += 256) {
        const size_t r = ((size_t)c * n_save + n) * row;
        float s2 = 0.0f;
        for (int i = 0; i < row; i++) {
            const float q = (a[r + i] - b[r + i]) / (floor + fabsf(b[r + i]));
            s2 += q * q;
        }
        const float v = sqrtf(s2 / (float)row);
        mx = (v <= 3.0e38f) ? fmaxf(mx, v) : __int_as_float(0x7f800000);              // a NaN or Inf anywhere: +inf
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) out[n] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

hipError_t launch_rel_diff_save_max(const float* a, const float* b, int n_col, int n_save, int row, float floor, float* out, hipStream_t stream) {
    if (n_col < 1 || n_save < 1 || row < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rel_diff_save_max_kernel, dim3(n_save), dim3(256), 0, stream, a, b, n_col, n_save, row, floor, out);
    return hipGetLastError();
}

// ... and per member and save point (colnde_ensemble_error_estimate, colnde_ensemble_choose_schedule): out[k][n] = max over the columns of the row norm
// of rows [member][column][n_save][row].  One workgroup per (save point, member); 16 lanes share a column's row — lane j takes the entries j, j + 16, ...
// in that order, the 16 partial sums meet in a butterfly — and the workgroup walks the columns 16 at a time, so eight simulations fill half a wavefront
// where a lane per column would fill an eighth, and the row is read in 64-byte runs.  Every sum has one order and a maximum has none: two launches
// give the same bits.  Scalar loads: nothing is asked of the rows' alignment.
__global__ void __launch_bounds__(256) rel_diff_member_save_max_kernel(const float* __restrict__ a, const float* __restrict__ b, int n_col, int n_save, int row, float floor,
                                                                       float* __restrict__ out) {
    const int n = blockIdx.x, k = blockIdx.y, j = threadIdx.x & 15;
    float mx = 0.0f;
    for (int c0 = 0; c0 < n_col; c0 += 16) {                                          // (uniform trip count: every lane reaches the shuffles)
        const int c = c0 + (threadIdx.x >> 4);
        float s2 = 0.0f;
        if (c < n_col) {
            const size_t r = (((size_t)k * n_col + c) * n_save + n) * row;
            for (int i = j; i < row; i += 16) {
                const float q = (a[r + i] - b[r + i]) / (floor + fabsf(b[r + i]));
                s2 += q * q;
            }
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s2 += __shfl_xor(s2, off, 16);
        const float v = sqrtf(s2 / (float)row);
        mx = (v <= 3.0e38f) ? fmaxf(mx, v) : __int_as_float(0x7f800000);              // a NaN or Inf anywhere: +inf
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) out[(size_t)k * n_save + n] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

hipError_t launch_rel_diff_member_save_max(const float* a, const float* b, int K, int n_col, int n_save, int row, float floor, float* out, hipStream_t stream) {
    if (K < 1 || K > 65535 || n_col < 1 || n_save < 1 || row < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rel_diff_member_save_max_kernel, dim3(n_save, K), dim3(256), 0, stream, a, b, n_col, n_save, row, floor, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Free-convection ensembles (colnde_create_fc_ensemble): judging K networks on the same simulations.
// ------------------------------------------------------------------------------------------------
// out[k][c][n] = mean over the Nz levels of (sol[k][c][n][:] - truth[c][n][:])^2 — Flux.mse(true, nde, agg = x -> mean(x, dims=1)) of
// free_convection/src/testing.jl:83 for every model, simulation and save point.  A lane per level, NZ lanes per row (two rows per wavefront at
// Nz = 32); the sum is a shuffle tree over the row's lanes, always in the same order: two launches give the same bits.  Bandwidth-bound: sol is read once.
template <int NZ>
__global__ void __launch_bounds__(256) column_loss_kernel(const float* __restrict__ sol, const float* __restrict__ truth, long rows_per_model, long n_rows,
                                                          float* __restrict__ out) {
    const int lvl = threadIdx.x & (NZ - 1);
    const long row = (long)blockIdx.x * (256 / NZ) + threadIdx.x / NZ;           // (model, simulation, save point)
    float v = 0.0f;
    if (row < n_rows) {
        const float d = sol[row * NZ + lvl] - truth[(row % rows_per_model) * NZ + lvl];
        v = d * d;
    }
#pragma unroll
    for (int off = NZ / 2; off > 0; off >>= 1) v += __shfl_down(v, off, NZ);
    if (lvl == 0 && row < n_rows) out[row] = v * (1.0f / (float)NZ);
}

hipError_t launch_column_loss(const float* sol, const float* truth, int Nz, long rows_per_model, int n_models, float* out, hipStream_t stream) {
    if ((Nz != 32 && Nz != 64) || rows_per_model < 1 || n_models < 1) return hipErrorInvalidValue;
    const long n_rows = rows_per_model * n_models, per_block = 256 / Nz, blocks = (n_rows + per_block - 1) / per_block;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    if (Nz == 64) hipLaunchKernelGGL((column_loss_kernel<64>), dim3((unsigned)blocks), dim3(256), 0, stream, sol, truth, rows_per_model, n_rows, out);
    else hipLaunchKernelGGL((column_loss_kernel<32>), dim3((unsigned)blocks), dim3(256), 0, stream, sol, truth, rows_per_model, n_rows, out);
    return hipGetLastError();
}

// The soft spatial-causality penalty of train_free_convection_nde.jl:186-197 for every model: c_k sum_{r < q} W1_k[r, q]^2 over the strict upper triangle of
// the first Dense weight (H x M, W1[r, q] at w1_off + q * H + r: Flux.destructure's column-major order; the plain network: 4 Nz x Nz at offset 0, the
// --conv network: 4 Nz x (Nz - c + 1) at offset c + 1 — ps[dense_layer_params_idx], :189-195; M <= H), added to the total of the model's result
// row, and its gradient 2 c_k W1_k[r, q] added to the row's gradient entries.  One workgroup per model; thread t owns the masked entries e = t, t + 256, ...
// of the triangle's column-by-column enumeration and the partial sums meet in a fixed tree, so the value is bit-reproducible.  c_k = 0: the row is not
// touched at all (not even rewritten).  Plain vector loads and stores; every entry has one owner, so nothing is atomic.
__global__ void __launch_bounds__(256) causal_penalty_kernel(const float* __restrict__ w, const float* __restrict__ coeff, float* __restrict__ result,
                                                             int H, int M, int w1_off, int n_params) {
    __shared__ float part[256];
    const size_t k = blockIdx.x;
    const float c = coeff[k];
    if (c == 0.0f) return;                                           // (uniform over the workgroup)
    const float* W = w + k * (size_t)n_params + w1_off;
    float* row = result + k * ((size_t)n_params + 8);
    const int n_mask = M * (M - 1) / 2;
    float s = 0.0f;
    for (int e = threadIdx.x; e < n_mask; e += 256) {
        // column q holds the q entries r = 0 .. q - 1; entries of columns < q: q (q - 1) / 2
        int q = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)e)) * 0.5f);
        while (q * (q - 1) / 2 > e) q--;
        while ((q + 1) * q / 2 <= e) q++;
        const int r = e - q * (q - 1) / 2;
        const int idx = q * H + r;
        const float v = W[idx];
        s += v * v;
        row[w1_off + idx] += 2.0f * c * v;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) row[n_params + 6] += c * part[0];
}

hipError_t launch_causal_penalty(const float* w, const float* coeff, float* result, int H, int M, int w1_off, int n_params, int n_models, hipStream_t stream) {
    if (M < 2 || M > H || n_models < 1 || w1_off < 0 || (long)w1_off + (long)H * M > n_params) return hipErrorInvalidValue;
    hipLaunchKernelGGL(causal_penalty_kernel, dim3(n_models), dim3(256), 0, stream, w, coeff, result, H, M, w1_off, n_params);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The --conv network of the free-convection driver (train_free_convection_nde.jl:110-122; colnde_create_conv): Conv((c, 1), 1 => 1, relu) in front of
// the three Dense layers.  The fc32 kernels run the dense chain on W1 padded with zero columns to 4Nz x Nz; these three kernels are what surrounds them.
//   theta  = [w (c); b; vec(W1) (4Nz x M, column-major, M = Nz - c + 1); b1; W2; b2; W3; b3]        the user's vector (Flux.params order)
//   padded = [vec(W1), 4Nz (c - 1) zeros; b1; ...]                                                  the plain network's vector the engine packs
// ------------------------------------------------------------------------------------------------
// (blockIdx.y = model of a conv ensemble: the user's vectors theta_stride floats apart, the padded ones n_pad)
__global__ void __launch_bounds__(256) fc_conv_pad_kernel(const float* __restrict__ theta, int c, int w1_end, int n_zero, int n_pad, float* __restrict__ padded,
                                                           size_t theta_stride) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pad) return;
    theta += blockIdx.y * theta_stride;
    padded += blockIdx.y * (size_t)n_pad;
    padded[p] = p < w1_end ? theta[c + 1 + p] : (p < w1_end + n_zero ? 0.0f : theta[c + 1 + p - n_zero]);
}

// The filter's gradient from the conv tape [row = (record, column)][x (Nz) | z̄ (Nz)]: slot d of a workgroup's output row is the sum over its rows and
// levels of z̄[i] x[i + d] (= ∂/∂w[c - d], 1-based), slot FC_CG_SLOTS - 1 the sum of z̄ (= ∂/∂b).  Lane = level (Nz = 32: two rows per wave); x[i + d]
// comes from the lane d above — within the row wherever z̄[i] can be non-zero (i < M).  Every sum in a fixed order: a thread over its rows, then one
// thread per slot over the 256 partial sums.  blockIdx.y = model of a conv ensemble (its tape and its slab rows at a stride): the sums of a model are
// those of a single handle, in the same order.
#define FC_CG_TAPS 8                               // = FC_CONV_MAX (engine_fc.h)
#define FC_CG_SLOTS (FC_CG_TAPS + 1)
template <int NZ>
__global__ void __launch_bounds__(256) fc_conv_grad_kernel(const float* __restrict__ ctape, long n_rows, long rows_per_wg, int c, float* __restrict__ out,
                                                            size_t ctape_stride, size_t out_stride) {
    __shared__ float scr[FC_CG_SLOTS][256];
    ctape += blockIdx.y * ctape_stride;
    out += blockIdx.y * out_stride;
    constexpr int RPB = 256 / NZ;                   // rows in flight per workgroup
    const int tid = threadIdx.x, i = tid & (NZ - 1), rs = tid / NZ;
    const long r0 = (long)blockIdx.x * rows_per_wg, r1 = r0 + rows_per_wg < n_rows ? r0 + rows_per_wg : n_rows;
    float acc[FC_CG_SLOTS];
#pragma unroll
    for (int k = 0; k < FC_CG_SLOTS; k++) acc[k] = 0.0f;
    for (long base = r0; base < r1; base += RPB) {  // (uniform trip count: the shifts below need every lane)
        const long row = base + rs;
        const bool ok = row < r1;
        const float x = ok ? ctape[row * (2 * NZ) + i] : 0.0f;
        const float z = ok ? ctape[row * (2 * NZ) + NZ + i] : 0.0f;
#pragma unroll
        for (int d = 0; d < FC_CG_TAPS; d++)
            if (d < c) acc[d] = fmaf(z, __shfl_down(x, d), acc[d]);
        acc[FC_CG_SLOTS - 1] += z;
    }
#pragma unroll
    for (int k = 0; k < FC_CG_SLOTS; k++) scr[k][tid] = acc[k];
    __syncthreads();
    if (tid < FC_CG_SLOTS) {
        float s = 0.0f;
        for (int t = 0; t < 256; t++) s += scr[tid][t];
        out[(size_t)blockIdx.x * FC_CG_SLOTS + tid] = s;
    }
}

// The user's result [c + 1 filter entries; the padded gradient without W1's padded columns (exactly zero: their input is); 8 loss slots]: the filter
// entries are the sums over the rows of the filter slab, in row order.  blockIdx.y = model of a conv ensemble (strides in floats; the rows of out: n_out).
__global__ void __launch_bounds__(256) fc_conv_fold_kernel(const float* __restrict__ gpad, const float* __restrict__ cslab, int n_rows, int c, int w1_end,
                                                            int n_zero, int n_out, float* __restrict__ out, size_t gpad_stride, size_t cslab_stride) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_out) return;
    gpad += blockIdx.y * gpad_stride;
    cslab += blockIdx.y * cslab_stride;
    out += blockIdx.y * (size_t)n_out;
    if (idx <= c) {
        const int slot = idx < c ? c - 1 - idx : FC_CG_SLOTS - 1;
        float s = 0.0f;
        for (int r = 0; r < n_rows; r++) s += cslab[(size_t)r * FC_CG_SLOTS + slot];
        out[idx] = s;
        return;
    }
    const int q = idx - (c + 1);
    out[idx] = gpad[q < w1_end ? q : q + n_zero];
}

hipError_t launch_fc_conv_pad(const float* theta, int c, int w1_end, int n_zero, int n_pad, float* padded, hipStream_t stream, int n_models, size_t theta_stride) {
    if (c < 2 || c > FC_CG_TAPS || w1_end < 1 || n_zero < 1 || n_pad < w1_end + n_zero || n_models < 1 || n_models > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fc_conv_pad_kernel, dim3((n_pad + 255) / 256, n_models), dim3(256), 0, stream, theta, c, w1_end, n_zero, n_pad, padded, theta_stride);
    return hipGetLastError();
}

int fc_conv_grad_slices(long n_rows) {
    const long s = (n_rows + 255) / 256;            // at least 256 rows per workgroup
    return (int)(s < 1 ? 1 : (s > FC_CONV_GRAD_MAX_SLICES ? FC_CONV_GRAD_MAX_SLICES : s));
}

hipError_t launch_fc_conv_grad(const float* ctape, long n_rows, int Nz, int c, float* slab_rows, hipStream_t stream, int n_models, size_t ctape_stride,
                               size_t slab_stride) {
    if (n_rows < 1 || c < 2 || c > FC_CG_TAPS || (Nz != 32 && Nz != 64) || n_models < 1 || n_models > 65535) return hipErrorInvalidValue;
    const int n_wg = fc_conv_grad_slices(n_rows);
    const int rpb = 256 / Nz;
    const long per = ((n_rows + n_wg - 1) / n_wg + rpb - 1) / rpb * rpb;
    if (Nz == 64) hipLaunchKernelGGL(fc_conv_grad_kernel<64>, dim3(n_wg, n_models), dim3(256), 0, stream, ctape, n_rows, per, c, slab_rows, ctape_stride, slab_stride);
    else hipLaunchKernelGGL(fc_conv_grad_kernel<32>, dim3(n_wg, n_models), dim3(256), 0, stream, ctape, n_rows, per, c, slab_rows, ctape_stride, slab_stride);
    return hipGetLastError();
}

hipError_t launch_fc_conv_fold(const float* gpad, const float* cslab, int n_rows, int c, int w1_end, int n_zero, int n_out, float* out, hipStream_t stream,
                               int n_models, size_t gpad_stride, size_t cslab_stride) {
    if (n_rows < 1 || c < 2 || c > FC_CG_TAPS || n_out <= c + 1 || n_models < 1 || n_models > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fc_conv_fold_kernel, dim3((n_out + 255) / 256, n_models), dim3(256), 0, stream, gpad, cslab, n_rows, c, w1_end, n_zero, n_out, out,
                       gpad_stride, cslab_stride);
    return hipGetLastError();
}
