// engine_tile16.hip — the MFMA tile engine (gfx950 / CDNA4 only).
//
// One workgroup owns a tile of CT = 16 columns for the whole time integration.  Every dense layer is a
// small GEMM on v_mfma_f32_16x16x4_f32 with N = the 16 columns:
//   forward     Z_l[c][j]   = b_l[j] + sum_k W_l[j][k] A_{l-1}[c][k]          (A = packed W, B = activations in LDS)
//   backward    dA_{l-1}[c][i] = sum_j W_l[j][i] dZ_l[c][j]                    (A = packed W^T)
//   weight grad dW_l[j][i] += sum_c A_{l-1}[c][i] dZ_l[c][j]                   (K = the 16 columns; accumulators stay in
//                                                                              registers for the whole kernel)
// Activations live in LDS as [column][feature] rows (row stride == 2 mod 4 keeps the B-operand reads conflict-free);
// weights are streamed from L2 in a pre-packed, zero-padded A-operand image (pack_weights_kernel), so the hot loops
// carry no bounds checks.  The physics (flux assembly, Richardson-number diffusivity, flux divergence, Coriolis) and
// its hand-written pullback run between the GEMMs, one thread per (column, face/cell).
//
// Reference arithmetic restated (paths relative to /root/reference):
//   wind_mixing/src/NDE_training.jl:46-165 (NDE, predict_flux, predict_NDE), training_postprocessing.jl:105-153 (NDE!),
//   free_convection/src/free_convection_nde.jl:29-38, convective_adjustment_nde.jl:33-48,
//   src/differentiation_operators.jl:6-29, wind_mixing/src/filtering_operators.jl:1-14, wind_mixing/src/loss.jl:1-9,
//   wind_mixing/src/NDE_training.jl:290-323 (losses), free_convection/double_gyre_nn.jl:149-168 (inference).
#include "colnde_dev.h"
#include <cstdlib>
#include "engine_tile16.h"
#include "engine_netsplit.h"   // RtPhys: the per-model closure constants of an ensemble
#include "kernel_select.h"
#include "split_bf16.h"
#include "pretrain_sample.h"
#include <algorithm>

#define FWD_MAXR 12   // owner-thread register items per state array in the forward kernel: CT*ns <= FWD_MAXR*blockDim
#define MAXB 4        // bias-gradient accumulators per thread: n_bias <= MAXB*blockDim

// Diagnostic build only (-DCOLNDE_STAMPS): per-phase cycle sums of workgroup 0 / wave 0, read back through
// colnde_debug_stamps().  No stamp executes in the shipped library.
#ifdef COLNDE_STAMPS
__device__ unsigned long long g_stamps[16];
#define STAMP_DECL unsigned long long st_t0 = 0, st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define STAMP_BEGIN() do { __builtin_amdgcn_sched_barrier(0); st_t0 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define STAMP(i) do { __builtin_amdgcn_sched_barrier(0); unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[i] += t_ - st_t0; st_t0 = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#define STAMP_FLUSH() do { if (blockIdx.x == 0 && threadIdx.x == 0) for (int q = 0; q < 8; q++) g_stamps[q] = st_acc[q]; } while (0)
__device__ unsigned long long g_fine[16];
#define FINE_BEGIN() unsigned long long ft0_; do { __builtin_amdgcn_sched_barrier(0); ft0_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define FINE(i) do { __builtin_amdgcn_sched_barrier(0); unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (blockIdx.x == 0 && threadIdx.x == 0) g_fine[i] += t_ - ft0_; ft0_ = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define FINE_BEGIN()
#define FINE(i)
#define STAMP_DECL
#define STAMP_BEGIN()
#define STAMP(i)
#define STAMP_FLUSH()
#endif

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// acc += sum_{s<n} mfma(ap[s*a_step], bp[s*b_step]): operands are read U steps at a time ahead of their MFMAs.
// (The engine is instruction-issue-bound, so the loop carries no clamps or selects: full chunks, then a remainder.)
#ifndef GU
#define GU 32     // prefetch depth (k-steps) of the chains whose A operand streams from L2 (packed weight image); measured on the
                  // 64-256-256-63 taped adjoint: depth 4: 296 ms, 8: 413 ms, 16: 247 ms, 32: 233 ms (remainders halve the depth)
#endif
template <int U>
__device__ __forceinline__ f32x4 gemm_chain(const float* ap, int a_step, const float* bp, int b_step, int n, f32x4 acc) {
    int s = 0;
    for (; s + U <= n; s += U) {
        float a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            a[u] = ap[(s + u) * a_step];
            b[u] = bp[(s + u) * b_step];
        }
#pragma unroll
        for (int u = 0; u < U; u++) acc = mfma16(a[u], b[u], acc);
    }
    if (U > 1) return s < n ? gemm_chain<(U > 1 ? U / 2 : 1)>(ap + s * a_step, a_step, bp + s * b_step, b_step, n - s, acc) : acc;
    for (; s < n; s++) acc = mfma16(ap[s * a_step], bp[s * b_step], acc);
    return acc;
}

// The same chain with both operands fetched FOUR k-steps at a time: the packed weight image holds, per lane, the A operands of four
// consecutive MFMAs contiguously (one 16-byte load from L2 instead of four dword loads, each of which cost a 64-bit address add), and
// the K index is dealt so that the matching four B operands are four consecutive floats of the activation row (two 8-byte LDS
// reads): k = 16 S + 4 q + j for group S, lane quarter q, MFMA j.  ~1.75 memory instructions per MFMA become ~0.75.
//   ap4: this lane's float4 of group 0 (groups are 64 lanes x 16 bytes apart); bp: the activation row + 4 q; n = groups of 16 k
template <int U>
__device__ __forceinline__ f32x4 gemm_chain4(const float4* ap4, const float* bp, int n, f32x4 acc) {
    int s = 0;
    for (; s + U <= n; s += U) {
        float4 a[U];
        float2 b0[U], b1[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            a[u] = ap4[(size_t)(s + u) * 64];
            b0[u] = *reinterpret_cast<const float2*>(bp + (s + u) * 16);
            b1[u] = *reinterpret_cast<const float2*>(bp + (s + u) * 16 + 2);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            acc = mfma16(a[u].x, b0[u].x, acc);
            acc = mfma16(a[u].y, b0[u].y, acc);
            acc = mfma16(a[u].z, b1[u].x, acc);
            acc = mfma16(a[u].w, b1[u].y, acc);
        }
    }
    if (U > 1) return s < n ? gemm_chain4<(U > 1 ? U / 2 : 1)>(ap4 + (size_t)s * 64, bp + s * 16, n - s, acc) : acc;
    for (; s < n; s++) {
        const float4 a = ap4[(size_t)s * 64];
        const float2 b0 = *reinterpret_cast<const float2*>(bp + s * 16), b1 = *reinterpret_cast<const float2*>(bp + s * 16 + 2);
        acc = mfma16(a.x, b0.x, acc);
        acc = mfma16(a.y, b0.y, acc);
        acc = mfma16(a.z, b1.x, acc);
        acc = mfma16(a.w, b1.y, acc);
    }
    return acc;
}
#ifndef GU4
#define GU4 8     // groups (of four k-steps) in flight in the L2-streamed chains: the same 32 k-steps of prefetch as GU
#endif

// ------------------------------------------------------------------------------------------------
// weight packing: raw Flux.destructure weights -> A-operand images (four floats per lane per group of four MFMAs)
//   forward image  Wf[net][l][mt][S][lane][j]: A[i = mt*16 + (lane&15)][k = 16 S + 4 (lane>>4) + j] = W_l[i][k]
//   backward image Wb[net][l][it][S][lane][j]: A[i = it*16 + (lane&15)][o = 16 S + 4 (lane>>4) + j] = W_l[o][i]
// (K padded with zeros to a multiple of 16.)  W_l[j][k] (out j, in k) sits at w_off[l] + k*no + j  (column-major out x in).
// ------------------------------------------------------------------------------------------------
__global__ void pack_weights_kernel(DevModel m, PackInfo pk, const float* __restrict__ w, float* __restrict__ wf,
                                    float* __restrict__ wb) {
#define T16_ENS 0
#include "t16_pack_weights_body.inc"
#undef T16_ENS
}
// Tile ensembles (colnde_create_tile_ensemble): the kernels below marked _ens carry the model index in blockIdx.y.  Each is the text of its single-model
// twin (the t16_*_body.inc files, included by both, so that the single-model kernels stay the machine code they were) behind a preamble that moves
// every pointer to what model blockIdx.y owns (T16Ens strides).
__global__ void pack_weights_ens_kernel(DevModel m, PackInfo pk, const float* __restrict__ w, float* __restrict__ wf,
                                        float* __restrict__ wb, T16Ens en) {
    w += blockIdx.y * en.w;
    wf += blockIdx.y * en.wf;
    wb += blockIdx.y * en.wb;
#define T16_ENS 1
#include "t16_pack_weights_body.inc"
#undef T16_ENS
}

// ------------------------------------------------------------------------------------------------
// dense layers on MFMA
// ------------------------------------------------------------------------------------------------
// Forward pass of all nets.  xs: [CT][ld_x] state rows; A (and Z when STORE_Z): [net][CT][ld_a].
// WLDS: `w` points at the raw weights staged in LDS (A operand read in place, rows clamped so that a padded tile
// never leaves the array; out-of-range k meets a zero B operand); otherwise `w` is global and the A operand comes
// from the packed image `wf`.
template <bool STORE_Z, bool WLDS>
__device__ __forceinline__ void mlp_forward(const DevModel& m, const PackInfo& pk, const float* w,
                                            const float* __restrict__ wf, const float* xs, float* Z, float* A,
                                            int wave, int nwaves, int lane, float* __restrict__ zrec = nullptr, int zld = 0) {
    const int c = lane & 15, kq = lane >> 4;
    FINE_BEGIN();
    for (int l = 0; l < m.n_layers; l++) {
        const int ni = m.sizes[l], no = m.sizes[l + 1];
        const int nmt = (no + 15) >> 4, nk4 = (ni + 3) >> 2;
        const int act = m.acts[l];
        FINE(0);
        for (int job = wave; job < nmt * m.n_nets; job += nwaves) {
            const int net = job / nmt, mt = job - net * nmt;
            const float* bl = w + (size_t)net * m.net_size + m.b_off[l];
            const float* in = (l == 0) ? xs + c * m.ld_x : A + (net * CT + c) * m.ld_a + m.act_off[l - 1];
            // the bias is fetched now and added after the chain, so that its load latency hides under the MFMAs
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            float bq[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = mt * 16 + 4 * kq + r;
                bq[r] = bl[min(row, no - 1)];
            }
            FINE(1);
            if (WLDS) {
                const float* ap = w + net * m.net_size + m.w_off[l] + kq * no + min(mt * 16 + (lane & 15), no - 1);
                acc = gemm_chain<4>(ap, 4 * no, in + kq, 4, nk4, acc);
            } else {
                const int nS = (ni + 15) >> 4;
                const float4* ap4 = reinterpret_cast<const float4*>(wf + (size_t)net * pk.pf_net + pk.pf_off[l]) + (size_t)mt * nS * 64 + lane;
                acc = gemm_chain4<GU4>(ap4, in + 4 * kq, nS, acc);
            }
            FINE(2);
            const int ro = (net * CT + c) * m.ld_a + m.act_off[l];
            float zv[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = mt * 16 + 4 * kq + r;
                zv[r] = acc[r] + bq[r];
                if (row < no) {
                    if (STORE_Z) Z[ro + row] = zv[r];
                    A[ro + row] = dev_act(act, zv[r]);
                }
            }
            // hidden-layer pre-activations taped for the adjoint: row [c][net][hidden features] of stride zld; the lane's four
            // rows are consecutive and 16-byte aligned (every segment starts at a multiple of 4 floats)
            if (zrec && l + 1 < m.n_layers) {
                float* zo = zrec + c * zld + net * m.act_off[m.n_layers - 1] + m.act_off[l] + mt * 16 + 4 * kq;
                if (mt * 16 + 4 * kq + 3 < no) *reinterpret_cast<float4*>(zo) = make_float4(zv[0], zv[1], zv[2], zv[3]);
                else
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (mt * 16 + 4 * kq + r < no) zo[r] = zv[r];
            }
            FINE(3);
        }
        __syncthreads();
        FINE(4);
    }
}

// Backward pass: on entry Z's last-layer slot holds dZ_L; on exit every Z slot holds dZ_l and xb += W_1^T dZ_1.
template <bool WLDS>
__device__ __forceinline__ void mlp_backward(const DevModel& m, const PackInfo& pk, const float* w,
                                             const float* __restrict__ wb, float* Z, float* xb, int wave, int nwaves,
                                             int lane) {
    const int c = lane & 15, jq = lane >> 4;
    for (int l = m.n_layers - 1; l >= 0; l--) {
        const int ni = m.sizes[l], no = m.sizes[l + 1];
        const int nit = (ni + 15) >> 4, nj4 = (no + 3) >> 2;
        if (l > 0) {
            const int actp = m.acts[l - 1];
            for (int job = wave; job < nit * m.n_nets; job += nwaves) {
                const int net = job / nit, it = job - net * nit;
                const float* dz = Z + (net * CT + c) * m.ld_a + m.act_off[l];
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                if (WLDS) {
                    const float* ap = w + net * m.net_size + m.w_off[l] + min(it * 16 + (lane & 15), ni - 1) * no + jq;
                    acc = gemm_chain<4>(ap, 4, dz + jq, 4, nj4, acc);
                } else {
                    const int nS = (no + 15) >> 4;
                    const float4* ap4 = reinterpret_cast<const float4*>(wb + (size_t)net * pk.pb_net + pk.pb_off[l]) + (size_t)it * nS * 64 + lane;
                    acc = gemm_chain4<GU4>(ap4, dz + 4 * jq, nS, acc);
                }
                const int ro = (net * CT + c) * m.ld_a + m.act_off[l - 1];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = it * 16 + 4 * jq + r;
                    if (row < ni) Z[ro + row] = acc[r] * dev_act_grad(actp, Z[ro + row]);
                }
            }
        } else {
            for (int it = wave; it < nit; it += nwaves) {
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int net = 0; net < m.n_nets; net++) {
                    const float* dz = Z + (net * CT + c) * m.ld_a + m.act_off[0];
                    if (WLDS) {
                        const float* ap = w + net * m.net_size + m.w_off[0] + min(it * 16 + (lane & 15), ni - 1) * no + jq;
                        acc = gemm_chain<4>(ap, 4, dz + jq, 4, nj4, acc);
                    } else {
                        const int nS = (no + 15) >> 4;
                        const float4* ap4 = reinterpret_cast<const float4*>(wb + (size_t)net * pk.pb_net + pk.pb_off[0]) + (size_t)it * nS * 64 + lane;
                        acc = gemm_chain4<GU4>(ap4, dz + 4 * jq, nS, acc);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = it * 16 + 4 * jq + r;
                    if (row < ni) xb[c * m.ld_x + row] += acc[r];
                }
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// The dense chains on the bf16 pipe (round 5; networks whose activation rows live in global memory — DevModel::ag — under COLNDE_MATRIX_BF16X3_EXACT): exact
// three-way operand split (split_bf16.h), six v_mfma_f32_16x16x32_bf16 per 32-deep k-block and 16-row tile.  The weights are split ONCE per call by
// pack_planes_kernel; the activation row's eight values of a lane are split once per k-block and shared by the TG row tiles a wave owns (the split costs
// as much vector time as six of these MFMAs cost matrix time: one tile per split would buy nothing).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 t16_mfma_bf(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 t16_mfma_bf3(const Bf3& a, const Bf3& b, f32x4 c) {     // smallest products first
    c = t16_mfma_bf(a.m, b.m, c);
    c = t16_mfma_bf(a.l, b.h, c);
    c = t16_mfma_bf(a.h, b.l, c);
    c = t16_mfma_bf(a.m, b.h, c);
    c = t16_mfma_bf(a.h, b.m, c);
    c = t16_mfma_bf(a.h, b.h, c);
    return c;
}
#define T16_TG 5      // row tiles per wave and split (25 tiles of a 400-row layer: five jobs per net)

__global__ void pack_planes_kernel(DevModel m, const float* __restrict__ w, unsigned* __restrict__ sf, unsigned* __restrict__ sb) {
#define T16_ENS 0
#include "t16_pack_planes_body.inc"
#undef T16_ENS
}
__global__ void pack_planes_ens_kernel(DevModel m, const float* __restrict__ w, unsigned* __restrict__ sf, unsigned* __restrict__ sb, T16Ens en) {
    w += blockIdx.y * en.w;
    sf += blockIdx.y * en.sf;
    sb += blockIdx.y * en.sb;
#define T16_ENS 1
#include "t16_pack_planes_body.inc"
#undef T16_ENS
}

// eight consecutive floats of an activation / delta row (8-byte aligned): fetched one k-block ahead of the split that makes them a B operand (the rows live in global memory)
struct T16Row8 { float2 v[4]; };
__device__ __forceinline__ T16Row8 t16_row_load8(const float* p) {
    T16Row8 r;
#pragma unroll
    for (int q = 0; q < 4; q++) r.v[q] = *reinterpret_cast<const float2*>(p + 2 * q);
    return r;
}
__device__ __forceinline__ Bf3 t16_row_split8(const T16Row8& r) {
    const float x[8] = {r.v[0].x, r.v[0].y, r.v[1].x, r.v[1].y, r.v[2].x, r.v[2].y, r.v[3].x, r.v[3].y};
    return bf3_split8(x);
}

// forward pass of all nets with the chains on the bf16 pipe (the f32 twin is mlp_forward<false, false>)
__device__ __forceinline__ void mlp_forward_split(const DevModel& m, const float* w, const float* xs, float* A, int wave, int nwaves, int lane,
                                                  float* __restrict__ zrec = nullptr, int zld = 0) {
    const int c = lane & 15, kq = lane >> 4;
    const u32x4* sf = reinterpret_cast<const u32x4*>(m.sf);
    for (int l = 0; l < m.n_layers; l++) {
        const int ni = m.sizes[l], no = m.sizes[l + 1];
        const int nmt = (no + 15) >> 4, nS = (ni + 31) >> 5, ngrp = (nmt + T16_TG - 1) / T16_TG;
        const int act = m.acts[l];
        for (int job = wave; job < ngrp * m.n_nets; job += nwaves) {
            const int net = job / ngrp, mt0 = (job - net * ngrp) * T16_TG;
            const float* bl = w + (size_t)net * m.net_size + m.b_off[l];
            const float* in = (l == 0) ? xs + c * m.ld_x : A + (net * CT + c) * m.ld_a + m.act_off[l - 1];
            f32x4 acc[T16_TG];
#pragma unroll
            for (int t = 0; t < T16_TG; t++) acc[t] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            const u32x4* ap = sf + (size_t)net * m.sf_net + m.sf_off[l] + (size_t)mt0 * nS * 3 * 64 + lane;
            // the A planes run TWO tiles ahead of their products (L2 latency under the other waves' and this wave's MFMAs); tiles past the layer's last
            // one read the last tile's planes again (never used)
            const int ntl = min(T16_TG, nmt - mt0);
            auto ldA = [&](int q) {                      // q = S * T16_TG + t, clamped
                const int S = min(q / T16_TG, nS - 1), t = min(q % T16_TG, ntl - 1);
                const u32x4* a = ap + ((size_t)t * nS + S) * 3 * 64;
                Bf3 r;
                r.h = a[0]; r.m = a[64]; r.l = a[128];
                return r;
            };
            Bf3 A0 = ldA(0), A1_ = ldA(1);
            T16Row8 rown = t16_row_load8(in + 8 * kq);
            for (int S = 0; S < nS; S++) {
                const Bf3 B = t16_row_split8(rown);
                rown = t16_row_load8(in + 32 * min(S + 1, nS - 1) + 8 * kq);
#pragma unroll
                for (int t = 0; t < T16_TG; t++) {
                    const Bf3 Aop = A0;
                    A0 = A1_;
                    A1_ = ldA(S * T16_TG + t + 2);
                    if (t < ntl) acc[t] = t16_mfma_bf3(Aop, B, acc[t]);
                }
            }
#pragma unroll
            for (int t = 0; t < T16_TG; t++) {
                const int mt = mt0 + t;
                if (mt >= nmt) continue;
                const int ro = (net * CT + c) * m.ld_a + m.act_off[l];
                float zv[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = mt * 16 + 4 * kq + r;
                    zv[r] = acc[t][r] + bl[min(row, no - 1)];
                    if (row < no) A[ro + row] = dev_act(act, zv[r]);
                }
                if (zrec && l + 1 < m.n_layers) {
                    float* zo = zrec + c * zld + net * m.act_off[m.n_layers - 1] + m.act_off[l] + mt * 16 + 4 * kq;
                    if (mt * 16 + 4 * kq + 3 < no) *reinterpret_cast<float4*>(zo) = make_float4(zv[0], zv[1], zv[2], zv[3]);
                    else
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (mt * 16 + 4 * kq + r < no) zo[r] = zv[r];
                }
            }
        }
        __syncthreads();
    }
}

// backward pass, layers L-1 .. 1 on the bf16 pipe (the layer-0 pullback into xb — 6 row tiles, a sum over the nets — stays on the f32 chain: 3 % of the work)
__device__ __forceinline__ void mlp_backward_split(const DevModel& m, const PackInfo& pk, const float* __restrict__ wb, float* Z, float* xb, int wave, int nwaves, int lane) {
    const int c = lane & 15, jq = lane >> 4;
    const u32x4* sb = reinterpret_cast<const u32x4*>(m.sb);
    for (int l = m.n_layers - 1; l >= 1; l--) {
        const int ni = m.sizes[l], no = m.sizes[l + 1];
        const int nit = (ni + 15) >> 4, nS = (no + 31) >> 5, ngrp = (nit + T16_TG - 1) / T16_TG;
        const int actp = m.acts[l - 1];
        for (int job = wave; job < ngrp * m.n_nets; job += nwaves) {
            const int net = job / ngrp, it0 = (job - net * ngrp) * T16_TG;
            const float* dz = Z + (net * CT + c) * m.ld_a + m.act_off[l];
            f32x4 acc[T16_TG];
#pragma unroll
            for (int t = 0; t < T16_TG; t++) acc[t] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            const u32x4* ap = sb + (size_t)net * m.sb_net + m.sb_off[l] + (size_t)it0 * nS * 3 * 64 + lane;
            const int ntl = min(T16_TG, nit - it0);
            auto ldA = [&](int q) {
                const int S = min(q / T16_TG, nS - 1), t = min(q % T16_TG, ntl - 1);
                const u32x4* a = ap + ((size_t)t * nS + S) * 3 * 64;
                Bf3 r;
                r.h = a[0]; r.m = a[64]; r.l = a[128];
                return r;
            };
            Bf3 A0 = ldA(0), A1_ = ldA(1);
            T16Row8 rown = t16_row_load8(dz + 8 * jq);
            for (int S = 0; S < nS; S++) {
                const Bf3 B = t16_row_split8(rown);
                rown = t16_row_load8(dz + 32 * min(S + 1, nS - 1) + 8 * jq);
#pragma unroll
                for (int t = 0; t < T16_TG; t++) {
                    const Bf3 Aop = A0;
                    A0 = A1_;
                    A1_ = ldA(S * T16_TG + t + 2);
                    if (t < ntl) acc[t] = t16_mfma_bf3(Aop, B, acc[t]);
                }
            }
            const int ro = (net * CT + c) * m.ld_a + m.act_off[l - 1];
#pragma unroll
            for (int t = 0; t < T16_TG; t++) {
                if (it0 + t >= nit) continue;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = (it0 + t) * 16 + 4 * jq + r;
                    if (row < ni) Z[ro + row] = acc[t][r] * dev_act_grad(actp, Z[ro + row]);
                }
            }
        }
        __syncthreads();
    }
    {   // l = 0: xb += sum over nets of W_1^T dZ_1 (f32 chain from the packed image)
        const int ni = m.sizes[0], no = m.sizes[1];
        const int nit = (ni + 15) >> 4, nS = (no + 15) >> 4;
        for (int it = wave; it < nit; it += nwaves) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int net = 0; net < m.n_nets; net++) {
                const float* dz = Z + (net * CT + c) * m.ld_a + m.act_off[0];
                const float4* ap4 = reinterpret_cast<const float4*>(wb + (size_t)net * pk.pb_net + pk.pb_off[0]) + (size_t)it * nS * 64 + lane;
                acc = gemm_chain4<GU4>(ap4, dz + 4 * jq, nS, acc);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = it * 16 + 4 * jq + r;
                if (row < ni) xb[c * m.ld_x + row] += acc[r];
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// physics
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float filt3(const float* x, int i, int N) {   // (F x)[i], filtering_operators.jl:1-14
    if (i == 0) return 0.5f * (x[0] + x[1]);
    if (i == N - 1) return 0.5f * (x[N - 2] + x[N - 1]);
    return (x[i - 1] + x[i] + x[i + 1]) * (1.0f / 3.0f);
}
__device__ __forceinline__ float filt3T(const float* x, int j, int N) {  // (F^T x)[j]
    float s = 0.0f;
    for (int i = j - 1; i <= j + 1; i++)
        if (i >= 0 && i < N) s += x[i] * ((i == 0 || i == N - 1) ? 0.5f : (1.0f / 3.0f));
    return s;
}

__device__ __forceinline__ float wm_top_flux(const DevModel& m, const float* bc, float t) {
    if (!m.diurnal) return bc[5];
    // scalings.wT(Q sin(2π/86400 · tτ)/(αg)) — NDE_training.jl:73, data_containers.jl:135
    const float wq = bc[5] * sinf(6.283185307179586f / 86400.0f * (t * m.tau)) / m.alpha_g;
    return (wq - m.mu_wT) / m.sig_wT;
}

// (FaceGrad, fast_tanh and wm_face: pretrain_sample.h, shared with wm_pretrain_ens_kernel)

// k[c][:] = RHS(xs[c][:]).  A holds the nets' activations (last layer = interior fluxes).  Ends with a barrier.
__device__ void physics_forward(const DevModel& m, const float* xs, const float* A, float* F, float* Ri_l,
                                const float* bcl, float t, float* kk, int tid, int nth) {
    const int Nz = m.Nz, nf = Nz + 1, nout = Nz - 1;
    const int oo = m.act_off[m.n_layers - 1];
    if (m.model == COLNDE_MODEL_WIND_MIXING) {
        const float eps = m.inplace ? 0.0f : m.eps;
        if (m.mpp && m.smooth_Ri) {
            for (int it = tid; it < CT * nf; it += nth) {
                const int c = it / nf, f = it - c * nf;
                Ri_l[c * m.ld_f + f] = wm_face(m, xs + c * m.ld_x, f, eps).Ri;
            }
            __syncthreads();
        }
        for (int it = tid; it < CT * nf; it += nth) {
            const int c = it / nf, f = it - c * nf;
            const bool in = f >= 1 && f < Nz;
            const float* bc = bcl + c * 8;
            float Fk[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float* o = A + (k * CT + c) * m.ld_a + oo;
                float ov = 0.0f;
                if (in) ov = m.smooth_NN ? filt3(o, f - 1, nout) : o[f - 1];
                const float bb = bc[2 * k];
                const float bt = (k == 2) ? wm_top_flux(m, bc, t) : bc[2 * k + 1];
                Fk[k] = m.zero_w ? ov : (f == 0 ? bb : (f == Nz ? bt : ov));
                if (m.mpp && m.zero_w) {
                    if (f == 0) Fk[k] += bb - m.s0[k];
                    if (f == Nz) Fk[k] += (m.inplace && m.diurnal && k == 2) ? bt : bt - m.s0[k];
                }
            }
            if (m.mpp) {
                if (in) {
                    const FaceGrad g = wm_face(m, xs + c * m.ld_x, f, eps);
                    const float Ris = m.smooth_Ri ? filt3(Ri_l + c * m.ld_f, f, nf) : g.Ri;
                    const float th = fast_tanh((Ris - m.Ric) * m.inv_dRi);
                    const float nu = m.nu0 + m.nu_minus * (1.0f - th) * 0.5f;   // tanh_step, :54,:125
                    float nuT = nu / m.Pr;
                    if (m.inplace && m.ca) nuT = g.gu > 0.0f ? nu / m.Pr : m.kappa;  // training_postprocessing.jl:118-121
                    Fk[0] -= m.cs[0] * nu * g.gu;
                    Fk[1] -= m.cs[1] * nu * g.gv;
                    Fk[2] -= m.cs[2] * nuT * g.gT;
                }
            } else if (m.ca && in) {
                const float* x = xs + c * m.ld_x;
                const float gT = (x[2 * Nz + f] - x[2 * Nz + f - 1]) * (float)Nz;
                Fk[2] -= m.cs[2] * m.kappa * fminf(0.0f, gT);
            }
#pragma unroll
            for (int k = 0; k < 3; k++) F[(k * CT + c) * m.ld_f + f] = Fk[k];
        }
        __syncthreads();
        for (int it = tid; it < CT * Nz; it += nth) {
            const int c = it / Nz, i = it - c * Nz;
            const float* x = xs + c * m.ld_x;
            const float* F0 = F + (0 * CT + c) * m.ld_f;
            const float* F1 = F + (1 * CT + c) * m.ld_f;
            const float* F2 = F + (2 * CT + c) * m.ld_f;
            float* ko = kk + c * m.ld_x;
            ko[i] = -m.A[0] * (F0[i + 1] - F0[i]) + m.cor_u * (m.sig_v * x[Nz + i] + m.mu_v);
            ko[Nz + i] = -m.A[1] * (F1[i + 1] - F1[i]) - m.cor_v * (m.sig_u * x[i] + m.mu_u);
            ko[2 * Nz + i] = -m.A[2] * (F2[i + 1] - F2[i]);
        }
    } else {
        const bool ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE;
        for (int it = tid; it < CT * nf; it += nth) {
            const int c = it / nf, f = it - c * nf;
            const bool in = f >= 1 && f < Nz;
            const float* x = xs + c * m.ld_x;
            const float* o = A + c * m.ld_a + oo;
            const float wv = f == 0 ? bcl[c * 8] : (f == Nz ? bcl[c * 8 + 1] : o[f - 1]);
            float q = 0.0f;
            if (ca && in) q = fminf(0.0f, m.ca_K * (x[f] - x[f - 1]) * (float)Nz);
            F[c * m.ld_f + f] = wv - q;     // dT = -C Nz d(w - q)
        }
        __syncthreads();
        const float CN = m.C_fc * (float)Nz;
        for (int it = tid; it < CT * Nz; it += nth) {
            const int c = it / Nz, i = it - c * Nz;
            const float* Fw = F + c * m.ld_f;
            kk[c * m.ld_x + i] = -CN * (Fw[i + 1] - Fw[i]);
        }
    }
    __syncthreads();
}

// Pullback of the physics for cotangent dbar: writes xb (physics part) and dZ_L into Z's last-layer slot.
// gb: [3][CT][ld_f] scratch, Ri_l / Rib_l: [CT][ld_f] scratch.  Ends with a barrier.
// sw_mode (RKC2 only): the pullback of the convective-adjustment switch min(0, K dT/dz).  Within one stabilised step the stage
// Jacobians must share ONE switch pattern: the stage polynomials rely on cancellations that hold only for a common Jacobian, and
// with per-stage patterns the exact discrete adjoint of the recurrence grows without bound (1e12 .. 1e57 measured on the oracle,
// DESIGN §2).  0: evaluate the switch at this stage's state (RK4: exact discrete adjoint); 1: evaluate it and record it in Ri_l
// (the first stage of a step the backward sweep meets, Y_{s-1}); 2: use the recorded pattern.
__device__ void physics_vjp(const DevModel& m, const float* xs, const float* dbar, float* Z, float* xb, float* gb,
                            float* Ri_l, float* Rib_l, int tid, int nth, int sw_mode = 0) {
    const int Nz = m.Nz, nf = Nz + 1, nout = Nz - 1;
    const int L = m.n_layers;
    const int oo = m.act_off[L - 1];
    const int actL = m.acts[L - 1];
    if (m.model == COLNDE_MODEL_WIND_MIXING) {
        const float eps = m.eps;
        if (m.mpp && m.smooth_Ri) {
            for (int it = tid; it < CT * nf; it += nth) {
                const int c = it / nf, f = it - c * nf;
                Ri_l[c * m.ld_f + f] = wm_face(m, xs + c * m.ld_x, f, eps).Ri;
            }
            __syncthreads();
        }
        for (int it = tid; it < CT * nf; it += nth) {
            const int c = it / nf, f = it - c * nf;
            const bool in = f >= 1 && f < Nz;
            const float* db = dbar + c * m.ld_x;
            float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, ribs = 0.0f;
            if (in) {
                const float Fb0 = m.A[0] * (db[f] - db[f - 1]);
                const float Fb1 = m.A[1] * (db[Nz + f] - db[Nz + f - 1]);
                const float Fb2 = m.A[2] * (db[2 * Nz + f] - db[2 * Nz + f - 1]);
                if (m.mpp) {
                    const FaceGrad g = wm_face(m, xs + c * m.ld_x, f, eps);
                    const float Ris = m.smooth_Ri ? filt3(Ri_l + c * m.ld_f, f, nf) : g.Ri;
                    const float th = fast_tanh((Ris - m.Ric) * m.inv_dRi);
                    const float nu = m.nu0 + m.nu_minus * (1.0f - th) * 0.5f;
                    const float D0 = -Fb0, D1 = -Fb1, D2 = -Fb2;
                    g0 = D0 * m.cs[0] * nu;
                    g1 = D1 * m.cs[1] * nu;
                    g2 = D2 * m.cs[2] * nu / m.Pr;
                    const float nub = D0 * m.cs[0] * g.gu + D1 * m.cs[1] * g.gv + D2 * m.cs[2] * g.gT / m.Pr;
                    ribs = nub * (-m.nu_minus / (2.0f * m.dRi)) * (1.0f - th * th);
                    if (!m.smooth_Ri) {
                        g2 += fast_div(ribs * m.B, g.S2);
                        const float q = fast_div(ribs * -g.Ri, g.S2) * 2.0f;
                        g0 += q * m.sig_u * m.sig_u * (g.gu + eps);
                        g1 += q * m.sig_v * m.sig_v * (g.gv + eps);
                    }
                } else if (m.ca) {
                    const float* x = xs + c * m.ld_x;
                    const float gT = (x[2 * Nz + f] - x[2 * Nz + f - 1]) * (float)Nz;
                    bool on = gT < 0.0f;
                    if (sw_mode == 2) on = Ri_l[c * m.ld_f + f] != 0.0f;
                    if (sw_mode == 1) Ri_l[c * m.ld_f + f] = on ? 1.0f : 0.0f;
                    g2 = on ? -Fb2 * m.cs[2] * m.kappa : 0.0f;
                }
            }
            gb[(0 * CT + c) * m.ld_f + f] = g0;
            gb[(1 * CT + c) * m.ld_f + f] = g1;
            gb[(2 * CT + c) * m.ld_f + f] = g2;
            if (m.mpp && m.smooth_Ri) Rib_l[c * m.ld_f + f] = ribs;
        }
        __syncthreads();
        if (m.mpp && m.smooth_Ri) {
            for (int it = tid; it < CT * nf; it += nth) {
                const int c = it / nf, f = it - c * nf;
                if (f >= 1 && f < Nz) {
                    const FaceGrad g = wm_face(m, xs + c * m.ld_x, f, eps);
                    const float rib = filt3T(Rib_l + c * m.ld_f, f, nf);
                    gb[(2 * CT + c) * m.ld_f + f] += rib * m.B / g.S2;
                    const float q = rib * (-g.Ri / g.S2) * 2.0f;
                    gb[(0 * CT + c) * m.ld_f + f] += q * m.sig_u * m.sig_u * (g.gu + eps);
                    gb[(1 * CT + c) * m.ld_f + f] += q * m.sig_v * m.sig_v * (g.gv + eps);
                }
            }
            __syncthreads();
        }
        for (int it = tid; it < CT * Nz; it += nth) {
            const int c = it / Nz, i = it - c * Nz;
            const float* db = dbar + c * m.ld_x;
            float* xo = xb + c * m.ld_x;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float* g = gb + (k * CT + c) * m.ld_f;
                float v = (g[i] - g[i + 1]) * (float)Nz;          // transpose of Dᶠ; g[0] = g[Nz] = 0
                if (k == 0) v += -m.cor_v * m.sig_u * db[Nz + i];
                if (k == 1) v += m.cor_u * m.sig_v * db[i];
                xo[k * Nz + i] = v;
            }
            if (i < nout) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    float ob;
                    if (m.smooth_NN) {
                        ob = 0.0f;
                        for (int q = i - 1; q <= i + 1; q++)
                            if (q >= 0 && q < nout)
                                ob += m.A[k] * (db[k * Nz + q + 1] - db[k * Nz + q]) * ((q == 0 || q == nout - 1) ? 0.5f : (1.0f / 3.0f));
                    } else {
                        ob = m.A[k] * (db[k * Nz + i + 1] - db[k * Nz + i]);
                    }
                    const int zo = (k * CT + c) * m.ld_a + oo + i;
                    Z[zo] = ob * dev_act_grad(actL, Z[zo]);
                }
            }
        }
    } else {
        const bool ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE;
        const float CN = m.C_fc * (float)Nz;
        for (int it = tid; it < CT * nf; it += nth) {
            const int c = it / nf, f = it - c * nf;
            float g = 0.0f;
            if (ca && f >= 1 && f < Nz) {
                const float* x = xs + c * m.ld_x;
                const float* db = dbar + c * m.ld_x;
                const float wbf = CN * (db[f] - db[f - 1]);
                const float gT = (x[f] - x[f - 1]) * (float)Nz;
                bool on = gT < 0.0f;
                if (sw_mode == 2) on = Ri_l[c * m.ld_f + f] != 0.0f;
                if (sw_mode == 1) Ri_l[c * m.ld_f + f] = on ? 1.0f : 0.0f;
                g = on ? -wbf * m.ca_K : 0.0f;
            }
            gb[c * m.ld_f + f] = g;
        }
        __syncthreads();
        for (int it = tid; it < CT * Nz; it += nth) {
            const int c = it / Nz, i = it - c * Nz;
            const float* db = dbar + c * m.ld_x;
            const float* g = gb + c * m.ld_f;
            xb[c * m.ld_x + i] = (g[i] - g[i + 1]) * (float)Nz;
            if (i < nout) {
                const int zo = c * m.ld_a + oo + i;
                Z[zo] = CN * (db[i + 1] - db[i]) * dev_act_grad(actL, Z[zo]);
            }
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// flux-MLP pre-training: `train_NN` — wind_mixing/src/NN_training.jl:207-249 with predict_uw/vw/wT (:25-169) —
// and the T -> wT pre-training of free_convection/train_free_convection_nde.jl:186-216.  `Flux.train!(NN_loss, params, data, opt)`
// makes ONE ADAM update per data point, in order: an inherently serial chain of tiny dense products, so one workgroup walks the
// whole (shuffled) data set with the weights, moments and activations on chip / in L2, and only the per-pass loss leaves the GPU.
//     NN_flux = [b; NN(x); t]-style face vector minus the diffusive / adjustment flux of the state (independent of the weights)
//     loss    = mse(NN_flux, flux) + gradient_scaling * mse(D^c flux, D^c NN_flux)
// update = 0 evaluates the mean loss at fixed weights (`total_loss(training_data)`, :234-236).
// The per-sample chain (forward, loss, backward, update) and the LDS carving live in pretrain_sample.h, shared with fc_pretrain_ens_kernel
// (engine_fc_pretrain.hip: one workgroup per model of a free-convection ensemble); this kernel adds the wind-mixing closures of the face flux.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512)
pretrain_kernel(DevModel m, int flux_type, float* __restrict__ theta, float* __restrict__ mom, float* __restrict__ vel,
                const float* __restrict__ X, const float* __restrict__ BC, const float* __restrict__ Y, const int* __restrict__ order,
                int n_samples, float gs, float eta, float b1, float b2, float eps_adam, double bt1, double bt2, int update,
                float* __restrict__ loss_out, double* __restrict__ bt_out) {
    extern __shared__ __attribute__((aligned(16))) float pt_smem[];
    const int tid = threadIdx.x, nth = blockDim.x;
    const int Nz = m.Nz, nf = Nz + 1;
    const PtLds lds = pt_carve(m, pt_smem);
    const float* a0 = lds.a0;
    float* cf = lds.cf;
    const bool wm = m.model == COLNDE_MODEL_WIND_MIXING;
    const int k = wm ? flux_type : 2;
    double p1 = bt1, p2 = bt2;                 // running powers beta^t (uniform over the workgroup)
    float loss_sum = 0.0f;
    for (int s = 0; s < n_samples; s++) {
        const int idx = order ? order[s] : s;
        pt_load(m, lds, X, Y, idx, tid, nth);
        __syncthreads();
        // weight-independent part of the face flux: boundary faces and the diffusive / adjustment flux of the state
        for (int f = tid; f < nf; f += nth) {
            const float* bc = BC + (size_t)idx * m.n_bc;
            cf[f] = wm ? pt_wm_face_const(m, a0, bc, k, f, m.nu0, m.nu_minus, m.Ric, m.inv_dRi, m.inv_Pr) : pt_bc_face(bc, f, Nz);
        }
        // the per-sample chain of pretrain_sample.h: forward, loss and cotangent, backward, Flux ADAM on every parameter of this net
        const float* th = theta + (wm ? k * m.net_size : 0);
        pt_forward(m, lds, th, a0, tid, nth);
        loss_sum += pt_loss(m, lds, gs, tid, nth);
        if (!update) { __syncthreads(); continue; }
        pt_backward(m, lds, th, tid, nth);
        const float c1 = (float)(1.0 / (1.0 - p1)), c2 = (float)(1.0 / (1.0 - p2));
        float* tw = theta + (wm ? k * m.net_size : 0);
        float* tm = mom + (wm ? k * m.net_size : 0);
        float* tv = vel + (wm ? k * m.net_size : 0);
        pt_update<true>(m, lds, tw, tm, tv, a0, 0.0f, eta, b1, b2, eps_adam, c1, c2, tid, nth);
        p1 *= (double)b1;
        p2 *= (double)b2;
        __syncthreads();
    }
    if (tid == 0) {
        loss_out[0] = loss_sum;
        if (bt_out) { bt_out[0] = p1; bt_out[1] = p2; }
    }
}

hipError_t launch_pretrain(const DevModel& m, int flux_type, float* theta, float* mom, float* vel, const float* X, const float* BC,
                           const float* Y, const int* order, int n_samples, float gs, float eta, float b1, float b2, float eps,
                           double bt1, double bt2, int update, float* loss_out, double* bt_out, hipStream_t stream) {
    const size_t lds = pretrain_lds_bytes(m);
    if (lds > PRETRAIN_LDS_CAP) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pretrain_kernel, dim3(1), dim3(512), lds, stream, m, flux_type, theta, mom, vel, X, BC, Y, order, n_samples, gs, eta,
                       b1, b2, eps, bt1, bt2, update, loss_out, bt_out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// LDS carving (must match engine_tile16.h: lds_floats_*)
// ------------------------------------------------------------------------------------------------
extern __shared__ __attribute__((aligned(16))) float smem[];

__device__ __forceinline__ void load_bcs(const DevModel& m, const float* __restrict__ bcs, float* bcl, int col0,
                                         int n_col, int tid) {
    if (tid < CT * 8) {
        const int c = tid >> 3, q = tid & 7;
        const int col = min(col0 + c, n_col - 1);
        bcl[tid] = q < m.n_bc ? bcs[(size_t)col * m.n_bc + q] : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------
// single RHS evaluation (NDE / NDE! / ∂T∂t drop-in)
// ------------------------------------------------------------------------------------------------
// AG: the activation rows live in the workgroup's slab of m.ag (global memory) instead of LDS — see DevModel::ag
template <bool AG = false>
__global__ void __launch_bounds__(256) rhs_kernel(DevModel m, PackInfo pk, const float* __restrict__ w, const float* __restrict__ wf,
                           const float* __restrict__ x, const float* __restrict__ bcs, float t,
                           float* __restrict__ dx, float* __restrict__ flux, int n_col) {
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nth >> 6;
    float* xs = smem;
    float* kk = xs + CT * m.ld_x;
    float* A = AG ? m.ag + (size_t)blockIdx.x * m.n_nets * CT * m.ld_a : kk + CT * m.ld_x;
    float* F = AG ? kk + CT * m.ld_x : A + m.n_nets * CT * m.ld_a;
    float* Ri_l = F + 3 * CT * m.ld_f;
    float* bcl = Ri_l + CT * m.ld_f;
    const int total = (int)(bcl + CT * 8 - smem);
    for (int i = tid; i < total; i += nth) smem[i] = 0.0f;
    __syncthreads();
    const int col0 = blockIdx.x * CT;
    load_bcs(m, bcs, bcl, col0, n_col, tid);
    for (int it = tid; it < CT * m.ns; it += nth) {
        const int c = it / m.ns, i = it - c * m.ns;
        xs[c * m.ld_x + i] = x[(size_t)min(col0 + c, n_col - 1) * m.ns + i];
    }
    __syncthreads();
    if (AG && m.sf) mlp_forward_split(m, w, xs, A, wave, nwaves, lane);
    else mlp_forward<false, false>(m, pk, w, wf, xs, nullptr, A, wave, nwaves, lane);
    physics_forward(m, xs, A, F, Ri_l, bcl, t, kk, tid, nth);
    if (dx)
        for (int it = tid; it < CT * m.ns; it += nth) {
            const int c = it / m.ns, i = it - c * m.ns;
            if (col0 + c < n_col) dx[(size_t)(col0 + c) * m.ns + i] = kk[c * m.ld_x + i];
        }
    if (flux) {
        // predict_flux (NDE_training.jl:83-147): the face vectors the tendencies difference — NN flux minus the closure's diffusive flux, with the
        // boundary faces as the conditions say; free convection: [b; NN(T); t] (- min(0, K dT/dz): free_convection/src/solve.jl:32-46)
        const int nf = m.Nz + 1;
        for (int it = tid; it < CT * m.n_nets * nf; it += nth) {
            const int c = it / (m.n_nets * nf), r = it - c * m.n_nets * nf, k = r / nf, f = r - k * nf;
            if (col0 + c < n_col) flux[((size_t)(col0 + c) * m.n_nets + k) * nf + f] = F[(k * CT + c) * m.ld_f + f];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// forward solve: classical RK4, S sub-steps per save interval, state at save points -> sol,
// stage inputs of every step -> tape (read back by the adjoint kernel)
// ------------------------------------------------------------------------------------------------
template <bool WLDS, int NTH, bool RKC = false, bool AG = false>
__global__ void __launch_bounds__(NTH) forward_kernel(DevModel m, PackInfo pk, const float* __restrict__ w, const float* __restrict__ wf,
                               const float* __restrict__ x0, const float* __restrict__ bcs,
                               const float* __restrict__ save_times, int n_save, int substeps,
                               float* __restrict__ sol, float* __restrict__ tape, int n_col, float* __restrict__ ztape) {
#define T16_ENS 0
#define T16_AG_TILE (size_t)blockIdx.x
#include "t16_forward_body.inc"
#undef T16_AG_TILE
#undef T16_ENS
}

// Model k of a tile ensemble sees the DevModel of a single handle built with its constants: the copy in LDS gets the closure constants of row k of the
// device table (RtPhys, dRi and Pr in its pad floats) and the model's own plane images.  One thread, between two barriers of the caller.
__device__ __forceinline__ void t16_ens_patch_model(DevModel& ml, const T16Ens& en, size_t k) {
    const RtPhys ph = en.phys[k];
    ml.nu0 = ph.nu0; ml.nu_minus = ph.nu_minus; ml.Ric = ph.Ric; ml.inv_dRi = ph.inv_dRi; ml.inv_Pr = ph.inv_Pr; ml.c_rib = ph.c_rib;
    ml.dRi = ph.pad0; ml.Pr = ph.pad1;
    if (ml.sf) ml.sf += k * en.sf;
    if (ml.sb) ml.sb += k * en.sb;
}

// K models of a tile ensemble: grid (tiles of ONE model's columns, K).  Model k's raw weights, packed image, solution and tapes lie the T16Ens strides
// behind model 0's (its tiles index them with blockIdx.x exactly as a single handle's do); x0, bcs and the save times are shared.  The model description,
// with model k's constants, sits at the head of the LDS (as the adjoint keeps it) and the tile's arrays behind it; the rows of m.ag are K x gridDim.x
// slabs, tile blockIdx.x of model k in slab k * gridDim.x + blockIdx.x — none shared between two workgroups.
template <bool WLDS, int NTH, bool RKC, bool AG>
__global__ void __launch_bounds__(NTH) forward_ens_kernel(DevModel m_arg, PackInfo pk, const float* __restrict__ w, const float* __restrict__ wf,
                               const float* __restrict__ x0, const float* __restrict__ bcs,
                               const float* __restrict__ save_times, int n_save, int substeps,
                               float* __restrict__ sol, float* __restrict__ tape, int n_col, float* __restrict__ ztape, T16Ens en) {
    DevModel& m_lds = *reinterpret_cast<DevModel*>(::smem);
    for (int i = threadIdx.x; i < (int)(sizeof(DevModel) / 4); i += blockDim.x) ((int*)&m_lds)[i] = ((const int*)&m_arg)[i];
    __syncthreads();
    if (threadIdx.x == 0) t16_ens_patch_model(m_lds, en, blockIdx.y);
    __syncthreads();
    const DevModel& m = m_lds;
    float* const smem = ::smem + MODEL_FLOATS;
    w += blockIdx.y * en.w;
    wf += blockIdx.y * en.wf;
    if (sol) sol += blockIdx.y * en.sol;
    if (tape) tape += blockIdx.y * en.tape;
    if (ztape) ztape += blockIdx.y * en.ztape;
#define T16_ENS 1
#define T16_AG_TILE ((size_t)blockIdx.y * gridDim.x + blockIdx.x)
#include "t16_forward_body.inc"
#undef T16_AG_TILE
#undef T16_ENS
}

// ------------------------------------------------------------------------------------------------
// loss value only (no gradient): per-tile partial sums of the six squared-error terms
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void loss_inject(const DevModel& m, const float* __restrict__ sol,
                                            const float* __restrict__ truth, size_t base, int i,
                                            const float* w6, float& lam, float* sums) {
    // base = offset of (column, save point) row; i = index inside the row
    const int Nz = m.Nz;
    const float d = sol[base + i] - truth[base + i];
    if (m.model != COLNDE_MODEL_WIND_MIXING) {
        sums[2] += d * d;
        lam += 2.0f * w6[2] * d;
        return;
    }
    const int k = i / Nz, f = i - k * Nz;
    sums[k] += d * d;
    float add = 2.0f * w6[k] * d;
    // gradient terms: Dᶠ rows 1..Nz-1 (the two zero rows only enter the mean's denominator) — loss.jl:9
    float glo = 0.0f, ghi = 0.0f;
    if (f >= 1) glo = (d - (sol[base + i - 1] - truth[base + i - 1])) * (float)Nz;
    if (f + 1 < Nz) ghi = ((sol[base + i + 1] - truth[base + i + 1]) - d) * (float)Nz;
    sums[3 + k] += glo * glo;
    add += 2.0f * w6[3 + k] * (glo - ghi) * (float)Nz;
    lam += add;
}

__device__ __forceinline__ void block_reduce_sums(float* sums, int nq, float* red, float* out, int tid, int nth) {
    // red: LDS scratch [nwaves][8]; out: global [8]
    const int lane = tid & 63, wave = tid >> 6;
    for (int q = 0; q < nq; q++) {
        float v = sums[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) red[wave * 8 + q] = v;
    }
    __syncthreads();
    if (tid < nq) {
        float v = 0.0f;
        for (int wv = 0; wv < (nth >> 6); wv++) v += red[wv * 8 + tid];
        out[tid] = v;
    }
}

__global__ void loss_kernel(DevModel m, const float* __restrict__ sol, const float* __restrict__ truth, int n_save,
                            int n_col, float* __restrict__ partial /* [gridDim.x][8] */, size_t sol_mstride) {
    sol += (size_t)blockIdx.y * sol_mstride;              // ensembles: blockIdx.y = model (its solution and partial rows; truth shared)
    partial += (size_t)blockIdx.y * gridDim.x * 8;
    __shared__ float red[16 * 8];
    const int tid = threadIdx.x, nth = blockDim.x;
    float sums[6] = {0, 0, 0, 0, 0, 0};
    const float w6[6] = {0, 0, 0, 0, 0, 0};
    const size_t rows = (size_t)n_col * n_save;
    for (size_t row = blockIdx.x; row < rows; row += gridDim.x)
        for (int i = tid; i < m.ns; i += nth) {
            float dummy = 0.0f;
            loss_inject(m, sol, truth, row * m.ns, i, w6, dummy, sums);
        }
    block_reduce_sums(sums, 6, red, partial + (size_t)blockIdx.x * 8, tid, nth);
}

// The member loss of an ensemble (colnde_ensemble_set_member_loss): loss_kernel's sums with the column's weight of the member, colw[model][column].
// The weighted difference cw d is formed first and the sums take (cw d) d and (cw glo) glo: a weight of 1 gives loss_kernel's bits.  Same rows per
// workgroup, same order, no atomics.
__global__ void loss_member_kernel(DevModel m, const float* __restrict__ sol, const float* __restrict__ truth, int n_save,
                                   int n_col, float* __restrict__ partial /* [gridDim.x][8] */, size_t sol_mstride, const float* __restrict__ colw) {
    sol += (size_t)blockIdx.y * sol_mstride;
    partial += (size_t)blockIdx.y * gridDim.x * 8;
    colw += (size_t)blockIdx.y * n_col;
    __shared__ float red[16 * 8];
    const int tid = threadIdx.x, nth = blockDim.x;
    const int Nz = m.Nz;
    const bool wm = m.model == COLNDE_MODEL_WIND_MIXING;
    float sums[6] = {0, 0, 0, 0, 0, 0};
    const size_t rows = (size_t)n_col * n_save;
    for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const float cw = colw[row / n_save];
        const size_t base = row * m.ns;
        for (int i = tid; i < m.ns; i += nth) {
            const float d = sol[base + i] - truth[base + i];
            const float dw = cw * d;
            if (!wm) { sums[2] += dw * d; continue; }
            const int k = i / Nz, f = i - k * Nz;
            sums[k] += dw * d;
            if (f >= 1) {
                const float glo = (d - (sol[base + i - 1] - truth[base + i - 1])) * (float)Nz;
                sums[3 + k] += (cw * glo) * glo;
            }
        }
    }
    block_reduce_sums(sums, 6, red, partial + (size_t)blockIdx.x * 8, tid, nth);
}

// ------------------------------------------------------------------------------------------------
// adjoint: back-propagation through the RK4 steps, replaying the stage-input tape
// ------------------------------------------------------------------------------------------------
// TAPEDW: the weight gradients are not accumulated here.  Each stage's layer inputs and deltas are written to `dwtape` as
// [tile][step][stage][CT columns][xs | A of every net | dZ of every net] and contracted by dw_gemm_kernel (networks whose
// weight-gradient tiles would not fit the register file: 64-256-256-63 has 384 of them).
template <int MAXT, int NTH, int MAXR, bool WLDS, bool TAPEDW = false, bool RKC = false, bool AG = false>
__global__ void __launch_bounds__(NTH, (TAPEDW && NTH == 512) ? 4 : 1)   // taped mode, 512 threads: 128 registers, so that TWO workgroups share a CU and one's GEMMs cover the other's tape traffic
adjoint_kernel(DevModel m_arg, PackInfo pk, const float* __restrict__ w, const float* __restrict__ wf,
               const float* __restrict__ wb, const TileDesc* __restrict__ tiles, const int* __restrict__ bias_zoff,
               const int* __restrict__ bias_goff, const float* __restrict__ bcs, const float* __restrict__ save_times,
               int n_save, int substeps, const float* __restrict__ sol, const float* __restrict__ truth,
               const float* __restrict__ tape, LossWeights lw, float* __restrict__ slab /* [grid][n_params+8] */,
               int n_col, float* __restrict__ dwtape = nullptr, const float* __restrict__ ztape = nullptr) {
#define T16_ENS 0
#define T16_AG_TILE (size_t)blockIdx.x
#include "t16_adjoint_body.inc"
#undef T16_AG_TILE
#undef T16_ENS
}

// K models of a tile ensemble, taped dW at 1,024 threads: grid (tiles of ONE model's columns, K).  Model k's weights, images, solution, the three tapes and
// its slab rows lie the T16Ens strides behind model 0's; bcs, truth, the save times and the bias tables are shared (no in-register dW tiles: no TileDesc).
// The body patches model k's constants and plane images into its LDS copy of the description (T16_ENS) and takes the delta rows of slab
// k * gridDim.x + blockIdx.x of m.ag.
template <int MAXR, bool WLDS, bool RKC, bool AG>
__global__ void __launch_bounds__(1024, 1)
adjoint_ens_kernel(DevModel m_arg, PackInfo pk, const float* __restrict__ w, const float* __restrict__ wf, const float* __restrict__ wb,
                   const int* __restrict__ bias_zoff, const int* __restrict__ bias_goff, const float* __restrict__ bcs,
                   const float* __restrict__ save_times, int n_save, int substeps, const float* __restrict__ sol, const float* __restrict__ truth,
                   const float* __restrict__ tape, LossWeights lw, float* __restrict__ slab, int n_col, float* __restrict__ dwtape,
                   const float* __restrict__ ztape, T16Ens en) {
    constexpr int MAXT = 1;
    constexpr bool TAPEDW = true;
    const TileDesc* const tiles = nullptr;
    w += blockIdx.y * en.w;
    wf += blockIdx.y * en.wf;
    wb += blockIdx.y * en.wb;
    sol += blockIdx.y * en.sol;
    tape += blockIdx.y * en.tape;
    slab += blockIdx.y * en.slab;
    dwtape += blockIdx.y * en.dwtape;
    ztape += blockIdx.y * en.ztape;
#define T16_ENS 1
#define T16_AG_TILE ((size_t)blockIdx.y * gridDim.x + blockIdx.x)
#include "t16_adjoint_body.inc"
#undef T16_AG_TILE
#undef T16_ENS
}

// ------------------------------------------------------------------------------------------------
// embedded inference: compute_neural_network_forcing! (double_gyre_nn.jl:149-168)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) infer_kernel(DevModel m, PackInfo pk, const float* __restrict__ w, const float* __restrict__ wf,
                             const float* __restrict__ T, const float* __restrict__ top_flux, float inv_dz,
                             float* __restrict__ out, int n_col) {
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nth >> 6;
    float* xs = smem;
    float* A = xs + CT * m.ld_x;
    const int total = CT * m.ld_x + m.n_nets * CT * m.ld_a;
    for (int i = tid; i < total; i += nth) smem[i] = 0.0f;
    __syncthreads();
    const int Nz = m.Nz;
    const int oo = m.act_off[m.n_layers - 1];
    for (int tile = blockIdx.x; tile * CT < n_col; tile += gridDim.x) {
        const int col0 = tile * CT;
        for (int it = tid; it < CT * Nz; it += nth) {
            const int c = it / Nz, i = it - c * Nz;
            const float Tm = T[(size_t)min(col0 + c, n_col - 1) * Nz + i];
            xs[c * m.ld_x + i] = ((19.65f + Tm / 20.0f) - m.mu_T) / m.sig_T;      // :156, T_scaling :158
        }
        __syncthreads();
        mlp_forward<false, false>(m, pk, w, wf, xs, nullptr, A, wave, nwaves, lane);
        for (int it = tid; it < CT * Nz; it += nth) {
            const int c = it / Nz, i = it - c * Nz;
            if (col0 + c < n_col) {
                const float* o = A + c * m.ld_a + oo;
                const float lo = i == 0 ? 0.0f : m.sig_wT * o[i - 1] + m.mu_wT;           // enforce_fluxes(·, 0, surface) :160
                const float hi = i == Nz - 1 ? top_flux[col0 + c] : m.sig_wT * o[i] + m.mu_wT;
                out[(size_t)(col0 + c) * Nz + i] = -(hi - lo) * inv_dz;                    // forcing = -∂z wT :135
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers (declared in engine_tile16.h)
// ------------------------------------------------------------------------------------------------
// Kernel selection (kernel_select.h): per kernel family ONE table or selector names the instantiations; the launcher
// takes its kernel from it and set_kernel_attributes() walks it, so whatever can be launched has had its dynamic-LDS limit raised.
// To add an instantiation, add it there.
//
// adjoint_kernel: a geometry (threads, dW tiles per wave, state items per thread, weights in LDS) and its kernels, [0] RK4, [1] RKC2
using AdjointFn = decltype(&adjoint_kernel<16, 512, 3, true>);
struct AdjointInst { AdjointGeom g; AdjointFn k[2]; };
template <int MT, int NT, int MR, bool WL, bool TD = false, bool AG = false>
static constexpr AdjointInst adj_inst() {
    return {{NT, MT, MR, WL}, {adjoint_kernel<MT, NT, MR, WL, TD, false, AG>, adjoint_kernel<MT, NT, MR, WL, TD, true, AG>}};
}
// in-kernel dW: the host picks the first that fits (pick_adjoint_geom)
static const AdjointInst kGeoms[] = {adj_inst<16, 512, 3, true>(), adj_inst<32, 256, 6, true>(), adj_inst<32, 256, 6, false>(),
                                     adj_inst<32, 256, 12, false>(), adj_inst<32, 512, 6, false>(), adj_inst<48, 512, 3, false>()};
// taped dW (launch_adjoint chooses); the last: rows in global memory (DevModel::ag)
enum { TAPED_1024_WLDS, TAPED_1024, TAPED_512_R3, TAPED_512_R6, TAPED_AG };
static const AdjointInst kTapedGeoms[] = {adj_inst<1, 1024, 2, true, true>(), adj_inst<1, 1024, 2, false, true>(), adj_inst<1, 512, 3, false, true>(),
                                          adj_inst<1, 512, 6, false, true>(), adj_inst<1, 1024, 2, false, true, true>()};
static_assert(sizeof(kTapedGeoms) / sizeof(kTapedGeoms[0]) == TAPED_AG + 1, "one entry per TAPED_* index");

// forward_kernel<WLDS, NTH, RKC, AG>; nullptr: no such kernel (AG, rows in global memory: weights streamed from L2, 256 or 1,024 threads)
using ForwardFn = decltype(&forward_kernel<false, 256>);
static ForwardFn forward_pick(bool wlds, int nthreads, bool rkc, bool ag) {
    ForwardFn k = nullptr;
    with_bools([&](auto WL, auto RK, auto AG) {
        constexpr bool wl = decltype(WL)::value, rk = decltype(RK)::value, g = decltype(AG)::value;
        if constexpr (!(wl && g)) {
            if (nthreads == 256) k = forward_kernel<wl, 256, rk, g>;
            if (nthreads == 1024) k = forward_kernel<wl, 1024, rk, g>;
            if constexpr (!g) if (nthreads == 512) k = forward_kernel<wl, 512, rk, g>;
        }
    }, wlds, rkc, ag);
    return k;
}
static auto rhs_pick(bool ag) { return ag ? rhs_kernel<true> : rhs_kernel<false>; }

size_t lds_floats_adjoint_geom(const DevModel& m, const AdjointGeom& g) {
    return MODEL_FLOATS + lds_floats_adjoint(m) + (g.wlds ? (size_t)((m.n_params + 3) & ~3) + 128 : 0);
}

bool pick_adjoint_geom(const DevModel& m, AdjointGeom* geo, int force) {
    const size_t cap = 160 * 1024;
    int idx = 0;
    for (const AdjointInst& inst : kGeoms) {
        const AdjointGeom& g = inst.g;
        const int nwaves = g.nthreads / 64;
        const bool fits = m.n_tiles <= g.maxt * nwaves && CT * m.ns <= g.maxr * g.nthreads && m.n_bias <= MAXB * g.nthreads &&
                          lds_floats_adjoint_geom(m, g) * sizeof(float) <= cap;
        if (fits && (force < 0 || force == idx)) {
            *geo = g;
            return true;
        }
        idx++;
    }
    return false;
}

// The taped-dW adjoint's geometry for a launch of n_tiles tiles (a TAPED_* index, -1: none) and, in *lds_bytes, the LDS it takes: decided here for a
// single handle and for a tile ensemble alike — the ensemble asks with the tiles of ONE model, so that model k runs the kernel form a single handle of
// its columns runs.
static int pick_taped_geom(const DevModel& m, int n_tiles, bool have_ztape, size_t* lds_bytes) {
    if (m.ag) {
        // rows in global memory (wide networks): the Z tape is required (no A array), 1,024 threads (n_bias <= MAXB * 1,024, CT * ns <= 2 * 1,024: checked by the host)
        if (!have_ztape || CT * m.ns > 2 * 1024 || m.n_bias > MAXB * 1024) return -1;
        return TAPED_AG;
    }
    // Two 512-thread workgroups per CU (128 registers each) when two fit in the LDS: one's GEMMs then cover the other's tape
    // traffic, activations and physics (32-128-128-31: adjoint 84.6 -> 61.6 ms); one 1,024-thread workgroup (four waves per SIMD)
    // otherwise.  COLNDE_T16_TAPE_THREADS=512|1024 forces either.
    const char* et = getenv("COLNDE_T16_TAPE_THREADS");
    const int nth_env = et ? atoi(et) : ((n_tiles > 256 && 2 * *lds_bytes + 2048 <= 160 * 1024) ? 512 : 1024);   // (fewer tiles than CUs: a latency point, the wider workgroup finishes sooner)
    // latency points (fewer tiles than CUs) with a network that fits beside the tile's arrays: the raw weights staged in LDS, read in
    // place for W^T — no L2 round trip at the head of every backward chain (8 simulations: adjoint 29.3 -> 25.0 ms)
    const size_t wl_bytes = ((size_t)((m.n_params + 3) & ~3) + 128) * sizeof(float);
    const char* ew = getenv("COLNDE_T16_TAPE_WLDS");
    const bool wlds_ok = nth_env == 1024 && CT * m.ns <= 2 * 1024 && *lds_bytes + wl_bytes <= 160 * 1024;
    if (wlds_ok && (ew ? atoi(ew) != 0 : n_tiles <= 256)) { *lds_bytes += wl_bytes; return TAPED_1024_WLDS; }
    if (nth_env == 1024 && CT * m.ns <= 2 * 1024) return TAPED_1024;
    if (CT * m.ns <= 3 * 512) return TAPED_512_R3;
    if (CT * m.ns <= 6 * 512) return TAPED_512_R6;
    return -1;
}

// ---- tile ensembles: the instantiations an ensemble can reach — both steppers; weights in LDS or streamed; rows in LDS or in global memory (whose arithmetic
// is a runtime switch, DevModel::sf / sb).  No in-register adjoint geometry and no 512-thread taped one.
using ForwardEnsFn = decltype(&forward_ens_kernel<false, 256, false, false>);
static ForwardEnsFn forward_ens_pick(bool wlds, int nthreads, bool rkc, bool ag) {
    ForwardEnsFn k = nullptr;
    with_bools([&](auto RK) {
        constexpr bool rk = decltype(RK)::value;
        if (wlds && !ag && nthreads == 1024) k = forward_ens_kernel<true, 1024, rk, false>;
        if (!wlds && !ag && nthreads == 256) k = forward_ens_kernel<false, 256, rk, false>;
        if (!wlds && ag && nthreads == 1024) k = forward_ens_kernel<false, 1024, rk, true>;
    }, rkc);
    return k;
}
bool forward_ens_has(bool wlds, int nthreads, bool ag) { return forward_ens_pick(wlds, nthreads, false, ag) != nullptr; }
using AdjointEnsFn = decltype(&adjoint_ens_kernel<2, true, false, false>);
static AdjointEnsFn adjoint_ens_pick(int taped_geom, bool rkc) {      // by TAPED_* index
    AdjointEnsFn k = nullptr;
    with_bools([&](auto RK) {
        constexpr bool rk = decltype(RK)::value;
        if (taped_geom == TAPED_1024_WLDS) k = adjoint_ens_kernel<2, true, rk, false>;
        if (taped_geom == TAPED_1024) k = adjoint_ens_kernel<2, false, rk, false>;
        if (taped_geom == TAPED_AG) k = adjoint_ens_kernel<2, false, rk, true>;
    }, rkc);
    return k;
}

bool adjoint_ens_has(const DevModel& m, int n_tiles, size_t lds_bytes) {
    const int g = pick_taped_geom(m, n_tiles, true, &lds_bytes);
    return g >= 0 && adjoint_ens_pick(g, false) != nullptr;
}

hipError_t launch_pack_ens(const DevModel& m, const PackInfo& pk, const float* w, float* wf, float* wb, const T16Ens& en, hipStream_t stream) {
    const int total = (pk.pf_net + pk.pb_net) * m.n_nets;
    hipLaunchKernelGGL(pack_weights_ens_kernel, dim3((total + 255) / 256, en.n_models), dim3(256), 0, stream, m, pk, w, wf, wb, en);
    return hipGetLastError();
}

hipError_t launch_pack_planes_ens(const DevModel& m, const float* w, unsigned* sf, unsigned* sb, const T16Ens& en, hipStream_t stream) {
    const long total = ((long)m.sf_net + m.sb_net) * m.n_nets;
    hipLaunchKernelGGL(pack_planes_ens_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 65535), en.n_models), dim3(256), 0, stream, m, w, sf, sb, en);
    return hipGetLastError();
}

hipError_t launch_forward_ens(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* x0, const float* bcs,
                              const float* save_times, int n_save, int substeps, float* sol, float* tape, int n_col, int nthreads, bool wlds,
                              size_t lds_bytes, const T16Ens& en, hipStream_t stream, float* ztape) {
    const auto k = forward_ens_pick(wlds, nthreads, m.rkc != nullptr, m.ag != nullptr);
    if (!k || !en.phys || en.n_models < 1 || en.n_models > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3((n_col + CT - 1) / CT, en.n_models), dim3(nthreads), lds_bytes + t16_ens_forward_lds_extra(), stream, m, pk, w, wf, x0, bcs, save_times,
                       n_save, substeps, sol, tape, n_col, ztape, en);
    return hipGetLastError();
}

hipError_t launch_adjoint_ens(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* wb, const int* bias_zoff,
                              const int* bias_goff, const float* bcs, const float* save_times, int n_save, int substeps, const float* sol,
                              const float* truth, const float* tape, const LossWeights& lw, float* slab, int n_col, size_t lds_bytes,
                              const T16Ens& en, hipStream_t stream, float* dwtape, const float* ztape) {
    if (!dwtape || !ztape || !tape || !en.phys || en.n_models < 1 || en.n_models > 65535) return hipErrorInvalidValue;
    const int n_tiles = (n_col + CT - 1) / CT;               // of ONE model: the geometry a single handle of n_col columns runs
    size_t lds = lds_bytes;
    const int g = pick_taped_geom(m, n_tiles, true, &lds);
    const auto k = g < 0 ? nullptr : adjoint_ens_pick(g, m.rkc != nullptr);
    if (!k) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3(n_tiles, en.n_models), dim3(1024), lds, stream, m, pk, w, wf, wb, bias_zoff, bias_goff, bcs, save_times, n_save, substeps, sol, truth,
                       tape, lw, slab, n_col, dwtape, ztape, en);
    return hipGetLastError();
}

hipError_t launch_pack(const DevModel& m, const PackInfo& pk, const float* w, float* wf, float* wb, hipStream_t stream) {
    const int total = (pk.pf_net + pk.pb_net) * m.n_nets;
    hipLaunchKernelGGL(pack_weights_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, m, pk, w, wf, wb);
    return hipGetLastError();
}

hipError_t launch_pack_planes(const DevModel& m, const float* w, unsigned* sf, unsigned* sb, hipStream_t stream) {
    const long total = ((long)m.sf_net + m.sb_net) * m.n_nets;
    hipLaunchKernelGGL(pack_planes_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 65535)), dim3(256), 0, stream, m, w, sf, sb);
    return hipGetLastError();
}

hipError_t launch_rhs(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* x,
                      const float* bcs, float t, float* dx, int n_col, int nthreads, size_t lds_bytes, hipStream_t stream, float* flux) {
    hipLaunchKernelGGL(rhs_pick(m.ag != nullptr), dim3((n_col + CT - 1) / CT), dim3(nthreads), lds_bytes, stream, m, pk, w, wf, x, bcs, t, dx, flux, n_col);
    return hipGetLastError();
}

hipError_t launch_forward(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* x0,
                          const float* bcs, const float* save_times, int n_save, int substeps, float* sol, float* tape,
                          int n_col, int nthreads, bool wlds, size_t lds_bytes, hipStream_t stream, float* ztape) {
    const dim3 grid((n_col + CT - 1) / CT);
    // rows in global memory (wide networks): weights streamed from L2; 1,024 threads (four waves per SIMD hide the row loads) or 256
    if (m.ag && (wlds || (nthreads != 256 && nthreads != 1024))) return hipErrorInvalidValue;
    const auto k = forward_pick(wlds, nthreads, m.rkc != nullptr, m.ag != nullptr);
    if (!k) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, grid, dim3(nthreads), lds_bytes, stream, m, pk, w, wf, x0, bcs, save_times, n_save, substeps, sol, tape, n_col, ztape);
    return hipGetLastError();
}

hipError_t launch_loss(const DevModel& m, const float* sol, const float* truth, int n_save, int n_col, float* partial,
                       int n_blocks, hipStream_t stream, int n_models, size_t sol_mstride) {
    hipLaunchKernelGGL(loss_kernel, dim3(n_blocks, n_models), dim3(256), 0, stream, m, sol, truth, n_save, n_col, partial, sol_mstride);
    return hipGetLastError();
}

hipError_t launch_loss_member(const DevModel& m, const float* sol, const float* truth, int n_save, int n_col, float* partial,
                              int n_blocks, hipStream_t stream, int n_models, size_t sol_mstride, const float* colw) {
    if (!colw) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loss_member_kernel, dim3(n_blocks, n_models), dim3(256), 0, stream, m, sol, truth, n_save, n_col, partial, sol_mstride, colw);
    return hipGetLastError();
}

hipError_t launch_adjoint(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* wb,
                          const TileDesc* tiles, const int* bias_zoff, const int* bias_goff, const float* bcs,
                          const float* save_times, int n_save, int substeps, const float* sol, const float* truth,
                          const float* tape, const LossWeights& lw, float* slab, int n_col, const AdjointGeom& geo,
                          size_t lds_bytes, hipStream_t stream, float* dwtape, const float* ztape) {
    const int n_tiles = (n_col + CT - 1) / CT;
    auto launch = [&](const AdjointInst& a, size_t lds, float* dwt, const float* zt) {
        hipLaunchKernelGGL(a.k[m.rkc != nullptr], dim3(n_tiles), dim3(a.g.nthreads), lds, stream, m, pk, w, wf, wb, tiles, bias_zoff, bias_goff, bcs, save_times,
                           n_save, substeps, sol, truth, tape, lw, slab, n_col, dwt, zt);
        return hipGetLastError();
    };
    if (dwtape) {
        size_t lds = lds_bytes;
        const int g = pick_taped_geom(m, n_tiles, ztape != nullptr, &lds);
        return g < 0 ? hipErrorInvalidValue : launch(kTapedGeoms[g], lds, dwtape, ztape);
    }
    for (const AdjointInst& a : kGeoms)
        if (a.g.nthreads == geo.nthreads && a.g.maxt == geo.maxt && a.g.maxr == geo.maxr && !a.g.wlds == !geo.wlds) return launch(a, lds_bytes, nullptr, nullptr);
    return hipErrorInvalidValue;
}

hipError_t launch_infer(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* T,
                        const float* top_flux, float inv_dz, float* out, int n_col, int nthreads, size_t lds_bytes,
                        hipStream_t stream) {
    int n_tiles = (n_col + CT - 1) / CT;
    int grid = n_tiles < 2048 ? n_tiles : 2048;
    hipLaunchKernelGGL(infer_kernel, dim3(grid), dim3(nthreads), lds_bytes, stream, m, pk, w, wf, T, top_flux, inv_dz, out, n_col);
    return hipGetLastError();
}

hipError_t debug_read_stamps(unsigned long long* out16) {
#ifdef COLNDE_STAMPS
    hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 8);
    if (e != hipSuccess) return e;
    return hipMemcpyFromSymbol(out16 + 8, HIP_SYMBOL(g_fine), sizeof(unsigned long long) * 8);
#else
    for (int i = 0; i < 16; i++) out16[i] = 0;
    return hipSuccess;
#endif
}

hipError_t set_kernel_attributes(size_t max_lds_bytes) {
    hipError_t e = hipSuccess;
    auto set = [&](auto* k) { if (k && e == hipSuccess) e = set_max_lds(k, max_lds_bytes); };
    set(infer_kernel);
    set(pretrain_kernel);        // (deep or wide nets: above the 64 KB a kernel may take without the attribute)
    for (int ag = 0; ag < 2; ag++) set(rhs_pick(ag));
    for (int rkc = 0; rkc < 2; rkc++) {
        for (const AdjointInst& a : kGeoms) set(a.k[rkc]);
        for (const AdjointInst& a : kTapedGeoms) set(a.k[rkc]);
        for (int nthreads : {256, 512, 1024})
            for (int wlds = 0; wlds < 2; wlds++)
                for (int ag = 0; ag < 2; ag++) {
                    set(forward_pick(wlds, nthreads, rkc, ag));
                    set(forward_ens_pick(wlds, nthreads, rkc, ag));
                }
        for (int g = 0; g <= TAPED_AG; g++) set(adjoint_ens_pick(g, rkc));
    }
    return e;
}
