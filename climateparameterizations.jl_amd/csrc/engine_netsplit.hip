// engine_netsplit.hip — the net-split kernels of the static wind-mixing shape (gfx950 / CDNA4 only): the kernels of the LATENCY sizes.
// Engine AUTO up to 8,192 columns and every wind-mixing ensemble run these.  Such problems have fewer 32-column tiles than the GPU has SIMDs, so a
// 16-column tile is given to a whole workgroup instead: one wavefront per flux net — the three nets are independent given the state — plus a helper
// wavefront on the fourth SIMD for the Richardson-number closure (rt16sh_*; the three-wave forms rt16s_* are kept as independent implementations:
// COLNDE_T16_FWD_HELPER=0, COLNDE_T16_ADJ_HELPER=0).  Tapes and the dW GEMM are tile16's.  Tile layouts, chains and activations are regtile's (regtile_dev.h), the weight images
// engine_regtile.h's; the forward solve at the throughput sizes and its adjoint are in engine_regtile.hip.
//
// Reference arithmetic: wind_mixing/src/NDE_training.jl:46-165 (NDE, predict_flux, predict_NDE).
#include "engine_netsplit.h"
#include "engine_tile16.h"   // t16_ztape_col_floats: the pre-activation tape this unit's kernels share with tile16
#include "regtile_dev.h"
#include "kernel_select.h"

// ------------------------------------------------------------------------------------------------
// bf16 operand images (COLNDE_MATRIX_BF16X3_EXACT), made from the fp32 image of rt_pack_kernel: the exact three-way truncation split of each weight
// ------------------------------------------------------------------------------------------------
// The adjoint's W1_n^T products (RT_NSA_*: rt16sh_adjoint_kernel<ACT, RICH, false, true>): group G = (n * 2 + kb) * 6 + tile, lane (i, kq),
// element e <-> W1_n[feature 4 (8 kb + e) + kq][x index 16 tile + i] (zero beyond feature 49); planes h, m interleaved per group, plane l behind them
__global__ void rt_pack_split_nsadj_kernel(const float* __restrict__ img, unsigned* __restrict__ simg, int img_stride) {
    img += (size_t)blockIdx.y * img_stride;                 // ensembles: blockIdx.y = model
    simg += (size_t)blockIdx.y * img_stride;
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < 36 * 256; x += gridDim.x * blockDim.x) {
        const int G = x >> 8, lane = (x >> 2) & 63, pr = x & 3;
        const int n = G / 12, kb = (G / 6) & 1, tile = G % 6, i = lane & 15, kq = lane >> 4;
        float v[2];
#pragma unroll
        for (int z = 0; z < 2; z++) {
            const int f = 4 * (8 * kb + 2 * pr + z) + kq;
            v[z] = f < 50 ? img[RT_W1C + (n * 50 + f) * RT_LD1 + 16 * tile + i] : 0.0f;
        }
        const float r0 = v[0] - __uint_as_float(__float_as_uint(v[0]) & 0xffff0000u), r1 = v[1] - __uint_as_float(__float_as_uint(v[1]) & 0xffff0000u);
        const float l0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u), l1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
        simg[(size_t)(G * 2 + 0) * 256 + lane * 4 + pr] = (__float_as_uint(v[1]) & 0xffff0000u) | (__float_as_uint(v[0]) >> 16);
        simg[(size_t)(G * 2 + 1) * 256 + lane * 4 + pr] = (__float_as_uint(r1) & 0xffff0000u) | (__float_as_uint(r0) >> 16);
        simg[RT_NSA_L + (size_t)G * 256 + lane * 4 + pr] = (__float_as_uint(l1) & 0xffff0000u) | (__float_as_uint(l0) >> 16);
    }
}

// The forward kernel (RT_SIMG2_*): layer 1 per net (tiles of that kernel: quad Q = 4 t + (i & 3) of the net's 13, feature
// 4 Q + (i >> 2)), layer 2 as in rt_pack_split_kernel, and the 8 live lanes of each net's fourth layer-1 tile (quad 12: features 48, 49 -> rows i = 0, 4)
__global__ void rt_pack_split_ns_kernel(const float* __restrict__ img, unsigned* __restrict__ simg, int img_stride) {
    img += (size_t)blockIdx.y * img_stride;                 // ensembles: blockIdx.y = model
    simg += (size_t)blockIdx.y * img_stride;
    auto put = [&](unsigned* o, int plane_stride, float v0, float v1) {
        const float r0 = v0 - __uint_as_float(__float_as_uint(v0) & 0xffff0000u), r1 = v1 - __uint_as_float(__float_as_uint(v1) & 0xffff0000u);
        const float l0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u), l1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
        o[0] = (__float_as_uint(v1) & 0xffff0000u) | (__float_as_uint(v0) >> 16);
        o[plane_stride] = (__float_as_uint(r1) & 0xffff0000u) | (__float_as_uint(r0) >> 16);
        o[2 * plane_stride] = (__float_as_uint(l1) & 0xffff0000u) | (__float_as_uint(l0) >> 16);
    };
    const int n_full = 39 * 256, n_t3 = 9 * 8 * 4;
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < n_full + n_t3 + 4; x += gridDim.x * blockDim.x) {
        if (x >= n_full + n_t3) { simg[RT_SIMG2_ZERO + x - n_full - n_t3] = 0u; continue; }
        float v[2];
        if (x < n_full) {
            const int G = x >> 8, lane = (x >> 2) & 63, pr = x & 3;
            const int i = lane & 15, kg = lane >> 4, g_i = i >> 2, r_i = i & 3;
#pragma unroll
            for (int z = 0; z < 2; z++) {
                const int e = 2 * pr + z;
                float w = 0.0f;
                if (G < 27) {
                    const int n = G / 9, t = (G / 3) % 3, q = G % 3, f = 4 * (4 * t + r_i) + g_i;
                    const int lev = e < 4 ? 4 * kg + e : 16 + 4 * kg + (e - 4);
                    w = img[RT_W1C + (n * 50 + f) * RT_LD1 + 32 * q + lev];
                } else {
                    const int y = G - 27, n = y >> 2, u = (y >> 1) & 1, c = y & 1;
                    const int Q2 = 4 * u + r_i, qq = 8 * c + e, f = 4 * qq + kg;
                    if (Q2 < 5 && qq < 13 && f < 50) w = img[RT_W2C + (n * 20 + 4 * Q2 + g_i) * RT_LD2 + f];
                }
                v[z] = w;
            }
            put(simg + (size_t)G * 768 + lane * 4 + pr, 256, v[0], v[1]);
        } else {
            const int y = x - n_full, blk = y >> 5, l8 = (y >> 2) & 7, pr = y & 3;      // blk = n * 3 + q; l8 = g_i * 4 + kg
            const int n = blk / 3, q = blk % 3, g_i = l8 >> 2, kg = l8 & 3;
#pragma unroll
            for (int z = 0; z < 2; z++) {
                const int e = 2 * pr + z, lev = e < 4 ? 4 * kg + e : 16 + 4 * kg + (e - 4);
                v[z] = img[RT_W1C + (n * 50 + 48 + g_i) * RT_LD1 + 32 * q + lev];
            }
            put(simg + RT_SIMG2_T3 + (size_t)blk * 3 * 32 + l8 * 4 + pr, 32, v[0], v[1]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// forward solve of ONE 16-column tile by THREE wavefronts — the latency points (8 .. a few thousand simulations: fewer tiles than CUs,
// the shape the reference actually trains, NDE_training.jl:291).  The three flux nets are independent given the state, and so are the
// three variables' tendencies given the fluxes: wave n runs net n (4 + 2 + 2 output tiles: 132 MFMAs instead of 348 in a row) and advances
// variable n; the new stage input of each variable goes through a double-buffered LDS exchange (one barrier per stage).  Same
// arithmetic, layouts and chains as rt16_forward_kernel.  The tapes are written in tile16's formats, because at these sizes the gradient
// is taken by tile16's taped adjoint: stage inputs [tile][step][stage][column][3 Nz], hidden pre-activations [tile][step][stage][column][net][72].
// ------------------------------------------------------------------------------------------------
// RICH (small problems, where tape bytes cost nothing): instead of the hidden pre-activations in tile16's format, the forward kernel tapes what the
// net-split adjoint would otherwise recompute on its critical path, as register images (1-KB coalesced stores):
//   [tile][step][stage][ net 0..2: a1 (4 tiles) | act'(z1) (4) | a2 (2) | act'(z2) (2) ][ physics pullback coefficients dn_k, nu_k, c_k (k = 0..2) x 2 tiles ][64 lanes][4]
// — the activation derivatives with the padding slots already zeroed, and the nine per-level coefficients of rt16_physics_apply (everything in the
// Richardson-number closure that depends on the stage input alone: all the transcendental work of the pullback).
#define RT16S_RREC ((3 * 12 + 18) * 256)    // floats per rich tape record
// Behind a layer's MFMA chain of the forward kernels: the accumulators are moved to vector registers HERE, in the chain's own basic block, before the
// `if (oz)` / `if (orr)` branches that follow.  Without it the compiler sinks the v_accvgpr_read into both sides of the tape branch and gives only the
// fall-through side the wait states an MFMA result needs; a tape-less solve (colnde_forward, colnde_loss) takes the other side, five instructions
// behind the chain's last MFMA, and read accumulators short of its last products: tanh, fp32 MFMA, 7e-2 off the float64 solution and not
// repeatable from call to call (tests/test_gpu_distinct_nets.py; the taped solves behind colnde_loss_grad were right).  The fence computes nothing:
// it only fixes where the reads stand.
#define RT16S_ACC_FENCE(acc) asm volatile("" : "+v"(acc))
template <int ACT, bool RICH>
__global__ void __launch_bounds__(192)
rt16s_forward_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ x0, const float* __restrict__ bcs,
                     const float* __restrict__ save_times, int n_save, int substeps, float* __restrict__ sol,
                     float* __restrict__ t16_tape, float* __restrict__ t16_ztape, int n_col) {
    float* wl = rt_smem;
    for (int e = threadIdx.x; e < RT_IMG_FLOATS; e += 192) wl[e] = wimg[e];
    f32x4v* ex = reinterpret_cast<f32x4v*>(rt_smem + ((RT_IMG_FLOATS + 3) & ~3));          // [2 buffers][3 variables][2 tiles][64 lanes]
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                        // this wave's net = its variable
    const int j = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x;
    const int col = tile * 16 + j;
    const bool valid = col < n_col;
    const int colc = min(col, n_col - 1);
    const int i_ = lane & 15, g_i = i_ >> 2, r_i = i_ & 3;
    int a1b[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int Q = 4 * t + r_i, f = 4 * Q + g_i;
        a1b[t] = RT_W1C + (n * 50 + ((Q < 13 && f < 50) ? f : 0)) * RT_LD1 + 4 * g;       // padding rows read a valid row; never consumed
    }
    int a2b[2], a2l[2], a3b[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int Q2 = 4 * u + r_i;
        const int row2 = n * 20 + (Q2 < 5 ? 4 * Q2 + g_i : 0);
        a2b[u] = RT_W2C + row2 * RT_LD2 + g;
        a2l[u] = RT_W2C + row2 * RT_LD2 + (g < 2 ? 48 + g : 50);
        a3b[u] = RT_W3C + (n * 31 + 16 * u + i_ - 1) * RT_LD3 + g;
    }
    float bcb, bct, bc5;
    {
        const float* bp = bcs + (size_t)colc * 6;
        bcb = bp[2 * n];
        bct = bp[2 * n + 1];
        bc5 = bp[5];
    }
    V16 Xs[3], Xn, Kacc;
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int tau = 0; tau < 2; tau++) Xs[q].t[tau] = *reinterpret_cast<const f32x4v*>(x0 + (size_t)colc * 96 + q * 32 + 16 * tau + 4 * g);
    // (wave-uniform n: a select, not a dynamic register index)
#pragma unroll
    for (int tau = 0; tau < 2; tau++)
#pragma unroll
        for (int r = 0; r < 4; r++) Xn.t[tau][r] = n == 0 ? Xs[0].t[tau][r] : (n == 1 ? Xs[1].t[tau][r] : Xs[2].t[tau][r]);
    if (sol && valid)
#pragma unroll
        for (int tau = 0; tau < 2; tau++) *reinterpret_cast<f32x4v*>(sol + ((size_t)col * n_save) * 96 + n * 32 + 16 * tau + 4 * g) = Xn.t[tau];
    const int n_steps = (n_save - 1) * substeps;
    float* tp = t16_tape ? t16_tape + (size_t)tile * n_steps * 4 * 1536 + j * 96 + n * 32 + 4 * g : nullptr;
    float* tz = (t16_ztape && !RICH) ? t16_ztape + (size_t)tile * n_steps * 4 * (16 * 216) + j * 216 + n * 72 + g : nullptr;
    float* tr = (t16_ztape && RICH) ? t16_ztape + (size_t)tile * n_steps * 4 * RT16S_RREC + lane * 4 : nullptr;
    const float Nz = 32.0f;
    const float L2E = 1.4426950408889634f;
    const float cU = m.sig_u * Nz, sU = m.sig_u * m.eps, cV = m.sig_v * Nz, sV = m.sig_v * m.eps, cB = m.B * Nz, sB = m.B * m.eps;
    const float kE = 2.0f * m.inv_dRi * L2E, oE = -2.0f * m.Ric * m.inv_dRi * L2E, cE = 30.0f * L2E;
    const float nA = -0.5f * m.nu_minus, nB = m.nu0 + 0.5f * m.nu_minus;
    const float fn = n == 0 ? -m.cs[0] * Nz : (n == 1 ? -m.cs[1] * Nz : -m.cs[2] * m.inv_Pr * Nz);
    const float s0n = n == 0 ? m.s0[0] : (n == 1 ? m.s0[1] : m.s0[2]);
    const float An = n == 0 ? m.A[0] : (n == 1 ? m.A[1] : m.A[2]);
    const float rmn = n == 0 ? -m.cs[0] : (n == 1 ? -m.cs[1] : -m.cs[2] * m.inv_Pr);                 // m_n of rt16_physics_apply's coefficients
    int step = 0, buf = 0;
    RT_STAMP_DECL;
    for (int iv = 0; iv < n_save - 1; iv++) {
        const float t0 = save_times[iv];
        const float dt = (save_times[iv + 1] - t0) / (float)substeps;
        for (int s = 0; s < substeps; s++, step++) {
            const float ts = t0 + (float)s * dt;
            Kacc.t[0] = (f32x4t)(0.0f);
            Kacc.t[1] = (f32x4t)(0.0f);
#pragma nounroll
            for (int st = 0; st < 4; st++) {
                const float ca = st == 0 ? 0.0f : (st == 3 ? 1.0f : 0.5f);
                const float cb = (st == 0 || st == 3) ? 1.0f / 6.0f : 1.0f / 3.0f;
                RT_STAMP_BEGIN();
                V16 Xme;               // (element-wise selects on the wave-uniform n: a select between the aggregates becomes a scratch array)
#pragma unroll
                for (int tau = 0; tau < 2; tau++)
#pragma unroll
                    for (int r = 0; r < 4; r++) Xme.t[tau][r] = n == 0 ? Xs[0].t[tau][r] : (n == 1 ? Xs[1].t[tau][r] : Xs[2].t[tau][r]);
                if (tp) {
                    float* o = tp + ((size_t)step * 4 + st) * 1536;
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) *reinterpret_cast<f32x4v*>(o + 16 * tau) = Xme.t[tau];
                }
                float* oz = tz ? tz + ((size_t)step * 4 + st) * (16 * 216) : nullptr;
                float* orr = tr ? tr + ((size_t)step * 4 + st) * RT16S_RREC : nullptr;
                const float top_raw = n == 2 ? rt_top_flux(m, bc5, ts + ca * dt) : bct;
                RT_STAMP(0);
                // ---- net n ----------------------------------------------------------------------------------------------
                f32x4t A1[4];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    f32x4t acc;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int Q = 4 * t + r;
                        acc[r] = Q < 13 ? wl[RT_B1C + n * 50 + min(4 * Q + g, 49)] : 0.0f;
                    }
                    const int base = a1b[t];
                    acc = rt16_chain<24, 8>(wl, acc, [=](int k) { return base + (k >> 3) * 32 + ((k >> 2) & 1) * 16 + (k & 3); },
                                            [&](int k) { return Xs[k >> 3].t[(k >> 2) & 1][k & 3]; });
                    RT16S_ACC_FENCE(acc);
                    if (oz) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int Q = 4 * t + r;
                            if (Q < 13 && (Q < 12 || g < 2)) oz[4 * Q] = acc[r];             // feature 4 Q + g of layer 1
                        }
                    }
                    if (RICH && orr) {
                        f32x4t dd;
                        rt16_act_pair<ACT>(acc, A1[t], dd);
                        if (t == 3) { dd[1] = 0.0f; dd[2] = 0.0f; dd[3] = 0.0f; if (g >= 2) dd[0] = 0.0f; }   // padding: quads >= 13, features 50, 51
                        *reinterpret_cast<f32x4v*>(orr + (n * 12 + t) * 256) = A1[t];
                        *reinterpret_cast<f32x4v*>(orr + (n * 12 + 4 + t) * 256) = dd;
                    } else
                        A1[t] = rt_act4<ACT>(acc);
                }
                RT_STAMP(1);
                f32x4t A2[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    f32x4t acc;
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[r] = (4 * u + r < 5) ? wl[RT_B2C + n * 20 + 4 * (4 * u + r) + g] : 0.0f;
                    const int base = a2b[u], basel = a2l[u];
                    acc = rt16_chain<13, 13>(wl, acc, [=](int k) { return k < 12 ? base + 4 * k : basel; },
                                             [&](int k) { return A1[k >> 2][k & 3]; });
                    RT16S_ACC_FENCE(acc);
                    if (oz) {
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (4 * u + r < 5) oz[52 + 4 * (4 * u + r)] = acc[r];            // feature 4 Q2 + g of layer 2
                    }
                    if (RICH && orr) {
                        f32x4t dd;
                        rt16_act_pair<ACT>(acc, A2[u], dd);
                        if (u == 1) { dd[1] = 0.0f; dd[2] = 0.0f; dd[3] = 0.0f; }                             // padding: quads >= 5
                        *reinterpret_cast<f32x4v*>(orr + (n * 12 + 8 + u) * 256) = A2[u];
                        *reinterpret_cast<f32x4v*>(orr + (n * 12 + 10 + u) * 256) = dd;
                    } else
                        A2[u] = rt_act4<ACT>(acc);
                }
                V16 O;
#pragma unroll
                for (int v = 0; v < 2; v++) {
                    f32x4t acc;
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[r] = wl[RT_B3C + n * 32 + 16 * v + 4 * g + r];
                    const int base = a3b[v];
                    O.t[v] = rt16_chain<5, 5>(wl, acc, [=](int k) { return base + 4 * k; }, [&](int k) { return A2[k >> 2][k & 3]; });
                }
                RT_STAMP(2);
                // ---- physics: face flux and tendency of variable n (predict_flux / predict_NDE) -----------------------------
                V16 F, Pd, Pn, Pc;
                {
                    V16 Ud, Vd, Td;
                    if (m.mpp || m.ca) {
                        Ud = shift_down16(Xs[0], lane, 0.0f); Vd = shift_down16(Xs[1], lane, 0.0f); Td = shift_down16(Xs[2], lane, 0.0f);
                    }
                    if (m.mpp) {
#pragma unroll
                        for (int tau = 0; tau < 2; tau++)
#pragma unroll
                            for (int r = 0; r < 4; r += 2) {
                                const f32x2v dU = {Xs[0].t[tau][r] - Ud.t[tau][r], Xs[0].t[tau][r + 1] - Ud.t[tau][r + 1]};
                                const f32x2v dV = {Xs[1].t[tau][r] - Vd.t[tau][r], Xs[1].t[tau][r + 1] - Vd.t[tau][r + 1]};
                                const f32x2v dT = {Xs[2].t[tau][r] - Td.t[tau][r], Xs[2].t[tau][r + 1] - Td.t[tau][r + 1]};
                                const f32x2v a1 = dU * cU + sU, a2 = dV * cV + sV;
                                const f32x2v s2 = a2 * a2 + a1 * a1;
                                f32x2v rS;
                                rS.x = __builtin_amdgcn_rcpf(s2.x);
                                rS.y = __builtin_amdgcn_rcpf(s2.y);
                                const f32x2v arg = ((dT * cB + sB) * rS) * kE + oE;
                                f32x2v e;
                                e.x = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(arg.x, -cE, cE));
                                e.y = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(arg.y, -cE, cE));
                                const f32x2v e1 = e + 1.0f;
                                f32x2v rc;
                                rc.x = __builtin_amdgcn_rcpf(e1.x);
                                rc.y = __builtin_amdgcn_rcpf(e1.y);
                                const f32x2v th = rc * -2.0f + 1.0f;
                                const f32x2v nu = th * nA + nB;
                                const f32x2v dn = n == 0 ? dU : (n == 1 ? dV : dT);
                                const f32x2v on = {O.t[tau][r], O.t[tau][r + 1]};
                                const f32x2v f = (nu * dn) * fn + on;
                                F.t[tau][r] = f.x; F.t[tau][r + 1] = f.y;
                                if (RICH && orr) {
                                    // this wave's three of the nine pullback coefficients (rt16_physics_apply): dn_n, nu_n, c_n
                                    const f32x2v wf = (1.0f - th * th) * rS;                 // (1 - tanh²) / S2
                                    const f32x2v wR = wf * ((dT * cB + sB) * rS);            // ... times Ri
                                    const f32x2v cn = n == 0 ? wR * (a1 * (-2.0f * m.sig_u)) : (n == 1 ? wR * (a2 * (-2.0f * m.sig_v)) : wf * m.B);
                                    const f32x2v pd = dn * (rmn * (Nz * m.c_rib)), pn = nu * rmn;
                                    Pd.t[tau][r] = pd.x; Pd.t[tau][r + 1] = pd.y;
                                    Pn.t[tau][r] = pn.x; Pn.t[tau][r + 1] = pn.y;
                                    Pc.t[tau][r] = cn.x; Pc.t[tau][r + 1] = cn.y;
                                }
                            }
                        if (g == 0) F.t[0][0] = m.zero_w ? bcb - s0n : bcb;                 // face 0: the bottom boundary
                        if (RICH && g == 0) { Pn.t[0][0] = 0.0f; Pc.t[0][0] = 0.0f; }       // ... carries no diffusive flux
                    } else {
#pragma unroll
                        for (int tau = 0; tau < 2; tau++)
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                const bool in = !(tau == 0 && r == 0 && g == 0);
                                float f = in ? O.t[tau][r] : (m.zero_w ? 0.0f : bcb);
                                if (RICH) { Pd.t[tau][r] = 0.0f; Pn.t[tau][r] = 0.0f; Pc.t[tau][r] = 0.0f; }
                                if (m.ca && in && n == 2) {
                                    const float gT = (Xs[2].t[tau][r] - Td.t[tau][r]) * Nz;
                                    f -= m.cs[2] * m.kappa * fminf(0.0f, gT);
                                    if (RICH && gT < 0.0f) Pn.t[tau][r] = -m.cs[2] * m.kappa;
                                }
                                F.t[tau][r] = f;
                            }
                    }
                }
                if (RICH && orr && (m.mpp || m.ca)) {
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) {
                        *reinterpret_cast<f32x4v*>(orr + (36 + (0 * 3 + n) * 2 + tau) * 256) = Pd.t[tau];
                        *reinterpret_cast<f32x4v*>(orr + (36 + (1 * 3 + n) * 2 + tau) * 256) = Pn.t[tau];
                        *reinterpret_cast<f32x4v*>(orr + (36 + (2 * 3 + n) * 2 + tau) * 256) = Pc.t[tau];
                    }
                }
                {
                    const float top = m.zero_w ? top_raw - s0n : top_raw;
                    const V16 Fu = shift_up16(F, lane, top);
#pragma unroll
                    for (int tau = 0; tau < 2; tau++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            float v = -An * (Fu.t[tau][r] - F.t[tau][r]);
                            if (n == 0) v += m.cor_u * (m.sig_v * Xs[1].t[tau][r] + m.mu_v);
                            if (n == 1) v -= m.cor_v * (m.sig_u * Xs[0].t[tau][r] + m.mu_u);
                            F.t[tau][r] = v;                                                // F now holds the tendency of variable n
                        }
                }
                RT_STAMP(3);
                // ---- RK4 bookkeeping for variable n; the next stage input (or, after stage 3, the new state) is exchanged -------------
                V16 Xnext;
#pragma unroll
                for (int tau = 0; tau < 2; tau++) {
                    Kacc.t[tau] += cb * F.t[tau];
                    if (st < 3) {
                        const float can = st == 2 ? 1.0f : 0.5f;
                        Xnext.t[tau] = Xn.t[tau] + (can * dt) * F.t[tau];
                    } else {
                        Xn.t[tau] += dt * Kacc.t[tau];
                        Xnext.t[tau] = Xn.t[tau];
                    }
                }
                f32x4v* eb = ex + buf * 384;
#pragma unroll
                for (int tau = 0; tau < 2; tau++) eb[(n * 2 + tau) * 64 + lane] = Xnext.t[tau];
                // (a bare barrier behind the LDS writes: __syncthreads() would also drain vmcnt, i.e. wait for this stage's tape stores)
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
                for (int q = 0; q < 3; q++)
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) Xs[q].t[tau] = eb[(q * 2 + tau) * 64 + lane];
                buf ^= 1;
                RT_STAMP(4);
            }
            if (s == substeps - 1 && sol && valid) {
#pragma unroll
                for (int tau = 0; tau < 2; tau++)
                    *reinterpret_cast<f32x4v*>(sol + ((size_t)col * n_save + iv + 1) * 96 + n * 32 + 16 * tau + 4 * g) = Xn.t[tau];
            }
        }
    }
#ifdef COLNDE_STAMPS_FWD
    RT_STAMP_FLUSH();
#endif
}

// The Pacanowski-Philander constants of the kernels that read them per model (ensembles: RtEns::phys)
__device__ __forceinline__ RtPhys rt_phys_of(const DevModel& m) {
    RtPhys p;
    p.nu0 = m.nu0; p.nu_minus = m.nu_minus; p.Ric = m.Ric; p.inv_dRi = m.inv_dRi; p.inv_Pr = m.inv_Pr; p.c_rib = m.c_rib; p.pad0 = 0.0f; p.pad1 = 0.0f;
    return p;
}

// The same solve with a FOURTH wavefront (the workgroup's idle SIMD) as helper: it evaluates the Richardson-number closure of all three variables
// once per stage — the diffusive face fluxes go to LDS, the rich tape's nine pullback coefficients to HBM — while the three net waves run their
// chains; a second bare barrier per stage (B) hands the fluxes over.  Every wave executes exactly the barriers (B) and (A) in every stage.
// SPLIT (COLNDE_MATRIX_BF16X3_EXACT; RK4 and, since round 4, RKC2): layers 1 and 2 on v_mfma_f32_16x16x32_bf16 from exact three-way operand splits (rt16_forward_kernel<ACT, true>;
// image RT_SIMG2_*: rt_pack_split_ns_kernel); layer 3 and the biases stay on the tail of the fp32 image
// SCHED (colnde_set_schedule; RK4): save interval iv takes sched[iv] steps instead of `substeps` — one scalar load per save interval, the same trip
// counts in all four waves — and the tapes are indexed by the running step counter, total_steps = sum of sched in n_steps' place.  The body is one
// text, rt16sh_forward_body.inc, compiled twice (RT16SH_SCHED = 0 | 1: a preprocessor switch, so that rt16sh_forward_kernel stays the machine code it
// was — as an inlined function template with a SCHED parameter the same text came out as different code in every instantiation).
template <int ACT, bool RICH, bool RKC = false, bool SPLIT = false>
__global__ void __launch_bounds__(256)
rt16sh_forward_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ x0, const float* __restrict__ bcs,
                     const float* __restrict__ save_times, int n_save, int substeps, float* __restrict__ sol,
                     float* __restrict__ t16_tape, float* __restrict__ t16_ztape, int n_col, RtEns ens) {
#define RT16SH_SCHED 0
#include "rt16sh_forward_body.inc"
#undef RT16SH_SCHED
}
// ... under a step schedule (RK4): sched[n_save - 1] steps per save interval, total_steps their sum
template <int ACT, bool RICH, bool SPLIT>
__global__ void __launch_bounds__(256)
rt16sh_forward_sched_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ x0, const float* __restrict__ bcs,
                            const float* __restrict__ save_times, int n_save, float* __restrict__ sol,
                            float* __restrict__ t16_tape, float* __restrict__ t16_ztape, int n_col, RtEns ens,
                            const int* __restrict__ sched, int total_steps) {
    constexpr bool RKC = false;
    int substeps;                                          // the steps of the save interval in hand
#define RT16SH_SCHED 1
#include "rt16sh_forward_body.inc"
#undef RT16SH_SCHED
}

// ------------------------------------------------------------------------------------------------
// discrete adjoint of ONE 16-column tile by THREE wavefronts (the companion of rt16s_forward_kernel at the latency points).
//
// Wave n back-propagates flux net n: from the taped hidden pre-activations (no forward recomputation) through the three transposed
// chains W3^T, W2^T, W1^T (114 dependent 16x16x4 MFMAs instead of 342 in a row).  The physics pullback couples the three variables
// through the Richardson number and is cheap beside the chains, so every wave evaluates it in full — the three copies of λ, x̄ and
// the stage cotangent are bit-identical by construction (same operations, same order).  What a wave alone knows is its net's part of
// the state cotangent, W1_n^T δz1_n (96 rows): the three parts go through a double-buffered LDS exchange (one barrier per stage) and
// are summed in net order by everybody.
//
// The weight gradients are not accumulated here: the kernel writes tile16's delta-tape records
//   [tile][step][stage][column][ x (96) | a of net 0..2 (104 each: a1 at 0, a2 at 52) | δz of net 0..2 (104 each: δz1 at 0, δz2 at 52, δz3 at 72) ]
// and tile16's split-K dW GEMM contracts them (dw_gemm_lds_kernel) — no transposition, no accumulator registers, no flush code here.
// Bias gradients (column sums of the deltas) and the loss sums go to the tile's slab row, as in tile16's taped adjoint.
// ------------------------------------------------------------------------------------------------
#define RT16S_REC (16 * 720)       // floats per delta-tape record: 16 columns x (96 + 2 x 3 x 104)
#define RT16S_ZREC (16 * 216)      // floats per pre-activation tape record: 16 columns x 3 nets x 72
#define RT16S_STG (16 * 180)       // floats of one wave's record staging area in LDS

// NC independent chains of N k-steps advanced together, k-major, their A operands fetched as one group — early enough, by the caller, that the
// LDS latency is covered by other work.  (The grouping is for the operand fetch: a dependent fp32 MFMA chain issues at the full rate anyway,
// tools/probe/mfma_rate.hip.)
template <int NC, int N, class AF>
__device__ __forceinline__ void rt16_fetch_ops(const float* wl, float (&a)[NC][N], AF aidx) {
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int k = 0; k < N; k++) a[c][k] = wl[aidx(c, k)];
}
template <int NC, int N, class BF>
__device__ __forceinline__ void rt16_run_ops(const float (&a)[NC][N], f32x4t (&acc)[NC], BF bval) {
#pragma unroll
    for (int k = 0; k < N; k++)
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = mfma16t(a[c][k], bval(k), acc[c]);
}

__device__ __forceinline__ void rt16_physics_vjp(const DevModel& m, const RtPhys& ph, const V16 (&X)[3], V16 (&kd)[3], int lane, V16 (&xb)[3]) {
    const float Nz = 32.0f;
    const int g = lane >> 4;
#pragma unroll
    for (int tau = 0; tau < 2; tau++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            xb[0].t[tau][r] = -m.cor_v * m.sig_u * kd[1].t[tau][r];
            xb[1].t[tau][r] = m.cor_u * m.sig_v * kd[0].t[tau][r];
            xb[2].t[tau][r] = 0.0f;
        }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const V16 dn = shift_down16(kd[k], lane, 0.0f);
#pragma unroll
        for (int tau = 0; tau < 2; tau++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                kd[k].t[tau][r] = (tau == 0 && r == 0 && g == 0) ? 0.0f : m.A[k] * (kd[k].t[tau][r] - dn.t[tau][r]);
    }
    if (!m.mpp && !m.ca) return;
    V16 gb[3];
    if (m.mpp) {
        const V16 Ud = shift_down16(X[0], lane, 0.0f), Vd = shift_down16(X[1], lane, 0.0f), Td = shift_down16(X[2], lane, 0.0f);
        // the arithmetic of rt_physics_vjp, uniform factors folded
        const float cU = m.sig_u * Nz, sU = m.sig_u * m.eps, cV = m.sig_v * Nz, sV = m.sig_v * m.eps, cB = m.B * Nz, sB = m.B * m.eps;
        const float L2E = 1.4426950408889634f;
        const float kE = 2.0f * ph.inv_dRi * L2E, oE = -2.0f * ph.Ric * ph.inv_dRi * L2E, cE = 30.0f * L2E;
        const float nA = -0.5f * ph.nu_minus, nB = ph.nu0 + 0.5f * ph.nu_minus;
        const float m0 = -m.cs[0], m1 = -m.cs[1], m2 = -m.cs[2] * ph.inv_Pr;
        const float n0 = m0 * Nz * ph.c_rib, n1 = m1 * Nz * ph.c_rib, n2 = m2 * Nz * ph.c_rib;
        const float q0 = -2.0f * m.sig_u, q1 = -2.0f * m.sig_v;
#pragma unroll
        for (int tau = 0; tau < 2; tau++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool in = !(tau == 0 && r == 0 && g == 0);
                const float dU = X[0].t[tau][r] - Ud.t[tau][r], dV = X[1].t[tau][r] - Vd.t[tau][r], dT = X[2].t[tau][r] - Td.t[tau][r];
                const float a1 = fmaf(dU, cU, sU), a2 = fmaf(dV, cV, sV);
                const float rS = __builtin_amdgcn_rcpf(fmaf(a2, a2, a1 * a1));
                const float Ri = fmaf(dT, cB, sB) * rS;
                const float e = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(fmaf(Ri, kE, oE), -cE, cE));
                const float th = fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);
                const float nu = fmaf(th, nA, nB);
                const float k0 = kd[0].t[tau][r], k1 = kd[1].t[tau][r], k2 = kd[2].t[tau][r];
                const float t0 = k0 * nu, t1 = k1 * nu, t2 = k2 * nu;
                float nub = (k0 * dU) * n0;
                nub = fmaf(k1 * dV, n1, nub);
                nub = fmaf(k2 * dT, n2, nub);
                const float w = nub * (fmaf(-th, th, 1.0f) * rS);
                const float qq = w * Ri;
                const float g2 = fmaf(w, m.B, t2 * m2);
                const float g0 = fmaf(qq, a1 * q0, t0 * m0);
                const float g1 = fmaf(qq, a2 * q1, t1 * m1);
                gb[0].t[tau][r] = in ? g0 : 0.0f;
                gb[1].t[tau][r] = in ? g1 : 0.0f;
                gb[2].t[tau][r] = in ? g2 : 0.0f;
            }
    } else {
        const V16 Td = shift_down16(X[2], lane, 0.0f);
#pragma unroll
        for (int tau = 0; tau < 2; tau++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool in = !(tau == 0 && r == 0 && g == 0);
                const float gT = (X[2].t[tau][r] - Td.t[tau][r]) * Nz;
                gb[0].t[tau][r] = 0.0f;
                gb[1].t[tau][r] = 0.0f;
                gb[2].t[tau][r] = (in && gT < 0.0f) ? -kd[2].t[tau][r] * m.cs[2] * m.kappa : 0.0f;
            }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const V16 gu_ = shift_up16(gb[k], lane, 0.0f);
#pragma unroll
        for (int tau = 0; tau < 2; tau++)
#pragma unroll
            for (int r = 0; r < 4; r++) xb[k].t[tau][r] += (gb[k].t[tau][r] - gu_.t[tau][r]) * Nz;
    }
}

// The coupled (transcendental) half of the pullback read from the RICH tape instead of recomputed: nine coefficients per level,
//   face cotangent D_k = A_k (k̄_k[i] - k̄_k[i-1]);  g_k = nub c_k + D_k nu_k with nub = Σ_k D_k dn_k;  x̄_k += Nz (g_k[i] - g_k[i+1])
// (rt16_physics_vjp's arithmetic with the uniform factors and the level mask folded into the coefficients by the forward kernel).
// On entry kd holds k̄; on exit dO, and xb the physics part of the state cotangent.
struct PhysC { V16 dn0, dn1, dn2, nu0, nu1, nu2, c0, c1, c2; };

__device__ __forceinline__ void rt16_physics_apply(const DevModel& m, const PhysC& P, V16 (&kd)[3], int lane, V16 (&xb)[3]) {
    const float Nz = 32.0f;
    const int g = lane >> 4;
#pragma unroll
    for (int tau = 0; tau < 2; tau++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            xb[0].t[tau][r] = -m.cor_v * m.sig_u * kd[1].t[tau][r];
            xb[1].t[tau][r] = m.cor_u * m.sig_v * kd[0].t[tau][r];
            xb[2].t[tau][r] = 0.0f;
        }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const V16 dn = shift_down16(kd[k], lane, 0.0f);
#pragma unroll
        for (int tau = 0; tau < 2; tau++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                kd[k].t[tau][r] = (tau == 0 && r == 0 && g == 0) ? 0.0f : m.A[k] * (kd[k].t[tau][r] - dn.t[tau][r]);
    }
    if (!m.mpp && !m.ca) return;
    V16 gb[3];
#pragma unroll
    for (int tau = 0; tau < 2; tau++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float k0 = kd[0].t[tau][r], k1 = kd[1].t[tau][r], k2 = kd[2].t[tau][r];
            const float nub = fmaf(k2, P.dn2.t[tau][r], fmaf(k1, P.dn1.t[tau][r], k0 * P.dn0.t[tau][r]));
            gb[0].t[tau][r] = fmaf(nub, P.c0.t[tau][r], k0 * P.nu0.t[tau][r]);
            gb[1].t[tau][r] = fmaf(nub, P.c1.t[tau][r], k1 * P.nu1.t[tau][r]);
            gb[2].t[tau][r] = fmaf(nub, P.c2.t[tau][r], k2 * P.nu2.t[tau][r]);
        }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const V16 gu_ = shift_up16(gb[k], lane, 0.0f);
#pragma unroll
        for (int tau = 0; tau < 2; tau++)
#pragma unroll
            for (int r = 0; r < 4; r++) xb[k].t[tau][r] += (gb[k].t[tau][r] - gu_.t[tau][r]) * Nz;
    }
}

template <int ACT, bool RICH>
__global__ void __launch_bounds__(192)
rt16s_adjoint_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ save_times, int n_save, int substeps,
                     const float* __restrict__ sol, const float* __restrict__ truth, const float* __restrict__ t16_tape,
                     const float* __restrict__ t16_ztape, LossWeights lw, float* __restrict__ slab, int n_col,
                     float* __restrict__ dwtape) {
    float* wl = rt_smem;
    for (int e = threadIdx.x; e < RT_IMG_FLOATS; e += 192) wl[e] = wimg[e];
    f32x4v* ex = reinterpret_cast<f32x4v*>(rt_smem + ((RT_IMG_FLOATS + 3) & ~3));          // [2 buffers][3 nets][6 tiles][64 lanes]
    // staging of each wave's part of the delta-tape record: [16 columns][a1 52 | a2 20 | δz1 52 | δz2 20 | δz3 32] with row stride 180
    // (conflict-free for the element-wise writes, 16-byte aligned for the float4 read-back); the pad slots stay zero
    float* stg_all = rt_smem + ((RT_IMG_FLOATS + 3) & ~3) + 2 * (3 * 6 * 64) * 4;
    for (int e = threadIdx.x; e < 3 * RT16S_STG; e += 192) stg_all[e] = 0.0f;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                        // this wave's net
    float* stg = stg_all + n * RT16S_STG;
    const int j = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x;
    const int col = tile * 16 + j;
    const bool valid = col < n_col;
    const int colc = min(col, n_col - 1);
    const int i_ = lane & 15, g_i = i_ >> 2, r_i = i_ & 3;
    // A-operand bases of the transposed products (output row i_ of a tile, k-lane g): W3^T (rows = a2 features), W2^T (rows = a1 features),
    // W1^T (rows = state features); rows that are padding read the image's zero column
    int b3T[2], b2T[4];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int Q2 = 4 * u + r_i;
        b3T[u] = RT_W3C + (n * 31 + 4 * g - 1) * RT_LD3 + (Q2 < 5 ? 4 * Q2 + g_i : 20);
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int Q = 4 * t + r_i, f = 4 * Q + g_i;
        b2T[t] = RT_W2C + (n * 20 + g) * RT_LD2 + ((Q < 13 && f < 50) ? f : 50);
    }
    const int b1T = RT_W1C + (n * 50 + g) * RT_LD1 + i_;

    V16 lam[3], xb[3], xbs[3];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int tau = 0; tau < 2; tau++) { lam[q].t[tau] = (f32x4t)(0.0f); xb[q].t[tau] = (f32x4t)(0.0f); xbs[q].t[tau] = (f32x4t)(0.0f); }
    f32x4t gb1[4], gb2[2], gb3[2];                         // bias gradients: this lane's column of every delta, summed over the stages
#pragma unroll
    for (int t = 0; t < 4; t++) gb1[t] = (f32x4t)(0.0f);
#pragma unroll
    for (int u = 0; u < 2; u++) { gb2[u] = (f32x4t)(0.0f); gb3[u] = (f32x4t)(0.0f); }
    float sum_d = 0.0f, sum_g = 0.0f;                      // loss sums of variable n (profile and gradient terms)
    RT_STAMP_DECL;

    const int n_steps = (n_save - 1) * substeps;
    const float* tp = t16_tape + (size_t)tile * n_steps * 4 * 1536 + j * 96 + 4 * g;
    const float* tz = RICH ? t16_ztape + (size_t)tile * n_steps * 4 * RT16S_RREC + lane * 4      // the rich tape (see rt16s_forward_kernel)
                           : t16_ztape + (size_t)tile * n_steps * 4 * RT16S_ZREC + j * 216 + n * 72 + g;
    const bool phys = m.mpp || m.ca;
    float* rec0 = dwtape + (size_t)tile * n_steps * 4 * RT16S_REC;
    // the record's 11 float4 pieces this lane copies from the staging area each stage: piece e = 64 i + lane = column e / 44, float4 e % 44
    // of that column's 72 a-floats and 104 δ-floats
    int stg_rd[11], rec_wr[11];
#pragma unroll
    for (int i = 0; i < 11; i++) {
        const int e = 64 * i + lane, c = e / 44, f4 = e - 44 * c;
        stg_rd[i] = c * 180 + 4 * f4;
        rec_wr[i] = c * 720 + 96 + (f4 < 18 ? n * 104 + 4 * f4 : (3 + n) * 104 + 4 * (f4 - 18));
    }
    float* sw = stg + j * 180 + g;                          // element-wise staging writes of this lane: feature 4 Q + g of column j

    // loss injection at save point sv: λ += ∂loss/∂sol[:, sv] (all three variables, every wave); the sums of squares of variable n only
    auto inject = [&](int sv, bool add) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            V16 d;
#pragma unroll
            for (int tau = 0; tau < 2; tau++) {
                const size_t o = ((size_t)colc * n_save + sv) * 96 + q * 32 + 16 * tau + 4 * g;
                const f32x4v a = *reinterpret_cast<const f32x4v*>(sol + o);
                const f32x4v b = *reinterpret_cast<const f32x4v*>(truth + o);
#pragma unroll
                for (int e = 0; e < 4; e++) d.t[tau][e] = valid ? a[e] - b[e] : 0.0f;
            }
            const V16 dd = shift_down16(d, lane, 0.0f);
            V16 gg;
            float sd = 0.0f, sg = 0.0f;
#pragma unroll
            for (int tau = 0; tau < 2; tau++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    gg.t[tau][r] = (tau == 0 && r == 0 && g == 0) ? 0.0f : (d.t[tau][r] - dd.t[tau][r]) * 32.0f;
                    sd += d.t[tau][r] * d.t[tau][r];
                    sg += gg.t[tau][r] * gg.t[tau][r];
                }
            if (q == n) { sum_d += sd; sum_g += sg; }
            if (add) {
                const V16 gu_ = shift_up16(gg, lane, 0.0f);
#pragma unroll
                for (int tau = 0; tau < 2; tau++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        lam[q].t[tau][r] += 2.0f * lw.w[q] * d.t[tau][r] + 2.0f * lw.w[3 + q] * 32.0f * (gg.t[tau][r] - gu_.t[tau][r]);
            }
        }
    };
    inject(0, false);

    // stage inputs and hidden pre-activations (RICH: variable n of the stage input, this net's activations and derivatives, the nine
    // physics coefficients), fetched one stage ahead of their use
    V16 Xp[3];
    float z1p[13], z2p[5];
    f32x4t adp[12];
    PhysC Pp;
    auto prefetch = [&](int qs) __attribute__((always_inline)) {
        const float* sx = tp + (size_t)qs * 1536;
        if (RICH) {
#pragma unroll
            for (int tau = 0; tau < 2; tau++) Xp[0].t[tau] = *reinterpret_cast<const f32x4v*>(sx + n * 32 + 16 * tau);
            const float* sr = tz + (size_t)qs * RT16S_RREC;
#pragma unroll
            for (int e = 0; e < 12; e++) adp[e] = *reinterpret_cast<const f32x4v*>(sr + (n * 12 + e) * 256);
            if (phys) {
#pragma unroll
                for (int tau = 0; tau < 2; tau++) {
                    Pp.dn0.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 0 + tau) * 256);
                    Pp.dn1.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 2 + tau) * 256);
                    Pp.dn2.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 4 + tau) * 256);
                    Pp.nu0.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 6 + tau) * 256);
                    Pp.nu1.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 8 + tau) * 256);
                    Pp.nu2.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 10 + tau) * 256);
                    Pp.c0.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 12 + tau) * 256);
                    Pp.c1.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 14 + tau) * 256);
                    Pp.c2.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 16 + tau) * 256);
                }
            }
            return;
        }
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int tau = 0; tau < 2; tau++) Xp[q].t[tau] = *reinterpret_cast<const f32x4v*>(sx + q * 32 + 16 * tau);
        const float* sz = tz + (size_t)qs * RT16S_ZREC;
#pragma unroll
        for (int Q = 0; Q < 13; Q++) z1p[Q] = (Q < 12 || g < 2) ? sz[4 * Q] : 0.0f;
#pragma unroll
        for (int Q2 = 0; Q2 < 5; Q2++) z2p[Q2] = sz[52 + 4 * Q2];
    };
    prefetch(n_steps * 4 - 1);
    int buf = 0;

    for (int iv = n_save - 2; iv >= 0; iv--) {
        const float dt = (save_times[iv + 1] - save_times[iv]) / (float)substeps;
        inject(iv + 1, true);
        for (int s = substeps - 1; s >= 0; s--) {
            const int step = iv * substeps + s;
#pragma nounroll
            for (int st = 3; st >= 0; st--) {
                const float cwl = (st == 0 || st == 3) ? dt / 6.0f : dt / 3.0f;
                const float cwx = st == 3 ? 0.0f : (st == 2 ? dt : 0.5f * dt);
                const int qs = step * 4 + st;
                RT_STAMP_BEGIN();
                V16 X[3];
                f32x4t Z1[4], Z2[2];
                f32x4t A1[4], D1[4], A2[2], D2[2];
                V16 kb[3], xbp[3];
                // (1) stage cotangent k̄ = cwl λ + cwx x̄ (x̄: the state cotangent of the stage handled before), then the physics pullback
#pragma unroll
                for (int q = 0; q < 3; q++)
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) kb[q].t[tau] = cwl * lam[q].t[tau] + cwx * xb[q].t[tau];
                if (RICH) {
                    X[0] = Xp[0];                                                        // variable n only
#pragma unroll
                    for (int t = 0; t < 4; t++) { A1[t] = adp[t]; D1[t] = adp[4 + t]; }
#pragma unroll
                    for (int u = 0; u < 2; u++) { A2[u] = adp[8 + u]; D2[u] = adp[10 + u]; }
                    rt16_physics_apply(m, Pp, kb, lane, xbp);                            // kb now holds dO
                    if (qs > 0) prefetch(qs - 1);
                } else {
#pragma unroll
                    for (int q = 0; q < 3; q++) X[q] = Xp[q];
#pragma unroll
                    for (int t = 0; t < 4; t++)
#pragma unroll
                        for (int r = 0; r < 4; r++) Z1[t][r] = (4 * t + r < 13) ? z1p[(4 * t + r) < 13 ? 4 * t + r : 0] : 0.0f;
#pragma unroll
                    for (int u = 0; u < 2; u++)
#pragma unroll
                        for (int r = 0; r < 4; r++) Z2[u][r] = (4 * u + r < 5) ? z2p[(4 * u + r) < 5 ? 4 * u + r : 0] : 0.0f;
                    if (qs > 0) prefetch(qs - 1);
                    rt16_physics_vjp(m, rt_phys_of(m), X, kb, lane, xbp);                // kb now holds dO
                }
                RT_STAMP(0);
                V16 dO;                 // (element-wise selects on the wave-uniform n: a select between the aggregates becomes a scratch array)
#pragma unroll
                for (int tau = 0; tau < 2; tau++)
#pragma unroll
                    for (int r = 0; r < 4; r++) dO.t[tau][r] = n == 0 ? kb[0].t[tau][r] : (n == 1 ? kb[1].t[tau][r] : kb[2].t[tau][r]);
                // operands of the W3^T and W2^T products (fetched here: the activations below cover their LDS latency)
                float a3[2][8], a2[4][5];
                rt16_fetch_ops<2, 8>(wl, a3, [&](int u, int k) { return b3T[u] + (16 * (k >> 2) + (k & 3)) * RT_LD3; });
                rt16_fetch_ops<4, 5>(wl, a2, [&](int t, int k) { return b2T[t] + 4 * k * RT_LD2; });
                RT_SCHED_HARD();
                // (2) activations and their derivatives from the taped pre-activations (RICH: taped as such)
                if (!RICH) {
#pragma unroll
                    for (int t = 0; t < 4; t++) rt16_act_pair<ACT>(Z1[t], A1[t], D1[t]);
#pragma unroll
                    for (int u = 0; u < 2; u++) rt16_act_pair<ACT>(Z2[u], A2[u], D2[u]);
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if (r > 0) { D1[3][r] = 0.0f; D2[1][r] = 0.0f; }             // padding quads: Q >= 13, Q2 >= 5
                    }
                    if (g >= 2) D1[3][0] = 0.0f;                                         // features 50, 51 of quad 12
                }
                float* rec = rec0 + (size_t)qs * RT16S_REC;
                {
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) {
                        f32x4v xv;
#pragma unroll
                        for (int r = 0; r < 4; r++) xv[r] = (RICH || n == 0) ? X[0].t[tau][r] : (n == 1 ? X[1].t[tau][r] : X[2].t[tau][r]);
                        *reinterpret_cast<f32x4v*>(rec + j * 720 + n * 32 + 16 * tau + 4 * g) = xv;
                    }
#pragma unroll
                    for (int Q = 0; Q < 13; Q++)
                        if (Q < 12 || g < 2) sw[4 * Q] = A1[Q >> 2][Q & 3];
#pragma unroll
                    for (int Q2 = 0; Q2 < 5; Q2++) sw[52 + 4 * Q2] = A2[Q2 >> 2][Q2 & 3];
                }
                RT_STAMP(1);
                // (3) δz2 = (W3^T dO) ∘ act'(z2): 8 k-steps = the faces (v, r), lane g holding face 16 v + 4 g + r
                f32x4t dZ2[2] = {(f32x4t)(0.0f), (f32x4t)(0.0f)};
                rt16_run_ops<2, 8>(a3, dZ2, [&](int k) { return dO.t[k >> 2][k & 3]; });
#pragma unroll
                for (int u = 0; u < 2; u++) dZ2[u] *= D2[u];
                // operands of the first two W1^T tiles, in flight under the W2^T products
                float a1[2][2][13];
                rt16_fetch_ops<2, 13>(wl, a1[0], [&](int c, int k) { return b1T + 16 * c + 4 * k * RT_LD1; });
                RT_SCHED_HARD();
                // (4) δz1 = (W2^T δz2) ∘ act'(z1): 5 k-steps = the quads of a2
                f32x4t dZ1[4] = {(f32x4t)(0.0f), (f32x4t)(0.0f), (f32x4t)(0.0f), (f32x4t)(0.0f)};
                rt16_run_ops<4, 5>(a2, dZ1, [&](int k) { return dZ2[k >> 2][k & 3]; });
#pragma unroll
                for (int t = 0; t < 4; t++) dZ1[t] *= D1[t];
                RT_STAMP(2);
                {
#pragma unroll
                    for (int Q = 0; Q < 13; Q++)
                        if (Q < 12 || g < 2) sw[72 + 4 * Q] = dZ1[Q >> 2][Q & 3];
#pragma unroll
                    for (int Q2 = 0; Q2 < 5; Q2++) sw[124 + 4 * Q2] = dZ2[Q2 >> 2][Q2 & 3];
                    float* s3 = stg + j * 180 + 144 + 4 * g - 1;                         // output o = face - 1
#pragma unroll
                    for (int v = 0; v < 2; v++)
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (!(v == 0 && r == 0 && g == 0)) s3[16 * v + r] = dO.t[v][r];
                    // the wave's 16 x 176 floats leave as 11 float4 stores per lane (the element-wise form costs 52 scattered dword stores)
#pragma unroll
                    for (int i = 0; i < 11; i++) *reinterpret_cast<f32x4v*>(rec + rec_wr[i]) = *reinterpret_cast<const f32x4v*>(stg + stg_rd[i]);
                }
#pragma unroll
                for (int t = 0; t < 4; t++) gb1[t] += dZ1[t];
#pragma unroll
                for (int u = 0; u < 2; u++) { gb2[u] += dZ2[u]; gb3[u] += dO.t[u]; }
                RT_STAMP(3);
                // (5) this net's part of the state cotangent, W1_n^T δz1 (6 tiles x 13 k-steps), exchanged and summed in net order
                f32x4v* eb = ex + buf * (3 * 6 * 64);
#pragma unroll
                for (int q = 0; q < 3; q++) {                                            // variable q: its two 16-level tiles together
                    if (q < 2) rt16_fetch_ops<2, 13>(wl, a1[(q + 1) & 1], [&](int c, int k) { return b1T + 32 * (q + 1) + 16 * c + 4 * k * RT_LD1; });
                    RT_SCHED_HARD();
                    f32x4t c2[2] = {(f32x4t)(0.0f), (f32x4t)(0.0f)};
                    rt16_run_ops<2, 13>(a1[q & 1], c2, [&](int k) { return dZ1[k >> 2][k & 3]; });
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) eb[(n * 6 + q * 2 + tau) * 64 + lane] = c2[tau];
                    RT_SCHED_HARD();
                }
                RT_STAMP(4);
                // (a bare barrier behind the LDS writes: __syncthreads() would also drain vmcnt — this stage's tape stores and the next
                //  stage's prefetch)
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
                for (int q = 0; q < 3; q++)
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) {
                        const f32x4v c0 = eb[(0 * 6 + q * 2 + tau) * 64 + lane], c1 = eb[(1 * 6 + q * 2 + tau) * 64 + lane],
                                     c2 = eb[(2 * 6 + q * 2 + tau) * 64 + lane];
                        xb[q].t[tau] = xbp[q].t[tau] + ((c0 + c1) + c2);
                        xbs[q].t[tau] += xb[q].t[tau];
                    }
                buf ^= 1;
                RT_STAMP(5);
            }
            // λ_n = λ_{n+1} + x̄_1 + x̄_2 + x̄_3 + x̄_4
#pragma unroll
            for (int q = 0; q < 3; q++)
#pragma unroll
                for (int tau = 0; tau < 2; tau++) { lam[q].t[tau] += xbs[q].t[tau]; xbs[q].t[tau] = (f32x4t)(0.0f); }
        }
    }

#ifndef COLNDE_STAMPS_FWD
    RT_STAMP_FLUSH();
#endif
    // ---- the tile's slab row: bias gradients of net n (sums over the 16 columns = the lanes of a g-group) and the loss sums ----
    float* out = slab + (size_t)tile * (m.n_params + 8);
    auto colsum = [&](float v) {
        v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
        return v;
    };
#pragma unroll
    for (int Q = 0; Q < 13; Q++) {
        const float v = colsum(gb1[Q >> 2][Q & 3]);
        if (j == 0 && (Q < 12 || g < 2)) out[n * m.net_size + m.b_off[0] + 4 * Q + g] = v;
    }
#pragma unroll
    for (int Q2 = 0; Q2 < 5; Q2++) {
        const float v = colsum(gb2[Q2 >> 2][Q2 & 3]);
        if (j == 0) out[n * m.net_size + m.b_off[1] + 4 * Q2 + g] = v;
    }
#pragma unroll
    for (int v_ = 0; v_ < 2; v_++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float v = colsum(gb3[v_][r]);
            const int face = 16 * v_ + 4 * g + r;
            if (j == 0 && face >= 1) out[n * m.net_size + m.b_off[2] + face - 1] = v;
        }
    float sd = sum_d, sg = sum_g;
    for (int off = 32; off > 0; off >>= 1) { sd += __shfl_down(sd, off); sg += __shfl_down(sg, off); }
    if (lane == 0) {
        out[m.n_params + n] = sd;
        out[m.n_params + 3 + n] = sg;
        if (n == 0) { out[m.n_params + 6] = 0.0f; out[m.n_params + 7] = 0.0f; }
    }
}

// ------------------------------------------------------------------------------------------------
// The net-split adjoint with a FOURTH wavefront.  In rt16s_adjoint_kernel every net wave carries the whole state of the adjoint — λ, x̄, the
// stage cotangent, the physics pullback — in three bit-identical copies.  Here ONE wave (the helper, on the workgroup's fourth SIMD) carries
// it: per stage it forms k̄ = cwl λ + cwx x̄, runs the physics pullback once and hands the three dO over through LDS (barrier B); the net waves
// back-propagate their nets from dO_n, write the delta-tape record and their W1_n^T δz1_n parts to LDS (barrier A); the helper sums the
// parts into x̄.  While the helper works (between A and B) the net waves do what depends on the tapes alone: next stage's prefetch, this
// stage's activations, the record's x and a parts.  Every wave executes exactly the barriers B and A in every stage.
// ------------------------------------------------------------------------------------------------
// SPLIT (COLNDE_MATRIX_BF16X3_EXACT, RK4): the net waves' W1_n^T δz1_n products — 78 of a stage's 114 fp32 MFMAs, 3.0 k of its 8.2 k cycles — on
// v_mfma_f32_16x16x32_bf16 from exact three-way operand splits: δz1 is already held as the B operand needs it (lane group kq holds the features
// 4 Q + kq of its column: two 32-deep k-blocks, quads 0..7 and 8..12 + padding), W1_n^T comes pre-split (RT_NSA_*), planes h and m from LDS in the
// fp32 W1's place (the rest of the fp32 image moves down), plane l from L2 into registers before barrier B.
// SCHED (colnde_set_schedule; RK4): the intervals and their steps are walked in reverse with the forward kernel's counts — sched[iv] steps in save
// interval iv, the helper wave and the net waves alike — and the tapes and dW records are indexed by the running step counter (total_steps = sum of
// sched in n_steps' place).  One text compiled twice, as for the forward kernel: rt16sh_adjoint_body.inc under RT16SH_SCHED = 0 | 1.
template <int ACT, bool RICH, bool RKC = false, bool SPLIT = false>
__global__ void __launch_bounds__(256)
rt16sh_adjoint_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ save_times, int n_save, int substeps,
                      const float* __restrict__ sol, const float* __restrict__ truth, const float* __restrict__ t16_tape,
                      const float* __restrict__ t16_ztape, LossWeights lw, float* __restrict__ slab, int n_col,
                      float* __restrict__ dwtape, RtEns ens) {
#define RT16SH_SCHED 0
#define RT16SH_MEMBER 0
#include "rt16sh_adjoint_body.inc"
#undef RT16SH_MEMBER
#undef RT16SH_SCHED
}
// ... under a step schedule (RK4): the counts the forward kernel stepped with
template <int ACT, bool RICH, bool SPLIT>
__global__ void __launch_bounds__(256)
rt16sh_adjoint_sched_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ save_times, int n_save,
                            const float* __restrict__ sol, const float* __restrict__ truth, const float* __restrict__ t16_tape,
                            const float* __restrict__ t16_ztape, LossWeights lw, float* __restrict__ slab, int n_col,
                            float* __restrict__ dwtape, RtEns ens, const int* __restrict__ sched, int total_steps) {
    constexpr bool RKC = false;
    int substeps;                                          // the steps of the save interval in hand
#define RT16SH_SCHED 1
#define RT16SH_MEMBER 0
#include "rt16sh_adjoint_body.inc"
#undef RT16SH_MEMBER
#undef RT16SH_SCHED
}
// MEMBER (colnde_ensemble_set_member_loss): the same text once more under RT16SH_MEMBER = 1 — the helper wave reads the member's own loss
// weights, lwk[blockIdx.y] (wave-uniform), and this lane's column weight colw[blockIdx.y][column] once, before the interval loop; nothing is added inside
// the step or stage loops and the net waves' text is the same.  A preprocessor switch, as SCHED is, so that the kernels above keep their machine code.
template <int ACT, bool RICH, bool RKC = false, bool SPLIT = false>
__global__ void __launch_bounds__(256)
rt16sh_adjoint_member_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ save_times, int n_save, int substeps,
                             const float* __restrict__ sol, const float* __restrict__ truth, const float* __restrict__ t16_tape,
                             const float* __restrict__ t16_ztape, const LossWeights* __restrict__ lwk, const float* __restrict__ colw,
                             float* __restrict__ slab, int n_col, float* __restrict__ dwtape, RtEns ens) {
#define RT16SH_SCHED 0
#define RT16SH_MEMBER 1
#include "rt16sh_adjoint_body.inc"
#undef RT16SH_MEMBER
#undef RT16SH_SCHED
}
template <int ACT, bool RICH, bool SPLIT>
__global__ void __launch_bounds__(256)
rt16sh_adjoint_member_sched_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ save_times, int n_save,
                                   const float* __restrict__ sol, const float* __restrict__ truth, const float* __restrict__ t16_tape,
                                   const float* __restrict__ t16_ztape, const LossWeights* __restrict__ lwk, const float* __restrict__ colw,
                                   float* __restrict__ slab, int n_col, float* __restrict__ dwtape, RtEns ens, const int* __restrict__ sched,
                                   int total_steps) {
    constexpr bool RKC = false;
    int substeps;                                          // the steps of the save interval in hand
#define RT16SH_SCHED 1
#define RT16SH_MEMBER 1
#include "rt16sh_adjoint_body.inc"
#undef RT16SH_MEMBER
#undef RT16SH_SCHED
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// dynamic LDS of the kernels, in the order their heads carve rt_smem up
static constexpr size_t rt_pad4(size_t floats) { return (floats + 3) & ~(size_t)3; }
static constexpr size_t RT_IMG_BYTES = rt_pad4(RT_IMG_FLOATS) * sizeof(float);       // the fp32 weight image, padded to 16 bytes
static constexpr size_t RT16S_FWD_XCH = 3 * 2 * 64 * 16;                             // one exchange buffer of the net-split forward: [3 variables][2 tiles][64 lanes] x 16 bytes
static constexpr size_t RT16S_ADJ_XCH = 3 * 6 * 64 * 16;                             // ... of the net-split adjoint (the nets' parts of the state adjoint): [3 nets][6 tiles][64 lanes] x 16 bytes
static constexpr size_t RT16S_ADJ_STG = 3 * RT16S_STG * sizeof(float);               // the three net waves' record staging areas
// rt16s_forward_kernel: image, two exchange buffers
static size_t rt16s_forward_lds_bytes() { return RT_IMG_BYTES + 2 * RT16S_FWD_XCH; }
// rt16sh_forward_kernel: a third exchange buffer; SPLIT: the bf16 planes of layers 1 and 2 and the fp32 image from W3 on in the image's place
static size_t rt16sh_forward_lds_bytes(bool split) {
    return (split ? ((size_t)RT_SIMG2_WORDS + rt_pad4(RT_IMG_FLOATS - RT_W3C)) * sizeof(float) : RT_IMG_BYTES) + 3 * RT16S_FWD_XCH;
}
// rt16s_adjoint_kernel: image, two exchange buffers, staging
static size_t rt16s_adjoint_lds_bytes() { return RT_IMG_BYTES + 2 * RT16S_ADJ_XCH + RT16S_ADJ_STG; }
// rt16sh_adjoint_kernel: image, one exchange buffer, the helper's dO, staging; SPLIT: the fp32 image from W2 on, and the h / m planes of W1^T behind the staging
static size_t rt16sh_adjoint_lds_bytes(bool split) {
    const size_t rest = RT16S_ADJ_XCH + 3 * 2 * 64 * 16 + RT16S_ADJ_STG;
    return split ? rt_pad4(RT_IMG_FLOATS - RT_W2C) * sizeof(float) + rest + (size_t)RT_NSA_HM_WORDS * 4 : RT_IMG_BYTES + rest;
}
size_t rt_split_rich_record_floats() { return RT16S_RREC; }

// ---- kernel selection: one selector per kernel family, as in engine_regtile.hip (kernel_select.h)
using Rt16sForwardFn = decltype(&rt16s_forward_kernel<COLNDE_ACT_RELU, false>);
using Rt16shForwardFn = decltype(&rt16sh_forward_kernel<COLNDE_ACT_RELU, false>);
using Rt16sAdjointFn = decltype(&rt16s_adjoint_kernel<COLNDE_ACT_RELU, false>);
using Rt16shAdjointFn = decltype(&rt16sh_adjoint_kernel<COLNDE_ACT_RELU, false>);

static Rt16sForwardFn rt16s_forward_pick(int act, bool rich) {
    Rt16sForwardFn k = nullptr;
    with_act(act, [&](auto A) { with_bools([&](auto R) { k = rt16s_forward_kernel<decltype(A)::value, decltype(R)::value>; }, rich); });
    return k;
}
static Rt16shForwardFn rt16sh_forward_pick(int act, bool rich, bool rkc, bool split) {
    Rt16shForwardFn k = nullptr;
    with_act(act, [&](auto A) {
        with_bools([&](auto R, auto K, auto S) { k = rt16sh_forward_kernel<decltype(A)::value, decltype(R)::value, decltype(K)::value, decltype(S)::value>; }, rich, rkc, split);
    });
    return k;
}
using Rt16shForwardSchedFn = decltype(&rt16sh_forward_sched_kernel<COLNDE_ACT_RELU, false, false>);
using Rt16shAdjointSchedFn = decltype(&rt16sh_adjoint_sched_kernel<COLNDE_ACT_RELU, false, false>);
static Rt16shForwardSchedFn rt16sh_forward_sched_pick(int act, bool rich, bool split) {
    Rt16shForwardSchedFn k = nullptr;
    with_act(act, [&](auto A) { with_bools([&](auto R, auto S) { k = rt16sh_forward_sched_kernel<decltype(A)::value, decltype(R)::value, decltype(S)::value>; }, rich, split); });
    return k;
}
static Rt16shAdjointSchedFn rt16sh_adjoint_sched_pick(int act, bool rich, bool split) {
    Rt16shAdjointSchedFn k = nullptr;
    with_act(act, [&](auto A) { with_bools([&](auto R, auto S) { k = rt16sh_adjoint_sched_kernel<decltype(A)::value, decltype(R)::value, decltype(S)::value>; }, rich, split); });
    return k;
}
using Rt16shAdjointMemberFn = decltype(&rt16sh_adjoint_member_kernel<COLNDE_ACT_RELU, false>);
using Rt16shAdjointMemberSchedFn = decltype(&rt16sh_adjoint_member_sched_kernel<COLNDE_ACT_RELU, false, false>);
static Rt16shAdjointMemberFn rt16sh_adjoint_member_pick(int act, bool rich, bool rkc, bool split) {
    Rt16shAdjointMemberFn k = nullptr;
    with_act(act, [&](auto A) {
        with_bools([&](auto R, auto K, auto S) { k = rt16sh_adjoint_member_kernel<decltype(A)::value, decltype(R)::value, decltype(K)::value, decltype(S)::value>; }, rich, rkc, split);
    });
    return k;
}
static Rt16shAdjointMemberSchedFn rt16sh_adjoint_member_sched_pick(int act, bool rich, bool split) {
    Rt16shAdjointMemberSchedFn k = nullptr;
    with_act(act, [&](auto A) { with_bools([&](auto R, auto S) { k = rt16sh_adjoint_member_sched_kernel<decltype(A)::value, decltype(R)::value, decltype(S)::value>; }, rich, split); });
    return k;
}
static Rt16sAdjointFn rt16s_adjoint_pick(int act, bool rich) {
    Rt16sAdjointFn k = nullptr;
    with_act(act, [&](auto A) { with_bools([&](auto R) { k = rt16s_adjoint_kernel<decltype(A)::value, decltype(R)::value>; }, rich); });
    return k;
}
static Rt16shAdjointFn rt16sh_adjoint_pick(int act, bool rich, bool rkc, bool split) {
    Rt16shAdjointFn k = nullptr;
    with_act(act, [&](auto A) {
        with_bools([&](auto R, auto K, auto S) { k = rt16sh_adjoint_kernel<decltype(A)::value, decltype(R)::value, decltype(K)::value, decltype(S)::value>; }, rich, rkc, split);
    });
    return k;
}

hipError_t rt_set_attributes_split() {
    hipError_t e = hipSuccess;
    const size_t v = 160 * 1024;
    auto set = [&](auto* k) { if (k && e == hipSuccess) e = set_max_lds(k, v); };
    for_each_act([&](auto A) {
        for (int a = 0; a < 2; a++) {
            set(rt16s_forward_pick(A, a));
            set(rt16s_adjoint_pick(A, a));
            for (int b = 0; b < 2; b++)
                for (int c = 0; c < 2; c++) {
                    set(rt16sh_forward_pick(A, a, b, c));
                    set(rt16sh_adjoint_pick(A, a, b, c));
                    set(rt16sh_adjoint_member_pick(A, a, b, c));
                }
            for (int c = 0; c < 2; c++) {
                set(rt16sh_forward_sched_pick(A, a, c));
                set(rt16sh_adjoint_sched_pick(A, a, c));
                set(rt16sh_adjoint_member_sched_pick(A, a, c));
            }
        }
    });
    return e;
}

// the three-wavefronts-per-tile forward solve of the latency points; tapes (optional) in tile16's formats
hipError_t rt_launch_forward_split(const DevModel& m, const float* wimg, const float* x0, const float* bcs, const float* save_times,
                                   int n_save, int substeps, float* sol, float* t16_tape, float* t16_ztape, int n_col, bool rich, bool use_helper, bool want_split, hipStream_t stream,
                                   const RtEns& ens, const int* sched, int total_steps) {
    const dim3 grid((n_col + 15) / 16), block(192);
    const dim3 gridh((n_col + 15) / 16, ens.n_models), blockh(256);       // ensembles: grid.y = model (the four-wave kernels only)
    if (m.nst != 4 && !(m.rkc && use_helper)) return hipErrorInvalidValue;      // RKC2 lives in the four-wave kernels only
    if (sched && (!use_helper || m.rkc || m.nst != 4 || total_steps < n_save - 1)) return hipErrorInvalidValue;   // a schedule: the four-wave RK4 kernels only
    if (ens.n_models != 1 && !use_helper) return hipErrorInvalidValue;
    // layers 1 and 2 on the bf16 pipe with exact three-way operand splitting (COLNDE_MATRIX_BF16X3_EXACT; the four-wave kernels, RK4 and RKC2)
    const bool split = want_split && use_helper;
    if (split) hipLaunchKernelGGL(rt_pack_split_ns_kernel, dim3(41, ens.n_models), dim3(256), 0, stream, wimg, reinterpret_cast<unsigned*>(const_cast<float*>(wimg)) + RT_SIMG2_OFF, (int)ens.wimg);
    if (sched) {
        const auto k = rt16sh_forward_sched_pick(m.acts[0], rich, split);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, gridh, blockh, rt16sh_forward_lds_bytes(split), stream, m, wimg, x0, bcs, save_times, n_save, sol, t16_tape, t16_ztape, n_col, ens, sched, total_steps);
    } else if (use_helper) {
        const auto k = rt16sh_forward_pick(m.acts[0], rich, m.rkc != nullptr, split);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, gridh, blockh, rt16sh_forward_lds_bytes(split), stream, m, wimg, x0, bcs, save_times, n_save, substeps, sol, t16_tape, t16_ztape, n_col, ens);
    } else {
        const auto k = rt16s_forward_pick(m.acts[0], rich);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, grid, block, rt16s_forward_lds_bytes(), stream, m, wimg, x0, bcs, save_times, n_save, substeps, sol, t16_tape, t16_ztape, n_col);
    }
    return hipGetLastError();
}

bool rt_adjoint_split_has_bf16(const DevModel& m, bool use_helper) { return use_helper && (m.rkc || m.nst == 4); }

hipError_t rt_launch_adjoint_split(const DevModel& m, const float* wimg, const float* save_times, int n_save, int substeps, const float* sol,
                                   const float* truth, const float* t16_tape, const float* t16_ztape, const LossWeights& lw, float* slab,
                                   int n_col, float* dwtape, bool rich, bool use_helper, bool want_split, hipStream_t stream,
                                   const RtEns& ens, const int* sched, int total_steps, const LossWeights* member_lw, const float* member_colw) {
    if (sched && (!use_helper || m.rkc || m.nst != 4 || total_steps < n_save - 1)) return hipErrorInvalidValue;   // a schedule: the four-wave RK4 kernels only
    if ((member_lw != nullptr) != (member_colw != nullptr) || (member_lw && !use_helper)) return hipErrorInvalidValue;   // a member loss: the four-wave kernels only
    // the record formats this kernel reads and writes are tile16's for exactly this shape
    if (!rt_supported(m) || dwtape_row_floats(m) * CT != RT16S_REC || t16_ztape_col_floats(m) * CT != RT16S_ZREC || (m.nst != 4 && !(m.rkc && use_helper)))
        return hipErrorInvalidValue;
    const dim3 grid((n_col + 15) / 16), block(192);
    const dim3 gridh((n_col + 15) / 16, ens.n_models), blockh(256);       // ensembles: grid.y = model (the four-wave kernels only)
    if (ens.n_models != 1 && !use_helper) return hipErrorInvalidValue;
    // COLNDE_MATRIX_BF16X3_EXACT: the W1^T products on the bf16 pipe (four-wave kernels, RK4 and RKC2)
    const bool split = want_split && rt_adjoint_split_has_bf16(m, use_helper);
    if (split) hipLaunchKernelGGL(rt_pack_split_nsadj_kernel, dim3(36, ens.n_models), dim3(256), 0, stream, wimg, reinterpret_cast<unsigned*>(const_cast<float*>(wimg)) + RT_NSA_OFF, (int)ens.wimg);
    if (member_lw && sched) {
        const auto k = rt16sh_adjoint_member_sched_pick(m.acts[0], rich, split);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, gridh, blockh, rt16sh_adjoint_lds_bytes(split), stream, m, wimg, save_times, n_save, sol, truth, t16_tape, t16_ztape, member_lw, member_colw, slab, n_col, dwtape, ens, sched, total_steps);
    } else if (member_lw) {
        const auto k = rt16sh_adjoint_member_pick(m.acts[0], rich, m.rkc != nullptr, split);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, gridh, blockh, rt16sh_adjoint_lds_bytes(split), stream, m, wimg, save_times, n_save, substeps, sol, truth, t16_tape, t16_ztape, member_lw, member_colw, slab, n_col, dwtape, ens);
    } else if (sched) {
        const auto k = rt16sh_adjoint_sched_pick(m.acts[0], rich, split);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, gridh, blockh, rt16sh_adjoint_lds_bytes(split), stream, m, wimg, save_times, n_save, sol, truth, t16_tape, t16_ztape, lw, slab, n_col, dwtape, ens, sched, total_steps);
    } else if (use_helper) {
        const auto k = rt16sh_adjoint_pick(m.acts[0], rich, m.rkc != nullptr, split);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, gridh, blockh, rt16sh_adjoint_lds_bytes(split), stream, m, wimg, save_times, n_save, substeps, sol, truth, t16_tape, t16_ztape, lw, slab, n_col, dwtape, ens);
    } else {
        const auto k = rt16s_adjoint_pick(m.acts[0], rich);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, grid, block, rt16s_adjoint_lds_bytes(), stream, m, wimg, save_times, n_save, substeps, sol, truth, t16_tape, t16_ztape, lw, slab, n_col, dwtape);
    }
    return hipGetLastError();
}

hipError_t rt_debug_read_stamps_split(unsigned long long* out16) { return rt_read_unit_stamps(out16); }
