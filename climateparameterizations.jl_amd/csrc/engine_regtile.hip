// engine_regtile.hip — register-resident tile engine for the static wind-mixing shape (gfx950 / CDNA4 only): the kernels of the THROUGHPUT sizes.
// Engine MFMA, and engine AUTO above 8,192 columns (the benchmark), run these: rt16_forward_kernel (rt_forward_kernel with COLNDE_RT_FWD=32),
// rt_adjoint_kernel, the two dW1 kernels and their packers.  Up to 8,192 columns AUTO takes the net-split kernels of engine_netsplit.hip; what both
// share is in regtile_dev.h.
//
// One wavefront owns 32 columns.  Every quantity of a column lives in the MFMA 32x32 accumulator ("D") layout:
// lane (j = lane & 31, h = lane >> 5) holds, in element r of a 16-float tile, row  rho(r, h) = (r&3) + 8(r>>2) + 4h
// of column j.  With v_mfma_f32_32x32x2_f32 the B operand of k-step r is exactly element r of such a tile (K pair =
// rows rho(r,0), rho(r,1)), so a layer's output feeds the next layer with NO lane movement, no LDS round trip and no
// barrier: state [u;v;T] -> Dense(96,50) -> Dense(50,20) -> Dense(20,31) -> fluxes on faces, all in registers.
// The A operand (weights) is read from one compact LDS image (plain row-major matrices with odd row strides) as
// `per-lane base + compile-time immediate`: one ds_read_b32 per 64-cycle MFMA.  Vertical neighbours (the D^f / D^c
// stencils) are the previous/next tile element, except every fourth level where they sit in the partner lane (lane^32).
//
// Row placement (chosen here, free because K order and output-row order of a GEMM are arbitrary):
//   layer-1 outputs: the 3x50 features are stacked into 5 tiles; register G = 16*tile + r carries features
//                    (2g, 2g+1) of net n, with n = G / 25, g = G % 25 (G >= 75: padding, never consumed);
//   layer-2 outputs: registers r < 10 carry features (2r, 2r+1), the rest is padding;
//   layer-3 outputs: row = face index (row 0 = bottom boundary face, where the NN contributes nothing).
//
// Reference arithmetic: wind_mixing/src/NDE_training.jl:46-165 (NDE, predict_flux, predict_NDE).
#include <cstdlib>
#include "regtile_dev.h"
#include "kernel_select.h"

// (Tried and removed, see DESIGN.md §6: "parking" cotangents in an L2-resident scratch buffer to free registers — slower and
// 115 GB of extra traffic; prefetching the stage input one stage ahead — spilled under exposed waits.)
#ifndef RT16_WAVES
#define RT16_WAVES 8      // wavefronts per workgroup of the 16-column forward kernel (two per SIMD)
#endif
#ifndef RT_ADJ_CH
#define RT_ADJ_CH 8       // A-operand prefetch depth (k-steps) of the adjoint kernel's layer-1 chains
#endif
#define RT_TAPEZ (20 * 256)   // floats per (tile, step, stage) of the layer-1 pre-activation tape: the forward kernel's 10 tiles x 2 lane pairs x 64 lanes x 4
#define RT_TAPE2 (20 * 256)   // ... of the layer-1 delta tape: 20 groups x 64 lanes x 4, the three nets' 25 registers stacked (G = 25 n + g)

// Row stacking of layer 1 in the 16-column forward kernels (and so of the Z1 tape record): ten 16-row tiles, stacked quad Q = 4 t + e is element e of tile t and
// carries features 4 qq + g of one net.  A net has 13 quads (52 rows, 2 of them padding).  Its twelve full quads fill three whole tiles, Q = 12 n + qq (tiles
// 3n .. 3n+2); tile 9 takes the three half-empty quads qq = 12 (features 48, 49), net n in element n, and one slot of padding (Q = 39).  So every 16-byte group
// of the record but tile 9's belongs to ONE net, and the adjoint fetches no element it does not keep.  The one place that knows the map:
__host__ __device__ constexpr int rt16_q_net(int Q) { return Q < 36 ? Q / 12 : Q - 36; }          // Q = 39: padding (callers test Q < 39)
__host__ __device__ constexpr int rt16_q_quad(int Q) { return Q < 36 ? Q % 12 : 12; }
__host__ __device__ constexpr int rt16_q_slot(int n, int qq) { return qq < 12 ? 12 * n + qq : 36 + n; }

// The three MLPs on the stage input X (3 tiles u, v, T) -> face-flux tiles O (3 tiles), all in registers.
// The activations of a finished tile are issued as "filler" inside the next chain's chunks (MFMA shadow).
template <int ACT>
__device__ __forceinline__ void rt_mlp_forward(const float* wl, const RtBases& b, const f32x16 (&X)[3], int h, f32x16 (&O)[3]) {
    f32x16 A1[5];      // holds the raw pre-activation of a tile until the next chain's filler activates it in place
#pragma unroll
    for (int mt = 0; mt < 5; mt++) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int G = mt * 16 + r;
            acc[r] = wl[RT_B1C + (G < 75 ? (G / 25) * 50 + 2 * (G % 25) : 150 + 2 * (G - 75)) + h];
        }
        const int base = b.a1[mt];
        A1[mt] = rt_chain_fill<48, 8>(wl, acc, [=](int s) { return base + (s >> 4) * 32 + RHO0(s & 15); },
                                      [&](int s) { return X[s >> 4][s & 15]; },
                                      [&](int c) {
                                          if (mt > 0) {
#pragma unroll
                                              for (int r = 0; r < 16; r++)
                                                  if (r / 3 == c) A1[mt > 0 ? mt - 1 : 0][r] = rt_act<ACT>(A1[mt > 0 ? mt - 1 : 0][r]);
                                          }
                                      });
    }
    f32x16 Z2[3];
#pragma unroll
    for (int n = 0; n < 3; n++) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = r < 10 ? wl[RT_B2C + n * 20 + 2 * r + h] : 0.0f;
        const int base2 = b.a2 + n * 20 * RT_LD2;
        // net 0 reads layer-1 registers G < 25 only, so tile 4 (G >= 64) can still be activated under its chain;
        // nets 1, 2 activate the previous net's layer-2 outputs
        Z2[n] = rt_chain_fill<25, 5>(wl, acc, [=](int s) { return base2 + 2 * s; },
                                     [&](int s) { return A1[(25 * n + s) >> 4][(25 * n + s) & 15]; },
                                     [&](int c) {
                                         if (n == 0) {
#pragma unroll
                                             for (int r = 0; r < 16; r++)
                                                 if (r / 4 == c) A1[4][r] = rt_act<ACT>(A1[4][r]);
                                         } else {
#pragma unroll
                                             for (int r = 0; r < 10; r++)
                                                 if (r / 2 == c) Z2[n > 0 ? n - 1 : 0][r] = rt_act<ACT>(Z2[n > 0 ? n - 1 : 0][r]);
                                         }
                                     });
    }
#pragma unroll
    for (int r = 0; r < 10; r++) Z2[2][r] = rt_act<ACT>(Z2[2][r]);
#pragma unroll
    for (int n = 0; n < 3; n++) {
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; r++) o[r] = wl[RT_B3C + n * 32 + RHO0(r) + 4 * h];
        const int base3 = b.a3 + n * 31 * RT_LD3;
        O[n] = rt_chain<10, 10>(wl, o, [=](int s) { return base3 + 2 * s; }, [&](int s) { return Z2[n][s]; });
    }
}

struct RtBC { float b[3], t[3]; };   // scaled bottom / top fluxes of (uw, vw, wT) for this lane's column

// K = RHS(X) given the NN face fluxes O  (predict_flux :104-147, predict_NDE :160-162; MPP / CA branches, zero_weights)
__device__ __forceinline__ void rt_physics_forward(const DevModel& m, const f32x16 (&X)[3], const f32x16 (&O)[3],
                                                   const RtBC& bc, int h, f32x16 (&K)[3]) {
    const float Nz = 32.0f;
    f32x16 F[3];
    if (m.mpp || m.ca) {
        const f32x16 Ud = shift_down(X[0], h, 0.0f), Vd = shift_down(X[1], h, 0.0f), Td = shift_down(X[2], h, 0.0f);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const bool in = !(r == 0 && h == 0);                   // face rho(r,h) >= 1 (face 0 is the bottom boundary)
            const float gu = in ? (X[0][r] - Ud[r]) * Nz : 0.0f;
            const float gv = in ? (X[1][r] - Vd[r]) * Nz : 0.0f;
            const float gT = in ? (X[2][r] - Td[r]) * Nz : 0.0f;
            float f0 = in ? O[0][r] : 0.0f, f1 = in ? O[1][r] : 0.0f, f2 = in ? O[2][r] : 0.0f;
            if (!m.zero_w && !in) { f0 = bc.b[0]; f1 = bc.b[1]; f2 = bc.b[2]; }
            if (m.mpp) {
                if (in) {
                    const float a1 = m.sig_u * (gu + m.eps), a2 = m.sig_v * (gv + m.eps);
                    const float Ri = fast_div(m.B * (gT + m.eps), a1 * a1 + a2 * a2);
                    const float e = __expf(2.0f * fminf(fmaxf((Ri - m.Ric) * m.inv_dRi, -15.0f), 15.0f));
                    const float th = 1.0f - fast_div(2.0f, 1.0f + e);
                    const float nu = m.nu0 + m.nu_minus * (1.0f - th) * 0.5f;
                    f0 -= m.cs[0] * nu * gu;
                    f1 -= m.cs[1] * nu * gv;
                    f2 -= m.cs[2] * (nu * m.inv_Pr) * gT;
                } else if (m.zero_w) {
                    f0 += bc.b[0] - m.s0[0];
                    f1 += bc.b[1] - m.s0[1];
                    f2 += bc.b[2] - m.s0[2];
                }
            } else if (in) {
                f2 -= m.cs[2] * m.kappa * fminf(0.0f, gT);
            }
            F[0][r] = f0; F[1][r] = f1; F[2][r] = f2;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const bool in = !(r == 0 && h == 0);
            F[0][r] = in ? O[0][r] : bc.b[0];
            F[1][r] = in ? O[1][r] : bc.b[1];
            F[2][r] = in ? O[2][r] : bc.b[2];
        }
    }
    // top boundary face (face Nz): zero_weights: 0 - (-(BC - s(0))) ; else the BC itself
    float top[3];
#pragma unroll
    for (int k = 0; k < 3; k++) top[k] = m.zero_w ? bc.t[k] - m.s0[k] : bc.t[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const f32x16 Fu = shift_up(F[k], h, top[k]);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            float v = -m.A[k] * (Fu[r] - F[k][r]);
            if (k == 0) v += m.cor_u * (m.sig_v * X[1][r] + m.mu_v);
            if (k == 1) v -= m.cor_v * (m.sig_u * X[0][r] + m.mu_u);
            K[k][r] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// weight image
// ------------------------------------------------------------------------------------------------
__global__ void rt_pack_kernel(DevModel m, const float* __restrict__ w, float* __restrict__ img, int img_stride) {
    // ensembles: blockIdx.y = model, weights [K][n_params] -> images img_stride floats apart (grid.y = 1: one model)
    w += (size_t)blockIdx.y * m.n_params;
    img += (size_t)blockIdx.y * img_stride;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < RT_IMG_FLOATS; e += gridDim.x * blockDim.x) {
        float v = 0.0f;
        if (e < RT_W2C) {
            const int row = e / RT_LD1, c = e - row * RT_LD1;
            if (row < 150 && c < 96) { const int n = row / 50, f = row - n * 50; v = w[n * m.net_size + m.w_off[0] + c * 50 + f]; }
        } else if (e < RT_W3C) {
            const int q = e - RT_W2C, row = q / RT_LD2, c = q - row * RT_LD2;
            if (row < 60 && c < 50) { const int n = row / 20, f = row - n * 20; v = w[n * m.net_size + m.w_off[1] + c * 20 + f]; }
        } else if (e < RT_B1C) {
            const int q = e - RT_W3C, row = q / RT_LD3, c = q - row * RT_LD3;
            if (row < 93 && c < 20) { const int n = row / 31, f = row - n * 31; v = w[n * m.net_size + m.w_off[2] + c * 31 + f]; }
        } else if (e < RT_B2C) {
            const int q = e - RT_B1C;
            if (q < 150) { const int n = q / 50, f = q - n * 50; v = w[n * m.net_size + m.b_off[0] + f]; }
        } else if (e < RT_B3C) {
            const int q = e - RT_B2C;
            if (q < 60) { const int n = q / 20, f = q - n * 20; v = w[n * m.net_size + m.b_off[1] + f]; }
        } else {
            const int q = e - RT_B3C, n = q / 32, face = q - n * 32;
            if (face >= 1) v = w[n * m.net_size + m.b_off[2] + face - 1];
        }
        img[e] = v;
    }
}


// The forward nets as A operands of v_mfma_f32_16x16x32_bf16 (COLNDE_MATRIX_BF16X3_EXACT), made from the fp32 image: group G, plane p, lane (i = lane & 15,
// kg = lane >> 4), element e = the weight that multiplies the B element e of lane (column, kg) — see rt16_forward_kernel<ACT, true>:
//   layer 1, G = 3 t + q            : row of quad Q = 4 t + (i & 3), feature 4 rt16_q_quad(Q) + (i >> 2) of net rt16_q_net(Q); input 32 q + level(kg, e),
//                                     level = e < 4 ? 4 kg + e : 16 + 4 kg + (e - 4)          (the two D tiles of a 32-level variable)
//   layer 2, G = 30 + 4 n + 2 u + c : output 4 (4 u + (i & 3)) + (i >> 2) (< 20) of net n; input feature 4 (8 c + e) + kg (< 50)
//   layer 3, G = 42 + 2 n + v       : face 16 v + i (>= 1) of net n; input feature 4 e + kg (e < 5)
// everything else is zero.  The three planes are the exact truncation split of the fp32 weight.
__global__ void rt_pack_split_kernel(const float* __restrict__ img, unsigned* __restrict__ simg) {
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < RT_SIMG_GROUPS * 64 * 4; x += gridDim.x * blockDim.x) {
        const int G = x >> 8, lane = (x >> 2) & 63, pr = x & 3;           // pr: the pair of elements (2 pr, 2 pr + 1)
        const int i = lane & 15, kg = lane >> 4, g_i = i >> 2, r_i = i & 3;
        float v[2];
#pragma unroll
        for (int z = 0; z < 2; z++) {
            const int e = 2 * pr + z;
            float w = 0.0f;
            if (G < 30) {
                const int t = G / 3, q = G - 3 * t, Q = 4 * t + r_i, f = 4 * rt16_q_quad(Q) + g_i;
                const int lev = e < 4 ? 4 * kg + e : 16 + 4 * kg + (e - 4);
                if (Q < 39 && f < 50) w = img[RT_W1C + (rt16_q_net(Q) * 50 + f) * RT_LD1 + 32 * q + lev];
            } else if (G < 42) {
                const int y = G - 30, n = y >> 2, u = (y >> 1) & 1, c = y & 1;
                const int Q2 = 4 * u + r_i, qq = 8 * c + e, f = 4 * qq + kg;
                if (Q2 < 5 && qq < 13 && f < 50) w = img[RT_W2C + (n * 20 + 4 * Q2 + g_i) * RT_LD2 + f];
            } else {
                const int y = G - 42, n = y >> 1, vv = y & 1, face = 16 * vv + i;
                if (face >= 1 && e < 5) w = img[RT_W3C + (n * 31 + face - 1) * RT_LD3 + 4 * e + kg];
            }
            v[z] = w;
        }
        const float r0 = v[0] - __uint_as_float(__float_as_uint(v[0]) & 0xffff0000u), r1 = v[1] - __uint_as_float(__float_as_uint(v[1]) & 0xffff0000u);
        const float l0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u), l1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
        unsigned* o = simg + (size_t)G * 3 * 256 + lane * 4 + pr;
        o[0] = (__float_as_uint(v[1]) & 0xffff0000u) | (__float_as_uint(v[0]) >> 16);
        o[256] = (__float_as_uint(r1) & 0xffff0000u) | (__float_as_uint(r0) >> 16);
        o[512] = (__float_as_uint(l1) & 0xffff0000u) | (__float_as_uint(l0) >> 16);
    }
}

// ... and for the adjoint's W1^T operands (RT_ASIMG_*)
__global__ void rt_pack_split_adj_kernel(const float* __restrict__ img, unsigned* __restrict__ simg) {
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < 27 * 256 + 576; x += gridDim.x * blockDim.x) {
        if (x >= 27 * 256) {
            const int y = x - 27 * 256, n = y / 192, kh = (y / 96) & 1, c = y % 96;
            reinterpret_cast<float*>(simg)[RT_ASIMG_LEFT + y] = img[RT_W1C + (n * 50 + 48 + kh) * RT_LD1 + c];
            continue;
        }
        const int G = x >> 8, lane = (x >> 2) & 63, pr = x & 3;
        const int n = G / 9, c = (G / 3) % 3, q = G % 3, m = lane & 31, kh = lane >> 5;
        const float v0 = img[RT_W1C + (n * 50 + 2 * (8 * c + 2 * pr) + kh) * RT_LD1 + 32 * q + m];
        const float v1 = img[RT_W1C + (n * 50 + 2 * (8 * c + 2 * pr + 1) + kh) * RT_LD1 + 32 * q + m];
        const float r0 = v0 - __uint_as_float(__float_as_uint(v0) & 0xffff0000u), r1 = v1 - __uint_as_float(__float_as_uint(v1) & 0xffff0000u);
        const float l0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u), l1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
        simg[(size_t)(G * 2) * 256 + lane * 4 + pr] = (__float_as_uint(v1) & 0xffff0000u) | (__float_as_uint(v0) >> 16);
        simg[(size_t)(G * 2 + 1) * 256 + lane * 4 + pr] = (__float_as_uint(r1) & 0xffff0000u) | (__float_as_uint(r0) >> 16);
        simg[RT_ASIMG_L + (size_t)G * 256 + lane * 4 + pr] = (__float_as_uint(l1) & 0xffff0000u) | (__float_as_uint(l0) >> 16);
    }
}

// ------------------------------------------------------------------------------------------------
// forward solve (classical RK4); stage inputs -> tape in register-image order
//   tape[((tile*n_steps + step)*4 + stage)*3072 + (q*4 + g)*256 + lane*4 + e] = X[q][4g + e]
// ------------------------------------------------------------------------------------------------
template <int ACT>
__global__ void __launch_bounds__(256)
rt_forward_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ x0, const float* __restrict__ bcs,
                  const float* __restrict__ save_times, int n_save, int substeps, float* __restrict__ sol,
                  float* __restrict__ tape, int n_col) {
    float* wl = rt_smem;
    for (int e = threadIdx.x; e < RT_IMG_FLOATS; e += blockDim.x) wl[e] = wimg[e];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x * RT_WAVES + wave;
    if (tile * RT_COLS >= n_col) return;                    // no barrier after this point: waves are independent
    const int col = tile * RT_COLS + j;
    const bool valid = col < n_col;
    const int colc = min(col, n_col - 1);
    const RtBases bases = rt_bases(lane);
    RtBC bc;
    float bc5;
    {
        const float* bp = bcs + (size_t)colc * 6;
        bc.b[0] = bp[0]; bc.t[0] = bp[1]; bc.b[1] = bp[2]; bc.t[1] = bp[3]; bc.b[2] = bp[4]; bc5 = bp[5];
        bc.t[2] = bc5;
    }
    f32x16 Xn[3];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const f32x4v v = *reinterpret_cast<const f32x4v*>(x0 + (size_t)colc * 96 + q * 32 + 8 * g + 4 * h);
            Xn[q][4 * g] = v[0]; Xn[q][4 * g + 1] = v[1]; Xn[q][4 * g + 2] = v[2]; Xn[q][4 * g + 3] = v[3];
            if (sol && valid) *reinterpret_cast<f32x4v*>(sol + ((size_t)col * n_save) * 96 + q * 32 + 8 * g + 4 * h) = v;
        }
    const int n_steps = (n_save - 1) * substeps;
    float* tp = tape ? tape + (size_t)tile * n_steps * 4 * 3072 : nullptr;
    int step = 0;
    for (int iv = 0; iv < n_save - 1; iv++) {
        const float t0 = save_times[iv];
        const float dt = (save_times[iv + 1] - t0) / (float)substeps;
        for (int s = 0; s < substeps; s++, step++) {
            const float ts = t0 + (float)s * dt;
            f32x16 Xs[3], Ks[3], Kacc[3];
#pragma unroll
            for (int q = 0; q < 3; q++) { Xs[q] = Xn[q]; Kacc[q] = Xn[q] - Xn[q]; }
#pragma nounroll
            for (int st = 0; st < 4; st++) {
                const float ca = st == 0 ? 0.0f : (st == 3 ? 1.0f : 0.5f);
                const float cb = (st == 0 || st == 3) ? 1.0f / 6.0f : 1.0f / 3.0f;
                if (st > 0) {
#pragma unroll
                    for (int q = 0; q < 3; q++) Xs[q] = Xn[q] + (ca * dt) * Ks[q];
                }
                if (tp) {
                    float* o = tp + ((size_t)step * 4 + st) * 3072 + lane * 4;
#pragma unroll
                    for (int q = 0; q < 3; q++)
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            f32x4v v = {Xs[q][4 * g], Xs[q][4 * g + 1], Xs[q][4 * g + 2], Xs[q][4 * g + 3]};
                            *reinterpret_cast<f32x4v*>(o + (q * 4 + g) * 256) = v;
                        }
                }
                bc.t[2] = rt_top_flux(m, bc5, ts + ca * dt);
                f32x16 O[3];
                rt_mlp_forward<ACT>(wl, bases, Xs, h, O);
                rt_physics_forward(m, Xs, O, bc, h, Ks);
#pragma unroll
                for (int q = 0; q < 3; q++) Kacc[q] += cb * Ks[q];
            }
#pragma unroll
            for (int q = 0; q < 3; q++) Xn[q] += dt * Kacc[q];
            if (s == substeps - 1 && sol && valid) {
#pragma unroll
                for (int q = 0; q < 3; q++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        f32x4v v = {Xn[q][4 * g], Xn[q][4 * g + 1], Xn[q][4 * g + 2], Xn[q][4 * g + 3]};
                        *reinterpret_cast<f32x4v*>(sol + ((size_t)col * n_save + iv + 1) * 96 + q * 32 + 8 * g + 4 * h) = v;
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// adjoint (back-propagation through the RK4 stages), register-resident
// ------------------------------------------------------------------------------------------------
template <int ACT>
__device__ __forceinline__ void rt_act_pair4_at(f32x16 (&A)[2], f32x16 (&D)[2], int G) {     // registers G .. G+3 (G % 4 == 0)
    f32x2v z0 = {A[G >> 4][G & 15], A[G >> 4][(G & 15) + 1]}, z1 = {A[G >> 4][(G & 15) + 2], A[G >> 4][(G & 15) + 3]}, a0, d0, a1, d1;
    rt_act_pair4<ACT>(z0, z1, a0, d0, a1, d1);
    A[G >> 4][G & 15] = a0.x; A[G >> 4][(G & 15) + 1] = a0.y; A[G >> 4][(G & 15) + 2] = a1.x; A[G >> 4][(G & 15) + 3] = a1.y;
    D[G >> 4][G & 15] = d0.x; D[G >> 4][(G & 15) + 1] = d0.y; D[G >> 4][(G & 15) + 2] = d1.x; D[G >> 4][(G & 15) + 3] = d1.y;
}

// in place on register G' of a two-tile layer-1 block: A <- act(A), D <- act'(A)
template <int ACT>
__device__ __forceinline__ void rt_act_pair_at(f32x16 (&A)[2], f32x16 (&D)[2], int G) {
    float av, dv;
    rt_act_pair<ACT>(A[G >> 4][G & 15], av, dv);
    A[G >> 4][G & 15] = av;
    D[G >> 4][G & 15] = dv;
}

// Pullback of rt_physics_forward.  On entry kd holds the stage cotangent k̄; on exit it holds dO = the cotangent of the NN
// face fluxes (0 on face 0) and xb the physics part of the state cotangent (flux-divergence transpose + Coriolis).
// Ordered so that k̄ is consumed in place (Coriolis first, then F̄ overwrites k̄): this phase is the kernel's
// register-pressure peak.
__device__ __forceinline__ void rt_physics_vjp(const DevModel& m, const f32x16 (&X)[3], f32x16 (&kd)[3], int h, f32x16 (&xb)[3]) {
    const float Nz = 32.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        xb[0][r] = -m.cor_v * m.sig_u * kd[1][r];
        xb[1][r] = m.cor_u * m.sig_v * kd[0][r];
        xb[2][r] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const f32x16 dn = shift_down(kd[k], h, 0.0f);
#pragma unroll
        for (int r = 0; r < 16; r++) kd[k][r] = (r == 0 && h == 0) ? 0.0f : m.A[k] * (kd[k][r] - dn[r]);
    }
    if (!m.mpp && !m.ca) return;
    f32x16 gb[3];
    if (m.mpp) {
        const f32x16 Ud = shift_down(X[0], h, 0.0f), Vd = shift_down(X[1], h, 0.0f), Td = shift_down(X[2], h, 0.0f);
        // Same arithmetic as rt_physics_forward's diffusivity and its derivative, with every uniform factor folded into a handful
        // of wave-uniform constants (this phase has no MFMA beside it: each vector instruction is fully exposed).
        // level differences d = X[r] - X[r-1];  gu = Nz d_u etc.;  a1 = σ_u (gu + ε);  S2 = a1² + a2²;  Ri = B (gT + ε) / S2
        const float cU = m.sig_u * Nz, sU = m.sig_u * m.eps, cV = m.sig_v * Nz, sV = m.sig_v * m.eps, cB = m.B * Nz, sB = m.B * m.eps;
        // tanh((Ri - Riᶜ)/ΔRi) = 1 - 2 / (1 + exp2(kE Ri + oE)), argument clamped to ±30 log2(e)
        const float L2E = 1.4426950408889634f;
        const float kE = 2.0f * m.inv_dRi * L2E, oE = -2.0f * m.Ric * m.inv_dRi * L2E, cE = 30.0f * L2E;
        const float nA = -0.5f * m.nu_minus, nB = m.nu0 + 0.5f * m.nu_minus;                    // ν = nB + nA tanh
        const float m0 = -m.cs[0], m1 = -m.cs[1], m2 = -m.cs[2] * m.inv_Pr;                      // g_k = k̄_k ν m_k  (D = -k̄)
        const float n0 = m0 * Nz * m.c_rib, n1 = m1 * Nz * m.c_rib, n2 = m2 * Nz * m.c_rib;      // c_rib Σ D_k c_k g_k = Σ k̄_k d_k n_k
        const float q0 = -2.0f * m.sig_u, q1 = -2.0f * m.sig_v;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const bool in = !(r == 0 && h == 0);
            const float dU = X[0][r] - Ud[r], dV = X[1][r] - Vd[r], dT = X[2][r] - Td[r];
            const float a1 = fmaf(dU, cU, sU), a2 = fmaf(dV, cV, sV);
            const float rS = __builtin_amdgcn_rcpf(fmaf(a2, a2, a1 * a1));
            const float Ri = fmaf(dT, cB, sB) * rS;
            const float e = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(fmaf(Ri, kE, oE), -cE, cE));
            const float th = fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);
            const float nu = fmaf(th, nA, nB);
            const float t0 = kd[0][r] * nu, t1 = kd[1][r] * nu, t2 = kd[2][r] * nu;
            float nub = (kd[0][r] * dU) * n0;
            nub = fmaf(kd[1][r] * dV, n1, nub);
            nub = fmaf(kd[2][r] * dT, n2, nub);
            const float w = nub * (fmaf(-th, th, 1.0f) * rS);                                  // c_rib (1 - tanh²) Σ… / S2
            const float qq = w * Ri;
            const float g2 = fmaf(w, m.B, t2 * m2);
            const float g0 = fmaf(qq, a1 * q0, t0 * m0);
            const float g1 = fmaf(qq, a2 * q1, t1 * m1);
            gb[0][r] = in ? g0 : 0.0f;
            gb[1][r] = in ? g1 : 0.0f;
            gb[2][r] = in ? g2 : 0.0f;
        }
    } else {
        const f32x16 Td = shift_down(X[2], h, 0.0f);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const bool in = !(r == 0 && h == 0);
            const float gT = (X[2][r] - Td[r]) * Nz;
            gb[0][r] = 0.0f;
            gb[1][r] = 0.0f;
            gb[2][r] = (in && gT < 0.0f) ? -kd[2][r] * m.cs[2] * m.kappa : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const f32x16 gu_ = shift_up(gb[k], h, 0.0f);
#pragma unroll
        for (int r = 0; r < 16; r++) xb[k][r] += (gb[k][r] - gu_[r]) * Nz;
    }
}

// Cache policy of the tape streams (written once, read once, 100+ GB per step).  Measured in one process: non-temporal LDS-DMA in the dW1 kernel
// 19.92 -> 19.66 ms, non-temporal delta-tape stores in the adjoint 64.1 -> 63.8 ms; the forward kernel's tape stores showed nothing either way
// and stay default.
#define RT_DMA_AUX 2                                   // aux of global_load_lds: 2 = nt
// (in fc32 non-temporal tape STORES were the slower choice; here they are not — profiles/r03l_ab_regtile_nt.log)
#define RT_NT_STORE4(p, v) __builtin_nontemporal_store((f32x4v)(v), reinterpret_cast<f32x4v*>(p))
#define RT_TAPE_LOAD4(p) __builtin_nontemporal_load(reinterpret_cast<const f32x4v*>(p))   // the adjoint's stage-input and Z1 tape loads: 63.75 -> 63.48 ms
#define RT_TB (32 * 36)   // floats of a wave's transposition tile
// λ in LDS, wave-private: element e of a lane at [e / 4][lane][e % 4] — four consecutive elements are one 16-byte access
#define RT_LAM(e, lane) ((((e) >> 2) * 64 + (lane)) * 4 + ((e) & 3))
// LDS transposition buffer (one 32 x 36 float tile per wave): a D-layout tile (lane = column) becomes the MFMA operand of
// a product contracted over the 32 columns (lane = row, k-step s = columns 2s, 2s+1)
__device__ __forceinline__ f32x16 rt_transpose(float* tb, const f32x16 T, int wbase, int rbase) {
    // tile stored [column][row] with a 36-float column stride: the four registers 4a .. 4a+3 of a lane are rows 8a + 4h .. + 3 of its column —
    // one 16-byte write each; the operand of k-step s, lane (row m, kh), is tile[(2 s + kh)][m]
#pragma unroll
    for (int a = 0; a < 4; a++)
        *reinterpret_cast<f32x4v*>(tb + wbase + 8 * a) = (f32x4v){T[4 * a], T[4 * a + 1], T[4 * a + 2], T[4 * a + 3]};
    f32x16 o;
#pragma unroll
    for (int s = 0; s < 16; s++) o[s] = tb[rbase + 72 * s];
    return o;
}

__device__ __forceinline__ f32x16 rt_outer(f32x16 acc, const f32x16 TA, const f32x16 TB) {
#pragma unroll
    for (int s = 0; s < 16; s++) acc = mfma32(TA[s], TB[s], acc);
    return acc;
}

__device__ __forceinline__ float rt_sum16(const f32x16 v) {
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) s += v[r];
    return s;
}

// which nets own registers of layer-1 tile mt (register G = 16 mt + r belongs to net G / 25)
#define RT_NET_LO(mt) (((mt) * 16) / 25)
#define RT_NET_HI(mt) ((((mt) * 16 + 15) < 75 ? ((mt) * 16 + 15) : 74) / 25)
// index of the (net, tile) weight-gradient accumulator: combos (0,0) (0,1) (1,1) (1,2) (1,3) (2,3) (2,4)
__host__ __device__ constexpr int rt_combo(int n, int mt) { return n == 0 ? mt : (n == 1 ? 1 + mt : 2 + mt); }

// tape of stage inputs (written by rt_forward_kernel):  [tile][step][stage][12 groups][64 lanes][4]
// tape2 of layer-1 deltas (written here, read by rt_dw1_kernel): [tile][step][stage][20 groups][64 lanes][4]; element e of
// group grp is stacked register G = 4 grp + e = 25 n + g (features 2g, 2g+1 of net n; G >= 75: never written, never used)
// SPLIT (COLNDE_MATRIX_BF16X3_EXACT; with the Z1 tape only): the W1^T products — 225 of the stage's 552 fp32 MFMAs — on v_mfma_f32_32x32x16_bf16 from exact three-way
// operand splits (csrc/split_bf16.h): the h and m planes of W1^T take the fp32 W1's place in LDS, the l planes come from L2 into registers, the delta
// registers are split per 16-deep k-block; features 48, 49 of a net (register 24) keep one fp32 k-step.
template <int ACT, bool ZT, bool SPLIT = false>
__global__ void __launch_bounds__(256)
rt_adjoint_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ bcs,
                  const float* __restrict__ save_times, int n_save, int substeps, const float* __restrict__ sol,
                  const float* __restrict__ truth, const float* __restrict__ tape, float* __restrict__ tape2,
                  const float* __restrict__ tapez /* layer-1 pre-activations taped by the forward kernel (ZT) */,
                  LossWeights lw, float* __restrict__ slab, int n_col) {
    static_assert(!SPLIT || ZT, "the split W1^T operands replace the fp32 W1 in LDS: no layer-1 recomputation");
    float* wl = rt_smem;
    if constexpr (SPLIT) {
        // LDS: the h, m planes of W1^T and the fp32 rows of features 48, 49 take the fp32 W1's place (14,400 of its 14,552 floats); the fp32 image from
        // W2 on stays where it is, so wl[RT_W2C ...] etc. are unchanged
        static_assert(RT_ASIMG_HM_WORDS + 576 <= RT_W2C, "the split W1^T operands must fit the fp32 W1's place");
        const u32x4* src = reinterpret_cast<const u32x4*>(wimg + RT_ASIMG_OFF);
        for (int e = threadIdx.x; e < (RT_ASIMG_HM_WORDS + 576) / 4; e += blockDim.x) reinterpret_cast<u32x4*>(rt_smem)[e] = src[e];
        for (int e = RT_W2C + threadIdx.x; e < RT_IMG_FLOATS; e += blockDim.x) wl[e] = wimg[e];
    } else {
        for (int e = threadIdx.x; e < RT_IMG_FLOATS; e += blockDim.x) wl[e] = wimg[e];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x * RT_WAVES + wave;
    if (tile * RT_COLS >= n_col) return;
    float* lam = rt_smem + ((RT_IMG_FLOATS + 3) & ~3) + wave * (3072 + RT_TB);   // λ: [48][64] floats, wave-private (16-byte aligned base)
    float* tb = lam + 3072;                                            // transposition tile [32 columns][36]
    const int col = tile * RT_COLS + j;
    const bool valid = col < n_col;
    const int i_ = lane & 31, r_i = (i_ & 3) + 4 * (i_ >> 3), h_i = (i_ >> 2) & 1;
    // per-net layer-1 tiles (n, t): register G' = 16 t + r carries features (2G', 2G'+1) of net n (G' >= 25: padding)
    int a1n[2];
#pragma unroll
    for (int t = 0; t < 2; t++) a1n[t] = RT_W1C + (2 * min(t * 16 + r_i, 24) + h_i) * RT_LD1 + 4 * h;
    const int a2b = RT_W2C + ((r_i < 10) ? 2 * r_i + h_i : 0) * RT_LD2 + h;
    // transposed-product bases
    const int f2c = (r_i < 10) ? 2 * r_i + h_i : 20;                                   // a2 feature of output row i_ (20 = zero column)
    const int b3T = RT_W3C + (4 * h - 1) * RT_LD3 + f2c;
    int b2T[2];
#pragma unroll
    for (int t = 0; t < 2; t++) b2T[t] = RT_W2C + h * RT_LD2 + ((t * 16 + r_i < 25) ? 2 * (t * 16 + r_i) + h_i : 50);   // 50 = zero column
    const int b1T = RT_W1C + h * RT_LD1 + i_;
    const int wbase = j * 36 + 4 * h, rbase = h * 36 + i_;

    f32x16 gW3[3], gW2[3][2];
#pragma unroll
    for (int q = 0; q < 3; q++) { gW3[q] = (f32x16)(0.0f); gW2[q][0] = (f32x16)(0.0f); gW2[q][1] = (f32x16)(0.0f); }
    float b2acc[3] = {0, 0, 0}, b3acc[3] = {0, 0, 0};
    float sums[6] = {0, 0, 0, 0, 0, 0};
    RT_STAMP_DECL;
    f32x16 xb[3], X[3];
#pragma unroll
    for (int q = 0; q < 3; q++) xb[q] = (f32x16)(0.0f);
    f32x16 xbs[3];
#pragma unroll
    for (int q = 0; q < 3; q++) xbs[q] = (f32x16)(0.0f);
#pragma unroll
    for (int e = 0; e < 48; e++) lam[RT_LAM(e, lane)] = 0.0f;

    const int n_steps = (n_save - 1) * substeps;
    const float* tp = tape + (size_t)tile * n_steps * 4 * 3072 + lane * 4;
    float* tp2 = tape2 + (size_t)tile * n_steps * 4 * RT_TAPE2 + lane * 4;
    const float* tpz = ZT ? tapez + (size_t)tile * n_steps * 4 * RT_TAPEZ + lane * 4 : nullptr;

    // loss injection at save point n: λ += ∂loss/∂sol[:, n]; also the six raw sums of squares
    auto inject = [&](int n, bool add) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            f32x16 d;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const size_t o = ((size_t)min(col, n_col - 1) * n_save + n) * 96 + q * 32 + 8 * g + 4 * h;
                const f32x4v a = *reinterpret_cast<const f32x4v*>(sol + o);
                const f32x4v b = *reinterpret_cast<const f32x4v*>(truth + o);
#pragma unroll
                for (int e = 0; e < 4; e++) d[4 * g + e] = valid ? a[e] - b[e] : 0.0f;
            }
            const f32x16 dd = shift_down(d, h, 0.0f);
            f32x16 gg;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                gg[r] = (r == 0 && h == 0) ? 0.0f : (d[r] - dd[r]) * 32.0f;
                sums[q] += d[r] * d[r];
                sums[3 + q] += gg[r] * gg[r];
            }
            if (add) {
                const f32x16 gu_ = shift_up(gg, h, 0.0f);
#pragma unroll
                for (int r = 0; r < 16; r++)
                    lam[RT_LAM(q * 16 + r, lane)] += 2.0f * lw.w[q] * d[r] + 2.0f * lw.w[3 + q] * 32.0f * (gg[r] - gu_[r]);
            }
        }
    };
    inject(0, false);

    // taped layer-1 pre-activations of net n at (step, stage): registers G' < 25 of Z (padding registers untouched).  The record is the forward kernel's
    // ten layer-1 tiles as they left its accumulators: group (t, c), lane, element e = stacked quad Q = 4 t + e (rt16_q_net / rt16_q_quad), feature 4 qq + h + 2 c,
    // i.e. register G' = 2 qq + c of this lane.  Net n's twelve full quads are the whole tiles 3n .. 3n+2: six 16-byte loads, each one contiguous KiB per wave,
    // every element kept.  Its quad 12 (register 24) is element n of tile 9's first group: a 4-byte load.  No load has a destination register that nobody reads —
    // such registers are handed to the next instructions, which then have to wait for the load to land before they may write them (the earlier record, 13 quads
    // per net stacked back to back, put two nets into tiles 3 and 6: every net's request was waited for within a few instructions).  Every index is compile-time.
    auto load_z1 = [&](int step, int st, int n, f32x16 (&Z)[2]) {
        const float* srcz = tpz + ((size_t)step * 4 + st) * RT_TAPEZ;
#pragma unroll
        for (int t = 3 * n; t < 3 * n + 3; t++)
#pragma unroll
            for (int c = 0; c < 2; c++) {
                static_assert(rt16_q_slot(1, 0) == 12 && rt16_q_slot(2, 11) == 35 && rt16_q_slot(2, 12) == 38, "load_z1 addresses the record by this map");
                const f32x4v v = RT_TAPE_LOAD4(srcz + (2 * t + c) * 256);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int G = 2 * (rt16_q_quad(4 * t + e)) + c;
                    Z[G >> 4][G & 15] = v[e];
                }
            }
        Z[1][8] = __builtin_nontemporal_load(srcz + (rt16_q_slot(n, 12) >> 2) * 2 * 256 + (rt16_q_slot(n, 12) & 3));
    };

    // stage input (taped by the forward kernel)
    auto load_x = [&](int step, int st) {
        const float* src = tp + ((size_t)step * 4 + st) * 3072;
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f32x4v v = RT_TAPE_LOAD4(src + (q * 4 + g) * 256);
                X[q][4 * g] = v[0]; X[q][4 * g + 1] = v[1]; X[q][4 * g + 2] = v[2]; X[q][4 * g + 3] = v[3];
            }
    };

    for (int iv = n_save - 2; iv >= 0; iv--) {
        const float dt = (save_times[iv + 1] - save_times[iv]) / (float)substeps;
        inject(iv + 1, true);
        for (int s = substeps - 1; s >= 0; s--) {
            const int step = iv * substeps + s;
#pragma nounroll
            for (int st = 3; st >= 0; st--) {
                const float cwl = (st == 0 || st == 3) ? dt / 6.0f : dt / 3.0f;
                const float cwx = st == 3 ? 0.0f : (st == 2 ? dt : 0.5f * dt);
                RT_STAMP_BEGIN();
                f32x16 A1[2], D1[2];        // net n: act(z1), act'(z1) (then dZ1); register G' = 16 t + r <-> features 2G', 2G'+1
                f32x16 A1n[2], D1n[2];      // net n + 1, in flight under net n's W1^T products (ZT)
#pragma unroll
                for (int r = 9; r < 16; r++) { A1[1][r] = 0.0f; D1[1][r] = 0.0f; A1n[1][r] = 0.0f; D1n[1][r] = 0.0f; }
                load_x(step, st);
                // With the Z1 tape only the closure reads X, and `tape` is const __restrict__: LLVM sinks the twelve loads into rt_physics_vjp's closure branch, behind
                // the whole cotangent block, in two dependent batches — two exposed HBM round trips per stage.  Handing the tape pointer to an empty asm that may
                // write memory keeps them here (a bare memory clobber does not order a load through a noalias pointer); their wait stays at the closure's first use
                // of X, since the asm does not name the loaded registers.  (!ZT: layer 1 reads X, the loads are here already; the pin would only put a spill reload
                // behind them, and vmcnt, counting in order, would wait for all twelve with it.)
                if constexpr (ZT) asm volatile("" :: "v"(tp) : "memory");
                // (1) stage cotangent and the physics pullback: dO = cotangent of the NN fluxes, xb = physics part of x̄
                f32x16 dOk[3];
                {
                    f32x16 kb[3];
#pragma unroll
                    for (int q = 0; q < 3; q++)
#pragma unroll
                        for (int r = 0; r < 16; r++) kb[q][r] = cwl * lam[RT_LAM(q * 16 + r, lane)] + cwx * xb[q][r];
#ifdef COLNDE_STAMPS
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    RT_STAMP(8);                    // diagnostic build only: the stage-input request, kb and what is left of the loads' latency behind kb (the shipped build waits later, in the closure)
#endif
                    rt_physics_vjp(m, X, kb, h, xb);       // kb now holds dO
#pragma unroll
                    for (int q = 0; q < 3; q++) dOk[q] = kb[q];
                }
                RT_STAMP(0);
                float* dst = tp2 + ((size_t)step * 4 + st) * RT_TAPE2;
                float carry[2] = {0.0f, 0.0f};
                // diagnostic build only: stamps at the first use of net n + 1's record inside net n's W1^T products — the work since stamp 5, then what is left of the
                // latency of the record's loads behind it (dW2 and the W2^T chains, before stamp 5, cover it too)
                auto z1_stamp = [&](int n) {
#ifdef COLNDE_STAMPS
                    RT_STAMP(9 + 2 * n);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    RT_STAMP(10 + 2 * n);
#endif
                };
                // the nets are handled one after the other so that only one net's hidden state is live at a time
#pragma unroll
                for (int n = 0; n < 3; n++) {
                    const f32x16 dOn = dOk[n];
                    // (2) hidden layer 1 of net n: activation A1 (feeds layer 2 and the dW2 products) and derivative D1 (feeds dZ1),
                    //     evaluated once, together.  With the Z1 tape (ZT) nets 1 and 2 arrive already activated: their taped
                    //     pre-activations were fetched and activated in the shadow of the previous net's W1^T products (6).
                    constexpr bool EARLY3 = ZT;       // net 0 with the Z1 tape does two pieces of (3) here, under its tape's round trip
                    f32x16 TA3, da3;
                    if (ZT) {
                        if (n == 0) {
                            load_z1(step, st, 0, A1);      // (requested BEFORE the physics pullback instead: 55.9 -> 57.0 ms, round 5)
                            // Net 0's record is requested here and nothing above can cover it.  What follows needs
                            // dO only — layer 3's transposition and bias sum and the sixteen products of W3^T dO — so it runs first, and the wait for the
                            // tape moves from the request to the activation pairs.  Three things hold the order: the pointer handed to the asm keeps the loads
                            // ahead of the chain (as for the stage input), the scheduling barrier keeps the chain ahead of the pairs, and the second asm ties
                            // the pairs' inputs and the chain's result together, because both are pure arithmetic and instruction selection orders them freely
                            // otherwise (it put the pairs, and the wait with them, behind the chain's first product).
                            asm volatile("" :: "v"(tpz) : "memory");
                            TA3 = rt_transpose(tb, dOn, wbase, rbase);
                            b3acc[n] += rt_sum16(TA3);
                            const int base = b3T + n * 31 * RT_LD3;
                            da3 = rt_chain<16, 8>(wl, (f32x16)(0.0f), [=](int k) { return base + RHO0(k) * RT_LD3; },
                                                  [&](int k) { return dOn[k]; });
                            __builtin_amdgcn_sched_barrier(0);
#ifdef COLNDE_STAMPS
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                            RT_STAMP(7);            // diagnostic build only: what is left of the latency of net 0's Z1 loads behind that work
#endif
                            asm volatile("" : "+v"(A1[0][0]), "+v"(A1[0][1]), "+v"(A1[0][2]), "+v"(A1[0][3]), "+v"(A1[0][4]), "+v"(A1[0][5]), "+v"(A1[0][6]), "+v"(A1[0][7]),
                                              "+v"(A1[0][8]), "+v"(A1[0][9]), "+v"(A1[0][10]), "+v"(A1[0][11]), "+v"(A1[0][12]), "+v"(A1[0][13]), "+v"(A1[0][14]), "+v"(A1[0][15]),
                                              "+v"(A1[1][0]), "+v"(A1[1][1]), "+v"(A1[1][2]), "+v"(A1[1][3]), "+v"(A1[1][4]), "+v"(A1[1][5]), "+v"(A1[1][6]), "+v"(A1[1][7]),
                                              "+v"(A1[1][8]), "+a"(da3));
#pragma unroll
                            for (int G = 0; G < 24; G += 4) rt_act_pair4_at<ACT>(A1, D1, G);
                            rt_act_pair_at<ACT>(A1, D1, 24);
                        }
                    } else {
#pragma unroll
                        for (int t = 0; t < 2; t++) {
                            f32x16 acc;
#pragma unroll
                            for (int r = 0; r < 16; r++) acc[r] = (t * 16 + r < 25) ? wl[RT_B1C + n * 50 + 2 * (t * 16 + r) + h] : 0.0f;
                            const int base = a1n[t] + n * 50 * RT_LD1;
                            acc = rt_chain<48, RT_ADJ_CH>(wl, acc, [=](int k) { return base + (k >> 4) * 32 + RHO0(k & 15); },
                                                          [&](int k) { return X[k >> 4][k & 15]; });
#pragma unroll
                            for (int r = 0; r < 16; r++) {
                                float av = 0.0f, dv = 0.0f;
                                if (t * 16 + r < 25) rt_act_pair<ACT>(acc[r], av, dv);
                                A1[t][r] = av;
                                D1[t][r] = dv;
                            }
                        }
                    }
                    RT_STAMP(1);
                    f32x16 Z2;
                    {
                        f32x16 acc;
#pragma unroll
                        for (int r = 0; r < 16; r++) acc[r] = r < 10 ? wl[RT_B2C + n * 20 + 2 * r + h] : 0.0f;
                        const int base2 = a2b + n * 20 * RT_LD2;
                        Z2 = rt_chain<25, 5>(wl, acc, [=](int k) { return base2 + 2 * k; },
                                             [&](int k) { return A1[k >> 4][k & 15]; });
                    }
                    RT_STAMP(2);
                    // (3) layer 3: weight/bias gradient, then dZ2 = (W3^T dO) .* act'(Z2)
                    //     (evaluating the layer-2 activation pairs inside the W3^T chain instead was measured slower: 94.8 vs 89.7 ms)
                    {
                        f32x16 TA;
                        if (EARLY3 && n == 0) TA = TA3;
                        else { TA = rt_transpose(tb, dOn, wbase, rbase); b3acc[n] += rt_sum16(TA); }
                        f32x16 A2;
#pragma unroll
                        for (int r = 0; r < 16; r += 4) {
                            f32x2v a0 = {0.0f, 0.0f}, d0 = {0.0f, 0.0f}, a1 = {0.0f, 0.0f}, d1 = {0.0f, 0.0f};
                            if (r < 8) rt_act_pair4<ACT>((f32x2v){Z2[r], Z2[r + 1]}, (f32x2v){Z2[r + 2], Z2[r + 3]}, a0, d0, a1, d1);
                            else if (r == 8) rt_act_pair2<ACT>((f32x2v){Z2[8], Z2[9]}, a0, d0);
                            A2[r] = a0.x; A2[r + 1] = a0.y; A2[r + 2] = a1.x; A2[r + 3] = a1.y;
                            Z2[r] = d0.x; Z2[r + 1] = d0.y; Z2[r + 2] = d1.x; Z2[r + 3] = d1.y;     // Z2 now holds act'(z2)
                        }
                        const f32x16 TB = rt_transpose(tb, A2, wbase, rbase);
                        gW3[n] = rt_outer(gW3[n], TA, TB);
                    }
                    {
                        const int base = b3T + n * 31 * RT_LD3;
                        f32x16 da;
                        if (EARLY3 && n == 0) da = da3;
                        else da = rt_chain<16, 8>(wl, (f32x16)(0.0f), [=](int k) { return base + RHO0(k) * RT_LD3; },
                                                  [&](int k) { return dOn[k]; });
#pragma unroll
                        for (int r = 0; r < 16; r++) Z2[r] = da[r] * Z2[r];
                    }
                    RT_STAMP(3);
                    // fetch net n + 1's taped pre-activations now: dW2, W2^T and the first W1^T chunk cover the HBM latency
                    if (ZT && n < 2) load_z1(step, st, n + 1, A1n);
                    // (SPLIT) the l-plane operands of this net's W1^T products, from L2: the first k-block's three issued before the dW2 outer products (one phase earlier
                    // than needed: 56.5 -> 55.6 ms), the others one k-block ahead inside the products (all nine here: 36 live registers instead of 12-24, scratch 500 -> 536 B,
                    // adjoint 55.6 -> 56.2 ms)
                    u32x4 Lr[9];
                    const u32x4* lg = nullptr;
                    if constexpr (SPLIT) {
                        // (an opaque lane index per net: left loop-invariant, the 27 loads are hoisted out of the time loop and their 108 registers spilled)
                        int lz = lane;
                        asm volatile("" : "+v"(lz));
                        lg = reinterpret_cast<const u32x4*>(wimg + RT_ASIMG_OFF + RT_ASIMG_L) + n * 9 * 64 + lz;
#pragma unroll
                        for (int u = 0; u < 3; u++) Lr[u] = lg[u * 64];
                    }
                    // (4) layer 2: weight/bias gradient
                    {
                        const f32x16 TA = rt_transpose(tb, Z2, wbase, rbase);
                        b2acc[n] += rt_sum16(TA);
#pragma unroll
                        for (int t = 0; t < 2; t++) {
                            const f32x16 TB = rt_transpose(tb, A1[t], wbase, rbase);
                            gW2[n][t] = rt_outer(gW2[n][t], TA, TB);
                        }
                    }
                    RT_STAMP(4);
                    // (5) dZ1 = (W2^T dZ2) .* act'(Z1), in place; taped for the streaming dW1 kernel
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const int base = b2T[t] + n * 20 * RT_LD2;
                        const f32x16 da = rt_chain<10, 10>(wl, (f32x16)(0.0f), [=](int k) { return base + 2 * k * RT_LD2; },
                                                           [&](int k) { return Z2[k]; });
#pragma unroll
                        for (int r = 0; r < 16; r++) D1[t][r] = da[r] * D1[t][r];     // dZ1 in place of act'(z1)
                    }
                    auto store_delta = [&] {
                    // delta tape: register g of net n is stacked register G = 25 n + g, element G & 3 of 16-byte group G >> 2.  Whole groups
                    // leave with one store; the groups that straddle a net boundary (6: G 24 | 25..27, 12: G 48, 49 | 50, 51) wait in
                    // `carry` for the next net's first registers, so a stage writes 19 16-byte stores and no scattered dwords
#pragma unroll
                    for (int g = 0; g < 25; g++) {
                        const int G = 25 * n + g;
                        if ((G & 3) == 0 && g + 3 < 25) {
                            const f32x4v v = {D1[g >> 4][g & 15], D1[(g + 1) >> 4][(g + 1) & 15], D1[(g + 2) >> 4][(g + 2) & 15],
                                              D1[(g + 3) >> 4][(g + 3) & 15]};
                            RT_NT_STORE4(dst + (G >> 2) * 256, v);
                        }
                    }
                    if (n == 0) carry[0] = D1[1][8];                                                   // G 24
                    if (n == 1) {
                        RT_NT_STORE4(dst + 6 * 256, ((f32x4v){carry[0], D1[0][0], D1[0][1], D1[0][2]}));   // G 24 | 25, 26, 27
                        carry[0] = D1[1][7];                                                           // G 48
                        carry[1] = D1[1][8];                                                           // G 49
                    }
                    if (n == 2) {
                        RT_NT_STORE4(dst + 12 * 256, ((f32x4v){carry[0], carry[1], D1[0][0], D1[0][1]})); // G 48, 49 | 50, 51
                        RT_NT_STORE4(dst + 18 * 256, ((f32x4v){D1[1][6], D1[1][7], D1[1][8], 0.0f}));     // G 72, 73, 74, pad
                    }
                    };
                    if constexpr (!SPLIT) store_delta();       // (SPLIT: behind the W1^T products — vmcnt is in order, and the l-plane loads must not queue behind these stores)
                    RT_STAMP(5);
                    // (6) x̄ += W1_n^T dZ1_n
                    // Net n + 1's activation pairs below are pure arithmetic on the record's registers: left alone, the first instruction of a pair (a v_med3_f32) is
                    // lifted out of the products, past the W2^T chains and into dW2 (fp32 mish: 10 MFMAs behind the request), and the wait for the record comes with it.
                    // Nothing crosses this barrier, so the first wait stays behind dW2 and the W2^T chains.  (Tying the 25 registers to an asm at the first pair, as for
                    // net 0, makes the allocator copy them out of the loads' tuples at the request: a wait one instruction behind it.)
                    if (ZT && n < 2) __builtin_amdgcn_sched_barrier(0);
                    if constexpr (SPLIT) {
                        const u32x4* hm = reinterpret_cast<const u32x4*>(rt_smem) + lane;
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            if (c < 2) {
#pragma unroll
                                for (int u = 0; u < 3; u++) Lr[3 * (c + 1) + u] = lg[(3 * (c + 1) + u) * 64];
                            }
                            float d8[8];
#pragma unroll
                            for (int u = 0; u < 8; u++) d8[u] = D1[(8 * c + u) >> 4][(8 * c + u) & 15];
                            const Bf3 Bc = bf3_split8(d8);
#pragma unroll
                            for (int q = 0; q < 3; q++) {
                                const int G = n * 9 + c * 3 + q, slot = c * 3 + q;
                                const u32x4 Ah = hm[(G * 2) * 64], Am = hm[(G * 2 + 1) * 64];
                                // net n + 1's 25 activation pairs, spread over slots 2 .. 8 (as in the fp32 chain: not under the first chunks)
                                if (ZT && n < 2 && slot >= 2) {
                                    if (slot == 2) z1_stamp(n);
                                    if (slot < 8) rt_act_pair4_at<ACT>(A1n, D1n, 4 * (slot - 2));
                                    else rt_act_pair_at<ACT>(A1n, D1n, 24);
                                }
                                xb[q] = mfma_bf(Am, Bc.m, xb[q]);
                                xb[q] = mfma_bf(Ah, Bc.l, xb[q]);
                                xb[q] = mfma_bf(Am, Bc.h, xb[q]);
                                xb[q] = mfma_bf(Ah, Bc.m, xb[q]);
                                xb[q] = mfma_bf(Ah, Bc.h, xb[q]);
                                xb[q] = mfma_bf(Lr[slot], Bc.h, xb[q]);          // the operand from L2 last
                                RT_SCHED_FENCE();
                            }
                        }
                        // register 24 (features 48, 49): one fp32 k-step per state tile
                        const float* left = rt_smem + RT_ASIMG_LEFT + (n * 2 + h) * 96 + i_;
#pragma unroll
                        for (int q = 0; q < 3; q++) xb[q] = mfma32(left[q * 32], D1[1][8], xb[q]);
                        store_delta();
                    } else
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        const int base = b1T + q * 32 + n * 50 * RT_LD1;
                        xb[q] = rt_chain_fill<25, 5>(wl, xb[q], [=](int g) { return base + 2 * g * RT_LD1; },
                                                     [&](int g) { return D1[g >> 4][g & 15]; },
                                                     [&](int c) {
                                                         // net n + 1's 25 activation pairs, spread over the 15 chunks
                                                         if (ZT && n < 2 && (q > 0 || c > 0)) {
                                                             if (q * 5 + c == 2) z1_stamp(n);
#pragma unroll
                                                             for (int G = 0; G < 24; G += 4)
                                                                 if ((G >> 2) * 2 + 2 == q * 5 + c)
                                                                     rt_act_pair4_at<ACT>(A1n, D1n, G);
                                                             if (q * 5 + c == 14) rt_act_pair_at<ACT>(A1n, D1n, 24);
                                                         }
                                                     });
                    }
                    if (ZT && n < 2) {
#pragma unroll
                        for (int t = 0; t < 2; t++) { A1[t] = A1n[t]; D1[t] = D1n[t]; }
                    }
                }
                RT_STAMP(6);
#pragma unroll
                for (int q = 0; q < 3; q++) xbs[q] += xb[q];
            }
            // λ_n = λ_{n+1} + x̄_1 + x̄_2 + x̄_3 + x̄_4
#pragma unroll
            for (int q = 0; q < 3; q++) {
#pragma unroll
                for (int r = 0; r < 16; r++) lam[RT_LAM(q * 16 + r, lane)] += xbs[q][r];
                xbs[q] = (f32x16)(0.0f);
            }
        }
    }

#ifndef COLNDE_STAMPS_FWD
    RT_STAMP_FLUSH();
#endif
    // ---- flush this wave's partial gradients (row `tile` of the slab; dW1/db1 come from rt_dw1_kernel) ----
    float* out = slab + (size_t)tile * (m.n_params + 8);
    const int r_j = (j & 3) + 4 * (j >> 3), h_j = (j >> 2) & 1;     // this lane as a column index n' of a D tile
#pragma unroll
    for (int n = 0; n < 3; n++) {
        // dW3_n[out = face-1][in = f2]: D[m = face rho(r,h)][n' = a2 row j]
        if (r_j < 10) {
            const int f2 = 2 * r_j + h_j;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int face = RHO0(r) + 4 * h;
                if (face >= 1) out[n * m.net_size + m.w_off[2] + f2 * 31 + face - 1] = gW3[n][r];
            }
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
            // dW2_n[out = f2 = 2r+h][in = f1]: D[m = z2 row rho(r,h)][n' = row j of net n's layer-1 tile t]
            const int Gp = t * 16 + r_j;
            if (Gp < 25) {
                const int f1 = 2 * Gp + h_j;
#pragma unroll
                for (int r = 0; r < 10; r++) out[n * m.net_size + m.w_off[1] + f1 * 20 + 2 * r + h] = gW2[n][t][r];
            }
        }
        // biases: lanes (i, 0) and (i, 1) hold the even / odd column halves of row i_
        const float s2 = b2acc[n] + swap32(b2acc[n], h), s3 = b3acc[n] + swap32(b3acc[n], h);
        if (h == 0) {
            if (r_i < 10) out[n * m.net_size + m.b_off[1] + 2 * r_i + h_i] = s2;
            if (i_ >= 1) out[n * m.net_size + m.b_off[2] + i_ - 1] = s3;
        }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) {
        float v = sums[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) out[m.n_params + q] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// dW1 / db1: a streaming GEMM over the two tapes, contracted over (column, step, stage)
//   dW1[n*50+f][c] = sum dZ1[(n,f)][col] * X[c][col]
// Each wave walks items (tile, step, stage) and accumulates all 15 (layer-1 tile, state tile) products in registers; its
// partial result is one slab row.  An item's two tape records are register images of the kernels that wrote them
// (lane = column, registers = rows); the products contract over columns, so their MFMA operands are the transposed tiles.
// The transposition costs nothing here: the record goes HBM -> LDS by LDS-DMA (global_load_lds, 16 bytes per lane, no
// registers), and because the DMA's SOURCE address is per lane while its destination is lane-linear, each 1-KB
// wave-instruction gathers the 16-byte pieces (4 consecutive rows of one column) of 8 columns so that they land as a
// column-major tile [col][row] — the operand of k-step s, lane (row m, kh), is then the conflict-free read
// tile[(2 s + kh) * 32 + m].  The unit of the pipeline is a QUARTER item (8 columns of all 8 tiles: 8 DMA instructions,
// 8 KB, 60 MFMAs): a ring of four quarter buffers per wave, DMA issued three quarters ahead (counted vmcnt), operands
// read one quarter ahead into the other of two register sets — so neither the HBM latency nor the LDS reads are exposed.
// ------------------------------------------------------------------------------------------------
#define RT_DW1_LDS (4 * 2048)      // floats per wave: ring of four quarter-item buffers [8 tiles][8 cols][32 rows]
__global__ void __launch_bounds__(256)
rt_dw1_kernel(DevModel m, const float* __restrict__ tape, const float* __restrict__ tape2, long n_items,
              float* __restrict__ slab_rows) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    float* buf = rt_smem + wave * RT_DW1_LDS;
    const long gw = (long)blockIdx.x * RT_WAVES + wave, GW = (long)gridDim.x * RT_WAVES;
    f32x16 gW1[5][3];
#pragma unroll
    for (int mt = 0; mt < 5; mt++)
#pragma unroll
        for (int q = 0; q < 3; q++) gW1[mt][q] = (f32x16)(0.0f);
    float b1acc[5] = {0, 0, 0, 0, 0};
    const int NQ = gw < n_items ? 4 * (int)((n_items - gw + GW - 1) / GW) : 0;       // this wave's quarters
    // DMA piece i of tile T: lane L fetches rows 4 k .. 4 k + 3 (k = L & 7) of column 8 i + (L >> 3), which the record holds in
    // group 4 T + (k >> 1), lane (k & 1) * 32 + column
    const int soff = ((lane >> 1) & 3) * 256 + ((lane & 1) * 32 + (lane >> 3)) * 4;
    // quarter Q of this wave into ring slot `ring`; past the end the last quarter is fetched again (into a slot nobody reads), so that
    // the counted waits below always see the same number of DMAs in flight
    auto issue = [&](int Q, int ring) {
        const int Qc = Q < NQ ? Q : NQ - 1;
        const size_t item = (size_t)(gw + (long)(Qc >> 2) * GW);
        const float* sx = tape + item * 3072 + soff + (Qc & 3) * 32;
        const float* sz = tape2 + item * RT_TAPE2 + soff + (Qc & 3) * 32;
#pragma unroll
        for (int T = 0; T < 3; T++) __builtin_amdgcn_global_load_lds(sx + T * 1024, buf + ring * 2048 + T * 256, 16, 0, RT_DMA_AUX);
#pragma unroll
        for (int T = 0; T < 5; T++) __builtin_amdgcn_global_load_lds(sz + T * 1024, buf + ring * 2048 + (3 + T) * 256, 16, 0, RT_DMA_AUX);
    };
    const float* rd = buf + h * 32 + j;
    float op[2][8][4];                         // operand sets: [set][tile][k-step]: tile[(2 s + kh) * 32 + m]
    auto read_set = [&](int set, int ring) {
#pragma unroll
        for (int T = 0; T < 8; T++)
#pragma unroll
            for (int s = 0; s < 4; s++) op[set][T][s] = rd[ring * 2048 + T * 256 + 64 * s];
    };
    if (NQ > 0) {
        issue(0, 0);
        issue(1, 1);
        issue(2, 2);
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        read_set(0, 0);
    }
    for (int Qb = 0; Qb < NQ; Qb += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int cur = u & 1;
            // first delta tile of this quarter; behind it the DMA three quarters ahead and the operand reads one quarter ahead
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int q = 0; q < 3; q++) gW1[0][q] = mfma32(op[cur][3][s], op[cur][q][s], gW1[0][q]);
            b1acc[0] += (op[cur][3][0] + op[cur][3][1]) + (op[cur][3][2] + op[cur][3][3]);
            __builtin_amdgcn_sched_barrier(0);
            issue(Qb + u + 3, (u + 3) & 3);
            asm volatile("s_waitcnt vmcnt(16)" ::: "memory");       // quarter Qb + u + 1 has landed (two younger ones in flight)
            read_set(cur ^ 1, (u + 1) & 3);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 1; mt < 5; mt++) {
#pragma unroll
                for (int s = 0; s < 4; s++)
#pragma unroll
                    for (int q = 0; q < 3; q++) gW1[mt][q] = mfma32(op[cur][3 + mt][s], op[cur][q][s], gW1[mt][q]);
                b1acc[mt] += (op[cur][3 + mt][0] + op[cur][3 + mt][1]) + (op[cur][3 + mt][2] + op[cur][3 + mt][3]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    float* out = slab_rows + (size_t)gw * (m.n_params + 8);
    // D[m = layer-1 row rho(r,h) of tile mt][n' = state feature 32 q + j]
#pragma unroll
    for (int mt = 0; mt < 5; mt++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int G = mt * 16 + r;
            if (G < 75) {
                const int n = G / 25, f = 2 * (G % 25) + h;
#pragma unroll
                for (int q = 0; q < 3; q++) out[n * m.net_size + m.w_off[0] + (q * 32 + j) * 50 + f] = gW1[mt][q][r];
            }
        }
        const float s1 = b1acc[mt] + swap32(b1acc[mt], h);
        const int r_j = (j & 3) + 4 * (j >> 3), h_j = (j >> 2) & 1;
        const int G = mt * 16 + r_j;
        if (h == 0 && G < 75) out[(G / 25) * m.net_size + m.b_off[0] + 2 * (G % 25) + h_j] = s1;
    }
}

// ------------------------------------------------------------------------------------------------
// dW1 / db1 on the bf16 matrix pipe with EXACT three-way operand splitting (COLNDE_MATRIX_BF16X3_EXACT, the default)
//
// A float has 24 significant bits = three bf16 (8 bits each): x = x_h + x_m + x_l exactly, by truncation (x_h = the top half of the
// word, r = x - x_h is exact, x_m = the top half of r, x_l = r - x_m has at most 8 significant bits).  A product a b is then the nine
// products of the parts, each EXACT in fp32 (8 x 8 bits), accumulated in fp32 by v_mfma_f32_32x32x16_bf16; the six of them down to
// 2^-16 are kept (hh, hm, mh, hl, lh, mm), the three dropped ones are below 2^-23 |a b| together — the size of ONE fp32 rounding of
// the product, which the fp32 MFMA chain commits at every accumulation anyway.  Six 32-cycle instructions cover 16 k-steps that cost
// eight 64-cycle v_mfma_f32_32x32x2_f32: 192 cycles instead of 512.
//
// Same tapes, same LDS-DMA gather and the same [col][row] tiles as rt_dw1_kernel.  The unit is HALF an item (16 columns = one
// k-block): lane (row j, kh) contracts k = 8 kh + c with column c of quarter 2 H + kh, i.e. it reads eight floats of ONE quarter
// buffer (conflict-free, stride 32) per tile, splits them in registers (5.5 vector operations per value, issued under the MFMAs) and
// feeds 90 MFMAs.  Ring of four quarter buffers as before: the two quarters of half H + 2 are fetched into the slots of half H as soon
// as its operands are in registers.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
rt_dw1_split_kernel(DevModel m, const float* __restrict__ tape, const float* __restrict__ tape2, long n_items,
                    float* __restrict__ slab_rows) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    float* buf = rt_smem + wave * RT_DW1_LDS;
    const long gw = (long)blockIdx.x * RT_WAVES + wave, GW = (long)gridDim.x * RT_WAVES;
    f32x16 gW1[5][3];
#pragma unroll
    for (int mt = 0; mt < 5; mt++)
#pragma unroll
        for (int q = 0; q < 3; q++) gW1[mt][q] = (f32x16)(0.0f);
    float b1acc[5] = {0, 0, 0, 0, 0};
    const int NQ = gw < n_items ? 4 * (int)((n_items - gw + GW - 1) / GW) : 0;       // this wave's quarters
    const int soff = ((lane >> 1) & 3) * 256 + ((lane & 1) * 32 + (lane >> 3)) * 4;  // the gather of rt_dw1_kernel
    auto issue = [&](int Q, int ring) {
        const int Qc = Q < NQ ? Q : NQ - 1;
        const size_t item = (size_t)(gw + (long)(Qc >> 2) * GW);
        const float* sx = tape + item * 3072 + soff + (Qc & 3) * 32;
        const float* sz = tape2 + item * RT_TAPE2 + soff + (Qc & 3) * 32;
#pragma unroll
        for (int T = 0; T < 3; T++) __builtin_amdgcn_global_load_lds(sx + T * 1024, buf + ring * 2048 + T * 256, 16, 0, RT_DMA_AUX);
#pragma unroll
        for (int T = 0; T < 5; T++) __builtin_amdgcn_global_load_lds(sz + T * 1024, buf + ring * 2048 + (3 + T) * 256, 16, 0, RT_DMA_AUX);
    };
    const float* rd = buf + h * 2048 + j;        // lane half kh reads the quarter buffer (slot0 + kh)
    float raw[2][8][8];                          // [set][tile][column of the quarter]
    auto read_half = [&](int set, int slot0) {
#pragma unroll
        for (int T = 0; T < 8; T++)
#pragma unroll
            for (int c = 0; c < 8; c++) raw[set][T][c] = rd[slot0 * 2048 + T * 256 + c * 32];
    };
    // Pipeline: while half H is multiplied, half H + 1 sits in registers (read at the top of H) and halves H + 2, H + 3 are in flight —
    // a half's two slots are refilled as soon as its operands have been read (the whole ring is in flight during the MFMAs).
    if (NQ > 0) {
        issue(0, 0);
        issue(1, 1);
        issue(2, 2);
        issue(3, 3);
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        read_half(0, 0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        issue(4, 0);
        issue(5, 1);
    }
    for (int Qb = 0; Qb < NQ; Qb += 4) {
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int cur = u;
            asm volatile("s_waitcnt vmcnt(16)" ::: "memory");       // half H + 1 has landed (H + 2 may still be in flight)
            read_half(cur ^ 1, 2 * (u ^ 1));
            __builtin_amdgcn_sched_barrier(0);
            Bf3 X[3];
#pragma unroll
            for (int q = 0; q < 3; q++) X[q] = bf3_split8(raw[cur][q]);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // ... and is in registers: its slots take half H + 3
            issue(Qb + 2 * u + 6, 2 * (u ^ 1));
            issue(Qb + 2 * u + 7, 2 * (u ^ 1) + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 0; mt < 5; mt++) {
                const Bf3 Z = bf3_split8(raw[cur][3 + mt]);
#pragma unroll
                for (int q = 0; q < 3; q++) gW1[mt][q] = mfma_bf3(Z, X[q], gW1[mt][q]);
                const float* z = raw[cur][3 + mt];
                b1acc[mt] += ((z[0] + z[1]) + (z[2] + z[3])) + ((z[4] + z[5]) + (z[6] + z[7]));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    float* out = slab_rows + (size_t)gw * (m.n_params + 8);
#pragma unroll
    for (int mt = 0; mt < 5; mt++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int G = mt * 16 + r;
            if (G < 75) {
                const int n = G / 25, f = 2 * (G % 25) + h;
#pragma unroll
                for (int q = 0; q < 3; q++) out[n * m.net_size + m.w_off[0] + (q * 32 + j) * 50 + f] = gW1[mt][q][r];
            }
        }
        const float s1 = b1acc[mt] + swap32(b1acc[mt], h);
        const int r_j = (j & 3) + 4 * (j >> 3), h_j = (j >> 2) & 1;
        const int G = mt * 16 + r_j;
        if (h == 0 && G < 75) out[(G / 25) * m.net_size + m.b_off[0] + 2 * (G % 25) + h_j] = s1;
    }
}

// ------------------------------------------------------------------------------------------------
// forward solve on 16-column wave tiles (v_mfma_f32_16x16x4_f32), TWO wavefronts per SIMD
//
// Same idea as rt_forward_kernel with half the per-wave state: lane (j = lane & 15, g = lane >> 4) holds rows 4g..4g+3 of
// a 16-row x 16-column tile in a float4; the B operand of k-step r is element r (K quad = rows r, 4+r, 8+r, 12+r).  A
// 32-level variable is two tiles.  ~150 registers per wave, so eight waves (two per SIMD) share one LDS weight image and
// one wave's activations / physics / RK update hide under the other's MFMA chains.  The stage tape is written in the
// 32-column register-image format the adjoint and dW1 kernels read (two 16-column waves make one 32-column tile).
//
// Row placement: layer-1 outputs stacked into 10 tiles; quad Q = 4 t + r (rows 16t + 4g + r) carries features 4 rt16_q_quad(Q) + g
// of net rt16_q_net(Q) (13 quads = 52 rows per net, 2 of them padding; a net's twelve full quads are three whole tiles, the three
// quads 12 share tile 9 — see rt16_q_slot); layer-2 outputs: quad Q2 = 4u + r carries features
// 4 Q2 + g (Q2 < 5); layer-3 output row = face index.
// ------------------------------------------------------------------------------------------------
// Z1 tape of the 16-column forward kernels: layer-1 tile tt leaves as it sits in the accumulators, one 16-byte store per lane (a wave instruction writes four
// complete 256-byte runs, no address or mask arithmetic).  Record of one (32-column tile, step, stage): [t = 0..9][c = 0..1][64 lanes][4]; group (t, c), lane
// j + 16 half + 32 h, element e = the pre-activation of stacked quad Q = 4 t + e (net n = rt16_q_net(Q), qq = rt16_q_quad(Q)), feature 4 qq + g with g = h + 2 c,
// column j + 16 half: A1[t] of forward lane (j, g).  Groups (3n .. 3n+2, c) are net n's quads 0 .. 11 and nothing else; group (9, 0) holds the three nets' quad 12
// (features 48, 49) in elements 0, 1, 2.  The adjoint's loads do the renaming into its per-net registers (load_z1).  Slot Q = 39 and the qq = 12, g >= 2 slots (all of
// group (9, 1)) hold what the padding rows produce (finite, never read).  (The earlier record in the adjoint's per-net register-image format took 39 dword stores per lane and stage, each wave
// store filling 8 of every 16 bytes; assembling that format's 16-byte groups with v_permlane32_swap was measured slower still: forward 28.0 -> 31.7 ms, round 5.)
template <int ACT, bool SPLIT = false>
__global__ void __launch_bounds__(512)
rt16_forward_kernel(DevModel m, const float* __restrict__ wimg, const float* __restrict__ x0, const float* __restrict__ bcs,
                    const float* __restrict__ save_times, int n_save, int substeps, float* __restrict__ sol,
                    float* __restrict__ tape, float* __restrict__ tapez, int n_col) {
    float* wl = rt_smem;
    const float* bl = wl;                                 // biases: bl[RT_B1C ...]
    const u32x4* simg = reinterpret_cast<const u32x4*>(rt_smem);
    if constexpr (SPLIT) {
        // LDS: the bf16 operand image (RT_SIMG_WORDS words, behind the fp32 image in the same allocation) and the fp32 bias tail
        const unsigned* src = reinterpret_cast<const unsigned*>(wimg + RT_SIMG_OFF);
        unsigned* dst = reinterpret_cast<unsigned*>(rt_smem);
        for (int e = threadIdx.x; e < RT_SIMG_WORDS / 4; e += blockDim.x)
            reinterpret_cast<u32x4*>(dst)[e] = reinterpret_cast<const u32x4*>(src)[e];
        for (int e = threadIdx.x; e < RT_IMG_FLOATS - RT_B1C; e += blockDim.x) wl[RT_SIMG_WORDS + e] = wimg[RT_B1C + e];
        bl = wl + RT_SIMG_WORDS - RT_B1C;
    } else {
        for (int e = threadIdx.x; e < RT_IMG_FLOATS; e += blockDim.x) wl[e] = wimg[e];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int wt = blockIdx.x * (blockDim.x >> 6) + wave; // 16-column tile (1..RT16_WAVES wavefronts per workgroup)
    const int tile32 = wt >> 1, half = wt & 1;
    if (tile32 * 32 >= n_col) return;                     // (both halves of a live 32-column tile run: the tape must be whole)
    const int col = wt * 16 + j;
    const bool valid = col < n_col;
    const int colc = min(col, n_col - 1);
    // A-operand bases (this lane as output row i = 4 g_i + r_i of a 16-row tile; k index = g)
    const int i_ = lane & 15, g_i = i_ >> 2, r_i = i_ & 3;
    int a1b[10];
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const int Q = 4 * t + r_i, f = 4 * rt16_q_quad(Q) + g_i;
        const int row = (Q < 39 && f < 50) ? rt16_q_net(Q) * 50 + f : 0;       // padding rows read a valid row; never consumed
        a1b[t] = RT_W1C + row * RT_LD1 + 4 * g;
    }
    int a2b[2], a2l[2], a3b[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int Q2 = 4 * u + r_i;
        const int row2 = Q2 < 5 ? 4 * Q2 + g_i : 0;
        a2b[u] = RT_W2C + row2 * RT_LD2 + g;
        a2l[u] = RT_W2C + row2 * RT_LD2 + (g < 2 ? 48 + g : 50);           // last quad of a net: features 48, 49, then the zero column
        a3b[u] = RT_W3C + (16 * u + i_ - 1) * RT_LD3 + g;
    }
    RtBC bc;
    float bc5;
    {
        const float* bp = bcs + (size_t)colc * 6;
        bc.b[0] = bp[0]; bc.t[0] = bp[1]; bc.b[1] = bp[2]; bc.t[1] = bp[3]; bc.b[2] = bp[4]; bc5 = bp[5];
        bc.t[2] = bc5;
    }
    V16 Xn[3];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int tau = 0; tau < 2; tau++) {
            const f32x4v v = *reinterpret_cast<const f32x4v*>(x0 + (size_t)colc * 96 + q * 32 + 16 * tau + 4 * g);
            Xn[q].t[tau] = v;
            if (sol && valid) *reinterpret_cast<f32x4v*>(sol + ((size_t)col * n_save) * 96 + q * 32 + 16 * tau + 4 * g) = v;
        }
    const int n_steps = (n_save - 1) * substeps;
    RT_STAMP_DECL;
#ifdef COLNDE_STAMPS_FWD
    const unsigned long long rs_k0 = __builtin_amdgcn_s_memtime(), rs_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    // 32-column register image: group (q*4 + 2 tau + (g>>1)), lane32 = j + 16 half + 32 (g & 1)
    float* tp = tape ? tape + (size_t)tile32 * n_steps * 4 * 3072 + ((g >> 1) * 64 + j + 16 * half + 32 * (g & 1)) * 4 : nullptr;
    // layer-1 pre-activations, taped as whole accumulator tiles: tile t is group 2 t + (g >> 1), lane32 = j + 16 half + 32 (g & 1) (as the stage tape above)
    float* tz = tapez ? tapez + (size_t)tile32 * n_steps * 4 * RT_TAPEZ + ((g >> 1) * 64 + j + 16 * half + 32 * (g & 1)) * 4 : nullptr;
    const float Nz = 32.0f;
    struct { float cU, sU, cV, sV, cB, sB, kE, oE, cE, nA, nB, f0, f1, f2; } pc;
    {
        const float L2E = 1.4426950408889634f;
        pc.cU = m.sig_u * Nz; pc.sU = m.sig_u * m.eps; pc.cV = m.sig_v * Nz; pc.sV = m.sig_v * m.eps; pc.cB = m.B * Nz; pc.sB = m.B * m.eps;
        pc.kE = 2.0f * m.inv_dRi * L2E; pc.oE = -2.0f * m.Ric * m.inv_dRi * L2E; pc.cE = 30.0f * L2E;
        pc.nA = -0.5f * m.nu_minus; pc.nB = m.nu0 + 0.5f * m.nu_minus;
        pc.f0 = -m.cs[0] * Nz; pc.f1 = -m.cs[1] * Nz; pc.f2 = -m.cs[2] * m.inv_Pr * Nz;
    }
    int step = 0;
    for (int iv = 0; iv < n_save - 1; iv++) {
        const float t0 = save_times[iv];
        const float dt = (save_times[iv + 1] - t0) / (float)substeps;
        for (int s = 0; s < substeps; s++, step++) {
            const float ts = t0 + (float)s * dt;
            V16 Xs[3], Kacc[3];
#pragma unroll
            for (int q = 0; q < 3; q++) { Xs[q] = Xn[q]; Kacc[q].t[0] = (f32x4t)(0.0f); Kacc[q].t[1] = (f32x4t)(0.0f); }
#pragma nounroll
            for (int st = 0; st < 4; st++) {
                const float ca = st == 0 ? 0.0f : (st == 3 ? 1.0f : 0.5f);
                const float cb = (st == 0 || st == 3) ? 1.0f / 6.0f : 1.0f / 3.0f;
                RT_STAMP_BEGIN();
                if (tp) {
                    float* o = tp + ((size_t)step * 4 + st) * 3072;
#pragma unroll
                    for (int q = 0; q < 3; q++)
#pragma unroll
                        for (int tau = 0; tau < 2; tau++) *reinterpret_cast<f32x4v*>(o + (q * 4 + 2 * tau) * 256) = Xs[q].t[tau];
                }
                bc.t[2] = rt_top_flux(m, bc5, ts + ca * dt);
                RT_STAMP(0);
                // ---- three MLPs -------------------------------------------------------------------------------------
                f32x4t A1[10];
                // operand addresses stay (lane base + immediate): left loop-invariant, all ~150 of them are computed outside the time loop and spilled
                int lz = lane;
                if constexpr (SPLIT) asm volatile("" : "+v"(lz));
                if constexpr (SPLIT) {
                    // k-block (= variable) outer, output tile inner: one variable's B planes live at a time, ten independent accumulation chains
#pragma unroll
                    for (int t = 0; t < 10; t++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int Q = 4 * t + r;
                            A1[t][r] = Q < 39 ? bl[RT_B1C + rt16_q_net(Q) * 50 + min(4 * rt16_q_quad(Q) + g, 49)] : 0.0f;
                        }
                    Bf3 Apf = rt16_ldA(simg, 0, lz);
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        // B operand of the 32-deep k-block: the variable's eight levels of this lane, split exactly into three bf16 planes
                        const float x8[8] = {Xs[q].t[0][0], Xs[q].t[0][1], Xs[q].t[0][2], Xs[q].t[0][3], Xs[q].t[1][0], Xs[q].t[1][1], Xs[q].t[1][2], Xs[q].t[1][3]};
                        const Bf3 XB = bf3_split8(x8);
#pragma unroll
                        for (int t = 0; t < 10; t++) {
                            const Bf3 Ac = Apf;
                            const int nx = q * 10 + t + 1;                                        // the group after (q, t) in this order
                            if (nx < 30) Apf = rt16_ldA(simg, 3 * (nx % 10) + nx / 10, lz);
                            auto finish = [&](int tt) {        // tile tt is complete: tape store, activation
                                float* oz = tz ? tz + ((size_t)step * 4 + st) * RT_TAPEZ + 2 * tt * 256 : nullptr;
                                if (tz) *reinterpret_cast<f32x4v*>(oz) = A1[tt];
                                // (side-effect-free arithmetic is not ordered against the scheduling fences when the block is linearised: the empty
                                //  asm statements pin the activation's inputs below the products' issue point and its results above the closing fence)
#pragma unroll
                                for (int r = 0; r < 4; r++) asm volatile("" : "+v"(A1[tt][r]));
                                A1[tt] = rt_act4<ACT, false>(A1[tt]);       // scalar f32: this filler issues beside the partner wave's bf16 MFMAs (see rt_mish4_scalar)
#pragma unroll
                                for (int r = 0; r < 4; r++) asm volatile("" : "+v"(A1[tt][r]));
                            };
                            if (q == 2) RT_SCHED_HARD();
                            __builtin_amdgcn_s_setprio(1);
                            A1[t] = mfma16_bf3(Ac, XB, A1[t]);
                            __builtin_amdgcn_s_setprio(0);
                            if (q == 2) {
                                // the last k-block finishes the tiles one by one: tile t - 1's tape store and activation are issued BETWEEN tile t's
                                // six products (one wave issues in order: left to the scheduler, all activations sink behind all MFMAs)
                                if (t > 0) {
                                    finish(t - 1);
#pragma unroll
                                    for (int u = 0; u < 6; u++) {
                                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                                        __builtin_amdgcn_sched_group_barrier(0x402, 9, 0);
                                    }
                                }
                                RT_SCHED_HARD();
                                if (t == 9) finish(9);
                            } else
                                RT_SCHED_FENCE();
                        }
                    }
                } else {
                auto finish1 = [&](int tt) {          // tile tt of layer 1 is complete: Z1 tape store, activation (pinned as in `finish` above)
                    float* oz = tz ? tz + ((size_t)step * 4 + st) * RT_TAPEZ + 2 * tt * 256 : nullptr;
                    if (tz) *reinterpret_cast<f32x4v*>(oz) = A1[tt];
#pragma unroll
                    for (int r = 0; r < 4; r++) asm volatile("" : "+v"(A1[tt][r]));
                    A1[tt] = rt_act4<ACT>(A1[tt]);
#pragma unroll
                    for (int r = 0; r < 4; r++) asm volatile("" : "+v"(A1[tt][r]));
                };
#pragma unroll
                for (int t = 0; t < 10; t++) {
                    f32x4t acc;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int Q = 4 * t + r;
                        acc[r] = Q < 39 ? wl[RT_B1C + rt16_q_net(Q) * 50 + min(4 * rt16_q_quad(Q) + g, 49)] : 0.0f;
                    }
                    const int base = a1b[t];
                    // (tile t - 1's tape store and activation issued between tile t's MFMAs instead: 35.4 ms against 34.0-34.9 — two waves per SIMD already overlap what can be overlapped)
                    acc = rt16_chain<24, 8>(wl, acc, [=](int k) { return base + (k >> 3) * 32 + ((k >> 2) & 1) * 16 + (k & 3); },
                                            [&](int k) { return Xs[k >> 3].t[(k >> 2) & 1][k & 3]; });
                    A1[t] = acc;
                    finish1(t);
                }
                }
                RT_STAMP(1);
                V16 O[3];
#pragma unroll
                for (int n = 0; n < 3; n++) {
                    f32x4t A2[2];
                    Bf3 HB[2];
                    if constexpr (SPLIT) {
                        // net n's 13 quads of layer-1 activations as two 32-deep k-blocks (element e of block c: quad 8 c + e; three zero slots)
#pragma unroll
                        for (int c = 0; c < 2; c++) {
                            float a8[8];
#pragma unroll
                            for (int e = 0; e < 8; e++) a8[e] = 8 * c + e < 13 ? A1[rt16_q_slot(n, 8 * c + e) >> 2][rt16_q_slot(n, 8 * c + e) & 3] : 0.0f;
                            HB[c] = bf3_split8(a8);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        f32x4t acc;
#pragma unroll
                        for (int r = 0; r < 4; r++) acc[r] = (4 * u + r < 5) ? bl[RT_B2C + n * 20 + 4 * (4 * u + r) + g] : 0.0f;
                        if constexpr (SPLIT) {
                            const Bf3 Aa = rt16_ldA(simg, 30 + 4 * n + 2 * u, lz), Ab = rt16_ldA(simg, 30 + 4 * n + 2 * u + 1, lz);
                            __builtin_amdgcn_s_setprio(1);
                            acc = mfma16_bf3(Aa, HB[0], acc);
                            acc = mfma16_bf3(Ab, HB[1], acc);
                            __builtin_amdgcn_s_setprio(0);
                            RT_SCHED_FENCE();
                        } else {
                        const int base = a2b[u] + n * 20 * RT_LD2, basel = a2l[u] + n * 20 * RT_LD2;
                        acc = rt16_chain<13, 13>(wl, acc, [=](int k) { return k < 12 ? base + 4 * k : basel; },
                                                 [&](int k) { return A1[rt16_q_slot(n, k) >> 2][rt16_q_slot(n, k) & 3]; });
                        }
                        // (SPLIT: the four values of tile 0 on scalar f32, as layer 1; tile 1 has ONE live value, which the compiler evaluates on scalar instructions from
                        //  either form — its packed source form is kept, because there the split below contracts its residual onto the last product, and the bits hang on it)
                        A2[u] = SPLIT && u == 0 ? rt_act4<ACT, false>(acc) : rt_act4<ACT>(acc);
                    }
                    Bf3 GB;
                    if constexpr (SPLIT) {
                        const float a8[8] = {A2[0][0], A2[0][1], A2[0][2], A2[0][3], A2[1][0], 0.0f, 0.0f, 0.0f};
                        GB = bf3_split8(a8);
                    }
#pragma unroll
                    for (int v = 0; v < 2; v++) {
                        f32x4t acc;
#pragma unroll
                        for (int r = 0; r < 4; r++) acc[r] = bl[RT_B3C + n * 32 + 16 * v + 4 * g + r];
                        if constexpr (SPLIT) {
                            const Bf3 Aa = rt16_ldA(simg, 42 + 2 * n + v, lz);
                            __builtin_amdgcn_s_setprio(1);
                            O[n].t[v] = mfma16_bf3(Aa, GB, acc);
                            __builtin_amdgcn_s_setprio(0);
                            RT_SCHED_FENCE();
                        } else {
                        const int base = a3b[v] + n * 31 * RT_LD3;
                        O[n].t[v] = rt16_chain<5, 5>(wl, acc, [=](int k) { return base + 4 * k; },
                                                     [&](int k) { return A2[k >> 2][k & 3]; });
                        }
                    }
                }
                RT_STAMP(2);
                // ---- physics (predict_flux / predict_NDE), face index = level index ----------------------------------
                V16 F[3];
                {
                    V16 Ud, Vd, Td;
                    if (m.mpp || m.ca) {
                        Ud = shift_down16(Xs[0], lane, 0.0f); Vd = shift_down16(Xs[1], lane, 0.0f); Td = shift_down16(Xs[2], lane, 0.0f);
                    }
                    if (m.mpp) {
                        // the Richardson-number closure; uniform factors folded (see rt_physics_vjp): d = level difference, a = σ (Nz d + ε),
                        // Ri = B (Nz d_T + ε) / S2, tanh via exp2, ν = nB + nA tanh, diffusive flux = -(c Nz) ν d.  On f32 MFMAs: pairs of adjacent levels
                        // on packed f32 arithmetic (two levels per issue slot).  On bf16 MFMAs (SPLIT): the same operations level by level on scalar f32
                        // — v_fma_f32 where the packed form compiles to v_pk_fma_f32, contraction off so that nothing else fuses: the same bits — because
                        // beside the partner wave's bf16 MFMAs the packed instructions are the dearer ones
                        if constexpr (SPLIT) {
#pragma unroll
                            for (int tau = 0; tau < 2; tau++)
#pragma unroll
                                for (int r = 0; r < 4; r++) {
#pragma clang fp contract(off)
                                    const float dU = Xs[0].t[tau][r] - Ud.t[tau][r], dV = Xs[1].t[tau][r] - Vd.t[tau][r], dT = Xs[2].t[tau][r] - Td.t[tau][r];
                                    const float a1 = fmaf(dU, pc.cU, pc.sU), a2 = fmaf(dV, pc.cV, pc.sV);
                                    const float rS = __builtin_amdgcn_rcpf(fmaf(a1, a1, a2 * a2));        // (the shipped packed form: v_pk_mul a2 a2, then v_pk_fma a1 a1)
                                    const float arg = fmaf(fmaf(dT, pc.cB, pc.sB) * rS, pc.kE, pc.oE);
                                    const float e = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(arg, -pc.cE, pc.cE));
                                    const float rc = __builtin_amdgcn_rcpf(e + 1.0f);
                                    const float nu = fmaf(fmaf(rc, -2.0f, 1.0f), pc.nA, pc.nB);
                                    F[0].t[tau][r] = fmaf(nu * dU, pc.f0, O[0].t[tau][r]);
                                    F[1].t[tau][r] = fmaf(nu * dV, pc.f1, O[1].t[tau][r]);
                                    F[2].t[tau][r] = fmaf(nu * dT, pc.f2, O[2].t[tau][r]);
                                }
                        } else
#pragma unroll
                        for (int tau = 0; tau < 2; tau++)
#pragma unroll
                            for (int r = 0; r < 4; r += 2) {
                                const f32x2v dU = {Xs[0].t[tau][r] - Ud.t[tau][r], Xs[0].t[tau][r + 1] - Ud.t[tau][r + 1]};
                                const f32x2v dV = {Xs[1].t[tau][r] - Vd.t[tau][r], Xs[1].t[tau][r + 1] - Vd.t[tau][r + 1]};
                                const f32x2v dT = {Xs[2].t[tau][r] - Td.t[tau][r], Xs[2].t[tau][r + 1] - Td.t[tau][r + 1]};
                                const f32x2v a1 = dU * pc.cU + pc.sU, a2 = dV * pc.cV + pc.sV;
                                const f32x2v s2 = a2 * a2 + a1 * a1;
                                f32x2v rS;
                                rS.x = __builtin_amdgcn_rcpf(s2.x);
                                rS.y = __builtin_amdgcn_rcpf(s2.y);
                                const f32x2v arg = ((dT * pc.cB + pc.sB) * rS) * pc.kE + pc.oE;
                                f32x2v e;
                                e.x = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(arg.x, -pc.cE, pc.cE));
                                e.y = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(arg.y, -pc.cE, pc.cE));
                                const f32x2v e1 = e + 1.0f;
                                f32x2v rc;
                                rc.x = __builtin_amdgcn_rcpf(e1.x);
                                rc.y = __builtin_amdgcn_rcpf(e1.y);
                                const f32x2v nu = (rc * -2.0f + 1.0f) * pc.nA + pc.nB;
                                const f32x2v o0 = {O[0].t[tau][r], O[0].t[tau][r + 1]}, o1 = {O[1].t[tau][r], O[1].t[tau][r + 1]},
                                             o2 = {O[2].t[tau][r], O[2].t[tau][r + 1]};
                                const f32x2v f0 = (nu * dU) * pc.f0 + o0, f1 = (nu * dV) * pc.f1 + o1, f2 = (nu * dT) * pc.f2 + o2;
                                F[0].t[tau][r] = f0.x; F[0].t[tau][r + 1] = f0.y;
                                F[1].t[tau][r] = f1.x; F[1].t[tau][r + 1] = f1.y;
                                F[2].t[tau][r] = f2.x; F[2].t[tau][r + 1] = f2.y;
                            }
                        if (g == 0) {                                              // face 0: the bottom boundary
#pragma unroll
                            for (int k = 0; k < 3; k++) F[k].t[0][0] = m.zero_w ? bc.b[k] - m.s0[k] : bc.b[k];
                        }
                    } else
#pragma unroll
                    for (int tau = 0; tau < 2; tau++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const bool in = !(tau == 0 && r == 0 && g == 0);       // face >= 1
                            float f0 = in ? O[0].t[tau][r] : 0.0f, f1 = in ? O[1].t[tau][r] : 0.0f, f2 = in ? O[2].t[tau][r] : 0.0f;
                            if (!m.zero_w && !in) { f0 = bc.b[0]; f1 = bc.b[1]; f2 = bc.b[2]; }
                            if (m.ca && in) {
                                const float gT = (Xs[2].t[tau][r] - Td.t[tau][r]) * Nz;
                                f2 -= m.cs[2] * m.kappa * fminf(0.0f, gT);
                            }
                            F[0].t[tau][r] = f0; F[1].t[tau][r] = f1; F[2].t[tau][r] = f2;
                        }
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float top = m.zero_w ? bc.t[k] - m.s0[k] : bc.t[k];
                    const V16 Fu = shift_up16(F[k], lane, top);
#pragma unroll
                    for (int tau = 0; tau < 2; tau++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            float v = -m.A[k] * (Fu.t[tau][r] - F[k].t[tau][r]);
                            if (k == 0) v += m.cor_u * (m.sig_v * Xs[1].t[tau][r] + m.mu_v);
                            if (k == 1) v -= m.cor_v * (m.sig_u * Xs[0].t[tau][r] + m.mu_u);
                            F[k].t[tau][r] = v;                           // F now holds the tendency K
                        }
                }
                RT_STAMP(3);
                // ---- RK4 bookkeeping: accumulate, form the next stage input ------------------------------------------
                const float can = st == 2 ? 1.0f : 0.5f;                    // abscissa of the NEXT stage
#pragma unroll
                for (int q = 0; q < 3; q++)
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) {
                        Kacc[q].t[tau] += cb * F[q].t[tau];
                        Xs[q].t[tau] = Xn[q].t[tau] + (can * dt) * F[q].t[tau];
                    }
                RT_STAMP(4);
            }
#pragma unroll
            for (int q = 0; q < 3; q++)
#pragma unroll
                for (int tau = 0; tau < 2; tau++) Xn[q].t[tau] += dt * Kacc[q].t[tau];
            if (s == substeps - 1 && sol && valid) {
#pragma unroll
                for (int q = 0; q < 3; q++)
#pragma unroll
                    for (int tau = 0; tau < 2; tau++)
                        *reinterpret_cast<f32x4v*>(sol + ((size_t)col * n_save + iv + 1) * 96 + q * 32 + 16 * tau + 4 * g) = Xn[q].t[tau];
            }
        }
    }
#ifdef COLNDE_STAMPS_FWD
    rs_acc[6] = __builtin_amdgcn_s_memtime() - rs_k0;          // whole kernel, shader ticks
    rs_acc[7] = __builtin_amdgcn_s_memrealtime() - rs_r0;      // whole kernel, 100 MHz reference ticks
    RT_STAMP_FLUSH();
#endif
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
bool rt_supported(const DevModel& m) {
    return m.model == COLNDE_MODEL_WIND_MIXING && m.Nz == 32 && m.n_layers == 3 && m.sizes[0] == 96 && m.sizes[1] == 50 &&
           m.sizes[2] == 20 && m.sizes[3] == 31 && m.acts[0] == m.acts[1] && m.acts[2] == COLNDE_ACT_IDENTITY &&
           !m.smooth_NN && !m.smooth_Ri && !m.inplace;
}

size_t rt_forward_lds_bytes() { return (size_t)RT_IMG_FLOATS * sizeof(float); }
size_t rt_adjoint_lds_bytes() { return ((size_t)((RT_IMG_FLOATS + 3) & ~3) + RT_WAVES * (3072 + RT_TB)) * sizeof(float); }
// rt16_forward_kernel; SPLIT: the bf16 operand planes and the fp32 biases
static size_t rt16_forward_lds_bytes(bool split) { return split ? ((size_t)RT_SIMG_WORDS + (RT_IMG_FLOATS - RT_B1C)) * sizeof(float) : rt_forward_lds_bytes(); }
static size_t rt_dw1_lds_bytes() { return RT_WAVES * RT_DW1_LDS * sizeof(float); }
size_t rt_tape_floats(int n_col, int n_steps) { return (size_t)((n_col + RT_COLS - 1) / RT_COLS) * n_steps * 4 * 3072; }
size_t rt_tape2_floats(int n_col, int n_steps) { return (size_t)((n_col + RT_COLS - 1) / RT_COLS) * n_steps * 4 * RT_TAPE2; }
size_t rt_tapez_floats(int n_col, int n_steps) { return (size_t)((n_col + RT_COLS - 1) / RT_COLS) * n_steps * 4 * RT_TAPEZ; }
int rt_n_wtiles(int n_col) { return (n_col + RT_COLS - 1) / RT_COLS; }
int rt_dw1_waves(int n_col, int n_steps) {
    const long items = (long)rt_n_wtiles(n_col) * n_steps * 4;
    const long w = items < 1024 ? items : 1024;
    return (int)((w + RT_WAVES - 1) / RT_WAVES) * RT_WAVES;
}

// ---- kernel selection (kernel_select.h).  ONE selector per kernel family names its instantiations: the launchers call it with
// the run's flags, rt_set_attributes() with every value of them, so whatever can be launched has had its dynamic-LDS limit raised.
// nullptr: there is no such kernel.  To add an instantiation, add it to its family's selector (and, for a new flag, to the loop below).
using RtForwardFn = decltype(&rt_forward_kernel<COLNDE_ACT_RELU>);
using Rt16ForwardFn = decltype(&rt16_forward_kernel<COLNDE_ACT_RELU, false>);
using RtAdjointFn = decltype(&rt_adjoint_kernel<COLNDE_ACT_RELU, false>);

static RtForwardFn rt_forward_pick(int act) {
    RtForwardFn k = nullptr;
    with_act(act, [&](auto A) { k = rt_forward_kernel<decltype(A)::value>; });
    return k;
}
static Rt16ForwardFn rt16_forward_pick(int act, bool split) {
    Rt16ForwardFn k = nullptr;
    with_act(act, [&](auto A) { with_bools([&](auto S) { k = rt16_forward_kernel<decltype(A)::value, decltype(S)::value>; }, split); });
    return k;
}
static RtAdjointFn rt_adjoint_pick(int act, bool ztape, bool split) {
    RtAdjointFn k = nullptr;
    with_act(act, [&](auto A) {
        with_bools([&](auto Z, auto S) {
            if constexpr (decltype(Z)::value || !decltype(S)::value) k = rt_adjoint_kernel<decltype(A)::value, decltype(Z)::value, decltype(S)::value>;      // the split kernel reads the Z1 tape
        }, ztape, split);
    });
    return k;
}
static auto rt_dw1_pick(bool split) { return split ? rt_dw1_split_kernel : rt_dw1_kernel; }

hipError_t rt_set_attributes() {
    hipError_t e = hipSuccess;
    const size_t v = 160 * 1024;
    auto set = [&](auto* k) { if (k && e == hipSuccess) e = set_max_lds(k, v); };
    for_each_act([&](auto A) {
        set(rt_forward_pick(A));
        for (int a = 0; a < 2; a++) {
            set(rt16_forward_pick(A, a));
            for (int b = 0; b < 2; b++) set(rt_adjoint_pick(A, a, b));
        }
    });
    for (int split = 0; split < 2; split++) set(rt_dw1_pick(split));
    return e;
}

hipError_t rt_launch_pack(const DevModel& m, const float* w, float* wimg, hipStream_t stream, int n_models) {
    hipLaunchKernelGGL(rt_pack_kernel, dim3((RT_IMG_FLOATS + 255) / 256, n_models), dim3(256), 0, stream, m, w, wimg, (int)RT_IMG_STRIDE);
    return hipGetLastError();
}

// COLNDE_RT_FWD=32 selects the one-wave-per-SIMD 32-column forward kernel (A/B aid; it does not tape Z1)
bool rt_forward_is32() {
    const char* e = getenv("COLNDE_RT_FWD");
    return e && atoi(e) == 32;
}

hipError_t rt_launch_forward(const DevModel& m, const float* wimg, const float* x0, const float* bcs,
                             const float* save_times, int n_save, int substeps, float* sol, float* tape, float* tapez,
                             int n_col, bool fwd32, bool split, hipStream_t stream) {
    // COLNDE_RT_FWD=32 selects the one-wave-per-SIMD 32-column kernel (A/B aid); default: 16-column tiles, two waves per SIMD
    if (fwd32) {
        const int n_wtiles = (n_col + RT_COLS - 1) / RT_COLS;
        const dim3 grid((n_wtiles + RT_WAVES - 1) / RT_WAVES), block(64 * RT_WAVES);
        const auto k = rt_forward_pick(m.acts[0]);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, grid, block, rt_forward_lds_bytes(), stream, m, wimg, x0, bcs, save_times, n_save, substeps, sol, tape, n_col);
    } else {
        const int n_wt16 = 2 * ((n_col + RT_COLS - 1) / RT_COLS);
        // small problems spread over the CUs first (one wavefront per workgroup up to 256 tiles), then fill the SIMDs
        int wpw = (n_wt16 + 255) / 256;
        wpw = wpw < 1 ? 1 : (wpw > RT16_WAVES ? RT16_WAVES : wpw);
        const dim3 grid((n_wt16 + wpw - 1) / wpw), block(64 * wpw);
        // split: the nets on the bf16 pipe with exact three-way operand splitting (COLNDE_MATRIX_BF16X3_EXACT)
        if (split) hipLaunchKernelGGL(rt_pack_split_kernel, dim3(48), dim3(256), 0, stream, wimg, reinterpret_cast<unsigned*>(const_cast<float*>(wimg)) + RT_SIMG_OFF);
        const auto k = rt16_forward_pick(m.acts[0], split);
        if (!k) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, grid, block, rt16_forward_lds_bytes(split), stream, m, wimg, x0, bcs, save_times, n_save, substeps, sol, tape, tapez, n_col);
    }
    return hipGetLastError();
}

hipError_t rt_launch_adjoint(const DevModel& m, const float* wimg, const float* bcs, const float* save_times, int n_save,
                             int substeps, const float* sol, const float* truth, const float* tape, float* tape2,
                             const float* tapez, const LossWeights& lw, float* slab, int n_col, bool want_split, hipStream_t stream) {
    const int n_wtiles = rt_n_wtiles(n_col);
    const dim3 grid((n_wtiles + RT_WAVES - 1) / RT_WAVES), block(64 * RT_WAVES);
    // with the Z1 tape: the W1^T products on the bf16 pipe with exact three-way operand splitting (COLNDE_MATRIX_BF16X3_EXACT)
    const bool split = want_split && tapez;
    if (split) hipLaunchKernelGGL(rt_pack_split_adj_kernel, dim3(30), dim3(256), 0, stream, wimg, reinterpret_cast<unsigned*>(const_cast<float*>(wimg)) + RT_ASIMG_OFF);
    const auto k = rt_adjoint_pick(m.acts[0], tapez != nullptr, split);
    if (!k) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, grid, block, rt_adjoint_lds_bytes(), stream, m, wimg, bcs, save_times, n_save, substeps, sol, truth, tape, tape2, tapez, lw, slab, n_col);
    return hipGetLastError();
}

hipError_t rt_launch_dw1(const DevModel& m, const float* tape, const float* tape2, int n_col, int n_steps, float* slab_rows,
                         bool split, hipStream_t stream) {
    const long items = (long)rt_n_wtiles(n_col) * n_steps * 4;
    const int waves = rt_dw1_waves(n_col, n_steps);
    // split: dW1 on the bf16 pipe with exact three-way operand splitting (COLNDE_MATRIX_BF16X3_EXACT)
    hipLaunchKernelGGL(rt_dw1_pick(split), dim3(waves / RT_WAVES), dim3(64 * RT_WAVES), rt_dw1_lds_bytes(), stream, m, tape, tape2, items, slab_rows);
    return hipGetLastError();
}

hipError_t rt_debug_read_stamps(unsigned long long* out16) { return rt_read_unit_stamps(out16); }
