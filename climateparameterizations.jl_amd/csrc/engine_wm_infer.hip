// engine_wm_infer.hip — the deployment half of the wind-mixing NDE (gfx950 only): NN_uw_forcing / NN_vw_forcing / NN_wT_forcing of
// wind_mixing/src/NDE_oceananigans.jl:288-329 as progress_neural_network (:380-405) evaluates them every iteration of the embedding ocean
// column, alone or fused with modified_pacanowski_philander! (:61-101) on the same state.
//
// Layout.  One wavefront owns 32 columns, in the 32x32 MFMA accumulator layout regtile uses: lane (j = lane & 31, h = lane >> 5) holds, in
// element r of a 16-float tile, row rho(r, h) = (r & 3) + 8 (r >> 2) + 4 h of column j, so element r of a tile IS the B operand of k-step r
// of v_mfma_f32_32x32x2_f32 and a layer feeds the next one without lane movement.  Levels 8 q + 4 h .. + 3 of a field are one 16-byte load
// of lane (j, h) straight into that layout (q = 0..3: the four loads of a lane pair cover the column's 128-byte row), and the finished
// d/dz rows leave the same way as 16-byte stores: the state is read once, no staging for the networks.
//   layer 1: the 3 x 50 outputs of the three nets are stacked into 5 tiles (they share the input); register G = 16 tile + r carries
//            features (2 g, 2 g + 1) of net G / 25, g = G % 25 (G >= 75: padding);  layer 2: registers r < 10 carry features (2 r, 2 r + 1);
//            layer 3: row = index of the interior face.  345 MFMAs per 32 columns.
// Weights.  A persistent workgroup (4 waves) copies the flat weight vector VERBATIM into LDS once (78 KB: no packed image is needed — the
// A operand of every k-step is `per-lane base + compile-time offset` into Flux's column-major W, one ds_read_b32 per 64-cycle MFMA) and
// walks groups of four tiles.  The dense chains run on the f32 matrix pipe under either matrix_arithmetic: the three nets' bf16 planes
// (117 KB) do not fit beside the fused step's state rows, and one resident image serves both kernels (colnde_describe: wm_infer=f32).
// Fused step.  The raw state also goes to per-wave LDS rows [3][32][33]; one lane per column runs the shared sweeps of mpp_sweep.h in
// place and the wave writes u', v', T' back as coalesced float4 — before the networks, so the stores drain under the MFMA chains.  The
// networks read the state from the registers loaded BEFORE the sweep: the d/dz arrays are those of the state as given.
// Flux diagnosis (DIAG).  diagnose_NN_flux_uw / _vw / _wT (:226-286): the TOTAL fluxes on the 33 faces, F − ν ∂z φ.  Its NN faces are
// [0; inv(scaling).(y) .- inv(scaling)(0); top] (:235, :253, :274-276), evaluated as written: (σ y + μ) − (σ·0 + μ) in float32 — neither σ y nor the
// forcing chain's convention, which subtracts inv(scaling) of the ALREADY unscaled first element (the uw[1] quirk below, :292, :301).  So the d/dz
// arrays do not integrate to these faces.  Row rho(r, h) of a layer-3 tile is interior face rho + 1, the upper face of level rho — the level the same
// element of the raw state registers holds: the level differences, the diffusivities (mpp_sweep.h, the step's own face function with c = 1) and
// the subtraction are lane-local but for the level above every fourth one, which comes from lane ^ 32 (one exchange per four levels and
// field, before the networks); lane (j, 0) adds face 0, lane (j, 1)'s last element is the top face (halo cells above and below, or the
// zero-gradient fill).  A wave's 32 columns x 33 faces are one contiguous 16-byte-aligned 4,224-byte span of each output and the per-wave LDS rows
// [3][32][33] are its image: ν ∂z φ waits there during the chains (no registers held across them), each net's faces replace it and leave as
// coalesced 16-byte pieces.  The fused step's state rows are free once u', v', T' have been read out, so FUSED + DIAG uses the same rows.
#include "engine_wm_infer.h"
#include "colnde_dev.h"
#include "kernel_select.h"

typedef float wm_f32x16 __attribute__((ext_vector_type(16)));

#define WM_WAVES 4
#define WM_W_LDS (((3 * WM_NET + 3) / 4) * 4)             // floats of the weight image (padded to 16 bytes)
#define WM_LD (WM_NZ + 1)                                  // fused: row stride of the staged state (conflict-free column walks)
#define WM_FS (32 * WM_LD)                                 // ... floats per field of one wave's 32 columns
#define WM_OFF_B1 (96 * WM_H1)
#define WM_OFF_W2 (WM_OFF_B1 + WM_H1)
#define WM_OFF_B2 (WM_OFF_W2 + WM_H1 * WM_H2)
#define WM_OFF_W3 (WM_OFF_B2 + WM_H2)
#define WM_OFF_B3 (WM_OFF_W3 + WM_H2 * 31)
#define WM_RHO0(r) (((r) & 3) + 8 * ((r) >> 2))
// the staged state rows belong to ONE wave, whose LDS operations complete in order: no s_barrier, only the compiler is held to the order
#define WM_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

struct WmScal { float mu[3], inv_sig[3], fmu[3], fsig[3], inv_dz, dz; int act1, act2; };

// inv(scaling)(y) − inv(scaling)(0) = (σ y + μ) − (σ·0 + μ), each operation rounded to float32 as the reference's broadcast does
__device__ __forceinline__ float wm_unscaled_minus_zero(float sig, float mu, float y) {
#pragma clang fp contract(off)
    return (sig * y + mu) - (sig * 0.0f + mu);
}

__device__ __forceinline__ wm_f32x16 wm_mfma(float a, float b, wm_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// 16-byte loads of one tile's state: xr[f][q] = levels 8 q + 4 h .. + 3 of field f of the lane's column (zeros past the last column)
__device__ __forceinline__ void wm_load_tile(const float* const (&src)[3], long long col, int h, int n_col, f32x4 (&xr)[3][4]) {
#pragma unroll
    for (int f = 0; f < 3; f++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
            if (col < n_col) z = *reinterpret_cast<const f32x4*>(src[f] + (size_t)col * WM_NZ + 8 * q + 4 * h);
            xr[f][q] = z;
        }
}

// FUSED: the diffusion step too; DIAG: the face fluxes; the d/dz arrays are written unless the launch is the diagnosis alone (DIAG && !FUSED)
template <bool FUSED, bool DIAG>
__global__ void __launch_bounds__(64 * WM_WAVES, 1)
wm_infer_kernel(const float* __restrict__ w, WmScal S, const float* u, const float* v, const float* T, const float* __restrict__ top,
                const float* __restrict__ halo_bottom, const float* __restrict__ halo_top, MppParams P, float* __restrict__ dz_uw,
                float* __restrict__ dz_vw, float* __restrict__ dz_wT, float* uo, float* vo, float* To, float* __restrict__ f_uw,
                float* __restrict__ f_vw, float* __restrict__ f_wT, int n_col, int n_groups) {
    constexpr bool DZ = FUSED || !DIAG, RAW = FUSED || DIAG;
    extern __shared__ __attribute__((aligned(16))) float wm_smem[];
    float* wl = wm_smem;
    for (int i = threadIdx.x; i < WM_W_LDS; i += 64 * WM_WAVES) wl[i] = i < 3 * WM_NET ? w[i] : 0.0f;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const float* const src[3] = {u, v, T};
    float* const dzs[3] = {dz_uw, dz_vw, dz_wT};
    float* const fcs[3] = {f_uw, f_vw, f_wT};
    float* const st = wm_smem + WM_W_LDS + wave * 3 * WM_FS;          // FUSED, DIAG: this wave's rows [3][32][33]

    // A-operand bases (floats into wl).  Row i of an MFMA's A is row i of its result: register ri of lane half hi
    const int ri = (j & 3) + 4 * (j >> 3), hi = (j >> 2) & 1;
    int a1[5];                                    // layer 1, stacked tile tl: net n, feature 2 g + hi;  + 50 (32 t + rho(v, 0)) per k-step
#pragma unroll
    for (int tl = 0; tl < 5; tl++) {
        const int G = min(16 * tl + ri, 74);      // (G >= 75: padding rows, never consumed)
        a1[tl] = (G / 25) * WM_NET + 2 * (G % 25) + hi + 4 * h * WM_H1;
    }
    const int a2 = WM_OFF_W2 + min(2 * ri + hi, WM_H2 - 1) + h * WM_H2;     // layer 2: output feature 2 ri + hi; + 40 s per k-step
    const int a3 = WM_OFF_W3 + min(j, 30) + h * 31;                        // layer 3: output = interior face j;  + 62 s per k-step

    f32x4 xr[3][4];
    int g = blockIdx.x;
    if (g < n_groups) wm_load_tile(src, (long long)(g * WM_WAVES + wave) * 32 + j, h, n_col, xr);
    for (; g < n_groups; g += gridDim.x) {
        const long long col0 = (long long)(g * WM_WAVES + wave) * 32, col = col0 + j;
        const bool valid = col < n_col;
        // scaled input in the B layout: xs[16 t + 4 q + r] = field t, level rho(4 q + r, h)
        float xs[48];
#pragma unroll
        for (int f = 0; f < 3; f++)
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int r = 0; r < 4; r++) xs[16 * f + 4 * q + r] = (xr[f][q][r] - S.mu[f]) * S.inv_sig[f];

        float raw[RAW ? 48 : 1];                 // the unscaled state: the sweeps' rows, the level differences of the diagnosis
        if (RAW) {
#pragma unroll
            for (int f = 0; f < 3; f++)
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int r = 0; r < 4; r++) raw[(16 * f + 4 * q + r) % (RAW ? 48 : 1)] = xr[f][q][r];
        }
        // the next group's state, in flight under this group's work (one wave per SIMD: nothing else hides the latency; other columns,
        // so in-place outputs do not touch them)
        if (g + (int)gridDim.x < n_groups) wm_load_tile(src, (long long)((g + (int)gridDim.x) * WM_WAVES + wave) * 32 + j, h, n_col, xr);
        if (RAW) WM_WAVE_SYNC();                    // (the previous group's rows have been read out)
        if (FUSED) {
#pragma unroll
            for (int f = 0; f < 3; f++)
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int r = 0; r < 4; r++) st[f * WM_FS + j * WM_LD + 8 * q + 4 * h + r] = raw[(16 * f + 4 * q + r) % (RAW ? 48 : 1)];
            WM_WAVE_SYNC();
            if (h == 0 && valid) mpp_column_step<WM_NZ>(P, st + j * WM_LD, st + WM_FS + j * WM_LD, st + 2 * WM_FS + j * WM_LD, halo_bottom, (size_t)col, n_col);
            WM_WAVE_SYNC();
            float* const dsts[3] = {uo, vo, To};
#pragma unroll
            for (int f = 0; f < 3; f++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int e = i * 64 + lane, cl = e >> 3, k = (e & 7) * 4;
                    if (col0 + cl < n_col) {
                        const float* d = st + f * WM_FS + cl * WM_LD + k;
                        const f32x4 o = {d[0], d[1], d[2], d[3]};
                        *reinterpret_cast<f32x4*>(dsts[f] + (size_t)(col0 + cl) * WM_NZ + k) = o;
                    }
                }
            if (DIAG) WM_WAVE_SYNC();               // (u', v', T' have been read out: the rows take the faces)
        }
        if (DIAG) {
            // ---- ν ∂z u, ν ∂z v, νT ∂z T of the lane's 16 faces (element e: face rho(e, h) + 1) into the rows; face 0 finished here (F = 0)
            float up[3][4];                         // the level above levels 8 q + 4 h + 3: lane ^ 32's first of q (h = 0) or of q + 1 (h = 1)
#pragma unroll
            for (int f = 0; f < 3; f++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float mine = raw[(16 * f + 4 * q) % (RAW ? 48 : 1)], next = q < 3 ? raw[(16 * f + 4 * q + 4) % (RAW ? 48 : 1)] : 0.0f;
                    up[f][q] = __shfl_xor(h == 1 ? mine : next, 32);
                }
            if (h == 1)
#pragma unroll
                for (int f = 0; f < 3; f++)         // above level 31: the halo cell, or the zero-gradient fill
                    up[f][3] = halo_top && valid ? halo_top[(size_t)f * n_col + col] : raw[(16 * f + 15) % (RAW ? 48 : 1)];
#pragma unroll
            for (int e = 0; e < 16; e++) {
                float d[3];
#pragma unroll
                for (int f = 0; f < 3; f++) d[f] = ((e & 3) < 3 ? raw[(16 * f + e + 1) % (RAW ? 48 : 1)] : up[f][e >> 2]) - raw[(16 * f + e) % (RAW ? 48 : 1)];
                float g[3];
                mpp_face_nu_grad(P, S.dz, e == 15 && h == 1, d[0], d[1], d[2], g[0], g[1], g[2]);
#pragma unroll
                for (int f = 0; f < 3; f++) st[f * WM_FS + j * WM_LD + WM_RHO0(e) + 4 * h + 1] = g[f];
            }
            if (h == 0) {
                float d[3], g[3];
#pragma unroll
                for (int f = 0; f < 3; f++) d[f] = halo_bottom && valid ? raw[(16 * f) % (RAW ? 48 : 1)] - halo_bottom[(size_t)f * n_col + col] : 0.0f;
                mpp_face_nu_grad(P, S.dz, true, d[0], d[1], d[2], g[0], g[1], g[2]);
#pragma unroll
                for (int f = 0; f < 3; f++) st[f * WM_FS + j * WM_LD] = 0.0f - g[f];
            }
        }

        // ---- layer 1, the three nets stacked: 5 tiles x 48 k-steps
        wm_f32x16 acc1[5];
#pragma unroll
        for (int tl = 0; tl < 5; tl++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int G = 16 * tl + r < 75 ? 16 * tl + r : 74;
                acc1[tl][r] = wl[(G / 25) * WM_NET + WM_OFF_B1 + 2 * (G % 25) + h];
            }
#pragma unroll
        for (int s = 0; s < 48; s++) {
            const int in0 = 32 * (s >> 4) + WM_RHO0(s & 15);
#pragma unroll
            for (int tl = 0; tl < 5; tl++) acc1[tl] = wm_mfma(wl[a1[tl] + WM_H1 * in0], xs[s], acc1[tl]);
        }
#pragma unroll
        for (int tl = 0; tl < 5; tl++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc1[tl][r] = dev_act(S.act1, acc1[tl][r]);

#pragma unroll
        for (int n = 0; n < 3; n++) {
            // ---- layer 2: 25 k-steps over this net's registers of the stacked tiles
            wm_f32x16 acc2;
#pragma unroll
            for (int r = 0; r < 16; r++) acc2[r] = r < 10 ? wl[n * WM_NET + WM_OFF_B2 + 2 * r + h] : 0.0f;
#pragma unroll
            for (int s = 0; s < 25; s++) {
                const int G = 25 * n + s;
                acc2 = wm_mfma(wl[n * WM_NET + a2 + 2 * WM_H2 * s], acc1[G >> 4][G & 15], acc2);
            }
            // ---- layer 3: 10 k-steps; row rho(r, h) = interior face (row 31: padding)
            wm_f32x16 y;
#pragma unroll
            for (int r = 0; r < 16; r++) y[r] = wl[n * WM_NET + WM_OFF_B3 + min(WM_RHO0(r) + 4 * h, 30)];
#pragma unroll
            for (int s = 0; s < 10; s++) y = wm_mfma(wl[n * WM_NET + a3 + 62 * s], dev_act(S.act2, acc2[s]), y);

            // ---- interior face values in physical units, relative to the first (:292, :301, :318)
            // faces [0; interior; top] (:220-224): the cell's upper face is its own row (row 31: the top flux), its lower face the row below
            const float top_n = h == 1 && valid ? top[(size_t)n * n_col + col] : 0.0f;
            if (DIAG) {
                // ---- the diagnosed total flux: inv(scaling).(y) .- inv(scaling)(0) as written, minus what waits in the rows (each lane its own
                // slots), then the wave's span of this output in 16-byte pieces (a last tile of c columns: 33 c floats, the odd ones singly)
                float* row = st + n * WM_FS + j * WM_LD + 4 * h + 1;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float Fd = r == 15 && h == 1 ? top_n : wm_unscaled_minus_zero(S.fsig[n], S.fmu[n], y[r]);
                    row[WM_RHO0(r)] = Fd - row[WM_RHO0(r)];
                }
                WM_WAVE_SYNC();
                const int cnt = (int)min((long long)32, (long long)n_col - col0) * WM_LD;
                float* o = fcs[n] + (size_t)col0 * WM_LD;
                const float* img = st + n * WM_FS;
                if (cnt > 0) {
#pragma unroll
                    for (int i = 0; i < 5; i++) {
                        const int p = 4 * (i * 64 + lane);
                        if (p + 3 < cnt) *reinterpret_cast<f32x4*>(o + p) = *reinterpret_cast<const f32x4*>(img + p);
                        else if (p < cnt)
                            for (int t = p; t < cnt; t++) o[t] = img[t];
                    }
                }
            }
            if (!DZ) continue;
            const float y0 = __shfl(y[0], j);
            float F[16];
            if (n < 2) {
                // inv(scaling) applied a second time to the ALREADY unscaled first element, as the reference does (sic)
                const float a0 = S.fsig[n] * y0 + S.fmu[n];
                const float ref = S.fsig[n] * a0 + S.fmu[n];
#pragma unroll
                for (int r = 0; r < 16; r++) F[r] = (S.fsig[n] * y[r] + S.fmu[n]) - ref;
            } else {
#pragma unroll
                for (int r = 0; r < 16; r++) F[r] = S.fsig[2] * (y[r] - y0);
            }
            if (h == 1) F[15] = top_n;
            float* out = dzs[n];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float across = __shfl_xor(F[4 * q + 3], 32);        // row 8 q + 3 for h = 1, row 8 q + 7 for h = 0
                const float across_prev = q > 0 ? __shfl_xor(F[4 * q - 1], 32) : 0.0f;
                const float below = h == 1 ? across : across_prev;          // (h = 0, q = 0: face 0 carries no flux)
                f32x4 o;
                o[0] = (F[4 * q] - below) * S.inv_dz;
#pragma unroll
                for (int r = 1; r < 4; r++) o[r] = (F[4 * q + r] - F[4 * q + r - 1]) * S.inv_dz;
                if (valid) *reinterpret_cast<f32x4*>(out + (size_t)col * WM_NZ + 8 * q + 4 * h) = o;
            }
        }
    }
}

hipError_t launch_wm_infer(const WmInferArgs& a, hipStream_t stream) {
    if (a.n_col < 1 || !(a.Lz > 0.0f)) return hipErrorInvalidValue;
    const bool dz_out = a.fused || !a.diag;
    uintptr_t al = (uintptr_t)a.u | (uintptr_t)a.v | (uintptr_t)a.T;
    if (dz_out) al |= (uintptr_t)a.dz_uw | (uintptr_t)a.dz_vw | (uintptr_t)a.dz_wT;
    if (a.fused) al |= (uintptr_t)a.u_out | (uintptr_t)a.v_out | (uintptr_t)a.T_out;
    if (a.diag) al |= (uintptr_t)a.uw | (uintptr_t)a.vw | (uintptr_t)a.wT;
    if (al & 15) return hipErrorInvalidValue;
    int dev = 0, n_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    WmScal S;
    for (int f = 0; f < 3; f++) {
        S.mu[f] = a.mu[f];
        S.inv_sig[f] = 1.0f / a.sigma[f];
        S.fmu[f] = a.mu[3 + f];
        S.fsig[f] = a.sigma[3 + f];
    }
    S.inv_dz = (float)WM_NZ / a.Lz;
    S.dz = a.Lz / (float)WM_NZ;
    S.act1 = a.act1;
    S.act2 = a.act2;
    const int n_tiles = (a.n_col + 31) / 32, n_groups = (n_tiles + WM_WAVES - 1) / WM_WAVES;
    with_bools([&](auto FUSED, auto DIAG) {
        auto* k = wm_infer_kernel<FUSED(), DIAG()>;
        const size_t lds = (WM_W_LDS + (FUSED() || DIAG() ? WM_WAVES * 3 * WM_FS : 0)) * sizeof(float);
        e = set_max_lds(k, lds);
        if (e != hipSuccess) return;
        // persistent: one workgroup per CU, one wave per SIMD with the whole register file (five stacked accumulator tiles, the input, the
        // prefetched next tile: two waves per SIMD spill)
        const int resident = std::max(1, n_cu);
        hipLaunchKernelGGL(k, dim3(std::min(n_groups, resident)), dim3(64 * WM_WAVES), lds, stream, a.weights, S, a.u, a.v, a.T, a.top_flux,
                           a.halo_bottom, a.halo_top, a.mpp, a.dz_uw, a.dz_vw, a.dz_wT, a.u_out, a.v_out, a.T_out, a.uw, a.vw, a.wT, a.n_col, n_groups);
        e = hipGetLastError();
    }, a.fused, a.diag);
    return e;
}
