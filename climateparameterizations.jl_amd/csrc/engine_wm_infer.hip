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
// Ensemble (wm_infer_ens_kernel).  The K models of an ensemble in one launch: the same per-tile statements (wm_infer_tile.inc, included by both kernels)
// inside a walk over a model-major work list, the weight image re-copied at every model boundary.
#include "engine_wm_infer.h"
#include "colnde_dev.h"
#include "kernel_select.h"
#include "wm_infer_dev.h"              // the tile layout, the operand bases and the face stores, shared with engine_wm_profile.hip

struct WmScal { float mu[3], inv_sig[3], fmu[3], fsig[3], inv_dz, dz; int act1, act2; };

// inv(scaling)(y) − inv(scaling)(0) = (σ y + μ) − (σ·0 + μ), each operation rounded to float32 as the reference's broadcast does
__device__ __forceinline__ float wm_unscaled_minus_zero(float sig, float mu, float y) {
#pragma clang fp contract(off)
    return (sig * y + mu) - (sig * 0.0f + mu);
}

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

// the wave's span of one face output in 16-byte pieces (a last tile of c columns: 33 c floats, the odd ones singly); o is 16-byte aligned
#define WM_STORE_FACES_ALIGNED(o, img, cnt) \
                if (cnt > 0) { \
                    _Pragma("unroll") \
                    for (int i = 0; i < 5; i++) { \
                        const int p = 4 * (i * 64 + lane); \
                        if (p + 3 < cnt) *reinterpret_cast<f32x4*>(o + p) = *reinterpret_cast<const f32x4*>(img + p); \
                        else if (p < cnt) \
                            for (int t = p; t < cnt; t++) o[t] = img[t]; \
                    } \
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

    WM_OPERAND_BASES();

    f32x4 xr[3][4];
    int g = blockIdx.x;
    if (g < n_groups) wm_load_tile(src, (long long)(g * WM_WAVES + wave) * 32 + j, h, n_col, xr);
    for (; g < n_groups; g += gridDim.x) {
        const long long col0 = (long long)(g * WM_WAVES + wave) * 32, col = col0 + j;
#define WM_TILE_PREFETCH() \
        if (g + (int)gridDim.x < n_groups) wm_load_tile(src, (long long)((g + (int)gridDim.x) * WM_WAVES + wave) * 32 + j, h, n_col, xr)
#define WM_TILE_STORE_FACES(o, img, cnt) WM_STORE_FACES_ALIGNED(o, img, cnt)
#include "wm_infer_tile.inc"
#undef WM_TILE_PREFETCH
#undef WM_TILE_STORE_FACES
    }
}

// The ensemble form (engine_wm_infer.h: wm_ens_range): arrays carry a leading model index; the workgroup walks its contiguous items of the
// model-major list, holds ONE model's weight image at a time and re-copies it at a model boundary between two barriers — the first so that no
// wave still reads the old image, the second so that none reads the new one early.  The per-tile statements are wm_infer_kernel's
// (wm_infer_tile.inc); the d/dz arrays are written by all four instantiations.
template <bool FUSED, bool DIAG>
__global__ void __launch_bounds__(64 * WM_WAVES, 1)
wm_infer_ens_kernel(const float* __restrict__ w_all, size_t w_stride, WmScal S, const float* u_all, const float* v_all, const float* T_all,
                    const float* __restrict__ top, const float* __restrict__ hb_all, const float* __restrict__ ht_all,
                    const MppParams* __restrict__ Pm, float* __restrict__ dz_uw_all, float* __restrict__ dz_vw_all, float* __restrict__ dz_wT_all,
                    float* uo_all, float* vo_all, float* To_all, float* __restrict__ f_uw_all, float* __restrict__ f_vw_all,
                    float* __restrict__ f_wT_all, int n_col, int n_groups, int n_models) {
    constexpr bool DZ = true, RAW = FUSED || DIAG;
    extern __shared__ __attribute__((aligned(16))) float wm_smem[];
    float* wl = wm_smem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    float* const st = wm_smem + WM_W_LDS + wave * 3 * WM_FS;          // FUSED, DIAG: this wave's rows [3][32][33]
    WM_OPERAND_BASES();

    long long it, last;
    wm_ens_range((int)blockIdx.x, (int)gridDim.x, (long long)n_models * n_groups, &it, &last);
    if (it >= last) return;
    int m = (int)(it / n_groups), g = (int)(it % n_groups), loaded = -1;
    const size_t state_m = (size_t)n_col * WM_NZ, faces_m = (size_t)n_col * WM_LD, halo_m = (size_t)3 * n_col;
    f32x4 xr[3][4];
    {
        const float* const src0[3] = {u_all + m * state_m, v_all + m * state_m, T_all + m * state_m};
        wm_load_tile(src0, (long long)(g * WM_WAVES + wave) * 32 + j, h, n_col, xr);
    }
    MppParams P = Pm[m];
    for (; it < last; it++) {
        if (m != loaded) {                                            // (uniform over the workgroup: every wave walks the same items)
            if (loaded >= 0) __syncthreads();
            const float* w = w_all + m * w_stride;
            for (int i = threadIdx.x; i < WM_W_LDS; i += 64 * WM_WAVES) wl[i] = i < 3 * WM_NET ? w[i] : 0.0f;
            __syncthreads();
            loaded = m;
            P = Pm[m];                                                // the model's constants: once per model, not per column
        }
        float* const dzs[3] = {dz_uw_all + m * state_m, dz_vw_all + m * state_m, dz_wT_all + m * state_m};
        float* const fcs[3] = {DIAG ? f_uw_all + m * faces_m : nullptr, DIAG ? f_vw_all + m * faces_m : nullptr, DIAG ? f_wT_all + m * faces_m : nullptr};
        float* const uo = FUSED ? uo_all + m * state_m : nullptr;
        float* const vo = FUSED ? vo_all + m * state_m : nullptr;
        float* const To = FUSED ? To_all + m * state_m : nullptr;
        const float* const halo_bottom = hb_all ? hb_all + m * halo_m : nullptr;
        const float* const halo_top = ht_all ? ht_all + m * halo_m : nullptr;
        // the next item: the next group of this model, or the first group of the next one — whose state has its own base
        const int gn = g + 1 < n_groups ? g + 1 : 0, mn = g + 1 < n_groups ? m : m + 1;
        const long long col0 = (long long)(g * WM_WAVES + wave) * 32, col = col0 + j;
#define WM_TILE_PREFETCH() \
        if (it + 1 < last) { \
            const float* const srcn[3] = {u_all + mn * state_m, v_all + mn * state_m, T_all + mn * state_m}; \
            wm_load_tile(srcn, (long long)(gn * WM_WAVES + wave) * 32 + j, h, n_col, xr); \
        }
#define WM_TILE_STORE_FACES(o, img, cnt) WM_STORE_FACES_ANY(o, img, cnt)
#include "wm_infer_tile.inc"
#undef WM_TILE_PREFETCH
#undef WM_TILE_STORE_FACES
        g = gn;
        m = mn;
    }
}

// the scalings as the kernels take them (Args: WmInferArgs, WmEnsArgs)
template <class Args>
static WmScal wm_scal(const Args& a) {
    WmScal S;
    for (int f = 0; f < 3; f++) {
        S.mu[f] = a.mu[f];
        S.inv_sig[f] = 1.0f / a.sigma[f];
        S.fmu[f] = a.mu[3 + f];
        S.fsig[f] = a.sigma[3 + f];
    }
    S.inv_dz = (float)WM_NZ / a.io.Lz;
    S.dz = a.io.Lz / (float)WM_NZ;
    S.act1 = a.act1;
    S.act2 = a.act2;
    return S;
}
static hipError_t wm_cu_count(int* n_cu) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    return e != hipSuccess ? e : hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, dev);
}

hipError_t launch_wm_infer(const WmInferArgs& a, hipStream_t stream) {
    const WmEmbedIO& io = a.io;
    if (io.n_col < 1 || !(io.Lz > 0.0f)) return hipErrorInvalidValue;
    if (!wm_io_aligned(io, io.fused() || !io.diag())) return hipErrorInvalidValue;       // (the diagnosis alone writes no d/dz arrays)
    int n_cu = 0;
    hipError_t e = wm_cu_count(&n_cu);
    if (e != hipSuccess) return e;
    const WmScal S = wm_scal(a);
    const int n_tiles = (io.n_col + 31) / 32, n_groups = (n_tiles + WM_WAVES - 1) / WM_WAVES;
    with_bools([&](auto FUSED, auto DIAG) {
        auto* k = wm_infer_kernel<FUSED(), DIAG()>;
        const size_t lds = (WM_W_LDS + (FUSED() || DIAG() ? WM_WAVES * 3 * WM_FS : 0)) * sizeof(float);
        e = set_max_lds(k, lds);
        if (e != hipSuccess) return;
        // persistent: one workgroup per CU, one wave per SIMD with the whole register file (five stacked accumulator tiles, the input, the
        // prefetched next tile: two waves per SIMD spill)
        const int resident = std::max(1, n_cu);
        hipLaunchKernelGGL(k, dim3(std::min(n_groups, resident)), dim3(64 * WM_WAVES), lds, stream, a.weights, S, io.u, io.v, io.T, io.top_flux,
                           io.halo_bottom, io.halo_top, a.mpp, io.dz_uw, io.dz_vw, io.dz_wT, io.u_out, io.v_out, io.T_out, io.uw, io.vw, io.wT, io.n_col, n_groups);
        e = hipGetLastError();
    }, io.fused(), io.diag());
    return e;
}

hipError_t launch_wm_infer_ens(const WmEnsArgs& a, hipStream_t stream) {
    const WmEmbedIO& io = a.io;
    if (a.n_models < 1 || io.n_col < 1 || !(io.Lz > 0.0f) || !a.mpp) return hipErrorInvalidValue;
    if (!wm_io_aligned(io, true)) return hipErrorInvalidValue;
    int n_cu = 0;
    hipError_t e = wm_cu_count(&n_cu);
    if (e != hipSuccess) return e;
    const WmScal S = wm_scal(a);
    const int n_groups = wm_ens_groups(io.n_col), grid = wm_ens_grid(a.n_models, io.n_col, std::max(1, n_cu), a.grid_cap);
    with_bools([&](auto FUSED, auto DIAG) {
        auto* k = wm_infer_ens_kernel<FUSED(), DIAG()>;
        const size_t lds = (WM_W_LDS + (FUSED() || DIAG() ? WM_WAVES * 3 * WM_FS : 0)) * sizeof(float);
        e = set_max_lds(k, lds);
        if (e != hipSuccess) return;
        // persistent, one workgroup per CU as wm_infer_kernel (one wave per SIMD with the whole register file)
        hipLaunchKernelGGL(k, dim3(grid), dim3(64 * WM_WAVES), lds, stream, a.weights, a.w_stride, S, io.u, io.v, io.T, io.top_flux, io.halo_bottom, io.halo_top,
                           a.mpp, io.dz_uw, io.dz_vw, io.dz_wT, io.u_out, io.v_out, io.T_out, io.uw, io.vw, io.wT, io.n_col, n_groups, a.n_models);
        e = hipGetLastError();
    }, io.fused(), io.diag());
    return e;
}
