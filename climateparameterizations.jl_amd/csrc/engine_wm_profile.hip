// engine_wm_profile.hip — judging a wind-mixing sweep (gfx950 only): predict_flux and local_richardson on every saved state of every member of
// an ensemble in one launch — what NDE_profile (wind_mixing/src/training_postprocessing.jl:404-431, :474-495) loops over frame by frame.
//
// Layout.  engine_wm_infer.hip's: persistent workgroups of four waves, model k's flat Flux.destructure vector VERBATIM in LDS (78 KB), a model-major
// work list (wm_ens_range) with the weight image re-copied at every model boundary between two barriers.  One wavefront owns a tile of 32 consecutive
// STATES of one model in the 32x32 accumulator layout: state s = c n_save + n is row s of that model's sol [n_col][n_save][96] (384 bytes: every state
// is 16-byte aligned), levels 8 q + 4 h .. + 3 of a field are one 16-byte load of lane (j, h) straight into the B-operand layout.  The solution is in
// scaled units already: the loaded registers ARE the networks' input.  Lane j's simulation c = s / n_save selects its row of the shared bcs [n_col][6],
// its frame n = s % n_save the time of the diurnal top flux (rt_top_flux at save_times[n]); a tile may straddle simulations and frames.
// Networks.  wm_net_layer1.inc / wm_net_layer23.inc, the statements of the embedding's tile: stacked layer 1, 345 v_mfma_f32_32x32x2_f32 per tile,
// f32 under either matrix_arithmetic (colnde_describe: wm_profile=f32).
// Faces.  Row rho(r, h) of a layer-3 tile is interior face rho + 1, the upper face of level rho, which the same element of the state registers holds:
// the level differences are lane-local but for the level above every fourth one (lane ^ 32, one exchange per four levels and field, before the
// networks).  What the closure subtracts on the lane's 16 faces (nu dz u, nu dz v, nu / Pr dz T with eps = 1e-7 on the three gradients of the
// Richardson number; or kappa min(0, dz T); or nothing) waits in the wave's LDS rows [4][32][33] during the chains — no registers held across them —,
// each net's faces replace it there, and the wave's 32 states x 33 faces leave as one contiguous span of each output (WM_STORE_FACES_ANY: a model's
// rows are only 4-byte aligned).  Lane (j, 0) writes face 0, lane (j, 1)'s last element is face 32: the boundary fluxes (BC - scaling(0) under
// zero_weights with the closure, BC without, 0 under zero_weights without the closure), as predict_flux assembles them.
// Richardson number.  The fourth row: Bz / S2 WITHOUT eps (an IEEE division), stored before the chains so that it drains under them.  The two boundary
// faces are NaN, as in the reference (engine_wm_profile.h).
#include "engine_wm_profile.h"
#include "kernel_select.h"
#include "regtile_dev.h"               // rt_top_flux: the solver's own diurnal top flux
#include "wm_infer_dev.h"
#include <algorithm>
#include <climits>

#define WP_ROWS 4                      // a wave's face images: uw, vw, wT, Ri

struct WpScal { int act1, act2; };     // what the shared chains read through S

// 16-byte loads of one tile's states: xr[f][q] = levels 8 q + 4 h .. + 3 of field f of the lane's state (zeros past the last state)
__device__ __forceinline__ void wp_load_tile(const float* sol_m, int s, int h, int n_states, f32x4 (&xr)[3][4]) {
#pragma unroll
    for (int f = 0; f < 3; f++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
            if (s < n_states) z = *reinterpret_cast<const f32x4*>(sol_m + (size_t)s * 96 + 32 * f + 8 * q + 4 * h);
            xr[f][q] = z;
        }
}

// FLUX: uw, vw, wT (the networks run); RI: the Richardson number.  At least one.
template <bool FLUX, bool RI>
__global__ void __launch_bounds__(64 * WM_WAVES, 1)
wm_profile_ens_kernel(DevModel m, const float* __restrict__ w_all, size_t w_stride, const float* __restrict__ sol_all, const float* __restrict__ bcs,
                      const float* __restrict__ save_times, const RtPhys* __restrict__ phys, float* __restrict__ uw_all, float* __restrict__ vw_all,
                      float* __restrict__ wT_all, float* __restrict__ Ri_all, int n_states, int n_save, int n_groups, int n_models) {
    extern __shared__ __attribute__((aligned(16))) float wp_smem[];
    float* wl = wp_smem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    float* const st = wp_smem + WM_W_LDS + wave * WP_ROWS * WM_FS;      // this wave's rows [4][32][33]
    WM_OPERAND_BASES();
    (void)a1; (void)a2; (void)a3;
    const WpScal S = {m.acts[0], m.acts[1]};
    (void)S;

    long long it, last;
    wm_ens_range((int)blockIdx.x, (int)gridDim.x, (long long)n_models * n_groups, &it, &last);
    if (it >= last) return;
    int mi = (int)(it / n_groups), g = (int)(it % n_groups), loaded = -1;
    const size_t state_m = (size_t)n_states * 96, faces_m = (size_t)n_states * WM_LD;
    f32x4 xr[3][4];
    wp_load_tile(sol_all + mi * state_m, (g * WM_WAVES + wave) * 32 + j, h, n_states, xr);
    RtPhys P = phys[mi];
    const float Nz = (float)WM_NZ;
    for (; it < last; it++) {
        if (mi != loaded) {                                           // (uniform over the workgroup: every wave walks the same items)
            if (FLUX) {
                if (loaded >= 0) __syncthreads();
                const float* w = w_all + mi * w_stride;
                for (int i = threadIdx.x; i < WM_W_LDS; i += 64 * WM_WAVES) wl[i] = i < 3 * WM_NET ? w[i] : 0.0f;
                __syncthreads();
            }
            loaded = mi;
            P = phys[mi];                                             // the model's constants: once per model, not per state
        }
        // the next item: the next group of this model, or the first group of the next one — whose states have their own base
        const int gn = g + 1 < n_groups ? g + 1 : 0, mn = g + 1 < n_groups ? mi : mi + 1;
        const int s0 = (g * WM_WAVES + wave) * 32, s = s0 + j;
        const int cnt = max(0, min(32, n_states - s0)) * WM_LD;       // floats of this tile in each output
        // the networks' input in the B layout: xs[16 f + 4 q + r] = field f, level rho(4 q + r, h) — the solution as stored
        float xs[48];
#pragma unroll
        for (int f = 0; f < 3; f++)
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int r = 0; r < 4; r++) xs[16 * f + 4 * q + r] = xr[f][q][r];
        // the lane's simulation and frame: its boundary fluxes (h = 0: the bottom ones, h = 1: the top ones, wT's at the frame's time)
        float bnd[3];
        {
            const int sc = min(s, n_states - 1), c = sc / n_save, fr = sc - c * n_save;
            const float* bp = bcs + (size_t)c * 6;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float b = bp[2 * k + h];
                if (k == 2 && h == 1) b = rt_top_flux(m, b, save_times[fr]);
                bnd[k] = m.mpp ? (m.zero_w ? b - m.s0[k] : b) : (m.zero_w ? 0.0f : b);
            }
        }
        // the next tile's states, in flight under this tile's work (one wave per SIMD: nothing else hides the latency)
        if (it + 1 < last) wp_load_tile(sol_all + mn * state_m, (gn * WM_WAVES + wave) * 32 + j, h, n_states, xr);
        WM_WAVE_SYNC();                                               // (the previous tile's rows have been read out)
        {
            float up[3][4];                     // the level above levels 8 q + 4 h + 3: lane ^ 32's first of q (h = 0) or of q + 1 (h = 1)
#pragma unroll
            for (int f = 0; f < 3; f++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float mine = xs[16 * f + 4 * q], next = q < 3 ? xs[16 * f + 4 * q + 4] : 0.0f;
                    up[f][q] = __shfl_xor(h == 1 ? mine : next, 32);
                }
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const bool top = e == 15 && h == 1;                   // face 32: a zero row of D_face
                float gr[3];
#pragma unroll
                for (int f = 0; f < 3; f++) {
                    const float d = ((e & 3) < 3 ? xs[16 * f + e + 1] : up[f][e >> 2]) - xs[16 * f + e];
                    gr[f] = top ? 0.0f : d * Nz;
                }
                const int slot = j * WM_LD + WM_RHO0(e) + 4 * h + 1;
                if (RI) {
                    const float su = m.sig_u * gr[0], sv = m.sig_v * gr[1];
                    st[3 * WM_FS + slot] = (m.B * gr[2]) / (su * su + sv * sv);      // (face 32: 0 / 0)
                }
                if (FLUX) {
                    float D[3] = {0.0f, 0.0f, 0.0f};
                    if (m.mpp) {
                        const float su = m.sig_u * (gr[0] + m.eps), sv = m.sig_v * (gr[1] + m.eps);
                        const float ri = (m.B * (gr[2] + m.eps)) / (su * su + sv * sv);
                        const float th = dev_tanh((ri - P.Ric) * P.inv_dRi);
                        const float nu = P.nu0 + P.nu_minus * (1.0f - th) * 0.5f;
                        D[0] = m.cs[0] * nu * gr[0];
                        D[1] = m.cs[1] * nu * gr[1];
                        D[2] = m.cs[2] * (nu * P.inv_Pr) * gr[2];
                    } else if (m.ca) {
                        D[2] = m.cs[2] * m.kappa * fminf(0.0f, gr[2]);
                    }
#pragma unroll
                    for (int k = 0; k < 3; k++) st[k * WM_FS + slot] = D[k];
                }
            }
            if (h == 0) {                                             // face 0: finished here
                if (RI) st[3 * WM_FS + j * WM_LD] = __builtin_nanf("");
                if (FLUX)
#pragma unroll
                    for (int k = 0; k < 3; k++) st[k * WM_FS + j * WM_LD] = bnd[k];
            }
        }
        if (RI) {
            WM_WAVE_SYNC();
            float* o = Ri_all + mi * faces_m + (size_t)s0 * WM_LD;
            const float* img = st + 3 * WM_FS;
            WM_STORE_FACES_ANY(o, img, cnt);
        }
        if (FLUX) {
#include "wm_net_layer1.inc"
            float* const outs[3] = {uw_all, vw_all, wT_all};
#pragma unroll
            for (int n = 0; n < 3; n++) {
#include "wm_net_layer23.inc"
                // ---- the net's faces minus what waits in the rows (each lane its own slots); face 32: the top flux
                float* row = st + n * WM_FS + j * WM_LD + 4 * h + 1;
#pragma unroll
                for (int r = 0; r < 16; r++) row[WM_RHO0(r)] = r == 15 && h == 1 ? bnd[n] : y[r] - row[WM_RHO0(r)];
                WM_WAVE_SYNC();
                float* o = outs[n] + mi * faces_m + (size_t)s0 * WM_LD;
                const float* img = st + n * WM_FS;
                WM_STORE_FACES_ANY(o, img, cnt);
            }
        }
        g = gn;
        mi = mn;
    }
}

hipError_t launch_wm_profile_ens(const WmProfileArgs& a, hipStream_t stream) {
    const bool flux = a.uw != nullptr, ri = a.Ri != nullptr;
    if (a.n_models < 1 || a.n_col < 1 || a.n_save < 1 || !a.sol || !a.bcs || !a.save_times || !a.phys || (!flux && !ri)) return hipErrorInvalidValue;
    if (flux && (!a.weights || !a.vw || !a.wT)) return hipErrorInvalidValue;
    if ((long long)a.n_col * a.n_save > (long long)INT_MAX / 128) return hipErrorInvalidValue;      // state and face indices stay inside an int
    uintptr_t al = (uintptr_t)a.sol | (uintptr_t)a.Ri;
    if (flux) al |= (uintptr_t)a.uw | (uintptr_t)a.vw | (uintptr_t)a.wT;
    if (al & 15) return hipErrorInvalidValue;
    int dev = 0, n_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const int n_states = a.n_col * a.n_save;
    const int n_groups = wm_ens_groups(n_states), grid = wm_ens_grid(a.n_models, n_states, std::max(1, n_cu), a.grid_cap);
    with_bools([&](auto FLUX, auto RI) {
        if constexpr (FLUX() || RI()) {
            auto* k = wm_profile_ens_kernel<FLUX(), RI()>;
            const size_t lds = (WM_W_LDS + WM_WAVES * WP_ROWS * WM_FS) * sizeof(float);
            static bool raised[64] = {};                              // the dynamic-LDS limit of this instantiation: once per device
            if (dev < 0 || dev >= 64 || !raised[dev]) {
                e = set_max_lds(k, lds);
                if (e != hipSuccess) return;
                if (dev >= 0 && dev < 64) raised[dev] = true;
            }
            // persistent, one workgroup per CU as wm_infer_ens_kernel (one wave per SIMD with the whole register file)
            hipLaunchKernelGGL(k, dim3(grid), dim3(64 * WM_WAVES), lds, stream, a.m, a.weights, a.w_stride, a.sol, a.bcs, a.save_times, a.phys, a.uw, a.vw, a.wT,
                               a.Ri, n_states, a.n_save, n_groups, a.n_models);
            e = hipGetLastError();
        }
    }, flux, ri);
    return e;
}
