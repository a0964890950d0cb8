// engine_wm_embed_any.hip — the wind-mixing embedding for three flux networks of any layer sizes (96, h1, …, 31) and activations (gfx950 only;
// DESIGN §4t).  One launch computes, for one model, what wm_infer_ens_kernel (engine_wm_infer.hip) computes for the fixed 96-50-20-31 shape: the
// stored +∂z arrays of the state as given (NN_uw_forcing / NN_vw_forcing / NN_wT_forcing, wind_mixing/src/NDE_oceananigans.jl:288-329), optionally
// modified_pacanowski_philander! (:61-101) on that state and / or diagnose_NN_flux_uw / _vw / _wT (:226-286).
//
// Layout.  One workgroup of 8 waves per tile of 16 columns.  The tile's u, v, T are read ONCE, as 16-byte loads, into LDS: raw into the state rows
// st [3][16][33], scaled into the input rows xs [16][98].  Every later statement reads the state from LDS, so the barrier that follows the loads
// orders every read of the state before the first store and u_out, v_out, T_out may alias their inputs.
// Dense layers: v_mfma_f32_16x16x4_f32 with N = the 16 columns.  A job is a 16-row tile of a layer's output, dealt over the waves as in tile16's
// mlp_forward; the A operand of k-step s is W_l[(4 s + kq) no + i], read IN PLACE from the flat Flux.destructure vector in global memory (16
// consecutive floats per k: a wave's load is four 64-byte segments) — no pack launch, no cached image; the B operand is the activation row in LDS.
// Rows past `no` are clamped to the last row and never stored; the k-steps below ni / 4 are whole, the one after them loads W and the activation
// only where 4 s + kq < ni and zero elsewhere, so no address outside W_l is formed.  The nets are taken one after another and share one pair of
// activation buffers (engine_wm_embed_any.h: wm_any_plan); a net's last layer writes its own rows y [3][16][34].
// Step (FUSED): the last wave sweeps the state rows in place, one lane per column (mpp_sweep.h: mpp_column_step<32>, the function
// mpp_diffusion_kernel calls), and stores u′, v′, T′ as 16-byte pieces while the other seven waves run the dense chains; it takes no dense jobs.
// Faces (DIAG): ν ∂z u, ν ∂z v, νT ∂z T of the 33 faces (mpp_sweep.h: mpp_face_nu_grad) go to the rows g [3][16][33] BEFORE the step touches the
// state rows; after the nets each slot becomes F − ν ∂z φ and the rows, the image of the tile's contiguous 2,112-byte-aligned span of each output,
// leave as 16-byte pieces.
// One pipe under either matrix_arithmetic: f32 MFMA (colnde_describe: wm_embed=generic_f32).
#include "engine_wm_embed_any.h"
#include "colnde_dev.h"
#include "kernel_select.h"
#include <algorithm>

struct WmAnyScal { float mu[3], inv_sig[3], fmu[3], fsig[3], inv_dz, dz; };

__device__ __forceinline__ f32x4 wma_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// acc += Σ_{s<n} mfma(ap[s a_step], bp[4 s]): U k-steps' operands in flight ahead of their MFMAs (the A operand streams from L2), then a halved remainder.
// Measured on 3 x 96-400-400-31 at 18 columns (tools/wm_generic_rate.py): U = 16 one row tile per job 91 µs; two row tiles per job sharing the B operand
// (twice the loads in flight) 104 µs — the launch runs at what ONE CU fetches, not at a wave's load latency.
template <int U>
__device__ __forceinline__ f32x4 wma_chain(const float* __restrict__ ap, int a_step, const float* bp, int n, f32x4 acc) {
    int s = 0;
    for (; s + U <= n; s += U) {
        float a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            a[u] = ap[(s + u) * a_step];
            b[u] = bp[4 * (s + u)];
        }
#pragma unroll
        for (int u = 0; u < U; u++) acc = wma_mfma(a[u], b[u], acc);
    }
    if (U > 1) return s < n ? wma_chain<(U > 1 ? U / 2 : 1)>(ap + s * a_step, a_step, bp + 4 * s, n - s, acc) : acc;
    for (; s < n; s++) acc = wma_mfma(ap[s * a_step], bp[4 * s], acc);
    return acc;
}
#define WMA_U 16

// the staged rows of the step belong to ONE wave, whose LDS operations complete in order: only the compiler is held to the order
#define WMA_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// inv(scaling)(y) − inv(scaling)(0) = (σ y + μ) − (σ·0 + μ), each operation rounded to float32 as the reference's broadcast does
__device__ __forceinline__ float wma_unscaled_minus_zero(float sig, float mu, float y) {
#pragma clang fp contract(off)
    return (sig * y + mu) - (sig * 0.0f + mu);
}

// the flux on face f (0 … 32) of the forcing chain (:288-329 with enforce_fluxes, :220-224): [0; interior; top], the interior relative to its first
// element — for uw, vw with inv(scaling) applied a second time to the ALREADY unscaled first element, as the reference does (sic)
__device__ __forceinline__ float wma_forcing_face(int n, float sig, float mu, const float* y, int f, float top) {
#pragma clang fp contract(off)
    if (f == 0) return 0.0f;
    if (f == WMA_NZ) return top;
    const float y0 = y[0], yf = y[f - 1];
    if (n < 2) {
        const float a0 = sig * y0 + mu;
        const float ref = sig * a0 + mu;
        return (sig * yf + mu) - ref;
    }
    return sig * (yf - y0);
}

template <bool FUSED, bool DIAG>
__global__ void __launch_bounds__(64 * WMA_WAVES)
wm_embed_any_kernel(WmAnyNet N, WmAnyPlan L, const float* __restrict__ w, WmAnyScal S, const float* u, const float* v, const float* T,
                    const float* __restrict__ top, const float* __restrict__ halo_bottom, const float* __restrict__ halo_top, MppParams P,
                    float* __restrict__ dz_uw, float* __restrict__ dz_vw, float* __restrict__ dz_wT, float* uo, float* vo, float* To,
                    float* __restrict__ f_uw, float* __restrict__ f_vw, float* __restrict__ f_wT, int n_col) {
    extern __shared__ __attribute__((aligned(16))) float wma_smem[];
    float* const st = wma_smem + L.st;
    float* const gr = wma_smem + L.g;
    float* const xs = wma_smem + L.xs;
    float* const yb = wma_smem + L.y;
    constexpr int FS = WMA_CT * WMA_LD;                                // floats per field of the state rows and of the face rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long col0 = (long long)blockIdx.x * WMA_CT;
    const int ncol = (int)min((long long)WMA_CT, (long long)n_col - col0);   // >= 1: the grid is ceil(n_col / 16)

    // ---- the tile's state: 3 fields x 16 columns x 8 pieces of 16 bytes, one per thread; columns past n_col are zeros and are never read
    if (tid < 3 * WMA_CT * 8) {
        const int f = tid >> 7, c = (tid >> 3) & 15, q = tid & 7;
        const float* src = f == 0 ? u : (f == 1 ? v : T);
        f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        if (c < ncol) z = *reinterpret_cast<const f32x4*>(src + (size_t)(col0 + c) * WMA_NZ + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            st[f * FS + c * WMA_LD + 4 * q + r] = z[r];
            xs[c * WMA_LDX + WMA_NZ * f + 4 * q + r] = (z[r] - S.mu[f]) * S.inv_sig[f];
        }
    }
    __syncthreads();                                                   // every read of u, v, T lies before this barrier: the outputs may alias them

    if (DIAG) {
        // ---- ν ∂z u, ν ∂z v, νT ∂z T on the 33 faces of the state as given; the end faces from the halo cells or the zero-gradient fill
        for (int i = tid; i < WMA_CT * WMA_LD; i += 64 * WMA_WAVES) {
            const int c = i / WMA_LD, f = i - c * WMA_LD;
            if (c >= ncol) continue;
            const size_t col = (size_t)(col0 + c);
            float d[3], g[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float* row = st + k * FS + c * WMA_LD;
                if (f == 0) d[k] = halo_bottom ? row[0] - halo_bottom[(size_t)k * n_col + col] : 0.0f;
                else if (f == WMA_NZ) d[k] = (halo_top ? halo_top[(size_t)k * n_col + col] : row[WMA_NZ - 1]) - row[WMA_NZ - 1];
                else d[k] = row[f] - row[f - 1];
            }
            mpp_face_nu_grad(P, S.dz, f == 0 || f == WMA_NZ, d[0], d[1], d[2], g[0], g[1], g[2]);
#pragma unroll
            for (int k = 0; k < 3; k++) gr[k * FS + i] = g[k];
        }
        if (FUSED) __syncthreads();                                    // (the step overwrites the rows these differences were read from)
    }

    constexpr int DENSE_WAVES = FUSED ? WMA_WAVES - 1 : WMA_WAVES;
    if (FUSED && wave == WMA_WAVES - 1) {
        // ---- the implicit step, one lane per column, in place in the state rows; then u′, v′, T′ as 16-byte pieces
        if (lane < ncol) mpp_column_step<WMA_NZ>(P, st + lane * WMA_LD, st + FS + lane * WMA_LD, st + 2 * FS + lane * WMA_LD, halo_bottom, (size_t)(col0 + lane), n_col);
        WMA_WAVE_SYNC();
#pragma unroll
        for (int f = 0; f < 3; f++) {
            float* dst = f == 0 ? uo : (f == 1 ? vo : To);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int e = i * 64 + lane, c = e >> 3, k = (e & 7) * 4;
                if (c < ncol) {
                    const float* d = st + f * FS + c * WMA_LD + k;
                    const f32x4 o = {d[0], d[1], d[2], d[3]};
                    *reinterpret_cast<f32x4*>(dst + (size_t)(col0 + c) * WMA_NZ + k) = o;
                }
            }
        }
    }

    // ---- the three nets, one after another; a barrier closes every layer
    const int c = lane & 15, kq = lane >> 4;
    for (int n = 0; n < 3; n++) {
        const float* wn = w + (size_t)n * N.net_size;
        for (int l = 0; l < N.n_layers; l++) {
            const int ni = N.sizes[l], no = N.sizes[l + 1], act = N.acts[l];
            const int nmt = (no + 15) >> 4, nk = ni >> 2;
            const bool last = l + 1 == N.n_layers;
            const float* in = l == 0 ? xs + c * WMA_LDX : wma_smem + L.buf[(l - 1) & 1] + c * L.ld[(l - 1) & 1];
            float* out = last ? yb + (n * WMA_CT + c) * WMA_LDY : wma_smem + L.buf[l & 1] + c * L.ld[l & 1];
            const float* Wl = wn + N.w_off[l];
            const float* bl = wn + N.b_off[l];
            if (wave < DENSE_WAVES)
                for (int mt = wave; mt < nmt; mt += DENSE_WAVES) {
                    // the bias is fetched now and added after the chain, so that its load latency hides under the MFMAs
                    float bq[4];
#pragma unroll
                    for (int r = 0; r < 4; r++) bq[r] = bl[min(mt * 16 + 4 * kq + r, no - 1)];
                    const float* ap = Wl + kq * no + min(mt * 16 + c, no - 1);
                    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                    acc = wma_chain<WMA_U>(ap, 4 * no, in + kq, nk, acc);
                    if (4 * nk < ni) {                                 // the k-step that straddles ni: nothing is read at k >= ni
                        const int k = 4 * nk + kq;
                        const float a = k < ni ? ap[nk * 4 * no] : 0.0f, b = k < ni ? in[k] : 0.0f;
                        acc = wma_mfma(a, b, acc);
                    }
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int row = mt * 16 + 4 * kq + r;
                        if (row < no) out[row] = dev_act(act, acc[r] + bq[r]);
                    }
                }
            __syncthreads();
        }
    }

    // ---- the stored +∂z arrays: cell k of column c gets (F[k + 1] − F[k]) / Δz, one thread per cell
    {
        const int cc = tid >> 5, k = tid & 31;
        if (cc < ncol) {
            const size_t col = (size_t)(col0 + cc);
#pragma unroll
            for (int n = 0; n < 3; n++) {
                const float* y = yb + (n * WMA_CT + cc) * WMA_LDY;
                const float top_n = k == WMA_NZ - 1 ? top[(size_t)n * n_col + col] : 0.0f;
                const float hi = wma_forcing_face(n, S.fsig[n], S.fmu[n], y, k + 1, top_n), lo = wma_forcing_face(n, S.fsig[n], S.fmu[n], y, k, 0.0f);
                float* o = n == 0 ? dz_uw : (n == 1 ? dz_vw : dz_wT);
                o[col * WMA_NZ + k] = (hi - lo) * S.inv_dz;
            }
        }
    }
    if (DIAG) {
        // ---- the diagnosed total fluxes [0; inv(scaling).(y) .- inv(scaling)(0); top] − ν ∂z φ, each thread its own slots of the face rows
        for (int i = tid; i < WMA_CT * WMA_LD; i += 64 * WMA_WAVES) {
            const int cc = i / WMA_LD, f = i - cc * WMA_LD;
            if (cc >= ncol) continue;
            const size_t col = (size_t)(col0 + cc);
#pragma unroll
            for (int n = 0; n < 3; n++) {
                const float* y = yb + (n * WMA_CT + cc) * WMA_LDY;
                const float Fd = f == 0 ? 0.0f : (f == WMA_NZ ? top[(size_t)n * n_col + col] : wma_unscaled_minus_zero(S.fsig[n], S.fmu[n], y[f - 1]));
                gr[n * FS + i] = Fd - gr[n * FS + i];
            }
        }
        __syncthreads();
        const int cnt = ncol * WMA_LD;
#pragma unroll
        for (int n = 0; n < 3; n++) {
            float* o = (n == 0 ? f_uw : (n == 1 ? f_vw : f_wT)) + (size_t)col0 * WMA_LD;      // 16 x 33 floats per tile: 16-byte aligned
            const float* img = gr + n * FS;
            const int p = 4 * tid;
            if (p + 3 < cnt) *reinterpret_cast<f32x4*>(o + p) = *reinterpret_cast<const f32x4*>(img + p);
            else
                for (int t = p; t < cnt; t++) o[t] = img[t];
        }
    }
}

hipError_t launch_wm_embed_any(const WmAnyArgs& a, hipStream_t stream) {
    const WmEmbedIO& io = a.io;
    if (io.n_col < 1 || !(io.Lz > 0.0f)) return hipErrorInvalidValue;
    const WmAnyNet& N = a.net;
    if (N.n_layers < 1 || N.n_layers > WMA_MAX_LAYERS || N.sizes[0] != 3 * WMA_NZ || N.sizes[N.n_layers] != WMA_NZ - 1) return hipErrorInvalidValue;
    if (!wm_io_aligned(io, true)) return hipErrorInvalidValue;
    const WmAnyPlan L = wm_any_plan(N.n_layers, N.sizes);
    if (!wm_any_fits(L)) return hipErrorInvalidValue;
    WmAnyScal S;
    for (int f = 0; f < 3; f++) {
        S.mu[f] = a.mu[f];
        S.inv_sig[f] = 1.0f / a.sigma[f];
        S.fmu[f] = a.mu[3 + f];
        S.fsig[f] = a.sigma[3 + f];
    }
    S.inv_dz = (float)WMA_NZ / io.Lz;
    S.dz = io.Lz / (float)WMA_NZ;
    const int n_tiles = (io.n_col + WMA_CT - 1) / WMA_CT;
    hipError_t e = hipSuccess;
    with_bools([&](auto FUSED, auto DIAG) {
        auto* k = wm_embed_any_kernel<FUSED(), DIAG()>;
        e = set_max_lds(k, L.bytes);
        if (e != hipSuccess) return;
        hipLaunchKernelGGL(k, dim3(n_tiles), dim3(64 * WMA_WAVES), L.bytes, stream, N, L, a.weights, S, io.u, io.v, io.T, io.top_flux, io.halo_bottom, io.halo_top,
                           a.mpp, io.dz_uw, io.dz_vw, io.dz_wT, io.u_out, io.v_out, io.T_out, io.uw, io.vw, io.wT, io.n_col);
        e = hipGetLastError();
    }, io.fused(), io.diag());
    return e;
}
