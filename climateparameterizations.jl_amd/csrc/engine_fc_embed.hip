// engine_fc_embed.hip — the free-convection embedded step on fc32's sections (gfx950 only).
//
// What the reference runs per iteration of its free-convection embeddings (free_convection/src/oceananigans_nn.jl:153-165, over 96 x 96
// columns in free_convection/double_gyre_nn.jl:211-234) and writes out with every saved state (diagnose_wT_NN, oceananigans_nn.jl:100-118),
// per column, T [Nz] as given (k = 0 deepest), dz = Lz/Nz, c = dt/dz²:
//   1. forcing (:159-160, :120-126):  y = NN((T̃ − μ_T)/σ_T) (fc_infer_kernel's arithmetic, fc_chain.h), faces F = [0; σ_wT y + μ_wT; top_flux],
//      stored ∂z_wT_NN[k] = (F[k+1] − F[k])/dz — of T BEFORE the adjustment;
//   2. convective_adjustment!(model, Δt, K) (:162, :13-40): κ_k = K where the centred ∂T/∂z of cell k is negative, T′ = L \ T
//      (convadj_kernel's sweep, convadj_sweep.inc);
//   3. diagnose_wT_NN (:100-118): g_f = ∂T/∂z on the Nz + 1 faces (:107; the end faces from the halo cells), κ_f = g_f < 0 ? K : 0 (:110-113),
//      wT_faces = F − κ_f g_f (:115-117).  NaN < 0 is false, as in Julia.
//
// One kernel family, fce_kernel<NZ, CW, STEP, DIAG>: (STEP, !DIAG) = 1 + 2, (STEP, DIAG) = 1 + 2 + 3, (!STEP, DIAG) = 3 alone.  It is
// fc_infer_kernel with two things added around the SAME MFMA chains (fc_infer_chain.inc: the ∂z wT bits are fc_infer_kernel's):
//  * the tile's raw T rows are staged in LDS beside the scaled ones, in A2's rows, which nothing touches until layer 2's epilogues.  From them
//    one lane per column runs the Thomas sweep on a second copy of the rows, all threads form their κ_f g_f (kept in registers: OWN floats), and
//    T′ leaves as coalesced 16-byte stores BEFORE the chains start, so the stores drain under the MFMAs (the order DESIGN §4h describes);
//  * a workgroup has read all of its tile's T before it writes any T′, and tiles are disjoint: T_out may be T.
// LDS: fc_infer_kernel's carve + the two halo cells per column (256 B at most): 76 KB per workgroup at Nz = 64 on 32 columns, two fit a CU's 160 KB.
// Which launches the C entry points issue was decided by measurement (profiles/fc_embed_rate.json): the diagnosis-only and the
// three-output kernels always; forcing + adjustment alone runs as the two existing launches unless COLNDE_FC_EMBED_FUSED=1 (api_embed.hip).
// A second family, fce_ens_kernel<NZ, STEP, DIAG, CONV>, runs the K members of an ensemble in one launch (colnde_ensemble_fc_embedded):
// 16-column tiles, the model in blockIdx.y, the same per-tile text (fc_embed_body.inc), and — CONV — the --conv filter where the scaled rows go to LDS.
#include <algorithm>
#include "engine_fc_embed.h"
#include "engine_fc.h"
#include "kernel_select.h"
#include "fc_chain.h"

extern __shared__ float fce_smem[];

// Two workgroups per CU, as fc_infer_kernel — except (Nz = 64, 32 columns, with the sweep): the sweep's 3 x 64 live floats beside the tile's own state
// do not fit 256 registers (88 bytes of scratch under that bound), so this one shape takes the whole register file, one workgroup per CU.
template <int NZ, int CW, bool STEP> constexpr int fce_min_blocks() { return STEP && NZ == 64 && CW == 32 ? 1 : 2; }

template <int NZ, int CW, bool STEP, bool DIAG>
__global__ void __launch_bounds__(256, (fce_min_blocks<NZ, CW, STEP>()))
fce_kernel(const float* __restrict__ imgf, const float* __restrict__ bias, const float* T, const float* __restrict__ top_flux,
           const float* __restrict__ halo_bottom, const float* __restrict__ halo_top, float mu_T, float inv_sig_T, float sig_wT, float mu_wT,
           float inv_dz_out /* −Nz/Lz: fc_infer_kernel's argument for +∂z wT */, float inv_dz, float c, float K, float* __restrict__ dz_wT, float* T_out,
           float* __restrict__ faces, int n_col) {
    constexpr bool CONV = false;
    const float* const conv_taps = nullptr;
    const int conv_c = 0;
#include "fc_embed_body.inc"
}

// The K members of an ensemble in one launch (colnde_ensemble_fc_embedded): 16-column tiles, blockIdx.y = model, as the fc ensembles'
// kernels (engine_fc.h).  What a member owns — operand image, biases, filter, state, halos, outputs — lies at the strides of `en` from model 0's;
// the top flux is shared.  The offsets are scalar arithmetic on kernel arguments, once, here; the per-tile text is fce_kernel's.
// CONV: members with the --conv filter (taps [FC_CONV_MAX + 1] per model as fce_taps_kernel lays them out).
template <int NZ, bool STEP, bool DIAG, bool CONV>
__global__ void __launch_bounds__(256, 2)
fce_ens_kernel(const float* __restrict__ imgf, const float* __restrict__ bias, const float* T, const float* __restrict__ top_flux,
               const float* __restrict__ halo_bottom, const float* __restrict__ halo_top, float mu_T, float inv_sig_T, float sig_wT, float mu_wT,
               float inv_dz_out, float inv_dz, float c, float K, float* __restrict__ dz_wT, float* T_out, float* __restrict__ faces, int n_col,
               FceEns en, const float* __restrict__ conv_taps, int conv_c) {
    constexpr int CW = 16;
    {
        const size_t k = blockIdx.y;
        imgf += k * en.img;
        bias += k * en.bias;
        T += k * en.state;
        if (halo_bottom) halo_bottom += k * en.halo;
        if (halo_top) halo_top += k * en.halo;
        if constexpr (STEP) {
            dz_wT += k * en.state;
            T_out += k * en.state;
        }
        if constexpr (DIAG) faces += k * en.faces;
        if constexpr (CONV) conv_taps += k * (FC_CONV_MAX + 1);
    }
#include "fc_embed_body.inc"
}

// the filter of every member from the head of its parameter vector (w_stride floats apart) into the kernel's order: taps[d] = w[c - 1 - d], the tap
// that multiplies x[i + d] (NNlib's conv flips the kernel), zero beyond the filter; taps[FC_CONV_MAX] = b
__global__ void fce_taps_kernel(const float* __restrict__ w, size_t w_stride, int c, float* __restrict__ taps) {
    const int d = threadIdx.x;
    const float* wk = w + (size_t)blockIdx.x * w_stride;
    if (d <= FC_CONV_MAX) taps[(size_t)blockIdx.x * (FC_CONV_MAX + 1) + d] = d == FC_CONV_MAX ? wk[c] : (d < c ? wk[c - 1 - d] : 0.0f);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
template <int NZ, int CW> static size_t fce_lds() {
    return (size_t)(CW * Fc<NZ, CW>::LDX + 2 * CW * Fc<NZ, CW>::LDH + Fc<NZ, CW>::BIAS + 2 * CW) * sizeof(float);
}

// THE selector of the family: f(Nz, cw, step, diag, kernel, dynamic LDS bytes) for every instantiation.  fce_set_kernel_attributes raises the
// LDS limit of each; launch_fc_embed launches the one whose key matches — a kernel that can be launched has had its limit raised.
template <class F>
static void fce_for_each_kernel(F&& f) {
    auto shape = [&](auto N, auto W) {
        f(N(), W(), true, false, fce_kernel<N(), W(), true, false>, fce_lds<N(), W()>());
        f(N(), W(), false, true, fce_kernel<N(), W(), false, true>, fce_lds<N(), W()>());
        f(N(), W(), true, true, fce_kernel<N(), W(), true, true>, fce_lds<N(), W()>());
    };
    shape(std::integral_constant<int, 64>{}, std::integral_constant<int, 32>{});
    shape(std::integral_constant<int, 32>{}, std::integral_constant<int, 32>{});
    shape(std::integral_constant<int, 64>{}, std::integral_constant<int, 16>{});
    shape(std::integral_constant<int, 32>{}, std::integral_constant<int, 16>{});
}

// ... and its sibling for the ensemble family: f(Nz, step, diag, conv, kernel, dynamic LDS bytes), 16-column tiles
template <class F>
static void fce_ens_for_each_kernel(F&& f) {
    auto shape = [&](auto N, auto C) {
        f(N(), true, false, C(), fce_ens_kernel<N(), true, false, C()>, fce_lds<N(), 16>());
        f(N(), false, true, C(), fce_ens_kernel<N(), false, true, C()>, fce_lds<N(), 16>());
        f(N(), true, true, C(), fce_ens_kernel<N(), true, true, C()>, fce_lds<N(), 16>());
    };
    shape(std::integral_constant<int, 64>{}, std::false_type{});
    shape(std::integral_constant<int, 32>{}, std::false_type{});
    shape(std::integral_constant<int, 64>{}, std::true_type{});
    shape(std::integral_constant<int, 32>{}, std::true_type{});
}

hipError_t fce_set_kernel_attributes() {
    hipError_t e = hipSuccess;
    fce_for_each_kernel([&](int, int, bool, bool, auto* k, size_t lds) {
        if (e == hipSuccess) e = set_max_lds(k, lds);
    });
    fce_ens_for_each_kernel([&](int, bool, bool, bool, auto* k, size_t lds) {
        if (e == hipSuccess) e = set_max_lds(k, lds);
    });
    return e;
}

hipError_t launch_fc_embed(const DevModel& m, const FcEmbedArgs& a, hipStream_t stream) {
    if (a.n_col < 1 || !(a.Lz > 0.0f) || !a.imgf || !a.bias || !a.T || !a.top_flux) return hipErrorInvalidValue;
    const bool diag = a.wT_faces != nullptr;
    if (!a.step && !diag) return hipErrorInvalidValue;
    if (a.step && (!a.dz_wT || !a.T_out || !(a.dt > 0.0f))) return hipErrorInvalidValue;
    uintptr_t al = (uintptr_t)a.T | (uintptr_t)a.wT_faces;
    if (a.step) al |= (uintptr_t)a.dz_wT | (uintptr_t)a.T_out;
    if (al & 15) return hipErrorInvalidValue;
    const int n_tiles = (a.n_col + a.cw - 1) / a.cw;
    const dim3 grid(std::min(n_tiles, 512)), block(256);                         // two workgroups per CU, each walking over its tiles (fc_launch_infer)
    const float dz = a.Lz / (float)m.Nz;
    const float c = a.step ? a.dt / (dz * dz) : 0.0f;                            // colnde_convective_adjustment's dt/dz²
    const float inv_dz = (float)m.Nz / a.Lz;
    bool launched = false;
    fce_for_each_kernel([&](int Nz, int cw, bool step, bool dg, auto* k, size_t lds) {
        if (launched || Nz != m.Nz || cw != a.cw || step != a.step || dg != diag) return;
        hipLaunchKernelGGL(k, grid, block, lds, stream, a.imgf, a.bias, a.T, a.top_flux, a.halo_bottom, a.halo_top, m.mu_T, 1.0f / m.sig_T, m.sig_wT, m.mu_wT,
                           -1.0f * (float)m.Nz / a.Lz, inv_dz, c, a.K, a.dz_wT, a.T_out, a.wT_faces, a.n_col);
        launched = true;
    });
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

// All members in one launch: tiles along x, the model in grid.y.  The grid's x is capped as the single-model launch's, so a member's workgroups
// walk over its tiles with the operand ring streaming from one tile to the next.
hipError_t launch_fc_embed_ens(const DevModel& m, const FcEmbedArgs& a, int n_models, int conv, const float* taps, hipStream_t stream) {
    if (a.n_col < 1 || !(a.Lz > 0.0f) || !a.imgf || !a.bias || !a.T || !a.top_flux || a.cw != 16) return hipErrorInvalidValue;
    if (n_models < 1 || n_models > 65535) return hipErrorInvalidValue;
    if (conv && (conv < 2 || conv > FC_CONV_MAX || !taps)) return hipErrorInvalidValue;
    const bool diag = a.wT_faces != nullptr;
    if (!a.step && !diag) return hipErrorInvalidValue;
    if (a.step && (!a.dz_wT || !a.T_out || !(a.dt > 0.0f))) return hipErrorInvalidValue;
    uintptr_t al = (uintptr_t)a.T | (uintptr_t)a.wT_faces;
    if (a.step) al |= (uintptr_t)a.dz_wT | (uintptr_t)a.T_out;
    if (al & 15) return hipErrorInvalidValue;
    const int n_tiles = (a.n_col + 15) / 16;
    const dim3 grid(std::min(n_tiles, 512), n_models), block(256);
    const float dz = a.Lz / (float)m.Nz;
    const float c = a.step ? a.dt / (dz * dz) : 0.0f;
    const float inv_dz = (float)m.Nz / a.Lz;
    FceEns en;
    en.img = fc_image_floats(m.Nz);
    en.bias = fc_bias_floats(m.Nz);
    en.state = (size_t)a.n_col * m.Nz;
    en.halo = (size_t)a.n_col;
    en.faces = (size_t)a.n_col * (m.Nz + 1);
    bool launched = false;
    fce_ens_for_each_kernel([&](int Nz, bool step, bool dg, bool cv, auto* k, size_t lds) {
        if (launched || Nz != m.Nz || step != a.step || dg != diag || cv != (conv != 0)) return;
        hipLaunchKernelGGL(k, grid, block, lds, stream, a.imgf, a.bias, a.T, a.top_flux, a.halo_bottom, a.halo_top, m.mu_T, 1.0f / m.sig_T, m.sig_wT, m.mu_wT,
                           -1.0f * (float)m.Nz / a.Lz, inv_dz, c, a.K, a.dz_wT, a.T_out, a.wT_faces, a.n_col, en, taps, conv);
        launched = true;
    });
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_fce_taps(const float* w, size_t w_stride, int conv, int n_models, float* taps, hipStream_t stream) {
    if (!w || !taps || conv < 2 || conv > FC_CONV_MAX || n_models < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fce_taps_kernel, dim3(n_models), dim3(64), 0, stream, w, w_stride, conv, taps);
    return hipGetLastError();
}
