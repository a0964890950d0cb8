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
    static_assert(STEP || DIAG, "nothing to do");
    using S = Fc<NZ, CW>;
    constexpr int LDT = NZ + 1;                                  // raw rows: odd stride, conflict-free per-lane column walks (as convadj_kernel)
    static_assert(2 * CW * LDT <= CW * S::LDH, "the raw and the adjusted rows live in A2's rows");
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & (CW - 1), h = lane / CW;               // column of the tile; k / row quad
    float* X = fce_smem;
    float* A1 = X + CW * S::LDX;
    float* A2 = A1 + CW * S::LDH;
    float* PART = A1;
    float* BL = A2 + CW * S::LDH;
    float* HB = BL + S::BIAS;                                    // [CW] halo cell below k = 0 (absent: T[0])
    float* HT = HB + CW;                                         // [CW] halo cell above k = NZ - 1 (absent: T[NZ-1])
    float* TR = A2;                                              // [CW][LDT] T as given
    float* TS = A2 + CW * LDT;                                   // [CW][LDT] a second copy, solved in place: T′
    for (int q = tid; q < S::BIAS; q += 256) BL[q] = bias[q];
    FC_OWNER_INDEX();
    const f32x4* base[3];
    base[0] = reinterpret_cast<const f32x4*>(imgf + S::F1) + (w * S::S_IN) * 64;
    base[1] = reinterpret_cast<const f32x4*>(imgf + S::F2) + (w * S::S_H) * 64;
    base[2] = reinterpret_cast<const f32x4*>(imgf + S::F3) + ((w % S::MT3) * S::S_H + (w / S::MT3) * S::G3) * 64;
    // The A-operand ring streams from one tile to the next, as in fc_infer_kernel — except (Nz = 64, 16 columns, with the sweep): the sweep's 3 x 64
    // live floats and the ring's 32 registers do not fit 256 registers together (36 bytes of scratch), so there the ring is refilled after the sweep
    // of every tile (what the last groups of the previous tile prefetched is dropped: the L2 latency shows once per tile, under the other workgroup).
    constexpr bool REFILL = STEP && NZ == 64 && CW == 16;
    f32x4 ring[FC_PF];
    if constexpr (!REFILL) {
#pragma unroll
        for (int q = 0; q < FC_PF; q++) ring[q] = (base[fc_sec<NZ, CW>(q)] + fc_off<NZ, CW>(q))[lane];
    }
    const float b3v = oi < S::NO ? bias[2 * S::H + oi] : 0.0f;
    asm volatile("" :: "v"(b3v));
    const int n_tiles = (n_col + CW - 1) / CW;
#pragma nounroll
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int zero = 0;
        FC_OPAQUE_ZERO(zero);
        const f32x4* const sb[3] = {base[0] + zero, base[1] + zero, base[2] + zero};
        const int col0 = tile * CW;
        // ---- the tile's T: scaled rows (layer 1's B operand), raw rows, halo cells.  A partial tile repeats its last column.
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            const int col = min(col0 + oc[r], n_col - 1);
            const float t = T[(size_t)col * NZ + oi];
            X[oc[r] * S::LDX + oi] = fc_infer_scale(t, mu_T, inv_sig_T);
            TR[oc[r] * LDT + oi] = t;
            if constexpr (STEP) TS[oc[r] * LDT + oi] = t;
            if (oi == 0) HB[oc[r]] = halo_bottom ? halo_bottom[col] : t;
            if (oi == NZ - 1) HT[oc[r]] = halo_top ? halo_top[col] : t;
        }
        FC_BARRIER();
        // ---- convective_adjustment! (:13-40): one lane per column, then T′ out in 16-byte pieces before the chains start
        if constexpr (STEP) {
            if (w == 0 && lane < CW) {
                float* t = TS + lane * LDT;
                const float *halo_bottom = HB, *halo_top = HT;   // (never null here: the load above resolved an absent halo to the interior value)
                const int ca_i = lane;
#include "convadj_sweep.inc"
            }
            FC_BARRIER();
            constexpr int Q = NZ / 4;
#pragma unroll
            for (int e0 = 0; e0 < CW * Q; e0 += 256) {
                const int e = e0 + tid, cl = e / Q, k = (e % Q) * 4;
                if (e < CW * Q) {
                    const float* d = TS + cl * LDT + k;
                    const f32x4 q = {d[0], d[1], d[2], d[3]};
                    if (col0 + cl < n_col) *reinterpret_cast<f32x4*>(T_out + (size_t)(col0 + cl) * NZ + k) = q;
                }
            }
        }
        float tf[S::OWN];
        // ---- diagnose_wT_NN's κ_f ∂T/∂z (:107-115) of this thread's faces oi + 1 (kept for the end) and, oi = 0, face 0 (F[0] = 0: stored now)
        float kg[S::OWN];
        if constexpr (DIAG) {
#pragma unroll
            for (int r = 0; r < S::OWN; r++) {
                const int c = oc[r];
                const float tc = TR[c * LDT + oi];
                const float inside = TR[c * LDT + oi + 1];       // (oi = NZ - 1: the pad float of the row, not used)
                const float up = oi == NZ - 1 ? HT[c] : inside;
                const float g = (up - tc) * inv_dz;
                kg[r] = (g < 0.0f ? K : 0.0f) * g;
                if (oi == 0 && col0 + c < n_col) {
                    const float g0 = (tc - HB[c]) * inv_dz;
                    faces[(size_t)(col0 + c) * (NZ + 1)] = 0.0f - (g0 < 0.0f ? K : 0.0f) * g0;
                }
            }
        }
        // (loaded here, not with T: nothing but the sweep's own registers is live across it)
#pragma unroll
        for (int r = 0; r < S::OWN; r++) tf[r] = top_flux[min(col0 + oc[r], n_col - 1)];
        if constexpr (REFILL) {
#pragma unroll
            for (int q = 0; q < FC_PF; q++) ring[q] = (sb[fc_sec<NZ, CW>(q)] + fc_off<NZ, CW>(q))[lane];
        }
        // ---- the network (layer 2's epilogues overwrite TR and TS: every wave is past the barrier after layer 1 by then)
#include "fc_infer_chain.inc"
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            float lo, hi;
            fc_infer_faces<NZ, CW>(PART, oc[r], oi, b3v, sig_wT, mu_wT, tf[r], lo, hi);
            if (col0 + oc[r] < n_col) {
                if constexpr (STEP) dz_wT[(size_t)(col0 + oc[r]) * NZ + oi] = -(hi - lo) * inv_dz_out;
                if constexpr (DIAG) faces[(size_t)(col0 + oc[r]) * (NZ + 1) + oi + 1] = hi - kg[r];
            }
        }
        FC_BARRIER();                                                               // PART (= A1's rows), X, TR are rewritten by the next tile
    }
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

hipError_t fce_set_kernel_attributes() {
    hipError_t e = hipSuccess;
    fce_for_each_kernel([&](int, int, bool, bool, auto* k, size_t lds) {
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
