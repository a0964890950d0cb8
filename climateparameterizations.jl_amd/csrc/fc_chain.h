// fc_chain.h — device code shared by the fc32 kernels (engine_fc.hip) and the free-convection embedded step (engine_fc_embed.hip): the tile
// geometry Fc<NZ, CW>, the A-operand ring and its MFMA sections, and — with the three dense layers of fc_infer_chain.inc — the network
// evaluation of compute_neural_network_forcing! (free_convection/double_gyre_nn.jl:149-168) from the scaled input rows to the flux faces.  One
// definition, so that both kernels issue the same MFMA sequence and round the same way: their ∂z wT agree bit for bit.
#pragma once
#include "colnde_dev.h"
#include "engine_fc.h"                             // FC_CONV_MAX

typedef float fc16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32;

#ifndef FC_PF
#define FC_PF 8                                    // ring depth in groups of four MFMAs: 8 x 256 cycles of cover
#endif
// tape traffic: the default cache policy.  (Non-temporal was measured SLOWER: an nt store is acknowledged late, and every wait for a ring load — vmcnt
// is in order — waits behind it; figures in profiles/README.md)
#define FC_STORE(v, p) (*(p) = (v))
#define FC_LOAD(p) (*(p))
#define FC_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// The group addresses of a stage are loop-invariant: left alone, the optimiser computes all ~100 of them once, outside the time loop, and
// keeps them in (spilled) registers.  An opaque zero added to the wave-uniform bases at the top of every stage keeps them what they should
// be: a scalar base, a compile-time offset and the lane.  (The pointers themselves stay kernel-argument-derived: laundering THEM loses the global
// address space and turns every load into a flat_load, which counts against lgkmcnt as well.)
#define FC_OPAQUE_ZERO(z) asm volatile("" : "+s"(z))

// CW = columns per workgroup tile = N of the MFMA: 32 (v_mfma_f32_32x32x2_f32, the throughput shape) or 16 (v_mfma_f32_16x16x4_f32: half the
// matrix work per stage for problems that cannot fill 32-column tiles on every CU — the latency sizes, up to 4,096 columns).  Everything else is the
// same code: lane = (column n = lane % CW, k/row quad hq = lane / CW); a group is four MFMAs over KG = 256/CW consecutive k; an accumulator holds
// NQ = CW²/256 quads of four consecutive output rows: rows 8q + 4hq + e (CW = 32) or 4hq + e (CW = 16) of the row tile, column n.
template <int NZ, int CW = 32>
struct Fc {
    static_assert(CW == 32 || CW == 16, "tile width");
    static constexpr int H = 4 * NZ, NO = NZ - 1;
    static constexpr int LDX = NZ + 4, LDH = H + 4;              // LDS row strides: 16-byte aligned rows, stride/4 odd => conflict-free ds_read_b128
    static constexpr int KG = 256 / CW, NQ = CW * CW / 256, ACCN = 4 * NQ;   // k per group; accumulator quads (4 / 1); accumulator floats
    static constexpr int MT = H / CW, JH = MT / 4;               // row tiles of a hidden layer; jobs per wave
    static constexpr int S_IN = NZ / KG, S_H = H / KG;           // groups per chain: K = NZ, K = 4 NZ
    static constexpr int MT3 = NZ / CW, KS3 = MT3 >= 4 ? 1 : 4 / MT3, G3 = S_H / KS3;   // narrow layer (M = NZ): row tiles, K splits, groups per job
    static_assert(MT3 * KS3 == 4 && JH >= 1, "four jobs of the narrow layer, one per wave");
    static constexpr int F1 = 0, F1_SZ = MT * S_IN * 256;
    static constexpr int F2 = F1 + F1_SZ, F2_SZ = MT * S_H * 256;
    static constexpr int F3 = F2 + F2_SZ, F3_SZ = MT3 * S_H * 256;
    static constexpr int IMG = F3 + F3_SZ;                       // floats per operand image (forward and backward alike)
    static constexpr int BIAS = 2 * H + NZ;
    static constexpr int P = JH * S_IN + JH * S_H + G3;          // groups per stage and wave
    static constexpr int ACT4 = 2 * H + NZ;                      // dwtape_act4: (2H + NZ - 1) rounded up to 4
    static constexpr int R = NZ + 2 * ACT4;                      // floats per column of a delta-tape record (dwtape_row_floats)
    static constexpr int OWN = CW * NZ / 256;                    // state items (column, level) per thread
    static_assert(P % FC_PF == 0, "the ring must close over one stage");
    // ---- COLNDE_MATRIX_BF16X3_EXACT on the 16-column tiles (round 4; the 32-column tiles have their own kernels, engine_fc_split.hip): the same sections
    // on v_mfma_f32_16x16x32_bf16 from exact three-way operand splits (split_bf16.h).  The A operand is pre-split: per (16-row tile, 32-deep k-block) three
    // planes (h, m, l) of [64 lanes][8 bf16], lane (m = lane % 16, kq = lane / 16) holding k = 32 kb + 8 kq + i.  A wave's stream is contiguous per
    // section, k-block outer, its row tiles (jobs) inner, planes innermost: the B operand (8 consecutive floats of the column's activation row, split
    // in registers: 44 vector instructions) is shared by the wave's jobs.  Unit below: one SLOT = one plane fragment (64 lanes x 16 bytes).
    static constexpr int KB_IN = NZ / 32, KB_H = H / 32, KB3 = KB_H / KS3;          // k-blocks per chain: K = NZ, K = 4 NZ, the narrow layer's K part
    static constexpr int SF1 = 0, SF1_SZ = MT * KB_IN * 3 * 256;                    // u32 words
    static constexpr int SF2 = SF1 + SF1_SZ, SF2_SZ = MT * KB_H * 3 * 256;
    static constexpr int SF3 = SF2 + SF2_SZ, SF3_SZ = MT3 * KB_H * 3 * 256;
    static constexpr int SIMG = SF3 + SF3_SZ;                                       // words per split operand image (1.5 x IMG: engine_fc_split's size)
    static constexpr int PS0 = JH * 3 * KB_IN, PS1 = JH * 3 * KB_H, PS2 = 3 * KB3, PS = PS0 + PS1 + PS2;   // slots per stage and wave
    static constexpr int PFS = 12;                                                  // ring depth in slots
    static_assert(CW != 16 || (PS % PFS == 0 && KB_IN >= 1), "the split ring must close over one stage");
    typedef float acc_t __attribute__((ext_vector_type(ACCN)));
    // first row (within the row tile) of accumulator quad q for this lane's hq
    __device__ static constexpr int qrow(int q, int hq) { return (CW == 32 ? 8 * q : 0) + 4 * hq; }
};

// stream position -> layer section (0: K = NZ hidden, 1: K = 4NZ hidden, 2: the narrow layer) and offset in float4 units from the wave's base
template <int NZ, int CW> __host__ __device__ constexpr int fc_sec(int p) {
    p %= Fc<NZ, CW>::P;
    return p < Fc<NZ, CW>::JH * Fc<NZ, CW>::S_IN ? 0 : (p < Fc<NZ, CW>::JH * (Fc<NZ, CW>::S_IN + Fc<NZ, CW>::S_H) ? 1 : 2);
}
template <int NZ, int CW> __host__ __device__ constexpr int fc_off(int p) {
    using S = Fc<NZ, CW>;
    p %= S::P;
    if (p < S::JH * S::S_IN) return (4 * (p / S::S_IN) * S::S_IN + p % S::S_IN) * 64;
    p -= S::JH * S::S_IN;
    if (p < S::JH * S::S_H) return (4 * (p / S::S_H) * S::S_H + p % S::S_H) * 64;
    return (p - S::JH * S::S_H) * 64;
}

// One section of the wave's stream: NJ jobs (output row tiles) of NG groups each, starting at stream position P0.  Per group: four
// MFMAs fed by one ring slot (A: four k-steps of this lane's weight row) and one 16-byte LDS read (B: the same four k of column n);
// the slot is refilled with the group FC_PF positions ahead — possibly the next layer's or the next stage's.
template <int NZ, int CW, int P0, int NJ, int NG, class Epi>
__device__ __forceinline__ void fc_section(f32x4 (&ring)[FC_PF], const f32x4* const (&base)[3], int lane, const float* brow, Epi&& epi) {
    using S = Fc<NZ, CW>;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        typename S::acc_t acc = (typename S::acc_t)(0.0f);
        f32x4 b[2];
        b[0] = *reinterpret_cast<const f32x4*>(brow);
#pragma unroll
        for (int g = 0; g < NG; g++) {
            const int p = P0 + j * NG + g;
            if (g + 1 < NG) b[(g + 1) & 1] = *reinterpret_cast<const f32x4*>(brow + S::KG * (g + 1));
            const f32x4 a = ring[p % FC_PF];
            ring[p % FC_PF] = (base[fc_sec<NZ, CW>(p + FC_PF)] + fc_off<NZ, CW>(p + FC_PF))[lane];
            const f32x4 bv = b[g & 1];
            if constexpr (CW == 32) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv.w, acc, 0, 0, 0);
            } else {
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bv.w, acc, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        epi(j, acc);
    }
}

// state items owned by a thread: item it = tid + 256 r  ->  (column it / NZ, level it % NZ)
#define FC_OWNER_INDEX()                                                   \
    int oc[S::OWN];                                                        \
    const int oi = tid & (NZ - 1);                                         \
    _Pragma("unroll") for (int r = 0; r < S::OWN; r++) oc[r] = (tid + 256 * r) / NZ

// The --conv filter's pre-activation (FcConv, engine_fc.h) for this lane's level from the column's levels in the lanes above (d = 0: the lane's own):
// ONE instruction sequence for the forward kernel, the adjoint's recomputation and the embedded step, so that all see the same bits and the same sign.
// cw[d] multiplies x[i + d] (w[c - d], 1-based), cb = b.
__device__ __forceinline__ float fc_conv_pre(float x, const float (&cw)[FC_CONV_MAX], float cb, int c) {
    float pre = cb;
#pragma unroll
    for (int d = 0; d < FC_CONV_MAX; d++)
        if (d < c) pre = fmaf(cw[d], __shfl_down(x, d), pre);                   // taps in a fixed order: w[c], w[c-1], ..., w[1]
    return pre;
}

// ------------------------------------------------------------------------------------------------
// embedded inference, shared pieces (fc_infer_kernel, fce_kernel).  LDS rows as in the forward solve: X [CW][LDX] the scaled input,
// A1, A2 [CW][LDH] the hidden activations, PART = A1 the partial sums of the last layer, BL the biases.
// ------------------------------------------------------------------------------------------------
// T̂ = T_scaling(19.65 + T/20) (double_gyre_nn.jl:156-158)
__device__ __forceinline__ float fc_infer_scale(float T, float mu_T, float inv_sig_T) { return ((19.65f + T / 20.0f) - mu_T) * inv_sig_T; }

// wT = enforce_fluxes(inv(wT_scaling)(NN(T̂)), 0, surface_flux) (:160) for the state item (column c of the tile, level oi): the faces below (lo,
// face oi) and above (hi, face oi + 1) the cell.  Lane oi - 1 holds face oi (a column's levels are consecutive lanes).
template <int NZ, int CW>
__device__ __forceinline__ void fc_infer_faces(const float* PART, int c, int oi, float b3v, float sig_wT, float mu_wT, float tf, float& lo, float& hi) {
    using S = Fc<NZ, CW>;
    float o = b3v;
#pragma unroll
    for (int ks = 0; ks < S::KS3; ks++) o += PART[(ks * CW + c) * NZ + oi];
    const float wT = sig_wT * o + mu_wT;                                   // face oi + 1
    const float below = __shfl_up(wT, 1);                                  // face oi
    lo = oi == 0 ? 0.0f : below;
    hi = oi == NZ - 1 ? tf : wT;
}
