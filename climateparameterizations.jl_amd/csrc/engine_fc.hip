// engine_fc.hip — "fc32": the free-convection NDE on 32-column MFMA tiles with compile-time shapes (gfx950 only).
//
// Covers FreeConvectionNDE (free_convection/src/free_convection_nde.jl:29-38: dT/dt = -(σ_wT/σ_T)(τ/H) Dᶜ [b; NN(T); t]) with the network
// the reference trains, Dense(Nz,4Nz,relu) -> Dense(4Nz,4Nz,relu) -> Dense(4Nz,Nz-1) (train_free_convection_nde.jl:119-121), Nz = 32 or
// 64 (BASELINE configs[3] and its 32-level sibling), classical RK4.  Everything else stays on the generic tile16 engine.
//
// Why a second engine for this shape: 64-256-256-63 has 98,623 weights (394 KB) — they cannot live in a CU's LDS, so every stage of every
// column tile streams the whole A-operand image from L2.  tile16 feeds v_mfma_f32_16x16x4_f32 with 16-column tiles: 8 flop per streamed
// byte, i.e. 19.6 TB/s of L2->CU traffic at the fp32 MFMA peak, plus ≈50 address instructions per MFMA from runtime shapes (measured
// 44 % of peak on config 4).  Here a workgroup owns 32 columns and every dense layer runs on v_mfma_f32_32x32x2_f32 (M = 32 output
// rows, N = the 32 columns, 64 cycles): the same flops per cycle with HALF the operand bytes per flop for both operands, one 16-byte
// L2 load + one ds_read_b128 per FOUR MFMAs (256 cycles), all offsets compile-time immediates.
//
//  * 256 threads = 4 wavefronts, two workgroups per CU (LDS 75 KB / 67 KB): one's epilogues, physics and barriers hide under the
//    other's MFMA chains.  Layer l's row tiles are dealt to the waves (tiles w, w + 4); the last layer's two row tiles are split in K
//    so that all four waves work (partial sums to LDS, added in a fixed order by the physics).
//  * The A operand of a wave is ONE continuous stream — the same sequence of 16-byte groups every stage — fetched PF groups ahead
//    through a register ring that runs across layer boundaries, barriers and stages: L2 latency is exposed once per kernel.
//  * Workgroup barriers are bare `s_waitcnt lgkmcnt(0); s_barrier` (a __syncthreads() would drain the prefetch ring and the tape stores).
//  * Tapes: the forward kernel writes the stage input and the hidden activations a1, a2 STRAIGHT into tile16's delta-tape record
//    ([16 columns][xs | a1 a2 . | dz1 dz2 dz3], two records per 32-column tile and stage) and, separately, relu's derivative as one
//    bit per hidden unit in the accumulator layout (2 KB per tile and stage instead of 64 KB of pre-activations); the adjoint kernel
//    reads back nothing but those bits, back-propagates through W3ᵀ, W2ᵀ, W1ᵀ and fills the record's dz part; tile16's split-K dW GEMM
//    contracts the records unchanged.  Per column and stage: 4.9 KB of tape against tile16's 7.2 KB.
//  * Everything is summed in a fixed order: bit-reproducible gradients.
//  * COLNDE_MATRIX_BF16X3_EXACT (round 4): the 32-column tiles have kernels of their own (engine_fc_split.hip); the 16-column tiles of the latency sizes
//    (up to 4,096 columns) run THIS file's kernels with the operand stream swapped (FcStream<NZ, 16, true>): pre-split weight planes through the same kind
//    of ring, activations split by the wave that reads them (one split per 32-deep k-block, shared by its four / two row tiles, software-pipelined under
//    the previous block's MFMAs), v_mfma_f32_16x16x32_bf16.  Tapes, masks, epilogues, physics: unchanged.  8 simulations x 64 levels: 30.3 -> 24.6 ms.
#include <type_traits>
#include "engine_fc.h"
#include "split_bf16.h"
#include "fc_chain.h"

extern __shared__ float fc_smem[];

// slot position of the split stream (16-column tiles) -> section, and offset in 16-byte units from the wave's base of that section
template <int NZ> __host__ __device__ constexpr int fc16s_sec(int p) {
    p %= Fc<NZ, 16>::PS;
    return p < Fc<NZ, 16>::PS0 ? 0 : (p < Fc<NZ, 16>::PS0 + Fc<NZ, 16>::PS1 ? 1 : 2);
}
template <int NZ> __host__ __device__ constexpr int fc16s_off(int p) {
    using S = Fc<NZ, 16>;
    p %= S::PS;
    return (p < S::PS0 ? p : (p < S::PS0 + S::PS1 ? p - S::PS0 : p - S::PS0 - S::PS1)) * 64;
}

__device__ __forceinline__ f32x4 fc_mfma16_bf(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// The split twin of fc_section on 16-column tiles: NJ jobs of NKB 32-deep k-blocks, stream position P0 (slots).  Per k-block: two 16-byte LDS reads
// (the 8 floats of column n this lane multiplies), ONE exact three-way split of them (shared by the jobs), and per job three ring slots (the
// pre-split planes of the weight fragment) and six bf16 MFMAs, smallest products first; every slot is refilled PFS positions ahead as it is consumed.
template <int NZ, int P0, int NJ, int NKB, int PFS, class Epi>
__device__ __forceinline__ void fc_section_bf(u32x4 (&ring)[PFS], const u32x4* const (&base)[3], int lane, const float* brow, Epi&& epi) {
    using S = Fc<NZ, 16>;
    static_assert(PFS == S::PFS, "ring depth");
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[j] = (f32x4)(0.0f);
    // Software pipeline over the k-blocks: the split of block kb + 1 is issued in pieces BETWEEN the jobs' MFMA groups of block kb (one wave per SIMD at the
    // latency sizes: nothing else hides those 44 vector instructions), its eight floats were requested one block earlier still.
    f32x4 lo = *reinterpret_cast<const f32x4*>(brow), hi = *reinterpret_cast<const f32x4*>(brow + 4);
    f32x4 lo1 = lo, hi1 = hi;
    if (NKB > 1) {
        lo1 = *reinterpret_cast<const f32x4*>(brow + 32);
        hi1 = *reinterpret_cast<const f32x4*>(brow + 36);
    }
    Bf3 B;
    {
        const float x8[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        B = bf3_split8(x8);
    }
#pragma unroll
    for (int kb = 0; kb < NKB; kb++) {
        const float n8[8] = {lo1.x, lo1.y, lo1.z, lo1.w, hi1.x, hi1.y, hi1.z, hi1.w};      // block kb + 1 (landed during block kb - 1)
        if (kb + 2 < NKB) {
            lo1 = *reinterpret_cast<const f32x4*>(brow + 32 * (kb + 2));
            hi1 = *reinterpret_cast<const f32x4*>(brow + 32 * (kb + 2) + 4);
        }
        Bf3 Bn = B;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int p = P0 + (kb * NJ + j) * 3;
            const u32x4 Ah = ring[p % PFS], Am = ring[(p + 1) % PFS], Al = ring[(p + 2) % PFS];
            ring[p % PFS] = (base[fc16s_sec<NZ>(p + PFS)] + fc16s_off<NZ>(p + PFS))[lane];
            ring[(p + 1) % PFS] = (base[fc16s_sec<NZ>(p + 1 + PFS)] + fc16s_off<NZ>(p + 1 + PFS))[lane];
            ring[(p + 2) % PFS] = (base[fc16s_sec<NZ>(p + 2 + PFS)] + fc16s_off<NZ>(p + 2 + PFS))[lane];
            f32x4 c = acc[j];
            c = fc_mfma16_bf(Am, B.m, c);
            c = fc_mfma16_bf(Al, B.h, c);
            c = fc_mfma16_bf(Ah, B.l, c);
            c = fc_mfma16_bf(Am, B.h, c);
            c = fc_mfma16_bf(Ah, B.m, c);
            c = fc_mfma16_bf(Ah, B.h, c);
            acc[j] = c;
            __builtin_amdgcn_sched_barrier(0);
            if (kb + 1 < NKB) {
                // this job's share of the next block's split: pairs [4 j / NJ, 4 (j + 1) / NJ)
#pragma unroll
                for (int q = 4 * j / NJ; q < 4 * (j + 1) / NJ; q++) bf3_split_pair(n8[2 * q], n8[2 * q + 1], q, Bn);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        B = Bn;
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) epi(j, acc[j]);
}

// The operand stream of one wave behind one interface: f32 MFMA (fc_section: ring of FC_PF float4 groups) or, SPLIT (16-column tiles), bf16 MFMA on exact
// three-way splits (fc_section_bf: ring of PFS plane fragments).  `rows` is the LDS row of column n (B operand); section 2 starts at the wave's K part.
template <int NZ, int CW, bool SPLIT>
struct FcStream {
    using S = Fc<NZ, CW>;
    static_assert(!SPLIT || CW == 16, "this file's split path is the 16-column one (32 columns: engine_fc_split.hip)");
    typedef typename std::conditional<SPLIT, u32x4, f32x4>::type slot_t;
    static constexpr int DEPTH = SPLIT ? S::PFS : FC_PF;
    slot_t ring[DEPTH];
    const slot_t* base[3];

    __device__ __forceinline__ void init(const void* img, int w, int lane) {
        if constexpr (SPLIT) {
            const u32x4* im = reinterpret_cast<const u32x4*>(img);
            base[0] = im + S::SF1 / 4 + w * S::PS0 * 64;
            base[1] = im + S::SF2 / 4 + w * S::PS1 * 64;
            base[2] = im + S::SF3 / 4 + w * S::PS2 * 64;
#pragma unroll
            for (int q = 0; q < DEPTH; q++) ring[q] = (base[fc16s_sec<NZ>(q)] + fc16s_off<NZ>(q))[lane];
        } else {
            const float* im = reinterpret_cast<const float*>(img);
            base[0] = reinterpret_cast<const f32x4*>(im + S::F1) + (w * S::S_IN) * 64;
            base[1] = reinterpret_cast<const f32x4*>(im + S::F2) + (w * S::S_H) * 64;
            base[2] = reinterpret_cast<const f32x4*>(im + S::F3) + ((w % S::MT3) * S::S_H + (w / S::MT3) * S::G3) * 64;
#pragma unroll
            for (int q = 0; q < DEPTH; q++) ring[q] = (base[fc_sec<NZ, CW>(q)] + fc_off<NZ, CW>(q))[lane];
        }
    }
    // SEC 0: K = NZ hidden section, 1: K = 4 NZ hidden section, 2: the narrow layer (this wave's K part); h = lane / CW
    template <int SEC, class Epi>
    __device__ __forceinline__ void section(const slot_t* const (&sb)[3], int lane, int h, int w, const float* rows, Epi&& epi) {
        if constexpr (SPLIT) {
            if constexpr (SEC == 0) fc_section_bf<NZ, 0, S::JH, S::KB_IN>(ring, sb, lane, rows + 8 * h, epi);
            else if constexpr (SEC == 1) fc_section_bf<NZ, S::PS0, S::JH, S::KB_H>(ring, sb, lane, rows + 8 * h, epi);
            else fc_section_bf<NZ, S::PS0 + S::PS1, 1, S::KB3>(ring, sb, lane, rows + (w / S::MT3) * S::KB3 * 32 + 8 * h, epi);
        } else {
            if constexpr (SEC == 0) fc_section<NZ, CW, 0, S::JH, S::S_IN>(ring, sb, lane, rows + 4 * h, epi);
            else if constexpr (SEC == 1) fc_section<NZ, CW, S::JH * S::S_IN, S::JH, S::S_H>(ring, sb, lane, rows + 4 * h, epi);
            else fc_section<NZ, CW, S::JH * (S::S_IN + S::S_H), 1, S::G3>(ring, sb, lane, rows + (w / S::MT3) * S::G3 * S::KG + 4 * h, epi);
        }
    }
};

// ------------------------------------------------------------------------------------------------
// operand images.  Flux.destructure: W_l[o][i] (out o, in i) at w_off[l] + i*no + o, b_l[o] at b_off[l] + o.
//   forward  section (rows = outputs):  A[row = mt*CW + lane%CW][k = KG*S + 4(lane/CW) + j] = W_l[row][k]
//   backward section (rows = inputs):   A[row = it*CW + lane%CW][k = KG*S + 4(lane/CW) + j] = W_l[k][row]      (zero beyond the matrix)
// image[section][tile][S][lane][j]; backward sections in the order they are used: W3ᵀ (K = NZ), W2ᵀ, W1ᵀ (the narrow one).
// ------------------------------------------------------------------------------------------------
struct FcOffsets { int w[3], b[3]; };

// ENS (ensembles, 16-column tiles): blockIdx.y = model; the model's weights and images lie en.w / en.img / en.bias floats from model 0's.
template <int NZ, int CW, bool ENS = false>
__global__ void __launch_bounds__(256) fc_pack_kernel(FcOffsets o, const float* __restrict__ w, float* __restrict__ imgf, float* __restrict__ imgb,
                                                      float* __restrict__ bias, FcEns en) {
    using S = Fc<NZ, CW>;
    if constexpr (ENS) {
        const size_t k = blockIdx.y;
        w += k * en.w;
        imgf += k * en.img;
        if (imgb) imgb += k * en.img;
        bias += k * en.bias;
    }
    const int total = 2 * S::IMG + S::BIAS;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        if (idx >= 2 * S::IMG) {
            const int q = idx - 2 * S::IMG;
            float v;
            if (q < S::H) v = w[o.b[0] + q];
            else if (q < 2 * S::H) v = w[o.b[1] + q - S::H];
            else v = q - 2 * S::H < S::NO ? w[o.b[2] + q - 2 * S::H] : 0.0f;
            bias[q] = v;
            continue;
        }
        const bool fwd = idx < S::IMG;
        if (!fwd && !imgb) continue;                          // a forward-only pack (the embedding's ensemble images)
        const int e = fwd ? idx : idx - S::IMG;
        const int sec = e < S::F2 ? 0 : (e < S::F3 ? 1 : 2);
        const int r = e - (sec == 0 ? S::F1 : (sec == 1 ? S::F2 : S::F3));
        const int nS = sec == 0 ? S::S_IN : S::S_H;
        const int j = r & 3, lane = (r >> 2) & 63, blk = r >> 8;
        const int tile = blk / nS, Sg = blk - tile * nS;
        const int row = tile * CW + (lane & (CW - 1)), k = S::KG * Sg + 4 * (lane / CW) + j;
        float v = 0.0f;
        if (fwd) {
            // section 0: W1 (NZ -> H), 1: W2 (H -> H), 2: W3 (H -> NO)
            const int no = sec == 2 ? S::NO : S::H;
            if (row < no) v = w[o.w[sec] + k * no + row];
        } else {
            // section 0: W3ᵀ (rows = a2 features, k = outputs of layer 3), 1: W2ᵀ, 2: W1ᵀ (rows = state levels)
            const int l = 2 - sec;
            const int no = l == 2 ? S::NO : S::H;
            if (k < no) v = w[o.w[l] + row * no + k];
        }
        (fwd ? imgf : imgb)[e] = v;
    }
}

// The split images of the 16-column tiles (COLNDE_MATRIX_BF16X3_EXACT): the same two operand matrices as fc_pack_kernel's, every weight split exactly into
// three bf16 (x = h + m + l by truncation: split_bf16.h), laid out as each WAVE streams them — image[section][wave][k-block][job][plane][lane][8 bf16]:
// lane (m = lane % 16, kq = lane / 16), element i <-> k = 32 kb + 8 kq + i of row 16 (wave + 4 job) + m (sections 0, 1); section 2: row tile
// wave % MT3, k-blocks (wave / MT3) KB3 + g.
template <int NZ, bool ENS = false>
__global__ void __launch_bounds__(256) fc_pack_split16_kernel(FcOffsets o, const float* __restrict__ w, u32* __restrict__ simgf, u32* __restrict__ simgb,
                                                              FcEns en) {
    using S = Fc<NZ, 16>;
    if constexpr (ENS) {
        const size_t k = blockIdx.y;
        w += k * en.w;
        simgf += k * en.simg;
        simgb += k * en.simg;
    }
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < 2 * S::SIMG; idx += gridDim.x * 256) {
        const bool fwd = idx < S::SIMG;
        const int e = fwd ? idx : idx - S::SIMG;
        const int sec = e < S::SF2 ? 0 : (e < S::SF3 ? 1 : 2);
        const int r = e - (sec == 0 ? S::SF1 : (sec == 1 ? S::SF2 : S::SF3));
        const int i2 = r & 3, lane = (r >> 2) & 63, slot = r >> 8;                  // word of the fragment, lane, plane fragment
        const int per_wave = sec == 0 ? S::PS0 : (sec == 1 ? S::PS1 : S::PS2);
        const int wv = slot / per_wave, q = slot - wv * per_wave;
        const int pl = q % 3;
        int tile, kb;
        if (sec < 2) {
            const int j = (q / 3) % S::JH;
            kb = q / (3 * S::JH);
            tile = wv + 4 * j;
        } else {
            tile = wv % S::MT3;
            kb = (wv / S::MT3) * S::KB3 + q / 3;
        }
        const int row = tile * 16 + (lane & 15);
        u32 word = 0;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int k = 32 * kb + 8 * (lane >> 4) + 2 * i2 + t;
            float v = 0.0f;
            if (fwd) {
                const int no = sec == 2 ? S::NO : S::H;                              // sections: W1 (NZ -> H), W2 (H -> H), W3 (H -> NO)
                if (row < no) v = w[o.w[sec] + k * no + row];
            } else {
                const int l = 2 - sec;                                               // sections: W3^T (k = layer-3 outputs), W2^T, W1^T (rows = state levels)
                const int no = l == 2 ? S::NO : S::H;
                if (k < no) v = w[o.w[l] + row * no + k];
            }
            const float vh = __uint_as_float(__float_as_uint(v) & 0xffff0000u);
            const float rr = v - vh;
            const float vm = __uint_as_float(__float_as_uint(rr) & 0xffff0000u);
            const float part = pl == 0 ? vh : (pl == 1 ? vm : rr - vm);
            word |= (__float_as_uint(part) >> 16) << (16 * t);                      // element 2 i2 in the low half (Bf3's order)
        }
        (fwd ? simgf : simgb)[e] = word;
    }
}

// ------------------------------------------------------------------------------------------------
// forward solve (and, TAPE, the forward half of the tapes)
//   CA:  ConvectiveAdjustmentNDE (convective_adjustment_nde.jl:33-48): the face flux is [b; NN(T); t] - min(0, K dT/dz)
//   RKC: the s-stage RKC2 step of colnde_dev.h (coefficient table `rkc`, increment form: see tile16's forward_kernel) instead of classical RK4
// One record per right-hand-side evaluation: index step * nst + st, nst = 4 (RK4) or s.
// ------------------------------------------------------------------------------------------------
typedef unsigned long long u64;

//   ENS: an ensemble (colnde_create_fc_ensemble; 16-column tiles) — blockIdx.y = model.  What a model owns (operand image, biases, solution, the three
//        tapes; x0 when it is a saved state of the model's own solution) is offset ONCE, here in the prologue, by the strides of `en`: scalar arithmetic on
//        kernel arguments, no vector load is added before the stage loop.  The single-handle instantiations (ENS = false) never read `en`.
//   CONV: the --conv network (FcConv, engine_fc.h) — the filter is applied where the stage input goes to LDS.  The kernel's text is ONE body
//        (fc_forward_body.inc) behind two entry points: fc_forward_kernel (name and arguments as they were; CONV = false) and fc_forward_conv_kernel, which
//        adds the FcConv argument.  A template flag on fc_forward_kernel itself would rename every existing instantiation and lengthen its argument block.
//        ENS and CONV together (a conv ensemble) is a third entry point for the same reason: fc_forward_conv_ens_kernel, below.
// (the filter's pre-activation, fc_conv_pre: fc_chain.h — the embedded step applies the same filter)
// cw[d] = w[c - d] (1-based: the tap that multiplies x[i + d]), zero beyond the filter; cb = b
__device__ __forceinline__ void fc_conv_load(const FcConv& cv, float (&cw)[FC_CONV_MAX], float& cb) {
#pragma unroll
    for (int d = 0; d < FC_CONV_MAX; d++) cw[d] = d < cv.c ? cv.wb[cv.c - 1 - d] : 0.0f;
    cb = cv.wb[cv.c];
#pragma unroll
    for (int d = 0; d < FC_CONV_MAX; d++) asm volatile("" :: "v"(cw[d]));
    asm volatile("" :: "v"(cb));
}

template <int NZ, int CW, bool TAPE, bool CA, bool RKC, bool SPLIT = false, bool ENS = false>
__global__ void __launch_bounds__(256, 2)
fc_forward_kernel(const void* __restrict__ imgf, const float* __restrict__ bias, const float* __restrict__ x0, size_t x0_stride,
                  const float* __restrict__ bcs, const float* __restrict__ save_times, int n_save, int iv_begin, int iv_end, int tape_iv0, int substeps, float CN,
                  float caKN, int nst, const float* __restrict__ rkc, float* __restrict__ sol, float* __restrict__ dwtape, u32* __restrict__ masks,
                  u64* __restrict__ swtape, int n_col, FcEns en) {
    constexpr bool CONV = false;
    const FcConv cv = FcConv();
#include "fc_forward_body.inc"
}
template <int NZ, bool TAPE, bool CA, bool RKC, bool SPLIT>
__global__ void __launch_bounds__(256, 2)
fc_forward_conv_kernel(const void* __restrict__ imgf, const float* __restrict__ bias, const float* __restrict__ x0, size_t x0_stride,
                       const float* __restrict__ bcs, const float* __restrict__ save_times, int n_save, int iv_begin, int iv_end, int tape_iv0, int substeps,
                       float CN, float caKN, int nst, const float* __restrict__ rkc, float* __restrict__ sol, float* __restrict__ dwtape,
                       u32* __restrict__ masks, u64* __restrict__ swtape, int n_col, FcConv cv) {
    constexpr int CW = 16;
    constexpr bool ENS = false, CONV = true;
    const FcEns en = FcEns();
#include "fc_forward_body.inc"
}
// ENS and CONV together (colnde_create_conv_ensemble): blockIdx.y = model.  The body offsets what FcEns names; the filter's two pointers are offset here,
// once, the same way — scalar arithmetic on kernel arguments (cv0: model 0's, ce: the strides), before the body reads the taps.
template <int NZ, bool TAPE, bool CA, bool RKC, bool SPLIT>
__global__ void __launch_bounds__(256, 2)
fc_forward_conv_ens_kernel(const void* __restrict__ imgf, const float* __restrict__ bias, const float* __restrict__ x0, size_t x0_stride,
                           const float* __restrict__ bcs, const float* __restrict__ save_times, int n_save, int iv_begin, int iv_end, int tape_iv0,
                           int substeps, float CN, float caKN, int nst, const float* __restrict__ rkc, float* __restrict__ sol, float* __restrict__ dwtape,
                           u32* __restrict__ masks, u64* __restrict__ swtape, int n_col, FcConv cv0, FcEns en, FcConvEns ce) {
    constexpr int CW = 16;
    constexpr bool ENS = true, CONV = true;
    FcConv cv = cv0;
    cv.wb += (size_t)blockIdx.y * ce.wb;
    if constexpr (TAPE) cv.ctape += (size_t)blockIdx.y * ce.ctape;
#include "fc_forward_body.inc"
}

// ------------------------------------------------------------------------------------------------
// embedded inference: compute_neural_network_forcing! (free_convection/double_gyre_nn.jl:149-168; BASELINE configs[4]) — one evaluation of
// the network per column and the divergence of the flux it predicts.  The same sections as the forward solve, a workgroup walking over
// tiles (gridDim.x workgroups, tile += gridDim.x) so that the A-operand ring keeps streaming from one tile to the next.
//   T̂ = T_scaling(19.65 + T/20) (:156-158), wT = enforce_fluxes(inv(wT_scaling)(NN(T̂)), 0, surface_flux) (:160), forcing = -∂z wT (:135)
// ------------------------------------------------------------------------------------------------
template <int NZ, int CW>
__global__ void __launch_bounds__(256, 2)
fc_infer_kernel(const float* __restrict__ imgf, const float* __restrict__ bias, const float* __restrict__ T, const float* __restrict__ top_flux,
                float mu_T, float inv_sig_T, float sig_wT, float mu_wT, float inv_dz, float* __restrict__ out, int n_col) {
    using S = Fc<NZ, CW>;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & (CW - 1), h = lane / CW;               // column of the tile; k / row quad
    float* X = fc_smem;
    float* A1 = X + CW * S::LDX;
    float* A2 = A1 + CW * S::LDH;
    float* PART = A1;
    float* BL = A2 + CW * S::LDH;
    for (int q = tid; q < S::BIAS; q += 256) BL[q] = bias[q];
    FC_OWNER_INDEX();
    const f32x4* base[3];
    base[0] = reinterpret_cast<const f32x4*>(imgf + S::F1) + (w * S::S_IN) * 64;
    base[1] = reinterpret_cast<const f32x4*>(imgf + S::F2) + (w * S::S_H) * 64;
    base[2] = reinterpret_cast<const f32x4*>(imgf + S::F3) + ((w % S::MT3) * S::S_H + (w / S::MT3) * S::G3) * 64;
    f32x4 ring[FC_PF];
#pragma unroll
    for (int q = 0; q < FC_PF; q++) ring[q] = (base[fc_sec<NZ, CW>(q)] + fc_off<NZ, CW>(q))[lane];
    const float b3v = oi < S::NO ? bias[2 * S::H + oi] : 0.0f;
    asm volatile("" :: "v"(b3v));
    const int n_tiles = (n_col + CW - 1) / CW;
#pragma nounroll
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int zero = 0;
        FC_OPAQUE_ZERO(zero);
        const f32x4* const sb[3] = {base[0] + zero, base[1] + zero, base[2] + zero};
        const int col0 = tile * CW;
        float tf[S::OWN];
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            const int col = min(col0 + oc[r], n_col - 1);
            X[oc[r] * S::LDX + oi] = fc_infer_scale(T[(size_t)col * NZ + oi], mu_T, inv_sig_T);
            tf[r] = top_flux[col];
        }
        FC_BARRIER();
#include "fc_infer_chain.inc"
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            float lo, hi;
            fc_infer_faces<NZ, CW>(PART, oc[r], oi, b3v, sig_wT, mu_wT, tf[r], lo, hi);
            if (col0 + oc[r] < n_col) out[(size_t)(col0 + oc[r]) * NZ + oi] = -(hi - lo) * inv_dz;
        }
        FC_BARRIER();                                                               // PART (= A1's rows) is rewritten by the next tile's first layer
    }
}

// ------------------------------------------------------------------------------------------------
// adjoint: back-propagation through the stages from the taped relu (and switch) bits; fills the dz part of the delta-tape records.
// RKC: the discrete adjoint of the RKC2 recurrence as in tile16's adjoint_kernel — cotangents of Y_j (lam), Y_{j-1}, Y_{j-2}, Y_0 and F_0
// per state item — with ONE convective-adjustment switch pattern per step (that of Y_{s-1}, the first stage the backward sweep meets:
// DESIGN §2 "a finding about discrete adjoints of stabilised steppers").
// ------------------------------------------------------------------------------------------------
struct FcGrad { int b[3]; int n_params; };

// ENS: as in fc_forward_kernel — blockIdx.y = model; image, solution, tapes, λ hand-over and slab rows are the model's own, the truth is shared.
// CONV: as in the forward kernel, one body (fc_adjoint_body.inc) behind fc_adjoint_kernel (unchanged) and fc_adjoint_conv_kernel.  At the end of the pullback the filter's
// pre-activation is recomputed from the taped stage input (fc_conv_pre: the forward's bits), its cotangent goes to the second half of the conv-tape record
// (the filter's gradient is fc_conv_grad_kernel's: no accumulator rides along here) and x̄ = physics part + the filter's transpose applied to it.
template <int NZ, int CW, bool CA, bool RKC, bool SPLIT = false, bool ENS = false>
__global__ void __launch_bounds__(256, 2)
fc_adjoint_kernel(const void* __restrict__ imgb, const float* __restrict__ save_times, int n_save, int iv_begin, int iv_end, int substeps, float CN,
                  float caKN, int nst, const float* __restrict__ rkc, const float* __restrict__ sol, const float* __restrict__ truth,
                  float* __restrict__ dwtape, const u32* __restrict__ masks, const u64* __restrict__ swtape, float w_loss, float* __restrict__ lam_io,
                  float* __restrict__ slab, FcGrad go, int n_col, FcEns en) {
    constexpr bool CONV = false;
    const FcConv cv = FcConv();
#include "fc_adjoint_body.inc"
}
template <int NZ, bool CA, bool RKC, bool SPLIT>
__global__ void __launch_bounds__(256, 2)
fc_adjoint_conv_kernel(const void* __restrict__ imgb, const float* __restrict__ save_times, int n_save, int iv_begin, int iv_end, int substeps, float CN,
                       float caKN, int nst, const float* __restrict__ rkc, const float* __restrict__ sol, const float* __restrict__ truth,
                       float* __restrict__ dwtape, const u32* __restrict__ masks, const u64* __restrict__ swtape, float w_loss, float* __restrict__ lam_io,
                       float* __restrict__ slab, FcGrad go, int n_col, FcConv cv) {
    constexpr int CW = 16;
    constexpr bool ENS = false, CONV = true;
    const FcEns en = FcEns();
#include "fc_adjoint_body.inc"
}
template <int NZ, bool CA, bool RKC, bool SPLIT>
__global__ void __launch_bounds__(256, 2)
fc_adjoint_conv_ens_kernel(const void* __restrict__ imgb, const float* __restrict__ save_times, int n_save, int iv_begin, int iv_end, int substeps, float CN,
                           float caKN, int nst, const float* __restrict__ rkc, const float* __restrict__ sol, const float* __restrict__ truth,
                           float* __restrict__ dwtape, const u32* __restrict__ masks, const u64* __restrict__ swtape, float w_loss, float* __restrict__ lam_io,
                           float* __restrict__ slab, FcGrad go, int n_col, FcConv cv0, FcEns en, FcConvEns ce) {
    constexpr int CW = 16;
    constexpr bool ENS = true, CONV = true;
    FcConv cv = cv0;
    cv.wb += (size_t)blockIdx.y * ce.wb;
    cv.ctape += (size_t)blockIdx.y * ce.ctape;
#include "fc_adjoint_body.inc"
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
bool fc_supported(const DevModel& m, int stepper) {
    const bool fc = m.model == COLNDE_MODEL_FREE_CONVECTION, ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE;
    if (!(fc && stepper == COLNDE_STEPPER_RK4) && !(ca && (stepper == COLNDE_STEPPER_RK4 || stepper == COLNDE_STEPPER_RKC2))) return false;
    if (m.Nz != 32 && m.Nz != 64) return false;
    if (m.n_layers != 3 || m.n_nets != 1) return false;
    if (m.sizes[0] != m.Nz || m.sizes[1] != 4 * m.Nz || m.sizes[2] != 4 * m.Nz || m.sizes[3] != m.Nz - 1) return false;
    return m.acts[0] == COLNDE_ACT_RELU && m.acts[1] == COLNDE_ACT_RELU && m.acts[2] == COLNDE_ACT_IDENTITY;
}

size_t fc_image_floats(int Nz) { return Nz == 64 ? Fc<64>::IMG : Fc<32>::IMG; }        // (the same for both tile widths)
size_t fc_bias_floats(int Nz) { return Nz == 64 ? Fc<64>::BIAS : Fc<32>::BIAS; }
size_t fc_record_row_floats(int Nz) { return Nz == 64 ? Fc<64>::R : Fc<32>::R; }

template <int NZ, int CW> static size_t fc_lds_fwd() { return (size_t)(CW * Fc<NZ, CW>::LDX + 2 * CW * Fc<NZ, CW>::LDH + Fc<NZ, CW>::BIAS) * sizeof(float); }
template <int NZ, int CW> static size_t fc_lds_adj() { return (size_t)(2 * CW * Fc<NZ, CW>::LDH) * sizeof(float); }

// the instantiated (levels, tile width) x (model, stepper) combinations: FreeConvectionNDE x RK4; ConvectiveAdjustmentNDE x {RK4, RKC2}
#define FC_FOR_EACH_SHAPE(M, ...) M(64, 32, __VA_ARGS__) M(32, 32, __VA_ARGS__) M(64, 16, __VA_ARGS__) M(32, 16, __VA_ARGS__)
#define FC_FOR_EACH_FWD(M) FC_FOR_EACH_SHAPE(M, true, false, false) FC_FOR_EACH_SHAPE(M, false, false, false) \
                           FC_FOR_EACH_SHAPE(M, true, true, false) FC_FOR_EACH_SHAPE(M, false, true, false)   \
                           FC_FOR_EACH_SHAPE(M, true, true, true) FC_FOR_EACH_SHAPE(M, false, true, true)
#define FC_FOR_EACH_ADJ(M) FC_FOR_EACH_SHAPE(M, false, false) FC_FOR_EACH_SHAPE(M, true, false) FC_FOR_EACH_SHAPE(M, true, true)
// ... and their COLNDE_MATRIX_BF16X3_EXACT twins on 16-column tiles (this file; the 32-column ones: engine_fc_split.hip)
#define FC_FOR_EACH_SHAPE16(M, ...) M(64, 16, __VA_ARGS__) M(32, 16, __VA_ARGS__)
#define FC_FOR_EACH_FWD16(M) FC_FOR_EACH_SHAPE16(M, true, false, false) FC_FOR_EACH_SHAPE16(M, false, false, false) \
                             FC_FOR_EACH_SHAPE16(M, true, true, false) FC_FOR_EACH_SHAPE16(M, false, true, false)   \
                             FC_FOR_EACH_SHAPE16(M, true, true, true) FC_FOR_EACH_SHAPE16(M, false, true, true)
#define FC_FOR_EACH_ADJ16(M) FC_FOR_EACH_SHAPE16(M, false, false) FC_FOR_EACH_SHAPE16(M, true, false) FC_FOR_EACH_SHAPE16(M, true, true)

hipError_t fc_set_kernel_attributes() {
    hipError_t e;
#define FC_ATTR_F(N, W, T, C, K) if ((e = hipFuncSetAttribute((const void*)(fc_forward_kernel<N, W, T, C, K>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_fwd<N, W>())) != hipSuccess) return e;
#define FC_ATTR_A(N, W, C, K) if ((e = hipFuncSetAttribute((const void*)(fc_adjoint_kernel<N, W, C, K>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_adj<N, W>())) != hipSuccess) return e;
#define FC_ATTR_I(N, W, X) if ((e = hipFuncSetAttribute((const void*)(fc_infer_kernel<N, W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_fwd<N, W>())) != hipSuccess) return e;
    FC_FOR_EACH_FWD(FC_ATTR_F)
    FC_FOR_EACH_ADJ(FC_ATTR_A)
    FC_FOR_EACH_SHAPE(FC_ATTR_I, 0)
#define FC_ATTR_FS(N, W, T, C, K) if ((e = hipFuncSetAttribute((const void*)(fc_forward_kernel<N, W, T, C, K, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_fwd<N, W>())) != hipSuccess) return e;
#define FC_ATTR_AS(N, W, C, K) if ((e = hipFuncSetAttribute((const void*)(fc_adjoint_kernel<N, W, C, K, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_adj<N, W>())) != hipSuccess) return e;
    FC_FOR_EACH_FWD16(FC_ATTR_FS)
    FC_FOR_EACH_ADJ16(FC_ATTR_AS)
#undef FC_ATTR_FS
#undef FC_ATTR_AS
    // ... and the ensemble instantiations of the 16-column kernels, both arithmetics
#define FC_ATTR_FE(N, W, T, C, K)                                                                                                                                        \
    if ((e = hipFuncSetAttribute((const void*)(fc_forward_kernel<N, W, T, C, K, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_fwd<N, W>())) != hipSuccess) return e; \
    if ((e = hipFuncSetAttribute((const void*)(fc_forward_kernel<N, W, T, C, K, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_fwd<N, W>())) != hipSuccess) return e;
#define FC_ATTR_AE(N, W, C, K)                                                                                                                                           \
    if ((e = hipFuncSetAttribute((const void*)(fc_adjoint_kernel<N, W, C, K, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_adj<N, W>())) != hipSuccess) return e; \
    if ((e = hipFuncSetAttribute((const void*)(fc_adjoint_kernel<N, W, C, K, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_adj<N, W>())) != hipSuccess) return e;
    FC_FOR_EACH_FWD16(FC_ATTR_FE)
    FC_FOR_EACH_ADJ16(FC_ATTR_AE)
#undef FC_ATTR_FE
#undef FC_ATTR_AE
    // ... and the conv network's entry points (16-column tiles, both arithmetics)
#define FC_ATTR_FC(N, W, T, C, K)                                                                                                                                        \
    if ((e = hipFuncSetAttribute((const void*)(fc_forward_conv_kernel<N, T, C, K, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_fwd<N, W>())) != hipSuccess) return e; \
    if ((e = hipFuncSetAttribute((const void*)(fc_forward_conv_kernel<N, T, C, K, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_fwd<N, W>())) != hipSuccess) return e;
#define FC_ATTR_AC(N, W, C, K)                                                                                                                                           \
    if ((e = hipFuncSetAttribute((const void*)(fc_adjoint_conv_kernel<N, C, K, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_adj<N, W>())) != hipSuccess) return e; \
    if ((e = hipFuncSetAttribute((const void*)(fc_adjoint_conv_kernel<N, C, K, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_adj<N, W>())) != hipSuccess) return e;
    FC_FOR_EACH_FWD16(FC_ATTR_FC)
    FC_FOR_EACH_ADJ16(FC_ATTR_AC)
#undef FC_ATTR_FC
#undef FC_ATTR_AC
    // ... and those of a conv ensemble
#define FC_ATTR_FCE(N, W, T, C, K)                                                                                                                                       \
    if ((e = hipFuncSetAttribute((const void*)(fc_forward_conv_ens_kernel<N, T, C, K, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_fwd<N, W>())) != hipSuccess) return e; \
    if ((e = hipFuncSetAttribute((const void*)(fc_forward_conv_ens_kernel<N, T, C, K, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_fwd<N, W>())) != hipSuccess) return e;
#define FC_ATTR_ACE(N, W, C, K)                                                                                                                                          \
    if ((e = hipFuncSetAttribute((const void*)(fc_adjoint_conv_ens_kernel<N, C, K, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_adj<N, W>())) != hipSuccess) return e; \
    if ((e = hipFuncSetAttribute((const void*)(fc_adjoint_conv_ens_kernel<N, C, K, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fc_lds_adj<N, W>())) != hipSuccess) return e;
    FC_FOR_EACH_FWD16(FC_ATTR_FCE)
    FC_FOR_EACH_ADJ16(FC_ATTR_ACE)
#undef FC_ATTR_FCE
#undef FC_ATTR_ACE
#undef FC_ATTR_F
#undef FC_ATTR_A
#undef FC_ATTR_I
    return fcs_set_kernel_attributes();           // the split twins (engine_fc_split.hip)
}

// tile width for a problem of n_col columns: 16 while 32-column tiles could not put a workgroup on every CU twice over (COLNDE_FC_CW=16|32 forces)
int fc_tile_width(int n_col) {
    const char* e = getenv("COLNDE_FC_CW");
    if (e && (atoi(e) == 16 || atoi(e) == 32)) return atoi(e);
    return n_col <= 4096 ? 16 : 32;
}

hipError_t fc_launch_pack(const DevModel& m, int cw, const float* w, float* imgf, float* imgb, float* bias, unsigned int* simgf, unsigned int* simgb,
                          hipStream_t stream, const FcEns* ens) {
    FcOffsets o;
    for (int l = 0; l < 3; l++) { o.w[l] = m.w_off[l]; o.b[l] = m.b_off[l]; }
    if (ens) {                                             // every model's images in one launch each (16-column tiles only)
        // forward-only (imgb and both split images null): the f32 forward images and biases alone — what the embedded step reads
        const bool fwd_only = !imgb && !simgf && !simgb;
        if (cw != 16 || ens->n_models < 1 || ens->n_models > 65535 || !imgf || !bias || (!fwd_only && (!imgb || !simgf || !simgb))) return hipErrorInvalidValue;
        const unsigned K = (unsigned)ens->n_models;
        if (m.Nz == 64) {
            if (!fwd_only) hipLaunchKernelGGL((fc_pack_split16_kernel<64, true>), dim3(256, K), dim3(256), 0, stream, o, w, simgf, simgb, *ens);
            hipLaunchKernelGGL((fc_pack_kernel<64, 16, true>), dim3(256, K), dim3(256), 0, stream, o, w, imgf, imgb, bias, *ens);
        } else {
            if (!fwd_only) hipLaunchKernelGGL((fc_pack_split16_kernel<32, true>), dim3(128, K), dim3(256), 0, stream, o, w, simgf, simgb, *ens);
            hipLaunchKernelGGL((fc_pack_kernel<32, 16, true>), dim3(128, K), dim3(256), 0, stream, o, w, imgf, imgb, bias, *ens);
        }
        return hipGetLastError();
    }
    if (simgf && simgb && cw == 32) {                      // the split images of COLNDE_MATRIX_BF16X3_EXACT beside the f32 ones (the biases are shared)
        const hipError_t es = fcs_launch_pack(m, w, simgf, simgb, stream);
        if (es != hipSuccess) return es;
    } else if (simgf && simgb && cw == 16) {               // ... in the 16-column kernels' stream order (same size)
        if (m.Nz == 64) hipLaunchKernelGGL((fc_pack_split16_kernel<64>), dim3(256), dim3(256), 0, stream, o, w, simgf, simgb, FcEns());
        else hipLaunchKernelGGL((fc_pack_split16_kernel<32>), dim3(128), dim3(256), 0, stream, o, w, simgf, simgb, FcEns());
    }
    bool launched = false;
#define FC_PACK(N, W, X) if (!launched && m.Nz == N && cw == W) { hipLaunchKernelGGL((fc_pack_kernel<N, W>), dim3(N == 64 ? 256 : 128), dim3(256), 0, stream, o, w, imgf, imgb, bias, FcEns()); launched = true; }
    FC_FOR_EACH_SHAPE(FC_PACK, 0)
#undef FC_PACK
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t fc_launch_infer(const DevModel& m, int cw, const float* imgf, const float* bias, const float* T, const float* top_flux, float inv_dz,
                           float* out, int n_col, hipStream_t stream) {
    if (n_col < 1) return hipErrorInvalidValue;
    const int n_tiles = (n_col + cw - 1) / cw;
    const dim3 grid(n_tiles < 512 ? n_tiles : 512), block(256);                  // two workgroups per CU, each walking over its tiles
    bool launched = false;
#define FC_INF(N, W, X) if (!launched && m.Nz == N && cw == W) { hipLaunchKernelGGL((fc_infer_kernel<N, W>), grid, block, (fc_lds_fwd<N, W>()), stream, imgf, bias, T, top_flux, m.mu_T, 1.0f / m.sig_T, m.sig_wT, m.mu_wT, inv_dz, out, n_col); launched = true; }
    FC_FOR_EACH_SHAPE(FC_INF, 0)
#undef FC_INF
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t fc_launch_forward(const DevModel& m, int cw, const float* imgf, const unsigned int* simgf, const float* bias, const float* x0, size_t x0_stride,
                             const float* bcs, const float* save_times, int n_save, int iv_begin, int iv_end, int tape_iv0, int substeps, float* sol,
                             float* dwtape, unsigned int* masks, unsigned long long* swtape, int n_col, hipStream_t stream, const FcEns* ens, const FcConv* conv, const FcConvEns* cens) {
    if (n_col < 1 || iv_begin < 0 || iv_end > n_save - 1 || iv_begin >= iv_end || tape_iv0 < iv_begin || tape_iv0 >= iv_end) return hipErrorInvalidValue;
    if (conv) {                                             // the --conv network: the CONV entry points of the 16-column kernels, either arithmetic
        if (cw != 16 || conv->c < 2 || conv->c > FC_CONV_MAX || !conv->wb || (dwtape && !conv->ctape)) return hipErrorInvalidValue;
        if (ens && (!cens || ens->n_models < 1 || ens->n_models > 65535)) return hipErrorInvalidValue;      // a conv ensemble: grid.y = model
        const dim3 grid((n_col + 15) / 16, ens ? ens->n_models : 1), block(256);
        const float CN = m.C_fc * (float)m.Nz, caKN = m.ca_K * (float)m.Nz;
        const bool tape = dwtape != nullptr, ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE, rk = m.rkc != nullptr, split = simgf != nullptr;
        if ((tape && (!masks || (ca && !swtape))) || (rk && !ca)) return hipErrorInvalidValue;
        bool launched = false;
#define FC_FWDC(N, W, T, C, K)                                                                                                                       \
    if (!launched && m.Nz == N && tape == T && ca == C && rk == K) {                                                                                 \
        if (ens && split)                                                                                                                            \
            hipLaunchKernelGGL((fc_forward_conv_ens_kernel<N, T, C, K, true>), grid, block, (fc_lds_fwd<N, W>()), stream, (const void*)simgf, bias, x0, x0_stride, bcs,   \
                               save_times, n_save, iv_begin, iv_end, tape_iv0, substeps, CN, caKN, m.nst, m.rkc, sol, dwtape, masks, swtape, n_col, *conv, *ens, *cens); \
        else if (ens)                                                                                                                                \
            hipLaunchKernelGGL((fc_forward_conv_ens_kernel<N, T, C, K, false>), grid, block, (fc_lds_fwd<N, W>()), stream, (const void*)imgf, bias, x0, x0_stride, bcs,   \
                               save_times, n_save, iv_begin, iv_end, tape_iv0, substeps, CN, caKN, m.nst, m.rkc, sol, dwtape, masks, swtape, n_col, *conv, *ens, *cens); \
        else if (split)                                                                                                                              \
            hipLaunchKernelGGL((fc_forward_conv_kernel<N, T, C, K, true>), grid, block, (fc_lds_fwd<N, W>()), stream, (const void*)simgf, bias, x0, x0_stride, bcs,       \
                               save_times, n_save, iv_begin, iv_end, tape_iv0, substeps, CN, caKN, m.nst, m.rkc, sol, dwtape, masks, swtape, n_col, *conv); \
        else                                                                                                                                         \
            hipLaunchKernelGGL((fc_forward_conv_kernel<N, T, C, K, false>), grid, block, (fc_lds_fwd<N, W>()), stream, (const void*)imgf, bias, x0, x0_stride, bcs,       \
                               save_times, n_save, iv_begin, iv_end, tape_iv0, substeps, CN, caKN, m.nst, m.rkc, sol, dwtape, masks, swtape, n_col, *conv); \
        launched = true;                                                                                                                             \
    }
        FC_FOR_EACH_FWD16(FC_FWDC)
#undef FC_FWDC
        return launched ? hipGetLastError() : hipErrorInvalidValue;
    }
    if (ens) {                                              // all models in one launch: the ENS instantiations of the 16-column kernels, grid.y = model
        if (cw != 16 || ens->n_models < 1 || ens->n_models > 65535) return hipErrorInvalidValue;
        const dim3 grid((n_col + 15) / 16, ens->n_models), block(256);
        const float CN = m.C_fc * (float)m.Nz, caKN = m.ca_K * (float)m.Nz;
        const bool tape = dwtape != nullptr, ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE, rk = m.rkc != nullptr, split = simgf != nullptr;
        if ((tape && (!masks || (ca && !swtape))) || (rk && !ca)) return hipErrorInvalidValue;
        bool launched = false;
#define FC_FWDE(N, W, T, C, K)                                                                                                                       \
    if (!launched && m.Nz == N && tape == T && ca == C && rk == K) {                                                                                 \
        if (split)                                                                                                                                   \
            hipLaunchKernelGGL((fc_forward_kernel<N, W, T, C, K, true, true>), grid, block, (fc_lds_fwd<N, W>()), stream, (const void*)simgf, bias, x0, x0_stride, bcs,    \
                               save_times, n_save, iv_begin, iv_end, tape_iv0, substeps, CN, caKN, m.nst, m.rkc, sol, dwtape, masks, swtape, n_col, *ens); \
        else                                                                                                                                         \
            hipLaunchKernelGGL((fc_forward_kernel<N, W, T, C, K, false, true>), grid, block, (fc_lds_fwd<N, W>()), stream, (const void*)imgf, bias, x0, x0_stride, bcs,    \
                               save_times, n_save, iv_begin, iv_end, tape_iv0, substeps, CN, caKN, m.nst, m.rkc, sol, dwtape, masks, swtape, n_col, *ens); \
        launched = true;                                                                                                                             \
    }
        FC_FOR_EACH_FWD16(FC_FWDE)
#undef FC_FWDE
        return launched ? hipGetLastError() : hipErrorInvalidValue;
    }
    if (simgf && cw == 32) {                                // COLNDE_MATRIX_BF16X3_EXACT: the same solve on the bf16 pipe (engine_fc_split.hip)
        if (dwtape && (!masks || (m.model == COLNDE_MODEL_CONV_ADJ_NDE && !swtape))) return hipErrorInvalidValue;
        if (m.rkc && m.model != COLNDE_MODEL_CONV_ADJ_NDE) return hipErrorInvalidValue;
        return fcs_launch_forward(m, simgf, bias, x0, x0_stride, bcs, save_times, n_save, iv_begin, iv_end, tape_iv0, substeps, sol, dwtape, masks, swtape, n_col, stream);
    }
    const dim3 grid((n_col + cw - 1) / cw), block(256);
    const float CN = m.C_fc * (float)m.Nz, caKN = m.ca_K * (float)m.Nz;
    const bool tape = dwtape != nullptr, ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE, rk = m.rkc != nullptr;
    if (tape && (!masks || (ca && !swtape))) return hipErrorInvalidValue;
    if (rk && !ca) return hipErrorInvalidValue;
    bool launched = false;
    if (simgf && cw == 16) {                                // ... and on 16-column tiles: the SPLIT instantiations of this file's kernels
#define FC_FWDS(N, W, T, C, K)                                                                                                                       \
    if (!launched && m.Nz == N && tape == T && ca == C && rk == K) {                                                                                 \
        hipLaunchKernelGGL((fc_forward_kernel<N, W, T, C, K, true>), grid, block, (fc_lds_fwd<N, W>()), stream, (const void*)simgf, bias, x0, x0_stride, bcs, save_times, n_save, \
                           iv_begin, iv_end, tape_iv0, substeps, CN, caKN, m.nst, m.rkc, sol, dwtape, masks, swtape, n_col, FcEns());                \
        launched = true;                                                                                                                             \
    }
        FC_FOR_EACH_FWD16(FC_FWDS)
#undef FC_FWDS
        return launched ? hipGetLastError() : hipErrorInvalidValue;
    }
#define FC_FWD(N, W, T, C, K)                                                                                                                        \
    if (!launched && m.Nz == N && cw == W && tape == T && ca == C && rk == K) {                                                                      \
        hipLaunchKernelGGL((fc_forward_kernel<N, W, T, C, K>), grid, block, (fc_lds_fwd<N, W>()), stream, (const void*)imgf, bias, x0, x0_stride, bcs, save_times, n_save, \
                           iv_begin, iv_end, tape_iv0, substeps, CN, caKN, m.nst, m.rkc, sol, dwtape, masks, swtape, n_col, FcEns());                \
        launched = true;                                                                                                                             \
    }
    FC_FOR_EACH_FWD(FC_FWD)
#undef FC_FWD
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t fc_launch_adjoint(const DevModel& m, int cw, const float* imgb, const unsigned int* simgb, const float* save_times, int n_save, int iv_begin, int iv_end,
                             int substeps, const float* sol, const float* truth, float* dwtape, const unsigned int* masks, const unsigned long long* swtape,
                             float w_loss, float* lam_io, float* slab, int n_col, hipStream_t stream, const FcEns* ens, const FcConv* conv, const FcConvEns* cens) {
    if (n_col < 1 || !dwtape || !masks || iv_begin < 0 || iv_end > n_save - 1 || iv_begin >= iv_end) return hipErrorInvalidValue;
    if ((iv_begin > 0 || iv_end < n_save - 1) && !lam_io) return hipErrorInvalidValue;
    if (conv) {
        if (cw != 16 || conv->c < 2 || conv->c > FC_CONV_MAX || !conv->wb || !conv->ctape) return hipErrorInvalidValue;
        if (ens && (!cens || ens->n_models < 1 || ens->n_models > 65535)) return hipErrorInvalidValue;
        const dim3 grid((n_col + 15) / 16, ens ? ens->n_models : 1), block(256);
        const float CN = m.C_fc * (float)m.Nz, caKN = m.ca_K * (float)m.Nz;
        const bool ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE, rk = m.rkc != nullptr, split = simgb != nullptr;
        if ((ca && !swtape) || (rk && !ca)) return hipErrorInvalidValue;
        FcGrad go;
        for (int l = 0; l < 3; l++) go.b[l] = m.b_off[l];
        go.n_params = m.n_params;
        bool launched = false;
#define FC_ADJC(N, W, C, K)                                                                                                                          \
    if (!launched && m.Nz == N && ca == C && rk == K) {                                                                                              \
        if (ens && split)                                                                                                                            \
            hipLaunchKernelGGL((fc_adjoint_conv_ens_kernel<N, C, K, true>), grid, block, (fc_lds_adj<N, W>()), stream, (const void*)simgb, save_times, n_save, iv_begin,  \
                               iv_end, substeps, CN, caKN, m.nst, m.rkc, sol, truth, dwtape, masks, swtape, w_loss, lam_io, slab, go, n_col, *conv, *ens, *cens); \
        else if (ens)                                                                                                                                \
            hipLaunchKernelGGL((fc_adjoint_conv_ens_kernel<N, C, K, false>), grid, block, (fc_lds_adj<N, W>()), stream, (const void*)imgb, save_times, n_save, iv_begin,  \
                               iv_end, substeps, CN, caKN, m.nst, m.rkc, sol, truth, dwtape, masks, swtape, w_loss, lam_io, slab, go, n_col, *conv, *ens, *cens); \
        else if (split)                                                                                                                              \
            hipLaunchKernelGGL((fc_adjoint_conv_kernel<N, C, K, true>), grid, block, (fc_lds_adj<N, W>()), stream, (const void*)simgb, save_times, n_save, iv_begin,      \
                               iv_end, substeps, CN, caKN, m.nst, m.rkc, sol, truth, dwtape, masks, swtape, w_loss, lam_io, slab, go, n_col, *conv); \
        else                                                                                                                                         \
            hipLaunchKernelGGL((fc_adjoint_conv_kernel<N, C, K, false>), grid, block, (fc_lds_adj<N, W>()), stream, (const void*)imgb, save_times, n_save, iv_begin,      \
                               iv_end, substeps, CN, caKN, m.nst, m.rkc, sol, truth, dwtape, masks, swtape, w_loss, lam_io, slab, go, n_col, *conv); \
        launched = true;                                                                                                                             \
    }
        FC_FOR_EACH_ADJ16(FC_ADJC)
#undef FC_ADJC
        return launched ? hipGetLastError() : hipErrorInvalidValue;
    }
    if (ens) {
        if (cw != 16 || ens->n_models < 1 || ens->n_models > 65535) return hipErrorInvalidValue;
        const dim3 grid((n_col + 15) / 16, ens->n_models), block(256);
        const float CN = m.C_fc * (float)m.Nz, caKN = m.ca_K * (float)m.Nz;
        const bool ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE, rk = m.rkc != nullptr, split = simgb != nullptr;
        if ((ca && !swtape) || (rk && !ca)) return hipErrorInvalidValue;
        FcGrad go;
        for (int l = 0; l < 3; l++) go.b[l] = m.b_off[l];
        go.n_params = m.n_params;
        bool launched = false;
#define FC_ADJE(N, W, C, K)                                                                                                                          \
    if (!launched && m.Nz == N && ca == C && rk == K) {                                                                                              \
        if (split)                                                                                                                                   \
            hipLaunchKernelGGL((fc_adjoint_kernel<N, W, C, K, true, true>), grid, block, (fc_lds_adj<N, W>()), stream, (const void*)simgb, save_times, n_save, iv_begin,  \
                               iv_end, substeps, CN, caKN, m.nst, m.rkc, sol, truth, dwtape, masks, swtape, w_loss, lam_io, slab, go, n_col, *ens); \
        else                                                                                                                                         \
            hipLaunchKernelGGL((fc_adjoint_kernel<N, W, C, K, false, true>), grid, block, (fc_lds_adj<N, W>()), stream, (const void*)imgb, save_times, n_save, iv_begin,  \
                               iv_end, substeps, CN, caKN, m.nst, m.rkc, sol, truth, dwtape, masks, swtape, w_loss, lam_io, slab, go, n_col, *ens); \
        launched = true;                                                                                                                             \
    }
        FC_FOR_EACH_ADJ16(FC_ADJE)
#undef FC_ADJE
        return launched ? hipGetLastError() : hipErrorInvalidValue;
    }
    if (simgb && cw == 32) {
        if ((m.model == COLNDE_MODEL_CONV_ADJ_NDE && !swtape) || (m.rkc && m.model != COLNDE_MODEL_CONV_ADJ_NDE)) return hipErrorInvalidValue;
        return fcs_launch_adjoint(m, simgb, save_times, n_save, iv_begin, iv_end, substeps, sol, truth, dwtape, masks, swtape, w_loss, lam_io, slab, n_col, stream);
    }
    const dim3 grid((n_col + cw - 1) / cw), block(256);
    const float CN = m.C_fc * (float)m.Nz, caKN = m.ca_K * (float)m.Nz;
    const bool ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE, rk = m.rkc != nullptr;
    if ((ca && !swtape) || (rk && !ca)) return hipErrorInvalidValue;
    FcGrad go;
    for (int l = 0; l < 3; l++) go.b[l] = m.b_off[l];
    go.n_params = m.n_params;
    bool launched = false;
    if (simgb && cw == 16) {
#define FC_ADJS(N, W, C, K)                                                                                                                          \
    if (!launched && m.Nz == N && ca == C && rk == K) {                                                                                              \
        hipLaunchKernelGGL((fc_adjoint_kernel<N, W, C, K, true>), grid, block, (fc_lds_adj<N, W>()), stream, (const void*)simgb, save_times, n_save, iv_begin, iv_end, substeps, \
                           CN, caKN, m.nst, m.rkc, sol, truth, dwtape, masks, swtape, w_loss, lam_io, slab, go, n_col, FcEns());                     \
        launched = true;                                                                                                                             \
    }
        FC_FOR_EACH_ADJ16(FC_ADJS)
#undef FC_ADJS
        return launched ? hipGetLastError() : hipErrorInvalidValue;
    }
#define FC_ADJ(N, W, C, K)                                                                                                                           \
    if (!launched && m.Nz == N && cw == W && ca == C && rk == K) {                                                                                   \
        hipLaunchKernelGGL((fc_adjoint_kernel<N, W, C, K>), grid, block, (fc_lds_adj<N, W>()), stream, (const void*)imgb, save_times, n_save, iv_begin, iv_end, substeps, \
                           CN, caKN, m.nst, m.rkc, sol, truth, dwtape, masks, swtape, w_loss, lam_io, slab, go, n_col, FcEns());                     \
        launched = true;                                                                                                                             \
    }
    FC_FOR_EACH_ADJ(FC_ADJ)
#undef FC_ADJ
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}
