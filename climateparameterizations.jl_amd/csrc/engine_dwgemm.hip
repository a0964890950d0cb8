// engine_dwgemm.hip — the gradient tail every training path runs (gfx950 / CDNA4 only): the taped weight-gradient GEMM in its three forms (f32
// operands straight from L2, f32 operands staged in LDS, exact three-way bf16 split planes in LDS) and the fixed-order reduction of the slab rows.
// The records are written by tile16's taped adjoint, the fc32 adjoints and the net-split adjoint; which blocks, passes and slices run is planned on
// the host (dw_plan.h).
#include "engine_dwgemm.h"
#include <cstdlib>
#include "kernel_select.h"
#include "split_bf16.h"

extern __shared__ __attribute__((aligned(16))) float smem[];

// ------------------------------------------------------------------------------------------------
// taped weight gradients: dW[i][j] = Σ_{records, columns} a[c][i] · dz[c][j], a split-K GEMM over the rows taped by
// adjoint_kernel<..., TAPEDW>.  The contracted index (column, stage) is the row index of the tape, so both MFMA operands
// are read from HBM/L2 already in operand layout (lane = feature, 128-byte segments): no LDS, no transposition.
// One wavefront owns one 64x64 block (2 x 2 tiles of v_mfma_f32_32x32x2_f32) for one slice of the records; the four
// waves of a workgroup hold consecutive blocks (same layer: shared input rows hit L1).  Workgroups that share a slice
// are placed on the same XCD (id mod 8) so that the slice streams through that XCD's L2 once.
// ------------------------------------------------------------------------------------------------
typedef float dwf32x16 __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(256)
dw_gemm_kernel(const float* __restrict__ dwtape, size_t n_records, int R, const DwMacro* __restrict__ macros, int n_macros,
               int n_groups, int n_slices, float* __restrict__ slab_rows, int stride, size_t tape_mstride, size_t slab_mstride) {
    dwtape += (size_t)blockIdx.y * tape_mstride;          // ensembles: blockIdx.y = model (its delta tape and slab rows); grid.y = 1: one model
    slab_rows += (size_t)blockIdx.y * slab_mstride;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = blockIdx.x, xcd = L & 7, k = L >> 3;
    const int group = k % n_groups, slice = (k / n_groups) * 8 + xcd;
    const int mi = group * 4 + wave;
    if (slice >= n_slices || mi >= n_macros) return;
    const DwMacro mc = macros[mi];
    const size_t per = (n_records + n_slices - 1) / n_slices;
    const size_t r0 = (size_t)slice * per, r1 = r0 + per < n_records ? r0 + per : n_records;
    const int f = lane & 31, kk = lane >> 5;
    const bool a_hi = mc.ni_rem > 32, d_hi = mc.no_rem > 32;
    const int fa0 = min(mc.a_feat + f, R - 1), fa1 = min(mc.a_feat + 32 + f, R - 1);
    const int fd0 = min(mc.d_feat + f, R - 1), fd1 = min(mc.d_feat + 32 + f, R - 1);
    dwf32x16 acc00 = (dwf32x16)(0.0f), acc01 = acc00, acc10 = acc00, acc11 = acc00;
    for (size_t r = r0; r < r1; r++) {
        const float* rec = dwtape + r * ((size_t)CT * R) + (size_t)kk * R;
        float a0[8], a1[8], d0[8], d1[8];
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const float* row = rec + (size_t)(2 * s) * R;
            a0[s] = row[fa0];
            d0[s] = row[fd0];
            a1[s] = a_hi ? row[fa1] : 0.0f;
            d1[s] = d_hi ? row[fd1] : 0.0f;
        }
#pragma unroll
        for (int s = 0; s < 8; s++) {
            acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], d0[s], acc00, 0, 0, 0);
            if (d_hi) acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], d1[s], acc01, 0, 0, 0);
            if (a_hi) acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], d0[s], acc10, 0, 0, 0);
            if (a_hi && d_hi) acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], d1[s], acc11, 0, 0, 0);
        }
    }
    // D layout: lane (j = lane & 31, h = lane >> 5), register r -> row i = 8 (r / 4) + 4 h + (r % 4)
    float* out = slab_rows + (size_t)slice * stride + mc.g_off;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int i = 8 * (r >> 2) + 4 * kk + (r & 3);
        if (i < mc.ni_rem && f < mc.no_rem) out[(size_t)i * mc.no + f] = acc00[r];
        if (i < mc.ni_rem && f + 32 < mc.no_rem) out[(size_t)i * mc.no + f + 32] = acc01[r];
        if (i + 32 < mc.ni_rem && f < mc.no_rem) out[(size_t)(i + 32) * mc.no + f] = acc10[r];
        if (i + 32 < mc.ni_rem && f + 32 < mc.no_rem) out[(size_t)(i + 32) * mc.no + f + 32] = acc11[r];
    }
}

// LDS-staged variant: one workgroup streams its slice of records through two LDS buffers (global_load_lds, 16 bytes per lane: no
// register staging) and its DW_NW waves contract up to DW_MAXM blocks each from LDS, so the tape is read from HBM exactly once.
// Chosen when two records fit in LDS and the network has at most DW_NW * DW_MAXM blocks (64-256-256-63: 24 blocks, 77.7 KB records).
#define DW_MAXM 3          // blocks per wave: 3 x 64 accumulator registers leave room for two waves per SIMD
#define DW_NW 8            // waves per workgroup

// Round 3: (a) the operands of k-step t + 1 are read from LDS BEFORE the four MFMAs of step t are issued (the straight compiler schedule
// issued eight reads after each eight MFMAs and waited for them with the pipe draining: 72 % busy, profiles/r03g_cs_table.csv); (b) MAXM is a
// template parameter chosen from the number of blocks (a 32-level network has 8: one per wave, not three slots of which two are empty);
// (c) small records are staged RPB at a time, so that a barrier closes at least ~6 k cycles of MFMA work.
template <int MAXM, int NW, int RPB>
__global__ void __launch_bounds__(64 * NW)
dw_gemm_lds_kernel(const float* __restrict__ dwtape, size_t n_records, int R, const DwMacro* __restrict__ macros, int n_macros,
                   int n_slices, float* __restrict__ slab_rows, int stride, size_t tape_mstride, size_t slab_mstride) {
    dwtape += (size_t)blockIdx.y * tape_mstride;          // ensembles: blockIdx.y = model (its delta tape and slab rows); grid.y = 1: one model
    slab_rows += (size_t)blockIdx.y * slab_mstride;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.x;
    const int rec_floats = CT * R;                       // multiple of 4 (checked by the host)
    const int stage_floats = RPB * rec_floats;           // one LDS buffer: RPB consecutive records
    const size_t per = (n_records + n_slices - 1) / n_slices;
    const size_t r0 = (size_t)slice * per, r1 = r0 + per < n_records ? r0 + per : n_records;
    const int f = lane & 31, kk = lane >> 5;
    DwMacro mc[MAXM];
    int fa0[MAXM], fa1[MAXM], fd0[MAXM], fd1[MAXM];
    dwf32x16 acc[MAXM][4];
#pragma unroll
    for (int q = 0; q < MAXM; q++) {
        const int mi = wave + NW * q;
        if (mi < n_macros) mc[q] = macros[mi];
        else { mc[q].a_feat = 0; mc[q].d_feat = 0; mc[q].ni_rem = 0; mc[q].no_rem = 0; mc[q].g_off = 0; mc[q].no = 1; }
        fa0[q] = min(mc[q].a_feat + f, R - 1) + kk * R;
        fa1[q] = min(mc[q].a_feat + 32 + f, R - 1) + kk * R;
        fd0[q] = min(mc[q].d_feat + f, R - 1) + kk * R;
        fd1[q] = min(mc[q].d_feat + 32 + f, R - 1) + kk * R;
#pragma unroll
        for (int t = 0; t < 4; t++) acc[q][t] = (dwf32x16)(0.0f);
    }
    // asynchronous copy of up to RPB records into an LDS buffer: 1 KB per wave instruction, lanes contiguous
    // (issuing a stage's copy in slices between the blocks of the stage before it was measured slower: 56.4 -> 67.3 ms, profiles/r03s_gemm_spread.log)
    auto fetch = [&](size_t r, int dst /* float offset of the buffer inside smem */) {
        const size_t nrec = r1 - r < (size_t)RPB ? r1 - r : (size_t)RPB;
        const int nfl = (int)nrec * rec_floats;
        const float* src = dwtape + r * (size_t)rec_floats;
        for (int o = wave * 256; o < nfl; o += NW * 256)
            if (o + lane * 4 < nfl) __builtin_amdgcn_global_load_lds(src + o + lane * 4, smem + dst + o, 16, 0, 0);
    };
    if (r0 < r1) fetch(r0, 0);
    __syncthreads();
    int cur = 0;                                         // float offset of the buffer being contracted
    for (size_t r = r0; r < r1; r += RPB) {
        if (r + RPB < r1) fetch(r + RPB, stage_floats - cur);
        const int nv = (int)(r1 - r < (size_t)RPB ? r1 - r : (size_t)RPB);
#pragma unroll
        for (int rr = 0; rr < RPB; rr++) {
            if (rr >= nv) break;                         // wave-uniform: the last stage of a slice may hold fewer records
            const float* rec = smem + cur + rr * rec_floats;
            // straight-line over the wave's MAXM blocks x 8 k-steps (2 columns each); all four 32x32 tiles of a block are issued (a block
            // narrower than 64 reads clamped, in-range features whose products are never stored; an empty slot likewise)
            constexpr int T = MAXM * 8;
            float op[2][4];
            auto load = [&](int t, float (&o)[4]) {
                const int q = t >> 3, sgrp = t & 7;
                const float* row = rec + 2 * sgrp * R;
                o[0] = row[fa0[q]]; o[1] = row[fd0[q]]; o[2] = row[fa1[q]]; o[3] = row[fd1[q]];
            };
            load(0, op[0]);
#pragma unroll
            for (int t = 0; t < T; t++) {
                if (t + 1 < T) load(t + 1, op[(t + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                const int q = t >> 3;
                const float a0 = op[t & 1][0], d0 = op[t & 1][1], a1 = op[t & 1][2], d1 = op[t & 1][3];
                acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, d0, acc[q][0], 0, 0, 0);
                acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, d1, acc[q][1], 0, 0, 0);
                acc[q][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, d0, acc[q][2], 0, 0, 0);
                acc[q][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, d1, acc[q][3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();          // every wave is done with this buffer, and (vmcnt drain) the next stage has landed
        cur = stage_floats - cur;
    }
#pragma unroll
    for (int q = 0; q < MAXM; q++) {
        if (mc[q].ni_rem == 0) continue;
        float* out = slab_rows + (size_t)slice * stride + mc[q].g_off;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = 8 * (r >> 2) + 4 * kk + (r & 3);
            if (i < mc[q].ni_rem && f < mc[q].no_rem) out[(size_t)i * mc[q].no + f] = acc[q][0][r];
            if (i < mc[q].ni_rem && f + 32 < mc[q].no_rem) out[(size_t)i * mc[q].no + f + 32] = acc[q][1][r];
            if (i + 32 < mc[q].ni_rem && f < mc[q].no_rem) out[(size_t)(i + 32) * mc[q].no + f] = acc[q][2][r];
            if (i + 32 < mc[q].ni_rem && f + 32 < mc[q].no_rem) out[(size_t)(i + 32) * mc[q].no + f + 32] = acc[q][3][r];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dW GEMM with exact three-way bf16 operand splitting (COLNDE_MATRIX_BF16X3_EXACT).  One workgroup of 8 waves per slice of records, as above, but the record
// does not go to LDS as floats: every thread loads its share (two adjacent features x eight columns, 8-byte loads, two records ahead in
// registers), splits the values and writes three bf16 planes [feature][column half][8 bf16] — MFMA-operand order, so a block's operands
// are 12 ds_read_b128 per record and nothing is split twice.  Two plane buffers, ONE bare barrier per record (a wave that passed the
// barrier of record r has finished the products of record r - 1, whose buffer record r + 1 overwrites).  A pass holds the operand
// features of some layers only (compact order, DwPassDesc), so the planes and 2 x 64 accumulator registers per wave fit; the passes
// together read each tape float once.
// ------------------------------------------------------------------------------------------------
#define DWS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
typedef float dws_f32x2 __attribute__((ext_vector_type(2)));

template <int MAXM, int NIT>
__global__ void __launch_bounds__(512)
dw_gemm_split_kernel(const float* __restrict__ dwtape, size_t n_records, int R, const DwMacro* __restrict__ macros, DwPassDesc ps,
                     int n_slices, float* __restrict__ slab_rows, int stride, size_t tape_mstride, size_t slab_mstride) {
    dwtape += (size_t)blockIdx.y * tape_mstride;          // ensembles: blockIdx.y = model (its delta tape and slab rows); grid.y = 1: one model
    slab_rows += (size_t)blockIdx.y * slab_mstride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slice = blockIdx.x;
    const size_t per = (n_records + n_slices - 1) / n_slices;
    const size_t r0 = (size_t)slice * per, r1 = r0 + per < n_records ? r0 + per : n_records;
    if (r0 >= r1) return;                                  // (whole workgroup)
    const int Fc = ps.Fc, FcP = Fc + 64;
    u32x4* planes = reinterpret_cast<u32x4*>(smem);        // [2 buffers][3 planes][FcP features][2 column halves]
    // pad features (read by the clamped tiles of narrow blocks, never stored) must be finite
    for (int e = tid; e < 2 * 3 * 64 * 2; e += 512) {
        const int kh = e & 1, f = (e >> 1) & 63, bp = e >> 7;
        planes[((size_t)bp * FcP + Fc + f) * 2 + kh] = (u32x4)(0u);
    }
    // loader role: item `it` = (feature pair j, column half kh), j fastest (coalesced 8-byte loads)
    int src_off[NIT], cfeat[NIT], ikh[NIT];
    bool live[NIT];
#pragma unroll
    for (int k = 0; k < NIT; k++) {
        const int it = tid + 512 * k, np = Fc >> 1;
        live[k] = it < Fc;
        const int j = live[k] ? it % np : 0;
        ikh[k] = live[k] ? it / np : 0;
        cfeat[k] = 2 * j;
        int so = 0;
        for (int sg = 0; sg < ps.n_seg; sg++)
            if (cfeat[k] >= ps.seg[sg].dst && cfeat[k] < ps.seg[sg].dst + ps.seg[sg].len) so = ps.seg[sg].src + cfeat[k] - ps.seg[sg].dst;
        src_off[k] = so + 8 * ikh[k] * R;
    }
    const int f = lane & 31, kk = lane >> 5;
    DwMacro mc[MAXM];
    sp_f32x16 acc[MAXM][4];
#pragma unroll
    for (int q = 0; q < MAXM; q++) {
        const int mi = wave + 8 * q;
        if (mi < ps.n_macros) mc[q] = macros[ps.m0 + mi];
        else { mc[q].a_feat = 0; mc[q].d_feat = 0; mc[q].ni_rem = 0; mc[q].no_rem = 0; mc[q].g_off = 0; mc[q].no = 1; }
#pragma unroll
        for (int t = 0; t < 4; t++) acc[q][t] = (sp_f32x16)(0.0f);
    }
    dws_f32x2 pre[2][NIT][8];
    auto gl = [&](size_t r, dws_f32x2 (&dst)[NIT][8]) {
        const size_t rc = r < r1 ? r : r1 - 1;             // past the end: the last record again (loaded, never used)
        const float* rec = dwtape + rc * ((size_t)CT * R);
#pragma unroll
        for (int k = 0; k < NIT; k++)
#pragma unroll
            for (int c = 0; c < 8; c++) dst[k][c] = *reinterpret_cast<const dws_f32x2*>(rec + src_off[k] + c * R);
    };
    auto sp = [&](const dws_f32x2 (&src)[NIT][8], int buf) {
#pragma unroll
        for (int k = 0; k < NIT; k++) {
            if (!live[k]) continue;
#pragma unroll
            for (int z = 0; z < 2; z++) {
                float x8[8];
#pragma unroll
                for (int c = 0; c < 8; c++) x8[c] = src[k][c][z];
                const Bf3 b = bf3_split8(x8);
                u32x4* o = planes + ((size_t)(buf * 3) * FcP + cfeat[k] + z) * 2 + ikh[k];
                o[0] = b.h;
                o[(size_t)FcP * 2] = b.m;
                o[(size_t)FcP * 4] = b.l;
            }
        }
    };
    auto ld = [&](int buf, int cf) {
        const u32x4* o = planes + ((size_t)(buf * 3) * FcP + cf + f) * 2 + kk;
        Bf3 b;
        b.h = o[0];
        b.m = o[(size_t)FcP * 2];
        b.l = o[(size_t)FcP * 4];
        return b;
    };
    // (wave-uniform) the wave's two blocks are full 64 x 64 blocks of the same output columns: their d operands are read once
    const bool shared_d = MAXM == 2 && mc[0].ni_rem > 32 && mc[MAXM - 1].ni_rem > 32 && mc[0].no_rem > 32 && mc[MAXM - 1].no_rem > 32 &&
                          mc[0].d_feat == mc[MAXM - 1].d_feat;
    auto products = [&](int buf) {
        if (MAXM == 2 && shared_d) {
            // four a tiles against the same two d tiles: the next a tile is read while the current one is multiplied
            const Bf3 d0 = ld(buf, mc[0].d_feat), d1 = ld(buf, mc[0].d_feat + 32);
            Bf3 A = ld(buf, mc[0].a_feat);
#pragma unroll
            for (int t = 0; t < 2 * MAXM; t++) {
                const Bf3 Ac = A;
                if (t + 1 < 2 * MAXM) A = ld(buf, mc[(t + 1) >> 1].a_feat + 32 * ((t + 1) & 1));
                acc[t >> 1][2 * (t & 1)] = mfma_bf3(Ac, d0, acc[t >> 1][2 * (t & 1)]);
                acc[t >> 1][2 * (t & 1) + 1] = mfma_bf3(Ac, d1, acc[t >> 1][2 * (t & 1) + 1]);
                __builtin_amdgcn_sched_barrier(0);
            }
            return;
        }
#pragma unroll
        for (int q = 0; q < MAXM; q++) {
            if (mc[q].ni_rem == 0) continue;               // (wave-uniform) an empty slot
            const Bf3 a0 = ld(buf, mc[q].a_feat), d0 = ld(buf, mc[q].d_feat);
            acc[q][0] = mfma_bf3(a0, d0, acc[q][0]);
            if (mc[q].no_rem > 32) {
                const Bf3 d1 = ld(buf, mc[q].d_feat + 32);
                acc[q][1] = mfma_bf3(a0, d1, acc[q][1]);
                if (mc[q].ni_rem > 32) {
                    const Bf3 a1 = ld(buf, mc[q].a_feat + 32);
                    acc[q][2] = mfma_bf3(a1, d0, acc[q][2]);
                    acc[q][3] = mfma_bf3(a1, d1, acc[q][3]);
                }
            } else if (mc[q].ni_rem > 32) {
                const Bf3 a1 = ld(buf, mc[q].a_feat + 32);
                acc[q][2] = mfma_bf3(a1, d0, acc[q][2]);
            }
        }
    };
    // Between two barriers a wave multiplies record r (plane buffer r & 1) AND splits record r + 1 into the other buffer (free since the last
    // barrier: everybody has finished record r - 1).  The two waves of a SIMD (w, w + 4) take the two jobs in opposite order, so that one's
    // vector work and LDS round trips run under the other's MFMAs instead of both queueing for the matrix pipe at the same moment.
    const size_t n = r1 - r0;
    const bool split_first = (wave >> 2) & 1;
    gl(r0, pre[0]);
    gl(r0 + 1, pre[1]);
    sp(pre[0], 0);
    gl(r0 + 2, pre[0]);
    DWS_BARRIER();
    for (size_t i = 0; i < n; i += 2) {
        if (split_first) { sp(pre[1], 1); gl(r0 + i + 3, pre[1]); products(0); }
        else { products(0); sp(pre[1], 1); gl(r0 + i + 3, pre[1]); }
        DWS_BARRIER();
        if (i + 1 < n) {
            if (split_first) { sp(pre[0], 0); gl(r0 + i + 4, pre[0]); products(1); }
            else { products(1); sp(pre[0], 0); gl(r0 + i + 4, pre[0]); }
            DWS_BARRIER();
        }
    }
#pragma unroll
    for (int q = 0; q < MAXM; q++) {
        if (mc[q].ni_rem == 0) continue;
        float* out = slab_rows + (size_t)slice * stride + mc[q].g_off;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = 8 * (r >> 2) + 4 * kk + (r & 3);
            if (i < mc[q].ni_rem && f < mc[q].no_rem) out[(size_t)i * mc[q].no + f] = acc[q][0][r];
            if (i < mc[q].ni_rem && f + 32 < mc[q].no_rem) out[(size_t)i * mc[q].no + f + 32] = acc[q][1][r];
            if (i + 32 < mc[q].ni_rem && f < mc[q].no_rem) out[(size_t)(i + 32) * mc[q].no + f] = acc[q][2][r];
            if (i + 32 < mc[q].ni_rem && f + 32 < mc[q].no_rem) out[(size_t)(i + 32) * mc[q].no + f + 32] = acc[q][3][r];
        }
    }
}

// the instantiations of the two LDS-staged dW kernels: launched from, and their dynamic-LDS limit raised through, these tables
using DwSplitFn = decltype(&dw_gemm_split_kernel<1, 1>);
static const DwSplitFn kDwSplitKernels[2][2] = {{dw_gemm_split_kernel<1, 1>, dw_gemm_split_kernel<1, 2>},      // [maxm > 1][nit > 1]
                                                {dw_gemm_split_kernel<2, 1>, dw_gemm_split_kernel<2, 2>}};
using DwLdsFn = decltype(&dw_gemm_lds_kernel<1, DW_NW, 1>);
static const DwLdsFn kDwLdsKernels[3][3] = {{dw_gemm_lds_kernel<1, DW_NW, 1>, dw_gemm_lds_kernel<1, DW_NW, 2>, dw_gemm_lds_kernel<1, DW_NW, 4>},   // [maxm - 1][log2 rpb]
                                            {dw_gemm_lds_kernel<2, DW_NW, 1>, dw_gemm_lds_kernel<2, DW_NW, 2>, dw_gemm_lds_kernel<2, DW_NW, 4>},
                                            {dw_gemm_lds_kernel<3, DW_NW, 1>, dw_gemm_lds_kernel<3, DW_NW, 2>, dw_gemm_lds_kernel<3, DW_NW, 4>}};

hipError_t dw_set_kernel_attributes(size_t max_lds_bytes) {
    hipError_t e = hipSuccess;
    auto set = [&](auto* k) { if (k && e == hipSuccess) e = set_max_lds(k, max_lds_bytes); };
    for (const auto& row : kDwSplitKernels) for (auto k : row) set(k);
    for (const auto& row : kDwLdsKernels) for (auto k : row) set(k);
    return e;
}

hipError_t launch_dw_gemm_split(const float* dwtape, size_t n_records, int row_floats, const DwPlan& plan, const DwMacro* d_split_macros, int n_slices,
                                float* slab_rows, int slab_stride, hipStream_t stream, int n_models, size_t tape_mstride, size_t slab_mstride) {
    if (n_records == 0 || n_slices < 1 || plan.passes.empty()) return hipErrorInvalidValue;
    for (const DwPassDesc& pd : plan.passes) {
        const size_t lds = (size_t)2 * 3 * (pd.Fc + 64) * 2 * 16;
        const auto k = kDwSplitKernels[pd.maxm > 1][pd.nit > 1];
        hipLaunchKernelGGL(k, dim3(n_slices, n_models), dim3(512), lds, stream, dwtape, n_records, row_floats, d_split_macros, pd, n_slices, slab_rows, slab_stride, tape_mstride, slab_mstride);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

bool dw_gemm_lds_fits(int row_floats, int n_macros) {
    const char* e = getenv("COLNDE_T16_DWLDS");           // 0: always the L2-streaming kernel (testing aid)
    if (e && atoi(e) == 0) return false;
    return n_macros <= DW_NW * DW_MAXM && ((CT * row_floats) & 3) == 0 && (size_t)2 * CT * row_floats * sizeof(float) <= 160 * 1024;
}

// records staged per LDS buffer: as many as fit in half the LDS, at most 4
static int dw_gemm_rpb(int row_floats) {
    const size_t rec = (size_t)CT * row_floats * sizeof(float);
    const size_t n = (80 * 1024) / rec;
    return n >= 4 ? 4 : (n >= 2 ? 2 : 1);
}

hipError_t launch_dw_gemm(const float* dwtape, size_t n_records, int row_floats, const DwMacro* macros, int n_macros, int n_slices,
                          float* slab_rows, int slab_stride, hipStream_t stream, int n_models, size_t tape_mstride, size_t slab_mstride) {
    if (dw_gemm_lds_fits(row_floats, n_macros)) {
        if (n_records == 0 || n_slices < 1) return hipErrorInvalidValue;
        const int maxm = (n_macros + DW_NW - 1) / DW_NW, rpb = dw_gemm_rpb(row_floats);
        const size_t lds = (size_t)2 * rpb * CT * row_floats * sizeof(float);
        const auto k = kDwLdsKernels[maxm == 1 ? 0 : maxm == 2 ? 1 : 2][rpb == 4 ? 2 : rpb == 2 ? 1 : 0];
        hipLaunchKernelGGL(k, dim3(n_slices, n_models), dim3(64 * DW_NW), lds, stream, dwtape, n_records, row_floats, macros, n_macros, n_slices, slab_rows, slab_stride, tape_mstride, slab_mstride);
        return hipGetLastError();
    }
    if (n_records == 0 || n_macros < 1 || n_slices < 8 || (n_slices & 7)) return hipErrorInvalidValue;
    const int n_groups = (n_macros + 3) / 4;
    const int grid = n_groups * n_slices;          // = 8 * n_groups * (n_slices / 8): every (group, slice) pair once
    hipLaunchKernelGGL(dw_gemm_kernel, dim3(grid, n_models), dim3(256), 0, stream, dwtape, n_records, row_floats, macros, n_macros, n_groups,
                       n_slices, slab_rows, slab_stride, tape_mstride, slab_mstride);
    return hipGetLastError();
}

// grad[p] = Σ_rows slab[row][p] in a fixed order (deterministic): 64 parameters x 16 row lanes per workgroup, lane ry sums
// rows ry, ry + 16, ..., then the 16 partial sums are added in order; the 6 raw sums become scaled mean terms
__global__ void __launch_bounds__(1024) reduce_kernel(const float* __restrict__ slab, int n_tiles, int n_params, int stride, LossWeights lw,
                                                      float* __restrict__ out /* [n_params + 8] */, size_t slab_mstride, int out_mstride) {
    slab += (size_t)blockIdx.y * slab_mstride;            // ensembles: blockIdx.y = model; grid.y = 1: one model
    out += (size_t)blockIdx.y * out_mstride;
    __shared__ float part[16][65];
    const int px = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + px;
    float s = 0.0f;
    if (p < n_params + 6)
        for (int t = ry; t < n_tiles; t += 16) s += slab[(size_t)t * stride + p];
    part[ry][px] = s;
    __syncthreads();
    if (ry == 0 && p < n_params + 6) {
        float tot = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; q++) tot += part[q][px];
        if (p >= n_params) tot *= lw.w[p - n_params];
        out[p] = tot;
    }
}

// reduce_kernel under a member loss: the same sums in the same order, the six raw sums of model k scaled by its own weights lwk[k]
__global__ void __launch_bounds__(1024) reduce_member_kernel(const float* __restrict__ slab, int n_tiles, int n_params, int stride,
                                                             const LossWeights* __restrict__ lwk, float* __restrict__ out /* [n_params + 8] */,
                                                             size_t slab_mstride, int out_mstride) {
    slab += (size_t)blockIdx.y * slab_mstride;
    out += (size_t)blockIdx.y * out_mstride;
    __shared__ float part[16][65];
    const int px = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + px;
    float s = 0.0f;
    if (p < n_params + 6)
        for (int t = ry; t < n_tiles; t += 16) s += slab[(size_t)t * stride + p];
    part[ry][px] = s;
    __syncthreads();
    if (ry == 0 && p < n_params + 6) {
        float tot = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; q++) tot += part[q][px];
        if (p >= n_params) tot *= lwk[blockIdx.y].w[p - n_params];
        out[p] = tot;
    }
}

__global__ void finish_loss_kernel(float* __restrict__ out8, int out_mstride) {
    out8 += (size_t)blockIdx.x * out_mstride;             // ensembles: one workgroup per model
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int q = 0; q < 6; q++) t += out8[q];
        out8[6] = t;
        out8[7] = 0.0f;
    }
}

hipError_t launch_reduce(const float* slab, int n_tiles, int n_params, int stride, const LossWeights& lw, float* out,
                         hipStream_t stream, int n_models, size_t slab_mstride, int out_mstride) {
    hipLaunchKernelGGL(reduce_kernel, dim3((n_params + 6 + 63) / 64, n_models), dim3(1024), 0, stream, slab, n_tiles, n_params, stride, lw, out,
                       slab_mstride, out_mstride);
    hipLaunchKernelGGL(finish_loss_kernel, dim3(n_models), dim3(64), 0, stream, out + n_params, out_mstride);
    return hipGetLastError();
}

hipError_t launch_reduce_member(const float* slab, int n_tiles, int n_params, int stride, const LossWeights* lwk, float* out,
                                hipStream_t stream, int n_models, size_t slab_mstride, int out_mstride) {
    if (!lwk) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reduce_member_kernel, dim3((n_params + 6 + 63) / 64, n_models), dim3(1024), 0, stream, slab, n_tiles, n_params, stride, lwk, out,
                       slab_mstride, out_mstride);
    hipLaunchKernelGGL(finish_loss_kernel, dim3(n_models), dim3(64), 0, stream, out + n_params, out_mstride);
    return hipGetLastError();
}
