// regtile_dev.h — device code shared by the two kernel families of the static wind-mixing shape (Nz = 32, three 96-50-20-31 nets; gfx950 / CDNA4 only):
// regtile proper (engine_regtile.hip: one wavefront per 32- or 16-column tile) and the net-split kernels (engine_netsplit.hip: one wavefront per flux net).
// The register-tile primitives of the 32-column layout (v_mfma_f32_32x32x2_f32: mfma32, the level shifts, the operand-prefetching chains), the same for
// the 16-column layout (v_mfma_f32_16x16x4_f32 and the bf16 products: V16, rt16_chain), the activation value / derivative forms, and the phase stamps of
// the diagnostic builds.  Everything here is __forceinline__: each translation unit compiles its own copy into its kernels.
#pragma once
#include "engine_regtile.h"
#include "split_bf16.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// diagnostic build only (-DCOLNDE_STAMPS): per-phase cycle sums of wave 0 of workgroup 0.  The array is `static`: each translation unit that includes this
// header has its own (device symbols cannot be shared between units without relocatable device code), read back by rt_read_unit_stamps below.
#ifdef COLNDE_STAMPS
static __device__ unsigned long long g_rt_stamps[16];
#define RT_STAMP_DECL unsigned long long rs_t0 = 0, rs_acc[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; const unsigned long long rs_kk = __builtin_amdgcn_s_memtime(), rs_rr = __builtin_amdgcn_s_memrealtime()
#define RT_STAMP_BEGIN() do { __builtin_amdgcn_sched_barrier(0); rs_t0 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define RT_STAMP(i) do { __builtin_amdgcn_sched_barrier(0); unsigned long long t_ = __builtin_amdgcn_s_memtime(); rs_acc[i] += t_ - rs_t0; rs_t0 = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
// slots 8, 9: the whole kernel in shader ticks and in 100 MHz reference ticks (their ratio is the clock the kernel ran at); slot 10: phase stamp 8; slots 11 .. 14: phase stamps 9 .. 12
#define RT_STAMP_FLUSH() do { if (blockIdx.x == 0 && threadIdx.x == 0) { for (int q_ = 0; q_ < 8; q_++) g_rt_stamps[q_] = rs_acc[q_]; g_rt_stamps[8] = __builtin_amdgcn_s_memtime() - rs_kk; g_rt_stamps[9] = __builtin_amdgcn_s_memrealtime() - rs_rr; g_rt_stamps[10] = rs_acc[8]; for (int q_ = 9; q_ < 13; q_++) g_rt_stamps[q_ + 2] = rs_acc[q_]; } } while (0)
static inline hipError_t rt_read_unit_stamps(unsigned long long* out16) { return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_rt_stamps), sizeof(unsigned long long) * 16); }
#else
#define RT_STAMP_DECL
#define RT_STAMP_BEGIN()
#define RT_STAMP(i)
#define RT_STAMP_FLUSH()
static inline hipError_t rt_read_unit_stamps(unsigned long long* out16) {
    for (int i = 0; i < 8; i++) out16[i] = 0;
    return hipSuccess;
}
#endif

// ---- the 32-column layout: lane (j = lane & 31, h = lane >> 5) holds, in element r of a 16-float tile, row rho(r, h) = RHO0(r) + 4 h of column j
//      (the layout essay is at the head of engine_regtile.hip)
#define RHO0(r) (((r) & 3) + 8 * ((r) >> 2))

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// exchange between the two lane halves with v_permlane32_swap (one VALU op, no LDS round trip): lanes h = 0 receive
// `from_hi` as held by their partner lane + 32, lanes h = 1 receive `from_lo` as held by their partner lane - 32.
// (The instruction swaps vdst[32:63] with src0[0:31]: result 0 = {vdst.lo, src0.lo}, result 1 = {vdst.hi, src0.hi};
// probed on gfx950 by tools/probe/permlane.hip.)  The two values go in as separate operands on purpose: selecting the
// value to send per lane first (`h ? T[i] : T[j]`) is folded by LLVM into a divergent dynamic index into the register
// tile, which lowers to a 16-long v_cmp/v_cndmask chain per exchange.
__device__ __forceinline__ float xchg32(float from_hi, float from_lo, int h) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(from_hi), __float_as_uint(from_lo), false, false);
    return __uint_as_float(h ? r[0] : r[1]);
}
__device__ __forceinline__ float swap32(float x, int h) { return xchg32(x, x, h); }

// tile value one level below (rho - 1); level -1 reads `below`
__device__ __forceinline__ f32x16 shift_down(const f32x16 T, int h, float below) {
    f32x16 o;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        // row 8g (h = 0) takes T[4g-1] of the upper half; row 8g+4 (h = 1) takes T[4g+3] of the lower half
        const float recv = xchg32(g > 0 ? T[(4 * g + 15) & 15] : 0.0f, T[4 * g + 3], h);
        o[4 * g] = (h == 0 && g == 0) ? below : recv;
        o[4 * g + 1] = T[4 * g];
        o[4 * g + 2] = T[4 * g + 1];
        o[4 * g + 3] = T[4 * g + 2];
    }
    return o;
}

// tile value one level above (rho + 1); level 32 reads `above`
__device__ __forceinline__ f32x16 shift_up(const f32x16 T, int h, float above) {
    f32x16 o;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        // row 8g+3 (h = 0) takes T[4g] of the upper half; row 8g+7 (h = 1) takes T[4g+4] of the lower half
        const float recv = xchg32(T[4 * g], g < 3 ? T[(4 * g + 4) & 15] : 0.0f, h);
        o[4 * g + 3] = (h == 1 && g == 3) ? above : recv;
        o[4 * g] = T[4 * g + 1];
        o[4 * g + 1] = T[4 * g + 2];
        o[4 * g + 2] = T[4 * g + 3];
    }
    return o;
}

// per-lane A-operand bases into the LDS weight image
struct RtBases {
    int a1[5];   // layer 1, stacked tiles: row of tile mt for this lane's output row
    int a2;      // layer 2
    int a3;      // layer 3
};

__device__ __forceinline__ RtBases rt_bases(int lane) {
    const int i = lane & 31, h = lane >> 5;
    const int r_i = (i & 3) + 4 * (i >> 3), h_i = (i >> 2) & 1;
    RtBases b;
#pragma unroll
    for (int mt = 0; mt < 5; mt++) {
        const int G = min(mt * 16 + r_i, 74);                       // padding rows read a valid row; their output is never used
        const int row = (G / 25) * 50 + 2 * (G % 25) + h_i;
        b.a1[mt] = RT_W1C + row * RT_LD1 + 4 * h;
    }
    b.a2 = RT_W2C + ((r_i < 10) ? 2 * r_i + h_i : 0) * RT_LD2 + h;
    b.a3 = RT_W3C + (i - 1) * RT_LD3 + h;                           // output row i = face i <- NN output i-1 (row 0 masked later)
    return b;
}

// acc += sum_{s<N} A_s * B_s on the matrix pipe, with the A operands (one ds_read_b32 each) fetched one chunk of CH
// k-steps ahead of their MFMAs.  The sched_barrier mask lets ALU work (e.g. the previous tile's activations) be
// scheduled into the MFMA shadow but pins the DS reads to their region: left alone, the scheduler hoists hundreds of
// operand reads and spills.
#define RT_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0x00F)
#define RT_SCHED_HARD() __builtin_amdgcn_sched_barrier(0)      // nothing crosses: the operand fetches of a software pipeline stay AHEAD of the MFMAs that cover them

template <int N, int CH, class AF, class BF, class FF>
__device__ __forceinline__ f32x16 rt_chain_fill(const float* wl, f32x16 acc, AF aidx, BF bval, FF fill) {
    float a[2][CH];
#pragma unroll
    for (int u = 0; u < CH; u++)
        if (u < N) a[0][u] = wl[aidx(u)];
    RT_SCHED_FENCE();
#pragma unroll
    for (int c = 0; c * CH < N; c++) {
#pragma unroll
        for (int u = 0; u < CH; u++)
            if ((c + 1) * CH + u < N) a[(c + 1) & 1][u] = wl[aidx((c + 1) * CH + u)];
        fill(c);        // independent VALU work: scheduled into the gaps between this chunk's dependent MFMAs
#pragma unroll
        for (int u = 0; u < CH; u++)
            if (c * CH + u < N) acc = mfma32(a[c & 1][u], bval(c * CH + u), acc);
        RT_SCHED_FENCE();
    }
    return acc;
}

template <int N, int CH, class AF, class BF>
__device__ __forceinline__ f32x16 rt_chain(const float* wl, f32x16 acc, AF aidx, BF bval) {
    return rt_chain_fill<N, CH>(wl, acc, aidx, bval, [](int) {});
}

// ---- what the kernels of both units share beside the tiles
__device__ __forceinline__ float rt_top_flux(const DevModel& m, float bc5, float t) {
    if (!m.diurnal) return bc5;
    const float wq = bc5 * __sinf(6.283185307179586f / 86400.0f * (t * m.tau)) / m.alpha_g;
    return (wq - m.mu_wT) / m.sig_wT;
}

extern __shared__ __attribute__((aligned(16))) float rt_smem[];

// ---- activations: value, derivative, and both in one evaluation
// tanh's argument, clamped where e^{2z} leaves float32's range; a NaN z stays NaN (fminf / fmaxf alone answer -15 to it: colnde_dev.h, dev_tanh)
__device__ __forceinline__ float rt_tanh_arg(float z) {
    const float c = fminf(fmaxf(z, -15.0f), 15.0f);
    return z != z ? z : c;
}

template <int ACT>
__device__ __forceinline__ float rt_act(float z) {
    if (ACT == COLNDE_ACT_RELU) return !(z <= 0.0f) ? z : 0.0f;      // a NaN goes through (colnde_dev.h, dev_act)
    if (ACT == COLNDE_ACT_MISH) {
        const float e = __expf(__builtin_amdgcn_fmed3f(z, -3.0e38f, 20.0f));
        const float n = e * (e + 2.0f);
        return z * fast_div(n, n + 2.0f);
    }
    if (ACT == COLNDE_ACT_SWISH) return fast_div(z, 1.0f + __expf(-z));
    if (ACT == COLNDE_ACT_TANH) { const float e = __expf(2.0f * rt_tanh_arg(z)); return 1.0f - fast_div(2.0f, 1.0f + e); }
    if (ACT == COLNDE_ACT_LEAKYRELU) return z > 0.0f ? z : 0.01f * z;
    return z;
}

template <int ACT>
__device__ __forceinline__ float rt_act_grad(float z) {
    if (ACT == COLNDE_ACT_RELU) return z > 0.0f ? 1.0f : 0.0f;
    if (ACT == COLNDE_ACT_MISH) {
        const float e = __expf(__builtin_amdgcn_fmed3f(z, -3.0e38f, 20.0f));
        const float n = e * (e + 2.0f);
        const float t = fast_div(n, n + 2.0f);
        const float sg = fast_div(e, 1.0f + e);
        return t + z * (1.0f - t * t) * sg;
    }
    if (ACT == COLNDE_ACT_SWISH) { const float sg = fast_div(1.0f, 1.0f + __expf(-z)); return sg + z * sg * (1.0f - sg); }
    if (ACT == COLNDE_ACT_TANH) { const float e = __expf(2.0f * rt_tanh_arg(z)); const float t = 1.0f - fast_div(2.0f, 1.0f + e); return 1.0f - t * t; }
    if (ACT == COLNDE_ACT_LEAKYRELU) return z > 0.0f ? 1.0f : 0.01f;
    return 1.0f;
}

// activation and its derivative in one evaluation: one exponential and one reciprocal.
// mish(z) = z n / (n + 2) with n = e (e + 2), e = exp(z);  mish'(z) = e w / (n + 2)^2 with
// w = 4 (z + 1) + 4 e^2 + e^3 + e (4 z + 6) = p + e (n + 2 e + p + 2), p = 4 z + 4.
template <int ACT>
__device__ __forceinline__ void rt_act_pair(float z, float& a, float& d) {
    if (ACT == COLNDE_ACT_MISH) {
        const float e = __expf(__builtin_amdgcn_fmed3f(z, -3.0e38f, 20.0f));
        const float n = e * (e + 2.0f);
        const float q = n + 2.0f;
        const float r = __builtin_amdgcn_rcpf(q);
        const float p = 4.0f * z + 4.0f;
        const float w = fmaf(e, fmaf(2.0f, e, q) + p, p);          // n + 2 e + p + 2 = (q + 2 e) + p
        a = z * (n * r);
        d = (e * r) * (w * r);
    } else if (ACT == COLNDE_ACT_SWISH) {
        const float sg = fast_div(1.0f, 1.0f + __expf(-z));
        a = z * sg;
        d = sg + a * (1.0f - sg);
    } else {
        a = rt_act<ACT>(z);
        d = rt_act_grad<ACT>(z);
    }
}

// The SCALAR twin of rt_act4's packed mish form (rt_act4<ACT, false>): four values side by side, each through exactly the operations the packed
// form compiles to — v_fma_f32 where the shipped ISA has v_pk_fma_f32 (q = e (e + 2) + 2, beside the separately rounded n = e (e + 2)), separately
// rounded v_mul_f32 / v_add_f32 where it has v_pk_mul_f32 / v_pk_add_f32 — so the results are the same bits (tools/probe/pk_beside_mfma.hip,
// tests/test_gpu_regtile_bits.py).  Contraction is off in here: the one fused operation is spelled out, nothing else may fuse.
__device__ __forceinline__ f32x4v rt_mish4_scalar(f32x4v z) {
#pragma clang fp contract(off)
    float e[4], s[4], n[4], r[4];
#pragma unroll
    for (int i = 0; i < 4; i++) e[i] = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(z[i], -3.0e38f, 20.0f) * 1.4426950408889634f);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s[i] = e[i] + 2.0f;
        n[i] = e[i] * s[i];
        r[i] = __builtin_amdgcn_rcpf(fmaf(e[i], s[i], 2.0f));
    }
    return (f32x4v){z[0] * (n[0] * r[0]), z[1] * (n[1] * r[1]), z[2] * (n[2] * r[2]), z[3] * (n[3] * r[3])};
}

// Two activation value/derivative pairs at once on packed f32 arithmetic (v_pk_mul / v_pk_add / v_pk_fma: two lanes' worth of the same
// instruction per issue slot): 13 packed + 6 scalar (clamp, exp, rcp) instructions for two pairs instead of 34.  That pays where the wave has the
// SIMD's vector issue to itself — the adjoint (one wave per SIMD), whose pairs sit in vector-only phases or are a small part of what its W1^T
// products overlap (scalar twins measured there: neutral under the products, +1.5 ms in the vector-only phases) — and alone on a SIMD the packed
// sequence is the faster one (59 against 83 ticks per pair).  It does NOT hold beside another wave's MFMAs: there a packed instruction waits far
// longer for issue than the two scalar ones it replaces (452 against 141 ticks per pair beside v_mfma_f32_16x16x32_bf16:
// tools/probe/pk_beside_mfma.hip), which is why the two-waves-per-SIMD forward kernel on bf16 MFMAs uses rt_mish4_scalar.
template <int ACT>
__device__ __forceinline__ void rt_act_pair2(f32x2v z, f32x2v& a, f32x2v& d) {
    if (ACT == COLNDE_ACT_MISH) {
        f32x2v zc;
        zc.x = __builtin_amdgcn_fmed3f(z.x, -3.0e38f, 20.0f);
        zc.y = __builtin_amdgcn_fmed3f(z.y, -3.0e38f, 20.0f);
        const f32x2v t = zc * 1.4426950408889634f;
        f32x2v e;
        e.x = __builtin_amdgcn_exp2f(t.x);
        e.y = __builtin_amdgcn_exp2f(t.y);
        const f32x2v n = e * (e + 2.0f);
        const f32x2v q = n + 2.0f;
        f32x2v r;
        r.x = __builtin_amdgcn_rcpf(q.x);
        r.y = __builtin_amdgcn_rcpf(q.y);
        const f32x2v p = z * 4.0f + 4.0f;
        const f32x2v w = e * ((e * 2.0f + q) + p) + p;
        a = z * (n * r);
        d = (e * r) * (w * r);
    } else {
        float a0, d0, a1, d1;
        rt_act_pair<ACT>(z.x, a0, d0);
        rt_act_pair<ACT>(z.y, a1, d1);
        a.x = a0; a.y = a1; d.x = d0; d.y = d1;
    }
}

// activation VALUE only (forward kernels), four elements on packed arithmetic
template <int ACT, bool PK = true>
__device__ __forceinline__ f32x4v rt_act4(f32x4v z) {
    if (ACT == COLNDE_ACT_MISH && !PK) return rt_mish4_scalar(z);
    if (ACT == COLNDE_ACT_MISH) {
        f32x2v z0 = {z[0], z[1]}, z1 = {z[2], z[3]}, c0, c1, e0, e1, r0, r1;
        c0.x = __builtin_amdgcn_fmed3f(z0.x, -3.0e38f, 20.0f); c0.y = __builtin_amdgcn_fmed3f(z0.y, -3.0e38f, 20.0f);
        c1.x = __builtin_amdgcn_fmed3f(z1.x, -3.0e38f, 20.0f); c1.y = __builtin_amdgcn_fmed3f(z1.y, -3.0e38f, 20.0f);
        const f32x2v t0 = c0 * 1.4426950408889634f, t1 = c1 * 1.4426950408889634f;
        e0.x = __builtin_amdgcn_exp2f(t0.x); e0.y = __builtin_amdgcn_exp2f(t0.y);
        e1.x = __builtin_amdgcn_exp2f(t1.x); e1.y = __builtin_amdgcn_exp2f(t1.y);
        const f32x2v n0 = e0 * (e0 + 2.0f), n1 = e1 * (e1 + 2.0f);
        const f32x2v q0 = n0 + 2.0f, q1 = n1 + 2.0f;
        r0.x = __builtin_amdgcn_rcpf(q0.x); r0.y = __builtin_amdgcn_rcpf(q0.y);
        r1.x = __builtin_amdgcn_rcpf(q1.x); r1.y = __builtin_amdgcn_rcpf(q1.y);
        const f32x2v a0 = z0 * (n0 * r0), a1 = z1 * (n1 * r1);
        return (f32x4v){a0.x, a0.y, a1.x, a1.y};
    }
    return (f32x4v){rt_act<ACT>(z[0]), rt_act<ACT>(z[1]), rt_act<ACT>(z[2]), rt_act<ACT>(z[3])};
}

// four at once: two packed flows side by side, so that the results of the transcendental unit are not consumed by the very next instruction
template <int ACT>
__device__ __forceinline__ void rt_act_pair4(f32x2v z0, f32x2v z1, f32x2v& a0, f32x2v& d0, f32x2v& a1, f32x2v& d1) {
    if (ACT == COLNDE_ACT_MISH) {
        f32x2v c0, c1, e0, e1, r0, r1;
        c0.x = __builtin_amdgcn_fmed3f(z0.x, -3.0e38f, 20.0f); c0.y = __builtin_amdgcn_fmed3f(z0.y, -3.0e38f, 20.0f);
        c1.x = __builtin_amdgcn_fmed3f(z1.x, -3.0e38f, 20.0f); c1.y = __builtin_amdgcn_fmed3f(z1.y, -3.0e38f, 20.0f);
        const f32x2v t0 = c0 * 1.4426950408889634f, t1 = c1 * 1.4426950408889634f;
        e0.x = __builtin_amdgcn_exp2f(t0.x); e0.y = __builtin_amdgcn_exp2f(t0.y);
        e1.x = __builtin_amdgcn_exp2f(t1.x); e1.y = __builtin_amdgcn_exp2f(t1.y);
        const f32x2v p0 = z0 * 4.0f + 4.0f, p1 = z1 * 4.0f + 4.0f;
        const f32x2v n0 = e0 * (e0 + 2.0f), n1 = e1 * (e1 + 2.0f);
        const f32x2v q0 = n0 + 2.0f, q1 = n1 + 2.0f;
        r0.x = __builtin_amdgcn_rcpf(q0.x); r0.y = __builtin_amdgcn_rcpf(q0.y);
        r1.x = __builtin_amdgcn_rcpf(q1.x); r1.y = __builtin_amdgcn_rcpf(q1.y);
        const f32x2v w0 = e0 * ((e0 * 2.0f + q0) + p0) + p0, w1 = e1 * ((e1 * 2.0f + q1) + p1) + p1;
        a0 = z0 * (n0 * r0); a1 = z1 * (n1 * r1);
        d0 = (e0 * r0) * (w0 * r0); d1 = (e1 * r1) * (w1 * r1);
    } else {
        rt_act_pair2<ACT>(z0, a0, d0);
        rt_act_pair2<ACT>(z1, a1, d1);
    }
}

// ---- the 16-column layout (v_mfma_f32_16x16x4_f32): lane (j = lane & 15, g = lane >> 4) holds rows 4g..4g+3 of a 16-row x 16-column tile in a float4; the B
//      operand of k-step r is element r (K quad = rows r, 4+r, 8+r, 12+r).  A 32-level variable is two tiles (V16).
typedef float f32x4t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4t mfma16t(float a, float b, f32x4t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x4t mfma16_bf(u32x4 a, u32x4 b, f32x4t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// c += A B over one 32-deep k-block from the exact three-way splits of both operands (see rt_dw1_split_kernel)
__device__ __forceinline__ f32x4t mfma16_bf3(const Bf3& a, const Bf3& b, f32x4t c) {
    c = mfma16_bf(a.m, b.m, c);
    c = mfma16_bf(a.l, b.h, c);
    c = mfma16_bf(a.h, b.l, c);
    c = mfma16_bf(a.m, b.h, c);
    c = mfma16_bf(a.h, b.m, c);
    c = mfma16_bf(a.h, b.h, c);
    return c;
}
__device__ __forceinline__ Bf3 rt16_ldA(const u32x4* simg, int G, int lane) {
    Bf3 a;
    a.h = simg[(G * 3 + 0) * 64 + lane];
    a.m = simg[(G * 3 + 1) * 64 + lane];
    a.l = simg[(G * 3 + 2) * 64 + lane];
    return a;
}

__device__ __forceinline__ float rot_dn16(float x, int lane) { return __shfl(x, (lane + 48) & 63); }   // from lane - 16
__device__ __forceinline__ float rot_up16(float x, int lane) { return __shfl(x, (lane + 16) & 63); }   // from lane + 16

struct V16 { f32x4t t[2]; };    // one 32-level variable of 16 columns: level = 16 tau + 4 g + r

__device__ __forceinline__ V16 shift_down16(const V16& T, int lane, float below) {
    const int g = lane >> 4;
    const float r0 = rot_dn16(T.t[0][3], lane), r1 = rot_dn16(T.t[1][3], lane);
    V16 o;
    o.t[0][0] = g == 0 ? below : r0;
    o.t[1][0] = g == 0 ? r0 : r1;
#pragma unroll
    for (int tau = 0; tau < 2; tau++) { o.t[tau][1] = T.t[tau][0]; o.t[tau][2] = T.t[tau][1]; o.t[tau][3] = T.t[tau][2]; }
    return o;
}

__device__ __forceinline__ V16 shift_up16(const V16& T, int lane, float above) {
    const int g = lane >> 4;
    const float r0 = rot_up16(T.t[0][0], lane), r1 = rot_up16(T.t[1][0], lane);
    V16 o;
    o.t[0][3] = g == 3 ? r1 : r0;
    o.t[1][3] = g == 3 ? above : r1;
#pragma unroll
    for (int tau = 0; tau < 2; tau++) { o.t[tau][0] = T.t[tau][1]; o.t[tau][1] = T.t[tau][2]; o.t[tau][2] = T.t[tau][3]; }
    return o;
}

// acc += sum_{s<N} A_s B_s on 16x16x4 MFMAs, A operands prefetched one chunk ahead (see rt_chain)
template <int N, int CH, class AF, class BF>
__device__ __forceinline__ f32x4t rt16_chain(const float* wl, f32x4t acc, AF aidx, BF bval) {
    float a[2][CH];
#pragma unroll
    for (int u = 0; u < CH; u++)
        if (u < N) a[0][u] = wl[aidx(u)];
    RT_SCHED_FENCE();
    __builtin_amdgcn_s_setprio(1);      // two waves share a SIMD in rt16_forward_kernel: the one inside a chain issues first (35.0 -> 34.3 ms)
#pragma unroll
    for (int c = 0; c * CH < N; c++) {
#pragma unroll
        for (int u = 0; u < CH; u++)
            if ((c + 1) * CH + u < N) a[(c + 1) & 1][u] = wl[aidx((c + 1) * CH + u)];
#pragma unroll
        for (int u = 0; u < CH; u++)
            if (c * CH + u < N) acc = mfma16t(a[c & 1][u], bval(c * CH + u), acc);
        RT_SCHED_FENCE();
    }
    __builtin_amdgcn_s_setprio(0);
    return acc;
}

// value and derivative of the activation on a four-element tile
template <int ACT>
__device__ __forceinline__ void rt16_act_pair(const f32x4t z, f32x4t& a, f32x4t& d) {
    const f32x2v z0 = {z[0], z[1]}, z1 = {z[2], z[3]};
    f32x2v a0, d0, a1, d1;
    rt_act_pair4<ACT>(z0, z1, a0, d0, a1, d1);
    a = (f32x4t){a0.x, a0.y, a1.x, a1.y};
    d = (f32x4t){d0.x, d0.y, d1.x, d1.y};
}
