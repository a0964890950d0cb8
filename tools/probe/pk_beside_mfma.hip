// Probe: what the PACKED f32 form of the mish value/derivative sequence (v_pk_fma/mul/add_f32: rt_act_pair4 of engine_regtile.hip) costs
// against its SCALAR twin (v_fma/mul/add_f32: rt_mish4_scalar's form, with the derivative), alone on a SIMD and beside a second wave that runs a dependent chain of bf16 MFMAs.
// Workgroups of 8 waves (two per SIMD), one workgroup per CU: waves 0..3 run MFMAs (MODE 1: v_mfma_f32_16x16x32_bf16, MODE 2: v_mfma_f32_32x32x16_bf16,
// MODE 0: idle) until their partner is done, waves 4..7 evaluate ROUNDS x 4 activations (value + derivative; each round feeds the next, so nothing is
// hoisted).  Reports the vector waves' shader ticks per activation and the MFMA waves' ticks per MFMA, then checks that the two forms give the same BITS
// over a sweep of pre-activations (dense in [-30, 30], every binade of both signs, the clamp at 20, large negative, +-0, subnormals); exit status 1 if not.
// build: hipcc -O3 -fno-slp-vectorize --offload-arch=gfx950 pk_beside_mfma.hip -o pk_beside_mfma_probe (the engine's flags: no SLP packing of the scalar form) ; run on the GPU box (never shipped, never timed).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// engine_regtile.hip, rt_act_pair4<COLNDE_ACT_MISH>
__device__ __forceinline__ void mish_pk(f32x2v z0, f32x2v z1, f32x2v& a0, f32x2v& d0, f32x2v& a1, f32x2v& d1) {
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
}

// the same operations on scalar f32 (engine_regtile.hip, rt_mish4_scalar, plus the derivative): fmaf where the packed form compiles to v_pk_fma_f32
__device__ __forceinline__ void mish_sc(const float (&z)[4], float (&a)[4], float (&d)[4]) {
#pragma clang fp contract(off)
    float e[4], s[4], n[4], q[4], r[4], p[4];
#pragma unroll
    for (int i = 0; i < 4; i++) e[i] = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(z[i], -3.0e38f, 20.0f) * 1.4426950408889634f);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        p[i] = fmaf(z[i], 4.0f, 4.0f);
        s[i] = e[i] + 2.0f;
        n[i] = e[i] * s[i];
        q[i] = fmaf(e[i], s[i], 2.0f);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = __builtin_amdgcn_rcpf(q[i]);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        a[i] = z[i] * (n[i] * r[i]);
        const float w = fmaf(e[i], fmaf(e[i], 2.0f, q[i]) + p[i], p[i]);
        d[i] = (e[i] * r[i]) * (w * r[i]);
    }
}

template <bool PK>
__device__ __forceinline__ void mish4(float (&z)[4], float (&a)[4], float (&d)[4]) {
    if (PK) {
        f32x2v a0, d0, a1, d1;
        mish_pk((f32x2v){z[0], z[1]}, (f32x2v){z[2], z[3]}, a0, d0, a1, d1);
        a[0] = a0.x; a[1] = a0.y; a[2] = a1.x; a[3] = a1.y;
        d[0] = d0.x; d[1] = d0.y; d[2] = d1.x; d[3] = d1.y;
    } else
        mish_sc(z, a, d);
}

constexpr int ROUNDS = 8192, MFMA_CAP = 1 << 20;      // the MFMA waves stop with their partner, or at the cap

// cyc[0]: vector wave 4's ticks, cyc[1]: MFMA wave 0's ticks, cyc[2]: its MFMA count (block 0)
template <int MODE, bool PK>
__global__ void __launch_bounds__(512) timing(float* out, unsigned long long* cyc) {
    __shared__ volatile int done[4];
    const int wave = threadIdx.x >> 6;
    if (threadIdx.x < 4) done[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    float s = 0.0f;
    unsigned long long count = 0;
    if (wave < 4) {
        if (MODE != 0) {
            const u32x4 au = {0x3f803f80u + threadIdx.x, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u}, bu = {0x3c003c00u, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u};
            const bf16x8 a = __builtin_bit_cast(bf16x8, au), b = __builtin_bit_cast(bf16x8, bu);
            f32x4 c = {0, 0, 0, 0};
            f32x16 c16 = (f32x16)(0.0f);
            for (int i = 0; i < MFMA_CAP / 64 && !done[wave]; i++) {
#pragma unroll
                for (int u = 0; u < 64; u++) {
                    if (MODE == 1) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
                    else c16 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c16, 0, 0, 0);
                }
                count += 64;
            }
            s = c[0] + c16[0];
        }
    } else {
        float z[4] = {0.001f * threadIdx.x, 0.5f - 0.002f * threadIdx.x, 1.0f + 0.001f * threadIdx.x, -0.25f - 0.001f * threadIdx.x}, a[4], d[4];
        for (int i = 0; i < ROUNDS / 4; i++)
#pragma unroll
            for (int u = 0; u < 4; u++) {
                mish4<PK>(z, a, d);
#pragma unroll
                for (int k = 0; k < 4; k++) z[k] = fmaf(a[k], 0.25f, d[k]) - 1.0f;
            }
        s = z[0] + z[1] + z[2] + z[3];
        if ((threadIdx.x & 63) == 0) done[wave - 4] = 1;
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (blockIdx.x == 0 && threadIdx.x == 256) cyc[0] = t1 - t0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { cyc[1] = t1 - t0; cyc[2] = count; }
}

// thread i: activations 4 i .. 4 i + 3 of the sweep, both forms; bits[0 .. 8 n): packed a, d; bits[8 n ..): scalar a, d
__global__ void both_forms(const float* zin, int n4, unsigned* pk, unsigned* sc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float z[4] = {zin[4 * i], zin[4 * i + 1], zin[4 * i + 2], zin[4 * i + 3]}, a[4], d[4];
    mish4<true>(z, a, d);
    for (int k = 0; k < 4; k++) { pk[8 * i + k] = __float_as_uint(a[k]); pk[8 * i + 4 + k] = __float_as_uint(d[k]); }
    mish4<false>(z, a, d);
    for (int k = 0; k < 4; k++) { sc[8 * i + k] = __float_as_uint(a[k]); sc[8 * i + 4 + k] = __float_as_uint(d[k]); }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

template <int MODE, bool PK>
static int run(float* out, unsigned long long* cyc, double* per_act, double* per_mfma) {
    unsigned long long h[3];
    for (int rep = 0; rep < 2; rep++) {          // the second launch counts
        CHECK(hipMemset(cyc, 0, 3 * sizeof(unsigned long long)));
        hipLaunchKernelGGL((timing<MODE, PK>), dim3(256), dim3(512), 0, 0, out, cyc);
        CHECK(hipDeviceSynchronize());
    }
    CHECK(hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost));
    *per_act = (double)h[0] / (ROUNDS * 4.0);
    *per_mfma = h[2] ? (double)h[1] / (double)h[2] : 0.0;
    return 0;
}

int main() {
    float* out; unsigned long long* cyc;
    CHECK(hipMalloc(&out, 256 * 512 * sizeof(float)));
    CHECK(hipMalloc(&cyc, 3 * sizeof(unsigned long long)));
    double act[3][2], mf[3][2];
    if (run<0, true>(out, cyc, &act[0][0], &mf[0][0]) || run<0, false>(out, cyc, &act[0][1], &mf[0][1]) ||
        run<1, true>(out, cyc, &act[1][0], &mf[1][0]) || run<1, false>(out, cyc, &act[1][1], &mf[1][1]) ||
        run<2, true>(out, cyc, &act[2][0], &mf[2][0]) || run<2, false>(out, cyc, &act[2][1], &mf[2][1])) return 2;
    const char* names[3] = {"alone on the SIMD", "beside v_mfma_f32_16x16x32_bf16", "beside v_mfma_f32_32x32x16_bf16"};
    printf("mish value + derivative, shader ticks per activation (4 per round, %d rounds; the round's 4 v_fma_f32 + 4 v_add_f32 of feedback included)\n", ROUNDS);
    for (int m = 0; m < 3; m++)
        printf("%-34s packed %7.2f   scalar %7.2f   packed - scalar %+6.2f   (MFMA wave: %.1f / %.1f ticks per MFMA)\n", names[m], act[m][0], act[m][1],
               act[m][0] - act[m][1], mf[m][0], mf[m][1]);

    // ---- the bit check
    std::vector<float> z;
    for (int i = 0; i <= 60000; i++) z.push_back(-30.0f + 0.001f * i);
    for (int e = -149; e <= 127; e++)
        for (float f : {1.0f, 1.3333334f, 1.9999999f}) { z.push_back(ldexpf(f, e)); z.push_back(-ldexpf(f, e)); }      // every binade, subnormals included
    for (float f : {0.0f, -0.0f, 20.0f, 20.000002f, 19.999998f, 21.0f, 25.0f, 88.0f, 89.0f, 1.0e4f, 3.0e38f, -20.0f, -87.0f, -88.5f, -104.0f, -150.0f, -1.0e4f,
                    -1.0e30f, -3.0e38f, 1.1754944e-38f, -1.1754944e-38f, 1.4e-45f, -1.4e-45f})
        z.push_back(f);
    while (z.size() % 4) z.push_back(1.0f);
    const int n = (int)z.size(), n4 = n / 4;
    float* dz; unsigned *dpk, *dsc;
    CHECK(hipMalloc(&dz, n * sizeof(float)));
    CHECK(hipMalloc(&dpk, 2 * n * sizeof(unsigned)));
    CHECK(hipMalloc(&dsc, 2 * n * sizeof(unsigned)));
    CHECK(hipMemcpy(dz, z.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(both_forms, dim3((n4 + 255) / 256), dim3(256), 0, 0, dz, n4, dpk, dsc);
    CHECK(hipDeviceSynchronize());
    std::vector<unsigned> pk(2 * n), sc(2 * n);
    CHECK(hipMemcpy(pk.data(), dpk, 2 * n * sizeof(unsigned), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(sc.data(), dsc, 2 * n * sizeof(unsigned), hipMemcpyDeviceToHost));
    int bad = 0, nonfinite = 0;
    for (int i = 0; i < 2 * n; i++) {
        float f; memcpy(&f, &pk[i], 4);
        nonfinite += !std::isfinite(f);
        if (pk[i] != sc[i]) {
            if (bad++ < 10) printf("MISMATCH z = %.9g (%s): packed %08x scalar %08x\n", z[4 * (i / 8) + i % 4], (i % 8) < 4 ? "value" : "derivative", pk[i], sc[i]);
        }
    }
    printf("bit check: %d pre-activations, value and derivative: %d mismatches between the packed and the scalar form (%d non-finite results, compared as bits too)\n",
           n, bad, nonfinite);
    return bad ? 1 : 0;
}
