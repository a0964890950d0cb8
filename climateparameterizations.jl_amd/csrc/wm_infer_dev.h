// wm_infer_dev.h — device code shared by the two kernel units that evaluate the three wind-mixing flux networks on 32-column register tiles out of a
// VERBATIM weight image in LDS: the embedding (engine_wm_infer.hip) and the judging of a sweep (engine_wm_profile.hip).  The layout essay is at the
// head of engine_wm_infer.hip; the dense chains themselves are wm_net_layer1.inc and wm_net_layer23.inc, included textually by both units' tiles.
// Everything here is a macro or __forceinline__: each translation unit compiles its own copy into its kernels.
#pragma once
#include "engine_wm_infer.h"
#include "colnde_dev.h"

typedef float wm_f32x16 __attribute__((ext_vector_type(16)));

#define WM_WAVES 4
#define WM_W_LDS (((3 * WM_NET + 3) / 4) * 4)             // floats of the weight image (padded to 16 bytes)
#define WM_LD (WM_NZ + 1)                                  // row stride of a wave's staged rows: the 33 faces (conflict-free column walks)
#define WM_FS (32 * WM_LD)                                 // ... floats per field of one wave's 32 columns
#define WM_OFF_B1 (96 * WM_H1)
#define WM_OFF_W2 (WM_OFF_B1 + WM_H1)
#define WM_OFF_B2 (WM_OFF_W2 + WM_H1 * WM_H2)
#define WM_OFF_W3 (WM_OFF_B2 + WM_H2)
#define WM_OFF_B3 (WM_OFF_W3 + WM_H2 * 31)
#define WM_RHO0(r) (((r) & 3) + 8 * ((r) >> 2))
// the staged rows belong to ONE wave, whose LDS operations complete in order: no s_barrier, only the compiler is held to the order
#define WM_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

__device__ __forceinline__ wm_f32x16 wm_mfma(float a, float b, wm_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// A-operand bases (floats into wl).  Row i of an MFMA's A is row i of its result: register ri of lane half hi.
//   a1[tl]: layer 1, stacked tile tl: net n, feature 2 g + hi;  + 50 (32 t + rho(v, 0)) per k-step (G >= 75: padding rows, never consumed)
//   a2: layer 2: output feature 2 ri + hi; + 40 s per k-step;  a3: layer 3: output = interior face j;  + 62 s per k-step
#define WM_OPERAND_BASES() \
    const int ri = (j & 3) + 4 * (j >> 3), hi = (j >> 2) & 1; \
    int a1[5]; \
    _Pragma("unroll") \
    for (int tl = 0; tl < 5; tl++) { \
        const int G = min(16 * tl + ri, 74); \
        a1[tl] = (G / 25) * WM_NET + 2 * (G % 25) + hi + 4 * h * WM_H1; \
    } \
    const int a2 = WM_OFF_W2 + min(2 * ri + hi, WM_H2 - 1) + h * WM_H2; \
    const int a3 = WM_OFF_W3 + min(j, 30) + h * 31;

// cnt floats of the wave's LDS image to o, which is only 4-byte aligned (model m's faces start m n_col 33 floats into the output): singly up to
// the first 16-byte boundary, 16-byte pieces from there, the rest singly.  An aligned o takes the pieces of WM_STORE_FACES_ALIGNED.
#define WM_STORE_FACES_ANY(o, img, cnt) \
                if (cnt > 0) { \
                    const int pad = (int)(((uintptr_t)(o) >> 2) & 3); \
                    _Pragma("unroll") \
                    for (int i = 0; i < 5; i++) { \
                        const int p = 4 * (i * 64 + lane) - pad; \
                        if (p >= 0 && p + 3 < cnt) { \
                            const f32x4 val = {img[p], img[p + 1], img[p + 2], img[p + 3]}; \
                            *reinterpret_cast<f32x4*>(o + p) = val; \
                        } else if (p + 3 >= 0 && p < cnt) \
                            for (int t = max(p, 0); t < min(p + 4, cnt); t++) o[t] = img[t]; \
                    } \
                }
