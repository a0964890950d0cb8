// engine_wm_embed_any.h — the wind-mixing embedding for networks of ANY trained architecture: what wm_infer_ens_kernel computes for one
// model of the fixed 96-50-20-31 shape — the three stored +∂z arrays of the state as given, optionally the implicit Pacanowski–Philander step and /
// or the total face fluxes — for three networks of layer sizes (96, h1, …, 31) and any per-layer activations, in one launch.  Nz = 32.
//
// The first part is plain C++ (no HIP): the LDS plan, compiled alone by tests/wm_generic_plan_check.cpp.
#pragma once
#include <cstddef>

#define WMA_NZ 32
#define WMA_CT 16                         // columns per workgroup tile = N of v_mfma_f32_16x16x4_f32
#define WMA_WAVES 8
#define WMA_MAX_LAYERS 8                  // = COLNDE_MAX_LAYERS (api_embed.hip asserts it)
#define WMA_LD (WMA_NZ + 1)               // row stride of the state rows and of the face rows: the 33 faces
#define WMA_LDX (3 * WMA_NZ + 2)          // row stride of the scaled input [u; v; T]
#define WMA_LDY (WMA_NZ + 2)              // row stride of a net's 31 outputs
#define WMA_LDS_LIMIT (160 * 1024)        // bytes of LDS a workgroup of a gfx950 CU can have

// row stride of `width` features: a multiple of 4 plus 2 (the B-operand reads of the 16 columns then fall into different banks)
inline int wma_row_stride(int width) { return width > 0 ? ((width + 3) / 4) * 4 + 2 : 0; }

// The LDS of one 16-column tile, in floats from the start of the workgroup's dynamic LDS.  The nets are taken one after another, so ONE pair of
// activation buffers serves all three: layer l < n_layers − 1 writes buffer l & 1 and layer l + 1 reads it, each buffer as wide as the widest layer
// it ever holds; the last layer writes the net's own output rows.
struct WmAnyPlan {
    int st;          // [3][16][33] the raw state u, v, T: the rows the step sweeps in place
    int g;           // [3][16][33] ν ∂z u, ν ∂z v, νT ∂z T on the faces, then the finished faces (the image of the tile's span of each output)
    int xs;          // [16][WMA_LDX] the scaled input
    int y;           // [3][16][WMA_LDY] the nets' outputs
    int buf[2];      // [16][ld[p]] the activation buffers
    int ld[2];
    int floats;
    size_t bytes;
};

inline WmAnyPlan wm_any_plan(int n_layers, const int* sizes) {
    WmAnyPlan p = {};
    int w[2] = {0, 0};
    for (int l = 0; l + 1 < n_layers; l++)
        if (sizes[l + 1] > w[l & 1]) w[l & 1] = sizes[l + 1];
    p.ld[0] = wma_row_stride(w[0]);
    p.ld[1] = wma_row_stride(w[1]);
    int o = 0;
    p.st = o; o += 3 * WMA_CT * WMA_LD;
    p.g = o; o += 3 * WMA_CT * WMA_LD;
    p.xs = o; o += WMA_CT * WMA_LDX;
    p.y = o; o += 3 * WMA_CT * WMA_LDY;
    p.buf[0] = o; o += WMA_CT * p.ld[0];
    p.buf[1] = o; o += WMA_CT * p.ld[1];
    p.floats = o;
    p.bytes = sizeof(float) * (size_t)o;
    return p;
}
inline bool wm_any_fits(const WmAnyPlan& p) { return p.bytes <= (size_t)WMA_LDS_LIMIT; }

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include "engine_wm_infer.h"             // WmEmbedIO

struct WmAnyNet {                         // one net's layout inside the flat Flux.destructure vector; the three nets lie net_size apart
    int n_layers, net_size;
    int sizes[WMA_MAX_LAYERS + 1], acts[WMA_MAX_LAYERS], w_off[WMA_MAX_LAYERS], b_off[WMA_MAX_LAYERS];
};

struct WmAnyArgs {
    WmEmbedIO io;                         // the d/dz arrays are always written
    WmAnyNet net;
    const float* weights;                 // [3 net_size] uw; vw; wT — read in place, no packed image
    float mu[6], sigma[6];                // scalings u, v, T, uw, vw, wT
    MppParams mpp;                        // fused or diag
};

// every pointer of the state and the outputs must be 16-byte aligned and the plan must fit (hipErrorInvalidValue otherwise)
hipError_t launch_wm_embed_any(const WmAnyArgs& a, hipStream_t stream);
#endif
