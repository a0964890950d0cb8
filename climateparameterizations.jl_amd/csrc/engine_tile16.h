// engine_tile16.h — host/device interface of the MFMA tile engine: pack, rhs, forward, loss, adjoint, infer, pretrain and their launch geometry.
// (The taped adjoint's records are contracted by engine_dwgemm.h's GEMM, every slab is reduced by its launch_reduce.)
#pragma once
#include "colnde_dev.h"
#include "engine_dwgemm.h"   // LossWeights, dwtape_row_floats (the record launch_adjoint's dwtape holds)

struct PackInfo {
    int pf_off[COLNDE_MAX_LAYERS + 1];   // per-layer offsets inside one net's forward A-operand image
    int pb_off[COLNDE_MAX_LAYERS + 1];   // ... backward (transposed) image
    int pf_net, pb_net;                  // floats per net
};

// launch geometry chosen by the host for the adjoint kernel
struct AdjointGeom { int nthreads, maxt, maxr, wlds; };

#define MODEL_FLOATS ((int)((sizeof(DevModel) / 4 + 3) & ~3))   // the model description at the head of the adjoint kernel's LDS

static inline int lds_pad(int n) { int p = (n + 3) & ~3; return p + 2; }   // == 2 (mod 4)

static inline size_t lds_floats_forward(const DevModel& m) {
    return (size_t)2 * CT * m.ld_x + (size_t)m.n_nets * CT * m.ld_a + (size_t)4 * CT * m.ld_f + CT * 8;
}
static inline size_t lds_floats_adjoint(const DevModel& m) {
    return (size_t)3 * CT * m.ld_x + (size_t)2 * m.n_nets * CT * m.ld_a + (size_t)5 * CT * m.ld_f + CT * 8 + 16 * 8;
}

// DevModel::ag set (rows in global memory): what remains in LDS
static inline size_t lds_floats_forward_ag(const DevModel& m) { return lds_floats_forward(m) - (size_t)m.n_nets * CT * m.ld_a; }
static inline size_t lds_floats_adjoint_ag(const DevModel& m) { return lds_floats_adjoint(m) - (size_t)2 * m.n_nets * CT * m.ld_a; }
static inline size_t ag_floats_per_tile(const DevModel& m) { return (size_t)m.n_nets * CT * m.ld_a; }

// taped mode with the hidden pre-activations taped: no activation array on chip
static inline size_t lds_floats_adjoint_noA(const DevModel& m) { return lds_floats_adjoint(m) - (size_t)m.n_nets * CT * m.ld_a; }

hipError_t set_kernel_attributes(size_t max_lds_bytes);
hipError_t launch_pack(const DevModel& m, const PackInfo& pk, const float* w, float* wf, float* wb, hipStream_t stream);
// bf16 plane images of the dense chains (DevModel::sf / sb; offsets and sizes in m, 16-byte units): the weights split exactly, once per call
hipError_t launch_pack_planes(const DevModel& m, const float* w, unsigned* sf, unsigned* sb, hipStream_t stream);
// dx [n_col][ns] tendencies and / or flux [n_col][n_nets][Nz + 1] face fluxes (predict_flux); either may be null
hipError_t launch_rhs(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* x,
                      const float* bcs, float t, float* dx, int n_col, int nthreads, size_t lds_bytes, hipStream_t stream, float* flux = nullptr);
hipError_t launch_forward(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* x0,
                          const float* bcs, const float* save_times, int n_save, int substeps, float* sol, float* tape,
                          int n_col, int nthreads, bool wlds, size_t lds_bytes, hipStream_t stream, float* ztape = nullptr);
// n_models > 1 (ensembles): grid.y = model, sol [K] sol_mstride floats apart, partial [K][n_blocks][8]; truth shared
hipError_t launch_loss(const DevModel& m, const float* sol, const float* truth, int n_save, int n_col, float* partial,
                       int n_blocks, hipStream_t stream, int n_models = 1, size_t sol_mstride = 0);
// ... under a member loss (colnde_ensemble_set_member_loss): column c of model k enters its sums with the weight colw[k][c] (device, [n_models][n_col])
hipError_t launch_loss_member(const DevModel& m, const float* sol, const float* truth, int n_save, int n_col, float* partial,
                              int n_blocks, hipStream_t stream, int n_models, size_t sol_mstride, const float* colw);
hipError_t launch_adjoint(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* wb,
                          const TileDesc* tiles, const int* bias_zoff, const int* bias_goff, const float* bcs,
                          const float* save_times, int n_save, int substeps, const float* sol, const float* truth,
                          const float* tape, const LossWeights& lw, float* slab, int n_col, const AdjointGeom& geo,
                          size_t lds_bytes, hipStream_t stream, float* dwtape = nullptr, const float* ztape = nullptr);
// ---- tile ensembles (colnde_create_tile_ensemble): K models of one architecture, the model index in blockIdx.y ------------------------------------
// What a model owns lies these strides apart (floats; sf / sb: 32-bit words; ag: floats per model = tiles x ag_floats_per_tile); x0, bcs, truth,
// the save times and the RKC table are shared.  phys: [n_models] closure constants with dRi and Pr in the two pad floats (tile16's pullback reads
// them), filled by the host expression a single handle uses.
struct RtPhys;
struct T16Ens {
    const RtPhys* phys = nullptr;
    size_t w = 0, wf = 0, wb = 0, sf = 0, sb = 0, sol = 0, tape = 0, ztape = 0, dwtape = 0, slab = 0;
    int n_models = 1;
};
// The ensemble kernels keep the model description (with model k's constants patched in) at the head of their LDS: the forward kernel's bytes grow by this
static inline size_t t16_ens_forward_lds_extra() { return (size_t)MODEL_FLOATS * sizeof(float); }
hipError_t launch_pack_ens(const DevModel& m, const PackInfo& pk, const float* w, float* wf, float* wb, const T16Ens& en, hipStream_t stream);
hipError_t launch_pack_planes_ens(const DevModel& m, const float* w, unsigned* sf, unsigned* sb, const T16Ens& en, hipStream_t stream);
// true when an ensemble entry point exists for this forward geometry (weights in LDS at 1,024 threads; weights streamed at 256, or at 1,024 with rows in global memory)
bool forward_ens_has(bool wlds, int nthreads, bool ag);
// lds_bytes: the single handle's (the launcher adds t16_ens_forward_lds_extra); the grid is (tiles of n_col, n_models): the geometry of ONE model's columns
hipError_t launch_forward_ens(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* x0, const float* bcs,
                              const float* save_times, int n_save, int substeps, float* sol, float* tape, int n_col, int nthreads, bool wlds,
                              size_t lds_bytes, const T16Ens& en, hipStream_t stream, float* ztape);
// ... and for the taped adjoint of n_tiles tiles of ONE model (lds_bytes: as for launch_adjoint; m.ag says where the rows live)
bool adjoint_ens_has(const DevModel& m, int n_tiles, size_t lds_bytes);
// the taped-dW adjoint at 1,024 threads, the geometry launch_adjoint picks for one model's tiles (anything else: hipErrorInvalidValue)
hipError_t launch_adjoint_ens(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* wb, const int* bias_zoff,
                              const int* bias_goff, const float* bcs, const float* save_times, int n_save, int substeps, const float* sol,
                              const float* truth, const float* tape, const LossWeights& lw, float* slab, int n_col, size_t lds_bytes,
                              const T16Ens& en, hipStream_t stream, float* dwtape, const float* ztape);

// hidden pre-activation tape of the taped-dW mode: floats per column
static inline size_t t16_ztape_col_floats(const DevModel& m) { return (size_t)((m.n_nets * m.act_off[m.n_layers - 1] + 3) & ~3); }
hipError_t launch_infer(const DevModel& m, const PackInfo& pk, const float* w, const float* wf, const float* T,
                        const float* top_flux, float inv_dz, float* out, int n_col, int nthreads, size_t lds_bytes,
                        hipStream_t stream);
// flux-MLP pre-training (train_NN): one pass over the data set, one ADAM update per sample (update = 0: mean-loss evaluation only).
// pretrain_lds_bytes: the dynamic LDS of pretrain_kernel's carving (x, three activation-sized arrays, three face vectors, the reduction
// slots); launch_pretrain refuses above PRETRAIN_LDS_CAP, and set_kernel_attributes raises the kernel's limit to it.
#define PRETRAIN_LDS_CAP ((size_t)160 * 1024)
static inline size_t pretrain_lds_bytes(const DevModel& m) {
    return (size_t)(((m.ns + 3) & ~3) + 3 * (m.act_total + 4) + 3 * (m.Nz + 4) + 64) * sizeof(float);
}
hipError_t launch_pretrain(const DevModel& m, int flux_type, float* theta, float* mom, float* vel, const float* X, const float* BC,
                           const float* Y, const int* order, int n_samples, float gs, float eta, float b1, float b2, float eps,
                           double bt1, double bt2, int update, float* loss_out, double* bt_out, hipStream_t stream);
bool pick_adjoint_geom(const DevModel& m, AdjointGeom* geo, int force);
size_t lds_floats_adjoint_geom(const DevModel& m, const AdjointGeom& g);
hipError_t debug_read_stamps(unsigned long long* out16);
