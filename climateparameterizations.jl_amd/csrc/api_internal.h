// api_internal.h — what the translation units of the C ABI share (api.hip and api_{grad,ensemble,closure,substeps,embed}.hip): the handle and the pool
// that owns its device buffers, the error and timing plumbing, the environment switches, the helpers that cross files, and the staging of host arrays
// through one device scratch.  Not part of the public header; nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine_dwgemm.h"
#include "engine_tile16.h"
#include "engine_regtile.h"
#include "engine_netsplit.h"
#include "engine_fc.h"
#include "column_ops.h"
#include "engine_closure.h"
#include "engine_wm_infer.h"
#include "engine_wm_embed_any.h"
#include "engine_wm_profile.h"
#include "engine_fc_embed.h"
#include "engine_fc_pretrain.h"
#include "engine_wm_pretrain.h"
#include "step_schedule.h"
#include "member_loss.h"

#pragma GCC visibility push(hidden)

struct colnde_handle;

// ---- defined once, in api.hip ------------------------------------------------------------------------------
int fail(const char* fmt, ...);   // stores the thread-local message of colnde_last_error, returns 1
int validate(const colnde_config* c);
int open_device(int device);      // selects it; refuses anything but a gfx950
double stiff_lambda(const colnde_config* c);
RtPhys closure_constants(float nu0, float nu_minus, float dRi, float Ric, float Pr);
void build_model(const colnde_config* c, DevModel* m, PackInfo* pk);
int refresh_rkc(colnde_handle* h);
int refuse_unstable_substeps(const colnde_config* cfg);
int check_stability(const colnde_handle* h);
int refuse_auto_on_a_shard(const colnde_handle* h);
int user_params(const colnde_handle* h);
void loss_weights(const colnde_handle* h, const float scalings[6], LossWeights* lw);
int pack(colnde_handle* h, const float* d_weights);
int fc_pack(colnde_handle* h, const float* d_weights);
FcConv fc_conv_args(const colnde_handle* h);
FcConvEns fc_conv_ens_args(const colnde_handle* h);
int ensure_tmp(colnde_handle* h, size_t n_columns);
int ensure_ag(colnde_handle* h, size_t tiles);
void resolve_arithmetic(colnde_handle* h);
void drain_events(colnde_handle* h);
int forward_impl(colnde_handle* h, const float* d_weights, float* d_sol, bool with_tape);
int rt_forward_range(colnde_handle* h, float* d_sol, bool with_tape, int c0, int nc);
int t16_forward_range(colnde_handle* h, const float* d_weights, float* d_sol, bool with_tape, int c0, int nc);
int fc_forward_range(colnde_handle* h, float* d_sol, bool with_tape, int c0, int nc, int iv0 = 0, int iv1 = -1, int tape_iv0 = -1);
// ---- api_grad.hip, api_ensemble.hip, api_substeps.hip -------------------------------------------------------
// the dW GEMM of the taped gradient paths: h->dw planned for n_rec records (dw_plan.h), its two block lists uploaded into slots of h->mem (inside the
// caller's mark / rollback bracket), and the one place that launches it — K models: grid.y, their records and slab rows the strides apart
void build_dw_plan(colnde_handle* h, size_t n_rec);
void dw_slab_rows(colnde_handle* h);      // h->blk.rows (and the models' slab stride) for h->dw.slices
int replan_dw_slices(colnde_handle* h);    // colnde_set_matrix_arithmetic: the slice count, slab rows and slab of the arithmetic switched to
hipError_t upload_dw_plan(colnde_handle* h);
hipError_t dw_launch(colnde_handle* h, size_t n_records, float* slab_rows, int K = 1, size_t tape_mstride = 0, size_t slab_mstride = 0);
int fc_plan_tapes(colnde_handle* h);      // fc32's tapes: a single handle's at its first gradient, an ensemble's (K = h->n_models) at creation
// tile16's taped mode for K models of n_rec records each: delta tape, dW plan, slab and stage tape (*at = 1 when that one fails), then the Z tape
hipError_t t16_alloc_tapes(colnde_handle* h, size_t K, size_t n_rec, int* at);
hipError_t t16_alloc_ztape(colnde_handle* h, size_t K, size_t n_rec, bool rich);
// scalings == nullptr: under the handle's member loss (an ensemble on which colnde_ensemble_set_member_loss has set one)
int fc_loss_grad(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out);
colnde_config model_config(const colnde_config* cfg, const float* physics, int k);
int choose_substeps_impl(colnde_handle* h, const float* d_weights, float reltol, int* chosen, float* estimate);
int schedule_minima(const colnde_handle* h, std::vector<int>* minima);   // per save interval; an ensemble: the largest any model needs (api_substeps.hip)
int ens_replan_tapes(colnde_handle* h);   // an ensemble's tapes, planned at creation, re-planned for the step total in force (colnde_set_schedule)
// ---- defined in api_embed.hip: the handles the embedding's kernels cover (colnde_describe reports them) ------
bool wm_infer_covers(const colnde_handle* h);
bool wm_generic_serves(const colnde_handle* h);
bool fce_covers(const colnde_handle* h);

// Entry points that take ONE weight vector refuse an ensemble handle (colnde_create_ensemble)
#define SINGLE_MODEL_ONLY(h)                                                                                                              \
    do {                                                                                                                                  \
        if ((h) && (h)->closure)                                                                                                          \
            return fail("%s takes a weight vector, but this is a closure handle (no networks, %d constant sets): use colnde_closure_* (include/colnde.h)", \
                        __func__, (h)->n_models);                                                                                         \
        if ((h) && (h)->ensemble)                                                                                                         \
            return fail("%s takes one weight vector, but this handle holds an ensemble of %d models: use colnde_ensemble_* (include/colnde.h)", \
                        __func__, (h)->n_models);                                                                                         \
    } while (0)

// Entry points outside the conv handle's list (include/colnde.h, colnde_create_conv) refuse it: the network they would evaluate has no filter
#define PLAIN_NETWORK_ONLY(h)                                                                                                             \
    do {                                                                                                                                  \
        if ((h) && (h)->conv.c)                                                                                                           \
            return fail("%s does not cover the convolutional first layer of a colnde_create_conv handle (conv=%d): conv handles solve, "  \
                        "differentiate and train (forward, loss, loss_grad, loss_per_tstep, adam_step)", __func__, (h)->conv.c);          \
    } while (0)

// Entry points whose kernels read a 96-50-20-31 image or a net-split tape refuse a tile ensemble (colnde_create_tile_ensemble), naming themselves
#define NOT_A_TILE_ENSEMBLE(h)                                                                                                            \
    do {                                                                                                                                  \
        if ((h) && (h)->tile_ens)                                                                                                         \
            return fail("%s does not serve a tile ensemble (colnde_create_tile_ensemble, %d models on the tile16 kernels): its kernels read the "  \
                        "net-split weight image and tapes of colnde_create_ensemble", __func__, (h)->n_models);                           \
    } while (0)

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// the timing slots of colnde_kernel_time
enum { K_FORWARD = 0, K_ADJOINT = 1, K_REDUCE = 2, K_RHS = 3, K_INFER = 4, K_DW1 = 5, K_CONVADJ = 6, K_ADAM = 7, K_IMPLDIFF = 8, K_FCEMBED = 9, K_FLUXDIAG = 10, K_PROFILE = 11, K_COUNT = 12 };

struct PendingEvent { hipEvent_t a, b; int which; };

// ---- environment switches ------------------------------------------------------------------------------------
// Every variable some part of the library reads: colnde_describe reports from this list.  The ABI files read through env_get alone, so a switch read
// there is in the list by construction; the engine files read FC_CW, RT_FWD, T16_DWLDS, T16_TAPE_THREADS and T16_TAPE_WLDS themselves.
#define COLNDE_ENV_LIST(X)                                                                                                                  \
    X(FWD_SPLIT) X(ADJ_SPLIT) X(DW_SPLIT) X(ADJ_GEOM) X(FWD_WLDS) X(FWD_THREADS) X(T16_FWD_HELPER) X(T16_ADJ_HELPER) X(T16_FWD_SPLIT)         \
    X(T16_ADJ_SPLIT) X(FC) X(FC_CW) X(FC_EMBED_FUSED) X(FC_BLOCK) X(FC_SEG) X(WM_ENS_GRID) X(WM_GENERIC) X(WM_PROFILE_GRID) X(RT_ZTAPE) X(RT_BLOCK) X(RT_FWD) X(ALLOW_UNSTABLE_DT) \
    X(T16_DWTAPE) X(T16_ZTAPE) X(T16_SPLIT_RICH) X(T16_BLOCK) X(T16_DWLDS) X(T16_TAPE_THREADS) X(T16_TAPE_WLDS)
#define X(n) ENV_##n,
enum EnvSwitch { COLNDE_ENV_LIST(X) ENV_COUNT };
#undef X
const char* env_name(EnvSwitch s);
const char* env_get(EnvSwitch s);                                      // the raw string, or null when unset or empty
inline int env_int(EnvSwitch s, int unset) { const char* e = env_get(s); return e ? atoi(e) : unset; }
inline int env_flag(EnvSwitch s) { const char* e = env_get(s); return e ? atoi(e) != 0 : -1; }      // tape_plan.h's FLAG_UNSET / FLAG_OFF / FLAG_ON
inline bool allow_unstable() { return env_int(ENV_ALLOW_UNSTABLE_DT, 0) != 0; }

// ---- device memory -------------------------------------------------------------------------------------------
// The owner of every device buffer a handle keeps.  The handle still names its pointers (launch code reads them); the pool remembers where they live,
// so that colnde_destroy, a refused creator and a planner that fails half-way free exactly what was allocated and leave the slots null.
class DevPool {
    std::vector<void**> slots_;

  public:
    // hipMalloc of `count` elements into *slot (which must not hold a buffer).  A failure clears the sticky error and leaves *slot null.
    template <class T> hipError_t alloc(T** slot, size_t count) {
        const hipError_t e = hipMalloc((void**)slot, count * sizeof(T));
        if (e != hipSuccess) { (void)hipGetLastError(); *slot = nullptr; }
        else if (*slot) slots_.push_back((void**)slot);
        return e;
    }
    template <class T> void release(T** slot) {
        if (!*slot) return;
        (void)hipFree(*slot);
        *slot = nullptr;
        slots_.erase(std::remove(slots_.begin(), slots_.end(), (void**)slot), slots_.end());
    }
    template <class T> hipError_t resize(T** slot, size_t count) { release(slot); return alloc(slot, count); }
    // resize that allocates BEFORE it frees: a failure leaves *slot (which holds a buffer) and its contents as they were
    template <class T> hipError_t replace(T** slot, size_t count) {
        T* fresh = nullptr;
        const hipError_t e = hipMalloc((void**)&fresh, count * sizeof(T));
        if (e != hipSuccess || !fresh) { (void)hipGetLastError(); return e != hipSuccess ? e : hipErrorOutOfMemory; }
        (void)hipFree(*slot);
        *slot = fresh;
        return hipSuccess;
    }
    size_t mark() const { return slots_.size(); }
    void rollback(size_t mark) {            // frees what was allocated since mark(), newest first (nothing may be released in between)
        while (slots_.size() > mark) {
            (void)hipFree(*slots_.back());
            *slots_.back() = nullptr;
            slots_.pop_back();
        }
    }
    void free_all() { rollback(0); }
};

// Device scratch of one call: freed when the call returns, after the work queued on the stream has drained
struct DevScratch {
    hipStream_t stream;
    float* p = nullptr;
    explicit DevScratch(hipStream_t s) : stream(s) {}
    DevScratch(const DevScratch&) = delete;
    hipError_t alloc(size_t bytes) { return hipMalloc((void**)&p, bytes); }
    ~DevScratch() {
        if (!p) return;
        (void)hipStreamSynchronize(stream);
        (void)hipFree(p);
    }
};

// colnde_create_conv: the filter in front of the plain fc32 network the handle holds in `m`
struct ConvBlock {
    int c = 0;                      // taps (0: not a conv handle)
    int n_params = 0;               // the user's parameter count: c + 1 + (plain count) - 4Nz (c - 1)
    int w1_end = 0, n_zero = 0;     // padded vector: W1's 4Nz M user entries end here, followed by 4Nz (c - 1) zeros
    const float* d_user = nullptr;  // the user's vector of the call in flight (the filter leads it)
    float* d_wpad = nullptr;        // [m.n_params] the padded vector the engine packs
    float* d_gpad = nullptr;        // [m.n_params + 8] the padded result of the reduction, folded into the user's layout
    float* d_ctape = nullptr;       // [record][16][2 Nz] stage inputs and filter cotangents (planned with the other tapes)
    float* d_cslab = nullptr;       // [block][segment][FC_CONV_GRAD_MAX_SLICES][FC_CONV_GRAD_SLOTS] the filter gradient's partial sums
    int cslab_rows = 0;
    size_t ctape_stride = 0, cslab_stride = 0;   // a conv ensemble: floats from one model's conv tape / filter slab to the next's (d_wpad: m.n_params, d_gpad: + 8)
};

struct colnde_handle {
    DevPool mem;                    // owns every d_* below
    colnde_config cfg;
    ConvBlock conv;
    std::vector<float> save_times;
    DevModel m;
    PackInfo pk;
    AdjointGeom geo;
    bool geo_ok = false;
    int device = 0;
    hipStream_t stream = nullptr;
    int n_col = 0, n_tiles = 0;
    int64_t n_col_total = 0;
    size_t lds_fwd = 0, lds_adj = 0, lds_fwd_solve = 0;
    int fwd_threads = 256;
    bool fwd_wlds = false;
    bool adj_helper = true;         // ... and in the adjoint: a helper wave carries λ, x̄ and the physics pullback for the three net waves
    bool fwd_helper = true;         // ... four waves per tile: a helper wave evaluates the Richardson-number closure for the three net waves
    bool split_rich = false;        // ... with the rich tape (activations, derivatives, physics coefficients) in place of the pre-activation tape
    bool adj_split = false;         // ... and the gradient by rt16s_adjoint_kernel + tile16's dW GEMM
    bool fwd_split = false;         // forward solves by the net-split kernels (rt16sh_forward_kernel: three net waves + a helper wave per tile)
    bool use_rt = false;            // register-resident tile engine (static 96-50-20-31 wind-mixing shape)
    bool sp_fwd = true, sp_adj = true, sp_dw = true;   // matrix arithmetic of the forward-solve / adjoint / weight-gradient kernels: exact three-way bf16 split (true) or
                                                      // f32 MFMA — cfg.matrix_arithmetic with the test overrides COLNDE_{FWD,ADJ,DW}_SPLIT (resolve_arithmetic)
    bool use_fc = false;            // 32-column free-convection engine (engine_fc.hip: Nz = 32 | 64, the reference's relu network, RK4)
    bool fce_ready = false;         // colnde_fc_embedded_step / colnde_fc_diagnose_wT: images allocated, LDS limits raised (first call)
    // colnde_ensemble_fc_embedded: the members' forward images, biases and filters at tile width 16, kept from one call to the next (weights == NULL
    // reuses them); allocated and the LDS limits raised on the first call, fce_ens_packed once a call has given weights
    bool fce_ens_ready = false, fce_ens_packed = false;
    float *d_fce_ens_imgf = nullptr, *d_fce_ens_bias = nullptr, *d_fce_ens_taps = nullptr;    float *d_fc_imgf = nullptr, *d_fc_imgb = nullptr, *d_fc_bias = nullptr;
    unsigned int *d_fc_simgf = nullptr, *d_fc_simgb = nullptr;   // the split operand images (COLNDE_MATRIX_BF16X3_EXACT; 32-column tiles)
    unsigned int* d_fc_masks = nullptr;
    unsigned long long* d_fc_switch = nullptr;   // ConvectiveAdjustmentNDE: the taped switch patterns
    int fc_seg = 0, fc_nseg = 0;                      // gradient path: save intervals per time segment of the tapes, segments (1: the tapes hold the whole axis)
    int fc_cw = 32;                                   // columns per workgroup tile: 32, or 16 for problems of at most 4,096 columns (fc_tile_width)
    float* d_fc_lam = nullptr;                        // λ handed from one time segment to the one before it
    float* d_wimg = nullptr;
    float *d_rt_tape = nullptr, *d_rt_tape2 = nullptr, *d_rt_slab = nullptr, *d_rt_tapez = nullptr;
    bool rt_fwd32 = false;         // COLNDE_RT_FWD=32 at creation: the 32-column forward kernel (no Z1 tape)
    bool rt_ztape = false;         // layer-1 pre-activations taped by the forward kernel instead of recomputed by the adjoint
    // the gradient path of the handle's engine: columns per pass (whole tiles: the tapes hold one block at a time), passes, partial-gradient slab rows
    struct { int block = 0, nblocks = 0, rows = 0; } blk;
    float *d_w = nullptr, *d_wf = nullptr, *d_wb = nullptr, *d_x0 = nullptr, *d_bcs = nullptr, *d_truth = nullptr,
          *d_sol = nullptr, *d_tape = nullptr, *d_slab = nullptr, *d_out = nullptr, *d_times = nullptr,
          *d_partial = nullptr, *d_tmp_a = nullptr, *d_tmp_b = nullptr, *d_tmp_c = nullptr;
    size_t tmp_cols = 0;
    TileDesc* d_tiles = nullptr;
    // tile16 taped-dW mode (networks whose weight-gradient tiles overflow the register file)
    int t16_dwtape = -1;            // -1 undecided, 0 off, 1 on
    float* d_dwtape = nullptr;
    float* d_t16_ztape = nullptr;   // taped mode: hidden pre-activations written by the forward kernel (the adjoint skips its forward GEMMs)
    DwPlan dw;                      // the dW GEMM's plan, built with the tapes' (build_dw_plan); its split passes run when sp_dw
    size_t dw_n_rec = 0;            // ... the records it was planned for (replan_dw_slices plans the slices again when the arithmetic changes)
    DwMacro *d_macros = nullptr, *d_split_macros = nullptr;   // ... and the device copies of its two block lists (the split one: null without a split plan)
    int *d_bias_zoff = nullptr, *d_bias_goff = nullptr;
    bool have_problem = false, have_truth = false;
    bool prof = false;
    int min_substeps = 1;           // least RK4 sub-steps per save interval inside the diffusive stability bound
    bool auto_substeps = false;     // cfg.substeps = 0 at creation: the first solve call chooses the sub-step count from cfg.reltol (choose_substeps)
    float last_estimate = -1.0f;    // ... and the error estimate it settled on
    unsigned* d_sf = nullptr;       // DevModel::sf / sb: bf16 plane images of the dense chains (networks with rows in global memory, BF16X3_EXACT)
    unsigned* d_sb = nullptr;
    float* d_ag = nullptr;          // DevModel::ag: per-tile activation / delta rows in global memory (networks whose rows do not fit the LDS)
    size_t ag_tiles = 0;            // ... tiles it holds
    std::vector<float> rkc_host;    // host copy of the RKC2 coefficient table in use (refresh_rkc)
    bool ag_rows = false;           // the tile16 kernels keep the activation rows in global memory (DevModel::ag)
    bool substeps_chosen = false;   // the count in use came out of choose_substeps_impl (colnde_describe says so, with the estimate)
    // step schedule (colnde_set_schedule; step_schedule.h): RK4 steps per save interval in cfg.substeps' place — empty: none — and its device copy
    std::vector<int> sched;
    int* d_sched = nullptr;         // [n_save - 1], allocated by the first colnde_set_schedule
    float* d_rkc = nullptr;         // RKC2 coefficient table (DevModel::rkc)
    // ensembles (colnde_create_ensemble): n_models models of this configuration in one launch per kernel (blockIdx.y = model)
    bool ensemble = false;
    int n_models = 1;
    std::vector<RtPhys> phys_host;  // per-model closure constants (closure_constants), and their device copy
    RtPhys* d_phys = nullptr;
    std::vector<float> phys_raw;    // ... as given: [n_models][5] {nu0, nu_minus, dRi, Ric, Pr} (empty: cfg's constants for every model)
    MppParams* d_wm_ens_mpp = nullptr;          // colnde_ensemble_wm_embedded: the per-model sweep constants on the device, and what they hold
    std::vector<MppParams> wm_ens_mpp_host;
    RtPhys* d_prof_phys = nullptr;  // colnde_ensemble_profile: the closure constants of a call that overrides the handle's (physics != NULL)
    RtEns ens;                      // per-model strides of the buffers a model owns
    bool tile_ens = false;          // colnde_create_tile_ensemble: the K models run tile16's own kernels (any architecture), at the strides of ...
    T16Ens tens;
    FcEns fens;                     // ... of a free-convection ensemble (colnde_create_fc_ensemble): the fc32 kernels' strides
    size_t ens_model_bytes = 0;     // device bytes per model (tapes, slab rows, solution, weight image)
    int ens_rkc_stages = 0;         // RKC2, automatic stage count: the largest any model needs (refresh_rkc)
    // member loss (colnde_ensemble_set_member_loss; member_loss.h): what the caller gave, and the device arrays the member kernels read — the K
    // LossWeights rows and the K x n_col column weights (ones where the caller gave none), allocated by the first call that sets one
    bool ml_scalings = false, ml_columns = false;
    LossWeights* d_ml_lw = nullptr;
    float* d_ml_cw = nullptr;
    // closure-only model (colnde_create_closure): n_models constant sets of the Pacanowski-Philander closure, no networks (engine_closure.hip)
    bool closure = false;
    ClosureModel cm = {};
    float *d_cl_tape = nullptr, *d_cl_rows = nullptr, *d_cl_params = nullptr;
    size_t cl_tape_bytes = 0;
    std::vector<PendingEvent> pending;
    double ms[K_COUNT] = {};
    int launches[K_COUNT] = {};
};

// The engine a handle runs, as colnde_engine and colnde_plan report it
inline int engine_id(const colnde_handle* h) { return h->use_rt ? COLNDE_ENGINE_MFMA : h->use_fc ? COLNDE_ENGINE_FC32 : COLNDE_ENGINE_GENERIC; }
// The steps of the whole time axis — what sizes the tapes, the slab rows' dW records and the kernels' tape strides: the one place that forms it
inline int total_steps(const colnde_handle* h) {
    return (int)sched_total(h->sched.empty() ? nullptr : h->sched.data(), h->cfg.n_save - 1, h->cfg.substeps);
}
// ... and the schedule argument of the net-split launches (null: cfg.substeps in every interval)
inline const int* sched_dev(const colnde_handle* h) { return h->sched.empty() ? nullptr : h->d_sched; }

// times the launches of its scope into slot `which` when the handle profiles (colnde_set_profiling)
struct Timed {
    colnde_handle* h;
    PendingEvent p;
    bool on;
    Timed(colnde_handle* h_, int which) : h(h_), on(h_->prof) {
        if (!on) return;
        p.which = which;
        if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(p.a, h->stream);
    }
    ~Timed() {
        if (!on) return;
        (void)hipEventRecord(p.b, h->stream);
        h->pending.push_back(p);
        if (h->pending.size() > 2048) drain_events(h);
    }
};

// ---- host-array twins: one device scratch per call --------------------------------------------------------
// A twin declares its arrays in the order they are copied, calls upload(), its _dev form on the device pointers it was given, and download():
//     HostStage st(h, "label");  st.to(h->d_w, weights, n);  st.in(&d_x, x, nx);  st.out(&d_y, y, ny);
//     if (st.upload()) return 1;  if (..._dev(h, h->d_w, d_x, d_y)) return 1;  return st.download();
// One hipMalloc holds every block, each on a 16-byte boundary (what the kernels ask of their arrays).  An array whose host pointer is null takes
// no room and its device pointer is null.  The first copy that fails leaves "<label>: host-to-device copy failed" / "<label>: device-to-host copy
// failed"; a failing _dev call keeps its own message.  However the twin returns, the stream is synchronised and the scratch freed.
class HostStage {
    struct Block { float *fixed, **d_src, **d_dst; const float* src; float* dst; size_t n, off; };
    colnde_handle* h_;
    const char* label_;
    std::vector<Block> blocks_;
    size_t total_ = 0;          // floats
    float* base_ = nullptr;

    void add(float** d_src, float** d_dst, const float* src, float* dst, size_t n) {
        if (d_src) *d_src = nullptr;
        if (d_dst) *d_dst = nullptr;
        if (!src && !dst) return;
        blocks_.push_back({nullptr, d_src, d_dst, src, dst, n, total_});
        total_ += (n + 3) / 4 * 4;
    }

  public:
    HostStage(colnde_handle* h, const char* label) : h_(h), label_(label) {}
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;
    ~HostStage() {
        if (!base_) return;
        (void)hipStreamSynchronize(h_->stream);
        (void)hipFree(base_);
    }
    // an input that goes to a buffer the handle owns (the weights to h->d_w), in order with the others
    void to(float* d_dst, const float* src, size_t n) { blocks_.push_back({d_dst, nullptr, nullptr, src, nullptr, n, 0}); }
    void in(float** d, const float* src, size_t n) { add(d, nullptr, src, nullptr, n); }
    void out(float** d, float* dst, size_t n) { add(nullptr, d, nullptr, dst, n); }
    // one block, uploaded from src and downloaded to dst: the call works in place on it.  *d_dst is null without dst (input only).
    void inout(float** d_src, float** d_dst, const float* src, float* dst, size_t n) { add(d_src, d_dst, src, dst, n); }

    int upload() {
        HIPCHK(hipMalloc((void**)&base_, total_ * sizeof(float)));
        bool ok = true;
        for (const Block& b : blocks_) {
            float* d = b.fixed ? b.fixed : base_ + b.off;
            if (b.d_src && b.src) *b.d_src = d;
            if (b.d_dst && b.dst) *b.d_dst = d;
            if (ok && b.src) ok = hipMemcpyAsync(d, b.src, b.n * sizeof(float), hipMemcpyHostToDevice, h_->stream) == hipSuccess;
        }
        return ok ? 0 : fail("%s: host-to-device copy failed", label_);
    }
    int download() {
        bool ok = true;
        for (const Block& b : blocks_)
            if (ok && b.dst) ok = hipMemcpyAsync(b.dst, base_ + b.off, b.n * sizeof(float), hipMemcpyDeviceToHost, h_->stream) == hipSuccess;
        return ok && hipStreamSynchronize(h_->stream) == hipSuccess ? 0 : fail("%s: device-to-host copy failed", label_);
    }
};

#pragma GCC visibility pop
