// api_embed.hip — the embedding's part of the C ABI (include/colnde.h): inference, the steps either side of it, the wind-mixing and free-convection
// embedded steps and the saved-state flux diagnoses.  Host code only; the kernels are column_ops.hip, engine_wm_infer.hip, engine_fc_embed.hip.
#include "api_internal.h"

// ---- embedded inference --------------------------------------------------------------------------------
// sign = +1: the forcing -dz(wT); -1: +dz(wT), what the reference stores in params.∂z_wT_NN (double_gyre_nn.jl:165)
static int infer_impl(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux, float Lz, float* d_out, int n_columns, float sign);
extern "C" int colnde_infer_forcing_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux,
                                        float Lz, float* d_out, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    return infer_impl(h, d_weights, d_T, d_top_flux, Lz, d_out, n_columns, 1.0f);
}
extern "C" int colnde_infer_dz_wT_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux,
                                      float Lz, float* d_out, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    return infer_impl(h, d_weights, d_T, d_top_flux, Lz, d_out, n_columns, -1.0f);
}
static int infer_impl(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux, float Lz, float* d_out, int n_columns, float sign) {
    if (!h) return fail("null handle");
    if (!d_weights || !d_T || !d_top_flux || !d_out) return fail("null pointer argument");
    if (h->m.model == COLNDE_MODEL_WIND_MIXING) return fail("infer_forcing needs a single T-only network (free-convection model)");
    if (n_columns < 1 || !(Lz > 0.0f)) return fail("n_columns >= 1 and Lz > 0 required");
    HIPCHK(hipSetDevice(h->device));
    if (h->use_fc && h->m.model == COLNDE_MODEL_FREE_CONVECTION) {
        // the reference's forcing network IS the fc32 shape (32-128-128-31 in double_gyre_nn.jl): the 32-column engine's sections, one evaluation
        const int cw = fc_tile_width(n_columns);                 // (the images are packed per call: this call's own tile width)
        hipError_t ef = fc_launch_pack(h->m, cw, d_weights, h->d_fc_imgf, h->d_fc_imgb, h->d_fc_bias, nullptr, nullptr, h->stream);
        if (ef != hipSuccess) return fail("fc32 pack launch failed: %s", hipGetErrorString(ef));
        Timed tm(h, K_INFER);
        ef = fc_launch_infer(h->m, cw, h->d_fc_imgf, h->d_fc_bias, d_T, d_top_flux, sign * (float)h->m.Nz / Lz, d_out, n_columns, h->stream);
        if (ef != hipSuccess) return fail("fc32 infer launch failed: %s", hipGetErrorString(ef));
        return 0;
    }
    if (pack(h, d_weights)) return 1;
    Timed tm(h, K_INFER);
    hipError_t e = launch_infer(h->m, h->pk, d_weights, h->d_wf, d_T, d_top_flux, sign * (float)h->m.Nz / Lz, d_out, n_columns, 256,
                                h->lds_fwd, h->stream);
    if (e != hipSuccess) return fail("infer launch failed: %s", hipGetErrorString(e));
    return 0;
}

static int infer_host(colnde_handle* h, const float* weights, const float* T, const float* top_flux, float Lz, float* out, int n_columns, float sign);
extern "C" int colnde_infer_forcing(colnde_handle* h, const float* weights, const float* T, const float* top_flux, float Lz,
                                    float* out, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    return infer_host(h, weights, T, top_flux, Lz, out, n_columns, 1.0f);
}
extern "C" int colnde_infer_dz_wT(colnde_handle* h, const float* weights, const float* T, const float* top_flux, float Lz,
                                  float* out, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    return infer_host(h, weights, T, top_flux, Lz, out, n_columns, -1.0f);
}
static int infer_host(colnde_handle* h, const float* weights, const float* T, const float* top_flux, float Lz, float* out, int n_columns, float sign) {
    if (!h) return fail("null handle");
    if (!weights || !T || !top_flux || !out) return fail("null pointer argument");
    if (n_columns < 1) return fail("n_columns must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    if (ensure_tmp(h, (size_t)n_columns)) return 1;
    const int Nz = h->m.Nz;
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * h->m.n_params, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_tmp_a, T, sizeof(float) * (size_t)n_columns * Nz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_tmp_b, top_flux, sizeof(float) * (size_t)n_columns, hipMemcpyHostToDevice, h->stream));
    if (infer_impl(h, h->d_w, h->d_tmp_a, h->d_tmp_b, Lz, h->d_tmp_c, n_columns, sign)) return 1;
    HIPCHK(hipMemcpyAsync(out, h->d_tmp_c, sizeof(float) * (size_t)n_columns * Nz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- the steps either side of the hot path ---------------------------------------------------
extern "C" int colnde_convective_adjustment_dev(colnde_handle* h, const float* d_T, const float* d_halo_bottom,
                                                const float* d_halo_top, float dt, float dz, float K, float* d_out, int n_columns) {
    if (!h) return fail("null handle");
    if (!d_T || !d_out) return fail("null pointer argument");
    if (n_columns < 1) return fail("n_columns must be >= 1");
    if (!(dt > 0.0f) || !(dz > 0.0f) || !(K >= 0.0f)) return fail("dt > 0, dz > 0 and K >= 0 required");
    if (h->m.Nz < 2 || h->m.Nz > 128) return fail("convective adjustment supports 2 <= Nz <= 128 (Nz = %d)", h->m.Nz);
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_CONVADJ);
    hipError_t e = launch_convective_adjustment(d_T, d_halo_bottom, d_halo_top, dt / (dz * dz), K, d_out, h->m.Nz, n_columns, h->stream);
    if (e != hipSuccess) return fail("convective adjustment launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_convective_adjustment(colnde_handle* h, const float* T, const float* halo_bottom, const float* halo_top,
                                            float dt, float dz, float K, float* out, int n_columns) {
    if (!h) return fail("null handle");
    if (!T || !out) return fail("null pointer argument");
    if (n_columns < 1) return fail("n_columns must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    if (ensure_tmp(h, (size_t)n_columns)) return 1;
    const int Nz = h->m.Nz;
    HIPCHK(hipMemcpyAsync(h->d_tmp_a, T, sizeof(float) * (size_t)n_columns * Nz, hipMemcpyHostToDevice, h->stream));
    float* d_hb = nullptr;
    float* d_ht = nullptr;
    if (halo_bottom) {
        d_hb = h->d_tmp_b;
        HIPCHK(hipMemcpyAsync(d_hb, halo_bottom, sizeof(float) * (size_t)n_columns, hipMemcpyHostToDevice, h->stream));
    }
    if (halo_top) {
        d_ht = h->d_tmp_b + n_columns;
        HIPCHK(hipMemcpyAsync(d_ht, halo_top, sizeof(float) * (size_t)n_columns, hipMemcpyHostToDevice, h->stream));
    }
    if (colnde_convective_adjustment_dev(h, h->d_tmp_a, d_hb, d_ht, dt, dz, K, h->d_tmp_c, n_columns)) return 1;
    HIPCHK(hipMemcpyAsync(out, h->d_tmp_c, sizeof(float) * (size_t)n_columns * Nz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// modified_pacanowski_philander! (wind_mixing/src/NDE_oceananigans.jl:61-101): one implicit diffusion step of u, v, T per column
static int impl_diff_check(colnde_handle* h, const void* a, const void* b, const void* c, const void* d, const void* e, const void* f,
                           float dt, float dz, const float params[7], int n_columns) {
    if (!h) return fail("null handle");
    if (!a || !b || !c || !d || !e || !f || !params) return fail("null pointer argument");
    if (n_columns < 1) return fail("n_columns must be >= 1");
    if (!(dt > 0.0f) || !(dz > 0.0f)) return fail("dt > 0 and dz > 0 required");
    if (!(params[0] >= 0.0f) || !(params[1] >= 0.0f)) return fail("nu0 >= 0 and nu_minus >= 0 required (the tridiagonal must stay diagonally dominant)");
    if (!(params[2] != 0.0f) || !(params[4] > 0.0f)) return fail("dRi != 0 and Pr > 0 required");
    if (h->m.Nz < 2 || h->m.Nz > 128) return fail("implicit diffusion supports 2 <= Nz <= 128 (Nz = %d)", h->m.Nz);
    return 0;
}

extern "C" int colnde_implicit_diffusion_dev(colnde_handle* h, const float* d_u, const float* d_v, const float* d_T,
                                             const float* d_halo_bottom, float dt, float dz, const float params[7],
                                             int convective_adjustment, float* d_u_out, float* d_v_out, float* d_T_out, int n_columns) {
    if (impl_diff_check(h, d_u, d_v, d_T, d_u_out, d_v_out, d_T_out, dt, dz, params, n_columns)) return 1;
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_IMPLDIFF);
    hipError_t e = launch_mpp_diffusion(d_u, d_v, d_T, d_halo_bottom, dt, dz, params, convective_adjustment, d_u_out, d_v_out, d_T_out,
                                        h->m.Nz, n_columns, h->stream);
    if (e != hipSuccess) return fail("implicit diffusion launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_implicit_diffusion(colnde_handle* h, const float* u, const float* v, const float* T, const float* halo_bottom,
                                         float dt, float dz, const float params[7], int convective_adjustment, float* u_out,
                                         float* v_out, float* T_out, int n_columns) {
    if (impl_diff_check(h, u, v, T, u_out, v_out, T_out, dt, dz, params, n_columns)) return 1;
    HIPCHK(hipSetDevice(h->device));
    const size_t nf = (size_t)n_columns * h->m.Nz;
    HostStage st(h, "implicit diffusion");       // a scratch of its own — the handle's are sized for its own state vector
    const float* src[3] = {u, v, T};
    float *dst[3] = {u_out, v_out, T_out}, *d_s[3], *d_o[3], *d_hb;
    for (int f = 0; f < 3; f++) st.inout(&d_s[f], &d_o[f], src[f], dst[f], nf);
    st.in(&d_hb, halo_bottom, 3 * (size_t)n_columns);
    if (st.upload()) return 1;
    if (colnde_implicit_diffusion_dev(h, d_s[0], d_s[1], d_s[2], d_hb, dt, dz, params, convective_adjustment, d_o[0], d_o[1], d_o[2], n_columns)) return 1;
    return st.download();
}

// a network as the refusals print it: 96-50-20-31
static std::string layer_sizes_string(const colnde_config& c) {
    std::string s;
    for (int l = 0; l <= c.n_layers; l++) s += (l ? "-" : "") + std::to_string(c.layer_sizes[l]);
    return s;
}

// ---- wind-mixing embedded inference (wind_mixing/src/NDE_oceananigans.jl:288-329, :380-405; engine_wm_infer.hip) ----------------------
// The configurations the kernels cover: 0 when h's is one.  Otherwise 1, and with fn (the entry point's name) the refusal is left as the message.
static int wm_shape_check(const colnde_handle* h, const char* fn) {
    const colnde_config& c = h->cfg;
    const bool shape = c.Nz == WM_NZ && c.n_layers == 3 && c.layer_sizes[0] == 3 * WM_NZ && c.layer_sizes[1] == WM_H1 && c.layer_sizes[2] == WM_H2 &&
                       c.layer_sizes[3] == WM_NZ - 1 && c.activations[2] == COLNDE_ACT_IDENTITY;
    if (c.model == COLNDE_MODEL_WIND_MIXING && !c.smooth_NN && shape) return 0;
    if (!fn) return 1;
    if (c.model != COLNDE_MODEL_WIND_MIXING)
        return fail("%s needs a wind-mixing handle (three flux networks on [u; v; T]); a free-convection handle has colnde_infer_forcing", fn);
    if (c.smooth_NN)
        return fail("%s: the embedding has no smoothing filter (NDE_oceananigans.jl:288-329 apply the networks unfiltered), so a handle with smooth_NN is refused", fn);
    // (the unified call serves other layer sizes itself: only the older entry points point at it)
    const bool unified = !strncmp(fn, "colnde_ensemble_wm_embedded", 27);
    return fail("%s covers Nz = 32 with three 96-50-20-31 networks and an identity output layer; this handle has Nz = %d, networks %s, output activation %d%s", fn,
                c.Nz, layer_sizes_string(c).c_str(), c.activations[c.n_layers - 1],
                unified ? "" : "; colnde_ensemble_wm_embedded deploys a single handle of any layer sizes 96-...-31 at Nz = 32 as K = 1");
}
// the handles the single-model entry points cover
bool wm_infer_covers(const colnde_handle* h) { return !h->closure && !h->ensemble && !wm_shape_check(h, nullptr); }

// ---- networks of any trained architecture (engine_wm_embed_any.hip: wm_embed_any_kernel) --------------------------------------------
static_assert(WMA_MAX_LAYERS == COLNDE_MAX_LAYERS && WMA_NZ == WM_NZ, "engine_wm_embed_any.h restates these");
// a single wind-mixing handle at Nz = 32 whose three nets are 96-...-31, whatever lies between; the fixed shape only under COLNDE_WM_GENERIC=1 (the
// kernel-against-kernel tests), the persistent kernel otherwise
static bool wm_generic_shape(const colnde_handle* h) {
    const colnde_config& c = h->cfg;
    return !h->closure && !h->ensemble && !h->conv.c && c.model == COLNDE_MODEL_WIND_MIXING && !c.smooth_NN && c.Nz == WM_NZ && c.n_layers >= 1 &&
           c.layer_sizes[0] == 3 * WM_NZ && c.layer_sizes[c.n_layers] == WM_NZ - 1 && (wm_shape_check(h, nullptr) || env_int(ENV_WM_GENERIC, 0) != 0);
}
static WmAnyPlan wm_generic_plan(const colnde_handle* h) { return wm_any_plan(h->cfg.n_layers, h->cfg.layer_sizes); }
// ... and whose LDS plan fits: the handles colnde_ensemble_wm_embedded sends to the generic kernel (colnde_describe: wm_embed=generic_f32)
bool wm_generic_serves(const colnde_handle* h) { return wm_generic_shape(h) && wm_any_fits(wm_generic_plan(h)); }

// One call of the wind-mixing embedding as its entry point received it: what it reads and writes (engine_wm_infer.h: the optional groups of the
// record choose the fused step and the face diagnosis) and what is the call's own.  params: seven constants — an ensemble call: [K][7], or null for
// the handle's own.
struct WmCall {
    WmEmbedIO io;
    const float* weights;
    float dt;                             // the step's
    const float* params;                  // the step's and the diagnosis'
    int ca;
};
// what every call has; the entry points add their groups by name
static WmCall wm_call(const float* weights, const float* u, const float* v, const float* T, const float* top_flux, float Lz, int n_columns) {
    WmCall c = {};
    c.weights = weights; c.io.u = u; c.io.v = v; c.io.T = T; c.io.top_flux = top_flux; c.io.Lz = Lz; c.io.n_col = n_columns;
    return c;
}
static void wm_dz_group(WmCall* c, float* dz_uw, float* dz_vw, float* dz_wT) { c->io.dz_uw = dz_uw; c->io.dz_vw = dz_vw; c->io.dz_wT = dz_wT; }
static void wm_step_group(WmCall* c, float* u_out, float* v_out, float* T_out) { c->io.u_out = u_out; c->io.v_out = v_out; c->io.T_out = T_out; }
static void wm_face_group(WmCall* c, float* uw, float* vw, float* wT) { c->io.uw = uw; c->io.vw = vw; c->io.wT = wT; }
static void wm_physics(WmCall* c, const float* halo_bottom, const float* halo_top, float dt, const float* params, int ca) {
    c->io.halo_bottom = halo_bottom; c->io.halo_top = halo_top; c->dt = dt; c->params = params; c->ca = ca;
}

// (its callers have refused ensembles and closure handles: SINGLE_MODEL_ONLY); fn names the entry point in the refusal.  dz, faces: the call
// writes the d/dz arrays, the face arrays
static int wm_infer_check(colnde_handle* h, const char* fn, const WmCall& c, bool dz, bool faces) {
    const WmEmbedIO& io = c.io;
    if (!h) return fail("null handle");
    if (wm_shape_check(h, fn)) return 1;
    if (!c.weights || !io.u || !io.v || !io.T || !io.top_flux) return fail("null pointer argument");
    if (dz && (!io.dz_uw || !io.dz_vw || !io.dz_wT)) return fail("null pointer argument");
    if (faces && (!io.uw || !io.vw || !io.wT)) return fail("null pointer argument");
    if (io.n_col < 1 || !(io.Lz > 0.0f)) return fail("n_columns >= 1 and Lz > 0 required");
    return 0;
}
static int wm_step_check(colnde_handle* h, const WmCall& c) {
    const WmEmbedIO& io = c.io;
    return impl_diff_check(h, io.u, io.v, io.T, io.u_out, io.v_out, io.T_out, c.dt, io.Lz / (float)WM_NZ, c.params, io.n_col);
}
// the scalings and hidden activations the kernels take from the configuration: WmInferArgs and WmEnsArgs
template <class Args>
static void wm_scalings(const colnde_handle* h, Args* a) {
    for (int i = 0; i < 6; i++) { a->mu[i] = h->cfg.mu[i]; a->sigma[i] = h->cfg.sigma[i]; }
    a->act1 = h->cfg.activations[0];
    a->act2 = h->cfg.activations[1];
}

// The one launch behind the four single-model entry points.  `what` names the call in the launch failure.
static int wm_launch(colnde_handle* h, int slot, const char* what, const WmCall& c) {
    HIPCHK(hipSetDevice(h->device));
    WmInferArgs a = {};
    wm_scalings(h, &a);
    a.io = c.io;
    a.weights = c.weights;
    const float dz = c.io.Lz / (float)WM_NZ;
    if (a.io.fused() || a.io.diag()) a.mpp = mpp_params(c.params, a.io.fused() ? c.dt : dz * dz, dz, c.ca);      // (the diagnosis alone takes no step: c is not read)
    Timed tm(h, slot);
    hipError_t e = launch_wm_infer(a, h->stream);
    if (e != hipSuccess) return fail("%s launch failed: %s (the state and output arrays must be 16-byte aligned)", what, hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_wm_infer_dz_flux_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T,
                                           const float* d_top_flux, float Lz, float* d_dz_uw, float* d_dz_vw, float* d_dz_wT, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    WmCall c = wm_call(d_weights, d_u, d_v, d_T, d_top_flux, Lz, n_columns);
    wm_dz_group(&c, d_dz_uw, d_dz_vw, d_dz_wT);
    if (wm_infer_check(h, __func__, c, true, false)) return 1;
    return wm_launch(h, K_INFER, "wm_infer", c);
}

extern "C" int colnde_wm_embedded_step_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T,
                                           const float* d_top_flux, const float* d_halo_bottom, float Lz, float dt, const float params[7],
                                           int convective_adjustment, float* d_dz_uw, float* d_dz_vw, float* d_dz_wT, float* d_u_out, float* d_v_out,
                                           float* d_T_out, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    WmCall c = wm_call(d_weights, d_u, d_v, d_T, d_top_flux, Lz, n_columns);
    wm_physics(&c, d_halo_bottom, nullptr, dt, params, convective_adjustment);
    wm_dz_group(&c, d_dz_uw, d_dz_vw, d_dz_wT);
    wm_step_group(&c, d_u_out, d_v_out, d_T_out);
    if (wm_infer_check(h, __func__, c, true, false)) return 1;
    if (wm_step_check(h, c)) return 1;
    return wm_launch(h, K_INFER, "wm_embedded_step", c);
}
// ---- the saved-state flux diagnoses of the wind-mixing embedding (NDE_oceananigans.jl:157-191, :226-286) ---------------------------------
// the device calls that write the faces; step: the d/dz arrays and u_out, v_out, T_out with them
static int wm_diag_check(colnde_handle* h, const char* fn, const WmCall& c, bool step) {
    const WmEmbedIO& io = c.io;
    if (!h) return fail("null handle");
    if (wm_shape_check(h, fn)) return 1;
    if (!io.u || !io.v || !io.T || !io.uw || !io.vw || !io.wT) return fail("null pointer argument");
    if (step && (!io.dz_uw || !io.dz_vw || !io.dz_wT || !io.u_out || !io.v_out || !io.T_out)) return fail("null pointer argument");
    if (io.n_col < 1 || !(io.Lz > 0.0f)) return fail("n_columns >= 1 and Lz > 0 required");
    if (!c.params) return fail("null pointer argument");
    if (!(c.params[2] != 0.0f) || !(c.params[4] > 0.0f)) return fail("dRi != 0 and Pr > 0 required");
    if (!wm_io_aligned(io, true)) return fail("%s: the state and output arrays must be 16-byte aligned", fn);
    if (!c.weights || !io.top_flux) return fail("null pointer argument");
    return 0;
}

extern "C" int colnde_wm_diagnose_flux_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T,
                                           const float* d_top_flux, const float* d_halo_bottom, const float* d_halo_top, float Lz, const float params[7],
                                           int convective_adjustment, float* d_uw, float* d_vw, float* d_wT, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    WmCall c = wm_call(d_weights, d_u, d_v, d_T, d_top_flux, Lz, n_columns);
    wm_physics(&c, d_halo_bottom, d_halo_top, 0.0f, params, convective_adjustment);
    wm_face_group(&c, d_uw, d_vw, d_wT);
    if (wm_diag_check(h, __func__, c, false)) return 1;
    return wm_launch(h, K_FLUXDIAG, __func__, c);
}

extern "C" int colnde_wm_embedded_step_flux_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T,
                                                const float* d_top_flux, const float* d_halo_bottom, const float* d_halo_top, float Lz, float dt,
                                                const float params[7], int convective_adjustment, float* d_dz_uw, float* d_dz_vw, float* d_dz_wT,
                                                float* d_u_out, float* d_v_out, float* d_T_out, float* d_uw, float* d_vw, float* d_wT, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    WmCall c = wm_call(d_weights, d_u, d_v, d_T, d_top_flux, Lz, n_columns);
    wm_physics(&c, d_halo_bottom, d_halo_top, dt, params, convective_adjustment);
    wm_dz_group(&c, d_dz_uw, d_dz_vw, d_dz_wT);
    wm_step_group(&c, d_u_out, d_v_out, d_T_out);
    wm_face_group(&c, d_uw, d_vw, d_wT);
    if (wm_diag_check(h, __func__, c, true)) return 1;
    if (wm_step_check(h, c)) return 1;
    // One launch, by measurement (profiles/wm_diag_rate.json): it beats colnde_wm_embedded_step_dev + colnde_wm_diagnose_flux_dev by far more than
    // the spread at 9,216, 65,536 and 1,048,576 columns.
    return wm_launch(h, K_FLUXDIAG, __func__, c);
}

// The host arrays of a call its entry point has checked: staged in one scratch, the call's _dev twin on the device blocks, the outputs copied back.
// The step works in place on the u | v | T blocks it uploaded.  ens: colnde_ensemble_wm_embedded — the K models' blocks, top_flux [3][n] shared by
// them, the halos [K][3][n]; otherwise the groups that are given choose among the four single-model calls.
static int wm_host(colnde_handle* h, const char* fn, const WmCall& c, bool ens) {
    HIPCHK(hipSetDevice(h->device));
    const WmEmbedIO& io = c.io;
    const size_t K = ens ? (size_t)h->n_models : 1, nc = (size_t)io.n_col;
    const float* src[3] = {io.u, io.v, io.T};
    float *dst[3] = {io.u_out, io.v_out, io.T_out}, *dzs[3] = {io.dz_uw, io.dz_vw, io.dz_wT}, *faces[3] = {io.uw, io.vw, io.wT};
    float *d_s[3], *d_o[3], *d_dz[3], *d_f[3], *d_top, *d_hb, *d_ht;
    HostStage st(h, fn);
    st.to(h->d_w, c.weights, K * (size_t)h->m.n_params);
    for (int f = 0; f < 3; f++) st.inout(&d_s[f], &d_o[f], src[f], dst[f], K * nc * WM_NZ);
    for (int f = 0; f < 3; f++) st.out(&d_dz[f], dzs[f], K * nc * WM_NZ);
    for (int f = 0; f < 3; f++) st.out(&d_f[f], faces[f], K * nc * (WM_NZ + 1));
    st.in(&d_top, io.top_flux, 3 * nc);
    st.in(&d_hb, io.halo_bottom, 3 * K * nc);
    st.in(&d_ht, io.halo_top, 3 * K * nc);
    if (st.upload()) return 1;
    const float* const w = h->d_w;
    const int n = io.n_col;
    int rc;
    if (ens)
        rc = colnde_ensemble_wm_embedded_dev(h, w, d_s[0], d_s[1], d_s[2], d_top, d_hb, d_ht, io.Lz, c.dt, c.params, c.ca, d_dz[0], d_dz[1], d_dz[2], d_o[0], d_o[1],
                                             d_o[2], d_f[0], d_f[1], d_f[2], n);
    else if (io.diag())
        rc = io.fused() ? colnde_wm_embedded_step_flux_dev(h, w, d_s[0], d_s[1], d_s[2], d_top, d_hb, d_ht, io.Lz, c.dt, c.params, c.ca, d_dz[0], d_dz[1], d_dz[2],
                                                           d_o[0], d_o[1], d_o[2], d_f[0], d_f[1], d_f[2], n)
                        : colnde_wm_diagnose_flux_dev(h, w, d_s[0], d_s[1], d_s[2], d_top, d_hb, d_ht, io.Lz, c.params, c.ca, d_f[0], d_f[1], d_f[2], n);
    else
        rc = io.fused() ? colnde_wm_embedded_step_dev(h, w, d_s[0], d_s[1], d_s[2], d_top, d_hb, io.Lz, c.dt, c.params, c.ca, d_dz[0], d_dz[1], d_dz[2], d_o[0],
                                                      d_o[1], d_o[2], n)
                        : colnde_wm_infer_dz_flux_dev(h, w, d_s[0], d_s[1], d_s[2], d_top, io.Lz, d_dz[0], d_dz[1], d_dz[2], n);
    return rc ? 1 : st.download();
}

extern "C" int colnde_wm_infer_dz_flux(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T, const float* top_flux, float Lz,
                                       float* dz_uw, float* dz_vw, float* dz_wT, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    WmCall c = wm_call(weights, u, v, T, top_flux, Lz, n_columns);
    wm_dz_group(&c, dz_uw, dz_vw, dz_wT);
    if (wm_infer_check(h, __func__, c, true, false)) return 1;
    return wm_host(h, __func__, c, false);
}

extern "C" int colnde_wm_embedded_step(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T, const float* top_flux,
                                       const float* halo_bottom, float Lz, float dt, const float params[7], int convective_adjustment, float* dz_uw,
                                       float* dz_vw, float* dz_wT, float* u_out, float* v_out, float* T_out, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    WmCall c = wm_call(weights, u, v, T, top_flux, Lz, n_columns);
    wm_physics(&c, halo_bottom, nullptr, dt, params, convective_adjustment);
    wm_dz_group(&c, dz_uw, dz_vw, dz_wT);
    wm_step_group(&c, u_out, v_out, T_out);
    if (wm_infer_check(h, __func__, c, true, false)) return 1;
    if (wm_step_check(h, c)) return 1;
    return wm_host(h, __func__, c, false);
}

extern "C" int colnde_wm_diagnose_flux(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T, const float* top_flux,
                                       const float* halo_bottom, const float* halo_top, float Lz, const float params[7], int convective_adjustment, float* uw,
                                       float* vw, float* wT, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    WmCall c = wm_call(weights, u, v, T, top_flux, Lz, n_columns);
    wm_physics(&c, halo_bottom, halo_top, 0.0f, params, convective_adjustment);
    wm_face_group(&c, uw, vw, wT);
    if (wm_infer_check(h, __func__, c, false, true)) return 1;
    if (!params) return fail("null pointer argument");
    return wm_host(h, __func__, c, false);
}

extern "C" int colnde_wm_embedded_step_flux(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T, const float* top_flux,
                                            const float* halo_bottom, const float* halo_top, float Lz, float dt, const float params[7],
                                            int convective_adjustment, float* dz_uw, float* dz_vw, float* dz_wT, float* u_out, float* v_out, float* T_out,
                                            float* uw, float* vw, float* wT, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    WmCall c = wm_call(weights, u, v, T, top_flux, Lz, n_columns);
    wm_physics(&c, halo_bottom, halo_top, dt, params, convective_adjustment);
    wm_dz_group(&c, dz_uw, dz_vw, dz_wT);
    wm_step_group(&c, u_out, v_out, T_out);
    wm_face_group(&c, uw, vw, wT);
    if (wm_infer_check(h, __func__, c, true, true)) return 1;
    if (wm_step_check(h, c)) return 1;
    return wm_host(h, __func__, c, false);
}

// ---- the K models of an ensemble in the embedding at once (engine_wm_infer.hip: wm_infer_ens_kernel) -------------------------------
// {nu0, nu_minus, dRi, Ric, Pr, alpha, g} of model k as the handle holds them (colnde_create_ensemble / colnde_ensemble_set_physics; cfg.alpha, cfg.g)
static void wm_ens_model_params(const colnde_handle* h, int k, float out[7]) {
    const colnde_config c = model_config(&h->cfg, h->phys_raw.empty() ? nullptr : h->phys_raw.data(), k);
    out[0] = c.nu0; out[1] = c.nu_minus; out[2] = c.dRi; out[3] = c.Ric; out[4] = c.Pr; out[5] = c.alpha; out[6] = c.g;
}

// everything the call refuses that does not depend on where the arrays live; host: the host twin's arrays (no alignment rule of their own)
static int wm_ens_check(colnde_handle* h, const char* fn, const WmCall& c, bool host) {
    const WmEmbedIO& io = c.io;
    if (!h) return fail("null handle");
    if (h->closure)
        return fail("%s takes K weight vectors, but this is a closure handle (no networks, %d constant sets): use colnde_closure_* (include/colnde.h)", fn,
                    h->n_models);
    if (wm_generic_shape(h)) {
        const WmAnyPlan plan = wm_generic_plan(h);
        if (!wm_any_fits(plan))
            return fail("%s: the networks %s need %zu bytes of LDS per 16-column tile (state and face rows, the scaled input, the outputs and two activation buffers "
                        "of %d and %d floats per column), more than the %d bytes of a workgroup; hidden widths up to 600 fit", fn,
                        layer_sizes_string(h->cfg).c_str(), plan.bytes, plan.ld[0], plan.ld[1], WMA_LDS_LIMIT);
    } else if (wm_shape_check(h, fn)) return 1;
    if (!c.weights || !io.u || !io.v || !io.T || !io.top_flux || !io.dz_uw || !io.dz_vw || !io.dz_wT) return fail("null pointer argument");
    const int n_step = (io.u_out != nullptr) + (io.v_out != nullptr) + (io.T_out != nullptr), n_flux = (io.uw != nullptr) + (io.vw != nullptr) + (io.wT != nullptr);
    if (n_step != 0 && n_step != 3)
        return fail("%s: u_out, v_out, T_out are one output group — all three given (the implicit step is taken) or all three NULL (no step); %d of 3 given", fn, n_step);
    if (n_flux != 0 && n_flux != 3)
        return fail("%s: uw, vw, wT are one output group — all three given (the face diagnosis) or all three NULL; %d of 3 given", fn, n_flux);
    if (io.n_col < 1 || !(io.Lz > 0.0f)) return fail("n_columns >= 1 and Lz > 0 required");
    if (n_step && !(c.dt > 0.0f)) return fail("%s: dt > 0 required when a step is asked for (u_out, v_out, T_out given); dt = %g", fn, c.dt);
    for (int k = 0; k < h->n_models; k++) {
        float own[7];
        const float* p = c.params ? c.params + (size_t)7 * k : own;
        if (!c.params) wm_ens_model_params(h, k, own);
        if (n_step && (!(p[0] >= 0.0f) || !(p[1] >= 0.0f))) return fail("nu0 >= 0 and nu_minus >= 0 required (the tridiagonal must stay diagonally dominant)");
        if (!(p[2] != 0.0f) || !(p[4] > 0.0f)) return fail("dRi != 0 and Pr > 0 required");
    }
    if (!host && !wm_io_aligned(io, true)) return fail("%s: the state and output arrays must be 16-byte aligned", fn);
    return 0;
}

// the device array [K] of the sweeps' constants: uploaded when it differs from what the device holds (an embedding calls with the same constants every iteration)
static int wm_ens_upload_mpp(colnde_handle* h, const float* params, bool step, float dt, float dz, int ca) {
    const size_t K = (size_t)h->n_models;
    std::vector<MppParams> P(K);
    for (size_t k = 0; k < K; k++) {
        float own[7];
        const float* p = params ? params + 7 * k : own;
        if (!params) wm_ens_model_params(h, (int)k, own);
        P[k] = mpp_params(p, step ? dt : dz * dz, dz, ca);            // (without a step c is not read: 1, as the single-model diagnosis passes it)
    }
    if (h->d_wm_ens_mpp && h->wm_ens_mpp_host.size() == K && !memcmp(h->wm_ens_mpp_host.data(), P.data(), K * sizeof(MppParams))) return 0;
    if (!h->d_wm_ens_mpp) HIPCHK(h->mem.alloc(&h->d_wm_ens_mpp, K));
    // (kernels in flight on the stream may still read the previous table: the copy is ordered on the stream and completed before returning)
    h->wm_ens_mpp_host.clear();
    HIPCHK(hipMemcpyAsync(h->d_wm_ens_mpp, P.data(), K * sizeof(MppParams), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->wm_ens_mpp_host.swap(P);
    return 0;
}

static int wm_ens_grid_cap() {
    const char* e = env_get(ENV_WM_ENS_GRID);      // test override: at most this many workgroups (several models per workgroup at small K)
    return e && *e ? std::max(0, atoi(e)) : 0;
}

// A single handle of any architecture as K = 1: the one launch of wm_embed_any_kernel (the caller has run wm_ens_check).  The constants are the
// handle's own unless params is given; they travel as a kernel argument, there is no device table.
static int wm_generic_launch(colnde_handle* h, const char* fn, const WmCall& c) {
    WmAnyArgs a = {};
    const DevModel& m = h->m;
    a.net.n_layers = m.n_layers;
    a.net.net_size = m.net_size;
    for (int l = 0; l < m.n_layers; l++) { a.net.sizes[l] = m.sizes[l]; a.net.acts[l] = m.acts[l]; a.net.w_off[l] = m.w_off[l]; a.net.b_off[l] = m.b_off[l]; }
    a.net.sizes[m.n_layers] = m.sizes[m.n_layers];
    for (int i = 0; i < 6; i++) { a.mu[i] = h->cfg.mu[i]; a.sigma[i] = h->cfg.sigma[i]; }
    a.io = c.io;
    a.weights = c.weights;
    const float dz = c.io.Lz / (float)WM_NZ;
    float own[7];
    if (!c.params) wm_ens_model_params(h, 0, own);
    a.mpp = mpp_params(c.params ? c.params : own, a.io.fused() ? c.dt : dz * dz, dz, c.ca);      // (without a step c is not read: 1, as the other diagnoses pass it)
    Timed tm(h, K_FLUXDIAG);
    hipError_t e = launch_wm_embed_any(a, h->stream);
    if (e != hipSuccess) return fail("%s launch failed: %s (the state and output arrays must be 16-byte aligned)", fn, hipGetErrorString(e));
    return 0;
}

// the K models of an ensemble (or a single handle of the fixed shape as K = 1): the one launch of wm_infer_ens_kernel
static int wm_ens_launch(colnde_handle* h, const char* fn, const WmCall& c) {
    if (wm_ens_upload_mpp(h, c.params, c.io.fused(), c.dt, c.io.Lz / (float)WM_NZ, c.ca)) return 1;
    WmEnsArgs a = {};
    wm_scalings(h, &a);
    a.io = c.io;
    a.n_models = h->n_models; a.weights = c.weights; a.w_stride = (size_t)h->m.n_params;
    a.mpp = h->d_wm_ens_mpp;
    a.grid_cap = wm_ens_grid_cap();
    // One launch at every size, by measurement (profiles/wm_ens_embed_rate.json)
    Timed tm(h, K_FLUXDIAG);
    hipError_t e = launch_wm_infer_ens(a, h->stream);
    if (e != hipSuccess) return fail("%s launch failed: %s (the state and output arrays must be 16-byte aligned)", fn, hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_ensemble_wm_embedded_dev(colnde_handle* h, const float* d_weights, const float* d_u, const float* d_v, const float* d_T,
                                               const float* d_top_flux, const float* d_halo_bottom, const float* d_halo_top, float Lz, float dt,
                                               const float* params, int convective_adjustment, float* d_dz_uw, float* d_dz_vw, float* d_dz_wT,
                                               float* d_u_out, float* d_v_out, float* d_T_out, float* d_uw, float* d_vw, float* d_wT, int n_columns) {
    NOT_A_TILE_ENSEMBLE(h);
    WmCall c = wm_call(d_weights, d_u, d_v, d_T, d_top_flux, Lz, n_columns);
    wm_physics(&c, d_halo_bottom, d_halo_top, dt, params, convective_adjustment);
    wm_dz_group(&c, d_dz_uw, d_dz_vw, d_dz_wT);
    wm_step_group(&c, d_u_out, d_v_out, d_T_out);
    wm_face_group(&c, d_uw, d_vw, d_wT);
    if (wm_ens_check(h, __func__, c, false)) return 1;
    HIPCHK(hipSetDevice(h->device));
    return wm_generic_serves(h) ? wm_generic_launch(h, __func__, c) : wm_ens_launch(h, __func__, c);
}

// host arrays (wm_host: the K models' blocks)
extern "C" int colnde_ensemble_wm_embedded(colnde_handle* h, const float* weights, const float* u, const float* v, const float* T, const float* top_flux,
                                           const float* halo_bottom, const float* halo_top, float Lz, float dt, const float* params, int convective_adjustment,
                                           float* dz_uw, float* dz_vw, float* dz_wT, float* u_out, float* v_out, float* T_out, float* uw, float* vw, float* wT,
                                           int n_columns) {
    NOT_A_TILE_ENSEMBLE(h);
    WmCall c = wm_call(weights, u, v, T, top_flux, Lz, n_columns);
    wm_physics(&c, halo_bottom, halo_top, dt, params, convective_adjustment);
    wm_dz_group(&c, dz_uw, dz_vw, dz_wT);
    wm_step_group(&c, u_out, v_out, T_out);
    wm_face_group(&c, uw, vw, wT);
    if (wm_ens_check(h, __func__, c, true)) return 1;
    return wm_host(h, __func__, c, true);
}

// diagnose_baseline_flux_uw / _vw / _wT (:157-191; column_ops.hip): no networks, any handle kind
static int mpp_diag_check(colnde_handle* h, const void* const* ptrs, int n_ptrs, float dz, const float params[7], int n_columns) {
    if (!h) return fail("null handle");
    for (int i = 0; i < n_ptrs; i++)
        if (!ptrs[i]) return fail("null pointer argument");
    if (!params) return fail("null pointer argument");
    if (n_columns < 1) return fail("n_columns must be >= 1");
    if (!(dz > 0.0f)) return fail("dz > 0 required");
    if (!(params[2] != 0.0f) || !(params[4] > 0.0f)) return fail("dRi != 0 and Pr > 0 required");
    if (h->m.Nz < 2 || h->m.Nz > 128) return fail("the flux diagnosis supports 2 <= Nz <= 128 (Nz = %d)", h->m.Nz);
    return 0;
}

extern "C" int colnde_mpp_diagnose_flux_dev(colnde_handle* h, const float* d_u, const float* d_v, const float* d_T, const float* d_top_flux,
                                            const float* d_halo_bottom, float dz, const float params[7], int convective_adjustment, float* d_uw, float* d_vw,
                                            float* d_wT, int n_columns) {
    const void* const ptrs[7] = {d_u, d_v, d_T, d_top_flux, d_uw, d_vw, d_wT};
    if (mpp_diag_check(h, ptrs, 7, dz, params, n_columns)) return 1;
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_FLUXDIAG);
    hipError_t e = launch_mpp_diagnose_flux(d_u, d_v, d_T, d_top_flux, d_halo_bottom, dz, params, convective_adjustment, d_uw, d_vw, d_wT, h->m.Nz, n_columns,
                                            h->stream);
    if (e != hipSuccess) return fail("mpp_diagnose_flux launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_mpp_diagnose_flux(colnde_handle* h, const float* u, const float* v, const float* T, const float* top_flux, const float* halo_bottom,
                                        float dz, const float params[7], int convective_adjustment, float* uw, float* vw, float* wT, int n_columns) {
    const void* const ptrs[7] = {u, v, T, top_flux, uw, vw, wT};
    if (mpp_diag_check(h, ptrs, 7, dz, params, n_columns)) return 1;
    HIPCHK(hipSetDevice(h->device));
    const size_t Nz = (size_t)h->m.Nz, nc = (size_t)n_columns;
    const float* src[3] = {u, v, T};
    float *faces[3] = {uw, vw, wT}, *d_s[3], *d_f[3], *d_top, *d_hb;
    HostStage st(h, "mpp_diagnose_flux");
    for (int f = 0; f < 3; f++) st.in(&d_s[f], src[f], nc * Nz);
    for (int f = 0; f < 3; f++) st.out(&d_f[f], faces[f], nc * (Nz + 1));
    st.in(&d_top, top_flux, 3 * nc);
    st.in(&d_hb, halo_bottom, 3 * nc);
    if (st.upload()) return 1;
    if (colnde_mpp_diagnose_flux_dev(h, d_s[0], d_s[1], d_s[2], d_top, d_hb, dz, params, convective_adjustment, d_f[0], d_f[1], d_f[2], n_columns)) return 1;
    return st.download();
}

// ---- free-convection embedded step (free_convection/src/oceananigans_nn.jl:100-118, :153-165; engine_fc_embed.hip) ----------------------
// the handles the kernels cover: the network shapes of fc32 (fc_supported), whatever engine and stepper the handle trains with — fce_shape_covers whatever
// the number of models (colnde_ensemble_fc_embedded), fce_covers the single-model entry points' (colnde_describe reports it)
static bool fce_shape_covers(const colnde_handle* h);
bool fce_covers(const colnde_handle* h) { return !h->ensemble && fce_shape_covers(h); }
static bool fce_shape_covers(const colnde_handle* h) {
    const DevModel& m = h->m;
    return !h->closure && !h->ag_rows && (m.model == COLNDE_MODEL_FREE_CONVECTION || m.model == COLNDE_MODEL_CONV_ADJ_NDE) &&
           (m.Nz == 32 || m.Nz == 64) && m.n_layers == 3 && m.n_nets == 1 && m.sizes[0] == m.Nz && m.sizes[1] == 4 * m.Nz && m.sizes[2] == 4 * m.Nz &&
           m.sizes[3] == m.Nz - 1 && m.acts[0] == COLNDE_ACT_RELU && m.acts[1] == COLNDE_ACT_RELU && m.acts[2] == COLNDE_ACT_IDENTITY;
}
// the refusals by kind and shape of the handle (its callers have dealt with ensembles and closure handles), fn named in each
static int fce_shape_check(const colnde_handle* h, const char* fn) {
    const colnde_config& c = h->cfg;
    if (c.model == COLNDE_MODEL_WIND_MIXING)
        return fail("%s needs a free-convection handle (one network on T); a wind-mixing handle has colnde_wm_embedded_step", fn);
    if (h->ag_rows) return fail("%s: this handle's network keeps its activation rows in global memory (a wide network); the embedded step covers the fc32 shapes only", fn);
    if (c.Nz != 32 && c.Nz != 64) return fail("%s covers Nz = 32 or 64 (this handle has Nz = %d)", fn, c.Nz);
    if (!fce_shape_covers(h))
        return fail("%s covers the fc32 network Dense(Nz,4Nz,relu), Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1); this handle has Nz = %d and network %s", fn, c.Nz,
                    layer_sizes_string(c).c_str());
    return 0;
}
static int fce_check(colnde_handle* h, const char* fn, const void* const* ptrs, int n_ptrs, float Lz, float K, int n_columns) {
    if (!h) return fail("null handle");
    if (fce_shape_check(h, fn)) return 1;
    for (int i = 0; i < n_ptrs; i++)
        if (!ptrs[i]) return fail("null pointer argument");
    if (n_columns < 1 || !(Lz > 0.0f)) return fail("n_columns >= 1 and Lz > 0 required");
    if (!(K >= 0.0f)) return fail("K >= 0 required");
    return 0;
}
// first call on a handle: the operand images (a handle on another engine has none yet) and the kernels' LDS limits
static int fce_prepare(colnde_handle* h) {
    HIPCHK(hipSetDevice(h->device));
    if (h->fce_ready) return 0;
    if (!h->d_fc_imgf) HIPCHK(h->mem.alloc(&h->d_fc_imgf, fc_image_floats(h->m.Nz)));
    if (!h->d_fc_imgb) HIPCHK(h->mem.alloc(&h->d_fc_imgb, fc_image_floats(h->m.Nz)));
    if (!h->d_fc_bias) HIPCHK(h->mem.alloc(&h->d_fc_bias, fc_bias_floats(h->m.Nz)));
    hipError_t e = fce_set_kernel_attributes();
    if (e != hipSuccess) return fail("hipFuncSetAttribute (fc_embed) failed: %s", hipGetErrorString(e));
    h->fce_ready = true;
    return 0;
}
// One call as its entry point received it: FcEmbedArgs (engine_fc_embed.h) without the operand images and the tile width, which the launch fills in.
// dz_wT given: the step.
static FcEmbedArgs fce_call(const float* T, const float* top_flux, const float* halo_bottom, const float* halo_top, float Lz, float dt, float K, float* dz_wT,
                            float* T_out, float* wT_faces, int n_columns) {
    FcEmbedArgs a = {};
    a.T = T; a.top_flux = top_flux; a.halo_bottom = halo_bottom; a.halo_top = halo_top;
    a.Lz = Lz; a.dt = dt; a.K = K; a.dz_wT = dz_wT; a.T_out = T_out; a.wT_faces = wT_faces; a.n_col = n_columns; a.step = dz_wT != nullptr;
    return a;
}

static int fce_launch(colnde_handle* h, const char* fn, const float* d_weights, FcEmbedArgs a) {
    if (fce_prepare(h)) return 1;
    a.cw = fc_tile_width(a.n_col);                           // (the images are packed per call: this call's own tile width, as colnde_infer_forcing)
    hipError_t e = fc_launch_pack(h->m, a.cw, d_weights, h->d_fc_imgf, h->d_fc_imgb, h->d_fc_bias, nullptr, nullptr, h->stream);
    if (e != hipSuccess) return fail("fc32 pack launch failed: %s", hipGetErrorString(e));
    a.imgf = h->d_fc_imgf; a.bias = h->d_fc_bias;
    Timed tm(h, K_FCEMBED);
    e = launch_fc_embed(h->m, a, h->stream);
    if (e != hipSuccess) return fail("%s launch failed: %s (T and the output arrays must be 16-byte aligned)", fn, hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_fc_embedded_step_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux, const float* d_halo_bottom,
                                           const float* d_halo_top, float Lz, float dt, float K, float* d_dz_wT, float* d_T_out, float* d_wT_faces,
                                           int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    const void* const ptrs[5] = {d_weights, d_T, d_top_flux, d_dz_wT, d_T_out};
    if (fce_check(h, __func__, ptrs, 5, Lz, K, n_columns)) return 1;
    if (!(dt > 0.0f)) return fail("dt > 0 required");
    // Measured (profiles/fc_embed_rate.json): without the diagnosis the fused kernel is slower than the two launches it replaces at
    // 65,536 columns (one lane per column sweeps while the other waves of the workgroup wait), so that is what this call issues — the same bits,
    // timed under slots 4 and 6.  With wT_faces the one launch beats the three it replaces at every size measured and is kept.
    // COLNDE_FC_EMBED_FUSED=1 forces the fused kernel (tools/fc_embed_rate.py measures it that way).
    const char* ef = env_get(ENV_FC_EMBED_FUSED);
    if (!d_wT_faces && !(ef && atoi(ef) != 0)) {
        if (((uintptr_t)d_T | (uintptr_t)d_dz_wT | (uintptr_t)d_T_out) & 15) return fail("%s: T and the output arrays must be 16-byte aligned", __func__);
        if (colnde_infer_dz_wT_dev(h, d_weights, d_T, d_top_flux, Lz, d_dz_wT, n_columns)) return 1;
        return colnde_convective_adjustment_dev(h, d_T, d_halo_bottom, d_halo_top, dt, Lz / (float)h->m.Nz, K, d_T_out, n_columns);
    }
    return fce_launch(h, __func__, d_weights, fce_call(d_T, d_top_flux, d_halo_bottom, d_halo_top, Lz, dt, K, d_dz_wT, d_T_out, d_wT_faces, n_columns));
}

extern "C" int colnde_fc_diagnose_wT_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux, const float* d_halo_bottom,
                                         const float* d_halo_top, float Lz, float K, float* d_wT_faces, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    const void* const ptrs[4] = {d_weights, d_T, d_top_flux, d_wT_faces};
    if (fce_check(h, __func__, ptrs, 4, Lz, K, n_columns)) return 1;
    return fce_launch(h, __func__, d_weights, fce_call(d_T, d_top_flux, d_halo_bottom, d_halo_top, Lz, 0.0f, K, nullptr, nullptr, d_wT_faces, n_columns));
}

// The host arrays of a call its entry point has checked: staged in one scratch, the call's _dev twin on the device blocks, the outputs copied back;
// the step works in place on the T block it uploaded.  ens: colnde_ensemble_fc_embedded — the K members' blocks, their vectors user_params(h) floats
// apart (weights == NULL: the images of the previous call), top_flux [n] shared by them, the halos [K][n]; otherwise T_out chooses between the two
// single-model calls.
static int fce_host(colnde_handle* h, const char* fn, const float* weights, const FcEmbedArgs& c, bool ens) {
    HIPCHK(hipSetDevice(h->device));
    const size_t K = ens ? (size_t)h->n_models : 1, Nz = (size_t)h->m.Nz, nc = (size_t)c.n_col;
    float *d_T, *d_To, *d_dz, *d_faces, *d_top, *d_hb, *d_ht;
    HostStage st(h, fn);
    if (weights) st.to(h->d_w, weights, K * (size_t)(ens ? user_params(h) : h->m.n_params));
    st.inout(&d_T, &d_To, c.T, c.T_out, K * nc * Nz);
    st.out(&d_dz, c.dz_wT, K * nc * Nz);
    st.out(&d_faces, c.wT_faces, K * nc * (Nz + 1));
    st.in(&d_top, c.top_flux, nc);
    st.in(&d_hb, c.halo_bottom, K * nc);
    st.in(&d_ht, c.halo_top, K * nc);
    if (st.upload()) return 1;
    const float* const w = weights ? h->d_w : nullptr;
    int rc;
    if (ens) rc = colnde_ensemble_fc_embedded_dev(h, w, d_T, d_top, d_hb, d_ht, c.Lz, c.dt, c.K, d_dz, d_To, d_faces, c.n_col);
    else if (c.T_out) rc = colnde_fc_embedded_step_dev(h, w, d_T, d_top, d_hb, d_ht, c.Lz, c.dt, c.K, d_dz, d_To, d_faces, c.n_col);
    else rc = colnde_fc_diagnose_wT_dev(h, w, d_T, d_top, d_hb, d_ht, c.Lz, c.K, d_faces, c.n_col);
    return rc ? 1 : st.download();
}

extern "C" int colnde_fc_embedded_step(colnde_handle* h, const float* weights, const float* T, const float* top_flux, const float* halo_bottom,
                                       const float* halo_top, float Lz, float dt, float K, float* dz_wT, float* T_out, float* wT_faces, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    const void* const ptrs[5] = {weights, T, top_flux, dz_wT, T_out};
    if (fce_check(h, __func__, ptrs, 5, Lz, K, n_columns)) return 1;
    if (!(dt > 0.0f)) return fail("dt > 0 required");
    return fce_host(h, __func__, weights, fce_call(T, top_flux, halo_bottom, halo_top, Lz, dt, K, dz_wT, T_out, wT_faces, n_columns), false);
}

extern "C" int colnde_fc_diagnose_wT(colnde_handle* h, const float* weights, const float* T, const float* top_flux, const float* halo_bottom,
                                     const float* halo_top, float Lz, float K, float* wT_faces, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    const void* const ptrs[4] = {weights, T, top_flux, wT_faces};
    if (fce_check(h, __func__, ptrs, 4, Lz, K, n_columns)) return 1;
    return fce_host(h, __func__, weights, fce_call(T, top_flux, halo_bottom, halo_top, Lz, 0.0f, K, nullptr, nullptr, wT_faces, n_columns), false);
}

// ---- the K networks of a free-convection ensemble in the embedding at once (engine_fc_embed.hip: fce_ens_kernel) -------------------
// A plain fc ensemble, a conv ensemble, or a single fc handle as K = 1, plain or conv.  Everything the call refuses that does not depend on where the
// arrays live; host: the host twin's arrays (no alignment rule of their own).
static int fce_ens_check(colnde_handle* h, const char* fn, const FcEmbedArgs& c, bool host) {
    if (!h) return fail("%s: null handle", fn);
    if (h->closure)
        return fail("%s takes K weight vectors, but this is a closure handle (no networks, %d constant sets): use colnde_closure_* (include/colnde.h)", fn,
                    h->n_models);
    if (h->cfg.model == COLNDE_MODEL_WIND_MIXING)
        return fail("%s needs free-convection networks (one network on T per model); a wind-mixing handle has colnde_ensemble_wm_embedded", fn);
    if (fce_shape_check(h, fn)) return 1;
    if (!c.T || !c.top_flux) return fail("%s: null pointer argument (T, top_flux)", fn);
    if ((c.dz_wT != nullptr) != (c.T_out != nullptr))
        return fail("%s: dz_wT and T_out are one output group — both given (the forcing and the adjustment step) or both NULL (no step); one of 2 given", fn);
    if (!c.dz_wT && !c.wT_faces) return fail("%s: nothing to compute — give the step group (dz_wT, T_out), wT_faces, or both", fn);
    if (c.n_col < 1 || !(c.Lz > 0.0f)) return fail("%s: n_columns >= 1 and Lz > 0 required", fn);
    if (c.dz_wT && !(c.dt > 0.0f)) return fail("%s: dt > 0 required when a step is asked for (dz_wT, T_out given); dt = %g", fn, c.dt);
    if (!(c.K >= 0.0f)) return fail("%s: K_ca >= 0 required; K_ca = %g", fn, c.K);
    if (!host && (((uintptr_t)c.T | (uintptr_t)c.dz_wT | (uintptr_t)c.T_out | (uintptr_t)c.wT_faces) & 15))
        return fail("%s: the base pointers of T, dz_wT, T_out and wT_faces must be 16-byte aligned", fn);
    return 0;
}

// first call on a handle: the members' images, biases and filters at tile width 16 (the handle's own training images are left alone) and the LDS limits
static int fce_ens_prepare(colnde_handle* h) {
    if (h->fce_ens_ready) return 0;
    const size_t K = (size_t)h->n_models;
    if (!h->d_fce_ens_imgf) HIPCHK(h->mem.alloc(&h->d_fce_ens_imgf, K * fc_image_floats(h->m.Nz)));
    if (!h->d_fce_ens_bias) HIPCHK(h->mem.alloc(&h->d_fce_ens_bias, K * fc_bias_floats(h->m.Nz)));
    if (h->conv.c && !h->d_fce_ens_taps) HIPCHK(h->mem.alloc(&h->d_fce_ens_taps, K * FCE_TAPS_FLOATS));
    hipError_t e = fce_set_kernel_attributes();
    if (e != hipSuccess) return fail("hipFuncSetAttribute (fc_embed) failed: %s", hipGetErrorString(e));
    h->fce_ens_ready = true;
    return 0;
}

// K forward images, bias blocks and (conv) filters from the members' vectors, user_params(h) floats apart; behind a filter the dense part goes through
// the padded vectors (W1 with zero columns), as in training (fc_pack)
static int fce_ens_pack(colnde_handle* h, const char* fn, const float* d_weights) {
    const float* dense = d_weights;
    FcEns en;
    en.n_models = h->n_models;
    en.w = (size_t)h->m.n_params;
    en.img = fc_image_floats(h->m.Nz);
    en.bias = fc_bias_floats(h->m.Nz);
    hipError_t e = hipSuccess;
    if (h->conv.c) {
        e = launch_fce_taps(d_weights, (size_t)h->conv.n_params, h->conv.c, h->n_models, h->d_fce_ens_taps, h->stream);
        if (e == hipSuccess)
            e = launch_fc_conv_pad(d_weights, h->conv.c, h->conv.w1_end, h->conv.n_zero, h->m.n_params, h->conv.d_wpad, h->stream, h->n_models,
                                   (size_t)h->conv.n_params);
        if (e != hipSuccess) return fail("%s: conv filter / weight padding launch failed: %s", fn, hipGetErrorString(e));
        dense = h->conv.d_wpad;
    }
    e = fc_launch_pack(h->m, 16, dense, h->d_fce_ens_imgf, nullptr, h->d_fce_ens_bias, nullptr, nullptr, h->stream, &en);
    if (e != hipSuccess) return fail("%s: forward-image pack launch failed: %s", fn, hipGetErrorString(e));
    h->fce_ens_packed = true;
    return 0;
}

extern "C" int colnde_ensemble_fc_embedded_dev(colnde_handle* h, const float* d_weights, const float* d_T, const float* d_top_flux, const float* d_halo_bottom,
                                               const float* d_halo_top, float Lz, float dt, float K_ca, float* d_dz_wT, float* d_T_out, float* d_wT_faces,
                                               int n_columns) {
    FcEmbedArgs a = fce_call(d_T, d_top_flux, d_halo_bottom, d_halo_top, Lz, dt, K_ca, d_dz_wT, d_T_out, d_wT_faces, n_columns);
    if (fce_ens_check(h, __func__, a, false)) return 1;
    if (!d_weights && !h->fce_ens_packed)
        return fail("%s: weights == NULL reuses the operand images of the previous call on this handle, and no call has given weights yet", __func__);
    HIPCHK(hipSetDevice(h->device));
    if (fce_ens_prepare(h)) return 1;
    // One launch at every size, 16-column tiles (profiles/fc_ens_embed_rate.json).  The pack runs outside the timed scope, as in
    // colnde_fc_embedded_step: slot 9 is the embedded kernel's alone.
    if (d_weights && fce_ens_pack(h, __func__, d_weights)) return 1;
    a.cw = 16;
    a.imgf = h->d_fce_ens_imgf; a.bias = h->d_fce_ens_bias;
    Timed tm(h, K_FCEMBED);
    hipError_t e = launch_fc_embed_ens(h->m, a, h->n_models, h->conv.c, h->d_fce_ens_taps, h->stream);
    if (e != hipSuccess) return fail("%s launch failed: %s", __func__, hipGetErrorString(e));
    return 0;
}

// host arrays (fce_host: the K members' blocks)
extern "C" int colnde_ensemble_fc_embedded(colnde_handle* h, const float* weights, const float* T, const float* top_flux, const float* halo_bottom,
                                           const float* halo_top, float Lz, float dt, float K_ca, float* dz_wT, float* T_out, float* wT_faces, int n_columns) {
    const FcEmbedArgs c = fce_call(T, top_flux, halo_bottom, halo_top, Lz, dt, K_ca, dz_wT, T_out, wT_faces, n_columns);
    if (fce_ens_check(h, __func__, c, true)) return 1;
    if (!weights && !h->fce_ens_packed)
        return fail("%s: weights == NULL reuses the operand images of the previous call on this handle, and no call has given weights yet", __func__);
    return fce_host(h, __func__, weights, c, true);
}
