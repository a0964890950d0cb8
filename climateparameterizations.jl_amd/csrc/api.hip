// api.hip — the C ABI of include/colnde.h on top of the MFMA tile engine.  gfx950 only; no CPU fallback.  Here: errors, validation, stability bounds,
// creation and destruction, setters, problem data, the forward solve and the loss, diagnostics, colnde_plan / colnde_describe.  Beside it: api_grad.hip
// (gradient), api_ensemble.hip, api_closure.hip, api_substeps.hip, api_embed.hip.
#include <cstdarg>
#include <cstdio>
#include <new>

#include "api_internal.h"

static thread_local std::string g_err;

int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

// shared with comm.hip (not part of the public header)
extern "C" int colnde_internal_set_error(const char* msg) { g_err = msg ? msg : "error"; return 1; }

extern "C" const char* colnde_last_error(void) { return g_err.c_str(); }
extern "C" int colnde_version(void) { return COLNDE_VERSION; }

#define X(n) "COLNDE_" #n,
static const char* const COLNDE_ENV_SWITCHES[ENV_COUNT] = {COLNDE_ENV_LIST(X)};
#undef X
const char* env_name(EnvSwitch s) { return COLNDE_ENV_SWITCHES[s]; }
const char* env_get(EnvSwitch s) {
    const char* e = getenv(COLNDE_ENV_SWITCHES[s]);
    return (e && *e) ? e : nullptr;
}

// ---- model construction -----------------------------------------------------------------------------
int validate(const colnde_config* c) {
    if (!c) return fail("null config");
    if (c->model < 0 || c->model > 2) return fail("unknown model %d", c->model);
    if (c->Nz < 4 || c->Nz > 128) return fail("Nz = %d outside 4..128", c->Nz);
    if (c->n_layers < 1 || c->n_layers > COLNDE_MAX_LAYERS) return fail("n_layers = %d outside 1..%d", c->n_layers, COLNDE_MAX_LAYERS);
    const int ns = c->model == COLNDE_MODEL_WIND_MIXING ? 3 * c->Nz : c->Nz;
    if (c->layer_sizes[0] != ns) return fail("first layer input %d != state size %d", c->layer_sizes[0], ns);
    if (c->layer_sizes[c->n_layers] != c->Nz - 1)
        return fail("last layer output %d != Nz-1 = %d interior faces", c->layer_sizes[c->n_layers], c->Nz - 1);
    for (int l = 0; l <= c->n_layers; l++)
        if (c->layer_sizes[l] < 1 || c->layer_sizes[l] > 4096) return fail("layer size %d out of range", c->layer_sizes[l]);
    for (int l = 0; l < c->n_layers; l++)
        if (c->activations[l] < 0 || c->activations[l] > COLNDE_ACT_LEAKYRELU) return fail("unknown activation %d", c->activations[l]);
    if (c->model == COLNDE_MODEL_WIND_MIXING) {
        if (c->modified_pacanowski_philander && c->convective_adjustment && !c->inplace_variant)
            return fail("modified_pacanowski_philander and convective_adjustment are exclusive (NDE_training.jl:171)");
        if (c->zero_weights && !c->modified_pacanowski_philander)
            return fail("zero_weights requires modified_pacanowski_philander (NDE_training.jl:192-194)");
    }
    if (c->n_save < 2 || !c->save_times) return fail("need >= 2 save times");
    if (c->substeps < 0) return fail("substeps must be >= 1 (or 0: chosen from reltol by the first solve, colnde_choose_substeps)");
    if (!(c->reltol >= 0.0f) || c->reltol >= 1.0f) return fail("reltol = %g outside [0, 1) (0 = the reference's 1e-3)", c->reltol);
    for (int i = 1; i < c->n_save; i++)
        if (!(c->save_times[i] > c->save_times[i - 1])) return fail("save_times must be strictly increasing");
    if (c->n_columns < 1) return fail("n_columns must be >= 1");
    if (c->engine != COLNDE_ENGINE_AUTO && c->engine != COLNDE_ENGINE_GENERIC && c->engine != COLNDE_ENGINE_MFMA && c->engine != COLNDE_ENGINE_FC32)
        return fail("unknown engine %d", c->engine);
    if (c->stepper != COLNDE_STEPPER_RK4 && c->stepper != COLNDE_STEPPER_RKC2) return fail("unknown stepper %d", c->stepper);
    if (c->rkc_stages != 0 && (c->rkc_stages < 2 || c->rkc_stages > 256)) return fail("rkc_stages = %d outside 2..256 (0 = automatic)", c->rkc_stages);
    if (c->matrix_arithmetic != COLNDE_MATRIX_BF16X3_EXACT && c->matrix_arithmetic != COLNDE_MATRIX_F32_MFMA)
        return fail("unknown matrix_arithmetic %d (COLNDE_MATRIX_BF16X3_EXACT = 0, COLNDE_MATRIX_F32_MFMA = 1)", c->matrix_arithmetic);
    return 0;
}

// ---- explicit-RK4 stability (DESIGN §2 "Stiffness") ---------------------------------------------------------
// The reference integrates these right-hand sides with a stabilised ROCK4 (wind_mixing/train_NDE.jl:143) because their vertical
// diffusion is stiff in proportion to Nz²: the discrete Laplacian with diffusivity D (in nondimensional time) has eigenvalues down
// to -4 D Nz².  Classical RK4 is stable on the real axis for |lambda dt| <= 2.785.  D is the largest diffusivity the configuration
// can switch on: tau (nu0 + nu_minus) max(1, 1/Pr) / H² for the Richardson-number closure, tau kappa / H² for the
// convective-adjustment branches (NDE_training.jl:141-143; NDE! nu_T switch, training_postprocessing.jl:118-121), C K for
// ConvectiveAdjustmentNDE (convective_adjustment_nde.jl:43-47).  (The MLP's own Jacobian is not bounded here.)
double stiff_lambda(const colnde_config* c) {
    const double Nz2 = (double)c->Nz * c->Nz;
    double D = 0.0;
    if (c->model == COLNDE_MODEL_WIND_MIXING) {
        const double k = (double)c->tau / ((double)c->H * c->H);
        if (c->modified_pacanowski_philander) {
            D = k * ((double)c->nu0 + c->nu_minus) * fmax(1.0, 1.0 / (double)c->Pr);
            if (c->inplace_variant && c->convective_adjustment) D = fmax(D, k * c->kappa);
        } else if (c->convective_adjustment) {
            D = k * c->kappa;
        }
    } else if (c->model == COLNDE_MODEL_CONV_ADJ_NDE) {
        D = (double)c->sigma[5] / c->sigma[2] * ((double)c->tau / c->H) * c->ca_K;
    }
    return 4.0 * D * Nz2;
}

#define COLNDE_RK4_REAL_BOUND 2.785

// ---- RKC2 (Sommeijer, Shampine, Verwer 1998, eqs. 2.1-2.8; damping eps = 2/13) ------------------------------------------------
//   Y_0 = y,  Y_1 = Y_0 + mu~_1 h F_0,  Y_j = (1 - mu_j - nu_j) Y_0 + mu_j Y_{j-1} + nu_j Y_{j-2} + mu~_j h F_{j-1} + gamma~_j h F_0
// tab = [5][s + 1]: mu, nu, mu~, gamma~, c; returns the real stability boundary beta(s).
static double rkc_tables(int s, std::vector<double>* tab) {
    const double eps = 2.0 / 13.0, w0 = 1.0 + eps / ((double)s * s);
    std::vector<double> T(s + 1, 0.0), dT(s + 1, 0.0), d2T(s + 1, 0.0), b(s + 1, 0.0);
    T[0] = 1.0; T[1] = w0; dT[1] = 1.0;
    for (int j = 2; j <= s; j++) {
        T[j] = 2 * w0 * T[j - 1] - T[j - 2];
        dT[j] = 2 * T[j - 1] + 2 * w0 * dT[j - 1] - dT[j - 2];
        d2T[j] = 4 * dT[j - 1] + 2 * w0 * d2T[j - 1] - d2T[j - 2];
    }
    const double w1 = dT[s] / d2T[s];
    for (int j = 2; j <= s; j++) b[j] = d2T[j] / (dT[j] * dT[j]);
    b[0] = b[1] = b[2];
    if (tab) {
        tab->assign((size_t)5 * (s + 1), 0.0);
        double* mu = tab->data(), *nu = mu + (s + 1), *mut = nu + (s + 1), *gat = mut + (s + 1), *c = gat + (s + 1);
        mut[1] = b[1] * w1;
        c[1] = mut[1];
        for (int j = 2; j <= s; j++) {
            mu[j] = 2 * b[j] * w0 / b[j - 1];
            nu[j] = -b[j] / b[j - 2];
            mut[j] = 2 * b[j] * w1 / b[j - 1];
            gat[j] = -(1.0 - b[j - 1] * T[j - 1]) * mut[j];
            c[j] = w1 * d2T[j] / dT[j];
        }
    }
    return (w0 + 1.0) * d2T[s] / dT[s];
}

#define COLNDE_RKC_SAFETY 0.9

static double widest_interval(const colnde_config* c) {
    double span = 0.0;
    for (int i = 1; i < c->n_save; i++) span = fmax(span, (double)c->save_times[i] - (double)c->save_times[i - 1]);
    return span;
}

extern "C" int colnde_rkc_stages(const colnde_config* c) {
    if (validate(c)) return -1;
    if (c->rkc_stages) return c->rkc_stages;
    const double z = stiff_lambda(c) * widest_interval(c) / (c->substeps > 0 ? c->substeps : 1);
    int s = 2;
    while (s < 256 && COLNDE_RKC_SAFETY * rkc_tables(s, nullptr) < z) s++;
    return s;
}

extern "C" int colnde_min_substeps(const colnde_config* c) {
    if (validate(c)) return -1;
    const double span = widest_interval(c);
    if (c->stepper == COLNDE_STEPPER_RKC2) {          // s stages cover lambda dt <= 0.9 beta(s); at most 256 stages per step
        const int s = c->rkc_stages ? c->rkc_stages : 256;
        const double need = span * stiff_lambda(c) / (COLNDE_RKC_SAFETY * rkc_tables(s, nullptr));
        return need <= 1.0 ? 1 : (int)ceil(need);
    }
    return sched_interval_min(span, stiff_lambda(c), COLNDE_RK4_REAL_BOUND);
}

// The same bound on each save interval's own length (RK4): what colnde_min_substeps gives for the two-point configuration of that interval
extern "C" int colnde_schedule_min(const colnde_config* c, int* counts) {
    if (!counts) return fail("null counts");
    if (validate(c)) return 1;
    if (c->stepper != COLNDE_STEPPER_RK4) return fail("a step schedule covers RK4 only: the RKC2 stage table depends on dt");
    sched_minima(c->save_times, c->n_save, stiff_lambda(c), COLNDE_RK4_REAL_BOUND, counts);
    return 0;
}

// inv_dRi, inv_Pr and c_rib of the Richardson-number closure from the five Pacanowski-Philander constants: ONE expression for the single
// handle (build_model) and for every model of an ensemble, so that model k and a handle built with model k's constants see identical floats
RtPhys closure_constants(float nu0, float nu_minus, float dRi, float Ric, float Pr) {
    RtPhys p;
    p.nu0 = nu0; p.nu_minus = nu_minus; p.Ric = Ric; p.inv_dRi = 1.0f / dRi; p.inv_Pr = 1.0f / Pr; p.c_rib = -nu_minus / (2.0f * dRi);
    p.pad0 = 0.0f; p.pad1 = 0.0f;
    return p;
}

void build_model(const colnde_config* c, DevModel* m, PackInfo* pk) {
    memset(m, 0, sizeof(*m));
    memset(pk, 0, sizeof(*pk));
    const bool wm = c->model == COLNDE_MODEL_WIND_MIXING;
    m->model = c->model;
    m->Nz = c->Nz;
    m->ns = wm ? 3 * c->Nz : c->Nz;
    m->n_nets = wm ? 3 : 1;
    m->n_bc = wm ? 6 : 2;
    m->n_layers = c->n_layers;
    int woff = 0, aoff = 0, nb = 0, pf = 0, pb = 0;
    for (int l = 0; l <= c->n_layers; l++) m->sizes[l] = c->layer_sizes[l];
    for (int l = 0; l < c->n_layers; l++) {
        const int ni = c->layer_sizes[l], no = c->layer_sizes[l + 1];
        m->acts[l] = c->activations[l];
        m->w_off[l] = woff;
        m->b_off[l] = woff + ni * no;
        woff += ni * no + no;
        m->act_off[l] = aoff;
        aoff += (no + 3) & ~3;
        nb += no;
        pk->pf_off[l] = pf;
        pk->pb_off[l] = pb;
        pf += ((no + 15) / 16) * ((ni + 15) / 16) * 256;      // [m-tile][group of 16 k][64 lanes][4]
        pb += ((ni + 15) / 16) * ((no + 15) / 16) * 256;
    }
    pk->pf_off[c->n_layers] = pf;
    pk->pb_off[c->n_layers] = pb;
    pk->pf_net = pf;
    pk->pb_net = pb;
    m->net_size = woff;
    m->n_params = woff * m->n_nets;
    m->act_total = aoff;
    m->n_bias = nb * m->n_nets;
    // tile reads may overrun a feature block by up to 15 floats: keep that inside the row
    m->ld_x = lds_pad(((m->ns + 15) / 16) * 16);
    m->ld_a = lds_pad(aoff + 16);
    m->ld_f = lds_pad(c->Nz + 1);
    m->mpp = wm && c->modified_pacanowski_philander;
    m->ca = wm && c->convective_adjustment;
    m->zero_w = wm && c->zero_weights;
    m->smooth_NN = wm && c->smooth_NN;
    m->smooth_Ri = wm && c->smooth_Ri;
    m->diurnal = wm && c->diurnal;
    m->inplace = wm && c->inplace_variant;
    const float* sg = c->sigma;
    const float* mu = c->mu;
    m->cs[0] = sg[0] / sg[3] / c->H;
    m->cs[1] = sg[1] / sg[4] / c->H;
    m->cs[2] = sg[2] / sg[5] / c->H;
    m->A[0] = c->tau / c->H * sg[3] / sg[0] * (float)c->Nz;
    m->A[1] = c->tau / c->H * sg[4] / sg[1] * (float)c->Nz;
    m->A[2] = c->tau / c->H * sg[5] / sg[2] * (float)c->Nz;
    for (int k = 0; k < 3; k++) m->s0[k] = -mu[3 + k] / sg[3 + k];
    m->B = c->H * c->g * c->alpha * sg[2];
    m->cor_u = c->f * c->tau / sg[0];
    m->cor_v = c->f * c->tau / sg[1];
    m->C_fc = (sg[5] / sg[2]) * (c->tau / c->H);
    m->sig_u = sg[0]; m->sig_v = sg[1]; m->mu_u = mu[0]; m->mu_v = mu[1];
    m->mu_wT = mu[5]; m->sig_wT = sg[5]; m->mu_T = mu[2]; m->sig_T = sg[2];
    const RtPhys ph = closure_constants(c->nu0, c->nu_minus, c->dRi, c->Ric, c->Pr);
    m->nu0 = ph.nu0; m->nu_minus = ph.nu_minus; m->Ric = ph.Ric; m->dRi = c->dRi; m->inv_dRi = ph.inv_dRi; m->inv_Pr = ph.inv_Pr; m->c_rib = ph.c_rib; m->Pr = c->Pr;
    m->kappa = c->kappa; m->eps = c->eps; m->ca_K = c->ca_K; m->tau = c->tau; m->alpha_g = c->alpha * c->g;
}

static void build_tables(const DevModel& m, std::vector<TileDesc>* tiles, std::vector<int>* bz, std::vector<int>* bg) {
    for (int net = 0; net < m.n_nets; net++)
        for (int l = 0; l < m.n_layers; l++) {
            const int ni = m.sizes[l], no = m.sizes[l + 1];
            for (int it = 0; it < (ni + 15) / 16; it++)
                for (int jt = 0; jt < (no + 15) / 16; jt++) {
                    TileDesc d;
                    d.a_src = l == 0 ? 0 : 1;
                    d.a_off = (l == 0 ? 0 : m.act_off[l - 1]) + it * 16;
                    d.d_off = m.act_off[l] + jt * 16;
                    d.net = net;
                    d.ni_rem = ni - it * 16 < 16 ? ni - it * 16 : 16;
                    d.no_rem = no - jt * 16 < 16 ? no - jt * 16 : 16;
                    d.g_off = net * m.net_size + m.w_off[l] + it * 16 * no + jt * 16;
                    d.no = no;
                    tiles->push_back(d);
                }
            for (int j = 0; j < no; j++) {
                bz->push_back(net * CT * m.ld_a + m.act_off[l] + j);
                bg->push_back(net * m.net_size + m.b_off[l] + j);
            }
        }
}

// cfg.matrix_arithmetic, per kernel family; COLNDE_FWD_SPLIT / COLNDE_ADJ_SPLIT / COLNDE_DW_SPLIT = 0 | 1 override one family each (test aid:
// isolates one kernel's arithmetic against the others').  Read here only — at creation and in colnde_set_matrix_arithmetic — never per call.
void resolve_arithmetic(colnde_handle* h) {
    const bool split = h->cfg.matrix_arithmetic == COLNDE_MATRIX_BF16X3_EXACT;
    h->sp_fwd = env_int(ENV_FWD_SPLIT, split) != 0;
    h->sp_adj = env_int(ENV_ADJ_SPLIT, split) != 0;
    h->sp_dw = env_int(ENV_DW_SPLIT, split) != 0;
    // tile16 with rows in global memory: the dense chains follow the arithmetic (plane images packed beside the f32 ones)
    h->m.sf = (h->ag_rows && h->sp_fwd) ? h->d_sf : nullptr;
    h->m.sb = (h->ag_rows && h->sp_adj) ? h->d_sb : nullptr;
}

// DevModel::ag for `tiles` workgroups (zero-filled once: the pad slots behind a layer's last feature are never written and must read as zero)
int ensure_ag(colnde_handle* h, size_t tiles) {
    if (!h->ag_rows || h->ag_tiles >= tiles) return 0;
    (void)hipStreamSynchronize(h->stream);
    h->m.ag = nullptr;
    h->ag_tiles = 0;
    const size_t bytes = tiles * ag_floats_per_tile(h->m) * sizeof(float);
    if (h->mem.resize(&h->d_ag, bytes / sizeof(float)) != hipSuccess) return fail("hipMalloc of the activation rows (%zu B) failed", bytes);
    // in stream order: the slab is new and the stream has drained, so the fill only has to precede the launches that follow on h->stream (a fill on the
    // null stream is not ordered before a kernel on a non-blocking stream)
    if (hipMemsetAsync(h->d_ag, 0, bytes, h->stream) != hipSuccess) return fail("hipMemsetAsync of the activation rows failed");
    h->ag_tiles = tiles;
    h->m.ag = h->d_ag;
    return 0;
}

// The RKC2 coefficient table for the sub-step count now in h->cfg: with rkc_stages = 0 the stage count FOLLOWS the step (least s with 0.9 beta(s) >= lambda dt),
// so colnde_choose_substeps / colnde_set_substeps / the doubled solve of colnde_error_estimate each run with the stage count their own step needs (a table
// frozen at creation would be too short for a longer step — unstable — and wastefully long for a shorter one).  Uploaded in stream order.
int refresh_rkc(colnde_handle* h) {
    if (h->cfg.stepper != COLNDE_STEPPER_RKC2) return 0;
    const int s = h->ens_rkc_stages ? h->ens_rkc_stages : colnde_rkc_stages(&h->cfg);
    if (s < 2) return 1;
    if (s == h->m.nst && !h->rkc_host.empty()) return 0;
    std::vector<double> tab;
    rkc_tables(s, &tab);
    h->rkc_host.assign((size_t)6 * RKC_LD, 0.0f);
    for (int q = 0; q < 5; q++)
        for (int j = 0; j <= s; j++) h->rkc_host[(size_t)q * RKC_LD + j] = (float)tab[(size_t)q * (s + 1) + j];
    // 1 - mu_j - nu_j (~ 1/s^2: formed in double — in float32 the cancellation would cost four digits of the Y_0 weight)
    for (int j = 0; j <= s; j++) h->rkc_host[(size_t)5 * RKC_LD + j] = (float)(1.0 - tab[j] - tab[(size_t)(s + 1) + j]);
    // (the previous table may still be read by kernels in flight on the stream; the host vector is reused, so the copy is completed before returning)
    if (hipMemcpyAsync(h->d_rkc, h->rkc_host.data(), h->rkc_host.size() * sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return fail("uploading the RKC coefficient table failed");
    h->m.nst = s;
    return 0;
}

int open_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail("no HIP device visible: colnde has no CPU fallback (the product path is the gfx950 HIP engine)");
    if (device < 0 || device >= ndev) return fail("device %d not in 0..%d", device, ndev - 1);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    return 0;
}

// Once the handle exists every refusal leaves through colnde_destroy: whatever was allocated by then goes back with it
extern "C" int colnde_create(const colnde_config* cfg, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (validate(cfg) || open_device(cfg->device)) return 1;
    colnde_handle* h = new (std::nothrow) colnde_handle();
    if (!h) return fail("out of host memory");
    h->cfg = *cfg;
    if (cfg->substeps == 0) {       // automatic: start from the least power of two inside the stability bound; the first solve call refines it
        h->auto_substeps = true;
        colnde_config c1 = *cfg;
        c1.substeps = 1;
        const int ms = colnde_min_substeps(&c1);
        int s2 = 1;
        while (s2 < ms) s2 *= 2;
        h->cfg.substeps = s2;
    }
    if (h->cfg.reltol == 0.0f) h->cfg.reltol = 1e-3f;            // solve(...; reltol=1f-3): NDE_training.jl:291
    h->save_times.assign(cfg->save_times, cfg->save_times + cfg->n_save);
    h->cfg.save_times = h->save_times.data();
    h->device = cfg->device;
    h->n_col = cfg->n_columns;
    h->n_col_total = cfg->n_columns;
    h->n_tiles = (cfg->n_columns + CT - 1) / CT;
    h->min_substeps = colnde_min_substeps(&h->cfg);
    resolve_arithmetic(h);
    build_model(cfg, &h->m, &h->pk);
    h->m.nst = 4;
    h->m.rkc = nullptr;
    if (cfg->stepper == COLNDE_STEPPER_RKC2) {
        if (h->mem.alloc(&h->d_rkc, (size_t)6 * RKC_LD) != hipSuccess) { colnde_destroy(h); return fail("allocating the RKC coefficient table failed"); }
        h->m.rkc = h->d_rkc;
        if (refresh_rkc(h)) { colnde_destroy(h); return 1; }
    }
    std::vector<TileDesc> tiles;
    std::vector<int> bz, bg;
    build_tables(h->m, &tiles, &bz, &bg);
    h->m.n_tiles = (int)tiles.size();
    const size_t lds_cap = 160 * 1024;
    {   // COLNDE_ADJ_GEOM=<index> / COLNDE_FWD_WLDS=0|1 / COLNDE_FWD_THREADS=256|512 override the heuristics (tuning aid)
        h->geo_ok = pick_adjoint_geom(h->m, &h->geo, env_int(ENV_ADJ_GEOM, -1));
    }
    h->lds_fwd = lds_floats_forward(h->m) * sizeof(float);
    h->lds_adj = h->geo_ok ? lds_floats_adjoint_geom(h->m, h->geo) * sizeof(float) : lds_floats_adjoint(h->m) * sizeof(float);
    {
        const size_t wl = ((size_t)((h->m.n_params + 3) & ~3) + 128) * sizeof(float);
        // Weights staged in LDS when they fit — unless that leaves room for only ONE workgroup per CU on a problem with more tiles than
        // CUs: there two 256-thread workgroups streaming the packed image from L2 (four k-steps per load) are faster
        // (32-128-128-31, 16,384 columns: forward 55.8 -> 42.9 ms); latency points keep the LDS copy (no L2 round trip per chain).
        h->fwd_wlds = h->lds_fwd + wl <= lds_cap && (h->n_tiles <= 256 || 2 * (h->lds_fwd + wl) <= lds_cap);
        const char* ew = env_get(ENV_FWD_WLDS);
        if (ew) h->fwd_wlds = h->lds_fwd + wl <= lds_cap && atoi(ew) != 0;
        // weights in LDS: 1,024 threads (four waves per SIMD; 8 simulations 19.7 vs 21.3 ms at 512, 32-128-128-31 54.7 vs 55.7 ms);
        // weights streamed from L2 (64-256-256-63): two independent 256-thread workgroups per CU do better (113 vs 121 ms)
        h->fwd_threads = h->fwd_wlds ? 1024 : 256;
        const char* et = env_get(ENV_FWD_THREADS);
        if (et && (atoi(et) == 256 || atoi(et) == 512 || atoi(et) == 1024)) h->fwd_threads = atoi(et);
        h->lds_fwd_solve = h->lds_fwd + (h->fwd_wlds ? wl : 0);
    }
    h->m.ag = nullptr;
    if (h->lds_fwd > lds_cap) {
        // The reference's wide wind-mixing architectures (3 x 96-400-400-31: wind_mixing/train_NDE.jl:101-102, train_NDE_args.jl:150-166) need 160 KB for the
        // tile's activation rows alone.  They run with THAT array in global memory (DevModel::ag; L2-resident, one slab per workgroup) and everything else as
        // before: weights streamed from L2, 256-thread forward, the taped-dW adjoint with the Z tape (no in-register weight-gradient tiles).
        const size_t need = h->lds_fwd;
        const size_t rest = lds_floats_forward_ag(h->m) * sizeof(float);
        if (rest > lds_cap || CT * h->m.ns > 2 * 1024) {
            colnde_destroy(h);
            return fail("network too large for the tile engine: forward needs %zu B of LDS (> %zu), %zu B even with the activation rows in global memory", need, lds_cap, rest);
        }
        h->ag_rows = true;
        h->lds_fwd = rest;
        h->lds_fwd_solve = rest;
        h->fwd_wlds = false;
        // one 1,024-thread workgroup per tile (four waves per SIMD hide the row and weight loads from L2): 12.4 M column-timesteps/s forward at 4,096 ... 32,768
        // columns against 8.6 M with 256-thread workgroups (tools/wide_threads.py).  COLNDE_FWD_THREADS=256|1024 overrides.
        h->fwd_threads = 1024;
        {
            const char* et = env_get(ENV_FWD_THREADS);
            if (et && (atoi(et) == 256 || atoi(et) == 1024)) h->fwd_threads = atoi(et);
        }
        h->geo_ok = false;
        if (ensure_ag(h, (size_t)h->n_tiles)) { colnde_destroy(h); return 1; }
        // plane images of the dense chains (16-byte items): forward [16-row tile][32-deep k-block][3 planes][64 lanes], transposed likewise
        int fo = 0, bo = 0;
        for (int l = 0; l < h->m.n_layers; l++) {
            const int ni = h->m.sizes[l], no = h->m.sizes[l + 1];
            h->m.sf_off[l] = fo;
            h->m.sb_off[l] = bo;
            fo += ((no + 15) / 16) * ((ni + 31) / 32) * 3 * 64;
            bo += ((ni + 15) / 16) * ((no + 31) / 32) * 3 * 64;
        }
        h->m.sf_net = fo;
        h->m.sb_net = bo;
        if (h->mem.alloc(&h->d_sf, (size_t)fo * h->m.n_nets * 4) != hipSuccess || h->mem.alloc(&h->d_sb, (size_t)bo * h->m.n_nets * 4) != hipSuccess) {
            colnde_destroy(h);
            return fail("allocating the bf16 plane images failed");
        }
        resolve_arithmetic(h);
    }
    if (h->lds_adj > lds_cap) h->geo_ok = false;
    {
        hipError_t e = set_kernel_attributes(lds_cap);
        if (e == hipSuccess) e = dw_set_kernel_attributes(lds_cap);
        if (e == hipSuccess) e = fcp_set_kernel_attributes(lds_cap);
        if (e == hipSuccess) e = wmp_set_kernel_attributes(lds_cap);
        if (e == hipSuccess) e = rt_set_attributes();
        if (e == hipSuccess) e = rt_set_attributes_split();
        if (e != hipSuccess) { colnde_destroy(h); return fail("hipFuncSetAttribute failed: %s", hipGetErrorString(e)); }
    }
    // AUTO: regtile where it applies, except for problems of at most 8,192 columns (two rounds of one 16-column tile per CU).  Those
    // are latency points for regtile — 32 columns per wavefront leave most SIMDs without a wave — and go to the net-split kernels
    // (one wavefront per flux net plus a helper wavefront per 16-column tile, below) with tile16's tapes and dW GEMM: 4,096 columns x 64 steps
    // 3.55 vs 9.48 ms per iteration, 8,192: 6.99 vs 9.84, 16,384: 12.8 vs 10.7 (tools/crossover.py)
    h->use_rt = rt_supported(h->m) && cfg->stepper == COLNDE_STEPPER_RK4 && cfg->engine != COLNDE_ENGINE_GENERIC &&
                (cfg->engine == COLNDE_ENGINE_MFMA || cfg->n_columns > 8192 || !h->geo_ok);
    h->rt_fwd32 = h->use_rt && rt_forward_is32();
    // AUTO on a regtile-shaped problem too small for regtile (a latency point): the net-split kernels take the forward solves and
    // the adjoint (8 simulations: forward 19.8 -> 8.3 ms, adjoint 25.0 -> 8.2 ms), tile16 the tapes' formats, the dW GEMM and the reduction.
    // An explicit engine = tile16 stays pure tile16; COLNDE_T16_FWD_SPLIT=0|1 and COLNDE_T16_ADJ_SPLIT=0 override.
    {
        // (round 3: the stabilised RKC2 stepper too — in the four-wave kernels, so only with both helper waves on)
        const char* eh = env_get(ENV_T16_FWD_HELPER);      // 0: the three-wave forward (8 simulations 9.8 vs 8.3 ms, 4,096 columns 8.27 vs 7.65 ms)
        h->fwd_helper = !(eh && atoi(eh) == 0);
        const char* eah = env_get(ENV_T16_ADJ_HELPER);     // 0: the three-wave adjoint (8 simulations 11.3 vs 8.2 ms)
        h->adj_helper = !(eah && atoi(eah) == 0);
        const bool stepper_ok = cfg->stepper == COLNDE_STEPPER_RK4 || (cfg->stepper == COLNDE_STEPPER_RKC2 && h->fwd_helper && h->adj_helper);
        h->fwd_split = !h->use_rt && rt_supported(h->m) && stepper_ok && cfg->engine == COLNDE_ENGINE_AUTO;
        const char* es = env_get(ENV_T16_FWD_SPLIT);
        if (es) h->fwd_split = !h->use_rt && rt_supported(h->m) && stepper_ok && atoi(es) != 0;
        // the gradient behind a split forward: rt16s_adjoint_kernel (same decomposition) when the taped mode with both tapes is planned
        const char* ea = env_get(ENV_T16_ADJ_SPLIT);
        h->adj_split = h->fwd_split && !(ea && atoi(ea) == 0);
    }
    if (cfg->engine == COLNDE_ENGINE_MFMA && !h->use_rt) {
        colnde_destroy(h);
        return fail("engine = regtile requested, but it covers only Nz=32, three 96-50-20-31 nets, no smoothing, training RHS, RK4");
    }
    // AUTO on the free-convection shape the reference trains: the 32-column engine (COLNDE_FC=0 keeps tile16)
    {
        const char* ef = env_get(ENV_FC);
        h->use_fc = fc_supported(h->m, cfg->stepper) && (cfg->engine == COLNDE_ENGINE_FC32 || (cfg->engine == COLNDE_ENGINE_AUTO && !(ef && atoi(ef) == 0)));
        if (cfg->engine == COLNDE_ENGINE_FC32 && !h->use_fc) {
            colnde_destroy(h);
            return fail("engine = fc32 requested, but it covers only FreeConvectionNDE (RK4) and ConvectiveAdjustmentNDE (RK4, RKC2) with Dense(Nz,4Nz,relu), Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1), Nz = 32 or 64");
        }
        if (h->use_fc) {
            h->fc_cw = fc_tile_width(cfg->n_columns);
            hipError_t e = fc_set_kernel_attributes();
            if (e != hipSuccess) { colnde_destroy(h); return fail("hipFuncSetAttribute (fc32) failed: %s", hipGetErrorString(e)); }
        }
    }
    const DevModel& m = h->m;
#define ALLOC(ptr, n, T)                                                                   \
    do {                                                                                   \
        hipError_t e_ = h->mem.alloc(&(ptr), (size_t)(n));                                 \
        if (e_ != hipSuccess) {                                                            \
            colnde_destroy(h);                                                             \
            return fail("hipMalloc of %zu bytes failed: %s", (size_t)(n) * sizeof(T), hipGetErrorString(e_)); \
        }                                                                                  \
    } while (0)
    ALLOC(h->d_w, m.n_params, float);
    ALLOC(h->d_wf, (size_t)h->pk.pf_net * m.n_nets, float);
    ALLOC(h->d_wb, (size_t)h->pk.pb_net * m.n_nets, float);
    ALLOC(h->d_wimg, RT_IMG_ALLOC, float);
    if (h->use_fc) {
        ALLOC(h->d_fc_imgf, fc_image_floats(m.Nz), float);
        ALLOC(h->d_fc_imgb, fc_image_floats(m.Nz), float);
        ALLOC(h->d_fc_bias, fc_bias_floats(m.Nz), float);
        ALLOC(h->d_fc_simgf, fc_split_image_words(m.Nz), unsigned int);
        ALLOC(h->d_fc_simgb, fc_split_image_words(m.Nz), unsigned int);
    }
    ALLOC(h->d_x0, (size_t)h->n_col * m.ns, float);
    ALLOC(h->d_bcs, (size_t)h->n_col * m.n_bc, float);
    ALLOC(h->d_sol, (size_t)h->n_col * cfg->n_save * m.ns, float);
    ALLOC(h->d_out, m.n_params + 8, float);
    ALLOC(h->d_times, cfg->n_save, float);
    ALLOC(h->d_partial, 1024 * 8, float);
    ALLOC(h->d_tiles, tiles.size(), TileDesc);
    ALLOC(h->d_bias_zoff, bz.size(), int);
    ALLOC(h->d_bias_goff, bg.size(), int);
#undef ALLOC
    hipError_t e = hipMemcpy(h->d_times, h->save_times.data(), sizeof(float) * cfg->n_save, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->d_tiles, tiles.data(), sizeof(TileDesc) * tiles.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->d_bias_zoff, bz.data(), sizeof(int) * bz.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->d_bias_goff, bg.data(), sizeof(int) * bg.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { colnde_destroy(h); return fail("table upload failed: %s", hipGetErrorString(e)); }
    *out = h;
    return 0;
}

void drain_events(colnde_handle* h) {
    for (PendingEvent& p : h->pending) {
        float ms = 0.0f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            h->ms[p.which] += ms;
            h->launches[p.which] += 1;
        }
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    h->pending.clear();
}

extern "C" void colnde_destroy(colnde_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    drain_events(h);
    h->mem.free_all();
    delete h;
}

// parameters of the vector the caller passes: the model's, except behind a conv filter (the handle's internal vector pads W1)
int user_params(const colnde_handle* h) { return h->conv.c ? h->conv.n_params : h->m.n_params; }
extern "C" int colnde_n_params(const colnde_handle* h) { return h ? user_params(h) : -1; }
extern "C" int colnde_conv_filter(const colnde_handle* h) { return h ? h->conv.c : -1; }
extern "C" int colnde_engine(const colnde_handle* h) { return h ? engine_id(h) : -1; }

extern "C" int colnde_set_stream(colnde_handle* h, void* s) {
    if (!h) return fail("null handle");
    if ((hipStream_t)s == h->stream) return 0;          // (free: the Python front-end issues one per method call)
    // what the handle wrote on the old stream without synchronising (the problem, packed images, tapes, the RKC table) is read on the new one
    HIPCHK(hipSetDevice(h->device));
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail("colnde_set_stream: draining the previous stream failed: %s", hipGetErrorString(e));
    h->stream = (hipStream_t)s;
    return 0;
}

extern "C" int colnde_set_matrix_arithmetic(colnde_handle* h, int ma) {
    if (!h) return fail("null handle");
    if (ma != COLNDE_MATRIX_BF16X3_EXACT && ma != COLNDE_MATRIX_F32_MFMA)
        return fail("unknown matrix_arithmetic %d (COLNDE_MATRIX_BF16X3_EXACT = 0, COLNDE_MATRIX_F32_MFMA = 1)", ma);
    const int before = h->cfg.matrix_arithmetic;
    h->cfg.matrix_arithmetic = ma;
    resolve_arithmetic(h);
    if (replan_dw_slices(h)) {              // a planned dW GEMM follows the arithmetic; when it cannot, the previous arithmetic stays
        h->cfg.matrix_arithmetic = before;
        resolve_arithmetic(h);
        return 1;
    }
    return 0;
}
extern "C" int colnde_matrix_arithmetic(const colnde_handle* h) { return h ? h->cfg.matrix_arithmetic : -1; }

extern "C" int colnde_set_global_columns(colnde_handle* h, int64_t n) {
    if (!(h && h->closure)) SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h) return fail("null handle");
    if (n < h->n_col) return fail("global column count %lld < local %d", (long long)n, h->n_col);
    h->n_col_total = n;
    return 0;
}

// ---- profiling -----------------------------------------------------------------------------------------
extern "C" int colnde_set_profiling(colnde_handle* h, int enabled) {
    if (!h) return fail("null handle");
    h->prof = enabled != 0;
    return 0;
}
extern "C" int colnde_kernel_time(colnde_handle* h, int which, float* ms_total, int* n_launches) {
    if (!h) return fail("null handle");
    if (which < 0 || which >= K_COUNT) return fail("kernel id %d outside 0..%d", which, K_COUNT - 1);
    HIPCHK(hipSetDevice(h->device));
    drain_events(h);
    if (ms_total) *ms_total = (float)h->ms[which];
    if (n_launches) *n_launches = h->launches[which];
    return 0;
}
extern "C" int colnde_reset_kernel_times(colnde_handle* h) {
    if (!h) return fail("null handle");
    drain_events(h);
    for (int i = 0; i < K_COUNT; i++) { h->ms[i] = 0; h->launches[i] = 0; }
    return 0;
}

// ---- problem data --------------------------------------------------------------------------------------
static int set_problem_impl(colnde_handle* h, const float* x0, const float* bcs, const float* truth, hipMemcpyKind kind) {
    if (!h) return fail("null handle");
    if (!x0 || !bcs) return fail("x0 and bcs must not be null");
    HIPCHK(hipSetDevice(h->device));
    const DevModel& m = h->m;
    HIPCHK(hipMemcpyAsync(h->d_x0, x0, sizeof(float) * (size_t)h->n_col * m.ns, kind, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_bcs, bcs, sizeof(float) * (size_t)h->n_col * m.n_bc, kind, h->stream));
    if (truth) {
        const size_t n = (size_t)h->n_col * h->cfg.n_save * m.ns;
        if (!h->d_truth) HIPCHK(h->mem.alloc(&h->d_truth, n));
        HIPCHK(hipMemcpyAsync(h->d_truth, truth, n * sizeof(float), kind, h->stream));
    }
    h->have_truth = truth != nullptr;
    h->have_problem = true;
    if (kind == hipMemcpyHostToDevice) HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
extern "C" int colnde_set_problem(colnde_handle* h, const float* x0, const float* bcs, const float* truth) {
    return set_problem_impl(h, x0, bcs, truth, hipMemcpyHostToDevice);
}
extern "C" int colnde_set_problem_dev(colnde_handle* h, const float* x0, const float* bcs, const float* truth) {
    return set_problem_impl(h, x0, bcs, truth, hipMemcpyDeviceToDevice);
}

int pack(colnde_handle* h, const float* d_weights) {
    hipError_t e = launch_pack(h->m, h->pk, d_weights, h->d_wf, h->d_wb, h->stream);
    if (e != hipSuccess) return fail("pack_weights launch failed: %s", hipGetErrorString(e));
    if (h->d_sf && (h->m.sf || h->m.sb)) {
        e = launch_pack_planes(h->m, d_weights, h->d_sf, h->d_sb, h->stream);
        if (e != hipSuccess) return fail("pack_planes launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

void loss_weights(const colnde_handle* h, const float scalings[6], LossWeights* lw) {
    const double np = (double)h->n_col_total * h->cfg.n_save * h->m.Nz;
    const double ng = (double)h->n_col_total * h->cfg.n_save * (h->m.Nz + 1);
    for (int q = 0; q < 8; q++) lw->w[q] = 0.0f;
    if (h->m.model == COLNDE_MODEL_WIND_MIXING) {
        for (int k = 0; k < 3; k++) {
            lw->w[k] = (float)(scalings[k] / np);
            lw->w[3 + k] = (float)(scalings[3 + k] / ng);
        }
    } else {
        lw->w[2] = (float)(scalings[2] / np);
    }
}

// ---- rhs -----------------------------------------------------------------------------------------------
extern "C" int colnde_rhs_dev(colnde_handle* h, const float* d_x, const float* d_weights, const float* d_bcs, float t,
                              float* d_dx, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h) return fail("null handle");
    if (!d_x || !d_weights || !d_bcs || !d_dx) return fail("null pointer argument");
    if (n_columns < 1) return fail("n_columns must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    if (pack(h, d_weights)) return 1;
    if (ensure_ag(h, ((size_t)n_columns + CT - 1) / CT)) return 1;
    Timed tm(h, K_RHS);
    hipError_t e = launch_rhs(h->m, h->pk, d_weights, h->d_wf, d_x, d_bcs, t, d_dx, n_columns, 256, h->lds_fwd, h->stream);
    if (e != hipSuccess) return fail("rhs launch failed: %s", hipGetErrorString(e));
    return 0;
}

int ensure_tmp(colnde_handle* h, size_t n_columns) {
    if (h->tmp_cols >= n_columns) return 0;
    h->tmp_cols = 0;
    HIPCHK(h->mem.resize(&h->d_tmp_a, n_columns * h->m.ns));
    HIPCHK(h->mem.resize(&h->d_tmp_b, n_columns * 8));
    HIPCHK(h->mem.resize(&h->d_tmp_c, n_columns * h->m.ns));
    h->tmp_cols = n_columns;
    return 0;
}

extern "C" int colnde_rhs(colnde_handle* h, const float* x, const float* weights, const float* bcs, float t, float* dx,
                          int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h) return fail("null handle");
    if (!x || !weights || !bcs || !dx) return fail("null pointer argument");
    if (n_columns < 1) return fail("n_columns must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    if (ensure_tmp(h, (size_t)n_columns)) return 1;
    const DevModel& m = h->m;
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * m.n_params, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_tmp_a, x, sizeof(float) * (size_t)n_columns * m.ns, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_tmp_b, bcs, sizeof(float) * (size_t)n_columns * m.n_bc, hipMemcpyHostToDevice, h->stream));
    if (colnde_rhs_dev(h, h->d_tmp_a, h->d_w, h->d_tmp_b, t, h->d_tmp_c, n_columns)) return 1;
    HIPCHK(hipMemcpyAsync(dx, h->d_tmp_c, sizeof(float) * (size_t)n_columns * m.ns, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// regtile forward solve of columns [c0, c0 + nc): sol rows and, when taping, the block's tapes
int rt_forward_range(colnde_handle* h, float* d_sol, bool with_tape, int c0, int nc) {
    const size_t ns = h->m.ns;
    Timed tm(h, K_FORWARD);
    hipError_t e = rt_launch_forward(h->m, h->d_wimg, h->d_x0 + (size_t)c0 * ns, h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times, h->cfg.n_save,
                                     h->cfg.substeps, d_sol ? d_sol + (size_t)c0 * h->cfg.n_save * ns : nullptr,
                                     with_tape ? h->d_rt_tape : nullptr, (with_tape && h->rt_ztape) ? h->d_rt_tapez : nullptr, nc,
                                     h->rt_fwd32, h->sp_fwd, h->stream);
    if (e != hipSuccess) return fail("rt forward launch failed: %s", hipGetErrorString(e));
    return 0;
}

// tile16 forward solve of columns [c0, c0 + nc) (c0 a multiple of the 16-column tile); with_tape: into the handle's (block) tapes
int t16_forward_range(colnde_handle* h, const float* d_weights, float* d_sol, bool with_tape, int c0, int nc) {
    const size_t ns = h->m.ns;
    if (with_tape && !h->d_tape) {     // in-register gradient mode: the whole problem's stage tape
        const size_t n = sched_tape_floats((size_t)h->n_tiles, total_steps(h), h->m.nst, CT * ns);
        hipError_t e = h->mem.alloc(&h->d_tape, n);
        if (e != hipSuccess) return fail("hipMalloc of the %zu-byte stage tape failed: %s", n * sizeof(float), hipGetErrorString(e));
    }
    Timed tm(h, K_FORWARD);
    if (h->fwd_split) {
        // latency points of the wind-mixing shape: one wavefront per flux net (+ a helper) per 16-column tile (engine_netsplit.hip); the tapes
        // come out in tile16's formats for its taped adjoint
        hipError_t es = rt_launch_pack(h->m, d_weights, h->d_wimg, h->stream);
        if (es == hipSuccess)
            es = rt_launch_forward_split(h->m, h->d_wimg, h->d_x0 + (size_t)c0 * ns, h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times, h->cfg.n_save,
                                         h->cfg.substeps, d_sol ? d_sol + (size_t)c0 * h->cfg.n_save * ns : nullptr,
                                         with_tape ? h->d_tape : nullptr, with_tape ? h->d_t16_ztape : nullptr, nc, with_tape && h->split_rich, h->fwd_helper, h->sp_fwd, h->stream,
                                         RtEns(), sched_dev(h), total_steps(h));
        if (es != hipSuccess) return fail("split forward launch failed: %s", hipGetErrorString(es));
        return 0;
    }
    if (!h->sched.empty()) return fail("a step schedule is set, but this solve does not run on rt16sh_forward_kernel");
    hipError_t e = launch_forward(h->m, h->pk, d_weights, h->d_wf, h->d_x0 + (size_t)c0 * ns, h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times,
                                  h->cfg.n_save, h->cfg.substeps, d_sol ? d_sol + (size_t)c0 * h->cfg.n_save * ns : nullptr,
                                  with_tape ? h->d_tape : nullptr, nc, h->fwd_threads, h->fwd_wlds, h->lds_fwd_solve, h->stream,
                                  with_tape ? h->d_t16_ztape : nullptr);
    if (e != hipSuccess) return fail("forward launch failed: %s", hipGetErrorString(e));
    return 0;
}

// fc32 forward solve of columns [c0, c0 + nc) (c0 a multiple of 32) over the save intervals [iv0, iv1); with_tape: into the handle's records and
// bits.  iv0 > 0 restarts from the state a previous (tape-less) pass saved in d_sol at save point iv0 — exact: the saved state is the stepper's.
// The conv handle's kernels take the filter from the head of the user's vector and the conv tape from the handle
FcConv fc_conv_args(const colnde_handle* h) {
    FcConv cv;
    cv.c = h->conv.c;
    cv.wb = h->conv.d_user;
    cv.ctape = h->conv.d_ctape;
    return cv;
}
// ... model 0's, in a conv ensemble; model k's lie at these strides (its own vector of conv.n_params floats, its own conv tape)
FcConvEns fc_conv_ens_args(const colnde_handle* h) {
    FcConvEns ce;
    ce.wb = (size_t)h->conv.n_params;
    ce.ctape = h->conv.ctape_stride;
    return ce;
}

// The operand images of the weights: one network's, or those of every model of a free-convection ensemble (FcEns strides).  The vector packed is the
// caller's, or — behind a conv filter — its dense part with W1 padded to 4Nz x Nz (one small kernel on the stream)
int fc_pack(colnde_handle* h, const float* d_weights) {
    hipError_t e = hipSuccess;
    if (h->conv.c) {
        h->conv.d_user = d_weights;
        e = launch_fc_conv_pad(d_weights, h->conv.c, h->conv.w1_end, h->conv.n_zero, h->m.n_params, h->conv.d_wpad, h->stream, h->n_models, (size_t)h->conv.n_params);
        if (e != hipSuccess) return fail("conv weight padding launch failed: %s", hipGetErrorString(e));
        d_weights = h->conv.d_wpad;
    }
    e = fc_launch_pack(h->m, h->fc_cw, d_weights, h->d_fc_imgf, h->d_fc_imgb, h->d_fc_bias, h->d_fc_simgf, h->d_fc_simgb, h->stream, h->ensemble ? &h->fens : nullptr);
    if (e != hipSuccess) return fail("fc32 %spack launch failed: %s", h->ensemble ? "ensemble " : "", hipGetErrorString(e));
    return 0;
}

// An ensemble is the case c0 = 0, nc = all columns: every model solves them, from the shared x0 (iv0 = 0) or from its own saved state
int fc_forward_range(colnde_handle* h, float* d_sol, bool with_tape, int c0, int nc, int iv0, int iv1, int tape_iv0) {
    const size_t ns = h->m.ns;
    const FcConv cv = fc_conv_args(h);
    const FcConvEns ce = fc_conv_ens_args(h);
    FcEns en = h->fens;
    en.x0 = iv0 == 0 ? 0 : en.sol;
    if (iv1 < 0) iv1 = h->cfg.n_save - 1;
    if (tape_iv0 < 0) tape_iv0 = iv0;                // (a later tape_iv0: the tape-less pass of a segmented gradient tapes its last segment on the way)
    const float* init = iv0 == 0 ? h->d_x0 + (size_t)c0 * ns : d_sol + ((size_t)c0 * h->cfg.n_save + iv0) * ns;
    const size_t stride = iv0 == 0 ? ns : (size_t)h->cfg.n_save * ns;
    Timed tm(h, K_FORWARD);
    hipError_t e = fc_launch_forward(h->m, h->fc_cw, h->d_fc_imgf, (h->sp_fwd && fc_split_supported(h->fc_cw)) ? h->d_fc_simgf : nullptr, h->d_fc_bias, init, stride, h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times, h->cfg.n_save,
                                     iv0, iv1, tape_iv0, h->cfg.substeps, d_sol ? d_sol + (size_t)c0 * h->cfg.n_save * ns : nullptr,
                                     with_tape ? h->d_dwtape : nullptr, with_tape ? h->d_fc_masks : nullptr, with_tape ? h->d_fc_switch : nullptr, nc,
                                     h->stream, h->ensemble ? &en : nullptr, h->conv.c ? &cv : nullptr, &ce);
    if (e != hipSuccess) return fail("fc32 %sforward launch failed: %s", h->ensemble ? "ensemble " : "", hipGetErrorString(e));
    return 0;
}

// ---- forward solve -------------------------------------------------------------------------------------
// A time step outside RK4's stability region gives a blown-up or NaN trajectory, loss and gradient with rc = 0: refuse it.
int check_stability(const colnde_handle* h) {
    if (!h->sched.empty()) {          // a schedule: each interval against its own bound
        std::vector<int> need;
        if (schedule_minima(h, &need)) return 1;
        int bad = 0;
        if (sched_validate(h->sched.data(), need.data(), (int)need.size(), allow_unstable(), &bad) == SCHED_BELOW_MIN)
            return fail("schedule[%d] = %d puts the RK4 step of save interval %d outside its stability region: need >= %d (colnde_schedule_min; "
                        "COLNDE_ALLOW_UNSTABLE_DT=1 overrides)", bad, h->sched[bad], bad, need[bad]);
        return 0;
    }
    if (h->cfg.substeps >= h->min_substeps || allow_unstable()) return 0;
    if (h->cfg.stepper == COLNDE_STEPPER_RKC2)
        return fail("substeps = %d with %d RKC2 stages does not cover the stiffest diffusive mode (lambda = -%.4g): need substeps >= %d, "
                    "or rkc_stages = 0 for the automatic stage count (COLNDE_ALLOW_UNSTABLE_DT=1 overrides)",
                    h->cfg.substeps, h->m.nst, stiff_lambda(&h->cfg), h->min_substeps);
    return fail("substeps = %d puts the RK4 step outside its stability region: the stiffest diffusive mode this configuration can "
                "switch on has lambda = -%.4g (4 D Nz^2), and lambda dt must stay within %.3f — need substeps >= %d "
                "(colnde_min_substeps; the reference uses a stabilised ROCK4 here; COLNDE_ALLOW_UNSTABLE_DT=1 overrides)",
                h->cfg.substeps, stiff_lambda(&h->cfg), COLNDE_RK4_REAL_BOUND, h->min_substeps);
}

// the refusal a creator that shares or fixes the sub-step count makes up front (ensembles of free-convection models, conv handles)
int refuse_unstable_substeps(const colnde_config* cfg) {
    const int ms = colnde_min_substeps(cfg);
    if (ms < 0) return 1;
    if (cfg->substeps < ms && !allow_unstable())
        return fail("substeps = %d is below colnde_min_substeps = %d: the step leaves the stepper's stability region (lambda = -%.4g; COLNDE_ALLOW_UNSTABLE_DT=1 overrides)",
                    cfg->substeps, ms, stiff_lambda(cfg));
    return 0;
}

// substeps = 0 picks the count from THIS handle's columns.  On a column shard (colnde_set_global_columns > the local count) every rank would settle on its
// own count: the SUM-all-reduced gradient would mix discretisations and the tapes would differ per rank.  The sharded recipe is explicit:
// colnde_choose_substeps on every rank, MAX over ranks, colnde_set_substeps (colnde.distributed.agree_substeps does exactly that).
int refuse_auto_on_a_shard(const colnde_handle* h) {
    if (h->n_col_total > h->n_col)
        return fail("substeps = 0 (chosen from reltol) on a column shard (%d of %lld columns): each rank would choose its own count — call colnde_choose_substeps "
                    "on every rank, take the MAX over ranks and impose it with colnde_set_substeps", h->n_col, (long long)h->n_col_total);
    return 0;
}

int forward_impl(colnde_handle* h, const float* d_weights, float* d_sol, bool with_tape) {
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    if (h->auto_substeps) {           // substeps = 0 at creation: settle the count now, from these weights and cfg.reltol
        if (refuse_auto_on_a_shard(h)) return 1;
        h->auto_substeps = false;
        if (choose_substeps_impl(h, d_weights, h->cfg.reltol, nullptr, nullptr)) { h->auto_substeps = true; return 1; }
    }
    if (check_stability(h)) return 1;
    if (h->use_rt) {
        // (the gradient path tapes block by block: colnde_loss_grad_dev drives rt_forward_range itself)
        hipError_t e = rt_launch_pack(h->m, d_weights, h->d_wimg, h->stream);
        if (e != hipSuccess) return fail("rt pack launch failed: %s", hipGetErrorString(e));
        return rt_forward_range(h, d_sol, false, 0, h->n_col);
    }
    if (h->use_fc) {
        if (fc_pack(h, d_weights)) return 1;
        return fc_forward_range(h, d_sol, false, 0, h->n_col);
    }
    if (pack(h, d_weights)) return 1;
    return t16_forward_range(h, d_weights, d_sol, with_tape, 0, h->n_col);
}

extern "C" int colnde_forward_dev(colnde_handle* h, const float* d_weights, float* d_sol) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!d_weights) return fail("null weights");
    HIPCHK(hipSetDevice(h->device));
    return forward_impl(h, d_weights, d_sol ? d_sol : h->d_sol, false);
}

extern "C" int colnde_forward(colnde_handle* h, const float* weights, float* sol) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!weights) return fail("null weights");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * user_params(h), hipMemcpyHostToDevice, h->stream));
    if (forward_impl(h, h->d_w, h->d_sol, false)) return 1;
    if (sol)
        HIPCHK(hipMemcpyAsync(sol, h->d_sol, sizeof(float) * (size_t)h->n_col * h->cfg.n_save * h->m.ns, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- loss / loss + gradient ----------------------------------------------------------------------------
extern "C" int colnde_loss_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out8) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!d_weights || !scalings || !d_out8) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    if (forward_impl(h, d_weights, h->d_sol, false)) return 1;
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    const int nblk = 256;
    hipError_t e = launch_loss(h->m, h->d_sol, h->d_truth, h->cfg.n_save, h->n_col, h->d_partial, nblk, h->stream);
    if (e == hipSuccess) e = launch_reduce(h->d_partial, nblk, 0, 8, lw, d_out8, h->stream);
    if (e != hipSuccess) return fail("loss launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_loss(colnde_handle* h, const float* weights, const float scalings[6], float terms[6], float* total) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!weights || !scalings || !terms || !total) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * user_params(h), hipMemcpyHostToDevice, h->stream));
    if (colnde_loss_dev(h, h->d_w, scalings, h->d_out)) return 1;
    float o[8];
    HIPCHK(hipMemcpyAsync(o, h->d_out, sizeof(o), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int q = 0; q < 6; q++) terms[q] = o[q];
    *total = o[6];
    if (!std::isfinite(o[6])) return fail("the loss is not finite (%g): the solve left the stable regime (time step, weights or inputs)", o[6]);
    return 0;
}

// ---- flux diagnostics: predict_flux and loss_per_tstep ---------------------------------------------------------------------------------
extern "C" int colnde_flux_dev(colnde_handle* h, const float* d_x, const float* d_weights, const float* d_bcs, float t, float* d_flux, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h) return fail("null handle");
    if (!d_x || !d_weights || !d_bcs || !d_flux) return fail("null pointer argument");
    if (n_columns < 1) return fail("n_columns must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    if (pack(h, d_weights)) return 1;
    if (ensure_ag(h, ((size_t)n_columns + CT - 1) / CT)) return 1;
    Timed tm(h, K_RHS);
    hipError_t e = launch_rhs(h->m, h->pk, d_weights, h->d_wf, d_x, d_bcs, t, nullptr, n_columns, 256, h->lds_fwd, h->stream, d_flux);
    if (e != hipSuccess) return fail("flux launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_flux(colnde_handle* h, const float* x, const float* weights, const float* bcs, float t, float* flux, int n_columns) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h) return fail("null handle");
    if (!x || !weights || !bcs || !flux) return fail("null pointer argument");
    if (n_columns < 1) return fail("n_columns must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    if (ensure_tmp(h, (size_t)n_columns)) return 1;
    const DevModel& m = h->m;
    HostStage st(h, "flux");
    float* d_fl = nullptr;
    st.to(h->d_w, weights, (size_t)m.n_params);
    st.to(h->d_tmp_a, x, (size_t)n_columns * m.ns);
    st.to(h->d_tmp_b, bcs, (size_t)n_columns * m.n_bc);
    st.out(&d_fl, flux, (size_t)n_columns * m.n_nets * (m.Nz + 1));
    if (st.upload()) return 1;
    if (colnde_flux_dev(h, h->d_tmp_a, h->d_w, h->d_tmp_b, t, d_fl, n_columns)) return 1;
    return st.download();
}

extern "C" int colnde_loss_per_tstep_dev(colnde_handle* h, const float* d_weights, float* d_out) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!d_weights || !d_out) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    if (forward_impl(h, d_weights, h->d_sol, false)) return 1;
    hipError_t e = launch_loss_per_tstep(h->d_sol, h->d_truth, h->n_col, h->cfg.n_save, h->m.Nz, h->m.ns / h->m.Nz, d_out, h->stream);
    if (e != hipSuccess) return fail("loss_per_tstep launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_loss_per_tstep(colnde_handle* h, const float* weights, float* out) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!weights || !out) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    HostStage st(h, "loss_per_tstep");
    float* d_o = nullptr;
    st.to(h->d_w, weights, (size_t)user_params(h));
    st.out(&d_o, out, (size_t)h->n_col * 6 * h->cfg.n_save);
    if (st.upload()) return 1;
    if (colnde_loss_per_tstep_dev(h, h->d_w, d_o)) return 1;
    return st.download();
}

extern "C" int colnde_adam_step_dev(colnde_handle* h, float* d_weights, const float* d_grad, float* d_m, float* d_v, float eta,
                                    float beta1, float beta2, float eps, float beta1_t, float beta2_t, int n) {
    if (!h) return fail("null handle");
    if (!d_weights || !d_grad || !d_m || !d_v) return fail("null pointer argument");
    if (n < 1) return fail("n must be >= 1");
    if (!(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f)) return fail("0 <= beta < 1 required");
    if (!(beta1_t < 1.0f && beta2_t < 1.0f)) return fail("running powers beta^t must be < 1");
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_ADAM);
    hipError_t e = launch_adam_step(d_weights, d_grad, d_m, d_v, eta, beta1, beta2, eps, beta1_t, beta2_t, n, h->stream);
    if (e != hipSuccess) return fail("ADAM launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_coarse_grain_dev(colnde_handle* h, const float* d_in, int n_rows, int N, int n, int location, float* d_out) {
    if (!h) return fail("null handle");
    if (!d_in || !d_out) return fail("null pointer argument");
    if (n_rows < 1 || N < 2 || n < 2 || n > N) return fail("need n_rows >= 1 and 2 <= n <= N (n_rows = %d, N = %d, n = %d)", n_rows, N, n);
    if (location != 0 && location != 1) return fail("location must be 0 (Center) or 1 (Face)");
    if (location == 0 && N % n != 0) return fail("coarse_grain(Center): n = %d must divide N = %d", n, N);
    HIPCHK(hipSetDevice(h->device));
    hipError_t e = launch_coarse_grain(d_in, n_rows, N, n, location, d_out, h->stream);
    if (e != hipSuccess) return fail("coarse_grain launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_zscore_stats_dev(colnde_handle* h, const float* d_x, int64_t count, float* d_mu_sigma) {
    if (!h) return fail("null handle");
    if (!d_x || !d_mu_sigma) return fail("null pointer argument");
    if (count < 2) return fail("need at least two values for a standard deviation");
    HIPCHK(hipSetDevice(h->device));
    hipError_t e = launch_zscore_stats(d_x, (long)count, d_mu_sigma, h->stream);
    if (e != hipSuccess) return fail("zscore_stats launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_scale_dev(colnde_handle* h, const float* d_x, int64_t count, const float* d_mu_sigma, float* d_out) {
    if (!h) return fail("null handle");
    if (!d_x || !d_mu_sigma || !d_out) return fail("null pointer argument");
    if (count < 1) return fail("count must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    hipError_t e = launch_zscore_scale(d_x, (long)count, d_mu_sigma, d_out, h->stream);
    if (e != hipSuccess) return fail("scale launch failed: %s", hipGetErrorString(e));
    return 0;
}

// [grad; terms; total; 0] of this rank summed over the communicator, on the handle's stream (comm.hip)
extern "C" int colnde_comm_allreduce_dev(colnde_comm* c, float* d_buf, int64_t n, int op, void* hip_stream);
extern "C" int colnde_allreduce_result_dev(colnde_handle* h, colnde_comm* comm, float* d_out) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h || !comm || !d_out) return fail("null argument");
    return colnde_comm_allreduce_dev(comm, d_out, (int64_t)h->m.n_params + 8, 0, (void*)h->stream);
}

// ---- flux-MLP pre-training (second half) ---------------------------------------------------------------------
extern "C" int colnde_pretrain_flux_dev(colnde_handle* h, int flux_type, float* d_theta, float* d_m, float* d_v, const float* d_profiles,
                                        const float* d_bcs, const float* d_flux, const int32_t* d_order, int n_samples,
                                        float gradient_scaling, float eta, float beta1, float beta2, float eps, double beta_t[2],
                                        int update, float* mean_loss) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h) return fail("null handle");
    if (!d_theta || !d_profiles || !d_bcs || !d_flux || !beta_t || !mean_loss) return fail("null pointer argument");
    if (update && (!d_m || !d_v)) return fail("the ADAM moments are needed when update != 0");
    if (n_samples < 1) return fail("n_samples must be >= 1");
    const bool wm = h->m.model == COLNDE_MODEL_WIND_MIXING;
    if (flux_type < 0 || flux_type > 2 || (!wm && flux_type != 2)) return fail("flux_type: 0 = uw, 1 = vw, 2 = wT (T-only models: 2)");
    if (h->m.smooth_NN || h->m.smooth_Ri) return fail("flux pre-training does not cover the smoothing options");
    if (h->m.inplace) return fail("flux pre-training uses the training arithmetic (inplace_variant = 0)");
    if (!(beta_t[0] < 1.0 && beta_t[1] < 1.0)) return fail("running powers beta^t must be < 1");
    if (pretrain_lds_bytes(h->m) > PRETRAIN_LDS_CAP)
        return fail("network too large for flux pre-training: its one workgroup needs %zu B of LDS for the activations, pre-activations and deltas (> %zu)",
                    pretrain_lds_bytes(h->m), PRETRAIN_LDS_CAP);
    HIPCHK(hipSetDevice(h->device));
    DevScratch sc(h->stream);
    HIPCHK(sc.alloc(sizeof(float) + 2 * sizeof(double) + 8));
    float* d_loss = sc.p;
    double* d_bt = reinterpret_cast<double*>(reinterpret_cast<char*>(d_loss) + 8);
    hipError_t e = launch_pretrain(h->m, flux_type, d_theta, d_m, d_v, d_profiles, d_bcs, d_flux, d_order, n_samples, gradient_scaling,
                                   eta, beta1, beta2, eps, beta_t[0], beta_t[1], update, d_loss, d_bt, h->stream);
    float loss = 0.0f;
    double bt[2] = {beta_t[0], beta_t[1]};
    if (e == hipSuccess) e = hipMemcpyAsync(&loss, d_loss, sizeof(float), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(bt, d_bt, sizeof(bt), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail("flux pre-training failed: %s", hipGetErrorString(e));
    *mean_loss = loss / (float)n_samples;
    if (update) { beta_t[0] = bt[0]; beta_t[1] = bt[1]; }
    return 0;
}

extern "C" int colnde_plan(const colnde_handle* h, int info[8]) {
    if (!h || !info) return fail("null argument");
    for (int i = 0; i < 8; i++) info[i] = 0;
    info[0] = engine_id(h);
    // RKC2 on a model with a convective-adjustment switch: the gradient is the one-switch-pattern pullback (include/colnde.h)
    info[7] = (h->cfg.stepper == COLNDE_STEPPER_RKC2 && (h->m.model == COLNDE_MODEL_CONV_ADJ_NDE || (h->m.ca && !h->m.mpp))) ? 1 : 0;
    // bits 1..3: which kernel families run the exact three-way bf16 split (where the engine has a split kernel for this shape)
    bool bf_fwd = false, bf_adj = false, bf_dw = false;
    if (h->use_rt) {
        bf_fwd = h->sp_fwd && !h->rt_fwd32;
        bf_adj = h->sp_adj && (h->d_rt_tape ? h->rt_ztape : !h->rt_fwd32);     // (needs the Z1 tape; before the tapes are planned: the expectation)
        bf_dw = h->sp_dw;
    } else if (h->use_fc) {
        bf_fwd = h->sp_fwd && fc_split_supported(h->fc_cw);
        bf_adj = h->sp_adj && fc_split_supported(h->fc_cw);
        bf_dw = h->sp_dw && (h->d_dwtape ? !h->dw.passes.empty() : true);
    } else {
        bf_fwd = (h->sp_fwd && h->fwd_split && h->fwd_helper) || h->m.sf != nullptr;
        bf_adj = (h->sp_adj && h->adj_split && rt_adjoint_split_has_bf16(h->m, h->adj_helper) && (h->t16_dwtape < 0 || (h->t16_dwtape == 1 && h->d_t16_ztape))) || h->m.sb != nullptr;
        bf_dw = h->sp_dw && h->t16_dwtape == 1 && !h->dw.passes.empty();
    }
    info[7] |= (bf_fwd ? 2 : 0) | (bf_adj ? 4 : 0) | (bf_dw ? 8 : 0);
    // the block of the handle's engine; tile16 reports it once the delta tape is in use
    if (h->use_rt || h->use_fc || h->t16_dwtape == 1) {
        info[1] = h->blk.block;
        info[2] = h->blk.nblocks;
    }
    if (h->use_fc) {
        info[3] = h->fc_nseg > 1 ? h->fc_nseg : 0;       // fc32: time segments of the tapes (0: the tapes hold the whole axis)
        info[4] = h->d_dwtape ? 1 : 0;
        info[5] = h->d_dwtape ? h->dw.slices : 0;
        info[6] = h->conv.c;
    } else if (h->use_rt) {
        info[3] = h->rt_ztape ? 1 : 0;
    } else {
        info[4] = h->t16_dwtape == 1 ? 1 : 0;
        info[5] = h->t16_dwtape == 1 ? h->dw.slices : 0;
        info[6] = (h->fwd_split ? 1 : 0) | ((h->adj_split && h->t16_dwtape == 1 && h->d_t16_ztape) ? 2 : 0) | (h->split_rich ? 4 : 0);
    }
    return 0;
}

// the string, cut to the caller's buffer; returns the bytes the whole of it needs
static int copy_out(const std::string& s, char* buf, int capacity) {
    const int need = (int)s.size() + 1;
    if (buf && capacity > 0) {
        const int n = need <= capacity ? need - 1 : capacity - 1;
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return need;
}

extern "C" int colnde_describe(const colnde_handle* h, char* buf, int capacity) {
    if (!h) { fail("null argument"); return -1; }
    int info[8];
    if (colnde_plan(h, info)) return -1;
    std::string s;
    char t[256];
    if (h->closure) {
        snprintf(t, sizeof t, "engine=closure sets=%d columns=%d Nz=%d stepper=rk4 substeps=%d tape=step_start_states tape_bytes=%zu gradient=exact discrete adjoint",
                 h->n_models, h->n_col, h->m.Nz, h->cfg.substeps, h->cl_tape_bytes);
        s = t;
        const char* e = env_get(ENV_ALLOW_UNSTABLE_DT);
        s += " | env";
        if (e) { s += " COLNDE_ALLOW_UNSTABLE_DT="; s += e; } else s += " (none set)";
        return copy_out(s, buf, capacity);
    }
    const char* eng = info[0] == COLNDE_ENGINE_MFMA ? "regtile" : info[0] == COLNDE_ENGINE_FC32 ? "fc32" : ((info[6] & 1) ? "tile16+net-split" : "tile16");
    if (info[0] == COLNDE_ENGINE_FC32) info[6] = 0;                  // (fc32: the filter length of a conv handle, reported below; the bits are tile16's)
    char why[96] = "";
    if (h->auto_substeps) snprintf(why, sizeof why, "(stability bound; pending: the first solve chooses from reltol=%g)", h->cfg.reltol);
    else if (h->substeps_chosen) snprintf(why, sizeof why, "(chosen from reltol, estimate=%.3g)", h->last_estimate);
    snprintf(t, sizeof t, "engine=%s columns=%d stepper=%s substeps=%d%s", eng, h->cfg.n_columns, h->cfg.stepper == COLNDE_STEPPER_RKC2 ? "rkc2" : "rk4",
             h->cfg.substeps, why);
    s += t;
    if (!h->sched.empty()) { snprintf(t, sizeof t, " schedule=%d/%d intervals", total_steps(h), h->cfg.n_save - 1); s += t; }
    if (h->conv.c) { snprintf(t, sizeof t, " conv=%d n_params=%d", h->conv.c, h->conv.n_params); s += t; }
    if (h->ensemble) { snprintf(t, sizeof t, " models=%d tape_bytes_per_model=%zu", h->n_models, h->ens_model_bytes); s += t; }
    if (h->tile_ens) s += " tile_ensemble=1";      // colnde_create_tile_ensemble: tile16's own kernels; the bytes per model count images and activation rows too
    // a member loss that is set (colnde_ensemble_set_member_loss): scalings | columns | scalings+columns; without one the line is what it was (none)
    if (h->ensemble && (h->ml_scalings || h->ml_columns)) { snprintf(t, sizeof t, " member_loss=%s", member_loss_kind(h->ml_scalings, h->ml_columns)); s += t; }
    if (h->cfg.stepper == COLNDE_STEPPER_RKC2) { snprintf(t, sizeof t, " rkc_stages=%d%s", h->m.nst, h->cfg.rkc_stages ? "" : "(automatic)"); s += t; }
    snprintf(t, sizeof t, " matrix_arithmetic=%s forward=%s adjoint=%s dw=%s", h->cfg.matrix_arithmetic == COLNDE_MATRIX_BF16X3_EXACT ? "bf16x3_exact" : "f32_mfma",
             (info[7] & 2) ? "bf16x3" : "f32", (info[7] & 4) ? "bf16x3" : "f32", (info[7] & 8) ? "bf16x3" : "f32");
    s += t;
    if (wm_infer_covers(h)) s += " wm_infer=f32";      // colnde_wm_infer_dz_flux / colnde_wm_embedded_step[_flux] / colnde_wm_diagnose_flux: the f32 matrix pipe under either arithmetic
    if (wm_generic_serves(h)) s += " wm_embed=generic_f32";      // colnde_ensemble_wm_embedded with this single handle as K = 1: engine_wm_embed_any.hip, likewise
    if (h->ensemble && !h->use_fc && !h->tile_ens) s += " wm_profile=f32";      // colnde_ensemble_profile: likewise
    if (!h->conv.c && fce_covers(h)) s += " fc_embed=f32";      // colnde_fc_embedded_step / colnde_fc_diagnose_wT: likewise
    if (info[1]) { snprintf(t, sizeof t, " block=%dx%d", info[1], info[2]); s += t; } else s += " block=(not planned yet)";
    if (info[0] == COLNDE_ENGINE_MFMA) { snprintf(t, sizeof t, " z1_tape=%d", info[3]); s += t; }
    if (info[0] == COLNDE_ENGINE_FC32) { snprintf(t, sizeof t, " time_segments=%d tile_width=%d dw_slices=%d", info[3], h->fc_cw, info[5]); s += t; }
    if (h->ag_rows) s += " activation_rows=global_memory(L2)";
    if (info[0] == COLNDE_ENGINE_GENERIC) {
        snprintf(t, sizeof t, " dw_taped=%d dw_slices=%d net_split_forward=%d net_split_adjoint=%d rich_tape=%d", info[4], info[5], info[6] & 1, (info[6] >> 1) & 1, (info[6] >> 2) & 1);
        s += t;
    }
    snprintf(t, sizeof t, " gradient=%s", (info[7] & 1) ? "one-switch-pattern RKC2 pullback (approximate)" : "exact discrete adjoint");
    s += t;
    s += " | env";
    bool any = false;
    for (int i = 0; i < ENV_COUNT; i++) {
        const char* e = env_get((EnvSwitch)i);
        if (e) { s += " "; s += COLNDE_ENV_SWITCHES[i]; s += "="; s += e; any = true; }
    }
    if (!any) s += " (none set)";
    // an environment override that contradicts the arithmetic selected through the API (colnde_config.matrix_arithmetic / colnde_set_matrix_arithmetic) wins —
    // say so, by name (it used to outrank the API call silently)
    {
        const bool split = h->cfg.matrix_arithmetic == COLNDE_MATRIX_BF16X3_EXACT;
        const struct { const char* name; bool v; } fam[3] = {{"COLNDE_FWD_SPLIT", h->sp_fwd}, {"COLNDE_ADJ_SPLIT", h->sp_adj}, {"COLNDE_DW_SPLIT", h->sp_dw}};
        for (const auto& f : fam)
            if (f.v != split) { snprintf(t, sizeof t, " | WARNING %s=%d overrides matrix_arithmetic=%s for its kernels", f.name, f.v ? 1 : 0, split ? "bf16x3_exact" : "f32_mfma"); s += t; }
    }
    return copy_out(s, buf, capacity);
}

// Diagnostic builds (-DCOLNDE_STAMPS) only; not part of include/colnde.h.  Returns zeros in the shipped library.
extern "C" int colnde_debug_stamps(colnde_handle* h, unsigned long long* out16) {
    if (!h || !out16) return fail("null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->use_rt || h->adj_split) {      // each translation unit keeps the stamps of its own kernels
        for (int i = 0; i < 16; i++) out16[i] = 0;
        HIPCHK(h->use_rt ? rt_debug_read_stamps(out16) : rt_debug_read_stamps_split(out16));
        return 0;
    }
    HIPCHK(debug_read_stamps(out16));
    return 0;
}
