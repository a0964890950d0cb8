// api.hip — the C ABI of include/colnde.h on top of the MFMA tile engine.  gfx950 only; no CPU fallback.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

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

// ---- model construction -----------------------------------------------------------------------------
static int validate(const colnde_config* c) {
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
static double stiff_lambda(const colnde_config* c) {
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
    const double need = span * stiff_lambda(c) / COLNDE_RK4_REAL_BOUND;
    return need <= 1.0 ? 1 : (int)ceil(need);
}

// inv_dRi, inv_Pr and c_rib of the Richardson-number closure from the five Pacanowski-Philander constants: ONE expression for the single
// handle (build_model) and for every model of an ensemble, so that model k and a handle built with model k's constants see identical floats
static RtPhys closure_constants(float nu0, float nu_minus, float dRi, float Ric, float Pr) {
    RtPhys p;
    p.nu0 = nu0; p.nu_minus = nu_minus; p.Ric = Ric; p.inv_dRi = 1.0f / dRi; p.inv_Pr = 1.0f / Pr; p.c_rib = -nu_minus / (2.0f * dRi);
    p.pad0 = 0.0f; p.pad1 = 0.0f;
    return p;
}

static void build_model(const colnde_config* c, DevModel* m, PackInfo* pk) {
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
static void resolve_arithmetic(colnde_handle* h) {
    const bool split = h->cfg.matrix_arithmetic == COLNDE_MATRIX_BF16X3_EXACT;
    auto ov = [split](const char* name) {
        const char* e = getenv(name);
        return (e && *e) ? atoi(e) != 0 : split;
    };
    h->sp_fwd = ov("COLNDE_FWD_SPLIT");
    h->sp_adj = ov("COLNDE_ADJ_SPLIT");
    h->sp_dw = ov("COLNDE_DW_SPLIT");
    // tile16 with rows in global memory: the dense chains follow the arithmetic (plane images packed beside the f32 ones)
    h->m.sf = (h->ag_rows && h->sp_fwd) ? h->d_sf : nullptr;
    h->m.sb = (h->ag_rows && h->sp_adj) ? h->d_sb : nullptr;
}

// DevModel::ag for `tiles` workgroups (zero-filled once: the pad slots behind a layer's last feature are never written and must read as zero)
int ensure_ag(colnde_handle* h, size_t tiles) {
    if (!h->ag_rows || h->ag_tiles >= tiles) return 0;
    (void)hipStreamSynchronize(h->stream);
    if (h->d_ag) { (void)hipFree(h->d_ag); h->d_ag = nullptr; h->m.ag = nullptr; h->ag_tiles = 0; }
    const size_t bytes = tiles * ag_floats_per_tile(h->m) * sizeof(float);
    if (hipMalloc((void**)&h->d_ag, bytes) != hipSuccess) { (void)hipGetLastError(); return fail("hipMalloc of the activation rows (%zu B) failed", bytes); }
    if (hipMemset(h->d_ag, 0, bytes) != hipSuccess) return fail("hipMemset of the activation rows failed");
    h->ag_tiles = tiles;
    h->m.ag = h->d_ag;
    return 0;
}

// The RKC2 coefficient table for the sub-step count now in h->cfg: with rkc_stages = 0 the stage count FOLLOWS the step (least s with 0.9 beta(s) >= lambda dt),
// so colnde_choose_substeps / colnde_set_substeps / the doubled solve of colnde_error_estimate each run with the stage count their own step needs (a table
// frozen at creation would be too short for a longer step — unstable — and wastefully long for a shorter one).  Uploaded in stream order.
static int refresh_rkc(colnde_handle* h) {
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

extern "C" int colnde_create(const colnde_config* cfg, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (validate(cfg)) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail("no HIP device visible: colnde has no CPU fallback (the product path is the gfx950 HIP engine)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail("device %d not in 0..%d", cfg->device, ndev - 1);
    HIPCHK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("device %d is %s; this library is built for gfx950 (MI355X) only", cfg->device, prop.gcnArchName);

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
        if (hipMalloc((void**)&h->d_rkc, (size_t)6 * RKC_LD * sizeof(float)) != hipSuccess) {
            delete h;
            return fail("allocating the RKC coefficient table failed");
        }
        h->m.rkc = h->d_rkc;
        if (refresh_rkc(h)) { colnde_destroy(h); return 1; }
    }
    std::vector<TileDesc> tiles;
    std::vector<int> bz, bg;
    build_tables(h->m, &tiles, &bz, &bg);
    h->m.n_tiles = (int)tiles.size();
    const size_t lds_cap = 160 * 1024;
    {   // COLNDE_ADJ_GEOM=<index> / COLNDE_FWD_WLDS=0|1 / COLNDE_FWD_THREADS=256|512 override the heuristics (tuning aid)
        const char* eg = getenv("COLNDE_ADJ_GEOM");
        h->geo_ok = pick_adjoint_geom(h->m, &h->geo, eg ? atoi(eg) : -1);
    }
    h->lds_fwd = lds_floats_forward(h->m) * sizeof(float);
    h->lds_adj = h->geo_ok ? lds_floats_adjoint_geom(h->m, h->geo) * sizeof(float) : lds_floats_adjoint(h->m) * sizeof(float);
    {
        const size_t wl = ((size_t)((h->m.n_params + 3) & ~3) + 128) * sizeof(float);
        // Weights staged in LDS when they fit — unless that leaves room for only ONE workgroup per CU on a problem with more tiles than
        // CUs: there two 256-thread workgroups streaming the packed image from L2 (four k-steps per load) are faster
        // (32-128-128-31, 16,384 columns: forward 55.8 -> 42.9 ms); latency points keep the LDS copy (no L2 round trip per chain).
        h->fwd_wlds = h->lds_fwd + wl <= lds_cap && (h->n_tiles <= 256 || 2 * (h->lds_fwd + wl) <= lds_cap);
        const char* ew = getenv("COLNDE_FWD_WLDS");
        if (ew) h->fwd_wlds = h->lds_fwd + wl <= lds_cap && atoi(ew) != 0;
        // weights in LDS: 1,024 threads (four waves per SIMD; 8 simulations 19.7 vs 21.3 ms at 512, 32-128-128-31 54.7 vs 55.7 ms);
        // weights streamed from L2 (64-256-256-63): two independent 256-thread workgroups per CU do better (113 vs 121 ms)
        h->fwd_threads = h->fwd_wlds ? 1024 : 256;
        const char* et = getenv("COLNDE_FWD_THREADS");
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
            delete h;
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
            const char* et = getenv("COLNDE_FWD_THREADS");
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
        if (hipMalloc((void**)&h->d_sf, (size_t)fo * h->m.n_nets * 16) != hipSuccess || hipMalloc((void**)&h->d_sb, (size_t)bo * h->m.n_nets * 16) != hipSuccess) {
            (void)hipGetLastError();
            colnde_destroy(h);
            return fail("allocating the bf16 plane images failed");
        }
        resolve_arithmetic(h);
    }
    if (h->lds_adj > lds_cap) h->geo_ok = false;
    {
        hipError_t e = set_kernel_attributes(lds_cap);
        if (e == hipSuccess) e = rt_set_attributes();
        if (e != hipSuccess) { delete h; return fail("hipFuncSetAttribute failed: %s", hipGetErrorString(e)); }
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
        const char* eh = getenv("COLNDE_T16_FWD_HELPER");      // 0: the three-wave forward (8 simulations 9.8 vs 8.3 ms, 4,096 columns 8.27 vs 7.65 ms)
        h->fwd_helper = !(eh && atoi(eh) == 0);
        const char* eah = getenv("COLNDE_T16_ADJ_HELPER");     // 0: the three-wave adjoint (8 simulations 11.3 vs 8.2 ms)
        h->adj_helper = !(eah && atoi(eah) == 0);
        const bool stepper_ok = cfg->stepper == COLNDE_STEPPER_RK4 || (cfg->stepper == COLNDE_STEPPER_RKC2 && h->fwd_helper && h->adj_helper);
        h->fwd_split = !h->use_rt && rt_supported(h->m) && stepper_ok && cfg->engine == COLNDE_ENGINE_AUTO;
        const char* es = getenv("COLNDE_T16_FWD_SPLIT");
        if (es) h->fwd_split = !h->use_rt && rt_supported(h->m) && stepper_ok && atoi(es) != 0;
        // the gradient behind a split forward: rt16s_adjoint_kernel (same decomposition) when the taped mode with both tapes is planned
        const char* ea = getenv("COLNDE_T16_ADJ_SPLIT");
        h->adj_split = h->fwd_split && !(ea && atoi(ea) == 0);
    }
    if (cfg->engine == COLNDE_ENGINE_MFMA && !h->use_rt) {
        delete h;
        return fail("engine = regtile requested, but it covers only Nz=32, three 96-50-20-31 nets, no smoothing, training RHS, RK4");
    }
    // AUTO on the free-convection shape the reference trains: the 32-column engine (COLNDE_FC=0 keeps tile16)
    {
        const char* ef = getenv("COLNDE_FC");
        h->use_fc = fc_supported(h->m, cfg->stepper) && (cfg->engine == COLNDE_ENGINE_FC32 || (cfg->engine == COLNDE_ENGINE_AUTO && !(ef && atoi(ef) == 0)));
        if (cfg->engine == COLNDE_ENGINE_FC32 && !h->use_fc) {
            delete h;
            return fail("engine = fc32 requested, but it covers only FreeConvectionNDE (RK4) and ConvectiveAdjustmentNDE (RK4, RKC2) with Dense(Nz,4Nz,relu), Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1), Nz = 32 or 64");
        }
        if (h->use_fc) {
            h->fc_cw = fc_tile_width(cfg->n_columns);
            hipError_t e = fc_set_kernel_attributes();
            if (e != hipSuccess) { delete h; return fail("hipFuncSetAttribute (fc32) failed: %s", hipGetErrorString(e)); }
        }
    }
    const DevModel& m = h->m;
#define ALLOC(ptr, n, T)                                                                   \
    do {                                                                                   \
        hipError_t e_ = hipMalloc((void**)&(ptr), (size_t)(n) * sizeof(T));                \
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
    void* ptrs[] = {h->d_rt_tapez, h->d_rt_tape, h->d_rt_tape2, h->d_rt_slab, h->d_wimg, h->d_w, h->d_wf, h->d_wb, h->d_x0, h->d_bcs, h->d_truth, h->d_sol, h->d_tape, h->d_slab, h->d_out,
                    h->d_times, h->d_partial, h->d_tmp_a, h->d_tmp_b, h->d_tmp_c, h->d_tiles, h->d_bias_zoff, h->d_bias_goff, h->d_dwtape, h->d_macros, h->d_t16_ztape, h->d_rkc, h->d_ag, h->d_sf, h->d_sb,
                    h->d_fc_imgf, h->d_fc_imgb, h->d_fc_bias, h->d_fc_masks, h->d_fc_switch, h->d_fc_lam, h->d_fc_simgf, h->d_fc_simgb, h->d_phys, h->d_wm_ens_mpp,
                    h->d_cl_tape, h->d_cl_rows, h->d_cl_params, h->conv.d_wpad, h->conv.d_gpad, h->conv.d_ctape, h->conv.d_cslab};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    dw_split_free(h->dw_split);
    delete h;
}

// parameters of the vector the caller passes: the model's, except behind a conv filter (the handle's internal vector pads W1)
static int user_params(const colnde_handle* h) { return h->conv.c ? h->conv.n_params : h->m.n_params; }
extern "C" int colnde_n_params(const colnde_handle* h) { return h ? user_params(h) : -1; }
extern "C" int colnde_conv_filter(const colnde_handle* h) { return h ? h->conv.c : -1; }
extern "C" int colnde_engine(const colnde_handle* h) { return h ? (h->use_rt ? COLNDE_ENGINE_MFMA : (h->use_fc ? COLNDE_ENGINE_FC32 : COLNDE_ENGINE_GENERIC)) : -1; }

extern "C" int colnde_set_stream(colnde_handle* h, void* s) {
    if (!h) return fail("null handle");
    h->stream = (hipStream_t)s;
    return 0;
}

extern "C" int colnde_set_matrix_arithmetic(colnde_handle* h, int ma) {
    if (!h) return fail("null handle");
    if (ma != COLNDE_MATRIX_BF16X3_EXACT && ma != COLNDE_MATRIX_F32_MFMA)
        return fail("unknown matrix_arithmetic %d (COLNDE_MATRIX_BF16X3_EXACT = 0, COLNDE_MATRIX_F32_MFMA = 1)", ma);
    h->cfg.matrix_arithmetic = ma;
    resolve_arithmetic(h);
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
        if (!h->d_truth) HIPCHK(hipMalloc((void**)&h->d_truth, n * sizeof(float)));
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

static void loss_weights(const colnde_handle* h, const float scalings[6], LossWeights* lw) {
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
    for (float** p : {&h->d_tmp_a, &h->d_tmp_b, &h->d_tmp_c})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    h->tmp_cols = 0;
    HIPCHK(hipMalloc((void**)&h->d_tmp_a, n_columns * h->m.ns * sizeof(float)));
    HIPCHK(hipMalloc((void**)&h->d_tmp_b, n_columns * 8 * sizeof(float)));
    HIPCHK(hipMalloc((void**)&h->d_tmp_c, n_columns * h->m.ns * sizeof(float)));
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

// Sizes the regtile engine's tapes.  They hold ONE block of columns; a problem whose tapes exceed the free HBM (many columns, or a
// long horizon: 1,153 frames need 4x the bytes per column of the 2-day suite) runs its gradient path block after block into the same
// buffers.  COLNDE_RT_BLOCK=<columns> forces a block size (testing aid).
static int rt_plan_tapes(colnde_handle* h) {
    if (h->d_rt_tape) return 0;
    const int n_steps = (h->cfg.n_save - 1) * h->cfg.substeps;
    const char* ez = getenv("COLNDE_RT_ZTAPE");
    bool want_z = !h->rt_fwd32 && !(ez && atoi(ez) == 0);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t margin = (size_t)2 << 30;
    const size_t budget = free_b > margin ? free_b - margin : 0;
    const size_t per_col_x = (size_t)n_steps * 4 * 96 * sizeof(float), per_col_2 = (size_t)n_steps * 4 * ((21 * 256) / 32) * sizeof(float);
    const size_t per_col_z = rt_tapez_floats(32, n_steps) / 32 * sizeof(float);      // (twice per_col_2 in the A/B build that tapes activation pairs)
    const int n32 = ((h->n_col + 31) / 32) * 32;
    int block = 0;
    for (int pass = 0; pass < 2 && block == 0; pass++) {
        const size_t per_col = per_col_x + per_col_2 + (want_z ? per_col_z : 0);
        const size_t fit = budget / per_col;
        if (fit >= (size_t)n32) block = n32;
        else if (fit >= 1024) {
            const int nb = (int)(((size_t)n32 + fit - 1) / fit);
            block = (((n32 + nb - 1) / nb) + 1023) / 1024 * 1024;
            if ((size_t)block > fit) block = (int)(fit / 1024) * 1024;
        } else if (want_z) want_z = false;       // not even 1,024 columns with the Z1 tape: try without it
    }
    const char* eb = getenv("COLNDE_RT_BLOCK");
    if (eb && atoi(eb) >= 32) block = std::min(n32, (atoi(eb) / 32) * 32);
    if (block == 0) return fail("the stage tapes of even 1,024 columns (%zu bytes per column) do not fit in %zu free bytes of HBM",
                                per_col_x + per_col_2, free_b);
    const size_t n1 = rt_tape_floats(block, n_steps), n2 = rt_tape2_floats(block, n_steps);
    hipError_t e = hipMalloc((void**)&h->d_rt_tape, n1 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_rt_tape2, n2 * sizeof(float));
    h->rt_ztape = want_z;
    if (e == hipSuccess && h->rt_ztape && hipMalloc((void**)&h->d_rt_tapez, rt_tapez_floats(block, n_steps) * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        h->d_rt_tapez = nullptr;
        h->rt_ztape = false;
    }
    if (e != hipSuccess) {
        for (float** q : {&h->d_rt_tape, &h->d_rt_tape2, &h->d_rt_tapez})      // leave no half-built state behind
            if (*q) { (void)hipFree(*q); *q = nullptr; }
        return fail("hipMalloc of the %zu-byte stage tapes failed: %s", (n1 + n2) * sizeof(float), hipGetErrorString(e));
    }
    h->rt_block = block;
    h->rt_nblocks = (n32 + block - 1) / block;
    return 0;
}

// regtile forward solve of columns [c0, c0 + nc): sol rows and, when taping, the block's tapes
static int rt_forward_range(colnde_handle* h, float* d_sol, bool with_tape, int c0, int nc) {
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
static int t16_forward_range(colnde_handle* h, const float* d_weights, float* d_sol, bool with_tape, int c0, int nc) {
    const size_t ns = h->m.ns;
    if (with_tape && !h->d_tape) {     // in-register gradient mode: the whole problem's stage tape
        const size_t n = (size_t)h->n_tiles * (h->cfg.n_save - 1) * h->cfg.substeps * h->m.nst * CT * ns;
        hipError_t e = hipMalloc((void**)&h->d_tape, n * sizeof(float));
        if (e != hipSuccess) return fail("hipMalloc of the %zu-byte stage tape failed: %s", n * sizeof(float), hipGetErrorString(e));
    }
    Timed tm(h, K_FORWARD);
    if (h->fwd_split) {
        // latency points of the wind-mixing shape: one wavefront per flux net (+ a helper) per 16-column tile (engine_regtile.hip); the tapes
        // come out in tile16's formats for its taped adjoint
        hipError_t es = rt_launch_pack(h->m, d_weights, h->d_wimg, h->stream);
        if (es == hipSuccess)
            es = rt_launch_forward_split(h->m, h->d_wimg, h->d_x0 + (size_t)c0 * ns, h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times, h->cfg.n_save,
                                         h->cfg.substeps, d_sol ? d_sol + (size_t)c0 * h->cfg.n_save * ns : nullptr,
                                         with_tape ? h->d_tape : nullptr, with_tape ? h->d_t16_ztape : nullptr, nc, with_tape && h->split_rich, h->fwd_helper, h->sp_fwd, h->stream);
        if (es != hipSuccess) return fail("split forward launch failed: %s", hipGetErrorString(es));
        return 0;
    }
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
static FcConv fc_conv_args(const colnde_handle* h) {
    FcConv cv;
    cv.c = h->conv.c;
    cv.wb = h->conv.d_user;
    cv.ctape = h->conv.d_ctape;
    return cv;
}

// The vector the fc32 engine packs: the caller's, or — behind a conv filter — its dense part with W1 padded to 4Nz x Nz (one small kernel on the stream)
static int fc_engine_weights(colnde_handle* h, const float* d_weights, const float** d_engine) {
    *d_engine = d_weights;
    if (!h->conv.c) return 0;
    h->conv.d_user = d_weights;
    hipError_t e = launch_fc_conv_pad(d_weights, h->conv.c, h->conv.w1_end, h->conv.n_zero, h->m.n_params, h->conv.d_wpad, h->stream);
    if (e != hipSuccess) return fail("conv weight padding launch failed: %s", hipGetErrorString(e));
    *d_engine = h->conv.d_wpad;
    return 0;
}

static int fc_forward_range(colnde_handle* h, float* d_sol, bool with_tape, int c0, int nc, int iv0 = 0, int iv1 = -1, int tape_iv0 = -1) {
    const size_t ns = h->m.ns;
    const FcConv cv = fc_conv_args(h);
    if (iv1 < 0) iv1 = h->cfg.n_save - 1;
    if (tape_iv0 < 0) tape_iv0 = iv0;                // (a later tape_iv0: the tape-less pass of a segmented gradient tapes its last segment on the way)
    const float* init = iv0 == 0 ? h->d_x0 + (size_t)c0 * ns : d_sol + ((size_t)c0 * h->cfg.n_save + iv0) * ns;
    const size_t stride = iv0 == 0 ? ns : (size_t)h->cfg.n_save * ns;
    Timed tm(h, K_FORWARD);
    hipError_t e = fc_launch_forward(h->m, h->fc_cw, h->d_fc_imgf, (h->sp_fwd && fc_split_supported(h->fc_cw)) ? h->d_fc_simgf : nullptr, h->d_fc_bias, init, stride, h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times, h->cfg.n_save,
                                     iv0, iv1, tape_iv0, h->cfg.substeps, d_sol ? d_sol + (size_t)c0 * h->cfg.n_save * ns : nullptr,
                                     with_tape ? h->d_dwtape : nullptr, with_tape ? h->d_fc_masks : nullptr, with_tape ? h->d_fc_switch : nullptr, nc,
                                     h->stream, nullptr, h->conv.c ? &cv : nullptr);
    if (e != hipSuccess) return fail("fc32 forward launch failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- forward solve -------------------------------------------------------------------------------------
// A time step outside RK4's stability region gives a blown-up or NaN trajectory, loss and gradient with rc = 0: refuse it.
static int check_stability(const colnde_handle* h) {
    if (h->cfg.substeps >= h->min_substeps) return 0;
    const char* e = getenv("COLNDE_ALLOW_UNSTABLE_DT");
    if (e && atoi(e) != 0) return 0;
    if (h->cfg.stepper == COLNDE_STEPPER_RKC2)
        return fail("substeps = %d with %d RKC2 stages does not cover the stiffest diffusive mode (lambda = -%.4g): need substeps >= %d, "
                    "or rkc_stages = 0 for the automatic stage count (COLNDE_ALLOW_UNSTABLE_DT=1 overrides)",
                    h->cfg.substeps, h->m.nst, stiff_lambda(&h->cfg), h->min_substeps);
    return fail("substeps = %d puts the RK4 step outside its stability region: the stiffest diffusive mode this configuration can "
                "switch on has lambda = -%.4g (4 D Nz^2), and lambda dt must stay within %.3f — need substeps >= %d "
                "(colnde_min_substeps; the reference uses a stabilised ROCK4 here; COLNDE_ALLOW_UNSTABLE_DT=1 overrides)",
                h->cfg.substeps, stiff_lambda(&h->cfg), COLNDE_RK4_REAL_BOUND, h->min_substeps);
}

static int choose_substeps_impl(colnde_handle* h, const float* d_weights, float reltol, int* chosen, float* estimate);

// substeps = 0 picks the count from THIS handle's columns.  On a column shard (colnde_set_global_columns > the local count) every rank would settle on its
// own count: the SUM-all-reduced gradient would mix discretisations and the tapes would differ per rank.  The sharded recipe is explicit:
// colnde_choose_substeps on every rank, MAX over ranks, colnde_set_substeps (colnde.distributed.agree_substeps does exactly that).
static int refuse_auto_on_a_shard(const colnde_handle* h) {
    if (h->n_col_total > h->n_col)
        return fail("substeps = 0 (chosen from reltol) on a column shard (%d of %lld columns): each rank would choose its own count — call colnde_choose_substeps "
                    "on every rank, take the MAX over ranks and impose it with colnde_set_substeps", h->n_col, (long long)h->n_col_total);
    return 0;
}

static int forward_impl(colnde_handle* h, const float* d_weights, float* d_sol, bool with_tape) {
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
        const float* d_we = nullptr;
        if (fc_engine_weights(h, d_weights, &d_we)) return 1;
        hipError_t e = fc_launch_pack(h->m, h->fc_cw, d_we, h->d_fc_imgf, h->d_fc_imgb, h->d_fc_bias, h->d_fc_simgf, h->d_fc_simgb, h->stream);
        if (e != hipSuccess) return fail("fc32 pack launch failed: %s", hipGetErrorString(e));
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

// tile16, taped weight gradients: decide once per handle.  On when the tapes fit in the free HBM (the in-register adjoint_kernel
// geometries remain the fallback; 64-256-256-63's 384 gradient tiles spill there);
// COLNDE_T16_DWTAPE=1 / 0 forces it on / off.
// The dW GEMM's work list: 64x64 blocks of every layer's weight matrix, and the number of K-slices of the records
static void build_dw_macros(colnde_handle* h, size_t n_rec, std::vector<DwMacro>& mac) {
    const DevModel& m = h->m;
    const size_t R = dwtape_row_floats(m);
    std::vector<int> matrix_of;
    for (int net = 0; net < m.n_nets; net++)
        for (int l = 0; l < m.n_layers; l++) {
            const int ni = m.sizes[l], no = m.sizes[l + 1];
            for (int i0 = 0; i0 < ni; i0 += 64)
                for (int j0 = 0; j0 < no; j0 += 64) {
                    DwMacro d;
                    d.a_feat = l == 0 ? i0 : dwtape_ns4(m) + net * dwtape_act4(m) + m.act_off[l - 1] + i0;
                    d.d_feat = dwtape_ns4(m) + (m.n_nets + net) * dwtape_act4(m) + m.act_off[l] + j0;
                    d.ni_rem = std::min(64, ni - i0);
                    d.no_rem = std::min(64, no - j0);
                    d.g_off = net * m.net_size + m.w_off[l] + i0 * no + j0;
                    d.no = no;
                    mac.push_back(d);
                    matrix_of.push_back(net * m.n_layers + l);
                }
        }
    h->n_macros = (int)mac.size();
    dw_split_free(h->dw_split);
    // the split (bf16-pipe) dW GEMM keeps only a pass's operand FEATURES in LDS, as planes: it also serves records that do not fit the LDS whole (the wide
    // wind-mixing networks: 325 KB per 16-column record), with the large matrices cut into chunks of output blocks (dw_split_build)
    const bool lds_fit = dw_gemm_lds_fits((int)R, h->n_macros);
    const bool split_ok = dw_split_build(mac, matrix_of, (int)R, h->dw_split);
    const int n_groups = (h->n_macros + 3) / 4;
    size_t slices = std::max<size_t>(8, ((size_t)2048 / n_groups + 7) / 8 * 8);
    slices = std::min(slices, std::max<size_t>(8, (n_rec / 8 + 7) / 8 * 8));
    if (lds_fit || (split_ok && h->sp_dw))           // one workgroup per CU (two records / two plane buffers in LDS): two rounds of slices
        slices = std::min<size_t>(512, std::max<size_t>(1, n_rec));
    h->dw_slices = (int)slices;
}

// fc32 gradient path: the records (forward: xs, a1, a2; adjoint: dz1, dz2, dz3) and the bit tapes.  When they do not fit in the free HBM for the
// whole problem there are two ways to cut it:
//   * column blocks (a multiple of the 32-column tile): forward -> adjoint -> dW GEMM block after block.  No extra work, but a block of fewer than
//     16,384 columns leaves CUs with one workgroup or none (the kernels get their speed from two per CU);
//   * time segments: ALL columns, the tapes hold `fc_seg` save intervals.  One tape-less forward pass first (it saves the state at every save
//     point, and tapes the last segment on its way), then, from the last segment to the first, a taped forward restarted from the saved state,
//     the adjoint over the segment (λ handed on through d_fc_lam) and the dW GEMM.  Costs (n_seg - 1)/n_seg of an extra forward solve, keeps every
//     CU at two workgroups.
// Blocks are used when they hold at least 16,384 columns (or everything), segments otherwise; COLNDE_FC_BLOCK=<columns> / COLNDE_FC_SEG=<intervals> force.
static int fc_plan_tapes(colnde_handle* h) {
    if (h->d_dwtape) return 0;
    const DevModel& m = h->m;
    const int n_iv = h->cfg.n_save - 1;
    const size_t R = dwtape_row_floats(m);
    if (R != fc_record_row_floats(m.Nz)) return fail("fc32: record layout mismatch (%zu vs %zu floats per column)", R, fc_record_row_floats(m.Nz));
    const bool ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE;
    // bytes of tape per column and save interval
    const int cw = h->fc_cw;
    const size_t per_col_iv = (size_t)h->cfg.substeps * m.nst * (R * sizeof(float) + fc_mask_words() * sizeof(unsigned int) / cw + (ca ? sizeof(unsigned long long) : 0) +
                                                                 (h->conv.c ? fc_conv_tape_floats(m.Nz) / 16 * sizeof(float) : 0));      // (conv handles: the conv tape)
    const int n32 = (h->n_col + 31) / 32 * 32;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t margin = ((size_t)3 << 30) + (size_t)(n32 / cw * 8 + 4096) * (m.n_params + 8) * sizeof(float) + (size_t)n32 * m.Nz * sizeof(float);
    const size_t budget = free_b > margin ? free_b - margin : 0;
    const size_t fit = budget / (per_col_iv * n_iv);                 // columns whose whole-axis tapes fit
    int block = 0, seg = n_iv;
    if (fit >= (size_t)n32) block = n32;
    else {
        if (fit >= 32) {
            const int nb = (int)(((size_t)n32 + fit - 1) / fit);
            block = ((n32 + nb - 1) / nb + 31) / 32 * 32;
            if (block >= 8192) block = (block + 8191) / 8192 * 8192;       // whole rounds of one workgroup pair per CU
            while ((size_t)block > fit) block -= block > 8192 ? 8192 : 32;
        }
        if (block < 16384) {
            // time segments of all columns instead (or of the largest column block one interval fits for)
            const size_t cols_iv = budget / per_col_iv / 32 * 32;     // columns whose ONE-interval tapes fit
            if (cols_iv >= 32) {
                block = (int)std::min<size_t>((size_t)n32, cols_iv);
                if (block < n32 && block >= 8192) block = block / 8192 * 8192;
                seg = (int)std::min<size_t>((size_t)n_iv, budget / (per_col_iv * (size_t)block));
                // the partial-gradient slab grows with the number of segments ([tile][segment] + [block][segment][<= 512 slices] rows of n_params + 8
                // floats: 50 GB at 128 segments of the 64-level network): it must fit beside the tapes it is chosen for
                auto slab_bytes = [&](int sg) {
                    const size_t nsg = ((size_t)n_iv + sg - 1) / sg, nblk = ((size_t)n32 + block - 1) / block;
                    return ((size_t)(n32 / cw) + nblk * 512) * nsg * (size_t)(m.n_params + 8) * sizeof(float);
                };
                while (seg > 1 && per_col_iv * (size_t)block * seg + slab_bytes(seg) > budget) seg--;
                if (per_col_iv * (size_t)block * seg + slab_bytes(seg) > budget) seg = 0;      // not even one interval with its slab: reported below
            }
        }
    }
    const char* eb = getenv("COLNDE_FC_BLOCK");
    if (eb && atoi(eb) >= 32) { block = std::min(n32, (atoi(eb) / 32) * 32); if (!getenv("COLNDE_FC_SEG")) seg = n_iv; }
    const char* es = getenv("COLNDE_FC_SEG");
    if (es && atoi(es) >= 1) seg = std::min(n_iv, atoi(es));
    if (block < 32 || seg < 1) return fail("fc32: the tapes of even one 32-column tile and one save interval (%zu bytes) do not fit in the free device memory", 32 * per_col_iv);
    h->fc_block = block;
    h->fc_nblocks = (n32 + block - 1) / block;
    h->fc_seg = seg;
    h->fc_nseg = (n_iv + seg - 1) / seg;
    const size_t tiles_b = (size_t)block / cw;                                  // (block is a multiple of 32)
    const size_t stage_recs = (size_t)seg * h->cfg.substeps * m.nst;          // (tile, stage) records per tile held by the tapes
    const size_t n_rec = tiles_b * (cw / 16) * stage_recs;                     // records are tile16's: 16 columns each
    std::vector<DwMacro> mac;
    build_dw_macros(h, n_rec, mac);
    h->fc_rows = (n32 / cw) * h->fc_nseg + h->fc_nblocks * h->fc_nseg * h->dw_slices;
    const int stride = m.n_params + 8;
    hipError_t e = hipMalloc((void**)&h->d_dwtape, n_rec * CT * R * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_fc_masks, tiles_b * stage_recs * fc_mask_words() * sizeof(unsigned int));
    if (e == hipSuccess && ca) e = hipMalloc((void**)&h->d_fc_switch, tiles_b * stage_recs * fc_switch_words(cw) * sizeof(unsigned long long));
    if (e == hipSuccess && h->fc_nseg > 1) e = hipMalloc((void**)&h->d_fc_lam, (size_t)n32 * m.Nz * sizeof(float));
    if (e == hipSuccess && h->conv.c) {
        h->conv.cslab_rows = h->fc_nblocks * h->fc_nseg * FC_CONV_GRAD_MAX_SLICES;
        e = hipMalloc((void**)&h->conv.d_ctape, n_rec * fc_conv_tape_floats(m.Nz) * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&h->conv.d_cslab, (size_t)h->conv.cslab_rows * FC_CONV_GRAD_SLOTS * sizeof(float));
    }
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_macros, mac.size() * sizeof(DwMacro));
    if (e == hipSuccess) e = hipMemcpy(h->d_macros, mac.data(), mac.size() * sizeof(DwMacro), hipMemcpyHostToDevice);
    if (e == hipSuccess && !h->d_slab) e = hipMalloc((void**)&h->d_slab, (size_t)h->fc_rows * stride * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (void** p : {(void**)&h->d_dwtape, (void**)&h->d_fc_masks, (void**)&h->d_fc_switch, (void**)&h->d_fc_lam, (void**)&h->d_macros, (void**)&h->conv.d_ctape,
                         (void**)&h->conv.d_cslab})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        return fail("fc32: hipMalloc of the tapes (%zu bytes for %d columns x %d save intervals) failed: %s", (size_t)block * per_col_iv * seg, block, seg,
                    hipGetErrorString(e));
    }
    return 0;
}

static int t16_plan_dwtape(colnde_handle* h) {
    if (h->t16_dwtape >= 0) return 0;
    const DevModel& m = h->m;
    const char* ev = getenv("COLNDE_T16_DWTAPE");
    // default: on whenever the tapes fit — with the hidden pre-activations taped too, the 1,024-thread accumulator-free adjoint beats
    // the in-register kernels at every size measured (8 columns: 53 vs 64 ms per iteration; 32-128-128-31: 162 vs 198 ms)
    bool want = ev ? atoi(ev) != 0 : true;
    const int n_steps = (h->cfg.n_save - 1) * h->cfg.substeps;
    const size_t R = dwtape_row_floats(m);
    if (want && (size_t)CT * m.ns > 6 * 512) want = false;
    // LDS of the taped adjoint: with the Z tape (the default) it holds no activation array; a network that fits only that way (3 x 96-400-31: 166 KB with
    // the array, 83 KB without) then NEEDS the Z tape
    bool need_z = false;
    if (want && !h->ag_rows && (MODEL_FLOATS + lds_floats_adjoint(m)) * sizeof(float) > 160 * 1024) {
        const char* ez = getenv("COLNDE_T16_ZTAPE");
        if (!(ez && atoi(ez) == 0) && (MODEL_FLOATS + lds_floats_adjoint_noA(m)) * sizeof(float) <= 160 * 1024 && m.n_bias <= 4 * 512) need_z = true;
        else want = false;
    }
    if (h->ag_rows) {       // rows in global memory: the taped adjoint with the Z tape is the ONLY gradient path (1,024 threads: n_bias <= 4 x 1,024, CT ns <= 2 x 1,024)
        if (!want) return fail("COLNDE_T16_DWTAPE=0: this network's activation rows live in global memory, and only the taped-dW adjoint runs that way");
        if (m.n_bias > 4 * 1024 || (MODEL_FLOATS + lds_floats_adjoint_ag(m)) * sizeof(float) > 160 * 1024)
            return fail("network too large for the taped adjoint with rows in global memory (%d biases, %zu B of LDS)", m.n_bias, (MODEL_FLOATS + lds_floats_adjoint_ag(m)) * sizeof(float));
    }
    // The tapes hold ONE block of columns (a multiple of the 16-column tile; whole rounds of 4,096 columns = one workgroup per CU when
    // possible); larger problems run forward -> adjoint -> dW GEMM block after block.  COLNDE_T16_BLOCK=<columns> forces a size.
    const size_t per_col = (size_t)n_steps * m.nst * (R + t16_ztape_col_floats(m) + m.ns) * sizeof(float);
    const int n16 = h->n_tiles * CT;
    int block = 0;
    // the net-split pair's rich tape replaces the pre-activation tape on small blocks and is 4x its size per column (13,824 floats per
    // 16-column record against 216 per column): it is part of the fit estimate, not an afterthought behind the 3 GB margin
    const char* ezt0 = getenv("COLNDE_T16_ZTAPE");
    const char* er0 = getenv("COLNDE_T16_SPLIT_RICH");
    const bool rich_possible = h->adj_split && !(ezt0 && atoi(ezt0) == 0) && !(er0 && atoi(er0) == 0);
    const size_t per_col_rich = (size_t)n_steps * m.nst * (R + rt_split_rich_record_floats() / CT + m.ns) * sizeof(float);
    bool want_rich = false;
    if (want) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        const size_t margin = ((size_t)3 << 30) + (size_t)h->n_tiles * (m.n_params + 8) * sizeof(float);
        const size_t budget = free_b > margin ? free_b - margin : 0;
        const size_t fit = budget / per_col;
        if (fit >= (size_t)n16) block = n16;
        else if (fit >= CT) {
            const int nb = (int)(((size_t)n16 + fit - 1) / fit);
            block = ((n16 + nb - 1) / nb + CT - 1) / CT * CT;
            if (block >= 4096) block = (block + 4095) / 4096 * 4096;
            while ((size_t)block > fit) block -= block > 4096 ? 4096 : CT;
        }
        const char* eb = getenv("COLNDE_T16_BLOCK");
        if (eb && atoi(eb) >= CT) block = std::min(n16, (atoi(eb) / CT) * CT);
        if (block <= 0) want = false;
        // rich tape: by default on blocks of at most 2,048 columns; forced on by COLNDE_T16_SPLIT_RICH=1.  It must fit WITH the other tapes:
        // a forced rich tape shrinks the block, an automatic one is dropped.
        want_rich = want && rich_possible && ((er0 && atoi(er0) != 0) || block <= 128 * CT);
        if (want_rich && (size_t)block * per_col_rich > budget) {
            const size_t fit_rich = budget / per_col_rich / CT * CT;
            if (er0 && atoi(er0) != 0 && fit_rich >= CT) block = (int)std::min<size_t>((size_t)block, fit_rich);
            else want_rich = false;
        }
    }
    if (!want) {
        if (h->ag_rows) return fail("the delta tape of this network (%zu B per column) does not fit in HBM beside the solve", per_col);
        h->t16_dwtape = 0;
        return 0;
    }
    const int tiles_b = block / CT;
    const size_t n_rec = (size_t)tiles_b * n_steps * h->m.nst;
    const size_t need = n_rec * CT * R * sizeof(float);
    h->t16_block = block;
    h->t16_nblocks = (n16 + block - 1) / block;
    std::vector<DwMacro> mac;
    build_dw_macros(h, n_rec, mac);
    h->t16_rows = h->n_tiles + h->t16_nblocks * h->dw_slices;
    const int stride = m.n_params + 8;
    hipError_t e = hipMalloc((void**)&h->d_dwtape, need);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_macros, mac.size() * sizeof(DwMacro));
    if (e == hipSuccess) e = hipMemcpy(h->d_macros, mac.data(), mac.size() * sizeof(DwMacro), hipMemcpyHostToDevice);
    if (e == hipSuccess && !h->d_slab) e = hipMalloc((void**)&h->d_slab, (size_t)h->t16_rows * stride * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (h->d_dwtape) { (void)hipFree(h->d_dwtape); h->d_dwtape = nullptr; }
        h->t16_dwtape = 0;
        if (h->ag_rows) return fail("allocating the delta tape (%zu B) failed: %s", need, hipGetErrorString(e));
        return 0;
    }
    h->t16_dwtape = 1;
    // the block's stage tape, and (COLNDE_T16_ZTAPE=0 disables) the hidden pre-activations the forward kernel tapes for the adjoint
    if (!h->d_tape) {
        e = hipMalloc((void**)&h->d_tape, n_rec * CT * m.ns * sizeof(float));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(h->d_dwtape); h->d_dwtape = nullptr;
            h->t16_dwtape = 0;
            if (h->ag_rows) return fail("allocating the stage tape failed: %s", hipGetErrorString(e));
            return 0;
        }
    }
    const char* ezt = getenv("COLNDE_T16_ZTAPE");
    // net-split kernels on a small block (<= 2,048 columns, where it pays: 64-step iteration with the four-wave kernels 2.36 vs 2.48 ms at 1,024
    // columns, 2.69 vs 2.77 at 2,048, 3.99 vs 3.53 at 4,096): the rich tape in place of the pre-activations
    {
        if (want_rich && hipMalloc((void**)&h->d_t16_ztape, n_rec * rt_split_rich_record_floats() * sizeof(float)) == hipSuccess) {
            h->split_rich = true;
            return 0;
        }
        (void)hipGetLastError();
        h->d_t16_ztape = nullptr;
    }
    if (!(ezt && atoi(ezt) == 0) && hipMalloc((void**)&h->d_t16_ztape, n_rec * CT * t16_ztape_col_floats(m) * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        h->d_t16_ztape = nullptr;
    }
    if ((h->ag_rows || need_z) && !h->d_t16_ztape)
        return fail("this network's taped adjoint needs the pre-activation tape (COLNDE_T16_ZTAPE=0 or its allocation failed): no gradient path for it without one");
    return 0;
}

extern "C" int colnde_loss_grad_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!d_weights || !scalings || !d_out) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    if (h->m.inplace) return fail("the in-place NDE! variant is an evaluation RHS; gradients use the training RHS (inplace_variant = 0)");
    HIPCHK(hipSetDevice(h->device));
    if (h->auto_substeps) {
        if (!h->have_problem) return fail("colnde_set_problem has not been called");
        if (refuse_auto_on_a_shard(h)) return 1;
        h->auto_substeps = false;
        if (choose_substeps_impl(h, d_weights, h->cfg.reltol, nullptr, nullptr)) { h->auto_substeps = true; return 1; }
    }
    if (check_stability(h)) return 1;
    const int stride = h->m.n_params + 8;
    if (h->use_rt) {
        if (!h->have_problem) return fail("colnde_set_problem has not been called");
        if (rt_plan_tapes(h)) return 1;
        const int n_steps = (h->cfg.n_save - 1) * h->cfg.substeps;
        const int n_wt = rt_n_wtiles(h->n_col), n_dw = rt_dw1_waves(h->rt_block, n_steps);
        if (!h->d_rt_slab) {
            h->rt_rows = n_wt + h->rt_nblocks * n_dw;
            hipError_t e = hipMalloc((void**)&h->d_rt_slab, (size_t)h->rt_rows * stride * sizeof(float));
            if (e != hipSuccess) return fail("hipMalloc of the partial-gradient slab failed: %s", hipGetErrorString(e));
        }
        LossWeights lw;
        loss_weights(h, scalings, &lw);
        hipError_t e = rt_launch_pack(h->m, d_weights, h->d_wimg, h->stream);
        if (e != hipSuccess) return fail("rt pack launch failed: %s", hipGetErrorString(e));
        HIPCHK(hipMemsetAsync(h->d_rt_slab, 0, (size_t)h->rt_rows * stride * sizeof(float), h->stream));
        const size_t ns = h->m.ns;
        for (int b = 0; b < h->rt_nblocks; b++) {
            const int c0 = b * h->rt_block, nc = std::min(h->rt_block, h->n_col - c0);
            if (nc <= 0) break;
            if (rt_forward_range(h, h->d_sol, true, c0, nc)) return 1;
            {
                Timed tm(h, K_ADJOINT);
                e = rt_launch_adjoint(h->m, h->d_wimg, h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times, h->cfg.n_save, h->cfg.substeps,
                                      h->d_sol + (size_t)c0 * h->cfg.n_save * ns, h->d_truth + (size_t)c0 * h->cfg.n_save * ns, h->d_rt_tape,
                                      h->d_rt_tape2, h->rt_ztape ? h->d_rt_tapez : nullptr, lw,
                                      h->d_rt_slab + (size_t)(c0 / 32) * stride, nc, h->sp_adj, h->stream);
                if (e != hipSuccess) return fail("rt adjoint launch failed: %s", hipGetErrorString(e));
            }
            {
                Timed tm(h, K_DW1);
                e = rt_launch_dw1(h->m, h->d_rt_tape, h->d_rt_tape2, nc, n_steps, h->d_rt_slab + ((size_t)n_wt + (size_t)b * n_dw) * stride,
                                  h->sp_dw, h->stream);
                if (e != hipSuccess) return fail("rt dW1 launch failed: %s", hipGetErrorString(e));
            }
        }
        {
            Timed tm(h, K_REDUCE);
            e = launch_reduce(h->d_rt_slab, h->rt_rows, h->m.n_params, stride, lw, d_out, h->stream);
            if (e != hipSuccess) return fail("reduce launch failed: %s", hipGetErrorString(e));
        }
        return 0;
    }
    if (h->use_fc) {
        if (!h->have_problem) return fail("colnde_set_problem has not been called");
        if (fc_plan_tapes(h)) return 1;
        LossWeights lw;
        loss_weights(h, scalings, &lw);
        const size_t ns = h->m.ns;
        const float* d_we = nullptr;
        if (fc_engine_weights(h, d_weights, &d_we)) return 1;
        const FcConv cv = fc_conv_args(h);                                  // (after the plan: the conv tape exists)
        hipError_t e = fc_launch_pack(h->m, h->fc_cw, d_we, h->d_fc_imgf, h->d_fc_imgb, h->d_fc_bias, h->d_fc_simgf, h->d_fc_simgb, h->stream);
        if (e != hipSuccess) return fail("fc32 pack launch failed: %s", hipGetErrorString(e));
        HIPCHK(hipMemsetAsync(h->d_slab, 0, (size_t)h->fc_rows * stride * sizeof(float), h->stream));
        if (h->conv.c) HIPCHK(hipMemsetAsync(h->conv.d_cslab, 0, (size_t)h->conv.cslab_rows * FC_CONV_GRAD_SLOTS * sizeof(float), h->stream));
        const int cw = h->fc_cw;
        const int n_wg = (h->n_col + cw - 1) / cw, n_iv = h->cfg.n_save - 1, nseg = h->fc_nseg;
        const size_t gemm_rows0 = (size_t)n_wg * nseg;                      // slab: [tile][segment] adjoint rows, then [block][segment][slice] GEMM rows
        for (int b = 0; b < h->fc_nblocks; b++) {
            const int c0 = b * h->fc_block, nc = std::min(h->fc_block, h->n_col - c0);
            if (nc <= 0) break;
            const size_t tiles_b = ((size_t)nc + cw - 1) / cw;
            // time segments: the states at the save points first (tape-less), then segment by segment from the end of the axis
            // (that first pass tapes the LAST segment on its way, which is the first one the backward sweep needs)
            if (nseg > 1 && fc_forward_range(h, h->d_sol, true, c0, nc, 0, n_iv, (nseg - 1) * h->fc_seg)) return 1;
            for (int sg = nseg - 1; sg >= 0; sg--) {
                const int iv0 = sg * h->fc_seg, iv1 = std::min(n_iv, iv0 + h->fc_seg);
                if (!(nseg > 1 && sg == nseg - 1) && fc_forward_range(h, h->d_sol, true, c0, nc, iv0, iv1)) return 1;
                {
                    Timed tm(h, K_ADJOINT);
                    e = fc_launch_adjoint(h->m, h->fc_cw, h->d_fc_imgb, (h->sp_adj && fc_split_supported(h->fc_cw)) ? h->d_fc_simgb : nullptr, h->d_times, h->cfg.n_save, iv0, iv1, h->cfg.substeps, h->d_sol + (size_t)c0 * h->cfg.n_save * ns,
                                          h->d_truth + (size_t)c0 * h->cfg.n_save * ns, h->d_dwtape, h->d_fc_masks, h->d_fc_switch, lw.w[2],
                                          nseg > 1 ? h->d_fc_lam + (size_t)c0 * h->m.Nz : nullptr,
                                          h->d_slab + ((size_t)sg * n_wg + (size_t)(c0 / cw)) * stride, nc, h->stream, nullptr, h->conv.c ? &cv : nullptr);
                    if (e != hipSuccess) return fail("fc32 adjoint launch failed: %s", hipGetErrorString(e));
                }
                {
                    Timed tm(h, K_DW1);
                    if (h->sp_dw && !h->dw_split.passes.empty())
                        e = launch_dw_gemm_split(h->d_dwtape, tiles_b * (cw / 16) * (size_t)(iv1 - iv0) * h->cfg.substeps * h->m.nst, (int)dwtape_row_floats(h->m), h->dw_split,
                                                 h->dw_slices, h->d_slab + (gemm_rows0 + ((size_t)b * nseg + sg) * h->dw_slices) * stride, stride, h->stream);
                    else
                    e = launch_dw_gemm(h->d_dwtape, tiles_b * (cw / 16) * (size_t)(iv1 - iv0) * h->cfg.substeps * h->m.nst, (int)dwtape_row_floats(h->m), h->d_macros,
                                       h->n_macros, h->dw_slices, h->d_slab + (gemm_rows0 + ((size_t)b * nseg + sg) * h->dw_slices) * stride, stride, h->stream);
                    if (e != hipSuccess) return fail("dW GEMM launch failed: %s", hipGetErrorString(e));
                    if (h->conv.c) {                                        // the filter's c + 1 entries, from the conv tape of the same records
                        e = launch_fc_conv_grad(h->conv.d_ctape, (long)(tiles_b * (size_t)(iv1 - iv0) * h->cfg.substeps * h->m.nst) * 16, h->m.Nz, h->conv.c,
                                                h->conv.d_cslab + ((size_t)b * nseg + sg) * FC_CONV_GRAD_MAX_SLICES * FC_CONV_GRAD_SLOTS, h->stream);
                        if (e != hipSuccess) return fail("conv filter gradient launch failed: %s", hipGetErrorString(e));
                    }
                }
            }
        }
        {
            Timed tm(h, K_REDUCE);
            e = launch_reduce(h->d_slab, h->fc_rows, h->m.n_params, stride, lw, h->conv.c ? h->conv.d_gpad : d_out, h->stream);
            if (e != hipSuccess) return fail("reduce launch failed: %s", hipGetErrorString(e));
            if (h->conv.c) {                                                // the user's layout: filter entries in front, W1's padded columns dropped
                e = launch_fc_conv_fold(h->conv.d_gpad, h->conv.d_cslab, h->conv.cslab_rows, h->conv.c, h->conv.w1_end, h->conv.n_zero, h->conv.n_params + 8, d_out,
                                        h->stream);
                if (e != hipSuccess) return fail("conv gradient fold launch failed: %s", hipGetErrorString(e));
            }
        }
        return 0;
    }
    if (t16_plan_dwtape(h)) return 1;
    if (h->t16_dwtape == 1) {
        if (!h->have_problem) return fail("colnde_set_problem has not been called");
        LossWeights lw;
        loss_weights(h, scalings, &lw);
        const int n_steps = (h->cfg.n_save - 1) * h->cfg.substeps;
        const size_t ns = h->m.ns;
        if (pack(h, d_weights)) return 1;
        HIPCHK(hipMemsetAsync(h->d_slab, 0, (size_t)h->t16_rows * stride * sizeof(float), h->stream));
        for (int b = 0; b < h->t16_nblocks; b++) {
            const int c0 = b * h->t16_block, nc = std::min(h->t16_block, h->n_col - c0);
            if (nc <= 0) break;
            const int tiles_b = (nc + CT - 1) / CT;
            if (t16_forward_range(h, d_weights, h->d_sol, true, c0, nc)) return 1;
            {
                Timed tm(h, K_ADJOINT);
                AdjointGeom g = {512, 1, 3, 0};
                hipError_t e;
                if (h->adj_split && h->d_t16_ztape)
                    // the companion of the split forward: one wavefront per flux net (+ a helper) per tile, writing tile16's delta tape
                    e = rt_launch_adjoint_split(h->m, h->d_wimg, h->d_times, h->cfg.n_save, h->cfg.substeps,
                                                h->d_sol + (size_t)c0 * h->cfg.n_save * ns, h->d_truth + (size_t)c0 * h->cfg.n_save * ns, h->d_tape,
                                                h->d_t16_ztape, lw, h->d_slab + (size_t)(c0 / CT) * stride, nc, h->d_dwtape, h->split_rich, h->adj_helper, h->sp_adj, h->stream);
                else
                e = launch_adjoint(h->m, h->pk, d_weights, h->d_wf, h->d_wb, h->d_tiles, h->d_bias_zoff, h->d_bias_goff,
                                              h->d_bcs + (size_t)c0 * h->m.n_bc, h->d_times, h->cfg.n_save, h->cfg.substeps,
                                              h->d_sol + (size_t)c0 * h->cfg.n_save * ns, h->d_truth + (size_t)c0 * h->cfg.n_save * ns, h->d_tape,
                                              lw, h->d_slab + (size_t)(c0 / CT) * stride, nc, g,
                                              (MODEL_FLOATS + (h->ag_rows ? lds_floats_adjoint_ag(h->m) : (h->d_t16_ztape ? lds_floats_adjoint_noA(h->m) : lds_floats_adjoint(h->m)))) * sizeof(float),
                                              h->stream, h->d_dwtape, h->d_t16_ztape);
                if (e != hipSuccess) return fail("adjoint (taped dW) launch failed: %s", hipGetErrorString(e));
            }
            {
                Timed tm(h, K_DW1);
                hipError_t e = (h->sp_dw && !h->dw_split.passes.empty())
                    ? launch_dw_gemm_split(h->d_dwtape, (size_t)tiles_b * n_steps * h->m.nst, (int)dwtape_row_floats(h->m), h->dw_split,
                                           h->dw_slices, h->d_slab + ((size_t)h->n_tiles + (size_t)b * h->dw_slices) * stride, stride, h->stream)
                    : launch_dw_gemm(h->d_dwtape, (size_t)tiles_b * n_steps * h->m.nst, (int)dwtape_row_floats(h->m), h->d_macros, h->n_macros,
                                              h->dw_slices, h->d_slab + ((size_t)h->n_tiles + (size_t)b * h->dw_slices) * stride, stride, h->stream);
                if (e != hipSuccess) return fail("dW GEMM launch failed: %s", hipGetErrorString(e));
            }
        }
        {
            Timed tm(h, K_REDUCE);
            hipError_t e = launch_reduce(h->d_slab, h->t16_rows, h->m.n_params, stride, lw, d_out, h->stream);
            if (e != hipSuccess) return fail("reduce launch failed: %s", hipGetErrorString(e));
        }
        return 0;
    }
    if (forward_impl(h, d_weights, h->d_sol, true)) return 1;
    if (!h->geo_ok)
        return fail("network too large for the tile engine's in-register adjoint (%d weight-gradient tiles, %zu B of LDS) and its "
                    "delta tape does not fit in HBM (or COLNDE_T16_DWTAPE=0)", h->m.n_tiles, h->lds_adj);
    if (!h->d_slab) {
        hipError_t e = hipMalloc((void**)&h->d_slab, (size_t)h->n_tiles * stride * sizeof(float));
        if (e != hipSuccess) return fail("hipMalloc of the partial-gradient slab failed: %s", hipGetErrorString(e));
    }
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    {
        Timed tm(h, K_ADJOINT);
        hipError_t e = launch_adjoint(h->m, h->pk, d_weights, h->d_wf, h->d_wb, h->d_tiles, h->d_bias_zoff, h->d_bias_goff,
                                      h->d_bcs, h->d_times, h->cfg.n_save, h->cfg.substeps, h->d_sol, h->d_truth, h->d_tape,
                                      lw, h->d_slab, h->n_col, h->geo, h->lds_adj, h->stream);
        if (e != hipSuccess) return fail("adjoint launch failed: %s", hipGetErrorString(e));
    }
    {
        Timed tm(h, K_REDUCE);
        hipError_t e = launch_reduce(h->d_slab, h->n_tiles, h->m.n_params, stride, lw, d_out, h->stream);
        if (e != hipSuccess) return fail("reduce launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

extern "C" int colnde_loss_grad(colnde_handle* h, const float* weights, const float scalings[6], float terms[6],
                                float* total, float* grad) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!weights || !scalings || !terms || !total || !grad) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    const int np = user_params(h);
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * np, hipMemcpyHostToDevice, h->stream));
    if (colnde_loss_grad_dev(h, h->d_w, scalings, h->d_out)) return 1;
    float o[8];
    HIPCHK(hipMemcpyAsync(grad, h->d_out, sizeof(float) * np, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(o, h->d_out + np, sizeof(o), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int q = 0; q < 6; q++) terms[q] = o[q];
    *total = o[6];
    if (!std::isfinite(o[6])) return fail("the loss is not finite (%g): the solve left the stable regime (time step, weights or inputs)", o[6]);
    return 0;
}

// ---- ensembles: K models of one architecture side by side (colnde_create_ensemble) ---------------------------------------------------------------
// The reference's sweep (wind_mixing/train_NDE_args.jl: activation, ADAM rate and Pacanowski-Philander constants per process) trains many small
// models of ONE architecture on the same simulations.  Here every kernel of a training iteration runs once for all K models with the model index in
// blockIdx.y: the net-split pair (rt16sh_*), the weight packers, tile16's dW GEMM, the loss and gradient reductions and the ADAM step.  A model owns
// its packed weights, solution, tapes and slab rows (RtEns strides) and its closure constants (RtPhys); x0, bcs and truth are shared.

// the configuration of model k: cfg with row k of physics ([K][5]: nu0, nu_minus, dRi, Ric, Pr)
colnde_config model_config(const colnde_config* cfg, const float* physics, int k) {
    colnde_config c = *cfg;
    if (physics) {
        const float* r = physics + (size_t)5 * k;
        c.nu0 = r[0]; c.nu_minus = r[1]; c.dRi = r[2]; c.Ric = r[3]; c.Pr = r[4];
    }
    return c;
}

// The shared sub-step count against every model's stability bound; RKC2 with automatic stages: the largest stage count any model needs.
// *min_sub / *stages: the ensemble's bound and stage count (stages = 0 for RK4).
static int ens_stability(const colnde_config* cfg, int K, const float* physics, int* min_sub, int* stages) {
    *min_sub = 1;
    *stages = 0;
    for (int k = 0; k < K; k++) {
        const colnde_config c = model_config(cfg, physics, k);
        if (physics) {
            const float* r = physics + (size_t)5 * k;
            for (int q = 0; q < 5; q++)
                if (!std::isfinite(r[q])) return fail("physics[%d][%d] = %g is not finite", k, q, r[q]);
            if (!(c.dRi > 0.0f) || !(c.Pr > 0.0f)) return fail("physics[%d]: dRi = %g and Pr = %g must be > 0", k, c.dRi, c.Pr);
        }
        const int ms = colnde_min_substeps(&c);
        if (ms < 0) return 1;
        *min_sub = std::max(*min_sub, ms);
        if (cfg->stepper == COLNDE_STEPPER_RKC2 && !cfg->rkc_stages) *stages = std::max(*stages, colnde_rkc_stages(&c));
        const char* e = getenv("COLNDE_ALLOW_UNSTABLE_DT");
        if (cfg->substeps < ms && !(e && atoi(e) != 0))
            return fail("model %d (nu0 = %g, nu_minus = %g, Pr = %g) needs substeps >= %d for a stable step (colnde_min_substeps; lambda = -%.4g), but the "
                        "ensemble shares substeps = %d (COLNDE_ALLOW_UNSTABLE_DT=1 overrides)", k, c.nu0, c.nu_minus, c.Pr, ms, stiff_lambda(&c), cfg->substeps);
    }
    return 0;
}

static int ens_upload_physics(colnde_handle* h, const float* physics) {
    std::vector<RtPhys> ph((size_t)h->n_models);
    for (int k = 0; k < h->n_models; k++) {
        const colnde_config c = model_config(&h->cfg, physics, k);
        ph[k] = closure_constants(c.nu0, c.nu_minus, c.dRi, c.Ric, c.Pr);
    }
    // (kernels in flight on the stream may still read the previous table: the copy is ordered on the stream and completed before returning)
    HIPCHK(hipMemcpyAsync(h->d_phys, ph.data(), ph.size() * sizeof(RtPhys), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->phys_host.swap(ph);
    if (physics) h->phys_raw.assign(physics, physics + (size_t)5 * h->n_models);
    else h->phys_raw.clear();
    return 0;
}

// The tapes of all K models, planned once at creation: tile16's taped-dW formats for ONE block of all columns per model (the net-split pair has no
// column-block loop across models), the rich tape while the K models' 16-column tiles number at most 128 (2,048 columns in flight: the single
// handle's crossover, which counts concurrent tiles whoever owns them).  Refused with the bytes it needs when it does not fit.
static int ens_plan_tapes(colnde_handle* h) {
    const DevModel& m = h->m;
    const int K = h->n_models;
    const int n_steps = (h->cfg.n_save - 1) * h->cfg.substeps;
    const size_t n_rec = (size_t)h->n_tiles * n_steps * m.nst;
    const size_t R = dwtape_row_floats(m), P8 = (size_t)m.n_params + 8;
    std::vector<DwMacro> mac;
    build_dw_macros(h, n_rec, mac);                          // the slice count a single handle of this size plans: same reduction order
    h->t16_rows = h->n_tiles + h->dw_slices;
    const size_t f_tape = n_rec * CT * m.ns, f_dw = n_rec * CT * R, f_rich = n_rec * rt_split_rich_record_floats(),
                 f_plain = n_rec * CT * t16_ztape_col_floats(m), f_slab = (size_t)h->t16_rows * P8,
                 f_sol = (size_t)h->n_col * h->cfg.n_save * m.ns, f_img = RT_IMG_STRIDE;
    const char* er = getenv("COLNDE_T16_SPLIT_RICH");
    const bool forced = er && *er;
    bool rich = forced ? atoi(er) != 0 : (size_t)K * h->n_tiles <= 128;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t margin = ((size_t)3 << 30) + (size_t)K * (P8 * 2 + 256 * 8) * sizeof(float);
    const size_t budget = free_b > margin ? free_b - margin : 0;
    auto per_model = [&](bool r) { return (f_tape + f_dw + (r ? f_rich : f_plain) + f_slab + f_sol + f_img) * sizeof(float); };
    if (rich && !forced && (size_t)K * per_model(true) > budget) rich = false;       // the automatic rich tape gives way to the plain one, as for one handle
    const size_t need = per_model(rich);
    if ((size_t)K * need > budget)
        return fail("an ensemble of %d models needs %zu bytes of device memory for its tapes, slab rows and solutions (%zu per model, %s tape, "
                    "%d substeps x %d stages x %d save intervals); %zu bytes are free (3 GB kept in reserve): use fewer models per handle",
                    K, (size_t)K * need, need, rich ? "rich" : "plain", h->cfg.substeps, m.nst, h->cfg.n_save - 1, free_b);
    const size_t f_z = rich ? f_rich : f_plain;
    hipError_t e = hipMalloc((void**)&h->d_dwtape, (size_t)K * f_dw * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_tape, (size_t)K * f_tape * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_t16_ztape, (size_t)K * f_z * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_slab, (size_t)K * f_slab * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_macros, mac.size() * sizeof(DwMacro));
    if (e == hipSuccess) e = hipMemcpy(h->d_macros, mac.data(), mac.size() * sizeof(DwMacro), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail("allocating the ensemble's tapes (%zu bytes, %zu per model) failed: %s", (size_t)K * need, need, hipGetErrorString(e));
    }
    h->t16_dwtape = 1;
    h->t16_block = h->n_tiles * CT;
    h->t16_nblocks = 1;
    h->split_rich = rich;
    h->ens.wimg = f_img;
    h->ens.sol = f_sol;
    h->ens.tape = f_tape;
    h->ens.ztape = f_z;
    h->ens.dwtape = f_dw;
    h->ens.slab = f_slab;
    h->ens.n_models = K;
    h->ens.phys = h->d_phys;
    h->ens_model_bytes = need;
    return 0;
}

extern "C" int colnde_create_ensemble(const colnde_config* cfg, int n_models, const float* physics, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (validate(cfg)) return 1;
    if (n_models < 1 || n_models > 65535) return fail("n_models = %d outside 1..65535", n_models);
    // only the configurations on which AUTO runs the four-wave net-split pair: those kernels carry the model index
    if (cfg->model != COLNDE_MODEL_WIND_MIXING)
        return fail("ensembles cover the wind-mixing NDE on the net-split kernels: the free-convection models (fc32 / tile16) run one handle per model");
    if (cfg->inplace_variant) return fail("ensembles train on the training RHS: inplace_variant (the NDE! evaluation RHS) is not supported");
    if (cfg->engine != COLNDE_ENGINE_AUTO)
        return fail("ensembles run the net-split kernels engine AUTO selects: engine forced to %d is not supported (those engines have no model index)", cfg->engine);
    if (cfg->substeps == 0)
        return fail("substeps = 0 (chosen from reltol by the first solve) is not supported: the models share one sub-step count, and the tapes are sized at "
                    "creation — choose it with a single handle (colnde_choose_substeps) and pass it");
    if (cfg->n_columns > 8192)
        return fail("%d columns per model: ensembles cover the net-split range (at most 8,192 columns per model); above it regtile runs one handle per model",
                    cfg->n_columns);
    {
        DevModel dm;
        PackInfo pk;
        build_model(cfg, &dm, &pk);
        if (!rt_supported(dm))
            return fail("ensembles cover the net-split shape only (Nz = 32, three 96-50-20-31 nets, one hidden activation, training RHS, no smoothing): "
                        "wide networks and other architectures run one handle per model");
    }
    if (physics && !cfg->modified_pacanowski_philander)
        return fail("a physics array needs modified_pacanowski_philander = 1: without the Richardson-number closure the five constants are unused (pass NULL)");
    // the environment switches that send a single handle down paths without a model index
    static const char* const no_index[] = {"COLNDE_T16_FWD_HELPER", "COLNDE_T16_ADJ_HELPER", "COLNDE_T16_FWD_SPLIT", "COLNDE_T16_ADJ_SPLIT", "COLNDE_T16_ZTAPE",
                                           "COLNDE_T16_DWTAPE"};
    for (const char* name : no_index) {
        const char* e = getenv(name);
        if (e && *e && atoi(e) == 0)
            return fail("%s=0 selects kernels without a model index (the three-wave or tile16 kernels, or no delta / pre-activation tape): ensembles refuse it", name);
    }
    if (getenv("COLNDE_T16_BLOCK")) return fail("COLNDE_T16_BLOCK: ensembles hold one block of columns per model (the column-block loop has no model index)");
    int min_sub = 1, stages = 0;
    if (ens_stability(cfg, n_models, physics, &min_sub, &stages)) return 1;
    colnde_handle* h = nullptr;
    if (colnde_create(cfg, &h)) return 1;
    if (h->use_rt || h->use_fc || h->ag_rows || !h->fwd_split || !h->adj_split || !h->fwd_helper || !h->adj_helper) {
        colnde_destroy(h);
        return fail("this configuration does not run the four-wave net-split pair under engine AUTO: ensembles refuse it");
    }
    h->ensemble = true;
    h->n_models = n_models;
    h->min_substeps = min_sub;
    if (stages > 0 && stages != h->m.nst) {
        h->ens_rkc_stages = stages;
        if (refresh_rkc(h)) { colnde_destroy(h); return 1; }
    } else if (stages > 0) {
        h->ens_rkc_stages = stages;
    }
    const size_t K = (size_t)n_models, P = (size_t)h->m.n_params;
    auto realloc_ = [&](float** p, size_t n) {
        if (*p) { (void)hipFree(*p); *p = nullptr; }
        if (hipMalloc((void**)p, n * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return false; }
        return true;
    };
    if (!realloc_(&h->d_w, K * P) || !realloc_(&h->d_out, K * (P + 8)) || !realloc_(&h->d_partial, K * 256 * 8) ||
        !realloc_(&h->d_sol, K * h->n_col * h->cfg.n_save * h->m.ns) || !realloc_(&h->d_wimg, K * RT_IMG_STRIDE) ||
        hipMalloc((void**)&h->d_phys, K * sizeof(RtPhys)) != hipSuccess) {
        (void)hipGetLastError();
        colnde_destroy(h);
        return fail("allocating the ensemble's per-model buffers (%d models) failed", n_models);
    }
    if (ens_upload_physics(h, physics) || ens_plan_tapes(h)) { colnde_destroy(h); return 1; }
    *out = h;
    return 0;
}

extern "C" int colnde_n_models(const colnde_handle* h) { return h ? h->n_models : -1; }

static int ensemble_only(const colnde_handle* h);

// ---- free-convection ensembles (colnde_create_fc_ensemble) ------------------------------------------------------------------------------------------
// The reference trains the free-convection NDE on 3 to 9 simulations (train_free_convection_nde.jl, --training-simulations): one 16-column workgroup.  Its
// sweep (one process per seed / optimiser rate / penalty setting) and the judging of a run (compute_nde_solution_history, testing.jl:1-32: the network of
// EVERY epoch re-solved on every simulation) are both "many networks, same few columns".  Here the 16-column fc32 kernels carry the model index in
// blockIdx.y (FcEns: the strides of what a model owns), tile16's dW GEMM, the reductions and the ADAM step already do; row k of every result is, bit for
// bit, what a colnde_create handle computes for model k's weights (under the same COLNDE_FC_SEG: the segment count orders the gradient's sums).

// Decided from the configuration and the environment alone, before any device work
static int fc_ens_refusals(const colnde_config* cfg, int n_models) {
    if (n_models < 1 || n_models > 65535) return fail("n_models = %d outside 1..65535", n_models);
    if (cfg->model == COLNDE_MODEL_WIND_MIXING)
        return fail("colnde_create_fc_ensemble covers the free-convection models (FreeConvectionNDE, ConvectiveAdjustmentNDE): a wind-mixing ensemble is colnde_create_ensemble's");
    if (cfg->engine != COLNDE_ENGINE_AUTO && cfg->engine != COLNDE_ENGINE_FC32)
        return fail("free-convection ensembles run the fc32 kernels (engine AUTO or FC32): engine forced to %d has no model index", cfg->engine);
    {
        DevModel dm;
        PackInfo pk;
        build_model(cfg, &dm, &pk);
        if (!fc_supported(dm, cfg->stepper))
            return fail("free-convection ensembles cover the fc32 shape only: FreeConvectionNDE (RK4) or ConvectiveAdjustmentNDE (RK4, RKC2) with Dense(Nz,4Nz,relu), "
                        "Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1), Nz = 32 or 64 (Nz = %d, %d layers here); other networks run one handle per model", cfg->Nz, cfg->n_layers);
    }
    if (cfg->substeps == 0)
        return fail("substeps = 0 (chosen from reltol by the first solve) is not supported: the models share one sub-step count, and the tapes are sized at "
                    "creation — choose it with a single handle (colnde_choose_substeps) and pass it");
    {
        const int ms = colnde_min_substeps(cfg);
        const char* e = getenv("COLNDE_ALLOW_UNSTABLE_DT");
        if (ms < 0) return 1;
        if (cfg->substeps < ms && !(e && atoi(e) != 0))
            return fail("substeps = %d is below colnde_min_substeps = %d: the step leaves the stepper's stability region (lambda = -%.4g; COLNDE_ALLOW_UNSTABLE_DT=1 overrides)",
                        cfg->substeps, ms, stiff_lambda(cfg));
    }
    if (cfg->n_columns > 4096)
        return fail("%d columns per model: free-convection ensembles cover the 16-column tiles (at most 4,096 columns per model, fc_tile_width); above it the 32-column "
                    "kernels run one handle per model", cfg->n_columns);
    // the switches that send a single handle to kernels without a model index
    {
        const char* e = getenv("COLNDE_FC");
        if (e && *e && atoi(e) == 0) return fail("COLNDE_FC=0 sends free convection to the tile16 engine, which has no model index here: free-convection ensembles refuse it");
        e = getenv("COLNDE_FC_CW");
        if (e && atoi(e) == 32) return fail("COLNDE_FC_CW=32 selects the 32-column kernels, which have no model index: free-convection ensembles refuse it");
        if (getenv("COLNDE_FC_BLOCK")) return fail("COLNDE_FC_BLOCK: free-convection ensembles hold one block of columns per model (the column-block loop has no model index)");
    }
    return 0;
}

// ---- the --conv network (train_free_convection_nde.jl:110-122): a handle of its own on the 16-column fc32 kernels -------------------------------------
// Decided from the configuration and the environment alone, before any device work
static int conv_refusals(const colnde_config* cfg, int c) {
    if (c < 2 || c > FC_CONV_MAX)
        return fail("conv_filter = %d outside 2..%d (the reference builds the plain three-Dense chain for --conv <= 1: colnde_create; the taps are an unrolled loop of %d)", c,
                    FC_CONV_MAX, FC_CONV_MAX);
    if (cfg->model == COLNDE_MODEL_WIND_MIXING)
        return fail("colnde_create_conv covers the free-convection models (FreeConvectionNDE, ConvectiveAdjustmentNDE): the wind-mixing driver has no --conv network");
    {
        DevModel dm;
        PackInfo pk;
        build_model(cfg, &dm, &pk);
        if (!fc_supported(dm, COLNDE_STEPPER_RK4))
            return fail("colnde_create_conv takes the plain fc32 configuration, layer_sizes = (Nz, 4Nz, 4Nz, Nz-1) with relu, relu, identity and Nz = 32 or 64 (Nz = %d, %d "
                        "layers here): conv_filter says that the first Dense takes Nz - c + 1 inputs behind the filter", cfg->Nz, cfg->n_layers);
    }
    if (cfg->engine != COLNDE_ENGINE_AUTO && cfg->engine != COLNDE_ENGINE_FC32)
        return fail("the conv network runs the fc32 kernels (engine AUTO or FC32): engine forced to %d has no filter", cfg->engine);
    if (cfg->model == COLNDE_MODEL_FREE_CONVECTION && cfg->stepper == COLNDE_STEPPER_RKC2)
        return fail("FreeConvectionNDE under RKC2: fc32 has no such kernel (RKC2 covers ConvectiveAdjustmentNDE; FreeConvectionNDE runs RK4)");
    if (cfg->substeps == 0)
        return fail("substeps = 0 (chosen from reltol by the first solve) is not supported on a conv handle: the error estimate does not cover the filter — choose the count "
                    "and pass it");
    {
        const int ms = colnde_min_substeps(cfg);
        const char* e = getenv("COLNDE_ALLOW_UNSTABLE_DT");
        if (ms < 0) return 1;
        if (cfg->substeps < ms && !(e && atoi(e) != 0))
            return fail("substeps = %d is below colnde_min_substeps = %d: the step leaves the stepper's stability region (lambda = -%.4g; COLNDE_ALLOW_UNSTABLE_DT=1 overrides)",
                        cfg->substeps, ms, stiff_lambda(cfg));
    }
    if (cfg->n_columns > 4096)
        return fail("%d columns: the conv network covers the 16-column tiles (at most 4,096 columns, fc_tile_width); the 32-column kernels have no filter", cfg->n_columns);
    {
        const char* e = getenv("COLNDE_FC");
        if (e && *e && atoi(e) == 0) return fail("COLNDE_FC=0 sends free convection to the tile16 engine, which has no filter: conv handles refuse it");
        e = getenv("COLNDE_FC_CW");
        if (e && atoi(e) == 32) return fail("COLNDE_FC_CW=32 selects the 32-column kernels, which have no filter: conv handles refuse it");
        if (getenv("COLNDE_FC_BLOCK")) return fail("COLNDE_FC_BLOCK: conv handles hold one block of columns (at most 4,096)");
    }
    return 0;
}

extern "C" int colnde_create_conv(const colnde_config* cfg, int conv_filter, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (validate(cfg)) return 1;
    if (conv_refusals(cfg, conv_filter)) return 1;
    colnde_handle* h = nullptr;
    if (colnde_create(cfg, &h)) return 1;
    if (!h->use_fc || h->fc_cw != 16) {
        colnde_destroy(h);
        return fail("colnde_create_conv: the configuration did not select the 16-column fc32 kernels");
    }
    const DevModel& m = h->m;
    const int H = 4 * m.Nz, M = m.Nz - conv_filter + 1;
    h->conv.w1_end = m.w_off[0] + H * M;
    h->conv.n_zero = H * (conv_filter - 1);
    h->conv.n_params = conv_filter + 1 + m.n_params - h->conv.n_zero;
    hipError_t e = m.w_off[0] == 0 ? hipMalloc((void**)&h->conv.d_wpad, (size_t)m.n_params * sizeof(float)) : hipErrorInvalidValue;
    if (e == hipSuccess) e = hipMalloc((void**)&h->conv.d_gpad, ((size_t)m.n_params + 8) * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        colnde_destroy(h);
        return fail("colnde_create_conv: allocating the padded weight and gradient vectors failed: %s", hipGetErrorString(e));
    }
    h->conv.c = conv_filter;
    *out = h;
    return 0;
}

// The tapes of all K models, planned once at creation by fc_plan_tapes' rules on a per-model budget of (free memory - margin) / K: one block of all columns
// (column blocks do not occur at <= 4,096 columns), the whole time axis when it fits and time segments otherwise (COLNDE_FC_SEG=<intervals> forces), the
// slice count a single handle of this size plans.  Refused with the bytes it needs when not even one save interval per segment fits.
static int fc_ens_plan_tapes(colnde_handle* h) {
    const DevModel& m = h->m;
    const size_t K = (size_t)h->n_models;
    const int n_iv = h->cfg.n_save - 1, cw = h->fc_cw;
    const size_t R = dwtape_row_floats(m), P8 = (size_t)m.n_params + 8;
    if (R != fc_record_row_floats(m.Nz)) return fail("fc32: record layout mismatch (%zu vs %zu floats per column)", R, fc_record_row_floats(m.Nz));
    const bool ca = m.model == COLNDE_MODEL_CONV_ADJ_NDE;
    const size_t per_col_iv = (size_t)h->cfg.substeps * m.nst * (R * sizeof(float) + fc_mask_words() * sizeof(unsigned int) / cw + (ca ? sizeof(unsigned long long) : 0));
    const int n32 = (h->n_col + 31) / 32 * 32;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t margin = (size_t)3 << 30;
    const size_t budget = (free_b > margin ? free_b - margin : 0) / K;
    // what a model owns beside the tapes: λ between segments and the slab rows ([tile][segment] + [segment][<= 512 slices] rows of n_params + 8 floats)
    auto rest_bytes = [&](int sg) {
        const size_t nsg = ((size_t)n_iv + sg - 1) / sg;
        return ((size_t)(n32 / cw) + 512) * nsg * P8 * sizeof(float) + (size_t)n32 * m.Nz * sizeof(float);
    };
    int seg = n_iv;
    while (seg > 1 && per_col_iv * (size_t)n32 * seg + rest_bytes(seg) > budget) seg--;
    const char* es = getenv("COLNDE_FC_SEG");
    if (es && atoi(es) >= 1) seg = std::min(n_iv, atoi(es));
    const size_t need = per_col_iv * (size_t)n32 * seg + rest_bytes(seg);
    if (need > budget)
        return fail("a free-convection ensemble of %d models needs %zu bytes of device memory for its tapes and slab rows (%zu per model with %d save interval(s) per "
                    "time segment, %d substeps x %d stages); %zu bytes are free (3 GB kept in reserve): use fewer models per handle",
                    h->n_models, K * need, need, seg, h->cfg.substeps, m.nst, free_b);
    h->fc_block = n32;
    h->fc_nblocks = 1;
    h->fc_seg = seg;
    h->fc_nseg = (n_iv + seg - 1) / seg;
    const size_t tiles_b = (size_t)n32 / cw;
    const size_t stage_recs = (size_t)seg * h->cfg.substeps * m.nst;
    const size_t n_rec = tiles_b * (cw / 16) * stage_recs;
    std::vector<DwMacro> mac;
    build_dw_macros(h, n_rec, mac);                          // the slice count a single handle of this size plans: same reduction order
    h->fc_rows = (n32 / cw) * h->fc_nseg + h->fc_nblocks * h->fc_nseg * h->dw_slices;
    FcEns& en = h->fens;
    en.dwtape = n_rec * CT * R;
    en.masks = tiles_b * stage_recs * fc_mask_words();
    en.swtape = ca ? tiles_b * stage_recs * fc_switch_words(cw) : 0;
    en.lam = (size_t)n32 * m.Nz;
    en.slab = (size_t)h->fc_rows * P8;
    hipError_t e = hipMalloc((void**)&h->d_dwtape, K * en.dwtape * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_fc_masks, K * en.masks * sizeof(unsigned int));
    if (e == hipSuccess && ca) e = hipMalloc((void**)&h->d_fc_switch, K * en.swtape * sizeof(unsigned long long));
    if (e == hipSuccess && h->fc_nseg > 1) e = hipMalloc((void**)&h->d_fc_lam, K * en.lam * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_macros, mac.size() * sizeof(DwMacro));
    if (e == hipSuccess) e = hipMemcpy(h->d_macros, mac.data(), mac.size() * sizeof(DwMacro), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_slab, K * en.slab * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail("allocating the free-convection ensemble's tapes (%zu bytes, %zu per model) failed: %s", K * need, need, hipGetErrorString(e));
    }
    h->ens.slab = en.slab;
    h->ens_model_bytes = (en.dwtape + en.slab + (h->fc_nseg > 1 ? en.lam : 0)) * sizeof(float) + en.masks * sizeof(unsigned int) + en.swtape * sizeof(unsigned long long);
    return 0;
}

extern "C" int colnde_create_fc_ensemble(const colnde_config* cfg, int n_models, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (validate(cfg)) return 1;
    if (fc_ens_refusals(cfg, n_models)) return 1;
    colnde_handle* h = nullptr;
    if (colnde_create(cfg, &h)) return 1;
    if (!h->use_fc || h->fc_cw != 16 || !fc_split_supported(16)) {
        colnde_destroy(h);
        return fail("this configuration does not run the 16-column fc32 kernels: free-convection ensembles refuse it");
    }
    h->ensemble = true;
    h->n_models = n_models;
    const size_t K = (size_t)n_models, P = (size_t)h->m.n_params;
    const int Nz = h->m.Nz;
    FcEns& en = h->fens;
    en.n_models = n_models;
    en.w = P;
    en.img = fc_image_floats(Nz);
    en.simg = fc_split_image_words(Nz);
    en.bias = (fc_bias_floats(Nz) + 3) / 4 * 4;
    en.sol = (size_t)h->n_col * h->cfg.n_save * h->m.ns;
    h->ens.sol = en.sol;
    h->ens.n_models = n_models;
    auto realloc_ = [&](void** p, size_t bytes) {
        if (*p) { (void)hipFree(*p); *p = nullptr; }
        if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
        return true;
    };
    if (!realloc_((void**)&h->d_w, K * P * sizeof(float)) || !realloc_((void**)&h->d_out, K * (P + 8) * sizeof(float)) ||
        !realloc_((void**)&h->d_partial, K * 256 * 8 * sizeof(float)) || !realloc_((void**)&h->d_sol, K * en.sol * sizeof(float)) ||
        !realloc_((void**)&h->d_fc_imgf, K * en.img * sizeof(float)) || !realloc_((void**)&h->d_fc_imgb, K * en.img * sizeof(float)) ||
        !realloc_((void**)&h->d_fc_bias, K * en.bias * sizeof(float)) || !realloc_((void**)&h->d_fc_simgf, K * en.simg * sizeof(unsigned int)) ||
        !realloc_((void**)&h->d_fc_simgb, K * en.simg * sizeof(unsigned int))) {
        colnde_destroy(h);
        return fail("allocating the free-convection ensemble's per-model buffers (%d models) failed", n_models);
    }
    if (fc_ens_plan_tapes(h)) { colnde_destroy(h); return 1; }
    h->ens_model_bytes += (2 * en.img + en.bias + en.sol) * sizeof(float) + 2 * en.simg * sizeof(unsigned int);
    *out = h;
    return 0;
}

static int fc_ens_pack(colnde_handle* h, const float* d_weights) {
    hipError_t e = fc_launch_pack(h->m, h->fc_cw, d_weights, h->d_fc_imgf, h->d_fc_imgb, h->d_fc_bias, h->d_fc_simgf, h->d_fc_simgb, h->stream, &h->fens);
    if (e != hipSuccess) return fail("fc32 ensemble pack launch failed: %s", hipGetErrorString(e));
    return 0;
}

// all models over the save intervals [iv0, iv1): from the shared x0 (iv0 = 0) or from every model's own saved state at save point iv0
static int fc_ens_forward_range(colnde_handle* h, float* d_sol, bool with_tape, int iv0, int iv1, int tape_iv0) {
    const size_t ns = h->m.ns;
    FcEns en = h->fens;
    en.x0 = iv0 == 0 ? 0 : en.sol;
    const float* init = iv0 == 0 ? h->d_x0 : d_sol + (size_t)iv0 * ns;
    const size_t stride = iv0 == 0 ? ns : (size_t)h->cfg.n_save * ns;
    Timed tm(h, K_FORWARD);
    hipError_t e = fc_launch_forward(h->m, h->fc_cw, h->d_fc_imgf, h->sp_fwd ? h->d_fc_simgf : nullptr, h->d_fc_bias, init, stride, h->d_bcs, h->d_times, h->cfg.n_save,
                                     iv0, iv1, tape_iv0, h->cfg.substeps, d_sol, with_tape ? h->d_dwtape : nullptr, with_tape ? h->d_fc_masks : nullptr,
                                     with_tape ? h->d_fc_switch : nullptr, h->n_col, h->stream, &en);
    if (e != hipSuccess) return fail("fc32 ensemble forward launch failed: %s", hipGetErrorString(e));
    return 0;
}

static int fc_ens_forward(colnde_handle* h, const float* d_weights, float* d_sol) {
    if (fc_ens_pack(h, d_weights)) return 1;
    return fc_ens_forward_range(h, d_sol, false, 0, h->cfg.n_save - 1, 0);
}

// colnde_loss_grad_dev's fc32 branch for all K models: the same launches in the same order, each once for every model; the models march through the
// time segments together (the tape-less pass first, then segment by segment from the end), λ carried per model.
static int fc_ens_loss_grad(colnde_handle* h, const float* d_weights, const LossWeights& lw, float* d_out) {
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    if (check_stability(h)) return 1;
    const int K = h->n_models, stride = h->m.n_params + 8, cw = h->fc_cw;
    const FcEns& en = h->fens;
    if (fc_ens_pack(h, d_weights)) return 1;
    HIPCHK(hipMemsetAsync(h->d_slab, 0, (size_t)K * en.slab * sizeof(float), h->stream));
    const int n_wg = (h->n_col + cw - 1) / cw, n_iv = h->cfg.n_save - 1, nseg = h->fc_nseg;
    const size_t gemm_rows0 = (size_t)n_wg * nseg;                          // a model's slab: [segment][tile] adjoint rows, then [segment][slice] GEMM rows
    const size_t tiles_b = (size_t)n_wg;
    hipError_t e;
    if (nseg > 1 && fc_ens_forward_range(h, h->d_sol, true, 0, n_iv, (nseg - 1) * h->fc_seg)) return 1;
    for (int sg = nseg - 1; sg >= 0; sg--) {
        const int iv0 = sg * h->fc_seg, iv1 = std::min(n_iv, iv0 + h->fc_seg);
        if (!(nseg > 1 && sg == nseg - 1) && fc_ens_forward_range(h, h->d_sol, true, iv0, iv1, iv0)) return 1;
        {
            Timed tm(h, K_ADJOINT);
            e = fc_launch_adjoint(h->m, cw, h->d_fc_imgb, h->sp_adj ? h->d_fc_simgb : nullptr, h->d_times, h->cfg.n_save, iv0, iv1, h->cfg.substeps, h->d_sol, h->d_truth,
                                  h->d_dwtape, h->d_fc_masks, h->d_fc_switch, lw.w[2], nseg > 1 ? h->d_fc_lam : nullptr, h->d_slab + (size_t)sg * n_wg * stride,
                                  h->n_col, h->stream, &en);
            if (e != hipSuccess) return fail("fc32 ensemble adjoint launch failed: %s", hipGetErrorString(e));
        }
        {
            Timed tm(h, K_DW1);
            const size_t n_rec = tiles_b * (cw / 16) * (size_t)(iv1 - iv0) * h->cfg.substeps * h->m.nst;
            float* rows = h->d_slab + (gemm_rows0 + (size_t)sg * h->dw_slices) * stride;
            e = (h->sp_dw && !h->dw_split.passes.empty())
                ? launch_dw_gemm_split(h->d_dwtape, n_rec, (int)dwtape_row_floats(h->m), h->dw_split, h->dw_slices, rows, stride, h->stream, K, en.dwtape, en.slab)
                : launch_dw_gemm(h->d_dwtape, n_rec, (int)dwtape_row_floats(h->m), h->d_macros, h->n_macros, h->dw_slices, rows, stride, h->stream, K, en.dwtape, en.slab);
            if (e != hipSuccess) return fail("ensemble dW GEMM launch failed: %s", hipGetErrorString(e));
        }
    }
    {
        Timed tm(h, K_REDUCE);
        e = launch_reduce(h->d_slab, h->fc_rows, h->m.n_params, stride, lw, d_out, h->stream, K, en.slab, stride);
        if (e != hipSuccess) return fail("ensemble reduce launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

static int fc_ensemble_only(const colnde_handle* h, const char* fn) {
    if (ensemble_only(h)) return 1;
    if (!h->use_fc) return fail("%s takes the handles of colnde_create_fc_ensemble: this ensemble holds wind-mixing models", fn);
    return 0;
}

extern "C" int colnde_ensemble_column_loss_dev(colnde_handle* h, const float* d_sol, float* d_out) {
    if (fc_ensemble_only(h, __func__)) return 1;
    if (!d_sol || !d_out) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_REDUCE);
    hipError_t e = launch_column_loss(d_sol, h->d_truth, h->m.Nz, (long)h->n_col * h->cfg.n_save, h->n_models, d_out, h->stream);
    if (e != hipSuccess) return fail("column loss launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_ensemble_causal_penalty_dev(colnde_handle* h, const float* d_weights, const float* d_coeff, float* d_result) {
    if (fc_ensemble_only(h, __func__)) return 1;
    if (!d_weights || !d_coeff || !d_result) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_REDUCE);
    hipError_t e = launch_causal_penalty(d_weights, d_coeff, d_result, h->m.Nz, h->m.w_off[0], h->m.n_params, h->n_models, h->stream);
    if (e != hipSuccess) return fail("causal penalty launch failed: %s", hipGetErrorString(e));
    return 0;
}

static int ensemble_only(const colnde_handle* h) {
    if (!h) return fail("null handle");
    if (h->closure) return fail("colnde_ensemble_* take weight vectors, but this is a closure handle (no networks): use colnde_closure_* (include/colnde.h)");
    if (h->conv.c) return fail("colnde_ensemble_* do not cover the convolutional first layer of a colnde_create_conv handle (conv=%d): ensembles of conv networks are out of scope", h->conv.c);
    if (!h->ensemble) return fail("not an ensemble handle: colnde_ensemble_* take the handles of colnde_create_ensemble (colnde_create: the single-model calls)");
    return 0;
}

extern "C" int colnde_ensemble_set_physics(colnde_handle* h, const float* physics) {
    if (ensemble_only(h)) return 1;
    if (h->use_fc)
        return fail("colnde_ensemble_set_physics: a free-convection ensemble has no closure constants to vary (its models differ in their weights and ADAM rates only)");
    if (!physics) return fail("null physics array");
    if (!h->cfg.modified_pacanowski_philander)
        return fail("a physics array needs modified_pacanowski_philander = 1: without the Richardson-number closure the five constants are unused");
    HIPCHK(hipSetDevice(h->device));
    int min_sub = 1, stages = 0;
    if (ens_stability(&h->cfg, h->n_models, physics, &min_sub, &stages)) return 1;
    // the tapes hold the stage count planned at creation
    if (stages > h->m.nst)
        return fail("the new constants need %d RKC2 stages per step, the ensemble's tapes were planned for %d: create a new ensemble", stages, h->m.nst);
    if (ens_upload_physics(h, physics)) return 1;
    h->min_substeps = min_sub;
    return 0;
}

// forward solve of all K models (with_tape: into the ensemble's tapes)
static int ens_forward(colnde_handle* h, const float* d_weights, float* d_sol, bool with_tape) {
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    if (check_stability(h)) return 1;
    if (h->use_fc) return fc_ens_forward(h, d_weights, d_sol);
    RtEns ens = h->ens;
    ens.sol = (size_t)h->n_col * h->cfg.n_save * h->m.ns;
    Timed tm(h, K_FORWARD);
    hipError_t e = rt_launch_pack(h->m, d_weights, h->d_wimg, h->stream, h->n_models);
    if (e == hipSuccess)
        e = rt_launch_forward_split(h->m, h->d_wimg, h->d_x0, h->d_bcs, h->d_times, h->cfg.n_save, h->cfg.substeps, d_sol,
                                    with_tape ? h->d_tape : nullptr, with_tape ? h->d_t16_ztape : nullptr, h->n_col, with_tape && h->split_rich,
                                    true, h->sp_fwd, h->stream, ens);
    if (e != hipSuccess) return fail("ensemble forward launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_ensemble_forward_dev(colnde_handle* h, const float* d_weights, float* d_sol) {
    if (ensemble_only(h)) return 1;
    if (!d_weights || !d_sol) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    return ens_forward(h, d_weights, d_sol, false);
}

extern "C" int colnde_ensemble_loss_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out8) {
    if (ensemble_only(h)) return 1;
    if (!d_weights || !scalings || !d_out8) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    if (ens_forward(h, d_weights, h->d_sol, false)) return 1;
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    const int nblk = 256;
    hipError_t e = launch_loss(h->m, h->d_sol, h->d_truth, h->cfg.n_save, h->n_col, h->d_partial, nblk, h->stream, h->n_models, h->ens.sol);
    if (e == hipSuccess) e = launch_reduce(h->d_partial, nblk, 0, 8, lw, d_out8, h->stream, h->n_models, (size_t)nblk * 8, 8);
    if (e != hipSuccess) return fail("ensemble loss launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_ensemble_loss_grad_dev(colnde_handle* h, const float* d_weights, const float scalings[6], float* d_out) {
    if (ensemble_only(h)) return 1;
    if (!d_weights || !scalings || !d_out) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    const int K = h->n_models, stride = h->m.n_params + 8;
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    if (h->use_fc) return fc_ens_loss_grad(h, d_weights, lw, d_out);
    HIPCHK(hipMemsetAsync(h->d_slab, 0, (size_t)K * h->ens.slab * sizeof(float), h->stream));
    if (ens_forward(h, d_weights, h->d_sol, true)) return 1;
    hipError_t e;
    {
        Timed tm(h, K_ADJOINT);
        e = rt_launch_adjoint_split(h->m, h->d_wimg, h->d_times, h->cfg.n_save, h->cfg.substeps, h->d_sol, h->d_truth, h->d_tape, h->d_t16_ztape, lw,
                                    h->d_slab, h->n_col, h->d_dwtape, h->split_rich, true, h->sp_adj, h->stream, h->ens);
        if (e != hipSuccess) return fail("ensemble adjoint launch failed: %s", hipGetErrorString(e));
    }
    {
        Timed tm(h, K_DW1);
        const size_t n_rec = (size_t)h->n_tiles * (h->cfg.n_save - 1) * h->cfg.substeps * h->m.nst;
        float* rows = h->d_slab + (size_t)h->n_tiles * stride;
        e = (h->sp_dw && !h->dw_split.passes.empty())
            ? launch_dw_gemm_split(h->d_dwtape, n_rec, (int)dwtape_row_floats(h->m), h->dw_split, h->dw_slices, rows, stride, h->stream, K, h->ens.dwtape, h->ens.slab)
            : launch_dw_gemm(h->d_dwtape, n_rec, (int)dwtape_row_floats(h->m), h->d_macros, h->n_macros, h->dw_slices, rows, stride, h->stream, K, h->ens.dwtape,
                             h->ens.slab);
        if (e != hipSuccess) return fail("ensemble dW GEMM launch failed: %s", hipGetErrorString(e));
    }
    {
        Timed tm(h, K_REDUCE);
        e = launch_reduce(h->d_slab, h->t16_rows, h->m.n_params, stride, lw, d_out, h->stream, K, h->ens.slab, stride);
        if (e != hipSuccess) return fail("ensemble reduce launch failed: %s", hipGetErrorString(e));
    }
    return 0;
}

extern "C" int colnde_ensemble_loss_grad(colnde_handle* h, const float* weights, const float scalings[6], float* out) {
    if (ensemble_only(h)) return 1;
    if (!weights || !scalings || !out) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    const size_t K = (size_t)h->n_models, P = (size_t)h->m.n_params;
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * K * P, hipMemcpyHostToDevice, h->stream));
    if (colnde_ensemble_loss_grad_dev(h, h->d_w, scalings, h->d_out)) return 1;
    HIPCHK(hipMemcpyAsync(out, h->d_out, sizeof(float) * K * (P + 8), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int colnde_ensemble_adam_step_dev(colnde_handle* h, float* d_weights, const float* d_result, float* d_m, float* d_v, const float* d_eta,
                                             float beta1, float beta2, float eps, float beta1_t, float beta2_t) {
    if (ensemble_only(h)) return 1;
    if (!d_weights || !d_result || !d_m || !d_v || !d_eta) return fail("null pointer argument");
    if (!(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f)) return fail("0 <= beta < 1 required");
    if (!(beta1_t < 1.0f && beta2_t < 1.0f)) return fail("running powers beta^t must be < 1");
    HIPCHK(hipSetDevice(h->device));
    Timed tm(h, K_ADAM);
    hipError_t e = launch_adam_ensemble(d_weights, d_result, h->m.n_params + 8, d_m, d_v, d_eta, beta1, beta2, eps, beta1_t, beta2_t, h->m.n_params,
                                        h->n_models, h->stream);
    if (e != hipSuccess) return fail("ensemble ADAM launch failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- error-controlled time stepping: what `reltol` means at this boundary ------------------------------------------------------------
// The reference hands the solve to an adaptive integrator (solve(prob, ROCK4(); reltol=1f-3, ...): NDE_training.jl:291,304,403; reltol=1e-4 at
// free_convection/src/solve.jl:4).  This path steps at a fixed `substeps` per save interval, so the tolerance is enforced a posteriori: a second
// forward solve at 2 x substeps and Richardson's estimate of the error of the first, e = (u_S - u_2S) 2^p / (2^p - 1) (p = 4: RK4, 2: RKC2), in
// the integrator's own norm: per column and save point the RMS over the state's components of e_i / (abstol / reltol + |u_i|), abstol / reltol = 1e-3
// (OrdinaryDiffEq's default abstol 1e-6 over the reference's reltol; its accept test is rms(err / (abstol + reltol |u|)) <= 1), then the maximum over
// columns and save points.
static int forward_at(colnde_handle* h, const float* d_weights, float* d_sol, int substeps) {
    const int keep = h->cfg.substeps;
    h->cfg.substeps = substeps;
    const bool au = h->auto_substeps;
    h->auto_substeps = false;
    int rc = refresh_rkc(h);
    if (!rc) rc = forward_impl(h, d_weights, d_sol, false);
    h->cfg.substeps = keep;
    h->auto_substeps = au;
    if (refresh_rkc(h)) rc = 1;
    return rc;
}

static int tapes_planned(const colnde_handle* h) { return h->d_rt_tape || h->d_dwtape || h->d_tape; }

// estimate at `substeps` given its solution d_a; d_b receives the solution at 2 x substeps; *d_est (device) the estimate
static int estimate_from(colnde_handle* h, const float* d_weights, const float* d_a, float* d_b, int substeps, float* d_est, float floor_) {
    if (forward_at(h, d_weights, d_b, 2 * substeps)) return 1;
    hipError_t e = launch_rel_diff_max(d_a, d_b, (long)h->n_col * h->cfg.n_save, h->m.ns, floor_, h->d_partial, d_est, h->stream);
    if (e != hipSuccess) return fail("error-estimate launch failed: %s", hipGetErrorString(e));
    return 0;
}

// 2^p / (2^p - 1) with the order the right-hand side lets the stepper reach: a SWITCHING right-hand side (ConvectiveAdjustmentNDE's min(0, K dT/dz),
// the wind-mixing convective-adjustment branch) converges at about first order through its kinks whatever the stepper's nominal order (measured:
// profiles/r05_rkc2_conditioning.json), so the conservative factor 2 is used there (p = 4 / 2 understated the error by up to 2x);
// smooth closures keep p = 4 (RK4) and p = 2 (RKC2).
static float richardson_factor(const colnde_handle* h) {
    if (h->m.ca || h->cfg.model == COLNDE_MODEL_CONV_ADJ_NDE) return 2.0f;
    return h->cfg.stepper == COLNDE_STEPPER_RKC2 ? 4.0f / 3.0f : 16.0f / 15.0f;
}
// abstol / reltol of the integrator's accept test rms(err / (abstol + reltol |u|)) <= 1, OrdinaryDiffEq's default abstol = 1e-6: 1e-3 at the wind-mixing
// reltol = 1e-3 (NDE_training.jl:291), 1e-2 at free convection's 1e-4 (solve.jl:4)
static float norm_floor(float reltol) { return 1e-6f / (reltol > 0.0f ? reltol : 1e-3f); }

extern "C" int colnde_error_estimate_dev(colnde_handle* h, const float* d_weights, float* max_rel_err) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h) return fail("null handle");
    if (!d_weights || !max_rel_err) return fail("null pointer argument");
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->n_col * h->cfg.n_save * h->m.ns;
    float* d_b = nullptr;
    HIPCHK(hipMalloc((void**)&d_b, (n + 4) * sizeof(float)));
    int rc = forward_at(h, d_weights, h->d_sol, h->cfg.substeps);
    if (!rc) rc = estimate_from(h, d_weights, h->d_sol, d_b, h->cfg.substeps, d_b + n, norm_floor(h->cfg.reltol));
    float est = 0.0f;
    if (!rc && (hipMemcpyAsync(&est, d_b + n, sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess))
        rc = fail("error estimate: device-to-host copy failed");
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(d_b);
    if (rc) return 1;
    *max_rel_err = est * richardson_factor(h);
    return 0;
}

extern "C" int colnde_error_estimate(colnde_handle* h, const float* weights, float* max_rel_err) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h) return fail("null handle");
    if (!weights || !max_rel_err) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * h->m.n_params, hipMemcpyHostToDevice, h->stream));
    return colnde_error_estimate_dev(h, h->d_w, max_rel_err);
}

// The least power-of-two sub-step count (not below the stability bound) whose estimate meets reltol; the handle keeps it.
static int choose_substeps_impl(colnde_handle* h, const float* d_weights, float reltol, int* chosen, float* estimate) {
    if (tapes_planned(h)) return fail("the sub-step count sizes the tapes: choose it before the first colnde_loss_grad of this handle");
    if (!(reltol > 0.0f)) return fail("reltol must be > 0");
    const size_t n = (size_t)h->n_col * h->cfg.n_save * h->m.ns;
    float* d_b = nullptr;
    HIPCHK(hipMalloc((void**)&d_b, (2 * n + 4) * sizeof(float)));
    float* buf[2] = {d_b, d_b + n};
    int S = 1;
    while (S < h->min_substeps) S *= 2;
    int rc = forward_at(h, d_weights, buf[0], S);
    float est = -1.0f, prev = -1.0f;
    int cur = 0;
    bool floor_hit = false;
    while (!rc) {
        rc = estimate_from(h, d_weights, buf[cur], buf[cur ^ 1], S, d_b + 2 * n, norm_floor(reltol));
        if (rc) break;
        float e = 0.0f;
        if (hipMemcpyAsync(&e, d_b + 2 * n, sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
            rc = fail("choose_substeps: device-to-host copy failed");
            break;
        }
        est = e * richardson_factor(h);
        if (!(est == est) || est > 3.0e38f) { rc = fail("the solve is not finite at %d sub-steps per save interval: no sub-step count can be chosen", S); break; }
        if (est <= reltol || S >= 4096) break;
        // halving a fourth-order step divides the error by ~16 (second order: 4; a switch in the right-hand side — ConvectiveAdjustmentNDE — makes it ~2);
        // an estimate that falls by less than a fifth is float32 round-off of the two solves it compares (more steps only add to it): the tolerance is
        // below what this arithmetic resolves
        if (prev > 0.0f && est > 0.8f * prev) { floor_hit = true; break; }
        prev = est;
        S *= 2;                      // the solution at 2S is already there: it is the next candidate's own
        cur ^= 1;
    }
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(d_b);
    if (rc) return 1;
    if (floor_hit) return fail("reltol = %g is below the float32 round-off floor of this solve: the estimate stopped falling at %g (%d sub-steps per save interval, "
                               "%g at half as many)", reltol, est, S, prev);
    if (est > reltol) return fail("reltol = %g is not met with %d sub-steps per save interval (estimate %g): the right-hand side is too stiff for this stepper", reltol, S, est);
    h->cfg.substeps = S;
    if (refresh_rkc(h)) return 1;
    h->last_estimate = est;
    h->substeps_chosen = true;
    if (chosen) *chosen = S;
    if (estimate) *estimate = est;
    return 0;
}

extern "C" int colnde_choose_substeps(colnde_handle* h, const float* weights, float reltol, int* substeps, float* estimate) {
    SINGLE_MODEL_ONLY(h);
    PLAIN_NETWORK_ONLY(h);
    if (!h) return fail("null handle");
    if (!weights) return fail("null weights");
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * h->m.n_params, hipMemcpyHostToDevice, h->stream));
    const bool au = h->auto_substeps;
    h->auto_substeps = false;
    const int rc = choose_substeps_impl(h, h->d_w, reltol > 0.0f ? reltol : h->cfg.reltol, substeps, estimate);
    if (rc) h->auto_substeps = au;
    return rc;
}

extern "C" int colnde_substeps(const colnde_handle* h) { return h ? h->cfg.substeps : -1; }

// Impose a sub-step count (e.g. the MAX over ranks of what colnde_choose_substeps chose on each shard).  Refused once the tapes are planned (the count
// sizes them) and outside the stepper's stability bound; clears a pending substeps = 0.
extern "C" int colnde_set_substeps(colnde_handle* h, int substeps) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (substeps < 1) return fail("substeps must be >= 1");
    if (substeps == h->cfg.substeps && !h->auto_substeps) return 0;
    if (tapes_planned(h)) return fail("the sub-step count sizes the tapes: set it before the first colnde_loss_grad of this handle");
    colnde_config c = h->cfg;
    c.substeps = substeps;
    const int need = colnde_min_substeps(&c);
    if (need < 0) return 1;
    if (substeps < need && !getenv("COLNDE_ALLOW_UNSTABLE_DT"))
        return fail("substeps = %d is outside the stepper's stability bound: need >= %d (colnde_min_substeps)", substeps, need);
    h->cfg.substeps = substeps;
    h->auto_substeps = false;
    h->substeps_chosen = false;
    h->last_estimate = -1.0f;
    return refresh_rkc(h);
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
    float* d_loss = nullptr;
    HIPCHK(hipMalloc((void**)&d_loss, sizeof(float) + 2 * sizeof(double) + 8));
    double* d_bt = reinterpret_cast<double*>(reinterpret_cast<char*>(d_loss) + 8);
    hipError_t e = launch_pretrain(h->m, flux_type, d_theta, d_m, d_v, d_profiles, d_bcs, d_flux, d_order, n_samples, gradient_scaling,
                                   eta, beta1, beta2, eps, beta_t[0], beta_t[1], update, d_loss, d_bt, h->stream);
    float loss = 0.0f;
    double bt[2] = {beta_t[0], beta_t[1]};
    if (e == hipSuccess) e = hipMemcpyAsync(&loss, d_loss, sizeof(float), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(bt, d_bt, sizeof(bt), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d_loss);
    if (e != hipSuccess) return fail("flux pre-training failed: %s", hipGetErrorString(e));
    *mean_loss = loss / (float)n_samples;
    if (update) { beta_t[0] = bt[0]; beta_t[1] = bt[1]; }
    return 0;
}

extern "C" int colnde_plan(const colnde_handle* h, int info[8]) {
    if (!h || !info) return fail("null argument");
    for (int i = 0; i < 8; i++) info[i] = 0;
    info[0] = h->use_rt ? COLNDE_ENGINE_MFMA : (h->use_fc ? COLNDE_ENGINE_FC32 : COLNDE_ENGINE_GENERIC);
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
        bf_dw = h->sp_dw && (h->d_dwtape ? !h->dw_split.passes.empty() : true);
    } else {
        bf_fwd = (h->sp_fwd && h->fwd_split && h->fwd_helper) || h->m.sf != nullptr;
        bf_adj = (h->sp_adj && h->adj_split && rt_adjoint_split_has_bf16(h->m, h->adj_helper) && (h->t16_dwtape < 0 || (h->t16_dwtape == 1 && h->d_t16_ztape))) || h->m.sb != nullptr;
        bf_dw = h->sp_dw && h->t16_dwtape == 1 && !h->dw_split.passes.empty();
    }
    info[7] |= (bf_fwd ? 2 : 0) | (bf_adj ? 4 : 0) | (bf_dw ? 8 : 0);
    if (h->use_fc) {
        info[1] = h->fc_block;
        info[2] = h->fc_nblocks;
        info[3] = h->fc_nseg > 1 ? h->fc_nseg : 0;       // fc32: time segments of the tapes (0: the tapes hold the whole axis)
        info[4] = h->d_dwtape ? 1 : 0;
        info[5] = h->d_dwtape ? h->dw_slices : 0;
        info[6] = h->conv.c;
    } else if (h->use_rt) {
        info[1] = h->rt_block;
        info[2] = h->rt_nblocks;
        info[3] = h->rt_ztape ? 1 : 0;
    } else {
        info[1] = h->t16_dwtape == 1 ? h->t16_block : 0;
        info[2] = h->t16_dwtape == 1 ? h->t16_nblocks : 0;
        info[4] = h->t16_dwtape == 1 ? 1 : 0;
        info[5] = h->t16_dwtape == 1 ? h->dw_slices : 0;
        info[6] = (h->fwd_split ? 1 : 0) | ((h->adj_split && h->t16_dwtape == 1 && h->d_t16_ztape) ? 2 : 0) | (h->split_rich ? 4 : 0);
    }
    return 0;
}

// Every environment variable some part of the library reads (api.hip, api_embed.hip, engine_*.hip): the list colnde_describe reports from.
static const char* const COLNDE_ENV_SWITCHES[] = {
    "COLNDE_FWD_SPLIT", "COLNDE_ADJ_SPLIT", "COLNDE_DW_SPLIT", "COLNDE_ADJ_GEOM", "COLNDE_FWD_WLDS", "COLNDE_FWD_THREADS", "COLNDE_T16_FWD_HELPER",
    "COLNDE_T16_ADJ_HELPER", "COLNDE_T16_FWD_SPLIT", "COLNDE_T16_ADJ_SPLIT", "COLNDE_FC", "COLNDE_FC_CW", "COLNDE_FC_EMBED_FUSED", "COLNDE_FC_BLOCK", "COLNDE_FC_SEG", "COLNDE_WM_ENS_GRID",
    "COLNDE_RT_ZTAPE", "COLNDE_RT_BLOCK", "COLNDE_RT_FWD", "COLNDE_ALLOW_UNSTABLE_DT", "COLNDE_T16_DWTAPE", "COLNDE_T16_ZTAPE", "COLNDE_T16_SPLIT_RICH",
    "COLNDE_T16_BLOCK", "COLNDE_T16_DWLDS", "COLNDE_T16_TAPE_THREADS", "COLNDE_T16_TAPE_WLDS"};

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
        const char* e = getenv("COLNDE_ALLOW_UNSTABLE_DT");
        s += " | env";
        if (e && *e) { s += " COLNDE_ALLOW_UNSTABLE_DT="; s += e; } else s += " (none set)";
        const int need = (int)s.size() + 1;
        if (buf && capacity > 0) {
            const int n = need <= capacity ? need - 1 : capacity - 1;
            memcpy(buf, s.data(), n);
            buf[n] = 0;
        }
        return need;
    }
    const char* eng = info[0] == COLNDE_ENGINE_MFMA ? "regtile" : info[0] == COLNDE_ENGINE_FC32 ? "fc32" : ((info[6] & 1) ? "tile16+net-split" : "tile16");
    if (info[0] == COLNDE_ENGINE_FC32) info[6] = 0;                  // (fc32: the filter length of a conv handle, reported below; the bits are tile16's)
    char why[96] = "";
    if (h->auto_substeps) snprintf(why, sizeof why, "(stability bound; pending: the first solve chooses from reltol=%g)", h->cfg.reltol);
    else if (h->substeps_chosen) snprintf(why, sizeof why, "(chosen from reltol, estimate=%.3g)", h->last_estimate);
    snprintf(t, sizeof t, "engine=%s columns=%d stepper=%s substeps=%d%s", eng, h->cfg.n_columns, h->cfg.stepper == COLNDE_STEPPER_RKC2 ? "rkc2" : "rk4",
             h->cfg.substeps, why);
    s += t;
    if (h->conv.c) { snprintf(t, sizeof t, " conv=%d n_params=%d", h->conv.c, h->conv.n_params); s += t; }
    if (h->ensemble) { snprintf(t, sizeof t, " models=%d tape_bytes_per_model=%zu", h->n_models, h->ens_model_bytes); s += t; }
    if (h->cfg.stepper == COLNDE_STEPPER_RKC2) { snprintf(t, sizeof t, " rkc_stages=%d%s", h->m.nst, h->cfg.rkc_stages ? "" : "(automatic)"); s += t; }
    snprintf(t, sizeof t, " matrix_arithmetic=%s forward=%s adjoint=%s dw=%s", h->cfg.matrix_arithmetic == COLNDE_MATRIX_BF16X3_EXACT ? "bf16x3_exact" : "f32_mfma",
             (info[7] & 2) ? "bf16x3" : "f32", (info[7] & 4) ? "bf16x3" : "f32", (info[7] & 8) ? "bf16x3" : "f32");
    s += t;
    if (wm_infer_covers(h)) s += " wm_infer=f32";      // colnde_wm_infer_dz_flux / colnde_wm_embedded_step[_flux] / colnde_wm_diagnose_flux: the f32 matrix pipe under either arithmetic
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
    for (const char* name : COLNDE_ENV_SWITCHES) {
        const char* e = getenv(name);
        if (e && *e) { s += " "; s += name; s += "="; s += e; any = true; }
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
    const int need = (int)s.size() + 1;
    if (buf && capacity > 0) {
        const int n = need <= capacity ? need - 1 : capacity - 1;
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return need;
}

// Diagnostic builds (-DCOLNDE_STAMPS) only; not part of include/colnde.h.  Returns zeros in the shipped library.
extern "C" int colnde_debug_stamps(colnde_handle* h, unsigned long long* out16) {
    if (!h || !out16) return fail("null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->use_rt || h->adj_split) {
        for (int i = 0; i < 16; i++) out16[i] = 0;
        HIPCHK(rt_debug_read_stamps(out16));
        return 0;
    }
    HIPCHK(debug_read_stamps(out16));
    return 0;
}

// ---- closure-only model: calibrating the five Pacanowski-Philander constants (colnde_create_closure) ------------------------------------------------
// The reference fits nu0, nu_minus, dRi, Ric, Pr to the LES profiles before any network is trained (optimise_modified_pacanowski_philander,
// wind_mixing/src/diffusivity_parameter_optimisation.jl:35-231): the same column ODE without the MLPs (DE, :1-33), the same six-term loss (:150-163).
// A closure handle holds K constant sets on the same columns; every kernel (engine_closure.hip) runs once for all K.

// cfg as the closure model reads it: wind mixing, MPP, one placeholder Dense layer so that validate() has a network to look at
static colnde_config closure_config(const colnde_config* cfg, const float* params) {
    colnde_config c = *cfg;
    c.n_layers = 1;
    c.layer_sizes[0] = 3 * c.Nz;
    c.layer_sizes[1] = c.Nz - 1;
    c.activations[0] = COLNDE_ACT_IDENTITY;
    if (params) { c.nu0 = params[0]; c.nu_minus = params[1]; c.dRi = params[2]; c.Ric = params[3]; c.Pr = params[4]; }
    return c;
}

static int closure_refusals(const colnde_config* cfg) {
    if (!cfg) return fail("null config");
    if (cfg->model != COLNDE_MODEL_WIND_MIXING) return fail("the closure model is the wind-mixing column without networks: model = %d is refused", cfg->model);
    if (!cfg->modified_pacanowski_philander) return fail("the closure model IS the modified Pacanowski-Philander closure: modified_pacanowski_philander must be 1");
    if (cfg->convective_adjustment) return fail("closure model: convective_adjustment is not part of DE (diffusivity_parameter_optimisation.jl:1-33)");
    if (cfg->smooth_NN) return fail("closure model: smooth_NN filters network outputs, and there are none");
    if (cfg->smooth_Ri) return fail("closure model: smooth_Ri is not part of DE (diffusivity_parameter_optimisation.jl:1-33)");
    if (cfg->diurnal) return fail("closure model: diurnal forcing is not supported (DE takes constant boundary fluxes)");
    if (cfg->inplace_variant) return fail("closure model: inplace_variant (the NDE! evaluation arithmetic) is not supported");
    if (cfg->stepper != COLNDE_STEPPER_RK4) return fail("closure model: classical RK4 only (RKC2 is not supported)");
    if (cfg->substeps == 0) return fail("closure model: substeps = 0 (chosen from reltol) is not supported: the tape is sized at creation — pass substeps >= "
                                        "colnde_closure_min_substeps of the constants you start from");
    if (cfg->engine != COLNDE_ENGINE_AUTO) return fail("closure model: engine forced to %d, but the closure kernels are an engine of their own (use COLNDE_ENGINE_AUTO)", cfg->engine);
    if (cfg->Nz > CLOSURE_MAX_NZ) return fail("closure model: Nz = %d outside 4..%d (a lane per level)", cfg->Nz, CLOSURE_MAX_NZ);
    return 0;
}

extern "C" int colnde_closure_min_substeps(const colnde_config* cfg, const float params[5]) {
    if (!cfg || !params) { fail("null argument"); return -1; }
    for (int q = 0; q < 5; q++)
        if (!std::isfinite(params[q])) { fail("params[%d] = %g is not finite", q, params[q]); return -1; }
    if (!(params[2] > 0.0f) || !(params[4] > 0.0f)) { fail("dRi = %g and Pr = %g must be > 0", params[2], params[4]); return -1; }
    colnde_config c = closure_config(cfg, params);
    c.model = COLNDE_MODEL_WIND_MIXING;
    c.modified_pacanowski_philander = 1;
    c.convective_adjustment = 0;
    c.inplace_variant = 0;
    c.stepper = COLNDE_STEPPER_RK4;
    return colnde_min_substeps(&c);
}

extern "C" int colnde_create_closure(const colnde_config* cfg, int n_sets, colnde_handle** out) {
    if (!out) return fail("null out pointer");
    *out = nullptr;
    if (closure_refusals(cfg)) return 1;
    const colnde_config cc = closure_config(cfg, nullptr);
    if (validate(&cc)) return 1;
    if (n_sets < 1) return fail("n_sets = %d must be >= 1", n_sets);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail("no HIP device visible: colnde has no CPU fallback (the product path is the gfx950 HIP engine)");
    if (cc.device < 0 || cc.device >= ndev) return fail("device %d not in 0..%d", cc.device, ndev - 1);
    HIPCHK(hipSetDevice(cc.device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cc.device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("device %d is %s; this library is built for gfx950 (MI355X) only", cc.device, prop.gcnArchName);

    colnde_handle* h = new (std::nothrow) colnde_handle();
    if (!h) return fail("out of host memory");
    h->cfg = cc;
    h->save_times.assign(cc.save_times, cc.save_times + cc.n_save);
    h->cfg.save_times = h->save_times.data();
    h->device = cc.device;
    h->n_col = cc.n_columns;
    h->n_col_total = cc.n_columns;
    h->closure = true;
    h->n_models = n_sets;
    PackInfo pk;
    build_model(&cc, &h->m, &pk);            // scalings and the physics prefactors; the network fields are not used
    h->m.n_params = CLOSURE_N_PARAMS;
    h->m.n_nets = 0;
    h->m.nst = 4;
    ClosureModel& cm = h->cm;
    cm.Nz = cc.Nz; cm.n_save = cc.n_save; cm.substeps = cc.substeps; cm.n_col = cc.n_columns; cm.n_sets = n_sets;
    for (int k = 0; k < 3; k++) { cm.cs[k] = h->m.cs[k]; cm.A[k] = h->m.A[k]; cm.s0[k] = h->m.s0[k]; }
    cm.B = h->m.B; cm.cor_u = h->m.cor_u; cm.cor_v = h->m.cor_v; cm.sig_u = h->m.sig_u; cm.sig_v = h->m.sig_v; cm.mu_u = h->m.mu_u; cm.mu_v = h->m.mu_v;
    cm.eps = h->m.eps;
    // the tape of all sets, the solutions and the partial rows are allocated here: a handle that does not fit is refused with the bytes it needs
    const size_t K = (size_t)n_sets, ns = (size_t)h->m.ns;
    const size_t b_tape = K * closure_tape_floats(cm) * sizeof(float), b_sol = K * h->n_col * cc.n_save * ns * sizeof(float),
                 b_rows = K * h->n_col * CLOSURE_ROW * sizeof(float), b_small = K * (CLOSURE_N_PARAMS + CLOSURE_N_PARAMS + 8) * sizeof(float),
                 b_problem = (size_t)h->n_col * (ns * (1 + cc.n_save) + 6) * sizeof(float);
    const size_t need = b_tape + b_sol + b_rows + b_small + b_problem;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { delete h; return fail("hipMemGetInfo failed"); }
    const size_t margin = (size_t)1 << 30;
    if (need + margin > free_b) {
        delete h;
        return fail("a closure handle of %d sets x %d columns needs %zu bytes of device memory (%zu of them the step-start tape: %d save intervals x %d substeps x "
                    "%zu floats per column and set); %zu bytes are free (1 GB kept in reserve): use fewer sets per handle",
                    n_sets, cc.n_columns, need, b_tape, cc.n_save - 1, cc.substeps, ns, free_b);
    }
    h->cl_tape_bytes = b_tape;
    hipError_t e = hipMalloc((void**)&h->d_cl_tape, b_tape);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_sol, b_sol);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_cl_rows, b_rows);
    if (e == hipSuccess) e = hipMemset(h->d_cl_rows, 0, b_rows);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_cl_params, K * CLOSURE_N_PARAMS * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_out, K * (CLOSURE_N_PARAMS + 8) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_x0, (size_t)h->n_col * ns * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_bcs, (size_t)h->n_col * 6 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_times, cc.n_save * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->d_times, h->save_times.data(), sizeof(float) * cc.n_save, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        colnde_destroy(h);
        return fail("allocating the closure handle's buffers (%zu bytes, %zu of them tape) failed: %s", need, b_tape, hipGetErrorString(e));
    }
    *out = h;
    return 0;
}

static int closure_only(const colnde_handle* h) {
    if (!h) return fail("null handle");
    if (h->conv.c) return fail("colnde_closure_* take the handles of colnde_create_closure: this is a colnde_create_conv handle (conv=%d)", h->conv.c);
    if (!h->closure) return fail("not a closure handle: colnde_closure_* take the handles of colnde_create_closure");
    return 0;
}

// host-side stability check of every set (the _dev calls cannot see the values)
static int closure_check_sets(const colnde_handle* h, const float* params) {
    const char* e = getenv("COLNDE_ALLOW_UNSTABLE_DT");
    const bool allow = e && atoi(e) != 0;
    for (int k = 0; k < h->n_models; k++) {
        const float* r = params + (size_t)CLOSURE_N_PARAMS * k;
        const int ms = colnde_closure_min_substeps(&h->cfg, r);
        if (ms < 0) return fail("set %d: %s", k, std::string(g_err).c_str());
        if (h->cfg.substeps < ms && !allow)
            return fail("set %d (nu0 = %g, nu_minus = %g, Pr = %g) needs substeps >= %d for a stable RK4 step (colnde_closure_min_substeps), but the handle runs "
                        "substeps = %d (COLNDE_ALLOW_UNSTABLE_DT=1 overrides)", k, r[0], r[1], r[4], ms, h->cfg.substeps);
    }
    return 0;
}

static int closure_forward_impl(colnde_handle* h, const float* d_params, float* d_sol, bool with_tape, bool with_loss) {
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    Timed tm(h, K_FORWARD);
    hipError_t e = closure_launch_forward(h->cm, d_params, h->d_x0, h->d_bcs, h->d_times, d_sol, with_tape ? h->d_cl_tape : nullptr,
                                          with_loss ? h->d_truth : nullptr, with_loss ? h->d_cl_rows : nullptr, h->stream);
    if (e != hipSuccess) return fail("closure forward launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_closure_forward_dev(colnde_handle* h, const float* d_params, float* d_sol) {
    if (closure_only(h)) return 1;
    if (!d_params) return fail("null pointer argument");
    HIPCHK(hipSetDevice(h->device));
    return closure_forward_impl(h, d_params, d_sol ? d_sol : h->d_sol, false, false);
}

extern "C" int colnde_closure_loss_dev(colnde_handle* h, const float* d_params, const float scalings[6], float* d_out8) {
    if (closure_only(h)) return 1;
    if (!d_params || !scalings || !d_out8) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    if (closure_forward_impl(h, d_params, h->d_sol, false, true)) return 1;
    Timed tm(h, K_REDUCE);
    hipError_t e = closure_launch_reduce(h->cm, h->d_cl_rows, lw, false, d_out8, h->stream);
    if (e != hipSuccess) return fail("closure reduce launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_closure_loss_grad_dev(colnde_handle* h, const float* d_params, const float scalings[6], float* d_out) {
    if (closure_only(h)) return 1;
    if (!d_params || !scalings || !d_out) return fail("null pointer argument");
    if (!h->have_truth) return fail("no truth trajectories: pass truth to colnde_set_problem");
    HIPCHK(hipSetDevice(h->device));
    LossWeights lw;
    loss_weights(h, scalings, &lw);
    if (closure_forward_impl(h, d_params, h->d_sol, true, true)) return 1;
    {
        Timed tm(h, K_ADJOINT);
        hipError_t e = closure_launch_adjoint(h->cm, d_params, h->d_bcs, h->d_times, h->d_sol, h->d_truth, h->d_cl_tape, lw, h->d_cl_rows, h->stream);
        if (e != hipSuccess) return fail("closure adjoint launch failed: %s", hipGetErrorString(e));
    }
    Timed tm(h, K_REDUCE);
    hipError_t e = closure_launch_reduce(h->cm, h->d_cl_rows, lw, true, d_out, h->stream);
    if (e != hipSuccess) return fail("closure reduce launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_closure_forward(colnde_handle* h, const float* params, float* sol) {
    if (closure_only(h)) return 1;
    if (!params) return fail("null pointer argument");
    if (closure_check_sets(h, params)) return 1;
    HIPCHK(hipSetDevice(h->device));
    const size_t K = (size_t)h->n_models;
    HIPCHK(hipMemcpyAsync(h->d_cl_params, params, sizeof(float) * K * CLOSURE_N_PARAMS, hipMemcpyHostToDevice, h->stream));
    if (closure_forward_impl(h, h->d_cl_params, h->d_sol, false, false)) return 1;
    if (sol)
        HIPCHK(hipMemcpyAsync(sol, h->d_sol, sizeof(float) * K * h->n_col * h->cfg.n_save * h->m.ns, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int colnde_closure_loss_grad(colnde_handle* h, const float* params, const float scalings[6], float* out) {
    if (closure_only(h)) return 1;
    if (!params || !scalings || !out) return fail("null pointer argument");
    if (closure_check_sets(h, params)) return 1;
    HIPCHK(hipSetDevice(h->device));
    const size_t K = (size_t)h->n_models;
    HIPCHK(hipMemcpyAsync(h->d_cl_params, params, sizeof(float) * K * CLOSURE_N_PARAMS, hipMemcpyHostToDevice, h->stream));
    if (colnde_closure_loss_grad_dev(h, h->d_cl_params, scalings, h->d_out)) return 1;
    HIPCHK(hipMemcpyAsync(out, h->d_out, sizeof(float) * K * (CLOSURE_N_PARAMS + 8), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
