// api_substeps.hip — the sub-step count: error estimate, colnde_choose_substeps, colnde_set_substeps.
#include "api_internal.h"

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
    DevScratch sc(h->stream);
    HIPCHK(sc.alloc((n + 4) * sizeof(float)));
    float* d_b = sc.p;
    int rc = forward_at(h, d_weights, h->d_sol, h->cfg.substeps);
    if (!rc) rc = estimate_from(h, d_weights, h->d_sol, d_b, h->cfg.substeps, d_b + n, norm_floor(h->cfg.reltol));
    float est = 0.0f;
    if (!rc && (hipMemcpyAsync(&est, d_b + n, sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess))
        rc = fail("error estimate: device-to-host copy failed");
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
int choose_substeps_impl(colnde_handle* h, const float* d_weights, float reltol, int* chosen, float* estimate) {
    if (tapes_planned(h)) return fail("the sub-step count sizes the tapes: choose it before the first colnde_loss_grad of this handle");
    if (!(reltol > 0.0f)) return fail("reltol must be > 0");
    const size_t n = (size_t)h->n_col * h->cfg.n_save * h->m.ns;
    DevScratch sc(h->stream);
    HIPCHK(sc.alloc((2 * n + 4) * sizeof(float)));
    float* d_b = sc.p;
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
    if (substeps < need && !allow_unstable())
        return fail("substeps = %d is outside the stepper's stability bound: need >= %d (colnde_min_substeps)", substeps, need);
    h->cfg.substeps = substeps;
    h->auto_substeps = false;
    h->substeps_chosen = false;
    h->last_estimate = -1.0f;
    return refresh_rkc(h);
}
