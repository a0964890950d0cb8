// api_substeps.hip — the sub-step count: error estimate, colnde_choose_substeps, colnde_set_substeps; the per-interval step schedule.
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
static int forward_scheduled(colnde_handle* h, const float* d_weights, float* d_sol, const std::vector<int>& S);
static int upload_schedule(colnde_handle* h, const int* counts);

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
    int rc = 0;
    if (!h->sched.empty()) {          // under a step schedule: the schedule against every interval doubled
        const std::vector<int> S = h->sched;
        std::vector<int> S2(S);
        for (int& c : S2) c *= 2;
        rc = forward_scheduled(h, d_weights, h->d_sol, S) || forward_scheduled(h, d_weights, d_b, S2);
        if (!rc && launch_rel_diff_max(h->d_sol, d_b, (long)h->n_col * h->cfg.n_save, h->m.ns, norm_floor(h->cfg.reltol), h->d_partial, d_b + n, h->stream) != hipSuccess)
            rc = fail("error-estimate launch failed");
        h->sched = S;                                                // the counts in force again, on the device too
        if (upload_schedule(h, S.data())) rc = 1;
    } else {
        rc = forward_at(h, d_weights, h->d_sol, h->cfg.substeps);
        if (!rc) rc = estimate_from(h, d_weights, h->d_sol, d_b, h->cfg.substeps, d_b + n, norm_floor(h->cfg.reltol));
    }
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
    // one count for every interval is what is chosen here: it takes a step schedule's place (which a failure puts back; its device copy is untouched)
    struct Restore {
        colnde_handle* h;
        std::vector<int> keep;
        bool done = false;
        ~Restore() { if (!done) h->sched.swap(keep); }
    } schedule_guard{h, {}};
    schedule_guard.keep.swap(h->sched);
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
    schedule_guard.done = true;
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
// sizes them) and outside the stepper's stability bound; clears a pending substeps = 0 and a step schedule (colnde_set_schedule).
extern "C" int colnde_set_substeps(colnde_handle* h, int substeps) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (substeps < 1) return fail("substeps must be >= 1");
    if (substeps == h->cfg.substeps && !h->auto_substeps && h->sched.empty()) return 0;
    if (tapes_planned(h)) return fail("the sub-step count sizes the tapes: set it before the first colnde_loss_grad of this handle");
    colnde_config c = h->cfg;
    c.substeps = substeps;
    const int need = colnde_min_substeps(&c);
    if (need < 0) return 1;
    if (substeps < need && !allow_unstable())
        return fail("substeps = %d is outside the stepper's stability bound: need >= %d (colnde_min_substeps)", substeps, need);
    h->cfg.substeps = substeps;
    h->sched.clear();                                      // one count for every interval again
    h->auto_substeps = false;
    h->substeps_chosen = false;
    h->last_estimate = -1.0f;
    return refresh_rkc(h);
}

// ---- the step schedule: RK4 steps per save interval (step_schedule.h) ------------------------------------------------------------------
// One global `substeps` makes every save interval pay for the most demanding one.  A schedule gives interval n its own count S_n, the same for all
// columns and members; the four-wave net-split pair (rt16sh_forward_sched_kernel / rt16sh_adjoint_sched_kernel) steps and tapes by it.

// per interval, what the stability bound asks: of an ensemble, the largest any model's constants ask
int schedule_minima(const colnde_handle* h, std::vector<int>* minima) {
    const int n_iv = h->cfg.n_save - 1;
    minima->assign((size_t)n_iv, 1);
    std::vector<int> one((size_t)n_iv);
    const bool per_model = h->ensemble && !h->phys_raw.empty();
    for (int k = 0; k < (per_model ? h->n_models : 1); k++) {
        const colnde_config c = per_model ? model_config(&h->cfg, h->phys_raw.data(), k) : h->cfg;
        if (colnde_schedule_min(&c, one.data())) return 1;
        for (int i = 0; i < n_iv; i++) (*minima)[i] = std::max((*minima)[i], one[i]);
    }
    return 0;
}

// Which handles step by a schedule: those whose solves run on rt16sh_forward_kernel / rt16sh_adjoint_kernel.  Decided from the handle alone, before any device work.
static int refuse_schedule(const colnde_handle* h) {
    static const char* only = "a step schedule covers the four-wave net-split kernels (rt16sh_forward_kernel / rt16sh_adjoint_kernel: the wind-mixing NDE, RK4, at most 8,192 columns)";
    if (h->closure) return fail("%s: the closure engine (colnde_create_closure) steps with one substeps", only);
    if (h->conv.c) return fail("%s: a conv handle (colnde_create_conv, conv=%d) runs the fc32 engine", only, h->conv.c);
    if (h->use_fc || h->cfg.model != COLNDE_MODEL_WIND_MIXING)
        return fail("%s: %s", only, h->ensemble ? "a free-convection ensemble (colnde_create_fc_ensemble) runs the fc32 engine" : "the free-convection models run the fc32 and tile16 engines");
    if (h->cfg.stepper == COLNDE_STEPPER_RKC2) return fail("a step schedule covers RK4 only: the RKC2 stage table depends on dt");
    if (h->use_rt) return fail("%s: this handle runs regtile (more than 8,192 columns, or engine = regtile)", only);
    if (!rt_supported(h->m))
        return fail("%s: this configuration (network shape, Nz, smoothing or inplace_variant) runs the tile16 engine", only);
    for (EnvSwitch sw : {ENV_T16_FWD_HELPER, ENV_T16_ADJ_HELPER, ENV_T16_FWD_SPLIT, ENV_T16_ADJ_SPLIT, ENV_T16_ZTAPE, ENV_T16_DWTAPE}) {
        const char* e = env_get(sw);
        if (e && atoi(e) == 0) return fail("%s: %s=0 selects the three-wave or tile16 kernels (or no delta / pre-activation tape)", only, env_name(sw));
    }
    if (!h->fwd_split || !h->adj_split || !h->fwd_helper || !h->adj_helper) return fail("%s: this handle's engine selection runs tile16", only);
    return 0;
}

static int upload_schedule(colnde_handle* h, const int* counts) {
    const size_t n_iv = (size_t)h->cfg.n_save - 1;
    HIPCHK(hipSetDevice(h->device));
    if (!h->d_sched && h->mem.alloc(&h->d_sched, n_iv) != hipSuccess) return fail("allocating the step schedule (%zu counts) failed", n_iv);
    // in stream order behind the kernels that still read the previous counts; completed before returning (the caller's array is not kept)
    if (hipMemcpyAsync(h->d_sched, counts, n_iv * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
        return fail("uploading the step schedule failed");
    return 0;
}

// The RK4 steps of every save interval (NULL: back to cfg.substeps everywhere).  Refused once a single handle's tapes are planned — the total sizes
// them; an ensemble's, planned at creation, are planned again — and outside each interval's stability bound.  Clears a pending substeps = 0.
extern "C" int colnde_set_schedule(colnde_handle* h, const int* counts) {
    if (!h) return fail("null handle");
    NOT_A_TILE_ENSEMBLE(h);
    const int n_iv = h->cfg.n_save - 1;
    const char* planned = "the step schedule sizes the tapes: set it before the first colnde_loss_grad of this handle";
    if (!counts) {
        if (h->sched.empty()) return 0;
        if (!h->ensemble && tapes_planned(h)) return fail("%s", planned);
        std::vector<int> keep;
        keep.swap(h->sched);
        if (h->ensemble && ens_replan_tapes(h)) {
            h->sched.swap(keep);
            return 1;
        }
        h->last_estimate = -1.0f;
        h->substeps_chosen = false;
        return 0;
    }
    if (refuse_schedule(h)) return 1;
    if (!h->sched.empty() && std::equal(h->sched.begin(), h->sched.end(), counts)) return 0;
    if (!h->ensemble && tapes_planned(h)) return fail("%s", planned);
    std::vector<int> need;
    if (schedule_minima(h, &need)) return 1;
    int bad = 0;
    switch (sched_validate(counts, need.data(), n_iv, allow_unstable(), &bad)) {
    case SCHED_NOT_POSITIVE: return fail("schedule[%d] = %d: every save interval takes at least one step", bad, counts[bad]);
    case SCHED_ABOVE_MAX: return fail("schedule[%d] = %d is above %d steps per save interval", bad, counts[bad], COLNDE_SCHEDULE_MAX);
    case SCHED_BELOW_MIN:
        return fail("schedule[%d] = %d is outside the stepper's stability bound on save interval %d: need >= %d (colnde_schedule_min; COLNDE_ALLOW_UNSTABLE_DT=1 overrides)",
                    bad, counts[bad], bad, need[bad]);
    case SCHED_OK: break;
    }
    std::vector<int> keep(counts, counts + n_iv);
    if (upload_schedule(h, keep.data())) return 1;
    keep.swap(h->sched);                                   // (keep: the schedule that was in force)
    if (h->ensemble && ens_replan_tapes(h)) {
        const std::string msg = colnde_last_error();
        h->sched.swap(keep);
        if (!h->sched.empty()) (void)upload_schedule(h, h->sched.data());
        (void)ens_replan_tapes(h);
        return fail("%s", msg.c_str());
    }
    h->auto_substeps = false;
    h->substeps_chosen = false;
    h->last_estimate = -1.0f;
    return 0;
}

// counts (nullable) receives the steps of every save interval — cfg.substeps each without a schedule; returns their total, -1 on a null handle
extern "C" int colnde_schedule(const colnde_handle* h, int* counts) {
    if (!h) { fail("null handle"); return -1; }
    if (counts)
        for (int i = 0; i < h->cfg.n_save - 1; i++) counts[i] = h->sched.empty() ? h->cfg.substeps : h->sched[i];
    return total_steps(h);
}

// forward solve under the counts S (uploaded; h->sched is left holding them)
static int forward_scheduled(colnde_handle* h, const float* d_weights, float* d_sol, const std::vector<int>& S) {
    if (upload_schedule(h, S.data())) return 1;
    h->sched = S;
    return forward_impl(h, d_weights, d_sol, false);
}

// The fixed-step form of reltol, interval by interval.  From the stability minima rounded up to powers of two: solve at S and at 2 S (every interval
// doubled), E[n] = the estimate of colnde_error_estimate at save point n alone (max over columns); while max E > reltol, the intervals that add the
// most to it — d[n] = max(0, E[n] - E[n-1]) at least half the largest — are doubled.  Errors are handed from one interval to the next, so E[n] - E[n-1]
// is what interval n adds; a diffusive solve damps what it inherits, hence the clamp at 0.
static int choose_schedule_impl(colnde_handle* h, const float* d_weights, float reltol, int* counts, float* estimate) {
    const int n_iv = h->cfg.n_save - 1, n_save = h->cfg.n_save;
    const size_t n = (size_t)h->n_col * n_save * h->m.ns;
    DevScratch sc(h->stream);
    HIPCHK(sc.alloc((2 * n + (size_t)n_save + 4) * sizeof(float)));
    float *d_a = sc.p, *d_b = sc.p + n, *d_e = sc.p + 2 * n;
    std::vector<int> S;
    if (schedule_minima(h, &S)) return 1;
    for (int& s : S) s = sched_pow2_ceil(s);
    std::vector<float> E((size_t)n_save), d((size_t)n_iv);
    float est = -1.0f, prev = -1.0f;
    for (;;) {
        std::vector<int> S2(S);
        for (int& s : S2) s *= 2;
        if (forward_scheduled(h, d_weights, d_a, S) || forward_scheduled(h, d_weights, d_b, S2)) return 1;
        hipError_t e = launch_rel_diff_save_max(d_a, d_b, h->n_col, n_save, h->m.ns, norm_floor(reltol), d_e, h->stream);
        if (e != hipSuccess) return fail("error-estimate launch failed: %s", hipGetErrorString(e));
        if (hipMemcpyAsync(E.data(), d_e, (size_t)n_save * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
            return fail("choose_schedule: device-to-host copy failed");
        est = 0.0f;
        const int total = (int)sched_total(S.data(), n_iv);
        for (int i = 0; i < n_save; i++) {
            E[i] *= richardson_factor(h);
            if (!(E[i] == E[i]) || E[i] > 3.0e38f) return fail("the solve is not finite under a schedule of %d steps in all: no schedule can be chosen", total);
            est = std::max(est, E[i]);
        }
        if (est <= reltol) break;
        // every interval doubled last round was one of its contributors (that is how they are picked), so an estimate that fell by less than a fifth is the
        // float32 round-off of the two solves it compares, as in colnde_choose_substeps
        if (prev > 0.0f && est > 0.8f * prev)
            return fail("reltol = %g is below the float32 round-off floor of this solve: the estimate stopped falling at %g (%d steps in all, %g before the last doubling)",
                        reltol, est, total, prev);
        prev = est;
        float dmax = 0.0f;
        for (int i = 0; i < n_iv; i++) { d[i] = std::max(0.0f, E[i + 1] - (i ? E[i] : 0.0f)); dmax = std::max(dmax, d[i]); }
        bool doubled = false;
        for (int i = 0; i < n_iv; i++)
            if (d[i] >= 0.5f * dmax && S[i] < COLNDE_SCHEDULE_MAX) { S[i] *= 2; doubled = true; }
        if (!doubled)
            return fail("reltol = %g is not met with %d steps in the save intervals that carry the error (estimate %g): the right-hand side is too stiff for this stepper",
                        reltol, COLNDE_SCHEDULE_MAX, est);
    }
    if (upload_schedule(h, S.data())) return 1;
    h->sched = S;
    h->last_estimate = est;
    h->substeps_chosen = false;
    if (counts) std::copy(S.begin(), S.end(), counts);
    if (estimate) *estimate = est;
    return 0;
}

extern "C" int colnde_choose_schedule(colnde_handle* h, const float* weights, float reltol, int* counts, float* estimate) {
    SINGLE_MODEL_ONLY(h);
    if (!h) return fail("null handle");
    if (!weights) return fail("null weights");
    if (refuse_schedule(h)) return 1;
    if (!h->have_problem) return fail("colnde_set_problem has not been called");
    if (refuse_auto_on_a_shard(h)) return 1;
    if (tapes_planned(h)) return fail("the step schedule sizes the tapes: choose it before the first colnde_loss_grad of this handle");
    if (reltol == 0.0f) reltol = h->cfg.reltol;
    if (!(reltol > 0.0f)) return fail("reltol must be > 0");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * h->m.n_params, hipMemcpyHostToDevice, h->stream));
    const std::vector<int> keep = h->sched;
    const bool au = h->auto_substeps;
    h->auto_substeps = false;
    if (choose_schedule_impl(h, h->d_w, reltol, counts, estimate)) {
        const std::string msg = colnde_last_error();
        h->sched = keep;
        h->auto_substeps = au;
        if (!keep.empty()) (void)upload_schedule(h, keep.data());
        return fail("%s", msg.c_str());
    }
    return 0;
}

// ---- ensembles: the estimate member by member, one schedule chosen for all K ------------------------------------------------------------
// A net-split ensemble steps all K members by one schedule; its members differ in what decides the step (the closure constants, the weights).  The
// estimate is colnde_error_estimate's, with the member kept: two tape-less ensemble solves (the model index in the launch grid) into scratch and
// rel_diff_member_save_max_kernel, out[k][n].  The solves run under counts that live in the call's scratch: the handle's schedule, its device copy
// and its tapes are not written, so what is in force afterwards is what was in force before, on failure too.

// refused before any device work, each reason with the entry point's name
static int ens_estimate_refusals(const colnde_handle* h, const char* fn) {
    if (!h) return fail("%s: null handle", fn);
    if (h->closure) return fail("%s estimates the solves of networks, but this is a closure handle (colnde_create_closure: no networks, %d constant sets)", fn, h->n_models);
    if (!h->ensemble)
        return fail("%s takes the handles of colnde_create_ensemble, colnde_create_tile_ensemble and colnde_create_fc_ensemble: a single handle's estimate is "
                    "colnde_error_estimate", fn);
    if (h->conv.c)
        return fail("%s does not cover the convolutional first layer of a colnde_create_conv_ensemble handle (conv=%d): colnde_error_estimate refuses conv handles too", fn, h->conv.c);
    if (!h->have_problem) return fail("%s: colnde_set_problem has not been called", fn);
    if (refuse_auto_on_a_shard(h)) {
        const std::string msg = colnde_last_error();
        return fail("%s: %s", fn, msg.c_str());
    }
    return 0;
}

// the RKC2 stage count of an ensemble whose stages follow the step (cfg.rkc_stages = 0), at `substeps`: the largest any member needs, as at creation
static int ens_stages_at(const colnde_handle* h, int substeps) {
    if (h->cfg.stepper != COLNDE_STEPPER_RKC2 || h->cfg.rkc_stages || !h->ens_rkc_stages) return h->ens_rkc_stages;
    colnde_config c = h->cfg;
    c.substeps = substeps;
    int stages = 0;
    for (int k = 0; k < h->n_models; k++) {
        const colnde_config ck = model_config(&c, h->phys_raw.empty() ? nullptr : h->phys_raw.data(), k);
        stages = std::max(stages, colnde_rkc_stages(&ck));
    }
    return stages;
}

// what a round changes in the handle, put back by restore(): the sub-step count, the RKC2 stage count and table, the schedule and where the launches read it
struct EnsStepKeep {
    colnde_handle* h;
    int substeps, stages;
    std::vector<int> sched;
    int* d_sched;
    bool done = false;
    explicit EnsStepKeep(colnde_handle* h_) : h(h_), substeps(h_->cfg.substeps), stages(h_->ens_rkc_stages), sched(h_->sched), d_sched(h_->d_sched) {}
    EnsStepKeep(const EnsStepKeep&) = delete;
    ~EnsStepKeep() { if (!done) (void)restore(); }           // (a path that leaves without restore(): the handle never keeps a pointer into freed scratch)
    int restore() {
        done = true;
        h->cfg.substeps = substeps;
        h->ens_rkc_stages = stages;
        h->sched = sched;
        h->d_sched = d_sched;
        return refresh_rkc(h);
    }
};

// Tape-less solve of all K members into d_sol.  S: the counts of every interval, already on the device at d_S (scratch); null: `substeps` everywhere.
static int ens_solve_under(colnde_handle* h, const float* d_weights, float* d_sol, const std::vector<int>* S, int* d_S, int substeps) {
    if (S) {
        h->sched = *S;
        h->d_sched = d_S;
    } else {
        h->sched.clear();
        h->ens_rkc_stages = ens_stages_at(h, substeps);
        h->cfg.substeps = substeps;
        if (refresh_rkc(h)) return 1;
    }
    return colnde_ensemble_forward_dev(h, d_weights, d_sol);
}

// the scratch of the two calls: two solutions of all K members, the estimates, and the counts of a round and their doubles — on the device and on the host,
// where they outlive the copies queued from them (members are destroyed after `sc`, whose destructor drains the stream)
struct EnsScratch {
    std::vector<int> at, at2;
    DevScratch sc;
    float *d_a = nullptr, *d_b = nullptr, *d_est = nullptr;
    int* d_S = nullptr;
    explicit EnsScratch(hipStream_t s) : sc(s) {}
    int alloc(const colnde_handle* h) {
        const size_t n = ((size_t)h->n_models * h->n_col * h->cfg.n_save * h->m.ns + 3) / 4 * 4, ne = ((size_t)h->n_models * h->cfg.n_save + 3) / 4 * 4;
        HIPCHK(sc.alloc((2 * n + ne) * sizeof(float) + 2 * (size_t)h->cfg.n_save * sizeof(int)));
        d_a = sc.p;
        d_b = sc.p + n;
        d_est = sc.p + 2 * n;
        d_S = reinterpret_cast<int*>(sc.p + 2 * n + ne);
        return 0;
    }
};

// One round into s.d_est [K][n_save] (Richardson's factor not applied): the solve under S (null: `substeps` everywhere) against every interval doubled
static int ens_estimate_round(colnde_handle* h, const float* d_weights, const std::vector<int>* S, int substeps, float floor_, EnsScratch& s) {
    const int n_iv = h->cfg.n_save - 1;
    if (S) {
        s.at = *S;
        s.at2 = *S;
        for (int& c : s.at2) c *= 2;
        if (hipMemcpyAsync(s.d_S, s.at.data(), (size_t)n_iv * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemcpyAsync(s.d_S + n_iv, s.at2.data(), (size_t)n_iv * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess)
            return fail("uploading the round's step counts failed");
    }
    if (ens_solve_under(h, d_weights, s.d_a, S ? &s.at : nullptr, s.d_S, substeps) || ens_solve_under(h, d_weights, s.d_b, S ? &s.at2 : nullptr, s.d_S + n_iv, 2 * substeps))
        return 1;
    const hipError_t e = launch_rel_diff_member_save_max(s.d_a, s.d_b, h->n_models, h->n_col, h->cfg.n_save, h->m.ns, floor_, s.d_est, h->stream);
    if (e != hipSuccess) return fail("error-estimate launch failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int colnde_ensemble_error_estimate_dev(colnde_handle* h, const float* d_weights, float* estimates) {
    if (!h) return fail("%s: null handle", __func__);
    if (!d_weights || !estimates) return fail("%s: null pointer argument", __func__);
    if (ens_estimate_refusals(h, __func__)) return 1;
    HIPCHK(hipSetDevice(h->device));
    EnsScratch s(h->stream);
    if (s.alloc(h)) return 1;
    const size_t ne = (size_t)h->n_models * h->cfg.n_save;
    EnsStepKeep keep(h);
    int rc = ens_estimate_round(h, d_weights, keep.sched.empty() ? nullptr : &keep.sched, keep.substeps, norm_floor(h->cfg.reltol), s);
    if (!rc && (hipMemcpyAsync(estimates, s.d_est, ne * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess))
        rc = fail("%s: device-to-host copy failed", __func__);
    const std::string msg = rc ? colnde_last_error() : "";
    if (keep.restore()) return 1;
    if (rc) return fail("%s", msg.c_str());
    const float factor = richardson_factor(h);
    for (size_t i = 0; i < ne; i++) estimates[i] *= factor;
    return 0;
}

extern "C" int colnde_ensemble_error_estimate(colnde_handle* h, const float* weights, float* estimates) {
    if (!h) return fail("%s: null handle", __func__);
    if (!weights || !estimates) return fail("%s: null pointer argument", __func__);
    if (ens_estimate_refusals(h, __func__)) return 1;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * (size_t)h->n_models * user_params(h), hipMemcpyHostToDevice, h->stream));
    return colnde_ensemble_error_estimate_dev(h, h->d_w, estimates);
}

// colnde_choose_schedule's greedy run with E[n] = the maximum over the members (step_schedule.h: sched_choose_round); on success S holds the schedule,
// member_est [K] every member's own maximum over the save points at it
static int ens_choose_rounds(colnde_handle* h, const float* d_weights, float reltol, EnsScratch& s, std::vector<int>& S, std::vector<float>& member_est, float* est_out) {
    const int K = h->n_models, n_save = h->cfg.n_save;
    if (schedule_minima(h, &S)) return 1;
    for (int& c : S) c = sched_pow2_ceil(c);
    std::vector<float> est((size_t)K * n_save), E((size_t)n_save);
    const float factor = richardson_factor(h);
    float prev = -1.0f;
    for (;;) {
        if (ens_estimate_round(h, d_weights, &S, 0, norm_floor(reltol), s)) return 1;
        if (hipMemcpyAsync(est.data(), s.d_est, est.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
            return fail("colnde_ensemble_choose_schedule: device-to-host copy failed");
        const int total = (int)sched_total(S.data(), n_save - 1);
        std::fill(E.begin(), E.end(), 0.0f);
        for (int k = 0; k < K; k++) {
            member_est[(size_t)k] = 0.0f;
            for (int n = 0; n < n_save; n++) {
                const float e = est[(size_t)k * n_save + n] * factor;
                if (!(e == e) || e > 3.0e38f)
                    return fail("the solve of member %d is not finite under a schedule of %d steps in all: no schedule can be chosen", k, total);
                E[(size_t)n] = std::max(E[(size_t)n], e);
                member_est[(size_t)k] = std::max(member_est[(size_t)k], e);
            }
        }
        float mx = 0.0f;
        switch (sched_choose_round(E.data(), n_save, reltol, prev, S.data(), &mx)) {
        case SCHED_ROUND_MET: *est_out = mx; return 0;
        case SCHED_ROUND_DOUBLED: prev = mx; break;
        // (not reached: the loop above has named the member; kept so that the switch covers the rule's verdicts)
        case SCHED_ROUND_NOT_FINITE: return fail("the solve is not finite under a schedule of %d steps in all: no schedule can be chosen", total);
        case SCHED_ROUND_FLOOR:
            return fail("reltol = %g is below the float32 round-off floor of this solve: the estimate stopped falling at %g (%d steps in all, %g before the last doubling)",
                        reltol, mx, total, prev);
        case SCHED_ROUND_TOO_STIFF:
            return fail("reltol = %g is not met with %d steps in the save intervals that carry the error (estimate %g): the right-hand side is too stiff for this stepper",
                        reltol, COLNDE_SCHEDULE_MAX, mx);
        }
    }
}

extern "C" int colnde_ensemble_choose_schedule(colnde_handle* h, const float* weights, float reltol, int* counts, float* estimates) {
    if (!h) return fail("%s: null handle", __func__);
    if (!weights) return fail("%s: null weights", __func__);
    NOT_A_TILE_ENSEMBLE(h);
    if (h->closure || !h->ensemble) {
        if (refuse_schedule(h)) return 1;                    // (a closure handle: its own reason)
        return fail("%s takes the handles of colnde_create_ensemble: a single handle's schedule is chosen by colnde_choose_schedule", __func__);
    }
    if (refuse_schedule(h)) return 1;
    if (ens_estimate_refusals(h, __func__)) return 1;
    if (reltol == 0.0f) reltol = h->cfg.reltol;
    if (!(reltol > 0.0f)) return fail("%s: reltol must be > 0", __func__);
    HIPCHK(hipSetDevice(h->device));
    const int K = h->n_models, n_iv = h->cfg.n_save - 1;
    std::vector<int> S;
    std::vector<float> member_est((size_t)K);
    float est = -1.0f;
    {
        EnsScratch s(h->stream);
        if (s.alloc(h)) return 1;
        HIPCHK(hipMemcpyAsync(h->d_w, weights, sizeof(float) * (size_t)K * user_params(h), hipMemcpyHostToDevice, h->stream));
        EnsStepKeep keep(h);
        const int rc = ens_choose_rounds(h, h->d_w, reltol, s, S, member_est, &est);
        (void)hipStreamSynchronize(h->stream);
        const std::string msg = rc ? colnde_last_error() : "";
        if (keep.restore()) return 1;
        if (rc) return fail("%s", msg.c_str());
    }                                                        // (the scratch is freed before the tapes are planned again)
    // the handle keeps the schedule: colnde_set_schedule's own steps (validation, upload, the tapes planned again; a total that does not fit is refused with
    // the bytes and the previous schedule and tapes kept)
    if (colnde_set_schedule(h, S.data())) return 1;
    h->last_estimate = est;
    if (counts) std::copy(S.begin(), S.begin() + n_iv, counts);
    if (estimates) std::copy(member_est.begin(), member_est.end(), estimates);
    return 0;
}
