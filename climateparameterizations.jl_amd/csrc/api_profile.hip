// api_profile.hip — colnde_ensemble_profile[_dev]: judging the K members of a wind-mixing sweep on given solutions (NDE_profile,
// wind_mixing/src/training_postprocessing.jl:250-632): the face fluxes and the Richardson number of every saved state in one launch
// (engine_wm_profile.hip) and the six loss_per_tstep series of every member in another (column_ops.hip).  Nothing is solved here.
#include "api_internal.h"

// what the call refuses wherever the arrays live; host: the host twin's arrays (no alignment rule of their own)
static int profile_check(colnde_handle* h, const char* fn, const float* weights, const float* sol, const float* physics, const float* uw, const float* vw,
                         const float* wT, const float* Ri, const float* losses, bool host) {
    if (!h) return fail("%s: null handle", fn);
    if (h->closure) return fail("%s takes K weight vectors, but this is a closure handle (no networks, %d constant sets): use colnde_closure_* (include/colnde.h)", fn, h->n_models);
    if (!h->ensemble)
        return fail("%s takes the handles of colnde_create_ensemble (K = 1 for one model): this is a single-model handle (colnde_flux and colnde_loss_per_tstep "
                    "diagnose one model)", fn);
    if (h->use_fc)
        return fail("%s covers wind-mixing ensembles: this ensemble holds free-convection models%s (colnde_ensemble_column_loss_dev judges those)", fn,
                    h->conv.c ? " behind a convolutional first layer" : "");
    if (!weights || !sol) return fail("%s: null pointer argument (weights and sol are required)", fn);
    const int n_flux = (uw != nullptr) + (vw != nullptr) + (wT != nullptr);
    if (n_flux != 0 && n_flux != 3) return fail("%s: uw, vw, wT are one output group — all three given or all three NULL; %d of 3 given", fn, n_flux);
    if (!n_flux && !Ri && !losses) return fail("%s: no outputs — give the flux group (uw, vw, wT), Ri or losses", fn);
    if (!h->have_problem) return fail("%s: colnde_set_problem has not been called (the boundary fluxes of the simulations come from it)", fn);
    if (losses && !h->have_truth) return fail("%s: losses need truth trajectories: pass truth to colnde_set_problem", fn);
    if (physics) {
        if (!h->cfg.modified_pacanowski_philander)
            return fail("%s: a physics array needs modified_pacanowski_philander = 1: without the Richardson-number closure the five constants are unused (pass NULL)", fn);
        for (int k = 0; k < h->n_models; k++) {
            const float* r = physics + (size_t)5 * k;
            for (int q = 0; q < 5; q++)
                if (!std::isfinite(r[q])) return fail("%s: physics[%d][%d] = %g is not finite", fn, k, q, r[q]);
            if (!(r[2] > 0.0f) || !(r[4] > 0.0f)) return fail("%s: physics[%d]: dRi = %g and Pr = %g must be > 0", fn, k, r[2], r[4]);
        }
    }
    if (!host) {
        const void* const ptrs[6] = {sol, uw, vw, wT, Ri, losses};
        for (const void* p : ptrs)
            if ((uintptr_t)p & 15) return fail("%s: the base pointers of sol and of the outputs must be 16-byte aligned", fn);
    }
    return 0;
}

static int profile_grid_cap() {
    const char* e = env_get(ENV_WM_PROFILE_GRID);      // test override: at most this many workgroups (several models per workgroup at small K)
    return e && *e ? std::max(0, atoi(e)) : 0;
}

extern "C" int colnde_ensemble_profile_dev(colnde_handle* h, const float* d_weights, const float* d_sol, const float* physics, float* d_uw, float* d_vw,
                                           float* d_wT, float* d_Ri, float* d_losses) {
    NOT_A_TILE_ENSEMBLE(h);
    if (profile_check(h, __func__, d_weights, d_sol, physics, d_uw, d_vw, d_wT, d_Ri, d_losses, false)) return 1;
    HIPCHK(hipSetDevice(h->device));
    const int K = h->n_models;
    if (d_uw || d_Ri) {
        const RtPhys* d_phys = h->d_phys;
        if (physics) {                                  // this call's constants: no stability check, nothing is integrated
            std::vector<RtPhys> ph((size_t)K);
            for (int k = 0; k < K; k++) {
                const float* r = physics + (size_t)5 * k;
                ph[k] = closure_constants(r[0], r[1], r[2], r[3], r[4]);
            }
            if (!h->d_prof_phys) HIPCHK(h->mem.alloc(&h->d_prof_phys, (size_t)K));
            // (a kernel in flight on the stream may still read the previous table: the copy is ordered on the stream and completed before returning)
            HIPCHK(hipMemcpyAsync(h->d_prof_phys, ph.data(), ph.size() * sizeof(RtPhys), hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            d_phys = h->d_prof_phys;
        }
        WmProfileArgs a = {};
        a.m = h->m;
        a.n_models = K; a.weights = d_weights; a.w_stride = (size_t)h->m.n_params;
        a.sol = d_sol; a.bcs = h->d_bcs; a.save_times = h->d_times; a.phys = d_phys;
        a.n_col = h->n_col; a.n_save = h->cfg.n_save;
        a.uw = d_uw; a.vw = d_vw; a.wT = d_wT; a.Ri = d_Ri;
        a.grid_cap = profile_grid_cap();
        Timed tm(h, K_PROFILE);
        hipError_t e = launch_wm_profile_ens(a, h->stream);
        if (e != hipSuccess) return fail("%s launch failed: %s", __func__, hipGetErrorString(e));
    }
    if (d_losses) {
        Timed tm(h, K_REDUCE);
        hipError_t e = launch_loss_per_tstep(d_sol, h->d_truth, h->n_col, h->cfg.n_save, h->m.Nz, h->m.ns / h->m.Nz, d_losses, h->stream, K);
        if (e != hipSuccess) return fail("%s: loss_per_tstep launch failed: %s", __func__, hipGetErrorString(e));
    }
    return 0;
}

extern "C" int colnde_ensemble_profile(colnde_handle* h, const float* weights, const float* sol, const float* physics, float* uw, float* vw, float* wT,
                                       float* Ri, float* losses) {
    NOT_A_TILE_ENSEMBLE(h);
    if (profile_check(h, __func__, weights, sol, physics, uw, vw, wT, Ri, losses, true)) return 1;
    HIPCHK(hipSetDevice(h->device));
    const size_t K = (size_t)h->n_models, states = (size_t)h->n_col * h->cfg.n_save;
    float *d_sol, *d_uw, *d_vw, *d_wT, *d_Ri, *d_losses;
    HostStage st(h, __func__);
    st.to(h->d_w, weights, K * h->m.n_params);
    st.in(&d_sol, sol, K * states * h->m.ns);
    st.out(&d_uw, uw, K * states * (WM_NZ + 1));
    st.out(&d_vw, vw, K * states * (WM_NZ + 1));
    st.out(&d_wT, wT, K * states * (WM_NZ + 1));
    st.out(&d_Ri, Ri, K * states * (WM_NZ + 1));
    st.out(&d_losses, losses, K * h->n_col * 6 * h->cfg.n_save);
    if (st.upload()) return 1;
    if (colnde_ensemble_profile_dev(h, h->d_w, d_sol, physics, d_uw, d_vw, d_wT, d_Ri, d_losses)) return 1;
    return st.download();
}
