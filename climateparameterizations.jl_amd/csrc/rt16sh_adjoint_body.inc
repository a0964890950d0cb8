// The body of rt16sh_adjoint_kernel and rt16sh_adjoint_sched_kernel (engine_netsplit.hip, which describes it): RT16SH_SCHED = 1 reads the steps of each save
// interval from sched[] and sizes the tapes by total_steps, 0 takes `substeps` everywhere.
// RT16SH_MEMBER = 1 (rt16sh_adjoint_member_kernel and its scheduled twin: the member loss of an ensemble, colnde_ensemble_set_member_loss): the loss
// weights are the member's own, lwk[blockIdx.y], and every column carries the member's weight colw[blockIdx.y][column] into the injection and the six
// sums.  0 compiles the text as it was.
    // ensembles: blockIdx.y = model — its weight image, solution, tapes, slab rows and closure constants (truth shared); grid.y = 1: one model
    wimg += (size_t)blockIdx.y * ens.wimg;
    sol += (size_t)blockIdx.y * ens.sol;
    t16_tape += (size_t)blockIdx.y * ens.tape;
    t16_ztape += (size_t)blockIdx.y * ens.ztape;
    slab += (size_t)blockIdx.y * ens.slab;
    dwtape += (size_t)blockIdx.y * ens.dwtape;
    const RtPhys ph = ens.phys ? ens.phys[blockIdx.y] : rt_phys_of(m);
#if RT16SH_MEMBER
    const LossWeights lw = lwk[blockIdx.y];                             // wave-uniform: the member's own weights
#endif
    // SPLIT: LDS holds the fp32 image from W2 on (addressed through wl as before: wl[RT_W2C + x]), no fp32 W1
    constexpr int IMG0 = SPLIT ? RT_W2C : 0;
    constexpr int IMGF = ((RT_IMG_FLOATS - IMG0) + 3) & ~3;
    float* wl = rt_smem - IMG0;
    for (int e = IMG0 + threadIdx.x; e < RT_IMG_FLOATS; e += 256) wl[e] = wimg[e];
    float* lbase = rt_smem + IMGF;
    f32x4v* ex = reinterpret_cast<f32x4v*>(lbase);                    // the nets' parts of x̄: [3 nets][6 tiles][64 lanes]
    f32x4v* dOl = ex + 3 * 6 * 64;                                     // the helper's dO: [3 variables][2 tiles][64 lanes]
    float* stg_all = lbase + (3 * 6 * 64 + 3 * 2 * 64) * 4;           // record staging: see rt16s_adjoint_kernel
    for (int e = threadIdx.x; e < 3 * RT16S_STG; e += 256) stg_all[e] = 0.0f;
    const u32x4* hm = reinterpret_cast<const u32x4*>(stg_all + 3 * RT16S_STG);      // SPLIT: [net][kb][tile][h, m][64 lanes] operand planes
    if constexpr (SPLIT) {
        const u32x4* src = reinterpret_cast<const u32x4*>(wimg + RT_NSA_OFF);
        u32x4* dst = reinterpret_cast<u32x4*>(stg_all + 3 * RT16S_STG);
        for (int e = threadIdx.x; e < RT_NSA_HM_WORDS / 4; e += 256) dst[e] = src[e];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool helper = role == 3;
    const int n = helper ? 0 : role;                                    // the net of a net wave
    const int j = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x;
    const int col = tile * 16 + j;
    const bool valid = col < n_col;
    const int colc = min(col, n_col - 1);
#if RT16SH_SCHED
    const int n_steps = total_steps;
#else
    const int n_steps = (n_save - 1) * substeps;
#endif
    const int nst = RKC ? m.nst : 4;                                    // RHS evaluations (= tape records) per step: 4 (RK4) or s (RKC2)
    constexpr bool rkc = RKC;
    const float* tp = t16_tape + (size_t)tile * n_steps * nst * 1536 + j * 96 + 4 * g;
    const bool phys = m.mpp || m.ca;
    float* out = slab + (size_t)tile * (m.n_params + 8);

    if (helper) {
        // ================================================= the helper wave: λ, x̄, loss injection, physics pullback ======================
        const float* tzr = t16_ztape + (size_t)tile * n_steps * nst * RT16S_RREC + lane * 4;             // RICH: the rich tape
        V16 lam[3], xb[3], xbs[3];
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int tau = 0; tau < 2; tau++) { lam[q].t[tau] = (f32x4t)(0.0f); xb[q].t[tau] = (f32x4t)(0.0f); xbs[q].t[tau] = (f32x4t)(0.0f); }
        float sum_d[3] = {0.0f, 0.0f, 0.0f}, sum_g[3] = {0.0f, 0.0f, 0.0f};
#if RT16SH_MEMBER
        // the member's weight of this lane's column, loaded once: cw d is formed first and carries the weight into the injection (linear in d), the
        // six sums take (cw d) d — a weight of 1 reproduces the unweighted operations exactly, a weight of 0 injects exact zeros
        const float cw = valid ? colw[(size_t)blockIdx.y * n_col + colc] : 0.0f;
#endif
        auto inject = [&](int sv, bool add) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                V16 d;
#pragma unroll
                for (int tau = 0; tau < 2; tau++) {
                    const size_t o = ((size_t)colc * n_save + sv) * 96 + q * 32 + 16 * tau + 4 * g;
                    const f32x4v a = *reinterpret_cast<const f32x4v*>(sol + o);
                    const f32x4v b = *reinterpret_cast<const f32x4v*>(truth + o);
#pragma unroll
                    for (int e = 0; e < 4; e++) d.t[tau][e] = valid ? a[e] - b[e] : 0.0f;
                }
#if RT16SH_MEMBER
                V16 dw;                                                  // cw d
#pragma unroll
                for (int tau = 0; tau < 2; tau++)
#pragma unroll
                    for (int e = 0; e < 4; e++) dw.t[tau][e] = cw * d.t[tau][e];
                const V16 dd = shift_down16(d, lane, 0.0f), ddw = shift_down16(dw, lane, 0.0f);
                V16 gg;                                                  // the gradient of cw d: what is injected
#pragma unroll
                for (int tau = 0; tau < 2; tau++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const bool top = tau == 0 && r == 0 && g == 0;
                        const float gu = top ? 0.0f : (d.t[tau][r] - dd.t[tau][r]) * 32.0f;
                        gg.t[tau][r] = top ? 0.0f : (dw.t[tau][r] - ddw.t[tau][r]) * 32.0f;
                        sum_d[q] += dw.t[tau][r] * d.t[tau][r];
                        sum_g[q] += gg.t[tau][r] * gu;
                    }
                d = dw;
#else
                const V16 dd = shift_down16(d, lane, 0.0f);
                V16 gg;
#pragma unroll
                for (int tau = 0; tau < 2; tau++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        gg.t[tau][r] = (tau == 0 && r == 0 && g == 0) ? 0.0f : (d.t[tau][r] - dd.t[tau][r]) * 32.0f;
                        sum_d[q] += d.t[tau][r] * d.t[tau][r];
                        sum_g[q] += gg.t[tau][r] * gg.t[tau][r];
                    }
#endif
                if (add) {
                    const V16 gu_ = shift_up16(gg, lane, 0.0f);
#pragma unroll
                    for (int tau = 0; tau < 2; tau++)
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            lam[q].t[tau][r] += 2.0f * lw.w[q] * d.t[tau][r] + 2.0f * lw.w[3 + q] * 32.0f * (gg.t[tau][r] - gu_.t[tau][r]);
                }
            }
        };
        // what the pullback reads from the tapes, one stage ahead: RICH the nine coefficients, otherwise the stage input
        PhysC Pp;
        V16 Xp[3];
        auto prefetch = [&](int qs) __attribute__((always_inline)) {
            if (RICH) {
                if (phys) {
                    const float* sr = tzr + (size_t)qs * RT16S_RREC;
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) {
                        Pp.dn0.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 0 + tau) * 256);
                        Pp.dn1.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 2 + tau) * 256);
                        Pp.dn2.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 4 + tau) * 256);
                        Pp.nu0.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 6 + tau) * 256);
                        Pp.nu1.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 8 + tau) * 256);
                        Pp.nu2.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 10 + tau) * 256);
                        Pp.c0.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 12 + tau) * 256);
                        Pp.c1.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 14 + tau) * 256);
                        Pp.c2.t[tau] = *reinterpret_cast<const f32x4v*>(sr + (36 + 16 + tau) * 256);
                    }
                }
            } else {
                const float* sx = tp + (size_t)qs * 1536;
#pragma unroll
                for (int q = 0; q < 3; q++)
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) Xp[q].t[tau] = *reinterpret_cast<const f32x4v*>(sx + q * 32 + 16 * tau);
            }
        };
        // RKC2 (discrete adjoint of the recurrence, as in tile16's adjoint_kernel): cotangents of Y_{j-1} (yb1), Y_{j-2} (yb2), Y_0 (yb0), F_0 (f0b);
        // lam is the cotangent of Y_j.  The convective-adjustment switch is pulled back with ONE pattern per step, that of Y_{s-1} (DESIGN §2):
        // the physics data of every stage of a step are then read from the record of its last stage.
        V16 yb0[3], yb1[3], yb2[3], f0b[3];
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int tau = 0; tau < 2; tau++) { yb0[q].t[tau] = (f32x4t)(0.0f); yb1[q].t[tau] = (f32x4t)(0.0f); yb2[q].t[tau] = (f32x4t)(0.0f); f0b[q].t[tau] = (f32x4t)(0.0f); }
        const float* mu_t = m.rkc, *nu_t = m.rkc + RKC_LD, *mut_t = m.rkc + 2 * RKC_LD, *gat_t = m.rkc + 3 * RKC_LD, *kap_t = m.rkc + 5 * RKC_LD;
        const bool one_pattern = rkc && m.ca && !m.mpp;
#define PHYS_Q(q) (one_pattern ? ((q) / nst) * nst + nst - 1 : (q))
        inject(0, false);
        prefetch(PHYS_Q(n_steps * nst - 1));
#if RT16SH_SCHED
        int step0 = n_steps;                                             // the running step index at which interval iv begins
#endif
        for (int iv = n_save - 2; iv >= 0; iv--) {
#if RT16SH_SCHED
            substeps = sched[iv];
            step0 -= substeps;
#endif
            const float dt = (save_times[iv + 1] - save_times[iv]) / (float)substeps;
            inject(iv + 1, true);
            for (int s = substeps - 1; s >= 0; s--) {
#if RT16SH_SCHED
                const int step = step0 + s;
#else
                const int step = iv * substeps + s;
#endif
#pragma nounroll
                for (int st = nst - 1; st >= 0; st--) {
                    const float cwl = (st == 0 || st == 3) ? dt / 6.0f : dt / 3.0f;
                    const float cwx = st == 3 ? 0.0f : (st == 2 ? dt : 0.5f * dt);
                    const int qs = step * nst + st;
                    V16 kb[3], xbp[3];
                    if (rkc) {
                        // stage input Y_st feeds Y_j, j = st + 1, through mu~_j h F_st
                        const float cmu = mu_t[st + 1], cnu = nu_t[st + 1], cmt = mut_t[st + 1] * dt, cga = gat_t[st + 1] * dt, ck0 = kap_t[st + 1];
#pragma unroll
                        for (int q = 0; q < 3; q++)
#pragma unroll
                            for (int tau = 0; tau < 2; tau++) {
                                if (st < nst - 1) {        // lam = cotangent of Y_j, complete once the previous pullback (xb: J(Y_j)^T F̄_j) is added
                                    lam[q].t[tau] = yb1[q].t[tau] + xb[q].t[tau];
                                    yb1[q].t[tau] = yb2[q].t[tau];
                                    yb2[q].t[tau] = (f32x4t)(0.0f);
                                }
                                if (st >= 1) {
                                    yb0[q].t[tau] += ck0 * lam[q].t[tau];
                                    yb1[q].t[tau] += cmu * lam[q].t[tau];
                                    yb2[q].t[tau] += cnu * lam[q].t[tau];
                                    f0b[q].t[tau] += cga * lam[q].t[tau];
                                    kb[q].t[tau] = cmt * lam[q].t[tau];
                                } else {                   // Y_1 = Y_0 + mu~_1 h F_0: lam holds Ȳ_1, yb1 the nu_2 part of Ȳ_0
                                    yb0[q].t[tau] += lam[q].t[tau] + yb1[q].t[tau];
                                    kb[q].t[tau] = f0b[q].t[tau] + cmt * lam[q].t[tau];
                                    yb1[q].t[tau] = (f32x4t)(0.0f);
                                    f0b[q].t[tau] = (f32x4t)(0.0f);
                                }
                            }
                    } else {
#pragma unroll
                    for (int q = 0; q < 3; q++)
#pragma unroll
                        for (int tau = 0; tau < 2; tau++) kb[q].t[tau] = cwl * lam[q].t[tau] + cwx * xb[q].t[tau];
                    }
                    if (RICH) {
                        rt16_physics_apply(m, Pp, kb, lane, xbp);                        // kb now holds dO
                        if (qs > 0) prefetch(PHYS_Q(qs - 1));
                    } else {
                        V16 X[3];
#pragma unroll
                        for (int q = 0; q < 3; q++) X[q] = Xp[q];
                        if (qs > 0) prefetch(PHYS_Q(qs - 1));
                        rt16_physics_vjp(m, ph, X, kb, lane, xbp);
                    }
#pragma unroll
                    for (int q = 0; q < 3; q++)
#pragma unroll
                        for (int tau = 0; tau < 2; tau++) dOl[(q * 2 + tau) * 64 + lane] = kb[q].t[tau];
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // (B) dO is in LDS
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // (A) the nets' parts of x̄ are in LDS
#pragma unroll
                    for (int q = 0; q < 3; q++)
#pragma unroll
                        for (int tau = 0; tau < 2; tau++) {
                            const f32x4v c0 = ex[(0 * 6 + q * 2 + tau) * 64 + lane], c1 = ex[(1 * 6 + q * 2 + tau) * 64 + lane],
                                         c2 = ex[(2 * 6 + q * 2 + tau) * 64 + lane];
                            xb[q].t[tau] = xbp[q].t[tau] + ((c0 + c1) + c2);
                            xbs[q].t[tau] += xb[q].t[tau];
                        }
                }
                // RK4: λ_n = λ_{n+1} + x̄_1 + x̄_2 + x̄_3 + x̄_4;  RKC2: λ_n = Ȳ_0 + J(Y_0)^T F̄_0
#pragma unroll
                for (int q = 0; q < 3; q++)
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) {
                        if (rkc) { lam[q].t[tau] = yb0[q].t[tau] + xb[q].t[tau]; yb0[q].t[tau] = (f32x4t)(0.0f); }
                        else lam[q].t[tau] += xbs[q].t[tau];
                        xbs[q].t[tau] = (f32x4t)(0.0f);
                    }
            }
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            float sd = sum_d[q], sg = sum_g[q];
            for (int off = 32; off > 0; off >>= 1) { sd += __shfl_down(sd, off); sg += __shfl_down(sg, off); }
            if (lane == 0) { out[m.n_params + q] = sd; out[m.n_params + 3 + q] = sg; }
        }
        if (lane == 0) { out[m.n_params + 6] = 0.0f; out[m.n_params + 7] = 0.0f; }
        return;
    }

    // ===================================================== the three net waves ========================================================
    float* stg = stg_all + n * RT16S_STG;
    const int i_ = lane & 15, g_i = i_ >> 2, r_i = i_ & 3;
    int b3T[2], b2T[4];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int Q2 = 4 * u + r_i;
        b3T[u] = RT_W3C + (n * 31 + 4 * g - 1) * RT_LD3 + (Q2 < 5 ? 4 * Q2 + g_i : 20);
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int Q = 4 * t + r_i, f = 4 * Q + g_i;
        b2T[t] = RT_W2C + (n * 20 + g) * RT_LD2 + ((Q < 13 && f < 50) ? f : 50);
    }
    const int b1T = RT_W1C + (n * 50 + g) * RT_LD1 + i_;
    f32x4t gb1[4], gb2[2], gb3[2];                         // bias gradients: this lane's column of every delta, summed over the stages
#pragma unroll
    for (int t = 0; t < 4; t++) gb1[t] = (f32x4t)(0.0f);
#pragma unroll
    for (int u = 0; u < 2; u++) { gb2[u] = (f32x4t)(0.0f); gb3[u] = (f32x4t)(0.0f); }
    const float* tz = RICH ? t16_ztape + (size_t)tile * n_steps * nst * RT16S_RREC + lane * 4
                           : t16_ztape + (size_t)tile * n_steps * nst * RT16S_ZREC + j * 216 + n * 72 + g;
    float* rec0 = dwtape + (size_t)tile * n_steps * nst * RT16S_REC;
    int stg_rd[11], rec_wr[11];
#pragma unroll
    for (int i = 0; i < 11; i++) {
        const int e = 64 * i + lane, c = e / 44, f4 = e - 44 * c;
        stg_rd[i] = c * 180 + 4 * f4;
        rec_wr[i] = c * 720 + 96 + (f4 < 18 ? n * 104 + 4 * f4 : (3 + n) * 104 + 4 * (f4 - 18));
    }
    float* sw = stg + j * 180 + g;
    // this net's tape data, one stage ahead: variable n of the stage input, and the activations with their derivatives (RICH) or the
    // pre-activations they are evaluated from
    V16 Xnp;
    float z1p[13], z2p[5];
    f32x4t adp[12];
    auto prefetch = [&](int qs) __attribute__((always_inline)) {
        const float* sx = tp + (size_t)qs * 1536;
#pragma unroll
        for (int tau = 0; tau < 2; tau++) Xnp.t[tau] = *reinterpret_cast<const f32x4v*>(sx + n * 32 + 16 * tau);
        if (RICH) {
            const float* sr = tz + (size_t)qs * RT16S_RREC;
#pragma unroll
            for (int e = 0; e < 12; e++) adp[e] = *reinterpret_cast<const f32x4v*>(sr + (n * 12 + e) * 256);
        } else {
            const float* sz = tz + (size_t)qs * RT16S_ZREC;
#pragma unroll
            for (int Q = 0; Q < 13; Q++) z1p[Q] = (Q < 12 || g < 2) ? sz[4 * Q] : 0.0f;
#pragma unroll
            for (int Q2 = 0; Q2 < 5; Q2++) z2p[Q2] = sz[52 + 4 * Q2];
        }
    };
    prefetch(n_steps * nst - 1);
    RT_STAMP_DECL;
#if RT16SH_SCHED
    int step0 = n_steps;                                                 // as in the helper wave: the same counts, the same trip counts
#endif
    for (int iv = n_save - 2; iv >= 0; iv--) {
#if RT16SH_SCHED
        substeps = sched[iv];
        step0 -= substeps;
#endif
        for (int s = substeps - 1; s >= 0; s--) {
#if RT16SH_SCHED
            const int step = step0 + s;
#else
            const int step = iv * substeps + s;
#endif
#pragma nounroll
            for (int st = nst - 1; st >= 0; st--) {
                const int qs = step * nst + st;
                RT_STAMP_BEGIN();
                // ---- before (B), beside the helper's pullback: everything that depends on the tapes alone ----
                f32x4t A1[4], D1[4], A2[2], D2[2];
                const V16 Xme = Xnp;
                if (RICH) {
#pragma unroll
                    for (int t = 0; t < 4; t++) { A1[t] = adp[t]; D1[t] = adp[4 + t]; }
#pragma unroll
                    for (int u = 0; u < 2; u++) { A2[u] = adp[8 + u]; D2[u] = adp[10 + u]; }
                } else {
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        f32x4t z;
#pragma unroll
                        for (int r = 0; r < 4; r++) z[r] = (4 * t + r < 13) ? z1p[(4 * t + r) < 13 ? 4 * t + r : 0] : 0.0f;
                        rt16_act_pair<ACT>(z, A1[t], D1[t]);
                    }
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        f32x4t z;
#pragma unroll
                        for (int r = 0; r < 4; r++) z[r] = (4 * u + r < 5) ? z2p[(4 * u + r) < 5 ? 4 * u + r : 0] : 0.0f;
                        rt16_act_pair<ACT>(z, A2[u], D2[u]);
                    }
#pragma unroll
                    for (int r = 1; r < 4; r++) { D1[3][r] = 0.0f; D2[1][r] = 0.0f; }   // padding quads: Q >= 13, Q2 >= 5
                    if (g >= 2) D1[3][0] = 0.0f;                                         // features 50, 51 of quad 12
                }
                if (qs > 0) prefetch(qs - 1);
                // (SPLIT) the twelve l-plane operands of this net's W1^T products, from L2: requested here, consumed behind barrier B and two chains
                // ... and the 24 h / m plane fragments from LDS: all of them before barrier B too, so that behind it the products wait for nothing
                // (fetched tile by tile in front of their products they exposed an LDS round trip per tile: 8.03 instead of 8.2 ms, no more)
                u32x4 Lr[12], Hm[24];
                if constexpr (SPLIT) {
                    int lz = lane;                        // (opaque: left loop-invariant the loads are hoisted out of the time loop and their registers pinned)
                    asm volatile("" : "+v"(lz));
                    const u32x4* lg = reinterpret_cast<const u32x4*>(wimg + RT_NSA_OFF + RT_NSA_L) + n * 12 * 64 + lz;
#pragma unroll
                    for (int u = 0; u < 12; u++) Lr[u] = lg[u * 64];
                    const u32x4* hn = hm + n * 24 * 64 + lz;
#pragma unroll
                    for (int u = 0; u < 24; u++) Hm[u] = hn[u * 64];
                }
                float a3[2][8], a2[4][5];
                rt16_fetch_ops<2, 8>(wl, a3, [&](int u, int k) { return b3T[u] + (16 * (k >> 2) + (k & 3)) * RT_LD3; });
                rt16_fetch_ops<4, 5>(wl, a2, [&](int t, int k) { return b2T[t] + 4 * k * RT_LD2; });
                float* rec = rec0 + (size_t)qs * RT16S_REC;
#pragma unroll
                for (int tau = 0; tau < 2; tau++) *reinterpret_cast<f32x4v*>(rec + j * 720 + n * 32 + 16 * tau + 4 * g) = Xme.t[tau];
#pragma unroll
                for (int Q = 0; Q < 13; Q++)
                    if (Q < 12 || g < 2) sw[4 * Q] = A1[Q >> 2][Q & 3];
#pragma unroll
                for (int Q2 = 0; Q2 < 5; Q2++) sw[52 + 4 * Q2] = A2[Q2 >> 2][Q2 & 3];
                RT_STAMP(0);
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");           // (B) the helper's dO is in LDS
                RT_STAMP(1);
                V16 dO;
#pragma unroll
                for (int tau = 0; tau < 2; tau++) dO.t[tau] = dOl[(n * 2 + tau) * 64 + lane];
                // (3) δz2 = (W3^T dO) ∘ act'(z2)
                f32x4t dZ2[2] = {(f32x4t)(0.0f), (f32x4t)(0.0f)};
                rt16_run_ops<2, 8>(a3, dZ2, [&](int k) { return dO.t[k >> 2][k & 3]; });
#pragma unroll
                for (int u = 0; u < 2; u++) dZ2[u] *= D2[u];
                float a1[2][2][13];
                if constexpr (!SPLIT) rt16_fetch_ops<2, 13>(wl, a1[0], [&](int c, int k) { return b1T + 16 * c + 4 * k * RT_LD1; });
                RT_SCHED_HARD();
                // (4) δz1 = (W2^T δz2) ∘ act'(z1)
                f32x4t dZ1[4] = {(f32x4t)(0.0f), (f32x4t)(0.0f), (f32x4t)(0.0f), (f32x4t)(0.0f)};
                rt16_run_ops<4, 5>(a2, dZ1, [&](int k) { return dZ2[k >> 2][k & 3]; });
#pragma unroll
                for (int t = 0; t < 4; t++) dZ1[t] *= D1[t];
                RT_STAMP(2);
                {
#pragma unroll
                    for (int Q = 0; Q < 13; Q++)
                        if (Q < 12 || g < 2) sw[72 + 4 * Q] = dZ1[Q >> 2][Q & 3];
#pragma unroll
                    for (int Q2 = 0; Q2 < 5; Q2++) sw[124 + 4 * Q2] = dZ2[Q2 >> 2][Q2 & 3];
                    float* s3 = stg + j * 180 + 144 + 4 * g - 1;                         // output o = face - 1
#pragma unroll
                    for (int v = 0; v < 2; v++)
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (!(v == 0 && r == 0 && g == 0)) s3[16 * v + r] = dO.t[v][r];
                    // (deferring this copy to the top of the next stage, beside the helper's pullback, was measured: 7.58 -> 7.63 ms in front of that
                    //  stage's loads, 7.89 ms behind them — the stores then sit in front of the l-plane loads in the in-order vmcnt queue)
#pragma unroll
                    for (int i = 0; i < 11; i++) *reinterpret_cast<f32x4v*>(rec + rec_wr[i]) = *reinterpret_cast<const f32x4v*>(stg + stg_rd[i]);
                }
#pragma unroll
                for (int t = 0; t < 4; t++) gb1[t] += dZ1[t];
#pragma unroll
                for (int u = 0; u < 2; u++) { gb2[u] += dZ2[u]; gb3[u] += dO.t[u]; }
                RT_STAMP(3);
                // (5) this net's part of the state cotangent, W1_n^T δz1 (6 tiles x 13 k-steps)
                if constexpr (SPLIT) {
                    // δz1 as the B operand of two 32-deep k-blocks: element e of k-block kb is quad 8 kb + e of this lane group (padding quads are zero)
                    const float d80[8] = {dZ1[0][0], dZ1[0][1], dZ1[0][2], dZ1[0][3], dZ1[1][0], dZ1[1][1], dZ1[1][2], dZ1[1][3]};
                    const float d81[8] = {dZ1[2][0], dZ1[2][1], dZ1[2][2], dZ1[2][3], dZ1[3][0], dZ1[3][1], dZ1[3][2], dZ1[3][3]};
                    // the first k-block over all six tiles, the second k-block's split issued in pieces between them (one wave per SIMD: nothing else hides
                    // its 44 vector instructions), then the second k-block
                    const Bf3 B0 = bf3_split8(d80);
                    Bf3 B1 = B0;
                    f32x4t c2[6];
#pragma unroll
                    for (int tl = 0; tl < 6; tl++) {
                        Bf3 A0;
                        A0.h = Hm[tl * 2 + 0]; A0.m = Hm[tl * 2 + 1]; A0.l = Lr[tl];
                        c2[tl] = mfma16_bf3(A0, B0, (f32x4t)(0.0f));
                        RT_SCHED_FENCE();
                        if (tl < 4) {
                            bf3_split_pair(d81[2 * tl], d81[2 * tl + 1], tl, B1);
                            RT_SCHED_FENCE();
                        }
                    }
#pragma unroll
                    for (int tl = 0; tl < 6; tl++) {
                        Bf3 A1_;
                        A1_.h = Hm[(6 + tl) * 2 + 0]; A1_.m = Hm[(6 + tl) * 2 + 1]; A1_.l = Lr[6 + tl];
                        c2[tl] = mfma16_bf3(A1_, B1, c2[tl]);
                        ex[(n * 6 + tl) * 64 + lane] = c2[tl];
                        RT_SCHED_FENCE();
                    }
                } else
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    if (q < 2) rt16_fetch_ops<2, 13>(wl, a1[(q + 1) & 1], [&](int c, int k) { return b1T + 32 * (q + 1) + 16 * c + 4 * k * RT_LD1; });
                    RT_SCHED_HARD();
                    f32x4t c2[2] = {(f32x4t)(0.0f), (f32x4t)(0.0f)};
                    rt16_run_ops<2, 13>(a1[q & 1], c2, [&](int k) { return dZ1[k >> 2][k & 3]; });
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) ex[(n * 6 + q * 2 + tau) * 64 + lane] = c2[tau];
                    RT_SCHED_HARD();
                }
                RT_STAMP(4);
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");           // (A) this net's part of x̄ is in LDS
                RT_STAMP(5);
            }
        }
    }
#ifndef COLNDE_STAMPS_FWD
    RT_STAMP_FLUSH();
#endif
    // ---- the tile's slab row: bias gradients of net n (sums over the 16 columns = the lanes of a g-group); the loss sums are the helper's ----
    auto colsum = [&](float v) {
        v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
        return v;
    };
#pragma unroll
    for (int Q = 0; Q < 13; Q++) {
        const float v = colsum(gb1[Q >> 2][Q & 3]);
        if (j == 0 && (Q < 12 || g < 2)) out[n * m.net_size + m.b_off[0] + 4 * Q + g] = v;
    }
#pragma unroll
    for (int Q2 = 0; Q2 < 5; Q2++) {
        const float v = colsum(gb2[Q2 >> 2][Q2 & 3]);
        if (j == 0) out[n * m.net_size + m.b_off[1] + 4 * Q2 + g] = v;
    }
#pragma unroll
    for (int v_ = 0; v_ < 2; v_++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float v = colsum(gb3[v_][r]);
            const int face = 16 * v_ + 4 * g + r;
            if (j == 0 && face >= 1) out[n * m.net_size + m.b_off[2] + face - 1] = v;
        }
