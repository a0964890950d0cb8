// Body of forward_kernel and forward_ens_kernel (engine_tile16.hip): included by both, so that the single-model kernel stays the text it was.
// In scope: the kernel's arguments, `m` (the kernel argument; the ensemble kernel: its patched copy in LDS), `smem` (the ensemble kernel: the dynamic LDS behind
// that copy) and T16_AG_TILE, the workgroup's slab of m.ag (blockIdx.x; the ensemble kernel: blockIdx.y * gridDim.x + blockIdx.x).
    constexpr int FMAXR = 3072 / NTH;      // owner-thread register items per state array: CT * ns <= 3072 (ns <= 192)
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nth >> 6;
    float* wl = smem;                                   // raw weights (WLDS) + 128 floats of zero padding
    float* xs = smem + (WLDS ? ((m.n_params + 3) & ~3) + 128 : 0);
    float* kk = xs + CT * m.ld_x;
    const int zld = (m.n_nets * m.act_off[m.n_layers - 1] + 3) & ~3;      // floats per column of the hidden pre-activation tape
    float* A = AG ? m.ag + T16_AG_TILE * m.n_nets * CT * m.ld_a : kk + CT * m.ld_x;
    float* F = AG ? kk + CT * m.ld_x : A + m.n_nets * CT * m.ld_a;
    float* Ri_l = F + 3 * CT * m.ld_f;
    float* bcl = Ri_l + CT * m.ld_f;
    const int total = (int)(bcl + CT * 8 - smem);
    for (int i = tid; i < total; i += nth) smem[i] = 0.0f;
    __syncthreads();
    if (WLDS) for (int i = tid; i < m.n_params; i += nth) wl[i] = w[i];
    const float* wsrc = WLDS ? wl : w;
    const int col0 = blockIdx.x * CT;
    const int n_items = CT * m.ns;
    load_bcs(m, bcs, bcl, col0, n_col, tid);

    float xn[FMAXR], acc[FMAXR];
#pragma unroll
    for (int r = 0; r < FMAXR; r++) {
        const int it = tid + r * nth;
        xn[r] = 0.0f;
        acc[r] = 0.0f;
        if (it < n_items) {
            const int c = it / m.ns, i = it - c * m.ns;
            xn[r] = x0[(size_t)min(col0 + c, n_col - 1) * m.ns + i];
            if (sol && col0 + c < n_col) sol[((size_t)(col0 + c) * n_save) * m.ns + i] = xn[r];
        }
    }
    const int n_steps = (n_save - 1) * substeps;
    const int nst = m.nst;                               // RHS evaluations (taped stage inputs) per step: 4 (RK4) or s (RKC2)
    float* tp = tape ? tape + (size_t)blockIdx.x * n_steps * nst * n_items : nullptr;
    int step = 0;
    if (RKC) {     // (a template parameter: the RK4 instantiation must not carry this branch's registers — 244 -> 262 VGPRs cost it a wave per SIMD)
        // ---- s-stage RKC2 steps (colnde_dev.h; coefficients from the host table): per owner item Y_0 = xn, Y_{j-1} = ym1,
        //      Y_{j-2} = ym2 and F_0 = f0 stay in registers; stage st evaluates F_st = f(Y_st), the step ends with Y_s
        const float* mu_t = m.rkc, *nu_t = m.rkc + RKC_LD, *mut_t = m.rkc + 2 * RKC_LD, *gat_t = m.rkc + 3 * RKC_LD, *c_t = m.rkc + 4 * RKC_LD;
        float ym1[FMAXR], ym2[FMAXR];                    // acc[] serves as f0
        for (int iv = 0; iv < n_save - 1; iv++) {
            const float t0 = save_times[iv];
            const float dt = (save_times[iv + 1] - t0) / (float)substeps;
            for (int s = 0; s < substeps; s++, step++) {
                const float ts = t0 + (float)s * dt;
#pragma nounroll
                for (int st = 0; st <= nst; st++) {      // st = nst: only the final combination Y_s
                    const float cmu = mu_t[st], cnu = nu_t[st], cmt = mut_t[st] * dt, cga = gat_t[st] * dt;
                    const bool last = st == nst;
                    const bool save = last && s == substeps - 1;
#pragma unroll
                    for (int r = 0; r < FMAXR; r++) {
                        const int it = tid + r * nth;
                        if (it < n_items) {
                            const int c = it / m.ns, i = it - c * m.ns;
                            const int o = c * m.ld_x + i;
                            // increment form d_j = Y_j - Y_0 (the weights of Y_0, Y_{j-1}, Y_{j-2} sum to one): the differences
                            // 2 d_{j-1} - d_{j-2} are taken between increments, not O(1) states — float32 stays accurate
                            float dj = 0.0f;
                            if (st == 1) {
                                acc[r] = kk[o];                                        // F_0
                                dj = cmt * acc[r];
                            } else if (st >= 2) {
                                dj = cmu * ym1[r] + cnu * ym2[r] + cmt * kk[o] + cga * acc[r];
                            }
                            const float v = xn[r] + dj;
                            ym2[r] = st == 0 ? 0.0f : ym1[r];
                            ym1[r] = dj;
                            if (last) {
                                xn[r] = v;
                                if (save && sol && col0 + c < n_col) sol[((size_t)(col0 + c) * n_save + iv + 1) * m.ns + i] = v;
                            } else {
                                xs[o] = v;
                                if (tp) tp[((size_t)step * nst + st) * n_items + it] = v;
                            }
                        }
                    }
                    __syncthreads();
                    if (last) break;
                    if (AG && m.sf) mlp_forward_split(m, wsrc, xs, A, wave, nwaves, lane,
                                             ztape ? ztape + ((size_t)blockIdx.x * n_steps * nst + (size_t)step * nst + st) * ((size_t)CT * zld) : nullptr, zld);
                    else
                    mlp_forward<false, WLDS>(m, pk, wsrc, wf, xs, nullptr, A, wave, nwaves, lane,
                                             ztape ? ztape + ((size_t)blockIdx.x * n_steps * nst + (size_t)step * nst + st) * ((size_t)CT * zld) : nullptr, zld);
                    physics_forward(m, xs, A, F, Ri_l, bcl, ts + c_t[st] * dt, kk, tid, nth);
                }
            }
        }
        return;
    }
    for (int iv = 0; iv < n_save - 1; iv++) {
        const float t0 = save_times[iv];
        const float dt = (save_times[iv + 1] - t0) / (float)substeps;
        for (int s = 0; s < substeps; s++, step++) {
            const float ts = t0 + (float)s * dt;
#pragma nounroll
            for (int st = 0; st < 4; st++) {
                const float ca = st == 0 ? 0.0f : (st == 3 ? 1.0f : 0.5f);            // stage abscissa
                const float cbp = (st == 1) ? 1.0f / 6.0f : 1.0f / 3.0f;               // weight of k_{st-1}
#pragma unroll
                for (int r = 0; r < FMAXR; r++) {
                    const int it = tid + r * nth;
                    if (it < n_items) {
                        const int c = it / m.ns, i = it - c * m.ns;
                        const int o = c * m.ld_x + i;
                        float v = xn[r];
                        if (st > 0) {
                            const float kv = kk[o];
                            acc[r] += cbp * kv;
                            v += ca * dt * kv;
                        }
                        xs[o] = v;
                        if (tp) tp[((size_t)step * 4 + st) * n_items + it] = v;
                    }
                }
                __syncthreads();
                if (AG && m.sf) mlp_forward_split(m, wsrc, xs, A, wave, nwaves, lane,
                                         ztape ? ztape + ((size_t)blockIdx.x * n_steps * 4 + (size_t)step * 4 + st) * ((size_t)CT * zld) : nullptr, zld);
                else
                mlp_forward<false, WLDS>(m, pk, wsrc, wf, xs, nullptr, A, wave, nwaves, lane,
                                         ztape ? ztape + ((size_t)blockIdx.x * n_steps * 4 + (size_t)step * 4 + st) * ((size_t)CT * zld) : nullptr, zld);
                physics_forward(m, xs, A, F, Ri_l, bcl, ts + ca * dt, kk, tid, nth);
            }
            const bool save = (s == substeps - 1);
#pragma unroll
            for (int r = 0; r < FMAXR; r++) {
                const int it = tid + r * nth;
                if (it < n_items) {
                    const int c = it / m.ns, i = it - c * m.ns;
                    acc[r] += (1.0f / 6.0f) * kk[c * m.ld_x + i];
                    xn[r] += dt * acc[r];
                    acc[r] = 0.0f;
                    if (save && sol && col0 + c < n_col)
                        sol[((size_t)(col0 + c) * n_save + iv + 1) * m.ns + i] = xn[r];
                }
            }
            __syncthreads();
        }
    }
