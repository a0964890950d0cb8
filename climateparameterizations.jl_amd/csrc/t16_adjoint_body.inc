// Body of adjoint_kernel and adjoint_ens_kernel (engine_tile16.hip): included by both, so that the single-model kernel stays the text it was.
// In scope: the kernel's arguments (the ensemble kernel has moved the pointers to model blockIdx.y's arrays; MAXT = 1, TAPEDW, tiles = nullptr there),
// T16_ENS (1: the model's constants and plane images are patched into the LDS copy of the description) and T16_AG_TILE, the workgroup's slab of m_arg.ag.
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nth >> 6;
    // the model description lives in LDS: per-layer fields indexed with a runtime layer number would otherwise be
    // dependent scalar loads from the kernarg segment (each followed by a full lgkmcnt(0) drain)
    // (kept inside the dynamic region: a static __shared__ object would shift its base, guide G17)
    DevModel& m_lds = *reinterpret_cast<DevModel*>(smem);
    float* const base = smem + MODEL_FLOATS;
    float* wl = base;                                   // raw weights (WLDS) + 128 floats of zero padding
    float* xs = base + (WLDS ? ((m_arg.n_params + 3) & ~3) + 128 : 0);
    float* dbar = xs + CT * m_arg.ld_x;
    float* xb = dbar + CT * m_arg.ld_x;
    static_assert(!AG || TAPEDW, "rows in global memory: the taped-dW adjoint only (the in-register one addresses its operands relative to LDS)");
    // (AG: the delta rows in the workgroup's slab of m_arg.ag; only with the Z tape, so that no A array exists — the host guarantees it)
    float* Z = AG ? m_arg.ag + T16_AG_TILE * m_arg.n_nets * CT * m_arg.ld_a : xb + CT * m_arg.ld_x;
    // taped mode with the hidden pre-activations taped: the activations go from the Z tape straight into the delta tape and are never
    // needed on chip — no A array, and two workgroups of a 64-level network fit in a CU's LDS
    const bool noA = TAPEDW && ztape != nullptr;
    float* A = AG ? Z : Z + m_arg.n_nets * CT * m_arg.ld_a;
    float* gb = AG ? xb + CT * m_arg.ld_x : (noA ? A : A + m_arg.n_nets * CT * m_arg.ld_a);
    float* Ri_l = gb + 3 * CT * m_arg.ld_f;
    float* Rib_l = Ri_l + CT * m_arg.ld_f;
    float* bcl = Rib_l + CT * m_arg.ld_f;
    float* red = bcl + CT * 8;
    const int total = (int)(red + 16 * 8 - smem);
    for (int i = tid; i < total; i += nth) smem[i] = 0.0f;
    __syncthreads();
    for (int i = tid; i < (int)(sizeof(DevModel) / 4); i += nth) ((int*)&m_lds)[i] = ((const int*)&m_arg)[i];
    if (WLDS) for (int i = tid; i < m_arg.n_params; i += nth) wl[i] = w[i];
#if T16_ENS
    __syncthreads();                                    // model blockIdx.y's constants and plane images into the copy, once it is complete
    if (tid == 0) t16_ens_patch_model(m_lds, en, blockIdx.y);
#endif
    __syncthreads();
    const DevModel& m = m_lds;
    const float* wsrc = WLDS ? wl : w;
    const int col0 = blockIdx.x * CT;
    const int n_items = CT * m.ns;
    load_bcs(m, bcs, bcl, col0, n_col, tid);

    f32x4 gacc[MAXT];
#pragma unroll
    for (int s = 0; s < MAXT; s++) gacc[s] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    float dbias[MAXB];
    int bz[MAXB];
#pragma unroll
    for (int r = 0; r < MAXB; r++) {
        dbias[r] = 0.0f;
        const int b = tid + r * nth;
        bz[r] = b < m.n_bias ? bias_zoff[b] : -1;
    }
    float lam[MAXR], xbs[MAXR], xpre[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; r++) lam[r] = 0.0f;
    float sums[6] = {0, 0, 0, 0, 0, 0};
    STAMP_DECL;

    // per-slot LDS addresses (float indices into smem, lane part folded in) of this wave's weight-gradient tiles
    int a_ad[MAXT], d_ad[MAXT];
    unsigned long long a_is_act = 0ull;
    if (!TAPEDW) {
        const int cq = lane >> 4;
#pragma unroll
        for (int sl = 0; sl < MAXT; sl++) {
            const int t = wave + sl * nwaves;
            a_ad[sl] = 0;
            d_ad[sl] = 0;
            if (t < m.n_tiles) {
                const TileDesc d = tiles[t];
                const int stride = d.a_src ? m.ld_a : m.ld_x;
                a_ad[sl] = (int)((d.a_src ? A + d.net * CT * m.ld_a : xs) - smem) + d.a_off + (lane & 15) + cq * stride;
                d_ad[sl] = (int)(Z - smem) + d.net * CT * m.ld_a + d.d_off + (lane & 15) + cq * m.ld_a;
                if (d.a_src) a_is_act |= 1ull << sl;
            }
        }
    }

    const int n_steps = (n_save - 1) * substeps;
    const int nst = m.nst;                               // taped stage inputs per step: 4 (RK4) or s (RKC2)
    constexpr bool rkc = RKC;            // a template parameter: the RK4 instantiations do not carry the RKC cotangent registers
    const float* mu_t = m.rkc, *nu_t = m.rkc + RKC_LD, *mut_t = m.rkc + 2 * RKC_LD, *gat_t = m.rkc + 3 * RKC_LD, *kap_t = m.rkc + 5 * RKC_LD;
    const float* tp = tape + (size_t)blockIdx.x * n_steps * nst * n_items;
    // the tape is read one stage ahead of its use (xpre) so that its HBM latency hides under the previous stage
#pragma unroll
    for (int r = 0; r < MAXR; r++) {
        const int it = tid + r * nth;
        xpre[r] = it < n_items ? tp[((size_t)n_steps * nst - 1) * n_items + it] : 0.0f;
    }
    // RKC2 (discrete adjoint of the recurrence in colnde_dev.h): cotangents of Y_j (lam), Y_{j-1} (yb1), Y_{j-2} (yb2), Y_0 (yb0)
    // and F_0 (f0b) per owner item; unused by the RK4 path
    float yb1[MAXR], yb2[MAXR], yb0[MAXR], f0b[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; r++) { yb1[r] = 0.0f; yb2[r] = 0.0f; yb0[r] = 0.0f; f0b[r] = 0.0f; }

    // save point 0 enters the loss value only (x0 does not depend on the weights)
#pragma unroll
    for (int r = 0; r < MAXR; r++) {
        const int it = tid + r * nth;
        if (it < n_items) {
            const int c = it / m.ns, i = it - c * m.ns;
            if (col0 + c < n_col) {
                float dummy = 0.0f;
                loss_inject(m, sol, truth, ((size_t)(col0 + c) * n_save) * m.ns, i, lw.w, dummy, sums);
            }
        }
    }

    for (int iv = n_save - 2; iv >= 0; iv--) {
        const float t0 = save_times[iv];
        const float dt = (save_times[iv + 1] - t0) / (float)substeps;
        // λ += ∂loss/∂sol[:, iv+1]
#pragma unroll
        for (int r = 0; r < MAXR; r++) {
            const int it = tid + r * nth;
            if (it < n_items) {
                const int c = it / m.ns, i = it - c * m.ns;
                if (col0 + c < n_col)
                    loss_inject(m, sol, truth, ((size_t)(col0 + c) * n_save + iv + 1) * m.ns, i, lw.w, lam[r], sums);
            }
        }
        for (int s = substeps - 1; s >= 0; s--) {
            const int step = iv * substeps + s;
#pragma unroll
            for (int r = 0; r < MAXR; r++) xbs[r] = 0.0f;
#pragma nounroll
            for (int st = nst - 1; st >= 0; st--) {
                // k̄4 = dt/6 λ; k̄3 = dt/3 λ + dt x̄4; k̄2 = dt/3 λ + dt/2 x̄3; k̄1 = dt/6 λ + dt/2 x̄2
                const float cwl = (st == 0 || st == 3) ? dt / 6.0f : dt / 3.0f;
                const float cwx = st == 2 ? dt : 0.5f * dt;
                // RKC2, stage input Y_st feeds Y_j, j = st + 1, through mu~_j h F_st:
                const float cmu = rkc ? mu_t[st + 1] : 0.0f, cnu = rkc ? nu_t[st + 1] : 0.0f;
                const float cmt = rkc ? mut_t[st + 1] * dt : 0.0f, cga = rkc ? gat_t[st + 1] * dt : 0.0f, ck0 = rkc ? kap_t[st + 1] : 0.0f;
                STAMP_BEGIN();
                // stage input from the tape; stage cotangent k̄_st = wl λ + wx x̄_{st+1}
#pragma unroll
                for (int r = 0; r < MAXR; r++) {
                    const int it = tid + r * nth;
                    if (it < n_items) {
                        const int c = it / m.ns, i = it - c * m.ns;
                        const int o = c * m.ld_x + i;
                        xs[o] = xpre[r];
                        float kb;
                        if (rkc) {
                            // lam = cotangent of Y_j, complete once the previous iteration's pullback (xb: J(Y_j)^T F̄_j) is added
                            if (st < nst - 1) {
                                const float yj = yb1[r] + xb[o];
                                yb1[r] = yb2[r];
                                yb2[r] = 0.0f;
                                lam[r] = yj;
                            }
                            if (st >= 1) {
                                yb0[r] += ck0 * lam[r];
                                yb1[r] += cmu * lam[r];
                                yb2[r] += cnu * lam[r];
                                f0b[r] += cga * lam[r];
                                kb = cmt * lam[r];
                            } else {
                                // Y_1 = Y_0 + mu~_1 h F_0: lam holds Ȳ_1, yb1 the nu_2 part of Ȳ_0
                                yb0[r] += lam[r] + yb1[r];
                                kb = f0b[r] + cmt * lam[r];
                                yb1[r] = 0.0f;
                                f0b[r] = 0.0f;
                            }
                        } else {
                            kb = cwl * lam[r];
                            if (st < 3) kb += cwx * xb[o];
                        }
                        dbar[o] = kb;
                    }
                }
                {
                    const int qn = step * nst + st - 1;            // the stage handled next (tape order is time order)
                    if (qn >= 0) {
#pragma unroll
                        for (int r = 0; r < MAXR; r++) {
                            const int it = tid + r * nth;
                            if (it < n_items) xpre[r] = tp[(size_t)qn * n_items + it];
                        }
                    }
                }
                __syncthreads();
                STAMP(0);
                if (TAPEDW && ztape) {
                    // hidden-layer pre-activations taped by the forward kernel: Z into LDS, A = act(Z) straight into this stage's record of
                    // the delta tape (the output layer enters the pullback linearly: its values are not needed; its A slot is never read
                    // by the dW GEMM either)
                    const int hid = m.act_off[m.n_layers - 1], zld = (m.n_nets * hid + 3) & ~3;
                    const float* zr = ztape + ((size_t)blockIdx.x * n_steps * nst + (size_t)step * nst + st) * ((size_t)CT * zld);
                    const int ns4r = (m.ns + 3) & ~3, act4r = (m.act_total + 3) & ~3;
                    const int Rr = ns4r + 2 * m.n_nets * act4r;
                    float* recA = dwtape + ((size_t)blockIdx.x * n_steps * nst + (size_t)step * nst + st) * ((size_t)CT * Rr) + ns4r;
                    // (segments start at multiples of 4 floats: one float4 never straddles two layers; up to four float4 per lane
                    //  are fetched back to back so that one HBM latency covers them)
                    const int nq = (m.n_nets * hid) >> 2;                      // float4 items per column
                    for (int c = wave; c < CT; c += nwaves)
                        for (int q0 = lane; q0 < nq; q0 += 4 * 64) {
                            float4 v[4];
#pragma unroll
                            for (int u = 0; u < 4; u++)
                                if (q0 + 64 * u < nq) v[u] = *reinterpret_cast<const float4*>(zr + c * zld + 4 * (q0 + 64 * u));
#pragma unroll
                            for (int u = 0; u < 4; u++) {
                                const int q = q0 + 64 * u;
                                if (q < nq) {
                                    const int f = 4 * q, net = f / hid, o = f - net * hid;
                                    int l = 0;
                                    while (o >= m.act_off[l + 1]) l++;
                                    const int a = m.acts[l];
                                    // the pad slots behind a layer's last feature were never written by the forward kernel: they must read as
                                    // zero (a backward chain multiplies them with whatever weight sits behind the row's end)
                                    const int nvalid = m.sizes[l + 1] - (o - m.act_off[l]);
                                    if (nvalid < 4) {
                                        if (nvalid < 1) v[u].x = 0.0f;
                                        if (nvalid < 2) v[u].y = 0.0f;
                                        if (nvalid < 3) v[u].z = 0.0f;
                                        v[u].w = 0.0f;
                                    }
                                    float* zd = Z + (net * CT + c) * m.ld_a + o;
                                    zd[0] = v[u].x; zd[1] = v[u].y; zd[2] = v[u].z; zd[3] = v[u].w;
                                    *reinterpret_cast<float4*>(recA + (size_t)c * Rr + net * act4r + o) =
                                        make_float4(dev_act(a, v[u].x), dev_act(a, v[u].y), dev_act(a, v[u].z), dev_act(a, v[u].w));
                                }
                            }
                        }
                    __syncthreads();
                } else
                    mlp_forward<true, WLDS>(m, pk, wsrc, wf, xs, Z, A, wave, nwaves, lane);
                STAMP(1);
                physics_vjp(m, xs, dbar, Z, xb, gb, Ri_l, Rib_l, tid, nth, rkc ? (st == nst - 1 ? 1 : 2) : 0);
                STAMP(2);
                if (AG && m.sb) mlp_backward_split(m, pk, wb, Z, xb, wave, nwaves, lane);
                else mlp_backward<WLDS>(m, pk, wsrc, wb, Z, xb, wave, nwaves, lane);
                STAMP(3);
                // weight gradients: dW += A_{l-1}^T dZ_l over the tile's 16 columns; operands of slot sl+1 are read
                // while the MFMAs of slot sl run
                if (TAPEDW) {
                    // row = [xs (ns4) | A of every net (act4 each) | dZ of every net (act4 each)], every segment padded to a multiple of
                    // 4 floats (the pads copy LDS row padding: finite, never stored by dw_gemm).  LDS rows are 8-byte aligned (stride
                    // == 2 mod 4), tape rows 16-byte aligned: copied two floats at a time
                    const int ns4 = (m.ns + 3) & ~3, act4 = (m.act_total + 3) & ~3;
                    const int R = ns4 + 2 * m.n_nets * act4;
                    float* rec = dwtape + ((size_t)blockIdx.x * n_steps * nst + (size_t)step * nst + st) * ((size_t)CT * R);
                    const int hx = ns4 >> 1, ha = act4 >> 1;                                        // float2 items per segment
                    for (int c = wave; c < CT; c += nwaves) {                                       // one wave per column
                        float* row = rec + (size_t)c * R;
                        for (int q = lane; q < hx; q += 64)
                            *reinterpret_cast<float2*>(row + 2 * q) = *reinterpret_cast<const float2*>(xs + c * m.ld_x + 2 * q);
                        for (int seg = noA ? m.n_nets : 0; seg < 2 * m.n_nets; seg++) {               // A of every net (unless already written), then dZ of every net
                            const int net = seg < m.n_nets ? seg : seg - m.n_nets;
                            const float* src = (seg < m.n_nets ? A : Z) + (net * CT + c) * m.ld_a;
                            float* dst = row + ns4 + seg * act4;
                            for (int o = lane; o < ha; o += 64)
                                *reinterpret_cast<float2*>(dst + 2 * o) = *reinterpret_cast<const float2*>(src + 2 * o);
                        }
                    }
                } else {
                    float pa[2][4], pb[2][4];
                    const int zs4 = 4 * m.ld_a;
                    if (wave < m.n_tiles) {
                        const int as4 = 4 * ((a_is_act & 1ull) ? m.ld_a : m.ld_x);
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            pa[0][q] = smem[a_ad[0] + q * as4];
                            pb[0][q] = smem[d_ad[0] + q * zs4];
                        }
                    }
#pragma unroll
                    for (int sl = 0; sl < MAXT; sl++) {
                        if (sl + 1 < MAXT && wave + (sl + 1) * nwaves < m.n_tiles) {
                            const int as4 = 4 * (((a_is_act >> (sl + 1)) & 1ull) ? m.ld_a : m.ld_x);
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                pa[(sl + 1) & 1][q] = smem[a_ad[(sl + 1) % MAXT] + q * as4];
                                pb[(sl + 1) & 1][q] = smem[d_ad[(sl + 1) % MAXT] + q * zs4];
                            }
                        }
                        if (wave + sl * nwaves < m.n_tiles) {
#pragma unroll
                            for (int q = 0; q < 4; q++) gacc[sl] = mfma16(pa[sl & 1][q], pb[sl & 1][q], gacc[sl]);
                        }
                    }
                }
                STAMP(4);
#pragma unroll
                for (int r = 0; r < MAXB; r++)
                    if (bz[r] >= 0) {
                        float sacc = 0.0f;
#pragma unroll
                        for (int c = 0; c < CT; c++) sacc += Z[bz[r] + c * m.ld_a];
                        dbias[r] += sacc;
                    }
#pragma unroll
                for (int r = 0; r < MAXR; r++) {
                    const int it = tid + r * nth;
                    if (it < n_items) {
                        const int c = it / m.ns, i = it - c * m.ns;
                        xbs[r] += xb[c * m.ld_x + i];
                    }
                }
                __syncthreads();
                STAMP(5);
            }
            if (rkc) {
                // λ_n = Ȳ_0 + J(Y_0)^T F̄_0 (xb of the st = 0 pullback; visible after the stage's closing barrier)
#pragma unroll
                for (int r = 0; r < MAXR; r++) {
                    const int it = tid + r * nth;
                    if (it < n_items) {
                        const int c = it / m.ns, i = it - c * m.ns;
                        lam[r] = yb0[r] + xb[c * m.ld_x + i];
                    }
                    yb0[r] = 0.0f;
                }
            } else {
#pragma unroll
                for (int r = 0; r < MAXR; r++) lam[r] += xbs[r];
            }
        }
    }

    STAMP_FLUSH();
    // flush this tile's partial gradient and loss sums
    float* out = slab + (size_t)blockIdx.x * (m.n_params + 8);
#pragma unroll
    for (int sl = 0; sl < MAXT; sl++) {
        const int t = wave + sl * nwaves;
        if (!TAPEDW && t < m.n_tiles) {
            const TileDesc d = tiles[t];
            const int j = lane & 15;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = 4 * (lane >> 4) + r;
                if (i < d.ni_rem && j < d.no_rem) out[d.g_off + i * d.no + j] = gacc[sl][r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < MAXB; r++) {
        const int b = tid + r * nth;
        if (b < m.n_bias) out[bias_goff[b]] = dbias[r];
    }
    block_reduce_sums(sums, 6, red, out + m.n_params, tid, nth);
    if (tid >= 6 && tid < 8) out[m.n_params + tid] = 0.0f;
