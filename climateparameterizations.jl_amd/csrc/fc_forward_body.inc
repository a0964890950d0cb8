// fc_forward_body.inc — the text of the fc32 forward kernel (engine_fc.hip), included by its three entry points: fc_forward_kernel (CONV = false),
// fc_forward_conv_kernel (CW = 16, ENS = false, CONV = true, the filter in `cv`) and fc_forward_conv_ens_kernel (CW = 16, ENS = CONV = true, `cv` already
// offset to the workgroup's model).  Textual inclusion, not an inlined function: the existing
// instantiations compile to the instructions they compiled to before the second entry point existed (an inlined body did not: tools/asm_same.py).
    static_assert(!ENS || CW == 16, "ensembles run the 16-column tiles");
    static_assert(!CONV || CW == 16, "the conv network runs the 16-column tiles");
    if constexpr (ENS) {
        const size_t k = blockIdx.y;
        if constexpr (SPLIT) imgf = reinterpret_cast<const u32*>(imgf) + k * en.simg;
        else imgf = reinterpret_cast<const float*>(imgf) + k * en.img;
        bias += k * en.bias;
        x0 += k * en.x0;
        if (sol) sol += k * en.sol;
        if constexpr (TAPE) {
            dwtape += k * en.dwtape;
            masks += k * en.masks;
            if constexpr (CA) swtape += k * en.swtape;
        }
    }
    // Save intervals [iv_begin, iv_end) of the time axis, starting from x0 (column stride x0_stride: the initial state, or — a time SEGMENT
    // of the gradient path — the state the tape-less pass saved at save point iv_begin; restarting there is exact: the saved state IS xn).
    // Only the intervals from tape_iv0 on are taped (the records are numbered from its first step): the tape-less pass of a time-segmented
    // gradient tapes its LAST segment on the way, which that segment's own pass would otherwise have to repeat.
    using S = Fc<NZ, CW>;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & (CW - 1), h = lane / CW;               // column of the tile; k / row quad
    float* X = fc_smem;                          // [32][LDX]   stage input
    float* A1 = X + CW * S::LDX;                 // [32][LDH]   relu(W1 x + b1)
    float* A2 = A1 + CW * S::LDH;                // [32][LDH]   relu(W2 a1 + b2)
    float* PART = A1;                            // [KS3][32][NZ] partial sums of the last layer (a1 is dead by then)
    float* BL = A2 + CW * S::LDH;                // [2H + NZ] biases (a global load in an epilogue would be waited for with vmcnt(0): the ring too)
    for (int q = tid; q < S::BIAS; q += 256) BL[q] = bias[q];
    const int col0 = blockIdx.x * CW;
    FC_OWNER_INDEX();

    typedef FcStream<NZ, CW, SPLIT> Stream;
    Stream strm;
    strm.init(imgf, w, lane);

    float xn[S::OWN], vst[S::OWN], kv[S::OWN], bcb[S::OWN], bct[S::OWN];
#pragma unroll
    for (int r = 0; r < S::OWN; r++) {
        const int col = min(col0 + oc[r], n_col - 1);
        xn[r] = x0[(size_t)col * x0_stride + oi];
        bcb[r] = bcs[(size_t)col * 2];
        bct[r] = bcs[(size_t)col * 2 + 1];
        kv[r] = 0.0f;
        if (sol && iv_begin == 0 && col0 + oc[r] < n_col) sol[((size_t)(col0 + oc[r]) * n_save) * NZ + oi] = xn[r];
    }
    const float b3v = oi < S::NO ? bias[2 * S::H + oi] : 0.0f;
    // every load issued so far is consumed HERE: a register still "in flight" at the loop header makes the wait-count pass put a
    // vmcnt(0) at the top of every stage, which would drain the prefetch ring each time
#pragma unroll
    for (int r = 0; r < S::OWN; r++) asm volatile("" :: "v"(xn[r]), "v"(bcb[r]), "v"(bct[r]));
    asm volatile("" :: "v"(b3v));
    float cwv[FC_CONV_MAX], cbv = 0.0f;          // CONV: the filter, read and consumed here (the same rule)
    if constexpr (CONV) fc_conv_load(cv, cwv, cbv);
    const int n_steps = (iv_end - tape_iv0) * substeps;          // taped steps (and, x nst, records per tile) of this launch
    const int step_t0 = (tape_iv0 - iv_begin) * substeps;         // first taped step

    // one right-hand-side evaluation: stage input vst[] (owner layout) -> kv[]; qi = record index step * nst + st
    auto rhs = [&](int qs) {
        const int qi = qs - step_t0 * nst;
        const bool tp = TAPE && qi >= 0;                              // wave-uniform
        int zero = 0;
        FC_OPAQUE_ZERO(zero);
        const typename Stream::slot_t* const sb[3] = {strm.base[0] + zero, strm.base[1] + zero, strm.base[2] + zero};
        const size_t ri = (size_t)blockIdx.x * n_steps * nst + qi;
        float* rec = tp ? dwtape + ri * ((size_t)CW * S::R) : nullptr;
        u32* mrec = tp ? masks + ri * 512 + w * 64 + lane : nullptr;
        // ---- stage input (owner layout) -> LDS rows, tape
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            if constexpr (CONV) {
                // y = relu(filter) on the M = NZ - c + 1 levels it covers, zero above: the layer-1 input, in LDS and in the dW record.  A shift past the
                // column's last lane reads the lane's own value (NZ = 64) or the wave's other column (NZ = 32): only at levels oi >= M, which are zeroed.
                // (the filter length and the level through the stage's opaque zero: left loop-invariant, the optimiser keeps one lane mask per tap
                //  and per comparison in scalar registers across the whole time loop and spills them)
                const int cc = cv.c + zero, oio = oi + zero;
                const float pre = fc_conv_pre(vst[r], cwv, cbv, cc);
                // (a conv ensemble lets a NaN pre-activation through, as Flux's relu = max(0, x) does: a member whose filter went NaN must show as a
                //  non-finite row, not as a silent all-zero filter output.  Finite values: the same bits either way.)
                const float y = (oio <= NZ - cc && (ENS ? !(pre <= 0.0f) : pre > 0.0f)) ? pre : 0.0f;
                X[oc[r] * S::LDX + oi] = y;
                if (tp) {
                    FC_STORE(y, rec + (size_t)oc[r] * S::R + oi);
                    FC_STORE(vst[r], cv.ctape + ri * (size_t)(CW * 2 * NZ) + oc[r] * (2 * NZ) + oi);
                }
            } else {
                X[oc[r] * S::LDX + oi] = vst[r];
                if (tp) FC_STORE(vst[r], rec + (size_t)oc[r] * S::R + oi);
            }
        }
        FC_BARRIER();
        // ---- hidden layers: z = W a + b on 32x32x2 MFMA, relu, rows to LDS (next layer's B operand) and to the tape
        auto hidden = [&](int l /* 1, 2 */, float* dstrows, int j, const typename S::acc_t& acc) {
            const int mt = w + 4 * j;
            u32 bits = 0;
#pragma unroll
            for (int q = 0; q < S::NQ; q++) {
                const int f = mt * CW + S::qrow(q, h);
                const f32x4 bq = *reinterpret_cast<const f32x4*>(BL + (l - 1) * S::H + f);
                f32x4 a;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float z = acc[4 * q + e] + bq[e];
                    a[e] = fmaxf(z, 0.0f);
                    bits |= (z > 0.0f ? 1u : 0u) << (4 * q + e);
                }
                *reinterpret_cast<f32x4*>(dstrows + n * S::LDH + f) = a;
                if (tp) FC_STORE(a, reinterpret_cast<f32x4*>(rec + (size_t)n * S::R + NZ + (l - 1) * S::H + f));
            }
            return bits;
        };
        {
            u32 mb = 0;
            strm.template section<0>(sb, lane, h, w, X + n * S::LDX,
                                     [&](int j, const typename S::acc_t& acc) { mb |= hidden(1, A1, j, acc) << (S::ACCN * j); });
            if (tp) FC_STORE(mb, mrec);
        }
        FC_BARRIER();
        {
            u32 mb = 0;
            strm.template section<1>(sb, lane, h, w, A1 + n * S::LDH,
                                     [&](int j, const typename S::acc_t& acc) { mb |= hidden(2, A2, j, acc) << (S::ACCN * j); });
            if (tp) FC_STORE(mb, mrec + 256);
        }
        FC_BARRIER();
        // ---- output layer: row tile w % MT3, K part w / MT3; partial sums to LDS
        strm.template section<2>(sb, lane, h, w, A2 + n * S::LDH,
            [&](int, const typename S::acc_t& acc) {
                float* pr = PART + ((w / S::MT3) * CW + n) * NZ + (w % S::MT3) * CW;
#pragma unroll
                for (int q = 0; q < S::NQ; q++) {
                    const f32x4 v = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
                    *reinterpret_cast<f32x4*>(pr + S::qrow(q, h)) = v;
                }
            });
        FC_BARRIER();
        // ---- physics: faces F = [b; NN(T); t] (free_convection_nde.jl:29-38) [- min(0, K dT/dz) on the interior faces,
        //      convective_adjustment_nde.jl:43-47], dT = -C Nz (F[i+1] - F[i])
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            float o = b3v;
#pragma unroll
            for (int ks = 0; ks < S::KS3; ks++) o += PART[(ks * CW + oc[r]) * NZ + oi];
            const float olo = __shfl_up(o, 1);                                // NN output of face i (lane i - 1 holds it)
            float wlo = oi == 0 ? bcb[r] : olo;
            float whi = oi == NZ - 1 ? bct[r] : o;
            if (CA) {
                const float vlo = __shfl_up(vst[r], 1), vhi = __shfl_down(vst[r], 1);
                const float glo = (vst[r] - vlo) * (float)NZ, ghi = (vhi - vst[r]) * (float)NZ;     // dT/dz on faces i and i + 1
                const bool on = oi >= 1 && glo < 0.0f;
                if (oi >= 1) wlo -= fminf(0.0f, caKN * (vst[r] - vlo));
                if (oi <= NZ - 2) whi -= fminf(0.0f, caKN * (vhi - vst[r]));
                (void)ghi;
                if (tp) {
                    // the switch pattern of the stage, one bit per face, for the pullback
                    const u64 bal = __ballot(on);
                    const u64 mine = NZ == 64 ? bal : (lane < 32 ? (bal & 0xffffffffull) : (bal >> 32));
                    if (oi == 0) swtape[ri * CW + oc[r]] = mine;
                }
            }
            kv[r] = -CN * (whi - wlo);
        }
    };

    int step = 0;
    if constexpr (!RKC) {
        float ac[S::OWN];
#pragma unroll
        for (int r = 0; r < S::OWN; r++) ac[r] = 0.0f;
        for (int iv = iv_begin; iv < iv_end; iv++) {
            const float dt = (save_times[iv + 1] - save_times[iv]) / (float)substeps;
            for (int s = 0; s < substeps; s++, step++) {
#pragma nounroll
                for (int st = 0; st < 4; st++) {
                    const float ca = st == 0 ? 0.0f : (st == 3 ? 1.0f : 0.5f);            // stage abscissa
                    const float cbp = st == 1 ? 1.0f / 6.0f : 1.0f / 3.0f;                 // RK4 weight of k_{st-1}
#pragma unroll
                    for (int r = 0; r < S::OWN; r++) {
                        float v = xn[r];
                        if (st > 0) {
                            ac[r] += cbp * kv[r];
                            v += ca * dt * kv[r];
                        }
                        vst[r] = v;
                    }
                    rhs(step * 4 + st);
                }
                const bool save = s == substeps - 1;
#pragma unroll
                for (int r = 0; r < S::OWN; r++) {
                    ac[r] += (1.0f / 6.0f) * kv[r];
                    xn[r] += dt * ac[r];
                    ac[r] = 0.0f;
                    if (save && sol && col0 + oc[r] < n_col) sol[((size_t)(col0 + oc[r]) * n_save + iv + 1) * NZ + oi] = xn[r];
                }
            }
        }
    } else {
        // Y_0 = xn, d_j = Y_j - Y_0 (increments: float32 stays accurate), F_0 = f0; stage st evaluates F_st = f(Y_st); Y_s ends the step
        const float* mu_t = rkc, *nu_t = rkc + RKC_LD, *mut_t = rkc + 2 * RKC_LD, *gat_t = rkc + 3 * RKC_LD;
        float ym1[S::OWN], ym2[S::OWN], f0[S::OWN];
#pragma unroll
        for (int r = 0; r < S::OWN; r++) { ym1[r] = 0.0f; ym2[r] = 0.0f; f0[r] = 0.0f; }
        for (int iv = iv_begin; iv < iv_end; iv++) {
            const float dt = (save_times[iv + 1] - save_times[iv]) / (float)substeps;
            for (int s = 0; s < substeps; s++, step++) {
#pragma nounroll
                for (int st = 0; st <= nst; st++) {      // st = nst: only the final combination Y_s
                    const float cmu = mu_t[st], cnu = nu_t[st], cmt = mut_t[st] * dt, cga = gat_t[st] * dt;
                    const bool last = st == nst;
                    const bool save = last && s == substeps - 1;
#pragma unroll
                    for (int r = 0; r < S::OWN; r++) {
                        float dj = 0.0f;
                        if (st == 1) {
                            f0[r] = kv[r];
                            dj = cmt * f0[r];
                        } else if (st >= 2) {
                            dj = cmu * ym1[r] + cnu * ym2[r] + cmt * kv[r] + cga * f0[r];
                        }
                        const float v = xn[r] + dj;
                        ym2[r] = st == 0 ? 0.0f : ym1[r];
                        ym1[r] = dj;
                        if (last) {
                            xn[r] = v;
                            if (save && sol && col0 + oc[r] < n_col) sol[((size_t)(col0 + oc[r]) * n_save + iv + 1) * NZ + oi] = v;
                        } else {
                            vst[r] = v;
                        }
                    }
                    if (last) break;
                    rhs(step * nst + st);
                }
            }
        }
    }
