// fc_adjoint_body.inc — the text of the fc32 adjoint kernel (engine_fc.hip), included by fc_adjoint_kernel (CONV = false), fc_adjoint_conv_kernel
// (CW = 16, ENS = false, CONV = true) and fc_adjoint_conv_ens_kernel (CW = 16, ENS = CONV = true): see fc_forward_body.inc.
    static_assert(!ENS || CW == 16, "ensembles run the 16-column tiles");
    static_assert(!CONV || CW == 16, "the conv network runs the 16-column tiles");
    if constexpr (ENS) {
        const size_t k = blockIdx.y;
        if constexpr (SPLIT) imgb = reinterpret_cast<const u32*>(imgb) + k * en.simg;
        else imgb = reinterpret_cast<const float*>(imgb) + k * en.img;
        sol += k * en.sol;
        dwtape += k * en.dwtape;
        masks += k * en.masks;
        if constexpr (CA) swtape += k * en.swtape;
        if (lam_io) lam_io += k * en.lam;
        slab += k * en.slab;
    }
    // Save intervals [iv_begin, iv_end), backwards.  lam_io [columns][NZ] (or null: one launch covers the axis) carries λ from one time
    // segment to the one before it: read unless this is the last segment of the axis, written unless it is the first.
    using S = Fc<NZ, CW>;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & (CW - 1), h = lane / CW;               // column of the tile; k / row quad
    float* DZ2 = fc_smem;                        // [32][LDH]
    float* DZ1 = DZ2 + CW * S::LDH;              // [32][LDH]
    float* DZ3 = DZ1;                            // [32][LDX]   dead before dz1 is written
    float* XBP = DZ2;                            // [KS3][32][NZ] partial sums of W1ᵀ dz1 (dz2 is dead by then)
    const int col0 = blockIdx.x * CW;
    FC_OWNER_INDEX();

    typedef FcStream<NZ, CW, SPLIT> Stream;
    Stream strm;
    strm.init(imgb, w, lane);

    float lam[S::OWN], xb[S::OWN], kb[S::OWN], db3[S::OWN];
    u32 swp = 0;                                 // switch bits of this thread's items: bit 2r = face oi, bit 2r + 1 = face oi + 1 of item r
    float db2 = 0.0f, db1 = 0.0f;                // bias gradients of hidden unit tid (< H): column sums of the dz rows, taken from LDS
    float sumsq = 0.0f;
    // ENS, a member loss (FcEns::member_w / member_colw; colnde_ensemble_set_member_loss): the model's own loss weight in w_loss' place and the weight
    // of every column of the tile.  The 16 weights are loaded here, before the first save point's reads, and parked in LDS (64 bytes of static LDS, the
    // ENS instantiations only): the load is consumed by its LDS write (the forward kernel's rule: a register still in flight at the loop header puts a
    // vmcnt(0) at the top of every stage), no register and no pointer stays live across the stage loop, and an injection reads its weights back with
    // LDS reads at immediate offsets from one address, formed where it is used (FC_MEMBER_CW: owned column r = tid / NZ + (256 / NZ) r; the opaque zero
    // keeps the address from being hoisted into a register that would live through the stage loop).  cw d is formed first: the injection takes it, the
    // sum (cw d) d — without a member loss cw = 1 and both are the unweighted operations, bit for bit.
#define FC_MEMBER_CW(p)                \
    const float* p = nullptr;          \
    if constexpr (ENS) {               \
        int zcw = 0;                   \
        FC_OPAQUE_ZERO(zcw);           \
        p = cwl + (tid + zcw) / NZ;    \
    }
    float wl = w_loss;
    float* cwl = nullptr;
    // CONV + ENS: the filter is read in front of the member block — behind its barrier (a memory clobber) the compiler no longer takes the taps for
    // invariant and fetches them with vector loads into nine registers per lane, where scalar loads kept them in SGPRs
    float cwv[FC_CONV_MAX], cbv = 0.0f;
    if constexpr (CONV && ENS) fc_conv_load(cv, cwv, cbv);
    if constexpr (ENS) {
        __shared__ float fc_member_cw[CW];
        cwl = fc_member_cw;
        if (en.member_w) wl = en.member_w[(size_t)blockIdx.y * 8];
        if (tid < CW) fc_member_cw[tid] = (en.member_colw && col0 + tid < n_col) ? en.member_colw[(size_t)blockIdx.y * n_col + col0 + tid] : 1.0f;
        FC_BARRIER();
    }
    {
        FC_MEMBER_CW(cwp);
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            lam[r] = 0.0f; xb[r] = 0.0f; db3[r] = 0.0f; kb[r] = 0.0f;
            if (lam_io && iv_end < n_save - 1) lam[r] = lam_io[(size_t)(col0 + oc[r]) * NZ + oi];
            if (iv_begin == 0 && col0 + oc[r] < n_col) {                // save point 0 enters the loss value only
                const size_t q = ((size_t)(col0 + oc[r]) * n_save) * NZ + oi;
                const float d = sol[q] - truth[q];
                if constexpr (ENS) sumsq += (cwp[(256 / NZ) * r] * d) * d;
                else sumsq += d * d;
            }
        }
    }
    const int n_steps = (iv_end - iv_begin) * substeps;          // steps (and, x nst, records per tile) of this launch
    if constexpr (CONV && !ENS) fc_conv_load(cv, cwv, cbv);

    // pullback of one right-hand-side evaluation: stage cotangent kb[] (owner layout) -> xb[] = J(Y)ᵀ kb; qi = record index
    auto pull = [&](int qi) {
        int zero = 0;
        FC_OPAQUE_ZERO(zero);
        const typename Stream::slot_t* const sb[3] = {strm.base[0] + zero, strm.base[1] + zero, strm.base[2] + zero};
        const size_t ri = (size_t)blockIdx.x * n_steps * nst + qi;
        float* rec = dwtape + ri * ((size_t)CW * S::R);
        const u32* mrec = masks + ri * 512 + w * 64 + lane;
        const u32 m1 = FC_LOAD(mrec), m2 = FC_LOAD(mrec + 256);
        float xc[S::OWN];                                                         // CONV: the stage input, requested here, used after the last section
        if constexpr (CONV) {
#pragma unroll
            for (int r = 0; r < S::OWN; r++) xc[r] = FC_LOAD(cv.ctape + ri * (size_t)(CW * 2 * NZ) + oc[r] * (2 * NZ) + oi);
        }
        // ---- physics pullback: dz3[i] = C Nz (k̄[i+1] - k̄[i]) on the Nz-1 interior faces; CA: x̄ += Dᶠᵀ(switch ∘ (-K) ∘ that)
        float xph[S::OWN];
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            const float kn = __shfl_down(kb[r], 1);
            const float dz = oi < S::NO ? CN * (kn - kb[r]) : 0.0f;                 // face i + 1
            xph[r] = 0.0f;
            if (CA) {
                const float dlo = __shfl_up(dz, 1);                                 // face i
                const float ghi = (oi < S::NO && ((swp >> (2 * r + 1)) & 1u)) ? -dz * caKN : 0.0f;
                const float glo = (oi >= 1 && ((swp >> (2 * r)) & 1u)) ? -dlo * caKN : 0.0f;
                xph[r] = glo - ghi;
            }
            DZ3[oc[r] * S::LDX + oi] = dz;
            FC_STORE(dz, rec + (size_t)oc[r] * S::R + NZ + S::ACT4 + 2 * S::H + oi);
            db3[r] += dz;
        }
        FC_BARRIER();
        auto hidden = [&](int l /* 2, 1: layer whose dz this is */, float* dstrows, u32 bits, int j, const typename S::acc_t& acc) {
            const int mt = w + 4 * j;
#pragma unroll
            for (int q = 0; q < S::NQ; q++) {
                f32x4 d;
#pragma unroll
                for (int e = 0; e < 4; e++) d[e] = ((bits >> (S::ACCN * j + 4 * q + e)) & 1u) ? acc[4 * q + e] : 0.0f;
                const int f = mt * CW + S::qrow(q, h);
                *reinterpret_cast<f32x4*>(dstrows + n * S::LDH + f) = d;
                FC_STORE(d, reinterpret_cast<f32x4*>(rec + (size_t)n * S::R + NZ + S::ACT4 + (l - 1) * S::H + f));
            }
        };
        // ---- dz2 = relu'(z2) ∘ W3ᵀ dz3
        strm.template section<0>(sb, lane, h, w, DZ3 + n * S::LDX,
                                          [&](int j, const typename S::acc_t& acc) { hidden(2, DZ2, m2, j, acc); });
        FC_BARRIER();
        // bias gradients: hidden unit tid's column sum of the finished dz rows, straight from LDS (16 accumulator registers per row tile
        // and layer — 64 at Nz = 64 — would otherwise ride along in every lane)
        auto colsum = [&](const float* rows) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
            for (int c = 0; c < CW; c += 4) {
                a0 += rows[(c + 0) * S::LDH + tid];
                a1 += rows[(c + 1) * S::LDH + tid];
                a2 += rows[(c + 2) * S::LDH + tid];
                a3 += rows[(c + 3) * S::LDH + tid];
            }
            return (a0 + a1) + (a2 + a3);
        };
        if (S::H == 256 || tid < S::H) db2 += colsum(DZ2);
        // ---- dz1 = relu'(z1) ∘ W2ᵀ dz2
        strm.template section<1>(sb, lane, h, w, DZ2 + n * S::LDH,
                                                       [&](int j, const typename S::acc_t& acc) { hidden(1, DZ1, m1, j, acc); });
        FC_BARRIER();
        if (S::H == 256 || tid < S::H) db1 += colsum(DZ1);
        // ---- x̄ = W1ᵀ dz1: row tile w % MT3, K part w / MT3
        strm.template section<2>(sb, lane, h, w, DZ1 + n * S::LDH,
            [&](int, const typename S::acc_t& acc) {
                float* pr = XBP + ((w / S::MT3) * CW + n) * NZ + (w % S::MT3) * CW;
#pragma unroll
                for (int q = 0; q < S::NQ; q++) {
                    const f32x4 v = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
                    *reinterpret_cast<f32x4*>(pr + S::qrow(q, h)) = v;
                }
            });
        FC_BARRIER();
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            if constexpr (CONV) {
                float yb = 0.0f;                                                  // ȳ = W1ᵀ dz1 (zero on the padded levels: W1's padded columns are zero)
#pragma unroll
                for (int ks = 0; ks < S::KS3; ks++) yb += XBP[(ks * CW + oc[r]) * NZ + oi];
                const int cc = cv.c + zero, oio = oi + zero;                     // (through the opaque zero: see the forward kernel)
                const float pre = fc_conv_pre(xc[r], cwv, cbv, cc);
                const float zb = (oio <= NZ - cc && (ENS ? !(pre <= 0.0f) : pre > 0.0f)) ? yb : 0.0f;      // (the forward's predicate)
                FC_STORE(zb, cv.ctape + ri * (size_t)(CW * 2 * NZ) + oc[r] * (2 * NZ) + NZ + oi);
                float v = xph[r];
#pragma unroll
                for (int d = 0; d < FC_CONV_MAX; d++)
                    if (d < cc) {
                        const float zs = __shfl_up(zb, d);                        // level oi - d of this column (below level 0: dropped)
                        if (oio >= d) v = fmaf(cwv[d], zs, v);
                    }
                xb[r] = v;
            } else {
                float v = xph[r];
#pragma unroll
                for (int ks = 0; ks < S::KS3; ks++) v += XBP[(ks * CW + oc[r]) * NZ + oi];
                xb[r] = v;
            }
        }
        // (the next evaluation writes DZ3 = DZ1's rows: every wave's reads of DZ1 ended before the barrier above; XBP = DZ2's rows
        //  are next written two barriers from here)
    };
    auto load_switch = [&](int qi) {
        if (CA) {
            const size_t ri = (size_t)blockIdx.x * n_steps * nst + qi;
            swp = 0;
#pragma unroll
            for (int r = 0; r < S::OWN; r++) swp |= (u32)((swtape[ri * CW + oc[r]] >> oi) & 3ull) << (2 * r);
        }
    };

    const float* mu_t = rkc, *nu_t = rkc + RKC_LD, *mut_t = rkc + 2 * RKC_LD, *gat_t = rkc + 3 * RKC_LD, *kap_t = rkc + 5 * RKC_LD;
    float xbs[S::OWN], yb1[S::OWN], yb2[S::OWN], yb0[S::OWN], f0b[S::OWN];
#pragma unroll
    for (int r = 0; r < S::OWN; r++) { xbs[r] = 0.0f; yb1[r] = 0.0f; yb2[r] = 0.0f; yb0[r] = 0.0f; f0b[r] = 0.0f; }
    for (int iv = iv_end - 1; iv >= iv_begin; iv--) {
        const float dt = (save_times[iv + 1] - save_times[iv]) / (float)substeps;
        // λ += ∂loss/∂sol[:, iv+1]   (nde_loss = Flux.mse over every (level, save point, simulation): training.jl:55-62)
        FC_MEMBER_CW(cwp);
#pragma unroll
        for (int r = 0; r < S::OWN; r++)
            if (col0 + oc[r] < n_col) {
                const size_t q = ((size_t)(col0 + oc[r]) * n_save + iv + 1) * NZ + oi;
                const float d = sol[q] - truth[q];
                if constexpr (ENS) {
                    const float dw = cwp[(256 / NZ) * r] * d;
                    sumsq += dw * d;
                    lam[r] += 2.0f * wl * dw;
                } else {
                    sumsq += d * d;
                    lam[r] += 2.0f * w_loss * d;
                }
            }
        for (int s = substeps - 1; s >= 0; s--) {
            const int step = (iv - iv_begin) * substeps + s;
            if constexpr (!RKC) {
#pragma unroll
                for (int r = 0; r < S::OWN; r++) xbs[r] = 0.0f;
#pragma nounroll
                for (int st = 3; st >= 0; st--) {
                    // k̄4 = dt/6 λ; k̄3 = dt/3 λ + dt x̄4; k̄2 = dt/3 λ + dt/2 x̄3; k̄1 = dt/6 λ + dt/2 x̄2
                    const float cwl = (st == 0 || st == 3) ? dt / 6.0f : dt / 3.0f;
                    const float cwx = st == 3 ? 0.0f : (st == 2 ? dt : 0.5f * dt);
#pragma unroll
                    for (int r = 0; r < S::OWN; r++) kb[r] = cwl * lam[r] + cwx * xb[r];
                    load_switch(step * 4 + st);                 // RK4: every stage's own pattern (the exact discrete adjoint)
                    pull(step * 4 + st);
#pragma unroll
                    for (int r = 0; r < S::OWN; r++) xbs[r] += xb[r];
                }
#pragma unroll
                for (int r = 0; r < S::OWN; r++) lam[r] += xbs[r];
            } else {
                load_switch(step * nst + nst - 1);              // one switch pattern per step: that of Y_{s-1}
#pragma nounroll
                for (int st = nst - 1; st >= 0; st--) {
                    // stage input Y_st feeds Y_j, j = st + 1, through mu~_j h F_st
                    const float cmu = mu_t[st + 1], cnu = nu_t[st + 1], cmt = mut_t[st + 1] * dt, cga = gat_t[st + 1] * dt, ck0 = kap_t[st + 1];
#pragma unroll
                    for (int r = 0; r < S::OWN; r++) {
                        // lam = cotangent of Y_j, complete once the previous iteration's pullback (xb: J(Y_j)ᵀ F̄_j) is added
                        if (st < nst - 1) {
                            const float yj = yb1[r] + xb[r];
                            yb1[r] = yb2[r];
                            yb2[r] = 0.0f;
                            lam[r] = yj;
                        }
                        if (st >= 1) {
                            yb0[r] += ck0 * lam[r];
                            yb1[r] += cmu * lam[r];
                            yb2[r] += cnu * lam[r];
                            f0b[r] += cga * lam[r];
                            kb[r] = cmt * lam[r];
                        } else {
                            // Y_1 = Y_0 + mu~_1 h F_0: lam holds Ȳ_1, yb1 the nu_2 part of Ȳ_0
                            yb0[r] += lam[r] + yb1[r];
                            kb[r] = f0b[r] + cmt * lam[r];
                            yb1[r] = 0.0f;
                            f0b[r] = 0.0f;
                        }
                    }
                    pull(step * nst + st);
                }
                // λ_n = Ȳ_0 + J(Y_0)ᵀ F̄_0
#pragma unroll
                for (int r = 0; r < S::OWN; r++) {
                    lam[r] = yb0[r] + xb[r];
                    yb0[r] = 0.0f;
                }
            }
        }
    }
    if (lam_io && iv_begin > 0)
#pragma unroll
        for (int r = 0; r < S::OWN; r++) lam_io[(size_t)(col0 + oc[r]) * NZ + oi] = lam[r];
    // ---- flush: bias gradients and the loss sum into this workgroup's slab row (weight gradients come from the dW GEMM)
    FC_BARRIER();
    float* out = slab + (size_t)blockIdx.x * (go.n_params + 8);
    float* scr = fc_smem;                                            // [4][NZ] + [4]
    {
        float s3 = 0.0f;
#pragma unroll
        for (int r = 0; r < S::OWN; r++) s3 += db3[r];              // this thread's columns, level oi
        if (NZ == 32) s3 += __shfl_down(s3, 32);                     // the wave's second column group
        if (lane < NZ) scr[w * NZ + lane] = s3;
        float v = sumsq;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) scr[4 * NZ + w] = v;
    }
    FC_BARRIER();
    if (tid < S::NO) out[go.b[2] + tid] = (scr[tid] + scr[NZ + tid]) + (scr[2 * NZ + tid] + scr[3 * NZ + tid]);
    if (tid == 0) out[go.n_params + 2] = (scr[4 * NZ] + scr[4 * NZ + 1]) + (scr[4 * NZ + 2] + scr[4 * NZ + 3]);
    if (tid < S::H) {
        out[go.b[0] + tid] = db1;
        out[go.b[1] + tid] = db2;
    }
#undef FC_MEMBER_CW
