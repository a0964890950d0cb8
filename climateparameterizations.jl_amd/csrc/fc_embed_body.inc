// fc_embed_body.inc — the text of the free-convection embedded step (engine_fc_embed.hip), included by its two entry points: fce_kernel (any tile
// width, CONV = false) and fce_ens_kernel (CW = 16; the arguments already offset to the workgroup's model; CONV: the filter's taps in `conv_taps`,
// its length in `conv_c`).  Textual inclusion, not an inlined function, as fc_forward_body.inc: fce_kernel's instantiations compile to the
// instructions they compiled to before the second entry point existed (tools/asm_same.py, DESIGN §4p).
    static_assert(STEP || DIAG, "nothing to do");
    static_assert(!CONV || CW == 16, "the conv network runs the 16-column tiles");
    using S = Fc<NZ, CW>;
    constexpr int LDT = NZ + 1;                                  // raw rows: odd stride, conflict-free per-lane column walks (as convadj_kernel)
    static_assert(2 * CW * LDT <= CW * S::LDH, "the raw and the adjusted rows live in A2's rows");
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & (CW - 1), h = lane / CW;               // column of the tile; k / row quad
    float* X = fce_smem;
    float* A1 = X + CW * S::LDX;
    float* A2 = A1 + CW * S::LDH;
    float* PART = A1;
    float* BL = A2 + CW * S::LDH;
    float* HB = BL + S::BIAS;                                    // [CW] halo cell below k = 0 (absent: T[0])
    float* HT = HB + CW;                                         // [CW] halo cell above k = NZ - 1 (absent: T[NZ-1])
    float* TR = A2;                                              // [CW][LDT] T as given
    float* TS = A2 + CW * LDT;                                   // [CW][LDT] a second copy, solved in place: T′
    for (int q = tid; q < S::BIAS; q += 256) BL[q] = bias[q];
    FC_OWNER_INDEX();
    const f32x4* base[3];
    base[0] = reinterpret_cast<const f32x4*>(imgf + S::F1) + (w * S::S_IN) * 64;
    base[1] = reinterpret_cast<const f32x4*>(imgf + S::F2) + (w * S::S_H) * 64;
    base[2] = reinterpret_cast<const f32x4*>(imgf + S::F3) + ((w % S::MT3) * S::S_H + (w / S::MT3) * S::G3) * 64;
    // The A-operand ring streams from one tile to the next, as in fc_infer_kernel — except (Nz = 64, 16 columns, with the sweep): the sweep's 3 x 64
    // live floats and the ring's 32 registers do not fit 256 registers together (36 bytes of scratch), so there the ring is refilled after the sweep
    // of every tile (what the last groups of the previous tile prefetched is dropped: the L2 latency shows once per tile, under the other workgroup).
    constexpr bool REFILL = STEP && NZ == 64 && CW == 16;
    f32x4 ring[FC_PF];
    if constexpr (!REFILL) {
#pragma unroll
        for (int q = 0; q < FC_PF; q++) ring[q] = (base[fc_sec<NZ, CW>(q)] + fc_off<NZ, CW>(q))[lane];
    }
    const float b3v = oi < S::NO ? bias[2 * S::H + oi] : 0.0f;
    asm volatile("" :: "v"(b3v));
    // CONV: the filter as fce_taps_kernel laid it out — cwv[d] multiplies x̃[i + d], zero beyond the filter; cbv = b.  Uniform per workgroup: read
    // through the scalar cache and held in scalar registers across the tile loop (fc_conv_load's vector registers are what (Nz = 64, STEP) lacks).
    float cwv[FC_CONV_MAX], cbv = 0.0f;
    if constexpr (CONV) {
#pragma unroll
        for (int d = 0; d < FC_CONV_MAX; d++) cwv[d] = conv_taps[d];
        cbv = conv_taps[FC_CONV_MAX];
#pragma unroll
        for (int d = 0; d < FC_CONV_MAX; d++) asm volatile("" :: "s"(cwv[d]));
        asm volatile("" :: "s"(cbv));
    }
    const int n_tiles = (n_col + CW - 1) / CW;
#pragma nounroll
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int zero = 0;
        FC_OPAQUE_ZERO(zero);
        const f32x4* const sb[3] = {base[0] + zero, base[1] + zero, base[2] + zero};
        const int col0 = tile * CW;
        // ---- the tile's T: scaled rows (layer 1's B operand), raw rows, halo cells.  A partial tile repeats its last column.
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            const int col = min(col0 + oc[r], n_col - 1);
            const float t = T[(size_t)col * NZ + oi];
            if constexpr (CONV) {
                // y = relu(filter) of the SCALED input on the M = NZ - c + 1 levels it covers, zero above: layer 1's B operand (W1 is padded with zero
                // columns).  A column's levels are consecutive lanes: fc_conv_pre's shifts, the forward solve's instruction sequence and bits.  A shift
                // past the column's last lane lands only in levels oi >= M, which are zeroed.  NaN passes (Flux's relu = max(0, x)), as in a conv
                // ensemble's forward solve.  The raw rows below — the sweep's and the face gradients' — never see the filter.
                const int cc = conv_c + zero, oio = oi + zero;
                const float pre = fc_conv_pre(fc_infer_scale(t, mu_T, inv_sig_T), cwv, cbv, cc);
                X[oc[r] * S::LDX + oi] = (oio <= NZ - cc && !(pre <= 0.0f)) ? pre : 0.0f;
            } else {
                X[oc[r] * S::LDX + oi] = fc_infer_scale(t, mu_T, inv_sig_T);
            }
            TR[oc[r] * LDT + oi] = t;
            if constexpr (STEP) TS[oc[r] * LDT + oi] = t;
            if (oi == 0) HB[oc[r]] = halo_bottom ? halo_bottom[col] : t;
            if (oi == NZ - 1) HT[oc[r]] = halo_top ? halo_top[col] : t;
        }
        FC_BARRIER();
        // ---- convective_adjustment! (:13-40): one lane per column, then T′ out in 16-byte pieces before the chains start
        if constexpr (STEP) {
            if (w == 0 && lane < CW) {
                float* t = TS + lane * LDT;
                const float *halo_bottom = HB, *halo_top = HT;   // (never null here: the load above resolved an absent halo to the interior value)
                const int ca_i = lane;
#include "convadj_sweep.inc"
            }
            FC_BARRIER();
            constexpr int Q = NZ / 4;
#pragma unroll
            for (int e0 = 0; e0 < CW * Q; e0 += 256) {
                const int e = e0 + tid, cl = e / Q, k = (e % Q) * 4;
                if (e < CW * Q) {
                    const float* d = TS + cl * LDT + k;
                    const f32x4 q = {d[0], d[1], d[2], d[3]};
                    if (col0 + cl < n_col) *reinterpret_cast<f32x4*>(T_out + (size_t)(col0 + cl) * NZ + k) = q;
                }
            }
        }
        float tf[S::OWN];
        // ---- diagnose_wT_NN's κ_f ∂T/∂z (:107-115) of this thread's faces oi + 1 (kept for the end) and, oi = 0, face 0 (F[0] = 0: stored now)
        float kg[S::OWN];
        if constexpr (DIAG) {
#pragma unroll
            for (int r = 0; r < S::OWN; r++) {
                const int c = oc[r];
                const float tc = TR[c * LDT + oi];
                const float inside = TR[c * LDT + oi + 1];       // (oi = NZ - 1: the pad float of the row, not used)
                const float up = oi == NZ - 1 ? HT[c] : inside;
                const float g = (up - tc) * inv_dz;
                kg[r] = (g < 0.0f ? K : 0.0f) * g;
                if (oi == 0 && col0 + c < n_col) {
                    const float g0 = (tc - HB[c]) * inv_dz;
                    faces[(size_t)(col0 + c) * (NZ + 1)] = 0.0f - (g0 < 0.0f ? K : 0.0f) * g0;
                }
            }
        }
        // (loaded here, not with T: nothing but the sweep's own registers is live across it)
#pragma unroll
        for (int r = 0; r < S::OWN; r++) tf[r] = top_flux[min(col0 + oc[r], n_col - 1)];
        if constexpr (REFILL) {
#pragma unroll
            for (int q = 0; q < FC_PF; q++) ring[q] = (sb[fc_sec<NZ, CW>(q)] + fc_off<NZ, CW>(q))[lane];
        }
        // ---- the network (layer 2's epilogues overwrite TR and TS: every wave is past the barrier after layer 1 by then)
#include "fc_infer_chain.inc"
#pragma unroll
        for (int r = 0; r < S::OWN; r++) {
            float lo, hi;
            fc_infer_faces<NZ, CW>(PART, oc[r], oi, b3v, sig_wT, mu_wT, tf[r], lo, hi);
            if (col0 + oc[r] < n_col) {
                if constexpr (STEP) dz_wT[(size_t)(col0 + oc[r]) * NZ + oi] = -(hi - lo) * inv_dz_out;
                if constexpr (DIAG) faces[(size_t)(col0 + oc[r]) * (NZ + 1) + oi + 1] = hi - kg[r];
            }
        }
        FC_BARRIER();                                                               // PART (= A1's rows), X, TR are rewritten by the next tile
    }
