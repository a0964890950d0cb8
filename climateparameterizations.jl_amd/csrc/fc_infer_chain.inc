// fc_infer_chain.inc — the three dense layers of one tile of the embedded inference, X -> A1 -> A2 -> PART: included as TEXT in the tile loop of
// fc_infer_kernel (engine_fc.hip) and fce_kernel (engine_fc_embed.hip), after the barrier that publishes X; ends with the barrier that publishes
// PART.  Text rather than a function, so that the code the compiler sees in fc_infer_kernel is what it was before the code was shared (a
// function changes the order of its address arithmetic).  In scope: S = Fc<NZ, CW>, ring, sb, lane, w, n, h, X, A1, A2, PART, BL.
        auto hidden = [&](int l, float* dstrows, int j, const typename S::acc_t& acc) {
            const int mt = w + 4 * j;
#pragma unroll
            for (int q = 0; q < S::NQ; q++) {
                const int f = mt * CW + S::qrow(q, h);
                const f32x4 bq = *reinterpret_cast<const f32x4*>(BL + (l - 1) * S::H + f);
                f32x4 a;
#pragma unroll
                for (int e = 0; e < 4; e++) a[e] = fmaxf(acc[4 * q + e] + bq[e], 0.0f);
                *reinterpret_cast<f32x4*>(dstrows + n * S::LDH + f) = a;
            }
        };
        fc_section<NZ, CW, 0, S::JH, S::S_IN>(ring, sb, lane, X + n * S::LDX + 4 * h, [&](int j, const typename S::acc_t& acc) { hidden(1, A1, j, acc); });
        FC_BARRIER();
        fc_section<NZ, CW, S::JH * S::S_IN, S::JH, S::S_H>(ring, sb, lane, A1 + n * S::LDH + 4 * h, [&](int j, const typename S::acc_t& acc) { hidden(2, A2, j, acc); });
        FC_BARRIER();
        fc_section<NZ, CW, S::JH * (S::S_IN + S::S_H), 1, S::G3>(ring, sb, lane, A2 + n * S::LDH + (w / S::MT3) * S::G3 * S::KG + 4 * h,
            [&](int, const typename S::acc_t& acc) {
                float* pr = PART + ((w / S::MT3) * CW + n) * NZ + (w % S::MT3) * CW;
#pragma unroll
                for (int q = 0; q < S::NQ; q++) {
                    const f32x4 v = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
                    *reinterpret_cast<f32x4*>(pr + S::qrow(q, h)) = v;
                }
            });
        FC_BARRIER();
