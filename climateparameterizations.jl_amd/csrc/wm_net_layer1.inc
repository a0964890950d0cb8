// wm_net_layer1.inc — layer 1 of the three wind-mixing flux networks on one 32-column tile, stacked (they share the input): 5 tiles x 48 k-steps of
// v_mfma_f32_32x32x2_f32, then the activation.  Included textually by wm_infer_tile.inc and engine_wm_profile.hip.  The including scope provides
// wl (the weight image in LDS), a1[5], h, S.act1 and xs[48] (the networks' input in the B layout); it leaves acc1[5].
        wm_f32x16 acc1[5];
#pragma unroll
        for (int tl = 0; tl < 5; tl++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int G = 16 * tl + r < 75 ? 16 * tl + r : 74;
                acc1[tl][r] = wl[(G / 25) * WM_NET + WM_OFF_B1 + 2 * (G % 25) + h];
            }
#pragma unroll
        for (int s = 0; s < 48; s++) {
            const int in0 = 32 * (s >> 4) + WM_RHO0(s & 15);
#pragma unroll
            for (int tl = 0; tl < 5; tl++) acc1[tl] = wm_mfma(wl[a1[tl] + WM_H1 * in0], xs[s], acc1[tl]);
        }
#pragma unroll
        for (int tl = 0; tl < 5; tl++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc1[tl][r] = dev_act(S.act1, acc1[tl][r]);
