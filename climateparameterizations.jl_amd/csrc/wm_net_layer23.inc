// wm_net_layer23.inc — layers 2 and 3 of flux network n on one 32-column tile, from the stacked layer-1 tiles acc1[5] (wm_net_layer1.inc).
// Included textually inside the loop over n by wm_infer_tile.inc and engine_wm_profile.hip.  The including scope provides wl, a2, a3, h, S.act2, n;
// it leaves y: row rho(r, h) = the network's output on interior face rho + 1 (row 31: padding).
            // ---- layer 2: 25 k-steps over this net's registers of the stacked tiles
            wm_f32x16 acc2;
#pragma unroll
            for (int r = 0; r < 16; r++) acc2[r] = r < 10 ? wl[n * WM_NET + WM_OFF_B2 + 2 * r + h] : 0.0f;
#pragma unroll
            for (int s = 0; s < 25; s++) {
                const int G = 25 * n + s;
                acc2 = wm_mfma(wl[n * WM_NET + a2 + 2 * WM_H2 * s], acc1[G >> 4][G & 15], acc2);
            }
            // ---- layer 3: 10 k-steps; row rho(r, h) = interior face (row 31: padding)
            wm_f32x16 y;
#pragma unroll
            for (int r = 0; r < 16; r++) y[r] = wl[n * WM_NET + WM_OFF_B3 + min(WM_RHO0(r) + 4 * h, 30)];
#pragma unroll
            for (int s = 0; s < 10; s++) y = wm_mfma(wl[n * WM_NET + a3 + 62 * s], dev_act(S.act2, acc2[s]), y);
