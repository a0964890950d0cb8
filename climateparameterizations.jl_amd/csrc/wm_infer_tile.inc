// wm_infer_tile.inc — one 32-column tile of the embedded wind-mixing inference: the body of the group loops of wm_infer_kernel and
// wm_infer_ens_kernel (engine_wm_infer.hip), included textually so both kernels compile the same statements.  The including scope provides:
//   constexpr bool FUSED, DIAG, DZ, RAW;  wl (the weight image in LDS), S, P (this tile's MppParams), dzs[3], fcs[3], uo, vo, To, top,
//   halo_bottom, halo_top, st, n_col, lane, j, h, a1[5], a2, a3, xr (this tile's state, loaded), col0, col, WM_TILE_PREFETCH(): the statement
//   that starts the loads of the NEXT tile's state into xr (or nothing), and WM_TILE_STORE_FACES(o, img, cnt): cnt floats of the wave's LDS image img to o.
        const bool valid = col < n_col;
        // scaled input in the B layout: xs[16 t + 4 q + r] = field t, level rho(4 q + r, h)
        float xs[48];
#pragma unroll
        for (int f = 0; f < 3; f++)
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int r = 0; r < 4; r++) xs[16 * f + 4 * q + r] = (xr[f][q][r] - S.mu[f]) * S.inv_sig[f];

        float raw[RAW ? 48 : 1];                 // the unscaled state: the sweeps' rows, the level differences of the diagnosis
        if (RAW) {
#pragma unroll
            for (int f = 0; f < 3; f++)
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int r = 0; r < 4; r++) raw[(16 * f + 4 * q + r) % (RAW ? 48 : 1)] = xr[f][q][r];
        }
        // the next group's state, in flight under this group's work (one wave per SIMD: nothing else hides the latency; other columns,
        // so in-place outputs do not touch them)
        WM_TILE_PREFETCH();
        if (RAW) WM_WAVE_SYNC();                    // (the previous group's rows have been read out)
        if (FUSED) {
#pragma unroll
            for (int f = 0; f < 3; f++)
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int r = 0; r < 4; r++) st[f * WM_FS + j * WM_LD + 8 * q + 4 * h + r] = raw[(16 * f + 4 * q + r) % (RAW ? 48 : 1)];
            WM_WAVE_SYNC();
            if (h == 0 && valid) mpp_column_step<WM_NZ>(P, st + j * WM_LD, st + WM_FS + j * WM_LD, st + 2 * WM_FS + j * WM_LD, halo_bottom, (size_t)col, n_col);
            WM_WAVE_SYNC();
            float* const dsts[3] = {uo, vo, To};
#pragma unroll
            for (int f = 0; f < 3; f++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int e = i * 64 + lane, cl = e >> 3, k = (e & 7) * 4;
                    if (col0 + cl < n_col) {
                        const float* d = st + f * WM_FS + cl * WM_LD + k;
                        const f32x4 o = {d[0], d[1], d[2], d[3]};
                        *reinterpret_cast<f32x4*>(dsts[f] + (size_t)(col0 + cl) * WM_NZ + k) = o;
                    }
                }
            if (DIAG) WM_WAVE_SYNC();               // (u', v', T' have been read out: the rows take the faces)
        }
        if (DIAG) {
            // ---- ν ∂z u, ν ∂z v, νT ∂z T of the lane's 16 faces (element e: face rho(e, h) + 1) into the rows; face 0 finished here (F = 0)
            float up[3][4];                         // the level above levels 8 q + 4 h + 3: lane ^ 32's first of q (h = 0) or of q + 1 (h = 1)
#pragma unroll
            for (int f = 0; f < 3; f++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float mine = raw[(16 * f + 4 * q) % (RAW ? 48 : 1)], next = q < 3 ? raw[(16 * f + 4 * q + 4) % (RAW ? 48 : 1)] : 0.0f;
                    up[f][q] = __shfl_xor(h == 1 ? mine : next, 32);
                }
            if (h == 1)
#pragma unroll
                for (int f = 0; f < 3; f++)         // above level 31: the halo cell, or the zero-gradient fill
                    up[f][3] = halo_top && valid ? halo_top[(size_t)f * n_col + col] : raw[(16 * f + 15) % (RAW ? 48 : 1)];
#pragma unroll
            for (int e = 0; e < 16; e++) {
                float d[3];
#pragma unroll
                for (int f = 0; f < 3; f++) d[f] = ((e & 3) < 3 ? raw[(16 * f + e + 1) % (RAW ? 48 : 1)] : up[f][e >> 2]) - raw[(16 * f + e) % (RAW ? 48 : 1)];
                float g[3];
                mpp_face_nu_grad(P, S.dz, e == 15 && h == 1, d[0], d[1], d[2], g[0], g[1], g[2]);
#pragma unroll
                for (int f = 0; f < 3; f++) st[f * WM_FS + j * WM_LD + WM_RHO0(e) + 4 * h + 1] = g[f];
            }
            if (h == 0) {
                float d[3], g[3];
#pragma unroll
                for (int f = 0; f < 3; f++) d[f] = halo_bottom && valid ? raw[(16 * f) % (RAW ? 48 : 1)] - halo_bottom[(size_t)f * n_col + col] : 0.0f;
                mpp_face_nu_grad(P, S.dz, true, d[0], d[1], d[2], g[0], g[1], g[2]);
#pragma unroll
                for (int f = 0; f < 3; f++) st[f * WM_FS + j * WM_LD] = 0.0f - g[f];
            }
        }

        // ---- layer 1, the three nets stacked: 5 tiles x 48 k-steps
#include "wm_net_layer1.inc"

#pragma unroll
        for (int n = 0; n < 3; n++) {
#include "wm_net_layer23.inc"

            // ---- interior face values in physical units, relative to the first (:292, :301, :318)
            // faces [0; interior; top] (:220-224): the cell's upper face is its own row (row 31: the top flux), its lower face the row below
            const float top_n = h == 1 && valid ? top[(size_t)n * n_col + col] : 0.0f;
            if (DIAG) {
                // ---- the diagnosed total flux: inv(scaling).(y) .- inv(scaling)(0) as written, minus what waits in the rows (each lane its own
                // slots), then the wave's span of this output in 16-byte pieces (a last tile of c columns: 33 c floats, the odd ones singly)
                float* row = st + n * WM_FS + j * WM_LD + 4 * h + 1;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float Fd = r == 15 && h == 1 ? top_n : wm_unscaled_minus_zero(S.fsig[n], S.fmu[n], y[r]);
                    row[WM_RHO0(r)] = Fd - row[WM_RHO0(r)];
                }
                WM_WAVE_SYNC();
                const int cnt = (int)min((long long)32, (long long)n_col - col0) * WM_LD;
                float* o = fcs[n] + (size_t)col0 * WM_LD;
                const float* img = st + n * WM_FS;
                WM_TILE_STORE_FACES(o, img, cnt);
            }
            if (!DZ) continue;
            const float y0 = __shfl(y[0], j);
            float F[16];
            if (n < 2) {
                // inv(scaling) applied a second time to the ALREADY unscaled first element, as the reference does (sic)
                const float a0 = S.fsig[n] * y0 + S.fmu[n];
                const float ref = S.fsig[n] * a0 + S.fmu[n];
#pragma unroll
                for (int r = 0; r < 16; r++) F[r] = (S.fsig[n] * y[r] + S.fmu[n]) - ref;
            } else {
#pragma unroll
                for (int r = 0; r < 16; r++) F[r] = S.fsig[2] * (y[r] - y0);
            }
            if (h == 1) F[15] = top_n;
            float* out = dzs[n];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float across = __shfl_xor(F[4 * q + 3], 32);        // row 8 q + 3 for h = 1, row 8 q + 7 for h = 0
                const float across_prev = q > 0 ? __shfl_xor(F[4 * q - 1], 32) : 0.0f;
                const float below = h == 1 ? across : across_prev;          // (h = 0, q = 0: face 0 carries no flux)
                f32x4 o;
                o[0] = (F[4 * q] - below) * S.inv_dz;
#pragma unroll
                for (int r = 1; r < 4; r++) o[r] = (F[4 * q + r] - F[4 * q + r - 1]) * S.inv_dz;
                if (valid) *reinterpret_cast<f32x4*>(out + (size_t)col * WM_NZ + 8 * q + 4 * h) = o;
            }
        }
