// Body of pack_planes_kernel and pack_planes_ens_kernel (engine_tile16.hip): included by both.  In scope: m, w, sf, sb (model blockIdx.y's in the ensemble kernel).
    const long total_f = (long)m.sf_net * m.n_nets, total_b = (long)m.sb_net * m.n_nets;         // 16-byte items
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total_f + total_b; idx += (long)gridDim.x * blockDim.x) {
        const bool fwd = idx < total_f;
        long e = fwd ? idx : idx - total_f;
        const int pn = fwd ? m.sf_net : m.sb_net;
        const int net = (int)(e / pn);
        e -= (long)net * pn;
        int l = 0;
        while (l + 1 < m.n_layers && e >= (fwd ? m.sf_off[l + 1] : m.sb_off[l + 1])) l++;
        e -= fwd ? m.sf_off[l] : m.sb_off[l];
        const int ni = m.sizes[l], no = m.sizes[l + 1];
        const int lane = (int)(e & 63), plane = (int)((e >> 6) % 3);
        const long blk = (e >> 6) / 3;
        const int nS = fwd ? (ni + 31) >> 5 : (no + 31) >> 5;
        const int tile = (int)(blk / nS), S = (int)(blk - (long)tile * nS);
        const float* W = w + (size_t)net * m.net_size + m.w_off[l];
        const int i = tile * 16 + (lane & 15);
        unsigned out[4];
#pragma unroll
        for (int pr = 0; pr < 4; pr++) {
            float v[2];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int k = 32 * S + 8 * (lane >> 4) + 2 * pr + q;
                float x = 0.0f;
                if (fwd) { if (i < no && k < ni) x = W[(size_t)k * no + i]; }            // A[i = out row][k = in]
                else { if (i < ni && k < no) x = W[(size_t)i * no + k]; }               // A[i = in row][k = out]
                const float hh = __uint_as_float(__float_as_uint(x) & 0xffff0000u), r1 = x - hh;
                const float mm = __uint_as_float(__float_as_uint(r1) & 0xffff0000u), ll = r1 - mm;
                v[q] = plane == 0 ? hh : (plane == 1 ? mm : ll);
            }
            out[pr] = (__float_as_uint(v[1]) & 0xffff0000u) | (__float_as_uint(v[0]) >> 16);
        }
        unsigned* dst = (fwd ? sf : sb) + (size_t)(fwd ? idx : idx - total_f) * 4;
        dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2]; dst[3] = out[3];
    }
