// Body of pack_weights_kernel and pack_weights_ens_kernel (engine_tile16.hip): included by both, so that the single-model kernel stays the text it was.
// In scope: m, pk, w, wf, wb (the ensemble kernel has moved them to model blockIdx.y's arrays).
    const int total_f = pk.pf_net * m.n_nets, total_b = pk.pb_net * m.n_nets;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total_f + total_b; idx += gridDim.x * blockDim.x) {
        const bool fwd = idx < total_f;
        int e = fwd ? idx : idx - total_f;
        const int pn = fwd ? pk.pf_net : pk.pb_net;
        const int net = e / pn;
        e -= net * pn;
        int l = 0;
        while (l + 1 < m.n_layers && e >= (fwd ? pk.pf_off[l + 1] : pk.pb_off[l + 1])) l++;
        e -= fwd ? pk.pf_off[l] : pk.pb_off[l];
        const int ni = m.sizes[l], no = m.sizes[l + 1];
        const int jj = e & 3, lane = (e >> 2) & 63;
        const int blk = e >> 8;
        const float* W = w + (size_t)net * m.net_size + m.w_off[l];
        float v = 0.0f;
        if (fwd) {
            const int nS = (ni + 15) >> 4;
            const int mt = blk / nS, S = blk - mt * nS;
            const int i = mt * 16 + (lane & 15), k = 16 * S + 4 * (lane >> 4) + jj;
            if (i < no && k < ni) v = W[(size_t)k * no + i];
            wf[idx] = v;
        } else {
            const int nS = (no + 15) >> 4;
            const int it = blk / nS, S = blk - it * nS;
            const int i = it * 16 + (lane & 15), j = 16 * S + 4 * (lane >> 4) + jj;
            if (i < ni && j < no) v = W[(size_t)i * no + j];
            wb[idx - total_f] = v;
        }
    }
