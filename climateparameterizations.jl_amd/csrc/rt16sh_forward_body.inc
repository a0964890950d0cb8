// The body of rt16sh_forward_kernel and rt16sh_forward_sched_kernel (engine_netsplit.hip, which describes it): RT16SH_SCHED = 1 reads the steps of each save
// interval from sched[] and sizes the tapes by total_steps, 0 takes `substeps` everywhere.
    // ensembles: blockIdx.y = model — its weight image, solution, tapes and closure constants (x0, bcs shared); grid.y = 1: one model
    wimg += (size_t)blockIdx.y * ens.wimg;
    if (sol) sol += (size_t)blockIdx.y * ens.sol;
    if (t16_tape) t16_tape += (size_t)blockIdx.y * ens.tape;
    if (t16_ztape) t16_ztape += (size_t)blockIdx.y * ens.ztape;
    const RtPhys ph = ens.phys ? ens.phys[blockIdx.y] : rt_phys_of(m);
    float* wl = rt_smem;
    const u32x4* simg = reinterpret_cast<const u32x4*>(rt_smem);
    f32x4v* ex = reinterpret_cast<f32x4v*>(rt_smem + ((RT_IMG_FLOATS + 3) & ~3));          // [2 buffers][3 variables][2 tiles][64 lanes]
    if constexpr (SPLIT) {
        // LDS: [bf16 operand image RT_SIMG2_WORDS][fp32 image from RT_W3C on: W3 and the biases][exchange][closure]
        const u32x4* src = reinterpret_cast<const u32x4*>(wimg + RT_SIMG2_OFF);
        u32x4* dst = reinterpret_cast<u32x4*>(rt_smem);
        for (int e = threadIdx.x; e < RT_SIMG2_WORDS / 4; e += 256) dst[e] = src[e];
        for (int e = threadIdx.x; e < RT_IMG_FLOATS - RT_W3C; e += 256) rt_smem[RT_SIMG2_WORDS + e] = wimg[RT_W3C + e];
        wl = rt_smem + RT_SIMG2_WORDS - RT_W3C;                                            // wl[RT_W3C ...], wl[RT_B1C ...] as in the fp32 layout
        ex = reinterpret_cast<f32x4v*>(rt_smem + RT_SIMG2_WORDS + ((RT_IMG_FLOATS - RT_W3C + 3) & ~3));
    } else {
        for (int e = threadIdx.x; e < RT_IMG_FLOATS; e += 256) wl[e] = wimg[e];
    }
    f32x4v* cl = ex + 2 * 384;                                                             // the helper wave's closure fluxes [3 variables][2 tiles][64 lanes]
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                     // 0..2: net = variable; 3: the helper (fourth SIMD)
    const bool helper = role == 3;
    const int n = helper ? 2 : role;
    const int j = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x;
    const int col = tile * 16 + j;
    const bool valid = col < n_col;
    const int colc = min(col, n_col - 1);
    const int i_ = lane & 15, g_i = i_ >> 2, r_i = i_ & 3;
    const bool live3 = r_i == 0 && g_i < 2;            // (SPLIT) this lane holds a row of the net's fourth layer-1 tile
    const int l83 = g_i * 4 + (lane >> 4);
    int a1b[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int Q = 4 * t + r_i, f = 4 * Q + g_i;
        a1b[t] = RT_W1C + (n * 50 + ((Q < 13 && f < 50) ? f : 0)) * RT_LD1 + 4 * g;       // padding rows read a valid row; never consumed
    }
    int a2b[2], a2l[2], a3b[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int Q2 = 4 * u + r_i;
        const int row2 = n * 20 + (Q2 < 5 ? 4 * Q2 + g_i : 0);
        a2b[u] = RT_W2C + row2 * RT_LD2 + g;
        a2l[u] = RT_W2C + row2 * RT_LD2 + (g < 2 ? 48 + g : 50);
        a3b[u] = RT_W3C + (n * 31 + 16 * u + i_ - 1) * RT_LD3 + g;
    }
    float bcb, bct, bc5;
    {
        const float* bp = bcs + (size_t)colc * 6;
        bcb = bp[2 * n];
        bct = bp[2 * n + 1];
        bc5 = bp[5];
    }
    V16 Xs[3], Xn, Kacc;
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int tau = 0; tau < 2; tau++) Xs[q].t[tau] = *reinterpret_cast<const f32x4v*>(x0 + (size_t)colc * 96 + q * 32 + 16 * tau + 4 * g);
    // (wave-uniform n: a select, not a dynamic register index)
#pragma unroll
    for (int tau = 0; tau < 2; tau++)
#pragma unroll
        for (int r = 0; r < 4; r++) Xn.t[tau][r] = n == 0 ? Xs[0].t[tau][r] : (n == 1 ? Xs[1].t[tau][r] : Xs[2].t[tau][r]);
    if (sol && valid && !helper)
#pragma unroll
        for (int tau = 0; tau < 2; tau++) *reinterpret_cast<f32x4v*>(sol + ((size_t)col * n_save) * 96 + n * 32 + 16 * tau + 4 * g) = Xn.t[tau];
#if RT16SH_SCHED
    const int n_steps = total_steps;
#else
    const int n_steps = (n_save - 1) * substeps;
#endif
    // stepper: classical RK4 (nst = 4) or the s-stage RKC2 step of colnde_dev.h (m.rkc: coefficient table; increment form as in tile16's
    // forward_kernel) — a template parameter: as a run-time switch it cost the RK4 latency kernels 8 % (8 simulations: 16.6 -> 18.2 ms)
    const int nst = RKC ? m.nst : 4;
    constexpr bool rkc = RKC;
    const float* mu_t = m.rkc, *nu_t = m.rkc + RKC_LD, *mut_t = m.rkc + 2 * RKC_LD, *gat_t = m.rkc + 3 * RKC_LD, *c_t = m.rkc + 4 * RKC_LD;
    float* tp = t16_tape ? t16_tape + (size_t)tile * n_steps * nst * 1536 + j * 96 + n * 32 + 4 * g : nullptr;
    float* tz = (t16_ztape && !RICH) ? t16_ztape + (size_t)tile * n_steps * nst * (16 * 216) + j * 216 + n * 72 + g : nullptr;
    float* tr = (t16_ztape && RICH) ? t16_ztape + (size_t)tile * n_steps * nst * RT16S_RREC + lane * 4 : nullptr;
    const float Nz = 32.0f;
    const float L2E = 1.4426950408889634f;
    const float cU = m.sig_u * Nz, sU = m.sig_u * m.eps, cV = m.sig_v * Nz, sV = m.sig_v * m.eps, cB = m.B * Nz, sB = m.B * m.eps;
    const float kE = 2.0f * ph.inv_dRi * L2E, oE = -2.0f * ph.Ric * ph.inv_dRi * L2E, cE = 30.0f * L2E;
    const float nA = -0.5f * ph.nu_minus, nB = ph.nu0 + 0.5f * ph.nu_minus;
    const float s0n = n == 0 ? m.s0[0] : (n == 1 ? m.s0[1] : m.s0[2]);
    const float An = n == 0 ? m.A[0] : (n == 1 ? m.A[1] : m.A[2]);
    int step = 0, buf = 0;
    RT_STAMP_DECL;
    for (int iv = 0; iv < n_save - 1; iv++) {
        const float t0 = save_times[iv];
#if RT16SH_SCHED
        substeps = sched[iv];                              // this interval's steps: wave-uniform, so all four waves take the same trip count
#endif
        const float dt = (save_times[iv + 1] - t0) / (float)substeps;
        for (int s = 0; s < substeps; s++, step++) {
            const float ts = t0 + (float)s * dt;
            Kacc.t[0] = (f32x4t)(0.0f);
            Kacc.t[1] = (f32x4t)(0.0f);
            V16 Ym1, Ym2, F0;                           // RKC2: d_{j-1}, d_{j-2} (increments Y_j - Y_0) and F_0 of variable n
#pragma unroll
            for (int tau = 0; tau < 2; tau++) { Ym1.t[tau] = (f32x4t)(0.0f); Ym2.t[tau] = (f32x4t)(0.0f); F0.t[tau] = (f32x4t)(0.0f); }
#pragma nounroll
            for (int st = 0; st < nst; st++) {
                const float ca = rkc ? c_t[st] : (st == 0 ? 0.0f : (st == 3 ? 1.0f : 0.5f));
                const float cb = (st == 0 || st == 3) ? 1.0f / 6.0f : 1.0f / 3.0f;
                RT_STAMP_BEGIN();
                f32x4v* eb = ex + buf * 384;
                if (helper) {
                    // ---- the Richardson-number closure of all three variables (predict_flux), once, on the fourth SIMD, while the net waves run
                    //      their chains: diffusive face fluxes to LDS, and (RICH) the nine pullback coefficients to the tape
                    float* orr = tr ? tr + ((size_t)step * nst + st) * RT16S_RREC : nullptr;
                    V16 C[3];
                    if (m.mpp) {
                        const V16 Ud = shift_down16(Xs[0], lane, 0.0f), Vd = shift_down16(Xs[1], lane, 0.0f), Td = shift_down16(Xs[2], lane, 0.0f);
                        const float f0 = -m.cs[0] * Nz, f1 = -m.cs[1] * Nz, f2 = -m.cs[2] * ph.inv_Pr * Nz;
                        const float m0 = -m.cs[0], m1 = -m.cs[1], m2 = -m.cs[2] * ph.inv_Pr, nr = Nz * ph.c_rib;
#pragma unroll
                        for (int tau = 0; tau < 2; tau++)
#pragma unroll
                            for (int r = 0; r < 4; r += 2) {
                                const f32x2v dU = {Xs[0].t[tau][r] - Ud.t[tau][r], Xs[0].t[tau][r + 1] - Ud.t[tau][r + 1]};
                                const f32x2v dV = {Xs[1].t[tau][r] - Vd.t[tau][r], Xs[1].t[tau][r + 1] - Vd.t[tau][r + 1]};
                                const f32x2v dT = {Xs[2].t[tau][r] - Td.t[tau][r], Xs[2].t[tau][r + 1] - Td.t[tau][r + 1]};
                                const f32x2v a1 = dU * cU + sU, a2 = dV * cV + sV;
                                const f32x2v s2 = a2 * a2 + a1 * a1;
                                f32x2v rS;
                                rS.x = __builtin_amdgcn_rcpf(s2.x);
                                rS.y = __builtin_amdgcn_rcpf(s2.y);
                                const f32x2v Ri = (dT * cB + sB) * rS;
                                const f32x2v arg = Ri * kE + oE;
                                f32x2v e;
                                e.x = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(arg.x, -cE, cE));
                                e.y = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(arg.y, -cE, cE));
                                const f32x2v e1 = e + 1.0f;
                                f32x2v rc;
                                rc.x = __builtin_amdgcn_rcpf(e1.x);
                                rc.y = __builtin_amdgcn_rcpf(e1.y);
                                const f32x2v th = rc * -2.0f + 1.0f;
                                const f32x2v nu = th * nA + nB;
                                const f32x2v c0 = (nu * dU) * f0, c1 = (nu * dV) * f1, c2 = (nu * dT) * f2;
                                C[0].t[tau][r] = c0.x; C[0].t[tau][r + 1] = c0.y;
                                C[1].t[tau][r] = c1.x; C[1].t[tau][r + 1] = c1.y;
                                C[2].t[tau][r] = c2.x; C[2].t[tau][r + 1] = c2.y;
                                if (RICH && orr) {
                                    const bool z0 = tau == 0 && r == 0 && g == 0;            // face 0 carries no diffusive flux
                                    const f32x2v wf = (1.0f - th * th) * rS, wR = wf * Ri;
                                    f32x2v pn = nu, pc0 = wR * (a1 * (-2.0f * m.sig_u)), pc1 = wR * (a2 * (-2.0f * m.sig_v)), pc2 = wf * m.B;
                                    if (z0) { pn.x = 0.0f; pc0.x = 0.0f; pc1.x = 0.0f; pc2.x = 0.0f; }
                                    float* o2 = orr + (36 + tau) * 256 + r;
                                    const f32x2v d0 = dU * (m0 * nr), d1 = dV * (m1 * nr), d2 = dT * (m2 * nr), q0 = pn * m0, q1 = pn * m1, q2 = pn * m2;
                                    *reinterpret_cast<f32x2v*>(o2 + 0 * 512) = d0;  *reinterpret_cast<f32x2v*>(o2 + 1 * 512) = d1;  *reinterpret_cast<f32x2v*>(o2 + 2 * 512) = d2;
                                    *reinterpret_cast<f32x2v*>(o2 + 3 * 512) = q0;  *reinterpret_cast<f32x2v*>(o2 + 4 * 512) = q1;  *reinterpret_cast<f32x2v*>(o2 + 5 * 512) = q2;
                                    *reinterpret_cast<f32x2v*>(o2 + 6 * 512) = pc0; *reinterpret_cast<f32x2v*>(o2 + 7 * 512) = pc1; *reinterpret_cast<f32x2v*>(o2 + 8 * 512) = pc2;
                                }
                            }
                    } else {
                        const V16 Td = shift_down16(Xs[2], lane, 0.0f);
#pragma unroll
                        for (int tau = 0; tau < 2; tau++)
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                const bool in = !(tau == 0 && r == 0 && g == 0);
                                const float gT = (Xs[2].t[tau][r] - Td.t[tau][r]) * Nz;
                                C[0].t[tau][r] = 0.0f;
                                C[1].t[tau][r] = 0.0f;
                                C[2].t[tau][r] = (m.ca && in) ? -m.cs[2] * m.kappa * fminf(0.0f, gT) : 0.0f;
                                if (RICH && orr && m.ca) {
                                    float* o2 = orr + (36 + tau) * 256 + r;
#pragma unroll
                                    for (int a9 = 0; a9 < 9; a9++) o2[a9 * 512] = (a9 == 5 && in && gT < 0.0f) ? -m.cs[2] * m.kappa : 0.0f;
                                }
                            }
                    }
#pragma unroll
                    for (int k = 0; k < 3; k++)
#pragma unroll
                        for (int tau = 0; tau < 2; tau++) cl[(k * 2 + tau) * 64 + lane] = C[k].t[tau];
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // (B) the closure is in LDS
                } else {
                V16 Xme;               // (element-wise selects on the wave-uniform n: a select between the aggregates becomes a scratch array)
#pragma unroll
                for (int tau = 0; tau < 2; tau++)
#pragma unroll
                    for (int r = 0; r < 4; r++) Xme.t[tau][r] = n == 0 ? Xs[0].t[tau][r] : (n == 1 ? Xs[1].t[tau][r] : Xs[2].t[tau][r]);
                if (tp) {
                    float* o = tp + ((size_t)step * nst + st) * 1536;
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) *reinterpret_cast<f32x4v*>(o + 16 * tau) = Xme.t[tau];
                }
                float* oz = tz ? tz + ((size_t)step * nst + st) * (16 * 216) : nullptr;
                float* orr = tr ? tr + ((size_t)step * nst + st) * RT16S_RREC : nullptr;
                const float top_raw = n == 2 ? rt_top_flux(m, bc5, ts + ca * dt) : bct;
                RT_STAMP(0);
                // ---- net n ----------------------------------------------------------------------------------------------
                int lz = lane;
                Bf3 XB[3];
                if constexpr (SPLIT) {
                    asm volatile("" : "+v"(lz));          // operand addresses stay (lane base + immediate): see rt16_forward_kernel
                    // only the first k-block's split stands in front of the products: those of blocks 1 and 2 follow tile 0's MFMAs of the block before
                    // (one wave per SIMD: nothing else hides their 88 vector instructions)
                    const float x8[8] = {Xs[0].t[0][0], Xs[0].t[0][1], Xs[0].t[0][2], Xs[0].t[0][3], Xs[0].t[1][0], Xs[0].t[1][1], Xs[0].t[1][2], Xs[0].t[1][3]};
                    XB[0] = bf3_split8(x8);
                }
                f32x4t A1[4];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    f32x4t acc;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int Q = 4 * t + r;
                        acc[r] = Q < 13 ? wl[RT_B1C + n * 50 + min(4 * Q + g, 49)] : 0.0f;
                    }
                    if constexpr (SPLIT) {
                        __builtin_amdgcn_s_setprio(1);
#pragma unroll
                        for (int q = 0; q < 3; q++) {
                            Bf3 A;
                            if (t < 3) A = rt16_ldA(simg, (n * 3 + t) * 3 + q, lz);
                            else {          // the net's fourth tile holds quad 12 alone: rows 0 and 4 (features 48, 49); every other lane reads the zero operand
                                const int at = live3 ? RT_SIMG2_T3 / 4 + (n * 3 + q) * 24 + l83 + (lz - lane) : RT_SIMG2_ZERO / 4 + (lz - lane);
                                A.h = simg[at]; A.m = simg[at + (live3 ? 8 : 0)]; A.l = simg[at + (live3 ? 16 : 0)];
                            }
                            acc = mfma16_bf3(A, XB[q], acc);
                            if (t == 0 && q < 2) {
                                const int qn = q < 2 ? q + 1 : 2;
                                const float n8[8] = {Xs[qn].t[0][0], Xs[qn].t[0][1], Xs[qn].t[0][2], Xs[qn].t[0][3], Xs[qn].t[1][0], Xs[qn].t[1][1], Xs[qn].t[1][2], Xs[qn].t[1][3]};
                                XB[qn] = bf3_split8(n8);
                            }
                        }
                        __builtin_amdgcn_s_setprio(0);
                        RT_SCHED_FENCE();
                    } else {
                    const int base = a1b[t];
                    acc = rt16_chain<24, 8>(wl, acc, [=](int k) { return base + (k >> 3) * 32 + ((k >> 2) & 1) * 16 + (k & 3); },
                                            [&](int k) { return Xs[k >> 3].t[(k >> 2) & 1][k & 3]; });
                    }
                    RT16S_ACC_FENCE(acc);
                    if (oz) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int Q = 4 * t + r;
                            if (Q < 13 && (Q < 12 || g < 2)) oz[4 * Q] = acc[r];             // feature 4 Q + g of layer 1
                        }
                    }
                    if (RICH && orr) {
                        f32x4t dd;
                        rt16_act_pair<ACT>(acc, A1[t], dd);
                        if (t == 3) { dd[1] = 0.0f; dd[2] = 0.0f; dd[3] = 0.0f; if (g >= 2) dd[0] = 0.0f; }   // padding: quads >= 13, features 50, 51
                        *reinterpret_cast<f32x4v*>(orr + (n * 12 + t) * 256) = A1[t];
                        *reinterpret_cast<f32x4v*>(orr + (n * 12 + 4 + t) * 256) = dd;
                    } else
                        A1[t] = rt_act4<ACT>(acc);
                }
                RT_STAMP(1);
                f32x4t A2[2];
                Bf3 HB[2];
                if constexpr (SPLIT) {
                    // the net's 13 quads of layer-1 activations as two 32-deep k-blocks (element e of block c: quad 8 c + e; three zero slots)
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        float a8[8];
#pragma unroll
                        for (int e = 0; e < 8; e++) a8[e] = 8 * c + e < 13 ? A1[(8 * c + e) >> 2][(8 * c + e) & 3] : 0.0f;
                        HB[c] = bf3_split8(a8);
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    f32x4t acc;
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[r] = (4 * u + r < 5) ? wl[RT_B2C + n * 20 + 4 * (4 * u + r) + g] : 0.0f;
                    if constexpr (SPLIT) {
                        const Bf3 Aa = rt16_ldA(simg, 27 + (n * 2 + u) * 2, lz), Ab = rt16_ldA(simg, 27 + (n * 2 + u) * 2 + 1, lz);
                        __builtin_amdgcn_s_setprio(1);
                        acc = mfma16_bf3(Aa, HB[0], acc);
                        acc = mfma16_bf3(Ab, HB[1], acc);
                        __builtin_amdgcn_s_setprio(0);
                        RT_SCHED_FENCE();
                    } else {
                    const int base = a2b[u], basel = a2l[u];
                    acc = rt16_chain<13, 13>(wl, acc, [=](int k) { return k < 12 ? base + 4 * k : basel; },
                                             [&](int k) { return A1[k >> 2][k & 3]; });
                    }
                    RT16S_ACC_FENCE(acc);
                    if (oz) {
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (4 * u + r < 5) oz[52 + 4 * (4 * u + r)] = acc[r];            // feature 4 Q2 + g of layer 2
                    }
                    if (RICH && orr) {
                        f32x4t dd;
                        rt16_act_pair<ACT>(acc, A2[u], dd);
                        if (u == 1) { dd[1] = 0.0f; dd[2] = 0.0f; dd[3] = 0.0f; }                             // padding: quads >= 5
                        *reinterpret_cast<f32x4v*>(orr + (n * 12 + 8 + u) * 256) = A2[u];
                        *reinterpret_cast<f32x4v*>(orr + (n * 12 + 10 + u) * 256) = dd;
                    } else
                        A2[u] = rt_act4<ACT>(acc);
                }
                V16 O;
#pragma unroll
                for (int v = 0; v < 2; v++) {
                    f32x4t acc;
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[r] = wl[RT_B3C + n * 32 + 16 * v + 4 * g + r];
                    const int base = a3b[v];
                    O.t[v] = rt16_chain<5, 5>(wl, acc, [=](int k) { return base + 4 * k; }, [&](int k) { return A2[k >> 2][k & 3]; });
                }
                RT_STAMP(2);
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");           // (B) the helper's closure fluxes are in LDS
                // ---- physics: face flux = NN flux + closure flux, tendency of variable n (predict_flux / predict_NDE) ---------
                V16 F;
#pragma unroll
                for (int tau = 0; tau < 2; tau++) F.t[tau] = O.t[tau] + cl[(n * 2 + tau) * 64 + lane];
                if (g == 0) F.t[0][0] = m.mpp ? (m.zero_w ? bcb - s0n : bcb) : (m.zero_w ? 0.0f : bcb);      // face 0: the bottom boundary
                {
                    const float top = m.zero_w ? top_raw - s0n : top_raw;
                    const V16 Fu = shift_up16(F, lane, top);
#pragma unroll
                    for (int tau = 0; tau < 2; tau++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            float v = -An * (Fu.t[tau][r] - F.t[tau][r]);
                            if (n == 0) v += m.cor_u * (m.sig_v * Xs[1].t[tau][r] + m.mu_v);
                            if (n == 1) v -= m.cor_v * (m.sig_u * Xs[0].t[tau][r] + m.mu_u);
                            F.t[tau][r] = v;                                                // F now holds the tendency of variable n
                        }
                }
                RT_STAMP(3);
                // ---- RK4 bookkeeping for variable n; the next stage input (or, after stage 3, the new state) is exchanged -------------
                V16 Xnext;
                if (rkc) {
                    // Y_j, j = st + 1: d_1 = mu~_1 h F_0;  d_j = mu_j d_{j-1} + nu_j d_{j-2} + mu~_j h F_{j-1} + gamma~_j h F_0;  Y_s ends the step
                    const int jj = st + 1;
                    const float cmu = mu_t[jj], cnu = nu_t[jj], cmt = mut_t[jj] * dt, cga = gat_t[jj] * dt;
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) {
                        if (st == 0) F0.t[tau] = F.t[tau];
                        const f32x4t dj = st == 0 ? cmt * F0.t[tau] : cmu * Ym1.t[tau] + cnu * Ym2.t[tau] + cmt * F.t[tau] + cga * F0.t[tau];
                        Xnext.t[tau] = Xn.t[tau] + dj;
                        Ym2.t[tau] = Ym1.t[tau];
                        Ym1.t[tau] = dj;
                        if (jj == nst) Xn.t[tau] = Xnext.t[tau];
                    }
                } else {
#pragma unroll
                for (int tau = 0; tau < 2; tau++) {
                    Kacc.t[tau] += cb * F.t[tau];
                    if (st < 3) {
                        const float can = st == 2 ? 1.0f : 0.5f;
                        Xnext.t[tau] = Xn.t[tau] + (can * dt) * F.t[tau];
                    } else {
                        Xn.t[tau] += dt * Kacc.t[tau];
                        Xnext.t[tau] = Xn.t[tau];
                    }
                }
                }
#pragma unroll
                for (int tau = 0; tau < 2; tau++) eb[(n * 2 + tau) * 64 + lane] = Xnext.t[tau];
                }
                // (a bare barrier behind the LDS writes: __syncthreads() would also drain vmcnt, i.e. wait for this stage's tape stores)
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
                for (int q = 0; q < 3; q++)
#pragma unroll
                    for (int tau = 0; tau < 2; tau++) Xs[q].t[tau] = eb[(q * 2 + tau) * 64 + lane];
                buf ^= 1;
                RT_STAMP(4);
            }
            if (s == substeps - 1 && sol && valid && !helper) {
#pragma unroll
                for (int tau = 0; tau < 2; tau++)
                    *reinterpret_cast<f32x4v*>(sol + ((size_t)col * n_save + iv + 1) * 96 + n * 32 + 16 * tau + 4 * g) = Xn.t[tau];
            }
        }
    }
#ifdef COLNDE_STAMPS_FWD
    RT_STAMP_FLUSH();
#endif
