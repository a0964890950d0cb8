// pretrain_sample.h — the per-sample body of flux-MLP pre-training, shared by pretrain_kernel (engine_tile16.hip: one model, one workgroup),
// fc_pretrain_ens_kernel (engine_fc_pretrain.hip: one workgroup per model) and wm_pretrain_ens_kernel (engine_wm_pretrain.hip: one workgroup per
// model and flux net).  The kernels instantiate THESE functions on the same LDS carving, so a model's chain of updates is the same sequence of float
// operations in each: row k of an ensemble pass holds the bits of the single call.
// Nothing here spreads a dot product over lanes: an output (forward), an input (backward) or a parameter (update) has one owning thread that walks its
// sum in index order.
#pragma once
#include "colnde_dev.h"

// LDS: act[act_total + ns] (a_0 = x, then every layer's activations), z[act_total] pre-activations, d[act_total] deltas,
//      F, y, c: [Nz + 1] face vectors, red[64].  (pretrain_lds_bytes, engine_tile16.h)
struct PtLds { float *a0, *act, *zz, *dd, *F, *yv, *cf, *red; };

__device__ __forceinline__ PtLds pt_carve(const DevModel& m, float* smem) {
    const int nf = m.Nz + 1;
    PtLds s;
    s.a0 = smem;                                 // x
    s.act = s.a0 + ((m.ns + 3) & ~3);            // a_l at act + act_off[l-1]... (act_off[l] = offset of layer l+1's outputs)
    s.zz = s.act + m.act_total + 4;
    s.dd = s.zz + m.act_total + 4;
    s.F = s.dd + m.act_total + 4;
    s.yv = s.F + nf + 3;
    s.cf = s.yv + nf + 3;
    s.red = s.cf + nf + 3;
    return s;
}

// sample idx into LDS: the profile and the 'true' flux (the caller synchronises)
__device__ __forceinline__ void pt_load(const DevModel& m, const PtLds& s, const float* __restrict__ X, const float* __restrict__ Y, int idx, int tid, int nth) {
    const int ns = m.ns, nf = m.Nz + 1;
    for (int i = tid; i < ns; i += nth) s.a0[i] = X[(size_t)idx * ns + i];
    for (int f = tid; f < nf; f += nth) s.yv[f] = Y[(size_t)idx * nf + f];
}

// T-only models: the weight-independent part of the face flux is the two boundary faces, [bottom; NN(T); top]
__device__ __forceinline__ float pt_bc_face(const float* bc, int f, int Nz) { return f == 0 ? bc[0] : (f == Nz ? bc[1] : 0.0f); }

struct FaceGrad { float gu, gv, gT, S2, Ri; };

// tanh(y) = 1 - 2/(1 + e^{2y}) on the fast exp / reciprocal units (|rel err| ~ 1e-6)
__device__ __forceinline__ float fast_tanh(float y) {
    const float e = __expf(2.0f * fminf(fmaxf(y, -15.0f), 15.0f));
    return 1.0f - fast_div(2.0f, 1.0f + e);
}

__device__ __forceinline__ FaceGrad wm_face(const DevModel& m, const float* x, int f, float eps) {
    const int Nz = m.Nz;
    const bool in = f >= 1 && f < Nz;
    FaceGrad g;
    g.gu = in ? (x[f] - x[f - 1]) * (float)Nz : 0.0f;
    g.gv = in ? (x[Nz + f] - x[Nz + f - 1]) * (float)Nz : 0.0f;
    g.gT = in ? (x[2 * Nz + f] - x[2 * Nz + f - 1]) * (float)Nz : 0.0f;
    const float a1 = m.sig_u * (g.gu + eps), a2 = m.sig_v * (g.gv + eps);
    g.S2 = a1 * a1 + a2 * a2;
    g.Ri = fast_div(m.B * (g.gT + eps), g.S2);   // local_richardson, NDE_training.jl:46-52
    return g;
}

// Wind-mixing models: the weight-independent part of face f of flux k (0 = uw, 1 = vw, 2 = wT) for the profile a0 and the sample's six boundary
// fluxes bc — the boundary faces (MPP's end faces under zero_weights: NN_training.jl:62-66), the Richardson-number closure, or the
// convective-adjustment term of wT.  The five closure constants are arguments: pretrain_kernel passes the handle's (DevModel), wm_pretrain_ens_kernel
// those of its model (RtPhys), and both evaluate this one text.
__device__ __forceinline__ float pt_wm_face_const(const DevModel& m, const float* a0, const float* bc, int k, int f, float nu0, float nu_minus, float Ric,
                                                  float inv_dRi, float inv_Pr) {
    const int Nz = m.Nz;
    float c = 0.0f;
    const float bb = bc[2 * k], bt = bc[2 * k + 1];
    const bool in = f >= 1 && f < Nz;
    if (!in) c = m.zero_w ? (f == 0 ? bb : bt) - m.s0[k] : (f == 0 ? bb : bt);
    else if (m.mpp) {
        const FaceGrad g = wm_face(m, a0, f, m.eps);
        const float nu = nu0 + nu_minus * (1.0f - fast_tanh((g.Ri - Ric) * inv_dRi)) * 0.5f;
        c = -m.cs[k] * (k == 2 ? nu * inv_Pr : nu) * (k == 0 ? g.gu : (k == 1 ? g.gv : g.gT));
    } else if (m.ca && k == 2) {
        const float gT = (a0[2 * Nz + f] - a0[2 * Nz + f - 1]) * (float)Nz;
        c = -m.cs[2] * m.kappa * fminf(0.0f, gT);
    }
    return c;
}

// forward through the dense layers of net `th`; ain0: the input of layer 0 (the profile, or the filter's activations)
__device__ __forceinline__ void pt_forward(const DevModel& m, const PtLds& s, const float* th, const float* ain0, int tid, int nth) {
    const int L = m.n_layers;
    for (int l = 0; l < L; l++) {
        const int ni = m.sizes[l], no = m.sizes[l + 1];
        const float* ain = l == 0 ? ain0 : s.act + m.act_off[l - 1];
        const float* W = th + m.w_off[l];
        for (int o = tid; o < no; o += nth) {
            float acc = th[m.b_off[l] + o];
            for (int i = 0; i < ni; i++) acc = fmaf(W[i * no + o], ain[i], acc);
            s.zz[m.act_off[l] + o] = acc;
            s.act[m.act_off[l] + o] = dev_act(m.acts[l], acc);
        }
        __syncthreads();
    }
}

// face flux, loss and its cotangent on the network output: the sample's loss, valid in thread 0 (the others return 0); leaves the workgroup synchronised
// on red[] (the caller synchronises before red[] is written again)
__device__ __forceinline__ float pt_loss(const DevModel& m, const PtLds& s, float gs, int tid, int nth) {
    const int Nz = m.Nz, nf = Nz + 1, L = m.n_layers;
    float* F = s.F;
    const float* yv = s.yv;
    const float* out = s.act + m.act_off[L - 1];
    for (int f = tid; f < nf; f += nth) F[f] = s.cf[f] + ((f >= 1 && f < Nz) ? out[f - 1] : 0.0f);
    __syncthreads();
    float part = 0.0f;
    for (int f = tid; f < nf; f += nth) {
        const float r = F[f] - yv[f];
        part += r * r * (1.0f / (float)nf);
        if (f < Nz) {
            const float dg = ((F[f + 1] - F[f]) - (yv[f + 1] - yv[f])) * (float)Nz;
            part += gs * dg * dg * (1.0f / (float)Nz);
        }
        if (f >= 1 && f < Nz) {
            const float dgm = ((F[f] - F[f - 1]) - (yv[f] - yv[f - 1])) * (float)Nz;
            const float dgp = ((F[f + 1] - F[f]) - (yv[f + 1] - yv[f])) * (float)Nz;
            const float g = 2.0f / (float)nf * r + gs * 2.0f * (dgm - dgp);
            s.dd[m.act_off[L - 1] + f - 1] = g * dev_act_grad(m.acts[L - 1], s.zz[m.act_off[L - 1] + f - 1]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off);
    if ((tid & 63) == 0) s.red[tid >> 6] = part;
    __syncthreads();
    float t = 0.0f;
    if (tid == 0)
        for (int w = 0; w < (nth >> 6); w++) t += s.red[w];
    return t;
}

// backward: every delta with the weights as they stood before this sample's update
__device__ __forceinline__ void pt_backward(const DevModel& m, const PtLds& s, const float* th, int tid, int nth) {
    const int L = m.n_layers;
    for (int l = L - 1; l >= 1; l--) {
        const int ni = m.sizes[l], no = m.sizes[l + 1];
        const float* W = th + m.w_off[l];
        for (int i = tid; i < ni; i += nth) {
            float acc = 0.0f;
            for (int o = 0; o < no; o++) acc = fmaf(W[i * no + o], s.dd[m.act_off[l] + o], acc);
            s.dd[m.act_off[l - 1] + i] = acc * dev_act_grad(m.acts[l - 1], s.zz[m.act_off[l - 1] + i]);
        }
        __syncthreads();
    }
}

// One parameter's update with its gradient element g.
//   ADAM:     Flux ADAM (apply! + update!), c1 = 1 / (1 - beta1^t), c2 = 1 / (1 - beta2^t)
//   Descent:  theta -= eta g; the moments are not touched (tm, tv may be null)
template <bool ADAM>
__device__ __forceinline__ void pt_apply(float* __restrict__ tw, float* __restrict__ tm, float* __restrict__ tv, int q, float g, float eta, float b1, float b2,
                                         float eps_adam, float c1, float c2) {
    if (ADAM) {
        const float mt = b1 * tm[q] + (1.0f - b1) * g;
        const float vt = b2 * tv[q] + (1.0f - b2) * g * g;
        tm[q] = mt;
        tv[q] = vt;
        tw[q] -= eta * (mt * c1) / (sqrtf(vt * c2) + eps_adam);
    } else {
        tw[q] -= eta * g;
    }
}

// The update of every parameter of the net; gradient element = delta_out * input (bias: delta_out), plus 2 pen W1[r, q] on the entries r < q of the
// first weight (the soft spatial-causality penalty; pen = 0: none).
template <bool ADAM>
__device__ __forceinline__ void pt_update(const DevModel& m, const PtLds& s, float* __restrict__ tw, float* __restrict__ tm, float* __restrict__ tv,
                                          const float* ain0, float pen, float eta, float b1, float b2, float eps_adam, float c1, float c2, int tid, int nth) {
    const int L = m.n_layers;
    for (int l = 0; l < L; l++) {
        const int ni = m.sizes[l], no = m.sizes[l + 1];
        const float* ain = l == 0 ? ain0 : s.act + m.act_off[l - 1];
        const int nw = ni * no;
        for (int e = tid; e < nw + no; e += nth) {
            const bool bias = e >= nw;
            const int o = bias ? e - nw : e % no, i = bias ? 0 : e / no;
            float g = s.dd[m.act_off[l] + o] * (bias ? 1.0f : ain[i]);
            const int q = (bias ? m.b_off[l] - nw : m.w_off[l]) + e;
            if (pen != 0.0f && l == 0 && !bias && o < i) g += 2.0f * pen * tw[q];
            pt_apply<ADAM>(tw, tm, tv, q, g, eta, b1, b2, eps_adam, c1, c2);
        }
    }
}
