// engine_fc_pretrain.hip — T -> wT pre-training of all K networks of a free-convection ensemble in one launch.
//
// free_convection/train_free_convection_nde.jl:182-216 fits the network to the LES fluxes before the NDE is trained: `Flux.train!` makes one optimiser
// update per (shuffled) sample, 10 epochs of ADAM() and 10 of Descent(1e-2), on mse([bottom; NN(T); top], wT) [+ sum(abs2, W1[mask]) under
// --spatial_causality soft].  The chain of updates of ONE network is serial (pretrain_kernel, engine_tile16.hip: one workgroup); the K networks of a
// sweep are independent, so here the model index is the launch grid: blockIdx.x = model, 512 threads, and model k touches only row k of theta, m, v
// ([K][n_params]), of order, eta and coeff.  All models read the same samples.
//
// Per sample the workgroup runs the chain of pretrain_sample.h — the very functions pretrain_kernel runs — so for a plain network under ADAM without
// penalty row k holds the bits of colnde_pretrain_flux_dev on a single handle (gradient_scaling = 0).  New here:
//   the --conv network: y[i] = relu(b + sum_d w[c - 1 - d] x[i + d]), i < M = Nz - c + 1, in front of Dense(M, 4Nz) (free_convection.conv_to_dense's
//     Toeplitz first layer); its c + 1 gradient entries are sums over the M outputs, each walked by ONE thread in index order (bit-reproducible);
//   the penalty c_k sum_{r<q} W1[r, q]^2 in the loss and 2 c_k W1[r, q] in the gradient (mask of colnde_ensemble_causal_penalty_dev);
//   Descent: theta -= eta g, no moments, the running powers untouched.
// LDS: pretrain_kernel's carving of the dense part, then the filter's pre-activations, activations and deltas (fc_pretrain_lds_bytes).
// Plain C++, vector loads and stores; every value has one owning thread, nothing is atomic.
#include "engine_fc_pretrain.h"
#include "kernel_select.h"
#include "pretrain_sample.h"

__global__ void __launch_bounds__(512)
fc_pretrain_ens_kernel(DevModel m, int conv, float* __restrict__ theta, float* __restrict__ mom, float* __restrict__ vel, const float* __restrict__ X,
                       const float* __restrict__ BC, const float* __restrict__ Y, const int* __restrict__ order, int n_samples,
                       const float* __restrict__ coeff, int optimiser, const float* __restrict__ eta_k, float gs, float b1, float b2, float eps_adam,
                       double bt1, double bt2, int update, float* __restrict__ loss_out, double* __restrict__ bt_out) {
    extern __shared__ __attribute__((aligned(16))) float fcp_smem[];
    const int tid = threadIdx.x, nth = blockDim.x;
    const int Nz = m.Nz, nf = Nz + 1;
    const size_t k = blockIdx.x, P = (size_t)m.n_params;
    float* tw = theta + k * P;
    float* tm = mom ? mom + k * P : nullptr;
    float* tv = vel ? vel + k * P : nullptr;
    const int* ord = order ? order + k * (size_t)n_samples : nullptr;
    const float pen = coeff ? coeff[k] : 0.0f;                // (uniform over the workgroup)
    const float eta = eta_k ? eta_k[k] : 0.0f;
    const bool adam = optimiser == FCP_ADAM;
    const PtLds lds = pt_carve(m, fcp_smem);
    const float* a0 = lds.a0;
    // the filter's M outputs: pre-activations, activations, deltas
    const int M = conv ? Nz - conv + 1 : 0, Mp = (M + 3) & ~3;
    float* cz = lds.red + 64;
    float* cy = cz + Mp;
    float* cd = cy + Mp;
    const float* ain0 = conv ? cy : a0;                       // what the first Dense reads
    const int M1 = m.sizes[0], H = m.sizes[1];                // the first Dense weight: H x M1 at w_off[0], W1[r, q] at q H + r
    double p1 = bt1, p2 = bt2;                                // running powers beta^t (uniform over the workgroup)
    float loss_sum = 0.0f;
    for (int s = 0; s < n_samples; s++) {
        const int idx = ord ? ord[s] : s;
        pt_load(m, lds, X, Y, idx, tid, nth);
        __syncthreads();
        for (int f = tid; f < nf; f += nth) lds.cf[f] = pt_bc_face(BC + (size_t)idx * m.n_bc, f, Nz);
        if (conv) {
            for (int i = tid; i < M; i += nth) {
                float acc = tw[conv];
                for (int d = 0; d < conv; d++) acc = fmaf(tw[conv - 1 - d], a0[i + d], acc);
                cz[i] = acc;
                cy[i] = dev_act(COLNDE_ACT_RELU, acc);
            }
            __syncthreads();
        }
        pt_forward(m, lds, tw, ain0, tid, nth);
        if (pen != 0.0f) {
            // the masked entries r < q of W1 (q < M1 <= H), enumerated over the M1 x M1 square; the partial sums meet in a fixed order.  red[8..15]:
            // beside pt_loss's slots, and published by its barrier
            float pp = 0.0f;
            const float* W1 = tw + m.w_off[0];
            for (int e = tid; e < M1 * M1; e += nth) {
                const int q = e / M1, r = e - q * M1;
                if (r < q) {
                    const float w = W1[q * H + r];
                    pp = fmaf(w, w, pp);
                }
            }
            for (int off = 32; off > 0; off >>= 1) pp += __shfl_down(pp, off);
            if ((tid & 63) == 0) lds.red[8 + (tid >> 6)] = pp;
        }
        float t = pt_loss(m, lds, gs, tid, nth);
        if (pen != 0.0f && tid == 0) {
            float ps = 0.0f;
            for (int w = 0; w < (nth >> 6); w++) ps += lds.red[8 + w];
            t = fmaf(pen, ps, t);
        }
        loss_sum += t;
        if (!update) { __syncthreads(); continue; }
        pt_backward(m, lds, tw, tid, nth);
        const float c1 = (float)(1.0 / (1.0 - p1)), c2 = (float)(1.0 / (1.0 - p2));
        if (conv) {
            // the filter outputs' deltas through W1 as it stood before this sample's update, then the filter's c + 1 gradient entries
            const float* W1 = tw + m.w_off[0];
            for (int i = tid; i < M; i += nth) {
                float acc = 0.0f;
                for (int o = 0; o < H; o++) acc = fmaf(W1[i * H + o], lds.dd[m.act_off[0] + o], acc);
                cd[i] = acc * dev_act_grad(COLNDE_ACT_RELU, cz[i]);
            }
            __syncthreads();
            if (tid <= conv) {
                // entry j < c: the tap w[j] multiplies x[i + c - 1 - j] in output i; entry c: the bias
                const int j = tid, d = conv - 1 - j;
                float g = 0.0f;
                if (j < conv) for (int i = 0; i < M; i++) g = fmaf(cd[i], a0[i + d], g);
                else for (int i = 0; i < M; i++) g += cd[i];
                if (adam) pt_apply<true>(tw, tm, tv, j, g, eta, b1, b2, eps_adam, c1, c2);
                else pt_apply<false>(tw, tm, tv, j, g, eta, b1, b2, eps_adam, c1, c2);
            }
        }
        if (adam) {
            pt_update<true>(m, lds, tw, tm, tv, ain0, pen, eta, b1, b2, eps_adam, c1, c2, tid, nth);
            p1 *= (double)b1;
            p2 *= (double)b2;
        } else {
            pt_update<false>(m, lds, tw, tm, tv, ain0, pen, eta, b1, b2, eps_adam, c1, c2, tid, nth);
        }
        __syncthreads();
    }
    if (tid == 0) {
        loss_out[k] = loss_sum;
        if (bt_out && k == 0) { bt_out[0] = p1; bt_out[1] = p2; }
    }
}

hipError_t fcp_set_kernel_attributes(size_t max_lds_bytes) { return set_max_lds(fc_pretrain_ens_kernel, max_lds_bytes); }

hipError_t launch_fc_pretrain_ens(const DevModel& dense, int conv, int n_models, float* theta, float* mom, float* vel, const float* X, const float* BC,
                                  const float* Y, const int* order, int n_samples, const float* coeff, int optimiser, const float* eta, float b1, float b2,
                                  float eps, double bt1, double bt2, int update, float* loss_out, double* bt_out, hipStream_t stream) {
    const size_t lds = fc_pretrain_lds_bytes(dense, conv);
    if (lds > PRETRAIN_LDS_CAP || n_models < 1 || n_samples < 1) return hipErrorInvalidValue;
    if (conv && (conv < 2 || dense.Nz - conv + 1 < 1 || dense.sizes[0] != dense.Nz - conv + 1)) return hipErrorInvalidValue;
    // gradient_scaling = 0: the reference's pre-training loss is the plain mse (a kernel argument, so that the loss is the single call's expression)
    hipLaunchKernelGGL(fc_pretrain_ens_kernel, dim3(n_models), dim3(512), lds, stream, dense, conv, theta, mom, vel, X, BC, Y, order, n_samples, coeff,
                       optimiser, eta, 0.0f, b1, b2, eps, bt1, bt2, update, loss_out, bt_out);
    return hipGetLastError();
}
