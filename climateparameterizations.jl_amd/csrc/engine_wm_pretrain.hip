// engine_wm_pretrain.hip — flux pre-training of all K x 3 networks of a wind-mixing ensemble in one launch.
//
// wind_mixing/train_NN.jl fits each of the three flux networks (uw, vw, wT) to the LES fluxes with `train_NN` (wind_mixing/src/NN_training.jl:207-249:
// one ADAM update per shuffled sample) before the NDE sweep starts.  The closure part of the face flux takes nu0, nu_minus, dRi, Ric and Pr, so a sweep over
// those constants needs K different pre-trainings of each net.  The chain of updates of ONE network is serial (pretrain_kernel, engine_tile16.hip: one
// workgroup); the K x 3 chains are independent, so here they are the launch grid: blockIdx.x = model k, blockIdx.y = net j (0 = uw, 1 = vw, 2 = wT), and
// workgroup (k, j) touches only floats [k P + j net_size, k P + (j + 1) net_size) of theta, m, v, row (k, j) of order and eta, and model k's constants
// (RtPhys).  A workgroup whose net is not in the mask `nets` returns before its first barrier.  All chains read the same samples.
//
// Per sample the workgroup runs the chain of pretrain_sample.h — the very functions pretrain_kernel runs, on the same LDS carving, with the same
// expression for the weight-independent part of the face flux (pt_wm_face_const) — so block (k, j) holds the bits of colnde_pretrain_flux_dev on a
// single handle whose config carries model k's constants, flux_type = j.
//
// LDS-resident parameters: the net's theta, m, v (3 x 6,521 floats = 78 KB; with the carving 80,656 B, two workgroups per CU) are staged into LDS behind the
// carving once (update = 0: theta only), every sample runs on the LDS copies, and the three blocks are written back once at the end — instead of a
// read-modify-write of 78 KB through L2 per sample in a latency-bound serial chain.  The same float operations on the same values.
// Measured against the form that leaves them in global memory, and at 128 / 256 / 512 threads (tools/wm_pretrain_rate.py): LDS-resident with 512
// threads is the fastest of the six at every K.  The other five are builds of this unit for that tool (WMP_IN_LDS=0, WMP_BLOCK=<threads>: make variant).
// Plain C++, vector loads and stores; every value has one owning thread, nothing is atomic.
#include "engine_wm_pretrain.h"
#include "kernel_select.h"
#include "pretrain_sample.h"

#ifndef WMP_IN_LDS
#define WMP_IN_LDS 1
#endif
#ifndef WMP_BLOCK
#define WMP_BLOCK 512
#endif
static_assert(WMP_BLOCK >= 64 && WMP_BLOCK <= 512 && WMP_BLOCK % 64 == 0, "a whole number of wavefronts, at most 512 threads");

__global__ void __launch_bounds__(WMP_BLOCK)
wm_pretrain_ens_kernel(DevModel m, int nets, const RtPhys* __restrict__ phys, float* __restrict__ theta, float* __restrict__ mom, float* __restrict__ vel,
                       const float* __restrict__ X, const float* __restrict__ BC, const float* __restrict__ Y, const int* __restrict__ order, int n_samples,
                       float gs, const float* __restrict__ eta_kj, float b1, float b2, float eps_adam, double bt1, double bt2, int update,
                       float* __restrict__ loss_out, double* __restrict__ bt_out) {
    extern __shared__ __attribute__((aligned(16))) float wmp_smem[];
    constexpr bool IN_LDS = WMP_IN_LDS;
    const int j = blockIdx.y;
    if (!((nets >> j) & 1)) return;                           // (uniform over the workgroup, before any barrier)
    const int tid = threadIdx.x, nth = blockDim.x;
    const int Nz = m.Nz, nf = Nz + 1, ns = m.net_size;
    const size_t k = blockIdx.x, chain = k * 3 + j, base = k * (size_t)m.n_params + (size_t)j * ns;
    const RtPhys ph = phys[k];
    const float* Yj = Y + (size_t)j * n_samples * nf;
    const int* ord = order ? order + chain * (size_t)n_samples : nullptr;
    const float eta = eta_kj ? eta_kj[chain] : 0.0f;          // (uniform over the workgroup)
    const PtLds lds = pt_carve(m, wmp_smem);
    const float* a0 = lds.a0;
    float* tw = theta + base;
    float* tm = mom ? mom + base : nullptr;
    float* tv = vel ? vel + base : nullptr;
    if (IN_LDS) {
        // the net's blocks behind the carving; the copies run on scalar loads (base is not a multiple of four floats)
        const int nsp = (ns + 3) & ~3;
        float* lw = lds.red + 64;
        float* lm = lw + nsp;
        float* lv = lm + nsp;
        for (int q = tid; q < ns; q += nth) {
            lw[q] = tw[q];
            if (update) { lm[q] = tm[q]; lv[q] = tv[q]; }
        }
        tw = lw; tm = lm; tv = lv;
        __syncthreads();
    }
    double p1 = bt1, p2 = bt2;                                // running powers beta^t (uniform over the workgroup)
    float loss_sum = 0.0f;
    for (int s = 0; s < n_samples; s++) {
        const int idx = ord ? ord[s] : s;
        pt_load(m, lds, X, Yj, idx, tid, nth);
        __syncthreads();
        const float* bc = BC + (size_t)idx * m.n_bc;
        for (int f = tid; f < nf; f += nth) lds.cf[f] = pt_wm_face_const(m, a0, bc, j, f, ph.nu0, ph.nu_minus, ph.Ric, ph.inv_dRi, ph.inv_Pr);
        pt_forward(m, lds, tw, a0, tid, nth);
        loss_sum += pt_loss(m, lds, gs, tid, nth);
        if (!update) { __syncthreads(); continue; }
        pt_backward(m, lds, tw, tid, nth);
        const float c1 = (float)(1.0 / (1.0 - p1)), c2 = (float)(1.0 / (1.0 - p2));
        pt_update<true>(m, lds, tw, tm, tv, a0, 0.0f, eta, b1, b2, eps_adam, c1, c2, tid, nth);
        p1 *= (double)b1;
        p2 *= (double)b2;
        __syncthreads();
    }
    if (IN_LDS && update) {
        float* gw = theta + base;
        float* gm = mom + base;
        float* gv = vel + base;
        for (int q = tid; q < ns; q += nth) { gw[q] = tw[q]; gm[q] = tm[q]; gv[q] = tv[q]; }
    }
    if (tid == 0) {
        loss_out[chain] = loss_sum;
        if (bt_out && k == 0 && j == __ffs(nets) - 1) { bt_out[0] = p1; bt_out[1] = p2; }     // every selected chain takes the same steps: one writes
    }
}

size_t wm_pretrain_lds_bytes(const DevModel& m, int update) {
    return pretrain_lds_bytes(m) + (WMP_IN_LDS ? (size_t)(update ? 3 : 1) * ((m.net_size + 3) & ~3) * sizeof(float) : 0);
}

hipError_t wmp_set_kernel_attributes(size_t max_lds_bytes) { return set_max_lds(wm_pretrain_ens_kernel, max_lds_bytes); }

hipError_t launch_wm_pretrain_ens(const DevModel& m, int n_models, int nets, const RtPhys* phys, float* theta, float* mom, float* vel, const float* X,
                                  const float* BC, const float* Y, const int* order, int n_samples, float gs, const float* eta, float b1, float b2, float eps,
                                  double bt1, double bt2, int update, float* loss_out, double* bt_out, hipStream_t stream) {
    const size_t lds = wm_pretrain_lds_bytes(m, update);
    if (lds > PRETRAIN_LDS_CAP || n_models < 1 || n_models > 65535 || n_samples < 1 || nets < 1 || nets > 7) return hipErrorInvalidValue;
    if (m.model != COLNDE_MODEL_WIND_MIXING || m.n_nets != 3 || m.n_params != 3 * m.net_size || !phys) return hipErrorInvalidValue;
    if (update && (!mom || !vel || !eta)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wm_pretrain_ens_kernel, dim3(n_models, 3), dim3(WMP_BLOCK), lds, stream, m, nets, phys, theta, mom, vel, X, BC, Y, order, n_samples, gs,
                       eta, b1, b2, eps, bt1, bt2, update, loss_out, bt_out);
    return hipGetLastError();
}
