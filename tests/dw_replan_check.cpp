// Stand-alone host check of the slice rule across a switch of the weight-gradient arithmetic (tests/test_handle_reuse_host.py compiles and runs it; no
// GPU, no library, no preload).  colnde_set_matrix_arithmetic asks csrc/dw_plan.h: dw_slice_count — the rule dw_plan_slices applies when the tape
// planners build a plan — for the arithmetic switched to.  For every network of tests/dw_plan_check.cpp, with and without LDS fit, in both directions:
// the count after the switch is the one a fresh plan of that arithmetic holds, and the kernel that will run takes it.  Beside it the program models
// what the library did before ("keep the count planned for the first arithmetic") and prints whether the launch rule takes THAT count: the test asserts
// that it does not at 12, 36 and 60 records.
// Compiled host-only with hipcc: DevModel and DwMacro live in colnde_dev.h, which includes the HIP headers; nothing here calls HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "dw_plan.h"

#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) { fprintf(stderr, "%s: %s:%d: %s\n", g_net, __FILE__, __LINE__, #c); exit(1); } \
    } while (0)
static const char* g_net = "";

struct Net { const char* name; int n_nets, ns, n_layers, sizes[4]; };
static const Net kNets[] = {      // tests/dw_plan_check.cpp's
    {"3x96-50-20-31", 3, 96, 3, {96, 50, 20, 31}},
    {"fc32_Nz32", 1, 32, 3, {32, 128, 128, 31}},
    {"fc32_Nz64", 1, 64, 3, {64, 256, 256, 63}},
    {"3x96-400-400-31", 3, 96, 3, {96, 400, 400, 31}},
    {"32-128-128-31", 1, 32, 3, {32, 128, 128, 31}},
    {"64-256-256-63", 1, 64, 3, {64, 256, 256, 63}},
};

// the fields of DevModel the plan reads, laid out as build_model (api.hip) lays them out
static DevModel model_of(const Net& n) {
    DevModel m;
    memset(&m, 0, sizeof m);
    m.ns = n.ns;
    m.n_nets = n.n_nets;
    m.n_layers = n.n_layers;
    int woff = 0, aoff = 0;
    for (int l = 0; l <= n.n_layers; l++) m.sizes[l] = n.sizes[l];
    for (int l = 0; l < n.n_layers; l++) {
        const int ni = n.sizes[l], no = n.sizes[l + 1];
        m.w_off[l] = woff;
        woff += ni * no + no;
        m.act_off[l] = aoff;
        aoff += (no + 3) & ~3;
    }
    m.net_size = woff;
    m.n_params = woff * m.n_nets;
    m.act_total = aoff;
    return m;
}

// what the launches ask of a slice count (engine_dwgemm.hip): launch_dw_gemm_split and the LDS-staged branch of launch_dw_gemm take any count >= 1,
// the L2-streaming branch multiples of 8 from 8 up (anything else: hipErrorInvalidValue)
static bool launch_takes(const DwPlan& p, bool sp_dw, int slices) {
    if (sp_dw && !p.passes.empty()) return slices >= 1;
    if (p.lds_fit) return slices >= 1;
    return slices >= 8 && (slices & 7) == 0;
}

int main() {
    const size_t recs[] = {1, 12, 36, 60, 72, 511, 512, 4096};
    for (const Net& n : kNets) {
        g_net = n.name;
        const DevModel m = model_of(n);
        for (size_t n_rec : recs)
            for (int lds_fit = 0; lds_fit < 2; lds_fit++)
                for (int from = 0; from < 2; from++) {
                    const bool to = !from;
                    DwPlan p, fresh;
                    dw_plan_blocks(m, p);
                    dw_plan_slices(p, n_rec, lds_fit != 0, from != 0);          // the handle's first loss_grad plans under `from`
                    CHECK(launch_takes(p, from != 0, p.slices));
                    const int kept = p.slices;                                   // before: the setter left it
                    const int replanned = dw_slice_count(p, n_rec, p.lds_fit, to);      // now: the setter asks the planners' rule
                    dw_plan_blocks(m, fresh);
                    dw_plan_slices(fresh, n_rec, lds_fit != 0, to);
                    CHECK(replanned == fresh.slices);
                    CHECK(launch_takes(p, to, replanned));
                    if (!lds_fit && !(to && p.split_ok)) CHECK(replanned >= 8 && replanned % 8 == 0);      // the f32 L2-streaming kernel will run
                    // ... and back again: the first plan's count
                    p.slices = replanned;
                    CHECK(dw_slice_count(p, n_rec, p.lds_fit, from != 0) == kept);
                    printf("switch %s n_rec %zu lds_fit %d from %d to %d fresh %d replanned %d kept %d kept_launches %d\n", n.name, n_rec, lds_fit, from, (int)to,
                           fresh.slices, replanned, kept, (int)launch_takes(p, to, kept));
                }
    }
    return 0;
}
