// Stand-alone host check of csrc/dw_plan.h (tests/test_dw_plan.py compiles and runs it; no GPU, no library, no preload).
// Walks the dW GEMM's plan for the networks below, asserts the planner's invariants, and prints every plan as text: the test compares that text,
// value for value, with tests/golden/dw_plan_parent.txt, which was recorded from the code dw_plan.h replaced.
// Compiled host-only with hipcc: DevModel and DwMacro live in colnde_dev.h, which includes the HIP headers; nothing here calls HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dw_plan.h"

#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) { fprintf(stderr, "%s: %s:%d: %s\n", g_net, __FILE__, __LINE__, #c); exit(1); } \
    } while (0)
static const char* g_net = "";

struct Net { const char* name; int n_nets, ns, n_layers, sizes[4]; };
static const Net kNets[] = {
    {"3x96-50-20-31", 3, 96, 3, {96, 50, 20, 31}},          // the wind-mixing shape (net-split pair, ensembles)
    {"fc32_Nz32", 1, 32, 3, {32, 128, 128, 31}},             // the free-convection engine's records are tile16's
    {"fc32_Nz64", 1, 64, 3, {64, 256, 256, 63}},
    {"3x96-400-400-31", 3, 96, 3, {96, 400, 400, 31}},       // records do not fit the LDS: the 400 x 400 matrices are cut into chunks
    {"32-128-128-31", 1, 32, 3, {32, 128, 128, 31}},         // tile16's taped adjoint on the same two shapes
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

static void print_macro(const char* tag, int i, const DwMacro& d) {
    printf("%s %d a_feat %d d_feat %d ni_rem %d no_rem %d g_off %d no %d\n", tag, i, d.a_feat, d.d_feat, d.ni_rem, d.no_rem, d.g_off, d.no);
}

static bool same_block(const DwMacro& a, const DwMacro& b) { return a.g_off == b.g_off && a.ni_rem == b.ni_rem && a.no_rem == b.no_rem && a.no == b.no; }

static void check_passes(const DwPlan& p, int R) {
    CHECK(p.split_ok == !p.passes.empty());
    if (!p.split_ok) { CHECK(p.split_macros.empty()); return; }
    CHECK((R & 1) == 0);
    // every block of the f32 list appears in exactly one pass (g_off names a block: its first element in the flat gradient)
    CHECK(p.split_macros.size() == p.macros.size());
    std::vector<int> seen(p.macros.size(), 0);
    int m0 = 0;
    for (const DwPassDesc& pd : p.passes) {
        CHECK(pd.m0 == m0 && pd.n_macros >= 1 && pd.n_macros <= 16 && pd.Fc >= 2 && pd.Fc <= 768 && (pd.Fc & 1) == 0 && pd.n_seg >= 1 && pd.n_seg <= 8);
        CHECK(pd.maxm == (pd.n_macros + 7) / 8 && pd.maxm <= 2 && pd.nit == (pd.Fc + 511) / 512 && pd.nit <= 2);      // (the kernel table: [maxm > 1][nit > 1])
        int dst = 0;
        for (int s = 0; s < pd.n_seg; s++) {                 // even-aligned pieces of the row, in order, compacted back to back
            const DwSeg& sg = pd.seg[s];
            CHECK(sg.len > 0 && (sg.src & 1) == 0 && (sg.len & 1) == 0 && sg.src + sg.len <= R && sg.dst == dst);
            if (s) CHECK(sg.src > pd.seg[s - 1].src + pd.seg[s - 1].len);
            dst += sg.len;
        }
        CHECK(dst == pd.Fc);
        for (int k = 0; k < pd.n_macros; k++) {
            const DwMacro& c = p.split_macros[pd.m0 + k];
            int found = -1;
            for (size_t i = 0; i < p.macros.size(); i++)
                if (same_block(p.macros[i], c)) { CHECK(found < 0); found = (int)i; }
            CHECK(found >= 0);
            seen[found]++;
            const DwMacro& f = p.macros[found];
            // compacted features lie inside their segment, at the offset the row feature has in it — the whole operand run of the block does
            auto inside = [&](int feat, int cfeat, int n) {
                for (int s = 0; s < pd.n_seg; s++) {
                    const DwSeg& sg = pd.seg[s];
                    if (feat >= sg.src && feat < sg.src + sg.len) return cfeat == sg.dst + feat - sg.src && feat + n <= sg.src + sg.len && cfeat + n <= pd.Fc;
                }
                return false;
            };
            CHECK(inside(f.a_feat, c.a_feat, f.ni_rem) && inside(f.d_feat, c.d_feat, f.no_rem));
        }
        m0 += pd.n_macros;
    }
    CHECK(m0 == (int)p.split_macros.size());
    for (int s : seen) CHECK(s == 1);
}

static int slice_rule(int n_macros, size_t n_rec, bool one_wg_per_cu) {
    if (one_wg_per_cu) return (int)(n_rec < 1 ? 1 : n_rec > 512 ? 512 : n_rec);
    const size_t n_groups = (size_t)(n_macros + 3) / 4;
    size_t a = (2048 / n_groups + 7) / 8 * 8, b = (n_rec / 8 + 7) / 8 * 8;
    if (a < 8) a = 8;
    if (b < 8) b = 8;
    return (int)(a < b ? a : b);
}

int main() {
    for (const Net& n : kNets) {
        g_net = n.name;
        const DevModel m = model_of(n);
        const int R = (int)dwtape_row_floats(m);
        DwPlan p;
        dw_plan_blocks(m, p);
        int blocks = 0;
        for (int l = 0; l < n.n_layers; l++) blocks += n.n_nets * ((n.sizes[l] + 63) / 64) * ((n.sizes[l + 1] + 63) / 64);
        CHECK(p.n_macros == blocks && (int)p.macros.size() == blocks);
        for (const DwMacro& d : p.macros)
            CHECK(d.ni_rem >= 1 && d.ni_rem <= 64 && d.no_rem >= 1 && d.no_rem <= 64 && d.a_feat >= 0 && d.a_feat + d.ni_rem <= R && d.d_feat + d.no_rem <= R &&
                  d.g_off >= 0 && d.g_off + (d.ni_rem - 1) * d.no + d.no_rem <= m.n_params);
        check_passes(p, R);
        printf("net %s R %d n_macros %d\n", n.name, R, p.n_macros);
        for (int i = 0; i < p.n_macros; i++) print_macro("mac", i, p.macros[i]);
        printf("split_ok %d passes %d\n", (int)p.split_ok, (int)p.passes.size());
        for (size_t q = 0; q < p.passes.size(); q++) {
            const DwPassDesc& pd = p.passes[q];
            printf("pass %d n_seg %d Fc %d m0 %d n_macros %d maxm %d nit %d\n", (int)q, pd.n_seg, pd.Fc, pd.m0, pd.n_macros, pd.maxm, pd.nit);
            for (int s = 0; s < pd.n_seg; s++) printf("seg %d %d src %d len %d dst %d\n", (int)q, s, pd.seg[s].src, pd.seg[s].len, pd.seg[s].dst);
        }
        for (size_t i = 0; i < p.split_macros.size(); i++) print_macro("smac", (int)i, p.split_macros[i]);
        for (size_t n_rec : {(size_t)1, (size_t)12, (size_t)4096})
            for (int lds_fit = 0; lds_fit < 2; lds_fit++)
                for (int sp_dw = 0; sp_dw < 2; sp_dw++) {
                    dw_plan_slices(p, n_rec, lds_fit != 0, sp_dw != 0);
                    CHECK(p.lds_fit == (lds_fit != 0) && p.slices == slice_rule(p.n_macros, n_rec, lds_fit || (p.split_ok && sp_dw)));
                    CHECK(lds_fit || (p.split_ok && sp_dw) || (p.slices >= 8 && p.slices % 8 == 0));      // what the L2-streaming kernel's launch asks for
                    printf("slices n_rec %zu lds_fit %d sp_dw %d = %d\n", n_rec, lds_fit, sp_dw, p.slices);
                }
    }
    return 0;
}
