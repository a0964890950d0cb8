// dw_plan.h — the dW GEMM's plan (engine_dwgemm.h: DwPlan) on the host: the 64x64 block list of every weight matrix, the passes of the split kernel and
// the number of K-slices of the records.  No HIP calls: plain C++17 over the plain structs, so that tests/dw_plan_check.cpp walks whole plans on the host;
// the API (build_dw_plan) uploads the two block lists into buffers the handle's pool owns.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>
#include "engine_dwgemm.h"

// Deal the blocks to passes (first fit, largest layer first): a pass = the blocks of some (net, layer) groups whose operand features, merged
// into at most 8 even-aligned segments of the record row, are at most 768 (two plane buffers in LDS) and whose blocks are at most 16.
// false (no passes, no compacted list): some matrix does not fit, or the row is odd — the f32 kernels serve the handle.
inline bool dw_plan_passes(const std::vector<DwMacro>& mac, const std::vector<int>& matrix_of, int R, DwPlan& plan) {
    plan.passes.clear();
    plan.split_macros.clear();
    struct Group { std::vector<int> idx; int feats; };
    std::vector<Group> groups;                 // the blocks of one weight matrix (net, layer) stay together
    for (int i = 0; i < (int)mac.size(); i++) {
        if (groups.empty() || matrix_of[i] != matrix_of[groups.back().idx[0]]) groups.push_back(Group{{}, 0});
        groups.back().idx.push_back(i);
    }
    auto segments = [&](const std::vector<int>& idx, std::vector<DwSeg>& segs) {
        std::vector<std::pair<int, int>> iv;
        for (int i : idx) {
            iv.push_back({mac[i].a_feat & ~1, std::min(R, (mac[i].a_feat + mac[i].ni_rem + 1) & ~1)});
            iv.push_back({mac[i].d_feat & ~1, std::min(R, (mac[i].d_feat + mac[i].no_rem + 1) & ~1)});
        }
        std::sort(iv.begin(), iv.end());
        segs.clear();
        int dst = 0;
        for (auto& v : iv) {
            if (!segs.empty() && v.first <= segs.back().src + segs.back().len) {
                const int end = std::max(segs.back().src + segs.back().len, v.second);
                dst += end - (segs.back().src + segs.back().len);
                segs.back().len = end - segs.back().src;
            } else {
                segs.push_back(DwSeg{v.first, v.second - v.first, dst});
                dst += v.second - v.first;
            }
        }
        return dst;
    };
    // A matrix too large for one pass (the wide wind-mixing layers: 400 x 400 = 49 blocks, 800 features) is cut along its OUTPUT blocks into chunks that fit
    // (<= 16 blocks, <= 768 compact features): every chunk keeps all input features of the matrix and takes a run of output-block columns.
    {
        std::vector<Group> cut;
        for (auto& g : groups) {
            std::vector<DwSeg> sg;
            if ((int)g.idx.size() <= 16 && segments(g.idx, sg) <= 768 && sg.size() <= 8) { cut.push_back(g); continue; }
            std::vector<int> dcols;                                  // distinct output-block columns (d_feat) of this matrix, in order
            for (int i : g.idx)
                if (std::find(dcols.begin(), dcols.end(), mac[i].d_feat) == dcols.end()) dcols.push_back(mac[i].d_feat);
            std::sort(dcols.begin(), dcols.end());
            size_t c0 = 0;
            while (c0 < dcols.size()) {
                Group best{{}, 0};
                for (size_t c1 = c0 + 1; c1 <= dcols.size(); c1++) {
                    Group trial{{}, 0};
                    for (int i : g.idx)
                        if (mac[i].d_feat >= dcols[c0] && mac[i].d_feat <= dcols[c1 - 1]) trial.idx.push_back(i);
                    std::vector<DwSeg> st;
                    if ((int)trial.idx.size() > 16 || segments(trial.idx, st) > 768 || st.size() > 8) break;
                    best = trial;
                }
                if (best.idx.empty()) return false;                   // one output-block column alone does not fit
                const int last = mac[best.idx.back()].d_feat;
                cut.push_back(best);
                while (c0 < dcols.size() && dcols[c0] <= last) c0++;
            }
        }
        groups.swap(cut);
    }
    for (auto& g : groups) { std::vector<DwSeg> sg; g.feats = segments(g.idx, sg); }
    std::vector<int> order(groups.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return groups[a].feats > groups[b].feats; });
    std::vector<std::vector<int>> bins;        // macro indices per pass
    for (int gi : order) {
        bool placed = false;
        for (auto& b : bins) {
            std::vector<int> trial = b;
            trial.insert(trial.end(), groups[gi].idx.begin(), groups[gi].idx.end());
            std::vector<DwSeg> sg;
            const int fc = segments(trial, sg);
            if (fc <= 768 && sg.size() <= 8 && trial.size() <= 16) { b = trial; placed = true; break; }
        }
        if (!placed) {
            std::vector<DwSeg> sg;
            const int fc = segments(groups[gi].idx, sg);
            if (fc > 768 || sg.size() > 8 || groups[gi].idx.size() > 16) return false;
            bins.push_back(groups[gi].idx);
        }
    }
    if ((R & 1) != 0) return false;            // 8-byte loads of feature pairs
    for (auto& b : bins) {
        DwPassDesc pd{};
        std::vector<DwSeg> sg;
        pd.Fc = segments(b, sg);
        pd.n_seg = (int)sg.size();
        for (int i = 0; i < pd.n_seg; i++) pd.seg[i] = sg[i];
        pd.m0 = (int)plan.split_macros.size();
        pd.n_macros = (int)b.size();
        pd.maxm = (pd.n_macros + 7) / 8;
        pd.nit = (pd.Fc + 511) / 512;
        auto compact = [&](int feat) {
            for (auto& s : sg) if (feat >= s.src && feat < s.src + s.len) return s.dst + feat - s.src;
            return 0;
        };
        for (int i : b) { DwMacro d = mac[i]; d.a_feat = compact(d.a_feat); d.d_feat = compact(d.d_feat); plan.split_macros.push_back(d); }
        plan.passes.push_back(pd);
    }
    return true;
}

// The work lists: 64x64 blocks of every layer's weight matrix, and the split kernel's passes over them.
// The split (bf16-pipe) dW GEMM keeps only a pass's operand FEATURES in LDS, as planes: it also serves records that do not fit the LDS whole (the wide
// wind-mixing networks: 325 KB per 16-column record), with the large matrices cut into chunks of output blocks (dw_plan_passes).
inline void dw_plan_blocks(const DevModel& m, DwPlan& plan) {
    const size_t R = dwtape_row_floats(m);
    std::vector<DwMacro>& mac = plan.macros;
    mac.clear();
    std::vector<int> matrix_of;
    for (int net = 0; net < m.n_nets; net++)
        for (int l = 0; l < m.n_layers; l++) {
            const int ni = m.sizes[l], no = m.sizes[l + 1];
            for (int i0 = 0; i0 < ni; i0 += 64)
                for (int j0 = 0; j0 < no; j0 += 64) {
                    DwMacro d;
                    d.a_feat = l == 0 ? i0 : dwtape_ns4(m) + net * dwtape_act4(m) + m.act_off[l - 1] + i0;
                    d.d_feat = dwtape_ns4(m) + (m.n_nets + net) * dwtape_act4(m) + m.act_off[l] + j0;
                    d.ni_rem = std::min(64, ni - i0);
                    d.no_rem = std::min(64, no - j0);
                    d.g_off = net * m.net_size + m.w_off[l] + i0 * no + j0;
                    d.no = no;
                    mac.push_back(d);
                    matrix_of.push_back(net * m.n_layers + l);
                }
        }
    plan.n_macros = (int)mac.size();
    plan.split_ok = dw_plan_passes(mac, matrix_of, (int)R, plan);
}

// K-slices of n_rec records.  lds_fit: the LDS-staged f32 kernel applies (dw_gemm_lds_fits, which reads its switch where it always has);
// sp_dw: the handle's weight-gradient arithmetic is the bf16 split.  The one rule: the tape planners call it when they build a plan, and
// colnde_set_matrix_arithmetic calls it again for the arithmetic switched to (the L2-streaming f32 kernel takes multiples of 8 only, the LDS-staged
// and split kernels any count), so that a handle always holds the count a fresh handle of its arithmetic plans.
inline int dw_slice_count(const DwPlan& plan, size_t n_rec, bool lds_fit, bool sp_dw) {
    const int n_groups = (plan.n_macros + 3) / 4;
    size_t slices = std::max<size_t>(8, ((size_t)2048 / n_groups + 7) / 8 * 8);
    slices = std::min(slices, std::max<size_t>(8, (n_rec / 8 + 7) / 8 * 8));
    if (lds_fit || (plan.split_ok && sp_dw))         // one workgroup per CU (two records / two plane buffers in LDS): two rounds of slices
        slices = std::min<size_t>(512, std::max<size_t>(1, n_rec));
    return (int)slices;
}

inline void dw_plan_slices(DwPlan& plan, size_t n_rec, bool lds_fit, bool sp_dw) {
    plan.lds_fit = lds_fit;
    plan.slices = dw_slice_count(plan, n_rec, lds_fit, sp_dw);
}
