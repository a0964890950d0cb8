// Reads planning cases from stdin, prints what csrc/tape_plan.h plans for each (tests/test_tape_plan.py).  Host only: the header has no HIP in it.
//   B n_padded fit tile granule                              -> block
//   F n32 n_iv cw per_col_iv budget n_params                 -> block seg
//   E n32 n_iv cw Nz per_col_iv budget n_params              -> seg
//   H free margin                                            -> budget
//   P substeps nst row_floats mask_words cw switch conv_floats -> fc32's bytes of tape per column and save interval
//   T n32 n_iv cw Nz n_params per_col_iv free ensemble K cslab_seg_floats forced_block forced_seg -> block seg model_bytes status      (plan_fc_tapes)
//   S n16 tile ns n_bias ag_rows adj_split lds lds_noA lds_ag per_col per_col_rich budget dwtape ztape split_rich forced_block
//                                                            -> status need_z block rich                                               (plan_t16_tapes)
//   N K n_tiles per_model_rich per_model_plain budget split_rich -> rich bytes_per_model refused                                      (plan_t16_ens_tapes)
//   R n32 per_col_x per_col_2 per_col_z budget want_z forced_block -> block ztape                                                      (plan_rt_tapes)
// Flags are -1 (unset), 0, 1; forced blocks and segments 0 when unset.
#include <cstdio>

#include "tape_plan.h"

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'B') {
            int n, tile, granule;
            size_t fit;
            if (scanf("%d %zu %d %d", &n, &fit, &tile, &granule) != 4) return 2;
            printf("%d\n", plan_column_block(n, fit, tile, granule));
        } else if (kind == 'F') {
            int n32, n_iv, cw, n_params;
            size_t per_col_iv, budget;
            if (scanf("%d %d %d %zu %zu %d", &n32, &n_iv, &cw, &per_col_iv, &budget, &n_params) != 6) return 2;
            const FcTapePlan p = plan_fc_block_seg(n32, n_iv, cw, per_col_iv, budget, n_params);
            printf("%d %d\n", p.block, p.seg);
        } else if (kind == 'E') {
            int n32, n_iv, cw, Nz, n_params;
            size_t per_col_iv, budget;
            if (scanf("%d %d %d %d %zu %zu %d", &n32, &n_iv, &cw, &Nz, &per_col_iv, &budget, &n_params) != 7) return 2;
            printf("%d\n", plan_fc_ens_seg(n32, n_iv, cw, Nz, per_col_iv, budget, n_params));
        } else if (kind == 'H') {
            size_t free_b, margin;
            if (scanf("%zu %zu", &free_b, &margin) != 2) return 2;
            printf("%zu\n", hbm_budget(free_b, margin));
        } else if (kind == 'P') {
            int substeps, nst, cw, sw;
            size_t row, mask, conv;
            if (scanf("%d %d %zu %zu %d %d %zu", &substeps, &nst, &row, &mask, &cw, &sw, &conv) != 7) return 2;
            printf("%zu\n", fc_tape_bytes_per_col_iv(substeps, nst, row, mask, cw, sw != 0, conv));
        } else if (kind == 'T') {
            FcTapesIn in;
            int ens;
            if (scanf("%d %d %d %d %d %zu %zu %d %d %zu %d %d", &in.n32, &in.n_iv, &in.cw, &in.Nz, &in.n_params, &in.per_col_iv, &in.free_bytes, &ens, &in.K,
                      &in.cslab_seg_floats, &in.forced_block, &in.forced_seg) != 12) return 2;
            in.ensemble = ens != 0;
            const FcTapes p = plan_fc_tapes(in);
            printf("%d %d %zu %d\n", p.block, p.seg, p.model_bytes, (int)p.status);
        } else if (kind == 'S') {
            T16TapesIn in;
            int ag, split;
            if (scanf("%d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %d %d %d %d", &in.n16, &in.tile, &in.ns, &in.n_bias, &ag, &split, &in.lds_adjoint, &in.lds_adjoint_noA,
                      &in.lds_adjoint_ag, &in.per_col, &in.per_col_rich, &in.budget, &in.dwtape, &in.ztape, &in.split_rich, &in.forced_block) != 16) return 2;
            in.ag_rows = ag != 0;
            in.adj_split = split != 0;
            const T16Tapes p = plan_t16_tapes(in);
            printf("%d %d %d %d\n", (int)p.status, (int)p.need_z, p.block, (int)p.rich);
        } else if (kind == 'N') {
            int K, n_tiles, rich;
            size_t pm_rich, pm_plain, budget;
            if (scanf("%d %d %zu %zu %zu %d", &K, &n_tiles, &pm_rich, &pm_plain, &budget, &rich) != 6) return 2;
            const T16EnsTapes p = plan_t16_ens_tapes(K, n_tiles, pm_rich, pm_plain, budget, rich);
            printf("%d %zu %d\n", (int)p.rich, p.bytes_per_model, (int)p.refused);
        } else if (kind == 'R') {
            int n32, want_z, forced;
            size_t px, p2, pz, budget;
            if (scanf("%d %zu %zu %zu %zu %d %d", &n32, &px, &p2, &pz, &budget, &want_z, &forced) != 7) return 2;
            const RtTapes p = plan_rt_tapes(n32, px, p2, pz, budget, want_z != 0, forced);
            printf("%d %d\n", p.block, (int)p.ztape);
        } else {
            return 2;
        }
    }
    return 0;
}
