// Reads planning cases from stdin, prints what csrc/tape_plan.h plans for each (tests/test_tape_plan.py).  Host only: the header has no HIP in it.
//   B n_padded fit tile granule                              -> block
//   F n32 n_iv cw per_col_iv budget n_params                 -> block seg
//   E n32 n_iv cw Nz per_col_iv budget n_params              -> seg
//   H free margin                                            -> budget
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
        } else {
            return 2;
        }
    }
    return 0;
}
