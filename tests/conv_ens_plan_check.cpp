// Reads planning cases from stdin, prints what csrc/tape_plan.h plans for a conv ensemble (tests/test_conv_ensemble_host.py).  Host only, its own
// main: built with -fsanitize=address,undefined and run as an executable.
//   M n32 n_iv cw Nz per_col_iv n_params seg cslab_seg_floats             -> bytes per model
//   S n32 n_iv cw Nz per_col_iv budget n_params cslab_seg_floats          -> seg  bytes per model at that seg
#include <cstdio>

#include "tape_plan.h"

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        int n32, n_iv, cw, Nz, n_params, seg;
        size_t per_col_iv, budget, cslab;
        if (kind == 'M') {
            if (scanf("%d %d %d %d %zu %d %d %zu", &n32, &n_iv, &cw, &Nz, &per_col_iv, &n_params, &seg, &cslab) != 8) return 2;
            printf("%zu\n", fc_conv_ens_model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg, cslab));
        } else if (kind == 'S') {
            if (scanf("%d %d %d %d %zu %zu %d %zu", &n32, &n_iv, &cw, &Nz, &per_col_iv, &budget, &n_params, &cslab) != 8) return 2;
            seg = plan_fc_conv_ens_seg(n32, n_iv, cw, Nz, per_col_iv, budget, n_params, cslab);
            printf("%d %zu\n", seg, fc_conv_ens_model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg, cslab));
        } else {
            return 2;
        }
    }
    return 0;
}
