// Reads planning cases from stdin, prints what csrc/tape_plan.h plans for a tile ensemble (tests/test_tile_ensemble_host.py).  Host only, its own
// main: built with -fsanitize=address,undefined and run as an executable.
//   K n_tiles n_steps nst ns n_params n_col n_save slab_rows row_floats ztape_col_floats image_floats plane_words ag_floats_per_tile free_bytes
//       -> records  bytes per model  a model's share of the budget  refused (0 | 1)
#include <cstdio>

#include "tape_plan.h"

int main() {
    T16TileEnsIn in;
    while (scanf("%d %d %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu", &in.K, &in.n_tiles, &in.n_steps, &in.nst, &in.ns, &in.n_params, &in.n_col, &in.n_save,
                 &in.slab_rows, &in.row_floats, &in.ztape_col_floats, &in.image_floats, &in.plane_words, &in.ag_floats_per_tile, &in.free_bytes) == 15) {
        const T16TileEns p = plan_t16_tile_ens(in);
        printf("%zu %zu %zu %d\n", p.records, p.bytes_per_model, p.share, p.refused ? 1 : 0);
    }
    return 0;
}
