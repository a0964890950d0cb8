// Reads layer-size lists from stdin, prints what csrc/engine_wm_embed_any.h plans for each (tests/test_wm_generic_host.py).  Host only: the plan part of
// the header has no HIP in it.
//   n_layers s_0 .. s_{n_layers}   -> bytes fits st g xs y buf0 buf1 ld0 ld1
#include <cstdio>
#include <vector>

#include "engine_wm_embed_any.h"

int main() {
    int n_layers;
    while (scanf("%d", &n_layers) == 1) {
        if (n_layers < 1 || n_layers > WMA_MAX_LAYERS) return 2;
        std::vector<int> s(n_layers + 1);
        for (int& v : s) if (scanf("%d", &v) != 1) return 2;
        const WmAnyPlan p = wm_any_plan(n_layers, s.data());
        printf("%zu %d %d %d %d %d %d %d %d %d\n", p.bytes, wm_any_fits(p) ? 1 : 0, p.st, p.g, p.xs, p.y, p.buf[0], p.buf[1], p.ld[0], p.ld[1]);
    }
    return 0;
}
