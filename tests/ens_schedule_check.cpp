// Reads rounds of the greedy schedule choice from stdin, prints what csrc/step_schedule.h's sched_choose_round decides for each
// (tests/test_ens_schedule_host.py).  Host only: the header has no HIP in it.  Floats cross as their 32 bits (NaN and Inf included).
//   n_save reltol prev_est E_0 .. E_{n_save-1} S_0 .. S_{n_save-2}    ->    verdict est S_0 .. S_{n_save-2}
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "step_schedule.h"

static bool read_float(float* f) {
    uint32_t u;
    if (scanf("%u", &u) != 1) return false;
    memcpy(f, &u, sizeof u);
    return true;
}

int main() {
    int n_save;
    while (scanf("%d", &n_save) == 1) {
        if (n_save < 2) return 2;
        float reltol, prev;
        if (!read_float(&reltol) || !read_float(&prev)) return 2;
        // exactly n_save and n_save - 1 elements: a read or write past either end is AddressSanitizer's to report
        std::vector<float> E((size_t)n_save);
        std::vector<int> S((size_t)n_save - 1);
        for (float& e : E) if (!read_float(&e)) return 2;
        for (int& s : S) if (scanf("%d", &s) != 1) return 2;
        float est = -1.0f;
        const int verdict = (int)sched_choose_round(E.data(), n_save, reltol, prev, S.data(), &est);
        uint32_t u;
        memcpy(&u, &est, sizeof u);
        printf("%d %u", verdict, u);
        for (int s : S) printf(" %d", s);
        printf("\n");
    }
    return 0;
}
