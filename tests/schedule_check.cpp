// Reads schedule cases from stdin, prints what csrc/step_schedule.h computes for each (tests/test_schedule_host.py).  Host only: the header has no HIP in it.
//   T n_iv substeps c_0 .. c_{n_iv-1}        -> total(schedule) total(no schedule) offset_0 .. offset_{n_iv}
//   R n_tiles nst rec_floats n_iv c_0 ..     -> records tape_floats
//   M span lambda bound                      -> minimum
//   V allow n_iv c_0 .. m_0 ..               -> verdict bad
//   P v                                      -> pow2_ceil
#include <cstdio>
#include <vector>

#include "step_schedule.h"

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'T') {
            int n_iv, substeps;
            if (scanf("%d %d", &n_iv, &substeps) != 2) return 2;
            std::vector<int> c(n_iv);
            for (int& v : c) if (scanf("%d", &v) != 1) return 2;
            printf("%lld %lld", sched_total(c.data(), n_iv), sched_total(nullptr, n_iv, substeps));
            for (int i = 0; i <= n_iv; i++) printf(" %lld", sched_offset(c.data(), i));
            printf("\n");
        } else if (kind == 'R') {
            size_t n_tiles, rec_floats;
            int nst, n_iv;
            if (scanf("%zu %d %zu %d", &n_tiles, &nst, &rec_floats, &n_iv) != 4) return 2;
            std::vector<int> c(n_iv);
            for (int& v : c) if (scanf("%d", &v) != 1) return 2;
            const long long total = sched_total(c.data(), n_iv);
            printf("%zu %zu\n", sched_records(n_tiles, total, nst), sched_tape_floats(n_tiles, total, nst, rec_floats));
        } else if (kind == 'M') {
            double span, lambda, bound;
            if (scanf("%lf %lf %lf", &span, &lambda, &bound) != 3) return 2;
            printf("%d\n", sched_interval_min(span, lambda, bound));
        } else if (kind == 'V') {
            int allow, n_iv;
            if (scanf("%d %d", &allow, &n_iv) != 2) return 2;
            std::vector<int> c(n_iv), m(n_iv);
            for (int& v : c) if (scanf("%d", &v) != 1) return 2;
            for (int& v : m) if (scanf("%d", &v) != 1) return 2;
            int bad = -1;
            const int verdict = (int)sched_validate(c.data(), m.data(), n_iv, allow != 0, &bad);
            printf("%d %d\n", verdict, bad);
        } else if (kind == 'P') {
            int v;
            if (scanf("%d", &v) != 1) return 2;
            printf("%d\n", sched_pow2_ceil(v));
        } else {
            return 2;
        }
    }
    return 0;
}
