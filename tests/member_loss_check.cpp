// Reads member-loss cases from stdin, prints what csrc/member_loss.h computes for each (tests/test_member_loss_host.py).  Host only: the header has no
// HIP in it.  Floats travel as their bit patterns (hex), so that NaN, infinities and the last bit survive the text.
//   W wind_mixing n_save Nz K n_col have_scalings have_weights [K*6 scalings] [K*n_col weights]   -> K lines of 8 weight bit patterns
//   V K n_col n_col_total have_scalings have_weights [K*6 scalings] [K*n_col weights]             -> verdict bad_k bad_i
//   N have_scalings have_columns                                                                   -> the word colnde_describe prints
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "member_loss.h"

static bool read_floats(std::vector<float>& v) {
    for (float& f : v) {
        unsigned bits;
        if (scanf("%x", &bits) != 1) return false;
        const uint32_t b = bits;
        memcpy(&f, &b, sizeof f);
    }
    return true;
}

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'W') {
            int wm, n_save, Nz, K, n_col, hs, hw;
            if (scanf("%d %d %d %d %d %d %d", &wm, &n_save, &Nz, &K, &n_col, &hs, &hw) != 7) return 2;
            std::vector<float> sc(hs ? (size_t)K * 6 : 0), cw(hw ? (size_t)K * n_col : 0);
            if (!read_floats(sc) || !read_floats(cw)) return 2;
            const float ones[6] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
            for (int k = 0; k < K; k++) {
                float w8[8];
                member_loss_weights(hs ? sc.data() + (size_t)k * 6 : ones, member_weight_sum(hw ? cw.data() + (size_t)k * n_col : nullptr, n_col), n_save, Nz, wm != 0, w8);
                for (int q = 0; q < 8; q++) {
                    uint32_t b;
                    memcpy(&b, &w8[q], sizeof b);
                    printf("%08x%c", (unsigned)b, q == 7 ? '\n' : ' ');
                }
            }
        } else if (kind == 'V') {
            int K, n_col, hs, hw;
            long long total;
            if (scanf("%d %d %lld %d %d", &K, &n_col, &total, &hs, &hw) != 5) return 2;
            std::vector<float> sc(hs ? (size_t)K * 6 : 0), cw(hw ? (size_t)K * n_col : 0);
            if (!read_floats(sc) || !read_floats(cw)) return 2;
            int bk = -1, bi = -1;
            const int v = (int)member_loss_validate(hs ? sc.data() : nullptr, hw ? cw.data() : nullptr, K, n_col, total, &bk, &bi);
            printf("%d %d %d\n", v, bk, bi);
        } else if (kind == 'N') {
            int hs, hc;
            if (scanf("%d %d", &hs, &hc) != 2) return 2;
            printf("%s\n", member_loss_kind(hs != 0, hc != 0));
        } else {
            return 2;
        }
    }
    return 0;
}
