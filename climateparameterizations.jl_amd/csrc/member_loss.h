// member_loss.h — the member loss of an ensemble (colnde_ensemble_set_member_loss): member k's loss is
//     Σ_q s[k][q] · Σ_c w[k][c] · (term q of column c) / Σ_c w[k][c]
// with its own six scalings s[k] and its own column weights w[k] — determine_loss_scalings per run (wind_mixing/src/NDE_training.jl:256-288 feeding
// calculate_loss_scalings, loss.jl:11-31) and the training-simulations axis (train_free_convection_nde.jl:60-66: a 0/1 weight per simulation).
// Pure host arithmetic — no HIP in here, compiled alone by tests/test_member_loss_host.py: the validation colnde_ensemble_set_member_loss applies and the
// K LossWeights the kernels read, formed in double by the expression of loss_weights() (api.hip) with Σ_c w[k][c] in n_col_total's place.
#pragma once
#include <cmath>
#include <cstddef>

enum MemberLossVerdict {
    MEMBER_LOSS_OK = 0,
    MEMBER_LOSS_BAD_SCALING = 1,      // a scaling that is negative or not finite (*bad_k, *bad_i: member, term)
    MEMBER_LOSS_BAD_WEIGHT = 2,       // a column weight that is negative or not finite (*bad_k, *bad_i: member, column)
    MEMBER_LOSS_EMPTY_MEMBER = 3,     // a member whose column weights sum to 0 (*bad_k)
    MEMBER_LOSS_GLOBAL_COLUMNS = 4    // the handle is a shard of a larger problem: the normaliser would be a global sum
};

// what describes the member loss in force: none | scalings | columns | scalings+columns
inline const char* member_loss_kind(bool have_scalings, bool have_columns) {
    return have_scalings ? (have_columns ? "scalings+columns" : "scalings") : (have_columns ? "columns" : "none");
}

// Σ_c w[c] in double, in column order (w == nullptr: every column 1)
inline double member_weight_sum(const float* w, int n_col) {
    if (!w) return (double)n_col;
    double s = 0.0;
    for (int c = 0; c < n_col; c++) s += (double)w[c];
    return s;
}

// the first entry that is refused, in this order: the handle's column counts, then member by member its scalings, its weights, their sum.
// scalings [K][6] and column_weights [K][n_col] may each be null.
inline MemberLossVerdict member_loss_validate(const float* scalings, const float* column_weights, int K, int n_col, long long n_col_total, int* bad_k, int* bad_i) {
    if (n_col_total != (long long)n_col) return MEMBER_LOSS_GLOBAL_COLUMNS;
    for (int k = 0; k < K; k++) {
        if (scalings)
            for (int q = 0; q < 6; q++) {
                const float s = scalings[(size_t)k * 6 + q];
                if (!std::isfinite(s) || s < 0.0f) {
                    if (bad_k) *bad_k = k;
                    if (bad_i) *bad_i = q;
                    return MEMBER_LOSS_BAD_SCALING;
                }
            }
        if (column_weights) {
            const float* w = column_weights + (size_t)k * n_col;
            for (int c = 0; c < n_col; c++)
                if (!std::isfinite(w[c]) || w[c] < 0.0f) {
                    if (bad_k) *bad_k = k;
                    if (bad_i) *bad_i = c;
                    return MEMBER_LOSS_BAD_WEIGHT;
                }
            if (!(member_weight_sum(w, n_col) > 0.0)) {
                if (bad_k) *bad_k = k;
                return MEMBER_LOSS_EMPTY_MEMBER;
            }
        }
    }
    return MEMBER_LOSS_OK;
}

// Member k's eight weights: loss_weights()'s expression with the member's weight sum for the column count.  wind_mixing: the three profile terms over
// sum * n_save * Nz elements and the three gradient terms over sum * n_save * (Nz + 1); otherwise only w[2] (the temperature profile term) is formed
// and only scalings[2] is read.
inline void member_loss_weights(const float scalings6[6], double weight_sum, int n_save, int Nz, bool wind_mixing, float w8[8]) {
    const double np = weight_sum * n_save * Nz;
    const double ng = weight_sum * n_save * (Nz + 1);
    for (int q = 0; q < 8; q++) w8[q] = 0.0f;
    if (wind_mixing) {
        for (int k = 0; k < 3; k++) {
            w8[k] = (float)(scalings6[k] / np);
            w8[3 + k] = (float)(scalings6[3 + k] / ng);
        }
    } else {
        w8[2] = (float)(scalings6[2] / np);
    }
}
