// step_schedule.h — the per-save-interval step schedule (colnde_set_schedule): n_save - 1 positive counts S_n, the RK4 steps of save interval n, the
// same for every column and member; interval n is stepped with dt_n = (t[n+1] - t[n]) / S_n.  Pure host arithmetic — no HIP in here, compiled alone
// by tests/test_schedule_host.py: the per-interval stability minimum, the total, where an interval's steps start in the tapes, what the tapes hold,
// and the validation colnde_set_schedule applies.  Tapes, slab rows and dW record counts are sized by the total: a wrong total is an out-of-bounds write.
#pragma once
#include <cmath>
#include <cstddef>

#define COLNDE_SCHEDULE_MAX 4096     // steps per save interval (the cap of colnde_choose_substeps)

// least number of steps that keeps lambda dt within `bound` on an interval `span` long (colnde_min_substeps's expression, on one interval)
inline int sched_interval_min(double span, double lambda, double bound) {
    const double need = span * lambda / bound;
    return need <= 1.0 ? 1 : (int)ceil(need);
}

inline void sched_minima(const float* save_times, int n_save, double lambda, double bound, int* counts) {
    for (int i = 0; i + 1 < n_save; i++) counts[i] = sched_interval_min((double)save_times[i + 1] - (double)save_times[i], lambda, bound);
}

// the steps of the whole axis; without a schedule (counts == nullptr) every interval takes `substeps`
inline long long sched_total(const int* counts, int n_iv, int substeps = 0) {
    if (!counts) return (long long)n_iv * substeps;
    long long t = 0;
    for (int i = 0; i < n_iv; i++) t += counts[i];
    return t;
}

// the running step index at which interval iv begins: the tapes and the dW records are indexed by it
inline long long sched_offset(const int* counts, int iv) { return sched_total(counts, iv); }

inline int sched_pow2_ceil(int v) {
    int p = 1;
    while (p < v) p *= 2;
    return p;
}

// (tile, step, stage) records of n_tiles tiles, and the floats of a tape that holds rec_floats per record
inline size_t sched_records(size_t n_tiles, long long total_steps, int nst) { return n_tiles * (size_t)total_steps * (size_t)nst; }
inline size_t sched_tape_floats(size_t n_tiles, long long total_steps, int nst, size_t rec_floats) { return sched_records(n_tiles, total_steps, nst) * rec_floats; }

enum SchedVerdict { SCHED_OK = 0, SCHED_NOT_POSITIVE = 1, SCHED_ABOVE_MAX = 2, SCHED_BELOW_MIN = 3 };
// the first count that is refused (*bad: its interval), in this order of reasons per interval; minima may be null (no stability check)
inline SchedVerdict sched_validate(const int* counts, const int* minima, int n_iv, bool allow_unstable, int* bad) {
    for (int i = 0; i < n_iv; i++) {
        SchedVerdict v = SCHED_OK;
        if (counts[i] < 1) v = SCHED_NOT_POSITIVE;
        else if (counts[i] > COLNDE_SCHEDULE_MAX) v = SCHED_ABOVE_MAX;
        else if (minima && counts[i] < minima[i] && !allow_unstable) v = SCHED_BELOW_MIN;
        if (v != SCHED_OK) {
            if (bad) *bad = i;
            return v;
        }
    }
    return SCHED_OK;
}

// One round of the greedy choice (colnde_choose_schedule's rule; colnde_ensemble_choose_schedule applies it through this function).  E[n_save]: the
// estimate at every save point alone — of an ensemble already the maximum over the members — with Richardson's factor applied; prev_est: the last
// round's *est (<= 0: none); S[n_save - 1]: the counts the estimates were formed at, doubled in place where the rule says so.  *est = max E.
//   NOT_FINITE  an entry is NaN or above 3e38 (S untouched; *est = that entry)
//   MET         est <= reltol
//   FLOOR       the estimate fell by less than a fifth since the last round: float32 round-off of the two solves it compares
//   DOUBLED     every interval whose own addition d[n] = max(0, E[n+1] - E[n]) (E[0] taken as 0) is at least half the largest, and below
//               COLNDE_SCHEDULE_MAX, was doubled
//   TOO_STIFF   none could be
enum SchedRound { SCHED_ROUND_MET = 0, SCHED_ROUND_DOUBLED = 1, SCHED_ROUND_NOT_FINITE = 2, SCHED_ROUND_FLOOR = 3, SCHED_ROUND_TOO_STIFF = 4 };
inline SchedRound sched_choose_round(const float* E, int n_save, float reltol, float prev_est, int* S, float* est) {
    float mx = 0.0f;
    for (int i = 0; i < n_save; i++) {
        if (!(E[i] == E[i]) || E[i] > 3.0e38f) {
            *est = E[i];
            return SCHED_ROUND_NOT_FINITE;
        }
        if (E[i] > mx) mx = E[i];
    }
    *est = mx;
    if (mx <= reltol) return SCHED_ROUND_MET;
    if (prev_est > 0.0f && mx > 0.8f * prev_est) return SCHED_ROUND_FLOOR;
    const int n_iv = n_save - 1;
    float dmax = 0.0f;
    for (int i = 0; i < n_iv; i++) {
        const float d = E[i + 1] - (i ? E[i] : 0.0f);
        if (d > dmax) dmax = d;
    }
    bool doubled = false;
    for (int i = 0; i < n_iv; i++) {
        const float d = E[i + 1] - (i ? E[i] : 0.0f);
        if ((d > 0.0f ? d : 0.0f) >= 0.5f * dmax && S[i] < COLNDE_SCHEDULE_MAX) {
            S[i] *= 2;
            doubled = true;
        }
    }
    return doubled ? SCHED_ROUND_DOUBLED : SCHED_ROUND_TOO_STIFF;
}
