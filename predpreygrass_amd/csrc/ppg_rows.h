// ppg_rows.h -- what the learner-side kernels (ppg_pack.h, ppg_record.h, ppg_obs_store.h, ppg_logp.h) share: the rows an env has in
// use, the one-wave prefix sum over per-env row counts, and the step index a recording kernel is launched with.  Written against
// the wave primitives of wave.h (the CPU test build runs the same source).
#pragma once

#include <stdint.h>

#include "../../include/ppg.h"

#ifndef PPG_WAVE_EMU
#include "wave.h"
#endif

namespace ppg {

// rows in use of species s in an env, as ppg_record's in_use sees them: never more than the region holds
template <class KP>
PPG_DEVICE int rows_in_use(const KP &K, const int32_t *es, int s) {
    const int n = es[s ? PPG_ENV_N_PREY_ROWS : PPG_ENV_N_PRED_ROWS], cap = s ? K.cap_prey : K.cap_pred;
    return n < 0 ? 0 : n > cap ? cap : n;
}

// ---- the row scan: ONE wavefront, exclusive prefix sums of per-env {predator, prey} counts ----------------------------------------
// Lane l owns the run of envs [lo, hi) = (n_envs + 63) / 64 consecutive ones.  Sums are uint32 and wrap; they are formed env by env
// within a run and run by run in lane order.
constexpr int ROWS_SCAN_LDS_BYTES = 64 * 2 * 4;   // the [64][2] run totals

struct RowScan {
    int lo, hi;          // this lane's envs
    uint32_t base[2];    // rows of each species in the envs below lo
    uint32_t total[2];   // rows of each species in all envs
};

// count(e, s): rows of species s in env e
template <class Count>
PPG_DEVICE RowScan rows_scan(int n_envs, unsigned char *lds, Count count) {
    const int ln = wv::lane();
    uint32_t *tot = (uint32_t *)lds;  // [64][2]
    const int per = (n_envs + 63) / 64;
    RowScan r;
    r.lo = ln * per < n_envs ? ln * per : n_envs;
    r.hi = (r.lo + per) < n_envs ? (r.lo + per) : n_envs;
    uint32_t sp = 0, sq = 0;
    for (int e = r.lo; e < r.hi; ++e) {
        sp += count(e, 0);
        sq += count(e, 1);
    }
    tot[2 * ln] = sp;
    tot[2 * ln + 1] = sq;
    wv::sync();
    r.base[0] = r.base[1] = r.total[0] = r.total[1] = 0;
    for (int l = 0; l < 64; ++l) {
        const uint32_t a = tot[2 * l], b = tot[2 * l + 1];
        if (l < ln) { r.base[0] += a; r.base[1] += b; }
        r.total[0] += a; r.total[1] += b;
    }
    return r;
}

// the second pass over the lane's envs: emit(e, rows of predators below e, rows of prey below e)
template <class Count, class Emit>
PPG_DEVICE void rows_scan_each(const RowScan &r, Count count, Emit emit) {
    uint32_t bp = r.base[0], bq = r.base[1];
    for (int e = r.lo; e < r.hi; ++e) {
        emit(e, bp, bq);
        bp += count(e, 0);
        bq += count(e, 1);
    }
}

// ---- the recorded step --------------------------------------------------------------------------------------------------------------
// A recording kernel finds its step index t in a launch argument, or (step_on_device) in an int32 word in device memory read when
// the kernel runs, so that a hipGraph holding step + record can be replayed while another node of the graph counts the word up.
// The word holds t + BIAS.  A parameter block takes these four fields by deriving from RecordedStep<BIAS>: the bias is stated
// there, once per call.  With t outside [0, T) a kernel writes nothing of the step: the ONLY uses of t as an index come after
// step_in_horizon().
template <int BIAS>
struct RecordedStep {
    static constexpr int step_word_bias = BIAS;
    int32_t T;                  // horizon: the recorded tensors are [T,B,S]
    int32_t step_on_device;     // t = *step_dev - BIAS when the kernel runs, else t = step
    int32_t step;               // checked against [0, T) by the host
    const int32_t *step_dev;
};

// int64 so that word - bias cannot overflow (every lane reads the same word)
template <class KP>
PPG_DEVICE int64_t recorded_step(const KP &K) { return K.step_on_device ? (int64_t)K.step_dev[0] - K.step_word_bias : (int64_t)K.step; }

template <class KP>
PPG_DEVICE bool step_in_horizon(const KP &K, int64_t t) { return t >= 0 && t < K.T; }

}  // namespace ppg
