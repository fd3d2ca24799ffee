// ppg_logp.h -- ppg_record_logp of include/ppg.h: what the behaviour policy thought of every stored sample of one step -- the
// log-probability of the action taken, the entropy and (on request) the logits themselves -- written into per-species tensors
// indexed by the slot numbers of a ppg_obs_store.
//
// ppg_policy_act leaves its float32 logits env-major in row order: row j of species s in env b is logits row off_s[b] + j, where
// off_s[b] counts the rows of species s in use in the envs below b.  The slots slot[t][b][.] of the same rows are in the store
// already (ppg_record_obs of step t), so two launches, both written against the wave primitives of wave.h (the CPU test build runs the
// same source), put the two together:
//   logp_scan  one wavefront: exclusive prefix sums of the two per-env row counts over B (rows_scan of ppg_rows.h) -> a
//              library-owned [B,2] int32 scratch.
//   logp_rows  one wavefront per env, one lane per row: the row's logits -> log-softmax at the action, entropy, a copy of the logits.
// Arithmetic: float32 logits widened to float64, max-shifted, summed in ascending action order, rounded ONCE to float32 at the store;
// no fused multiply-add (the library is built with -ffp-contract=off).  A logit of -inf is a masked action: its term is skipped,
// never formed as 0 * inf.
// Both kernels find the step index t the same way (ppg_rows.h: RecordedStep; the device word holds t + 1); with t outside [0, T)
// neither writes anything.  A slot number becomes an address only after 0 <= k < capacity was checked, a logits row
// only after 0 <= i < B * rows, an action indexes nothing at all.
// Ordinary vector loads / stores and LDS accesses only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "ppg_rows.h"

namespace ppg {

constexpr uint32_t LOGP_QNAN_BITS = 0x7FC00000u;   // the quiet NaN a float32 tensor filled with NaN holds

struct LogpParams : RecordedStep<1> {   // the device word holds t + 1; T = the horizon: slot is [T,B,S]
    int32_t batch, S, cap_pred, cap_prey;
    const int32_t *env_state;
    const float *logits[2];     // [B * rows_s, n_actions[s]], the first sum_b n_s(b) rows written by ppg_policy_act; NULL: skipped
    int32_t n_actions[2];       // 1 .. 32
    int64_t capacity[2];
    float *logp[2];
    float *entropy[2];          // both NULL, or both set
    uint32_t *dist[2];          // both NULL, or both set: [capacity[s], n_actions[s]] float32, copied as words
    const int32_t *slot;
    const int8_t *actions;      // [B,S]
    int32_t *off;               // library-owned [B,2]: logits row of the env's first row in use, per species
};

PPG_DEVICE float logp_qnan() {
    union { uint32_t u; float f; } v;
    v.u = LOGP_QNAN_BITS;
    return v.f;
}

// ---- launch 1: one wavefront ------------------------------------------------------------------------------------
template <class KP>
PPG_DEVICE void logp_scan_main(const KP &K, unsigned char *lds) {
    auto count = [&](int e, int s) { return (uint32_t)rows_in_use(K, K.env_state + (size_t)e * PPG_ENV_WORDS, s); };
    const RowScan r = rows_scan(K.batch, lds, count);
    if (!step_in_horizon(K, recorded_step(K))) return;   // (logp_rows checks t itself and then reads no offset)
    rows_scan_each(r, count, [&](int e, uint32_t bp, uint32_t bq) {
        K.off[2 * e] = (int32_t)bp;   // (at most B * rows per species, which the host holds below 2^31)
        K.off[2 * e + 1] = (int32_t)bq;
    });
}

// One row of A float32 logits: log-softmax at action a (quiet NaN for an action outside [0, A)) and the entropy, in float64, each
// rounded once.  The row is read three times (maximum, sums, and by the caller for the copy): at most 128 bytes, in cache.
PPG_DEVICE void logp_of_row(const float *row, int A, int a, float &logp, float &entropy) {
    double m = -INFINITY;
    for (int i = 0; i < A; ++i) {
        const double l = (double)row[i];
        if (l > m) m = l;   // (a NaN is never the maximum; it reaches the sum below)
    }
    if (!(m > -INFINITY && m < INFINITY)) {   // no finite maximum: every action masked, or a logit of +inf
        logp = logp_qnan();
        entropy = logp_qnan();
        return;
    }
    double s = 0.0, w = 0.0, da = 0.0;
    for (int i = 0; i < A; ++i) {
        const double d = (double)row[i] - m;   // (exact: both are float32 values)
        if (i == a) da = d;
        if (d == -INFINITY) continue;          // a masked action: exactly 0 in both sums
        const double e = exp(d);
        s += e;
        w += e * d;
    }
    const double ls = log(s);   // s >= 1: the maximum's own term
    logp = a >= 0 && a < A ? (float)(da - ls) : logp_qnan();
    entropy = (float)(ls - w / s);
}

// ---- launch 2: one wavefront per env, one lane per row -----------------------------------------------------------------
template <class KP>
PPG_DEVICE void logp_rows_main(const KP &K) {
    const int b = PPG_BLOCK_INDEX();
    if (b >= K.batch) return;
    const int ln = wv::lane();
    const int64_t t = recorded_step(K);
    if (!step_in_horizon(K, t)) return;   // nothing recorded yet, or a replay past the horizon
    const int S = K.S;
    const int32_t *es = K.env_state + (size_t)b * PPG_ENV_WORDS;
    const size_t at = ((size_t)t * K.batch + (size_t)b) * S;
    // The env's predator rows and then its prey rows share ONE run of lanes (a species without logits has no rows here): at the
    // default population an env has 6 + 7 rows in use, and a lane costs the same whether 6 or 13 of its neighbours work.
    const int n0 = K.logits[0] ? rows_in_use(K, es, 0) : 0, n1 = K.logits[1] ? rows_in_use(K, es, 1) : 0;
    for (int q = ln; q < n0 + n1; q += 64) {
        const bool s = q >= n0;
        const int j = s ? q - n0 : q, first = s ? K.cap_pred : 0, cap = s ? K.cap_prey : K.cap_pred;
        const int A = s ? K.n_actions[1] : K.n_actions[0];
        const int64_t capacity = s ? K.capacity[1] : K.capacity[0], rows = (int64_t)K.batch * cap;
        const int64_t k = K.slot[at + first + j], i = (int64_t)K.off[2 * b + (s ? 1 : 0)] + j;
        if (k < 0 || k >= capacity || i < 0 || i >= rows) continue;   // dropped by the store (-1), or a word that is no slot
        const float *row = (s ? K.logits[1] : K.logits[0]) + (size_t)i * A;
        const int a = K.actions[(size_t)b * S + first + j];
        float lp, h;
        logp_of_row(row, A, a, lp, h);
        (s ? K.logp[1] : K.logp[0])[k] = lp;
        float *entropy = s ? K.entropy[1] : K.entropy[0];
        if (entropy) entropy[k] = h;
        uint32_t *dist = s ? K.dist[1] : K.dist[0];
        if (dist) {
            const uint32_t *src = (const uint32_t *)row;
            uint32_t *dst = dist + (size_t)k * A;
            for (int c = 0; c < A; ++c) dst[c] = src[c];
        }
    }
}

}  // namespace ppg
