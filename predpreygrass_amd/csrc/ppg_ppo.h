// ppg_ppo.h -- ppg_ppo_loss of include/ppg.h: PPO's clipped surrogate, value, entropy and KL terms over one minibatch of one species,
// and their gradients with respect to the learner's logits and values, from the columns the sample store keeps per slot.
//
// Two launches of one-wave workgroups over chunks of PPG_PPO_CHUNK = 1024 minibatch rows, both written against the wave primitives of
// wave.h (the CPU test build runs the same source).  Lane l of workgroup g owns rows i = 1024 g + 64 j + l, j = 0 .. 15 ascending:
//   ppo_count  counts the chunk's valid rows -> partial[g][0].
//   ppo_rows   adds partial[0..G)[0] in ascending g (every workgroup, every lane: the same n and w = 1 / n), then per valid row the
//              arithmetic of include/ppg.h line by line -- float64, max-shifted like logp_of_row of ppg_logp.h, sums in ascending
//              action order, one rounding to float32 at each store, no fused multiply-add (the library is built with
//              -ffp-contract=off) -- the gradient row, the value gradient, and seven float64 accumulators per lane that an xor
//              butterfly combines at the end (the order ppg_backward_samples fixes for its stats) -> partial[g][1..8).
// Column 0 of partial is written only by the first launch and columns 1..7 only by the second: no scratch, no initial value.
// A row's exp(d_c) of the new and of the old logits are kept in LDS between the passes over the actions -- [32][64] float64 each, a
// lane reads and writes only its own column, consecutive lanes consecutive words -- so every exp is formed once and no array is indexed
// at run time in registers (no scratch).
// A slot number becomes an address only after 0 <= k < capacity was checked; an action is compared with [0, A) and with c, and never
// becomes an address.  An invalid row (include/ppg.h) is a selection: none of its other columns and nothing of its logits row is read.
// Ordinary vector loads / stores, LDS accesses and wave shuffles only: no atomics.
#pragma once

#include <math.h>
#include <stdint.h>

#include "ppg_rows.h"

namespace ppg {

constexpr int PPO_CHUNK = PPG_PPO_CHUNK;          // minibatch rows of one workgroup
constexpr int PPO_MAX_ACTIONS = 32;
constexpr int PPO_LDS_BYTES = 2 * PPO_MAX_ACTIONS * 64 * 8;   // exp(d_c) of the new | of the old logits, float64 [32][64] each
constexpr int PPO_PARTIAL = 8;                    // columns of partial

struct PpoParams {
    int64_t M;                  // 1 .. INT32_MAX (the host checks)
    int64_t capacity;           // 0 .. INT32_MAX
    int32_t A;                  // 1 .. 32
    int32_t G;                  // ceil(M / PPO_CHUNK)
    const int32_t *index;       // [M] or NULL: k = i
    const float *logits;        // [M,A]
    const float *values;        // [M] or NULL
    const int8_t *action;       // [capacity]
    const float *logp;          // [capacity]
    const float *dist;          // [capacity,A] or NULL
    const float *advantage;     // [capacity]
    const float *value_target;  // [capacity], NULL exactly when values is
    const double *adv_norm;     // device [2] {shift, scale} or NULL
    double clip_lo, clip_hi;    // 1 - clip, 1 + clip, formed once on the host
    double vf_clip, vf_coeff, ent_coeff, kl_coeff;
    float *grad_logits;         // [M,A]
    float *grad_values;         // [M] or NULL
    double *partial;            // [G,8]
};

// the slot of minibatch row i if the row is valid, else -1; a and lp_old: its action and behaviour log-probability
template <class KP>
PPG_DEVICE int64_t ppo_valid_slot(const KP &K, int64_t i, int &a, double &lp_old) {
    const int64_t k = K.index ? (int64_t)K.index[i] : i;
    if (k < 0 || k >= K.capacity) return -1;
    a = (int)K.action[k];
    if (a < 0 || a >= K.A) return -1;
    lp_old = (double)K.logp[k];
    if (!(lp_old > -INFINITY && lp_old < INFINITY)) return -1;   // NaN (no policy recorded), +-inf
    return k;
}

PPG_DEVICE double ppo_wave_sum(double x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = x + wv::shfl_xor_f64(x, m);
    return x;
}

// ---- launch 1: the valid rows of every chunk ----------------------------------------------------------------------------------------
template <class KP>
PPG_DEVICE void ppo_count_main(const KP &K) {
    const int g = PPG_BLOCK_INDEX();
    if (g >= K.G) return;
    const int ln = wv::lane();
    double n = 0.0;
    for (int j = 0; j < PPO_CHUNK / 64; ++j) {
        const int64_t i = (int64_t)g * PPO_CHUNK + 64 * j + ln;
        if (i >= K.M) break;
        int a;
        double lp_old;
        if (ppo_valid_slot(K, i, a, lp_old) >= 0) n = n + 1.0;
    }
    n = ppo_wave_sum(n);
    if (ln == 0) K.partial[(size_t)g * PPO_PARTIAL] = n;
}

// max of a row of A float32 logits, in float64 (a NaN is never the maximum; it reaches the sums)
PPG_DEVICE double ppo_row_max(const float *row, int A) {
    double m = -INFINITY;
    for (int c = 0; c < A; ++c) {
        const double l = (double)row[c];
        if (l > m) m = l;
    }
    return m;
}

// e_c = exp(l_c - m) of a row into the lane's LDS column (0 for a masked action: its term is skipped), and their sum
PPG_DEVICE double ppo_row_exp(const float *row, int A, double m, double *col) {
    double s = 0.0;
    for (int c = 0; c < A; ++c) {
        const double d = (double)row[c] - m;   // (exact: both are float32 values)
        double e = 0.0;
        if (d != -INFINITY) {
            e = exp(d);
            s = s + e;
        }
        col[64 * c] = e;
    }
    return s;
}

// ---- launch 2: the rows ---------------------------------------------------------------------------------------------------------------
template <class KP>
PPG_DEVICE void ppo_rows_main(const KP &K, unsigned char *lds) {
    const int g = PPG_BLOCK_INDEX();
    if (g >= K.G) return;
    const int ln = wv::lane(), A = K.A;
    double n = 0.0;
    for (int q = 0; q < K.G; ++q) n = n + K.partial[(size_t)q * PPO_PARTIAL];   // (whole numbers below 2^31: exact)
    const double w = n > 0.0 ? 1.0 / n : 0.0;
    const bool has_v = K.values != nullptr, has_kl = K.dist != nullptr;
    double shift = 0.0, scale = 1.0;
    if (K.adv_norm) { shift = K.adv_norm[0]; scale = K.adv_norm[1]; }
    double *en = (double *)lds + ln, *eo = en + PPO_MAX_ACTIONS * 64;   // this lane's columns: element c at [64 * c]
    double acc_surr = 0.0, acc_vfc = 0.0, acc_vf = 0.0, acc_h = 0.0, acc_kl = 0.0, acc_clip = 0.0, acc_akl = 0.0;
    for (int j = 0; j < PPO_CHUNK / 64; ++j) {
        const int64_t i = (int64_t)g * PPO_CHUNK + 64 * j + ln;
        if (i >= K.M) break;
        float *grow = K.grad_logits + (size_t)i * A;
        int a = 0;
        double lp_old = 0.0;
        const int64_t k = ppo_valid_slot(K, i, a, lp_old);
        if (k < 0) {
            for (int c = 0; c < A; ++c) grow[c] = 0.0f;
            if (K.grad_values) K.grad_values[i] = 0.0f;
            continue;
        }
        const float *row = K.logits + (size_t)i * A;
        const float *old = has_kl ? K.dist + (size_t)k * A : row;   // (not read without dist)
        const double m = ppo_row_max(row, A);
        const double s = ppo_row_exp(row, A, m, en);
        const double ls = log(s);
        double mo = 0.0, so = 1.0, lso = 0.0;
        if (has_kl) {
            mo = ppo_row_max(old, A);
            so = ppo_row_exp(old, A, mo, eo);
            lso = log(so);
        }
        // entropy and KL; p_c and q_c replace e_c in LDS for the gradient pass
        double hsum = 0.0, kl = 0.0, lp_a = 0.0;
        for (int c = 0; c < A; ++c) {
            const double d = (double)row[c] - m;
            const double lp = d - ls;
            const double p = en[64 * c] / s;
            en[64 * c] = p;
            if (c == a) lp_a = lp;
            if (d != -INFINITY) {
                const double t = p * lp;
                hsum = hsum + t;
            }
            if (has_kl) {
                const double dq = (double)old[c] - mo;
                const double lq = dq - lso;
                const double q = eo[64 * c] / so;
                eo[64 * c] = q;
                if (q != 0.0) {
                    const double diff = lq - lp;
                    const double t = q * diff;
                    kl = kl + t;
                }
            }
        }
        const double H = 0.0 - hsum;
        // the surrogate
        const double dl = lp_a - lp_old;
        const double r = exp(dl);
        double adv = (double)K.advantage[k];
        if (K.adv_norm) {
            const double centred = adv - shift;
            adv = centred * scale;
        }
        const double rc = r < K.clip_lo ? K.clip_lo : r > K.clip_hi ? K.clip_hi : r;
        const double s1 = adv * r, s2 = adv * rc;
        const bool clipped = s2 < s1;
        const double surr = clipped ? s2 : s1;
        const double c1 = clipped ? 0.0 : s1;
        // the value term
        if (has_v) {
            const double e = (double)K.values[i] - (double)K.value_target[k];
            const double vf = e * e;
            const bool over = vf > K.vf_clip;
            const double vfc = over ? K.vf_clip : vf;
            acc_vfc = acc_vfc + vfc;
            acc_vf = acc_vf + vf;
            if (K.grad_values) {
                const double e2 = e + e;
                const double ge = over ? 0.0 : e2;
                const double gv = K.vf_coeff * ge;
                K.grad_values[i] = (float)(w * gv);
            }
        }
        // the gradient row
        for (int c = 0; c < A; ++c) {
            const double d = (double)row[c] - m;
            if (d == -INFINITY) { grow[c] = 0.0f; continue; }   // a masked action
            const double lp = d - ls;
            const double p = en[64 * c];
            const double lh = lp + H;
            const double plh = p * lh;
            const double te = K.ent_coeff * plh;
            const double delta = (c == a ? 1.0 : 0.0) - p;
            const double ts = c1 * delta;
            double y = te - ts;
            if (has_kl) {
                const double pq = p - eo[64 * c];
                const double tk = K.kl_coeff * pq;
                y = y + tk;
            }
            grow[c] = (float)(w * y);
        }
        acc_surr = acc_surr + surr;
        acc_h = acc_h + H;
        if (has_kl) acc_kl = acc_kl + kl;
        acc_clip = acc_clip + (clipped ? 1.0 : 0.0);
        acc_akl = acc_akl + (lp_old - lp_a);
    }
    const double sums[PPO_PARTIAL - 1] = {acc_surr, acc_vfc, acc_vf, acc_h, acc_kl, acc_clip, acc_akl};
#pragma unroll
    for (int c = 0; c < PPO_PARTIAL - 1; ++c) {
        const double x = ppo_wave_sum(sums[c]);
        if (ln == 0) K.partial[(size_t)g * PPO_PARTIAL + 1 + (size_t)c] = x;
    }
}

}  // namespace ppg
