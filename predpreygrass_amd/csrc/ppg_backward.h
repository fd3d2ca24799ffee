// ppg_backward.h -- ppg_backward of include/ppg.h: discounted returns and generalised advantages over a recorded horizon, the
// backward pass of predpreygrass_amd.trajectory.AgentTrajectories, in ONE launch.
//
// One wavefront per env, written against the wave primitives of wave.h (the CPU test build runs the same source).  Rows interact only
// within their env, through next_row, so the whole state of the recursion is G, A and V of step t + 1 of ONE env: three arrays of S
// doubles in LDS.  Lane l owns rows 64q + l (q < S / 64 = 2 .. 6).  For t = T-1 .. 0 every lane
//   1. has its rows' inputs of step t in registers (reward, next_row, the three flags, V);
//   2. gathers G / A / V of step t + 1 of its successors from LDS -- the index is next_row only where it was checked against [0, S),
//      else 0, and the value read is SELECTED away, never multiplied away (a NaN in an unused slot reaches no output);
//   3. computes G[t], A[t] -- every line one IEEE float64 operation in the order of trajectory.py, this unit is built with
//      -ffp-contract=off -- and stores them to global memory (every element of the outputs is written, zeros included);
//   4. after a wv::sync() overwrites the LDS arrays with step t's values, and after another one goes on with step t - 1.
// With PREFETCH the inputs of step t - 1 are requested between 1 and 2: they do not depend on the recursion, so their latency
// hides behind the gather and the arithmetic of step t (measured: profiles/EXPERIMENTS.md, `ppg_backward`).
// Ordinary vector loads / stores and LDS accesses only: no atomics, no ballots.
#pragma once

#include <stdint.h>

#include "../../include/ppg.h"

namespace ppg {

constexpr int BACKWARD_MAX_ROWS = 128 + 256;                  // pred_capacity + prey_capacity at their largest
constexpr int BACKWARD_LDS_BYTES = 3 * BACKWARD_MAX_ROWS * 8; // G | A | V of step t + 1, float64 [S] each

struct BackwardParams {
    int32_t batch, S, T;
    int32_t values_f32;         // values is float32 (widened exactly) instead of float64
    int32_t prefetch;           // request step t - 1's inputs before step t's gather
    const double *reward;       // [T,B,S]
    const int16_t *next_row;    // [T,B,S]
    const uint8_t *in_use, *terminated, *truncated;   // [T,B,S], 0 / 1
    const void *values;         // [T,B,S] float64 / float32, NULL without advantages
    double gamma, gl;           // gl = gamma * lam, formed once on the host
    double *returns;            // [T,B,S], may be NULL
    double *advantages;         // [T,B,S], may be NULL (not both)
};

// a lane's rows of one step
template <int NR>
struct BackwardIn {
    double rew[NR], v[NR];
    int16_t nxt[NR];
    uint8_t used[NR], stop[NR];   // in_use; terminated | truncated
};

template <int NR, bool F32, class KP>
PPG_DEVICE void backward_load(const KP &K, size_t at, int ln, bool want_a, BackwardIn<NR> &in) {
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const size_t i = at + (size_t)(64 * q + ln);
        in.rew[q] = K.reward[i];
        in.nxt[q] = K.next_row[i];
        in.used[q] = K.in_use[i];
        in.stop[q] = (uint8_t)(K.terminated[i] | K.truncated[i]);
        in.v[q] = !want_a ? 0.0 : F32 ? (double)((const float *)K.values)[i] : ((const double *)K.values)[i];
    }
}

// ---- the recursion both kernels run (ppg_backward and ppg_backward_samples below) -------------------------------------------------
// what does not change from step to step: the outputs asked for, the discounts, and G | A | V of step t + 1 in LDS
struct BackwardRec {
    bool want_g, want_a;
    double gamma, gl;
    double *lg, *la, *lv;
};

template <class KP>
PPG_DEVICE BackwardRec backward_rec(const KP &K, unsigned char *lds, bool want_g, bool want_a) {
    BackwardRec R;
    R.want_g = want_g; R.want_a = want_a; R.gamma = K.gamma; R.gl = K.gl;
    R.lg = (double *)lds; R.la = R.lg + BACKWARD_MAX_ROWS; R.lv = R.la + BACKWARD_MAX_ROWS;
    return R;
}

// One row of step t: G[t] and A[t] from the row's inputs and its successor's values of step t + 1.  more: t + 1 < T (wave-uniform;
// the arrays hold nothing yet at the last step).  Every line one IEEE float64 operation, in the order of trajectory.py.
template <int S>
PPG_DEVICE void backward_row(const BackwardRec &R, bool more, bool used, bool stop, int16_t next, double rew, double v, double &g, double &a) {
    const int nx = (int)next;
    const bool has = more && used && !stop && nx >= 0 && nx < S;
    const int j = has ? nx : 0;   // the only LDS index a tensor's value ever becomes: checked against [0, S) above
    double g_succ = 0.0, a_succ = 0.0, v_succ = 0.0;
    if (more) {
        if (R.want_g) { const double x = R.lg[j]; g_succ = has ? x : 0.0; }
        if (R.want_a) { const double x = R.la[j], y = R.lv[j]; a_succ = has ? x : 0.0; v_succ = has ? y : 0.0; }
    }
    const double gm = g_succ * R.gamma;
    const double gq = rew + gm;
    g = used ? gq : 0.0;
    const double vm = v_succ * R.gamma;
    const double boot = rew + vm;
    const double delta = boot - v;
    const double am = a_succ * R.gl;
    const double aq = delta + am;
    a = used ? aq : 0.0;
}

// step t's values replace step t + 1's in LDS, between two ordering points
template <int NR>
PPG_DEVICE void backward_publish(const BackwardRec &R, int ln, const double (&g)[NR], const double (&a)[NR], const double (&v)[NR]) {
    wv::sync();   // every lane has read step t + 1's values
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int r = 64 * q + ln;
        if (R.want_g) R.lg[r] = g[q];
        if (R.want_a) { R.la[r] = a[q]; R.lv[r] = v[q]; }
    }
    wv::sync();   // step t's values are there for every lane
}

template <int NR, bool F32, bool PREFETCH, class KP>
PPG_DEVICE void backward_env(const KP &K, unsigned char *lds, int b, int ln) {
    const int S = 64 * NR, T = K.T;
    const bool want_g = K.returns != nullptr, want_a = K.advantages != nullptr;
    const BackwardRec R = backward_rec(K, lds, want_g, want_a);
    const size_t step = (size_t)K.batch * (size_t)S, env = (size_t)b * (size_t)S;
    BackwardIn<NR> cur, ahead;
    if (PREFETCH) backward_load<NR, F32>(K, (size_t)(T - 1) * step + env, ln, want_a, cur);
    for (int t = T - 1; t >= 0; --t) {
        const size_t at = (size_t)t * step + env;
        if (!PREFETCH) backward_load<NR, F32>(K, at, ln, want_a, cur);
        else if (t > 0) backward_load<NR, F32>(K, at - step, ln, want_a, ahead);
        double g[NR], a[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            backward_row<S>(R, t + 1 < T, cur.used[q] != 0, cur.stop[q] != 0, cur.nxt[q], cur.rew[q], cur.v[q], g[q], a[q]);
            const size_t i = at + (size_t)(64 * q + ln);
            if (want_g) K.returns[i] = g[q];
            if (want_a) K.advantages[i] = a[q];
        }
        if (t == 0) break;
        backward_publish(R, ln, g, a, cur.v);
        if (PREFETCH) cur = ahead;
    }
}

template <int NR, class KP>
PPG_DEVICE void backward_rows(const KP &K, unsigned char *lds, int b, int ln) {
    if (K.values_f32) {
        if (K.prefetch) backward_env<NR, true, true>(K, lds, b, ln);
        else backward_env<NR, true, false>(K, lds, b, ln);
    } else {
        if (K.prefetch) backward_env<NR, false, true>(K, lds, b, ln);
        else backward_env<NR, false, false>(K, lds, b, ln);
    }
}

template <class KP>
PPG_DEVICE void backward_main(const KP &K, unsigned char *lds) {
    const int b = PPG_BLOCK_INDEX();
    if (b >= K.batch) return;
    const int ln = wv::lane();
    // S / 64 = 2 .. 6 are the capacities ppg_create accepts (the host refuses anything else); another value computes nothing rather
    // than run an instantiation whose rows are not the env's
    switch (K.S) {
    case 128: backward_rows<2>(K, lds, b, ln); break;
    case 192: backward_rows<3>(K, lds, b, ln); break;
    case 256: backward_rows<4>(K, lds, b, ln); break;
    case 320: backward_rows<5>(K, lds, b, ln); break;
    case 384: backward_rows<6>(K, lds, b, ln); break;
    default: break;
    }
}

// ---- ppg_backward_samples of include/ppg.h: the same recursion, read and written in SAMPLE order ---------------------------------
// V of a row is gathered from the per-sample values through the slot table of ppg_record_obs (st->slot), and G / A of a stored row are
// rounded once to float32 and stored at its slot: no [T,B,S] tensor of values, returns or advantages exists.  The recursion is
// backward_row / backward_publish above (rows the store dropped take part with V = 0); what differs:
//   - a DEPENDENT load chain: slot[t][b][r] (4 bytes, dense) and then values[s][k] (4 or 8 bytes, scattered).  k is compared with
//     [0, capacity[s]) before it becomes an address, and a row that is not stored keeps k = -1 from then on.  With PREFETCH both are
//     requested for step t - 1 with the other inputs, in front of step t's LDS gather -- measured 3 % SLOWER than loading at the top
//     of the step here (profiles/EXPERIMENTS.md, `ppg_backward_samples`), so the host asks for it only when PPG_BACKWARD_PREFETCH
//     says so;
//   - two scattered 4-byte stores per STORED row instead of two dense 8-byte stores per element;
//   - STATS: three float64 accumulators per species and lane {count, sum A, sum A * A} over the stored rows in the order
//     include/ppg.h states, reduced by an xor butterfly at the end; lane 0 stores the six doubles of its env.
// The next_row / in_use / stop words of a row are packed into ONE register (BackwardSampleIn::meta) and `stored` into k's sign, and
// the species of a row register is a template argument (NP): the six-row instantiation with STATS has to stay free of scratch and
// within 128 VGPRs, four one-wave workgroups per SIMD (profiles/EXPERIMENTS.md, `ppg_backward_samples`).
// Ordinary vector loads / stores, LDS accesses and wave shuffles only: no atomics.
struct BackwardSamplesParams {
    int32_t batch, S, T;
    int32_t cap_pred;           // rows [0, cap_pred) are predators (species 0): a multiple of 64
    int32_t values_f32;         // values[] are float32 (widened exactly) instead of float64
    int32_t prefetch;           // request step t - 1's inputs before step t's gather
    int32_t capacity[2];        // slots of each species' store (checked against INT32_MAX on the host)
    const double *reward;       // [T,B,S]
    const int16_t *next_row;    // [T,B,S]
    const uint8_t *in_use, *terminated, *truncated;   // [T,B,S], 0 / 1
    const int32_t *slot;        // [horizon >= T,B,S]
    const void *values[2];      // [capacity[s]] float64 / float32, NULL: V = 0
    double gamma, gl;           // gl = gamma * lam, formed once on the host
    float *advantage[2];        // [capacity[s]], both NULL or both set
    float *returns[2];          // [capacity[s]], both NULL or both set (not both pairs NULL)
    double *stats;              // [B,2,3] or NULL
};

constexpr uint32_t BACKWARD_META_USED = 0x10000u, BACKWARD_META_STOP = 0x20000u;   // above next_row's 16 bits

// a lane's rows of one step
template <int NR>
struct BackwardSampleIn {
    double rew[NR], v[NR];
    uint32_t meta[NR];   // next_row (low 16 bits) | BACKWARD_META_USED | BACKWARD_META_STOP
    int32_t k[NR];       // the row's slot if it is stored (in use, 0 <= slot < capacity[s]), else -1
};

// NP: the row registers of the predators (pred_capacity / 64), so the species of register q is known when the code is compiled
template <int NR, int NP, class KP>
PPG_DEVICE void backward_samples_load(const KP &K, size_t at, int ln, bool want_a, BackwardSampleIn<NR> &in) {
    int32_t word[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) word[q] = K.slot[at + (size_t)(64 * q + ln)];   // (first: the gather below waits for these)
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const size_t i = at + (size_t)(64 * q + ln);
        in.rew[q] = K.reward[i];
        const uint32_t used = K.in_use[i] != 0, stop = (K.terminated[i] | K.truncated[i]) != 0;
        in.meta[q] = (uint32_t)(uint16_t)K.next_row[i] | (used ? BACKWARD_META_USED : 0u) | (stop ? BACKWARD_META_STOP : 0u);
    }
    const bool f32 = K.values_f32 != 0;   // (wave-uniform)
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int sp = q < NP ? 0 : 1;   // (a constant once the loop is unrolled)
        const int32_t k = word[q];
        const void *values = K.values[sp];
        const bool stored = (in.meta[q] & BACKWARD_META_USED) != 0 && k >= 0 && k < K.capacity[sp];
        in.k[q] = stored ? k : -1;
        double v = 0.0;
        if (want_a && stored && values != nullptr) {   // (a selection: an unreferenced slot's word is never loaded)
            if (f32) v = (double)((const float *)values)[k];
            else v = ((const double *)values)[k];
        }
        in.v[q] = v;
    }
}

template <int NR, int NP, bool PREFETCH, bool STATS, class KP>
PPG_DEVICE void backward_samples_env(const KP &K, unsigned char *lds, int b, int ln) {
    const int S = 64 * NR, T = K.T;
    const bool want_g = K.returns[0] != nullptr, want_a = K.advantage[0] != nullptr;
    const BackwardRec R = backward_rec(K, lds, want_g, want_a);
    const size_t step = (size_t)K.batch * (size_t)S, env = (size_t)b * (size_t)S;
    double cnt[2] = {0.0, 0.0}, sum[2] = {0.0, 0.0}, sq[2] = {0.0, 0.0};   // (indexed by constants only: registers)
    BackwardSampleIn<NR> cur, ahead;
    if (PREFETCH) backward_samples_load<NR, NP>(K, (size_t)(T - 1) * step + env, ln, want_a, cur);
    for (int t = T - 1; t >= 0; --t) {
        const size_t at = (size_t)t * step + env;
        if (!PREFETCH) backward_samples_load<NR, NP>(K, at, ln, want_a, cur);
        else if (t > 0) backward_samples_load<NR, NP>(K, at - step, ln, want_a, ahead);
        double g[NR], a[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const int sp = q < NP ? 0 : 1;   // (a constant once the loop is unrolled)
            const uint32_t meta = cur.meta[q];
            backward_row<S>(R, t + 1 < T, (meta & BACKWARD_META_USED) != 0, (meta & BACKWARD_META_STOP) != 0, (int16_t)(uint16_t)meta,
                            cur.rew[q], cur.v[q], g[q], a[q]);
            const int32_t k = cur.k[q];
            if (k >= 0) {                 // stored: in use and 0 <= k < capacity[s] (backward_samples_load)
                if (want_g) K.returns[sp][k] = (float)g[q];
                if (want_a) K.advantage[sp][k] = (float)a[q];
                if (STATS) {
                    cnt[sp] = cnt[sp] + 1.0;
                    sum[sp] = sum[sp] + a[q];
                    const double p = a[q] * a[q];
                    sq[sp] = sq[sp] + p;
                }
            }
        }
        if (t == 0) break;
        backward_publish(R, ln, g, a, cur.v);
        if (PREFETCH) cur = ahead;
    }
    if (STATS) {
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
            double x[3] = {cnt[sp], sum[sp], sq[sp]};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) x[c] = x[c] + wv::shfl_xor_f64(x[c], m);
                if (ln == 0) K.stats[((size_t)b * 2 + (size_t)sp) * 3 + (size_t)c] = x[c];
            }
        }
    }
}

template <int NR, int NP, class KP>
PPG_DEVICE void backward_samples_rows(const KP &K, unsigned char *lds, int b, int ln) {
    if (K.stats != nullptr) {
        if (K.prefetch) backward_samples_env<NR, NP, true, true>(K, lds, b, ln);
        else backward_samples_env<NR, NP, false, true>(K, lds, b, ln);
    } else {
        if (K.prefetch) backward_samples_env<NR, NP, true, false>(K, lds, b, ln);
        else backward_samples_env<NR, NP, false, false>(K, lds, b, ln);
    }
}

template <class KP>
PPG_DEVICE void backward_samples_main(const KP &K, unsigned char *lds) {
    const int b = PPG_BLOCK_INDEX();
    if (b >= K.batch) return;
    const int ln = wv::lane();
    // the five (pred_capacity, prey_capacity) ppg_create accepts, as 4 * (S / 64) + pred_capacity / 64; like backward_main another
    // geometry computes nothing rather than run an instantiation whose rows are not the env's
    switch (K.S / 64 * 4 + K.cap_pred / 64) {
    case 2 * 4 + 1: backward_samples_rows<2, 1>(K, lds, b, ln); break;   //  64 +  64
    case 3 * 4 + 1: backward_samples_rows<3, 1>(K, lds, b, ln); break;   //  64 + 128
    case 4 * 4 + 2: backward_samples_rows<4, 2>(K, lds, b, ln); break;   // 128 + 128
    case 5 * 4 + 1: backward_samples_rows<5, 1>(K, lds, b, ln); break;   //  64 + 256
    case 6 * 4 + 2: backward_samples_rows<6, 2>(K, lds, b, ln); break;   // 128 + 256
    default: break;
    }
}

}  // namespace ppg
