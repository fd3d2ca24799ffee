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

template <int NR, bool F32, bool PREFETCH, class KP>
PPG_DEVICE void backward_env(const KP &K, unsigned char *lds, int b, int ln) {
    const int S = 64 * NR, T = K.T;
    const bool want_g = K.returns != nullptr, want_a = K.advantages != nullptr;
    const double gamma = K.gamma, gl = K.gl;
    double *lg = (double *)lds, *la = lg + BACKWARD_MAX_ROWS, *lv = la + BACKWARD_MAX_ROWS;
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
            const int nx = (int)cur.nxt[q];
            const bool used = cur.used[q] != 0;
            const bool has = t + 1 < T && used && cur.stop[q] == 0 && nx >= 0 && nx < S;
            const int j = has ? nx : 0;   // the only index a tensor's value ever becomes: checked against [0, S) above
            double g_succ = 0.0, a_succ = 0.0, v_succ = 0.0;
            if (t + 1 < T) {              // (wave-uniform; the arrays hold nothing yet at the last step)
                if (want_g) { const double x = lg[j]; g_succ = has ? x : 0.0; }
                if (want_a) { const double x = la[j], y = lv[j]; a_succ = has ? x : 0.0; v_succ = has ? y : 0.0; }
            }
            const double rew = cur.rew[q];
            const double gm = g_succ * gamma;
            const double gq = rew + gm;
            g[q] = used ? gq : 0.0;
            const double vm = v_succ * gamma;
            const double boot = rew + vm;
            const double delta = boot - cur.v[q];
            const double am = a_succ * gl;
            const double aq = delta + am;
            a[q] = used ? aq : 0.0;
            const size_t i = at + (size_t)(64 * q + ln);
            if (want_g) K.returns[i] = g[q];
            if (want_a) K.advantages[i] = a[q];
        }
        if (t == 0) break;
        wv::sync();   // every lane has read step t + 1's values
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const int r = 64 * q + ln;
            if (want_g) lg[r] = g[q];
            if (want_a) { la[r] = a[q]; lv[r] = cur.v[q]; }
        }
        wv::sync();   // step t's values are there for every lane
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

}  // namespace ppg
