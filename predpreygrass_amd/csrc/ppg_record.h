// ppg_record.h -- ppg_record of include/ppg.h: the link of ppg_link.h plus the stores with which
// predpreygrass_amd.trajectory.AgentTrajectories keeps one env step, in ONE launch (as torch ops behind ppg_link: about nineteen).
//
// One wavefront per env, written against the wave primitives of wave.h (the CPU test build runs the same source).  The wavefront
//   1. requests the step index t (ppg_rows.h: RecordedStep);
//   2. links its env (link_env of ppg_link.h: the same code, snapshot and outputs as ppg_link_rows), after which next[] of both
//      species is still in LDS;
//   3. if 0 <= t < T writes for its rows r = 64q + lane
//        next_row[t-1][b][r] = next[r] from LDS (only if t > 0)      next_row[t][b][r] = -1
//        reward[t][b][r]     = the bits of row_reward[b][r] (all S rows: what a copy of the tensor does)
//        in_use[t][b][r]     = r < cap_pred ? r < n_pred_rows : r - cap_pred < n_prey_rows
//        terminated / truncated[t][b][r] = in_use && PPG_ROW_DIED / PPG_ROW_TRUNC of row_flags[b][r]
//      and nothing else; with t outside [0, T) the launch is exactly ppg_link's.
// Ordinary vector loads / stores and LDS accesses only: no atomics, no ballots.
#pragma once

#include <stdint.h>

#include "ppg_link.h"
#include "ppg_rows.h"

namespace ppg {

constexpr int RECORD_MAX_REGS = LINK_MAX_ROWS / 64;   // row registers per lane at the largest S

struct RecordParams : LinkParams, RecordedStep<0> {   // the device word holds t; T = the horizon: the buffers are [T,B,S]
    const uint64_t *row_reward; // [B,S] float64, moved as bits
    uint64_t *reward;           // [T,B,S]
    uint8_t *in_use, *terminated, *truncated;   // [T,B,S], 0 / 1
    int16_t *traj_next;         // [T,B,S]
};

template <class KP>
PPG_DEVICE void record_main(const KP &K, unsigned char *lds) {
    const int b = PPG_BLOCK_INDEX();
    if (b >= K.batch) return;
    const int ln = wv::lane();
    const int S = K.S;   // a multiple of 64, at most LINK_MAX_ROWS (the host refuses anything else): row registers q < S / 64 <= 6
    const size_t row0 = (size_t)b * S;
    // what the stores need and the link does not depend on is requested first: the loads return while the link runs
    const int64_t t = recorded_step(K);
    uint8_t f[RECORD_MAX_REGS];
    uint64_t rew[RECORD_MAX_REGS];
#pragma unroll
    for (int q = 0; q < RECORD_MAX_REGS; ++q) {
        const int r = 64 * q + ln;
        f[q] = r < S ? K.row_flags[row0 + r] : (uint8_t)0;
        rew[q] = r < S ? K.row_reward[row0 + r] : (uint64_t)0;
    }
    const LinkRows n = link_env(K, lds, b, ln);
    if (!step_in_horizon(K, t)) return;   // a replay past the horizon: the link above, and nothing else
    wv::sync();
    const int16_t *nxt = (const int16_t *)(lds + (size_t)LINK_MAX_ROWS * 4);
    const size_t step = (size_t)K.batch * S, at = (size_t)t * step + row0;
#pragma unroll
    for (int q = 0; q < RECORD_MAX_REGS; ++q) {
        const int r = 64 * q + ln;
        if (r >= S) continue;
        const bool used = r < K.cap_pred ? r < n.n_pred : r - K.cap_pred < n.n_prey;
        const size_t i = at + (size_t)r;
        if (t > 0) K.traj_next[i - step] = nxt[r];
        K.traj_next[i] = (int16_t)-1;
        K.reward[i] = rew[q];
        K.in_use[i] = (uint8_t)used;
        K.terminated[i] = (uint8_t)(used && (f[q] & PPG_ROW_DIED) != 0);
        K.truncated[i] = (uint8_t)(used && (f[q] & PPG_ROW_TRUNC) != 0);
    }
}

}  // namespace ppg
