// ppg_link.h -- ppg_link of include/ppg.h: which row of THIS call's output is the agent that stood in row r of the output the previous
// ppg_link call saw.  Row order is the API and changes with every call -- dead rows are dropped, last call's
// newborns are merged into sorted position, new newborns are appended -- so a learner that builds per-agent trajectories from the
// tensor API needs the join of two row_id tables.  This kernel does that join on the device, next to the step.
//
// One launch, one wavefront per env, written against the wave primitives of wave.h (the CPU test build runs the same source).
// Library-owned per-handle state (LinkParams::snap_*) holds what the previous link call saw: the ids [B,S], the episode word [B] and
// the row counts [B,2].  Per env and species:
//   1. the snapshot's ids go to LDS, next[] in LDS is set to -1; lane l holds the current row_id of rows 64q + l in registers;
//   2. for every snapshot row j (wave-uniform loop) all lanes read ids[j] (one LDS address: a broadcast) and compare it with their
//      registers; the lane that holds the id sets prev of its row to j and writes its own row into next[j] in LDS;
//   3. prev goes out from the registers, next from LDS, then the snapshot is overwritten with the current ids, episode and counts
//      (every lane writes exactly the snapshot words it read itself).
// No ballots, no atomics: ordinary LDS and global vector loads / stores only.
//
// Why a match is unique -- (species, row_id) never recurs within an episode:
//   base family        row_id = k of "predator_k" / "prey_k".  reset() hands out 0..n_initial-1 and every birth takes next_id[type],
//                      which only grows (Env::reproduce: `next_id[type] += 1`, BASE:397/426); an exhausted pool stops births
//                      (`next_id[type] >= npos`: no child), it never wraps.  The id of a dead agent is not handed out again.
//   second generation  row_id = creation_number << 17 | (type - 1) << 16 | k.  k comes from four growing pools, and the creation
//                      number -- agents created so far in the episode, all pools together (Env::spawn2: `seq`) -- is strictly
//                      increasing, so two agents of one episode differ in the high bits even if a (type, k) pair were to repeat.
//   walls, drive       the same id schemes (walls = second generation, drive = base family).
// Ids DO restart with every episode, which is why an env whose PPG_ENV_EPISODE differs from the snapshot's gets -1 everywhere, and
// why the host invalidates the snapshot when ppg_reset / ppg_reset_from_state / ppg_import_state rewrite state behind the episode
// word.  So at most one lane matches a snapshot row and the LDS write in step 2 has one writer; no id was found that can recur, and
// the kernel has no tie-break.  (A caller that writes row_id tensors by hand owns their uniqueness.)
//
// A row flagged PPG_ROW_NEWBORN is not matched at all (prev -1): it was created by the call whose output is being linked.  A row
// flagged PPG_ROW_DIED is still in use and links like any other: it is where the agent stood when it received its terminal reward.
#pragma once

#include <stdint.h>

#include "../../include/ppg.h"

namespace ppg {

constexpr int LINK_MAX_ROWS = 128 + 256;                      // pred_capacity + prey_capacity at their largest
constexpr int LINK_LDS_BYTES = LINK_MAX_ROWS * (4 + 2);       // snapshot ids int32[S] | next int16[S]

struct LinkParams {
    int32_t batch, S, cap_pred, cap_prey;
    int32_t valid;              // 0: the snapshot holds nothing this call may link to (first call, reset, ...): -1 everywhere
    const int32_t *row_id;      // [B,S]
    const uint8_t *row_flags;   // [B,S]
    const int32_t *env_state;   // [B,PPG_ENV_WORDS]
    int32_t *snap_id;           // [B,S]  library-owned: row_id as the previous link call saw it
    int32_t *snap_episode;      // [B]    PPG_ENV_EPISODE of that call
    int32_t *snap_rows;         // [B,2]  rows in use of that call (predators, prey); negative = this env's snapshot is invalid
    int16_t *prev_row;          // [B,S]  caller-owned, may be NULL
    int16_t *next_row;          // [B,S]  caller-owned, may be NULL
};

PPG_DEVICE int link_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One species of one env: rows [base, base + 64 * NR) of the [B,S] tables.  n_cur / n_old: rows in use now / in the snapshot
// (n_old = 0 when nothing may link).  ids / nxt: this species' part of the LDS arrays.
template <int NR, class KP>
PPG_DEVICE void link_species(const KP &K, size_t row0, int base, int n_cur, int n_old, int32_t *ids, int16_t *nxt, int ln) {
    int32_t id[NR];
    int16_t prev[NR];
    bool match[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int r = 64 * q + ln;
        ids[r] = K.snap_id[row0 + base + r];
        nxt[r] = (int16_t)-1;
        id[q] = K.row_id[row0 + base + r];
        match[q] = r < n_cur && !(K.row_flags[row0 + base + r] & PPG_ROW_NEWBORN);
        prev[q] = (int16_t)-1;
    }
    wv::sync();
    for (int j = 0; j < n_old; ++j) {
        const int32_t old = ids[j];   // every lane reads the same word
#pragma unroll
        for (int q = 0; q < NR; ++q)
            if (match[q] && id[q] == old) {
                prev[q] = (int16_t)(base + j);
                nxt[j] = (int16_t)(base + 64 * q + ln);
            }
    }
    wv::sync();
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int r = 64 * q + ln;
        if (K.prev_row) K.prev_row[row0 + base + r] = prev[q];
        if (K.next_row) K.next_row[row0 + base + r] = nxt[r];
        K.snap_id[row0 + base + r] = id[q];
    }
}

template <class KP>
PPG_DEVICE void link_species_n(const KP &K, int nr, size_t row0, int base, int n_cur, int n_old, int32_t *ids, int16_t *nxt, int ln) {
    // nr = capacity / 64: 1, 2 or 4 are the capacities ppg_create accepts; anything else (a future 192) links nothing rather than
    // run an instantiation that would index past the species' rows
    if (nr == 1) link_species<1>(K, row0, base, n_cur, n_old, ids, nxt, ln);
    else if (nr == 2) link_species<2>(K, row0, base, n_cur, n_old, ids, nxt, ln);
    else if (nr == 4) link_species<4>(K, row0, base, n_cur, n_old, ids, nxt, ln);
}

// rows in use of env b in the call that was linked: what link_env read from env_state, for kernels that go on from it (ppg_record.h)
struct LinkRows { int n_pred, n_prey; };

// The link of ONE env by its wavefront (ppg_link_rows, and the first half of ppg_record_rows).  On return next[] of both species is
// still in LDS at lds + LINK_MAX_ROWS * 4, int16 [S] in absolute rows, ordered behind a wv::sync().
template <class KP>
PPG_DEVICE LinkRows link_env(const KP &K, unsigned char *lds, int b, int ln) {
    const int32_t *es = K.env_state + (size_t)b * PPG_ENV_WORDS;
    const int episode = es[PPG_ENV_EPISODE];
    const int np = link_clamp(es[PPG_ENV_N_PRED_ROWS], K.cap_pred), nq = link_clamp(es[PPG_ENV_N_PREY_ROWS], K.cap_prey);
    const int op = K.snap_rows[2 * b], oq = K.snap_rows[2 * b + 1];
    // (the three snapshot words are read by every lane before lane 0 overwrites them below: drain_loads)
    const bool linked = K.valid != 0 && op >= 0 && oq >= 0 && K.snap_episode[b] == episode;
    const int n_op = linked ? link_clamp(op, K.cap_pred) : 0, n_oq = linked ? link_clamp(oq, K.cap_prey) : 0;
    int32_t *ids = (int32_t *)lds;
    int16_t *nxt = (int16_t *)(lds + (size_t)LINK_MAX_ROWS * 4);
    const size_t row0 = (size_t)b * K.S;
    link_species_n(K, K.cap_pred >> 6, row0, 0, np, n_op, ids, nxt, ln);
    link_species_n(K, K.cap_prey >> 6, row0, K.cap_pred, nq, n_oq, ids + K.cap_pred, nxt + K.cap_pred, ln);
    wv::drain_loads();
    if (ln == 0) {
        K.snap_episode[b] = episode;
        K.snap_rows[2 * b] = np;
        K.snap_rows[2 * b + 1] = nq;
    }
    return LinkRows{np, nq};
}

template <class KP>
PPG_DEVICE void link_main(const KP &K, unsigned char *lds) {
    const int b = PPG_BLOCK_INDEX();
    if (b >= K.batch) return;
    link_env(K, lds, b, wv::lane());
}

}  // namespace ppg
