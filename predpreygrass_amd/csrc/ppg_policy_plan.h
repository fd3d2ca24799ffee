// ppg_policy_plan.h -- the arithmetic of the policy kernels' PLAN, HIP-free (like ppg_policy_pack.h: plain C++, so that a CPU test
// and a stand-alone sanitizer program run the very functions the kernels call).
//
// The plan (csrc/ppg_policy.h: PolParams::plan / tile_env) is what stands between "so many samples" and the forward kernels:
//   plan[0]  samples of the launch
//   TILE MODE (the FC-chain kernels)      plan[1] = tiles of 128 samples in whole rounds of the resident workgroups, plan[2] = samples
//                                         per tile of the one last round (32 / 64 / 96 / 128)
//   RANGE MODE (the direct-head kernels)  plan[1] = samples of a workgroup's contiguous share, plan[2] = tiles per workgroup
//   plan[PPG_PLAN_HDR + e]  exclusive prefix sum of the row counts of env e;   tile_env[tile] = the env of the tile's first sample
// Part 1 are the decisions both plan kernels share -- plan_body (ppg_policy.h: the counts come from env_state, the prefix sums from a
// scan, tile_env from a bisection) and ppg_policy_plan_rows (below: everything in closed form from ONE number).
// Part 2 is the plan of a DENSE ROW TENSOR (ppg_policy_evaluate): rows [0, count) of a [capacity][C][R][R] tensor are read as
// pseudo-envs of PPG_POLICY_ROWS_CHUNK rows each, of which the first min(count - e CH, CH) are in use.  With one handle, slot0 = 0 and
// S = cap = CH the forward kernels' addresses -- obs + (e * cap + row) * row_bytes, actions + e * S + slot0 + row -- are linear in the
// sample number, so sample n IS row n, whatever CH is.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/ppg.h"

#if defined(__HIPCC__)
#define PPG_PLAN_HD __host__ __device__
#else
#define PPG_PLAN_HD
#endif

constexpr uint32_t PPG_PLAN_TILE = 128;   // samples per workgroup tile (ppgpol::TILE)
constexpr int PPG_PLAN_HDR = 3;           // words in front of the prefix sums (ppgpol::PLAN_HDR)

// ---- part 1: what plan_body and ppg_policy_plan_rows decide alike ----

// TILE MODE.  As many whole ROUNDS of 128-sample tiles as the resident workgroups (slots) can be given, then ONE last round in which the
// remaining samples are spread over the slots in tiles of 32 / 64 / 96 / 128 (ppg_policy.h: plan_body says why).
struct ppg_plan_tiles {
    uint32_t n_full, ts;
};
PPG_PLAN_HD inline ppg_plan_tiles ppg_plan_tiles_of(uint32_t all, uint32_t slots) {
    const uint32_t per_round = PPG_PLAN_TILE * slots;
    const uint32_t n_full = (all / per_round) * slots;
    const uint32_t rest = all - n_full * PPG_PLAN_TILE;
    uint32_t ts = 32u * ((rest + 32u * slots - 1u) / (32u * slots));   // 32 * ceil(rest / (32 * slots))
    if (ts < 32u) ts = 32u;
    return {n_full, ts};
}
PPG_PLAN_HD inline uint32_t ppg_plan_tile_count(uint32_t all, uint32_t n_full, uint32_t ts) {
    const uint32_t tail = all - n_full * PPG_PLAN_TILE;
    return n_full + (tail + ts - 1u) / ts;
}
PPG_PLAN_HD inline uint32_t ppg_plan_tile_first(uint32_t tile, uint32_t n_full, uint32_t ts) {
    return tile < n_full ? tile * PPG_PLAN_TILE : n_full * PPG_PLAN_TILE + (tile - n_full) * ts;
}

// RANGE MODE.  Workgroup w owns samples [w S, (w + 1) S), S = the per-workgroup share rounded up to whole sub-groups of st samples, as
// tpw tiles of tsz samples; slots * tpw tile slots exist, some of them empty.
struct ppg_plan_range {
    uint32_t share, tpw;
};
PPG_PLAN_HD inline ppg_plan_range ppg_plan_range_of(uint32_t all, uint32_t slots, uint32_t st, uint32_t tsz) {
    const uint32_t S = st * ((all + slots * st - 1u) / (slots * st));
    const uint32_t tpw = S ? (S + tsz - 1u) / tsz : 1u;
    return {S, tpw};
}
// first sample of a tile slot, all > 0.  An empty slot counts as standing behind every sample of the tiles in front of it: the list of
// first envs stays monotone.
PPG_PLAN_HD inline uint32_t ppg_plan_range_slot(uint32_t tile, uint32_t share, uint32_t tpw, uint32_t tsz) {
    return (tile / tpw) * share + (tile % tpw) * tsz;
}
PPG_PLAN_HD inline uint32_t ppg_plan_range_clamp(uint32_t n, uint32_t all) { return n > all - 1u ? all - 1u : n; }
PPG_PLAN_HD inline uint32_t ppg_plan_range_first(uint32_t tile, uint32_t share, uint32_t tpw, uint32_t tsz, uint32_t all) {
    return ppg_plan_range_clamp(ppg_plan_range_slot(tile, share, tpw, tsz), all);
}

// ---- part 2: the plan of a dense row tensor ----

constexpr uint32_t PPG_ROWS_CH = PPG_POLICY_ROWS_CHUNK;
constexpr int64_t PPG_ROWS_MAX = (int64_t)1 << 30;   // rows a plan can describe: sample numbers, and the kernels' `int` copies of them, stay in 31 bits

PPG_PLAN_HD inline uint32_t ppg_rows_envs(int64_t capacity) { return (uint32_t)((capacity + PPG_ROWS_CH - 1) / PPG_ROWS_CH); }

// rows to evaluate: the count clamped into [0, capacity]
PPG_PLAN_HD inline uint32_t ppg_rows_clamp(int64_t count, int64_t capacity) {
    return (uint32_t)(count < 0 ? 0 : count > capacity ? capacity : count);
}

// exclusive prefix sum of pseudo-env e: the envs in front of it are full, or the rows have run out
PPG_PLAN_HD inline uint32_t ppg_rows_prefix(uint32_t e, uint32_t all) {
    const uint32_t n = e * PPG_ROWS_CH;
    return n < all ? n : all;
}

// Everything a plan's words follow from.  range_tile > 0: range mode with sub-groups of range_st samples; 0: tile mode.
struct ppg_rows_shape {
    uint32_t all, n_envs;
    uint32_t range;        // 1: range mode
    uint32_t w1, w2;       // plan[1], plan[2]
    uint32_t tsz;          // range mode: samples per tile
    uint32_t tile_words;   // words of tile_env the plan writes
    uint32_t items;        // max(n_envs, tile_words): the loop that writes the plan runs over this many items
};
PPG_PLAN_HD inline ppg_rows_shape ppg_rows_shape_of(int64_t capacity, int64_t count, uint32_t slots, uint32_t range_tile, uint32_t range_st) {
    ppg_rows_shape s;
    s.all = ppg_rows_clamp(count, capacity);
    s.n_envs = ppg_rows_envs(capacity);
    s.range = range_tile > 0u ? 1u : 0u;
    s.tsz = range_tile;
    if (s.range) {
        const ppg_plan_range r = ppg_plan_range_of(s.all, slots, range_st, range_tile);
        s.w1 = r.share; s.w2 = r.tpw;
        s.tile_words = slots * r.tpw;
    } else {
        const ppg_plan_tiles t = ppg_plan_tiles_of(s.all, slots);
        s.w1 = t.n_full; s.w2 = t.ts;
        s.tile_words = ppg_plan_tile_count(s.all, t.n_full, t.ts);
    }
    s.items = s.n_envs > s.tile_words ? s.n_envs : s.tile_words;
    return s;
}

// Item i of the plan: the header (i = 0), the prefix sum of pseudo-env i, the first env of tile slot i.  No item reads what another wrote.
// The last env whose prefix sum is <= n, n < all, is n / CH: the envs up to it start at e CH <= n, the ones behind it at more than n or
// at `all`.
PPG_PLAN_HD inline void ppg_rows_item(uint32_t i, const ppg_rows_shape &s, uint32_t *plan, uint32_t *tile_env) {
    if (i == 0u) { plan[0] = s.all; plan[1] = s.w1; plan[2] = s.w2; }
    if (i < s.n_envs) plan[PPG_PLAN_HDR + i] = ppg_rows_prefix(i, s.all);
    if (i < s.tile_words) {
        uint32_t n;
        if (s.range) n = s.all ? ppg_plan_range_first(i, s.w1, s.w2, s.tsz, s.all) : 0u;
        else n = ppg_plan_tile_first(i, s.w1, s.w2);
        tile_env[i] = n / PPG_ROWS_CH;
    }
}

// words of tile_env a plan buffer for up to `capacity` rows needs, whatever the count: tile mode writes at most ceil(all / 32) tiles
// (every tile but the last of a launch holds 32 samples or more), range mode slots * tpw, which grows with the count
PPG_PLAN_HD inline size_t ppg_rows_max_tile_words(int64_t capacity, uint32_t slots, uint32_t range_tile, uint32_t range_st) {
    if (range_tile > 0u) return (size_t)slots * ppg_plan_range_of((uint32_t)capacity, slots, range_st, range_tile).tpw;
    return (size_t)((capacity + 31) / 32) + 1;
}

// The words ppg_policy_plan_rows writes for a grid of `slots` workgroups -- plan[0..2], the prefix sums, tile_env -- made by the same
// items on the CPU.  *n_words = their number; out == NULL or capacity_words too small: only the size is reported.  Returns false for
// arguments no plan exists for.
inline bool ppg_rows_plan_cpu(int64_t capacity, int64_t count, int32_t slots, int32_t range_tile, int32_t range_st, uint32_t *out,
                              uint64_t capacity_words, uint64_t *n_words) {
    if (capacity < 0 || capacity > PPG_ROWS_MAX || slots < 1 || slots > (1 << 20) || range_tile < 0 || (range_tile > 0 && range_st < 1)) return false;
    const ppg_rows_shape s = ppg_rows_shape_of(capacity, count, (uint32_t)slots, (uint32_t)range_tile, (uint32_t)range_st);
    *n_words = (uint64_t)PPG_PLAN_HDR + s.n_envs + s.tile_words;
    if (!out || capacity_words < *n_words) return true;
    if (s.items == 0u) { out[0] = s.all; out[1] = s.w1; out[2] = s.w2; }   // (no env, no tile: a launch would not happen either)
    for (uint32_t i = 0; i < s.items; ++i) ppg_rows_item(i, s, out, out + PPG_PLAN_HDR + s.n_envs);
    return true;
}
