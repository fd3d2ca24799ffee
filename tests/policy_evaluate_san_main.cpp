// policy_evaluate_san_main.cpp -- TEST-ONLY stand-alone program: the plan of ppg_policy_evaluate (predpreygrass_amd/csrc/ppg_policy_plan.h,
// the only project header included: it needs no HIP) built with -fsanitize=address,undefined by tests/test_policy_evaluate_sanitized.py.
// For tile mode and range mode, slots in {1, 3, 512}, capacity in {1, 200, 70000} and the count list of tests/test_policy_evaluate_plan.py
// the words are written into a heap block of EXACTLY n_words -- an item that writes outside its plan traps -- and checked against a
// scalar restatement: the header, the prefix sums of the pseudo-envs' row counts, the first env of every tile by a linear search, and a
// forward walk that must reach every row in [0, count) once, at its own index.  Exit status 0 = clean and right.
#include <stdio.h>

#include <memory>
#include <vector>

#include "../predpreygrass_amd/csrc/ppg_policy_plan.h"

static int fail(const char *what, long long capacity, long long count, int slots, int range_tile) {
    fprintf(stderr, "%s: capacity %lld count %lld slots %d range_tile %d\n", what, capacity, count, slots, range_tile);
    return 1;
}

static int run(int64_t capacity, int64_t count, int slots, int range_tile, int range_st) {
    uint64_t n_words = 0, again = 0;
    if (!ppg_rows_plan_cpu(capacity, count, slots, range_tile, range_st, nullptr, 0, &n_words)) return fail("refused", capacity, count, slots, range_tile);
    std::unique_ptr<uint32_t[]> w(new uint32_t[n_words]);
    for (uint64_t i = 0; i < n_words; ++i) w[i] = 0xDEADBEEFu;
    if (!ppg_rows_plan_cpu(capacity, count, slots, range_tile, range_st, w.get(), n_words, &again) || again != n_words)
        return fail("second call", capacity, count, slots, range_tile);
    const uint32_t CH = PPG_ROWS_CH, n_envs = (uint32_t)((capacity + CH - 1) / CH);
    const uint32_t all = (uint32_t)(count < 0 ? 0 : count > capacity ? capacity : count);
    if (w[0] != all) return fail("plan[0]", capacity, count, slots, range_tile);
    // prefix sums of the pseudo-envs' counts clamp(all - e CH, 0, CH)
    std::vector<uint32_t> pre(n_envs);
    uint32_t sum = 0;
    for (uint32_t e = 0; e < n_envs; ++e) {
        pre[e] = sum;
        const int64_t left = (int64_t)all - (int64_t)e * CH;
        sum += (uint32_t)(left < 0 ? 0 : left > CH ? CH : left);
        if (w[PPG_PLAN_HDR + e] != pre[e]) return fail("prefix sum", capacity, count, slots, range_tile);
    }
    if (sum != all) return fail("the pseudo-envs' counts", capacity, count, slots, range_tile);
    const uint32_t *tile_env = w.get() + PPG_PLAN_HDR + n_envs;
    const uint64_t tile_words = n_words - PPG_PLAN_HDR - n_envs;
    auto env_of = [&](uint32_t n) {   // the last env whose prefix sum is <= n
        uint32_t e = 0;
        for (uint32_t k = 0; k < n_envs; ++k) if (pre[k] <= n) e = k;
        return e;
    };
    std::vector<uint32_t> seen(all, 0u);
    auto walk = [&](uint64_t tile, uint32_t n0, uint32_t nt) {   // phase_conv's walk from the tile's first env
        if (tile >= tile_words) return false;
        for (uint32_t n = n0; n < n0 + nt; ++n) {
            uint32_t lo = tile_env[tile];
            while (lo + 1 < n_envs && pre[lo + 1] <= n) ++lo;
            const uint32_t row = n - pre[lo];
            if (n >= all || row >= CH || (uint64_t)lo * CH + row != n) return false;
            ++seen[n];
        }
        return true;
    };
    if (range_tile > 0) {
        const uint32_t share = w[1], tpw = w[2];
        const uint32_t want = (uint32_t)range_st * ((all + (uint32_t)slots * range_st - 1u) / ((uint32_t)slots * range_st));
        if (share != want || tpw != (share ? (share + range_tile - 1u) / range_tile : 1u) || tile_words != (uint64_t)slots * tpw)
            return fail("the range header", capacity, count, slots, range_tile);
        for (uint64_t tile = 0; tile < tile_words; ++tile) {
            uint32_t n = (uint32_t)(tile / tpw) * share + (uint32_t)(tile % tpw) * range_tile;
            if (all && n > all - 1u) n = all - 1u;
            if (tile_env[tile] != (all ? env_of(n) : 0u)) return fail("tile_env", capacity, count, slots, range_tile);
        }
        for (uint32_t wg = 0; wg < (uint32_t)slots; ++wg) {
            const uint32_t begin = wg * share, end = begin + share < all ? begin + share : all;
            for (uint32_t j = 0; j < tpw && begin + j * range_tile < end; ++j) {
                const uint32_t n0 = begin + j * range_tile, nt = end - n0 < (uint32_t)range_tile ? end - n0 : (uint32_t)range_tile;
                if (!walk((uint64_t)wg * tpw + j, n0, nt)) return fail("walk", capacity, count, slots, range_tile);
            }
        }
    } else {
        const uint32_t n_full = w[1], ts = w[2];
        if (n_full != (all / (128u * slots)) * slots || (ts != 32u && ts != 64u && ts != 96u && ts != 128u))
            return fail("the tile header", capacity, count, slots, range_tile);
        const uint32_t n_tiles = n_full + (all - n_full * 128u + ts - 1u) / ts;
        if (tile_words != n_tiles) return fail("the tile count", capacity, count, slots, range_tile);
        if ((uint64_t)(all - n_full * 128u) > (uint64_t)ts * slots) return fail("the last round", capacity, count, slots, range_tile);
        for (uint32_t tile = 0; tile < n_tiles; ++tile) {
            const uint32_t size = tile < n_full ? 128u : ts, n0 = tile < n_full ? tile * 128u : n_full * 128u + (tile - n_full) * ts;
            if (tile_env[tile] != env_of(n0)) return fail("tile_env", capacity, count, slots, range_tile);
            if (!walk(tile, n0, all - n0 < size ? all - n0 : size)) return fail("walk", capacity, count, slots, range_tile);
        }
    }
    for (uint32_t n = 0; n < all; ++n) if (seen[n] != 1u) return fail("a row was not reached exactly once", capacity, count, slots, range_tile);
    return 0;
}

int main() {
    // (range_tile, sub-group): tile mode; the one-role direct-head kernels' 126 = 14 x 9; the pipeline's 518 = 74 x 7; a tile of one sub-group
    static const int MODES[][2] = {{0, 9}, {126, 9}, {518, 7}, {16, 16}};
    static const int SLOTS[] = {1, 3, 512};
    static const int64_t CAPACITIES[] = {1, 200, 70000};
    int bad = 0;
    for (const auto &m : MODES)
        for (int slots : SLOTS)
            for (int64_t capacity : CAPACITIES) {
                const int64_t counts[] = {0, 1, 31, 32, 33, 127, 128, 129, capacity - 1, capacity, capacity + 5, -4};
                for (int64_t count : counts) bad |= run(capacity, count, slots, m[0], m[1]);
            }
    // capacity 0: a header and nothing else; arguments no plan exists for are refused
    uint64_t n = 0;
    bad |= run(0, 0, 4, 0, 9);
    bad |= ppg_rows_plan_cpu(-1, 0, 4, 0, 9, nullptr, 0, &n) ? 1 : 0;
    bad |= ppg_rows_plan_cpu(100, 0, 0, 0, 9, nullptr, 0, &n) ? 1 : 0;
    bad |= ppg_rows_plan_cpu(100, 0, 4, 128, 0, nullptr, 0, &n) ? 1 : 0;
    if (!bad) printf("POLICY-EVALUATE-SAN-CLEAN\n");
    return bad;
}
