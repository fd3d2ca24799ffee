// obs_store_san_main.cpp -- TEST-ONLY stand-alone program: the ppg_record_obs kernel source (predpreygrass_amd/csrc/ppg_obs_store.h)
// under the CPU wave emulator, built with -fsanitize=address,undefined by tests/test_obs_store_sanitized.py.  The scan gets exactly
// the LDS the HIP launch declares (ppg::ROWS_SCAN_LDS_BYTES; the emulator poisons the bytes behind it) and every tensor is a heap block
// of exactly its elements -- the stores `capacity` rows, slot [T,B,S] -- so an access outside any of them traps.  Compared with a
// scalar reference after every call, over: element sizes 8 / 4 / 2 and float64 -> float32, block sizes that leave the destination 0,
// 4, 8 and 12 bytes off a 16-byte line, stores that are not even 4-byte aligned (the byte loop), single-row runs that end inside the
// head, capacities that cut a predator run and a prey run, capacity 0, a device step word outside [0, T), and a slot[t-1] corrupted
// with out-of-range words, which must be ignored, not followed.  Exit status 0 = clean and equal.
#include "wave_emu/san_main.h"

#include "../predpreygrass_amd/csrc/ppg_obs_store.h"

constexpr uint64_t SEED = 0x9E3779B97F4A7C15ull;

constexpr int T = 4;

struct Case {
    const char *name;
    int B, cp, cq, blk_p, blk_q, src_elem, dst_elem;
    int64_t cap_p, cap_q;   // < 0: room for everything
    int shift;              // bytes the observation stores start into their heap block
    bool few_rows;          // envs of 0 .. 2 rows: single-row runs
};

// a heap block of exactly n bytes behind `shift` unused ones
struct Block {
    std::vector<unsigned char> mem;
    int shift;
    Block(size_t n, int shift_, unsigned char fill) : mem(n + (size_t)shift_, fill), shift(shift_) {}
    unsigned char *data() { return mem.data() + shift; }
};

struct Store {
    Block obs[2];
    std::vector<int32_t> sample[2], slot;
    std::vector<int8_t> action[2];
    int64_t cursor[4] = {0, 0, 0, 0};
    Store(const Case &c, const int64_t cap[2], size_t slots)
        : obs{Block((size_t)cap[0] * c.blk_p * c.dst_elem, c.shift, 0x5A), Block((size_t)cap[1] * c.blk_q * c.dst_elem, c.shift, 0x5A)},
          slot(slots, 0x5A5A5A5A) {
        for (int s = 0; s < 2; ++s) { sample[s].assign((size_t)cap[s], 0x5A5A5A5A); action[s].assign((size_t)cap[s], 0x5A); }
    }
    bool same(const Store &o) const {
        return obs[0].mem == o.obs[0].mem && obs[1].mem == o.obs[1].mem && sample[0] == o.sample[0] && sample[1] == o.sample[1] &&
               action[0] == o.action[0] && action[1] == o.action[1] && slot == o.slot && memcmp(cursor, o.cursor, sizeof cursor) == 0;
    }
};

struct World {
    std::vector<int32_t> env_state;
    Block src[2];
    std::vector<int8_t> actions;
    World(const Case &c)
        : env_state((size_t)c.B * PPG_ENV_WORDS, 0), src{Block((size_t)c.B * c.cp * c.blk_p * c.src_elem, 0, 0), Block((size_t)c.B * c.cq * c.blk_q * c.src_elem, 0, 0)},
          actions((size_t)c.B * (c.cp + c.cq), 0) {}
};

static void advance(const Case &c, World &w) {
    for (int b = 0; b < c.B; ++b) {
        int32_t *es = &w.env_state[(size_t)b * PPG_ENV_WORDS];
        es[PPG_ENV_N_PRED_ROWS] = c.few_rows ? below(3) : below(c.cp + 1);
        es[PPG_ENV_N_PREY_ROWS] = c.few_rows ? below(3) : below(c.cq + 1);
        if (below(7) == 0) es[PPG_ENV_N_PRED_ROWS] = c.cp + 5;   // (counts outside the region are taken as the region's size / as 0)
        if (below(7) == 0) es[PPG_ENV_N_PREY_ROWS] = -3;
    }
    for (int s = 0; s < 2; ++s) {
        if (c.src_elem == 8) {   // doubles that round: no NaN payloads (the conversion of a signalling NaN is not compared)
            double *d = (double *)w.src[s].data();
            for (size_t i = 0; i < w.src[s].mem.size() / 8; ++i) d[i] = ((double)rnd() - 1e9) / 977.0 * (below(4) == 0 ? 1e-30 : 1.0);
        } else {
            for (unsigned char &v : w.src[s].mem) v = (unsigned char)rnd();
        }
    }
    for (int8_t &a : w.actions) a = (int8_t)below(9);
}

static int rows_in_use(const Case &c, const World &w, int b, int s) {
    const int n = w.env_state[(size_t)b * PPG_ENV_WORDS + (s ? PPG_ENV_N_PREY_ROWS : PPG_ENV_N_PRED_ROWS)], cap = s ? c.cq : c.cp;
    return n < 0 ? 0 : n > cap ? cap : n;
}

static bool g_cut_inside[2];   // a call stored some rows of an env's run and dropped the rest

// the rules of include/ppg.h, row by row
static void ref_record(const Case &c, World &w, const int64_t cap[2], Store &x, int t, bool with_actions) {
    const int S = c.cp + c.cq;
    const size_t step = (size_t)c.B * S;
    for (int s = 0; s < 2; ++s) {
        const int first = s ? c.cp : 0, rows = s ? c.cq : c.cp, blk = s ? c.blk_q : c.blk_p;
        int64_t k = x.cursor[s];
        for (int b = 0; b < c.B; ++b) {
            const int n = rows_in_use(c, w, b, s);
            for (int j = 0; j < rows; ++j) {
                const size_t i = (size_t)t * step + (size_t)b * S + first + j;
                if (j >= n) { x.slot[i] = -1; continue; }
                if (k < cap[s]) {
                    const unsigned char *from = w.src[s].data() + ((size_t)b * rows + j) * blk * c.src_elem;
                    unsigned char *to = x.obs[s].data() + (size_t)k * blk * c.dst_elem;
                    if (c.src_elem == c.dst_elem) memcpy(to, from, (size_t)blk * c.src_elem);
                    else for (int e = 0; e < blk; ++e) { double v; memcpy(&v, from + 8 * (size_t)e, 8); const float f = (float)v; memcpy(to + 4 * (size_t)e, &f, 4); }
                    x.sample[s][(size_t)k] = (int32_t)i;
                    x.action[s][(size_t)k] = (int8_t)PPG_ACTION_UNSET;
                    x.slot[i] = (int32_t)k;
                    ++k;
                } else {
                    if (j > 0 && x.slot[i - 1] >= 0) g_cut_inside[s] = true;
                    x.slot[i] = -1;
                    ++x.cursor[2 + s];
                }
            }
        }
        x.cursor[s] = k;
        if (with_actions && t > 0)
            for (int b = 0; b < c.B; ++b)
                for (int j = 0; j < rows; ++j) {
                    const int64_t p = x.slot[(size_t)(t - 1) * step + (size_t)b * S + first + j];
                    if (p >= 0 && p < cap[s]) x.action[s][(size_t)p] = w.actions[(size_t)b * S + first + j];
                }
    }
}


static int run(const Case &c) {
    const int S = c.cp + c.cq;
    const int64_t all[2] = {(int64_t)T * c.B * c.cp, (int64_t)T * c.B * c.cq};
    const int64_t cap[2] = {c.cap_p < 0 ? all[0] : c.cap_p, c.cap_q < 0 ? all[1] : c.cap_q};
    World w(c);
    Store got(c, cap, (size_t)T * c.B * S), want(c, cap, (size_t)T * c.B * S);
    std::vector<int64_t> base((size_t)c.B * 2, 0);
    std::vector<int32_t> word(1, 0);
    int bad = 0;
    g_cut_inside[0] = g_cut_inside[1] = false;

    auto launch = [&](bool on_device, int t, bool with_actions) {
        ppg::ObsStoreParams K;
        memset((void *)&K, 0, sizeof K);
        K.batch = c.B; K.S = S; K.cap_pred = c.cp; K.cap_prey = c.cq;
        K.T = T; K.step_on_device = on_device; K.step = on_device ? 0 : t;
        word[0] = t;
        K.step_dev = on_device ? word.data() : nullptr;
        K.env_state = w.env_state.data();
        K.blk[0] = c.blk_p; K.blk[1] = c.blk_q; K.src_elem = c.src_elem; K.dst_elem = c.dst_elem;
        for (int s = 0; s < 2; ++s) {
            K.src[s] = w.src[s].data(); K.dst[s] = got.obs[s].data(); K.capacity[s] = cap[s];
            K.sample[s] = got.sample[s].data(); K.action[s] = got.action[s].data();
        }
        K.slot = got.slot.data(); K.cursor = got.cursor; K.base = base.data();
        K.actions = with_actions ? w.actions.data() : nullptr;
        run_grid<ppg::ObsStoreParams, ppg::obs_scan_main, ppg::ROWS_SCAN_LDS_BYTES>(K, 1);
        run_grid<ppg::ObsStoreParams, ppg::obs_rows_main>(K, c.B);
    };
    auto check = [&](const char *what, int t) {
        if (!got.same(want)) { fprintf(stderr, "%s, %s %d: the stores differ (cursor %lld %lld %lld %lld, want %lld %lld %lld %lld)\n", c.name, what, t,
                                       (long long)got.cursor[0], (long long)got.cursor[1], (long long)got.cursor[2], (long long)got.cursor[3],
                                       (long long)want.cursor[0], (long long)want.cursor[1], (long long)want.cursor[2], (long long)want.cursor[3]); bad = 1; }
    };

    for (int t = 0; t < T; ++t) {   // steps 0 .. 3: the host index, then (from step 2 on) the device word
        advance(c, w);
        if (t == 2) {   // slot[t-1] as a stale or foreign buffer would leave it: words outside [0, capacity) in rows in use and not
            static const int32_t junk[] = {INT32_MAX, INT32_MIN, -2, 0x5A5A5A5A, (int32_t)0x80000001};
            for (size_t i = (size_t)(t - 1) * c.B * S; i < (size_t)t * c.B * S; i += 3) {
                int32_t v = junk[(i / 3) % 5];
                if (v >= 0 && v < cap[i % S < (size_t)c.cp ? 0 : 1]) v = -7;
                got.slot[i] = want.slot[i] = v;
            }
            if (cap[0] > 0) got.slot[(size_t)(t - 1) * c.B * S] = want.slot[(size_t)(t - 1) * c.B * S] = (int32_t)cap[0];   // one past the end
        }
        launch(t >= 2, t, t != 3);
        ref_record(c, w, cap, want, t, t != 3);
        check("step", t);
    }
    static const int outside[] = {T, T + 9, -1, INT32_MIN, INT32_MAX};
    for (int v : outside) {   // a device word outside [0, T): nothing is written, the cursor included
        advance(c, w);
        launch(true, v, true);
        check("device word", v);
    }
    if (c.cap_p < 0 && (want.cursor[2] || want.cursor[3] || !want.cursor[0] || !want.cursor[1])) { fprintf(stderr, "%s: the run is empty or dropped rows\n", c.name); bad = 1; }
    if (c.cap_p > 0 && !(g_cut_inside[0] && g_cut_inside[1] && want.cursor[0] == cap[0] && want.cursor[1] == cap[1])) {
        fprintf(stderr, "%s: the capacities did not cut the run\n", c.name); bad = 1;
    }
    return bad;
}

int main() {
    lcg_seed(SEED);
    static const Case cases[] = {
        // name                  B  cp   cq  blk_p blk_q src dst cap_p cap_q shift few
        {"f64 7x7 / 9x9",         3, 64, 128, 196, 324, 8, 8, -1, -1, 0, false},     // aligned: the 16-byte main loop
        {"f64 -> f32, 5 / 7 ch",  3, 64, 128, 125, 343, 8, 4, -1, -1, 0, false},     // 500 / 1372-byte rows: heads of 1 .. 3 elements
        {"f32 5 ch 3x3 / 5x5",    5, 64, 128, 45, 125, 4, 4, -1, -1, 0, false},      // 180 / 500-byte rows: heads of 1 .. 3 words
        {"bf16 1x1, few rows",   67, 64, 64, 4, 4, 2, 2, -1, -1, 0, true},           // 8-byte rows, runs that end inside the head; 67 envs
        {"bf16 3x3 / 5x5",        3, 128, 256, 36, 100, 2, 2, -1, -1, 0, false},
        {"bf16, store + 2 bytes", 2, 64, 128, 36, 100, 2, 2, -1, -1, 2, false},      // the byte loop
        {"f64 -> f32 few rows",   5, 64, 64, 9, 25, 8, 4, -1, -1, 0, true},          // runs shorter than a head plus a quad
        {"capacity cut",          3, 64, 128, 36, 100, 2, 2, 150, 333, 0, false},    // inside a predator run and inside a prey run
        {"capacity cut, f32",     3, 64, 128, 125, 343, 8, 4, 101, 207, 0, false},
        {"capacity 0",            2, 64, 64, 36, 100, 2, 2, 0, 0, 0, false},
    };
    int bad = 0;
    for (const Case &c : cases) bad |= run(c);
    if (!bad) printf("OBS-STORE-SAN-CLEAN\n");
    return bad;
}
