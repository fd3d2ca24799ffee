// record_san_main.cpp -- TEST-ONLY stand-alone program: the ppg_record kernel source (predpreygrass_amd/csrc/ppg_record.h, which
// calls the link of ppg_link.h) under the CPU wave emulator, built with -fsanitize=address,undefined by
// tests/test_record_sanitized.py.  Every workgroup gets exactly the LDS the HIP launch declares (ppg::LINK_LDS_BYTES); the emulator
// poisons the bytes behind it, and every table is a heap block of exactly its elements -- the trajectory buffers [T,B,S] with
// T = 3 -- so an access outside either traps.  Steps 0, 1, 2 and launches whose device step word is outside [0, T) are compared with
// a scalar reference.  Exit status 0 = clean and equal.
#include "wave_emu/san_main.h"

#include "../predpreygrass_amd/csrc/ppg_record.h"

constexpr uint64_t SEED = 0x2545F4914F6CDD1Dull;

constexpr int T = 3;

// the tables of B envs as the step kernels leave them, and what the previous link call saw (the reference's own snapshot)
struct World {
    int B, cp, cq, S;
    std::vector<int32_t> row_id, env_state, old_id, old_rows, old_episode, next_id;
    std::vector<uint8_t> row_flags;
    std::vector<double> row_reward;
    bool have_old = false;
};

static World make_world(int B, int cp, int cq) {
    World w;
    w.B = B; w.cp = cp; w.cq = cq; w.S = cp + cq;
    const size_t n = (size_t)B * w.S;
    w.row_id.assign(n, 0); w.row_flags.assign(n, 0); w.row_reward.assign(n, 0.0);
    w.env_state.assign((size_t)B * PPG_ENV_WORDS, 0);
    w.old_id.assign(n, 0); w.old_rows.assign(2 * B, 0); w.old_episode.assign(B, 0); w.next_id.assign(2 * B, 0);
    return w;
}

// One "step": per species some agents die (their rows are dropped), the survivors keep their order, newborns get fresh ids; flags at
// random over ALL S rows (rows not in use hold whatever is there); now and then a new episode.  full: both species at capacity.
static void advance(World &w, bool full) {
    const int S = w.S;
    for (int b = 0; b < w.B; ++b) {
        int32_t *es = &w.env_state[(size_t)b * PPG_ENV_WORDS];
        const bool reset = below(5) == 0;
        if (reset) { es[PPG_ENV_EPISODE] += 1; w.next_id[2 * b] = w.next_id[2 * b + 1] = 0; }
        for (int sp = 0; sp < 2; ++sp) {
            const int base = sp ? w.cp : 0, cap = sp ? w.cq : w.cp, word = sp ? PPG_ENV_N_PREY_ROWS : PPG_ENV_N_PRED_ROWS;
            int32_t *id = &w.row_id[(size_t)b * S + base];
            uint8_t *fl = &w.row_flags[(size_t)b * S + base];
            int n = reset ? 0 : es[word], k = 0;
            for (int r = 0; r < n; ++r)
                if (below(6) != 0) { id[k] = id[r]; fl[k] = 0; ++k; }
            const int target = full ? cap : k + below(cap - k + 1);
            for (; k < target; ++k) { id[k] = w.next_id[2 * b + sp]++; fl[k] = PPG_ROW_NEWBORN; }
            es[word] = k;
            for (int r = 0; r < cap; ++r) {
                if (r >= k) { id[r] = below(8); fl[r] = (uint8_t)below(256); }   // not in use: ids that DO occur elsewhere, any flags
                else fl[r] |= (uint8_t)((below(8) == 0 ? PPG_ROW_DIED : 0) | (below(16) == 0 ? PPG_ROW_TRUNC : 0) | (below(2) ? PPG_ROW_ATE : 0));
                const int pick = below(10);
                w.row_reward[(size_t)b * S + base + r] = r >= k ? NAN : pick == 0 ? -0.0 : pick == 1 ? 0.0 : (double)below(2000) / 100.0 - 10.0;
            }
        }
    }
}

// the scalar link: fills prev / next [B,S] and takes the snapshot
static void ref_link(World &w, std::vector<int16_t> &prev, std::vector<int16_t> &next) {
    const int S = w.S;
    prev.assign((size_t)w.B * S, -1); next.assign((size_t)w.B * S, -1);
    for (int b = 0; b < w.B; ++b) {
        const int32_t *es = &w.env_state[(size_t)b * PPG_ENV_WORDS];
        const bool linked = w.have_old && w.old_episode[b] == es[PPG_ENV_EPISODE];
        for (int sp = 0; sp < 2; ++sp) {
            const int base = sp ? w.cp : 0, n_cur = es[sp ? PPG_ENV_N_PREY_ROWS : PPG_ENV_N_PRED_ROWS];
            const int n_old = linked ? w.old_rows[2 * b + sp] : 0;
            for (int j = 0; j < n_old; ++j)
                for (int r = 0; r < n_cur; ++r) {
                    const size_t at = (size_t)b * S + base;
                    if (!(w.row_flags[at + r] & PPG_ROW_NEWBORN) && w.row_id[at + r] == w.old_id[at + j]) {
                        prev[at + r] = (int16_t)(base + j);
                        next[at + j] = (int16_t)(base + r);
                    }
                }
            w.old_rows[2 * b + sp] = n_cur;
        }
        w.old_episode[b] = es[PPG_ENV_EPISODE];
    }
    w.old_id = w.row_id;
    w.have_old = true;
}

struct Buffers {
    std::vector<double> reward;
    std::vector<uint8_t> in_use, terminated, truncated;
    std::vector<int16_t> next_row;
    explicit Buffers(size_t n) : reward(n, 7.0), in_use(n, 0x55), terminated(n, 0x55), truncated(n, 0x55), next_row(n, 0x5555) {}
    bool operator==(const Buffers &o) const {
        return memcmp(reward.data(), o.reward.data(), reward.size() * 8) == 0 && in_use == o.in_use && terminated == o.terminated &&
               truncated == o.truncated && next_row == o.next_row;
    }
};

static void ref_store(const World &w, const std::vector<int16_t> &next, int t, Buffers &x) {
    const size_t step = (size_t)w.B * w.S;
    for (int b = 0; b < w.B; ++b) {
        const int32_t *es = &w.env_state[(size_t)b * PPG_ENV_WORDS];
        for (int r = 0; r < w.S; ++r) {
            const size_t at = (size_t)b * w.S + r, i = (size_t)t * step + at;
            const bool used = r < w.cp ? r < es[PPG_ENV_N_PRED_ROWS] : r - w.cp < es[PPG_ENV_N_PREY_ROWS];
            if (t > 0) x.next_row[i - step] = next[at];
            x.next_row[i] = -1;
            memcpy(&x.reward[i], &w.row_reward[at], 8);
            x.in_use[i] = used;
            x.terminated[i] = used && (w.row_flags[at] & PPG_ROW_DIED);
            x.truncated[i] = used && (w.row_flags[at] & PPG_ROW_TRUNC);
        }
    }
}


static int run(int cp, int cq) {
    const int B = 2;
    World w = make_world(B, cp, cq);
    const size_t rows = (size_t)B * w.S, n = (size_t)T * rows;
    Buffers got(n), want(n);
    std::vector<int32_t> snap_id(rows, 0), snap_episode(B, 0), snap_rows(2 * B, 0);
    std::vector<int16_t> prev(rows, 9), next(rows, 9), want_prev, want_next;
    std::vector<int32_t> word(1, 0);
    int valid = 0, bad = 0;
    char tag[96];

    auto launch = [&](bool on_device, int t) {
        ppg::RecordParams K;
        memset((void *)&K, 0, sizeof K);
        K.batch = B; K.S = w.S; K.cap_pred = cp; K.cap_prey = cq; K.valid = valid;
        K.row_id = w.row_id.data(); K.row_flags = w.row_flags.data(); K.env_state = w.env_state.data();
        K.snap_id = snap_id.data(); K.snap_episode = snap_episode.data(); K.snap_rows = snap_rows.data();
        K.prev_row = prev.data(); K.next_row = next.data();
        K.T = T; K.step_on_device = on_device; K.step = on_device ? 0 : t;
        word[0] = t;
        K.step_dev = on_device ? word.data() : nullptr;
        K.row_reward = (const uint64_t *)w.row_reward.data(); K.reward = (uint64_t *)got.reward.data();
        K.in_use = got.in_use.data(); K.terminated = got.terminated.data(); K.truncated = got.truncated.data();
        K.traj_next = got.next_row.data();
        run_grid<ppg::RecordParams, ppg::record_main, ppg::LINK_LDS_BYTES>(K, B);
        valid = 1;
    };
    auto check = [&](const char *what) {
        if (prev != want_prev || next != want_next) { fprintf(stderr, "%s: the [B,S] link maps differ\n", what); bad = 1; }
        if (!(got == want)) { fprintf(stderr, "%s: the trajectory buffers differ\n", what); bad = 1; }
    };

    long links = 0;
    for (int t = 0; t < T; ++t) {   // steps 0, 1, 2: the host index, then (step 2) the device word
        advance(w, t == 1);
        launch(t == 2, t);
        ref_link(w, want_prev, want_next);
        ref_store(w, want_next, t, want);
        for (int16_t v : want_next) links += v >= 0;
        snprintf(tag, sizeof tag, "S=%d step %d", w.S, t);
        check(tag);
    }
    static const int outside[] = {T, T + 5, -1, INT32_MIN, INT32_MAX};
    for (int v : outside) {   // a device word outside [0, T): the launch is the link alone
        advance(w, false);
        launch(true, v);
        ref_link(w, want_prev, want_next);
        snprintf(tag, sizeof tag, "S=%d device word %d", w.S, v);
        check(tag);
    }
    if (links == 0) { fprintf(stderr, "S=%d: nothing linked, the comparison is empty\n", w.S); bad = 1; }
    return bad;
}

int main() {
    lcg_seed(SEED);
    int bad = 0;
    bad |= run(64, 64);
    bad |= run(64, 128);
    bad |= run(128, 256);
    if (!bad) printf("RECORD-SAN-CLEAN\n");
    return bad;
}
