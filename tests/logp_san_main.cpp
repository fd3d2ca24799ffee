// logp_san_main.cpp -- TEST-ONLY stand-alone program: the ppg_record_logp kernel source (predpreygrass_amd/csrc/ppg_logp.h) under the
// CPU wave emulator, built with -fsanitize=address,undefined by tests/test_logp_sanitized.py.  The scan gets exactly the LDS the HIP
// launch declares (ppg::ROWS_SCAN_LDS_BYTES; the emulator poisons the bytes behind it) and every tensor is a heap block of exactly its
// elements -- logp / entropy `capacity` floats, dist capacity * A, the logits B * rows * A, slot [T,B,S], the offsets [B,2] -- so an
// access outside any of them traps.  Compared with a scalar reference after every call, over: capacities that cut a predator run and a
// prey run (rows behind the cut have slot -1), capacity 0, slot words corrupted with out-of-range values (ignored, not followed),
// actions outside [0, A) (PPG_ACTION_UNSET, A, -1, 127: they index nothing), A = 32 and A = 1, rows with one, several and only -inf
// logits, a NaN, magnitudes of 148, row counts outside the region, a skipped species, and device step words that give t = -1, the last
// step and steps past the horizon.  Exit status 0 = clean and equal.
#include "wave_emu/san_main.h"

#include "../predpreygrass_amd/csrc/ppg_logp.h"

constexpr uint64_t SEED = 0x9E3779B97F4A7C15ull;

constexpr int T = 4;
constexpr uint32_t FILL = 0x5A5A5A5Au;

struct Case {
    const char *name;
    int B, cp, cq, A_p, A_q;
    int64_t cap_p, cap_q;   // < 0: room for everything
    bool corrupt;           // slot words of rows in use replaced by values outside [0, capacity)
    int skip;               // species whose logits are NULL, or -1
};

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

struct Out {
    std::vector<uint32_t> logp[2], entropy[2], dist[2];   // float32 tensors as words: compared bit for bit
    Out(const Case &c, const int64_t cap[2]) {
        const int A[2] = {c.A_p, c.A_q};
        for (int s = 0; s < 2; ++s) {
            logp[s].assign((size_t)cap[s], ppg::LOGP_QNAN_BITS);
            entropy[s].assign((size_t)cap[s], ppg::LOGP_QNAN_BITS);
            dist[s].assign((size_t)cap[s] * A[s], FILL);
        }
    }
};

// within one float32 ulp (the program's libm on both sides: in practice the same bits); NaN and +-inf in the same places
static bool near(uint32_t got, uint32_t want) {
    float g, w;
    memcpy(&g, &got, 4); memcpy(&w, &want, 4);
    if (isnan(w) || isnan(g)) return isnan(w) && isnan(g);
    if (isinf(w) || isinf(g)) return g == w;
    return fabs((double)g - (double)w) <= fmax((double)nextafterf(fabsf(w), INFINITY) - (double)fabsf(w), 1e-11);
}

struct World {
    std::vector<int32_t> env_state, slot;
    std::vector<float> logits[2];
    std::vector<int8_t> actions;
    World(const Case &c) : env_state((size_t)c.B * PPG_ENV_WORDS, 0), slot((size_t)T * c.B * (c.cp + c.cq), -1),
                           logits{std::vector<float>((size_t)c.B * c.cp * c.A_p), std::vector<float>((size_t)c.B * c.cq * c.A_q)},
                           actions((size_t)c.B * (c.cp + c.cq), 0) {}
};

static int rows_in_use(const Case &c, const World &w, int b, int s) {
    const int n = w.env_state[(size_t)b * PPG_ENV_WORDS + (s ? PPG_ENV_N_PREY_ROWS : PPG_ENV_N_PRED_ROWS)], cap = s ? c.cq : c.cp;
    return n < 0 ? 0 : n > cap ? cap : n;
}

// new row counts, the slots ppg_record_obs would hand out for step t (cursor: rows stored so far), new logits and actions
static void advance(const Case &c, World &w, const int64_t cap[2], int64_t cursor[2], int t, bool &cut_p, bool &cut_q) {
    const int S = c.cp + c.cq;
    for (int b = 0; b < c.B; ++b) {
        int32_t *es = &w.env_state[(size_t)b * PPG_ENV_WORDS];
        es[PPG_ENV_N_PRED_ROWS] = below(c.cp + 1);
        es[PPG_ENV_N_PREY_ROWS] = below(c.cq + 1);
        if (below(7) == 0) es[PPG_ENV_N_PRED_ROWS] = c.cp + 5;   // (counts outside the region are taken as the region's size / as 0)
        if (below(7) == 0) es[PPG_ENV_N_PREY_ROWS] = -3;
    }
    for (int s = 0; s < 2; ++s) {
        const int first = s ? c.cp : 0, rows = s ? c.cq : c.cp;
        for (int b = 0; b < c.B; ++b) {
            const int n = rows_in_use(c, w, b, s);
            for (int j = 0; j < rows; ++j) {
                int32_t &k = w.slot[((size_t)t * c.B + b) * S + first + j];
                k = -1;
                if (j >= n) continue;
                if (cursor[s] < cap[s]) k = (int32_t)cursor[s]++;
                else if (j > 0 && (&k)[-1] >= 0) (s ? cut_q : cut_p) = true;
            }
        }
    }
    if (c.corrupt) {
        static const int32_t junk[] = {INT32_MAX, INT32_MIN, -2, 0x5A5A5A5A, (int32_t)0x80000001};
        for (size_t i = (size_t)t * c.B * S; i < (size_t)(t + 1) * c.B * S; i += 3) {
            const int s = i % S < (size_t)c.cp ? 0 : 1;
            int32_t v = junk[(i / 3) % 5];
            if (v >= 0 && v < cap[s]) v = -7;
            w.slot[i] = (i / 3) % 11 == 0 ? (int32_t)cap[s] : v;   // (exactly the capacity: one past the end)
        }
    }
    for (int s = 0; s < 2; ++s) {
        const int A = s ? c.A_q : c.A_p;
        std::vector<float> &L = w.logits[s];
        for (size_t r = 0; r < L.size() / A; ++r) {
            float *row = &L[r * A];
            const int kind = below(10);
            for (int a = 0; a < A; ++a) row[a] = kind == 0 ? uniform(-148.f, 148.f) : kind == 1 ? 0.25f : uniform(-6.f, 6.f);
            if (kind == 2) row[below(A)] = -INFINITY;                                            // one -inf
            if (kind == 3) for (int a = 0; a < A; ++a) if (below(3)) row[a] = -INFINITY;         // several, sometimes all
            if (kind == 4) for (int a = 0; a < A; ++a) row[a] = -INFINITY;                       // a row of all -inf
            if (kind == 5) row[below(A)] = NAN;
            if (kind == 6) { row[0] = 148.f; for (int a = 1; a < A; ++a) row[a] = -148.f; }
        }
    }
    static const int bad[] = {PPG_ACTION_UNSET, -1, 127};
    for (size_t i = 0; i < w.actions.size(); ++i) {
        const int A = i % S < (size_t)c.cp ? c.A_p : c.A_q, kind = below(8);
        w.actions[i] = (int8_t)(kind == 0 ? bad[below(3)] : kind == 1 ? A : below(A));   // (A = 32 .. 127 fit int8)
    }
}

// the rules of include/ppg.h, row by row
static void ref_record(const Case &c, const World &w, const int64_t cap[2], Out &x, int64_t t) {
    if (t < 0 || t >= T) return;
    const int S = c.cp + c.cq;
    for (int s = 0; s < 2; ++s) {
        if (s == c.skip) continue;
        const int first = s ? c.cp : 0, A = s ? c.A_q : c.A_p;
        int64_t i = 0;
        for (int b = 0; b < c.B; ++b) {
            const int n = rows_in_use(c, w, b, s);
            for (int j = 0; j < n; ++j, ++i) {
                const int64_t k = w.slot[((size_t)t * c.B + b) * S + first + j];
                if (k < 0 || k >= cap[s]) continue;
                const float *row = &w.logits[s][(size_t)i * A];
                const int a = w.actions[(size_t)b * S + first + j];
                double m = -INFINITY, sum = 0.0, ws = 0.0;
                bool has_nan = false;
                for (int q = 0; q < A; ++q) { if (isnan(row[q])) has_nan = true; else if (row[q] > m) m = row[q]; }
                float lp = NAN, h = NAN;
                if (!has_nan && isfinite(m)) {
                    for (int q = 0; q < A; ++q) {
                        if (row[q] == -INFINITY) continue;
                        const double d = (double)row[q] - m, e = exp(d);
                        sum += e; ws += e * d;
                    }
                    const double ls = log(sum);
                    if (a >= 0 && a < A) lp = (float)(((double)row[a] - m) - ls);
                    h = (float)(ls - ws / sum);
                }
                x.logp[s][(size_t)k] = bits(lp);
                x.entropy[s][(size_t)k] = bits(h);
                for (int q = 0; q < A; ++q) x.dist[s][(size_t)k * A + q] = bits(row[q]);
            }
        }
    }
}


static int run(const Case &c) {
    const int S = c.cp + c.cq;
    const int64_t all[2] = {(int64_t)T * c.B * c.cp, (int64_t)T * c.B * c.cq};
    const int64_t cap[2] = {c.cap_p < 0 ? all[0] : c.cap_p, c.cap_q < 0 ? all[1] : c.cap_q};
    World w(c);
    Out got(c, cap), want(c, cap);
    std::vector<int32_t> off((size_t)c.B * 2, 0), word(1, 0);
    int64_t cursor[2] = {0, 0};
    bool cut_p = false, cut_q = false;
    int bad = 0;

    auto launch = [&](bool on_device, int32_t value) {   // value: the host step, or the device word (= step + 1)
        ppg::LogpParams K;
        memset((void *)&K, 0, sizeof K);
        K.batch = c.B; K.S = S; K.cap_pred = c.cp; K.cap_prey = c.cq;
        K.T = T; K.step_on_device = on_device; K.step = on_device ? 0 : value;
        word[0] = value;
        K.step_dev = on_device ? word.data() : nullptr;
        K.env_state = w.env_state.data();
        for (int s = 0; s < 2; ++s) {
            K.logits[s] = s == c.skip ? nullptr : w.logits[s].data();
            K.n_actions[s] = s ? c.A_q : c.A_p; K.capacity[s] = cap[s];
            K.logp[s] = (float *)got.logp[s].data(); K.entropy[s] = (float *)got.entropy[s].data(); K.dist[s] = got.dist[s].data();
        }
        K.slot = w.slot.data(); K.actions = w.actions.data(); K.off = off.data();
        run_grid<ppg::LogpParams, ppg::logp_scan_main, ppg::ROWS_SCAN_LDS_BYTES>(K, 1);
        run_grid<ppg::LogpParams, ppg::logp_rows_main>(K, c.B);
    };
    auto check = [&](const char *what, long long t) {
        bool same = true;
        size_t finite = 0;
        for (int s = 0; s < 2; ++s) {
            same = same && got.dist[s] == want.dist[s];
            for (size_t k = 0; k < want.logp[s].size(); ++k) {
                same = same && near(got.logp[s][k], want.logp[s][k]) && near(got.entropy[s][k], want.entropy[s][k]);
                float v; memcpy(&v, &want.logp[s][k], 4);
                finite += isfinite(v);
            }
        }
        if (!same) { fprintf(stderr, "%s, %s %lld: the tensors differ from the reference\n", c.name, what, t); bad = 1; }
        return finite;
    };

    launch(true, 0);   // nothing recorded yet: t = -1
    check("device word", 0);
    size_t finite = 0;
    for (int t = 0; t < T; ++t) {   // steps 0, 1: the host index; 2, 3: the device word t + 1 (the last one = T)
        advance(c, w, cap, cursor, t, cut_p, cut_q);
        launch(t >= 2, t >= 2 ? t + 1 : t);
        ref_record(c, w, cap, want, t);
        finite = check("step", t);
    }
    static const int32_t outside[] = {T + 1, T + 9, -1, INT32_MIN, INT32_MAX};
    for (int32_t v : outside) {   // a device word that gives a step outside [0, T): nothing is written
        launch(true, v);
        check("device word", v);
    }
    if ((cap[0] > 0 || cap[1] > 0) && finite == 0) { fprintf(stderr, "%s: the run wrote no finite log-probability\n", c.name); bad = 1; }
    if (c.cap_p > 0 && !c.corrupt && !(cut_p && cut_q)) { fprintf(stderr, "%s: the capacities did not cut a run\n", c.name); bad = 1; }
    return bad;
}

int main() {
    lcg_seed(SEED);
    static const Case cases[] = {
        // name                     B  cp   cq  A_p A_q cap_p cap_q corrupt skip
        {"9 / 9 actions",            3, 64, 128,  9,  9,  -1,  -1, false, -1},
        {"32 / 1 actions",           5, 64,  64, 32,  1,  -1,  -1, false, -1},
        {"128 / 256 rows, 67 envs", 67, 128, 256, 5, 25,  -1,  -1, false, -1},     // the j += 64 loop, two envs per scan lane
        {"capacity cut",             3, 64, 128,  9, 32, 150, 333, false, -1},     // inside a predator run and inside a prey run
        {"capacity 0",               2, 64,  64,  9,  9,   0,   0, false, -1},
        {"corrupted slots",          3, 64, 128,  9, 32,  -1,  -1, true,  -1},
        {"corrupted slots, cut",     3, 64, 128, 32,  9, 101, 207, true,  -1},
        {"predators skipped",        3, 64, 128,  9,  9,  -1,  -1, false,  0},
        {"prey skipped",             3, 64, 128,  9,  9,  -1,  -1, false,  1},
    };
    int bad = 0;
    for (const Case &c : cases) bad |= run(c);
    if (!bad) printf("LOGP-SAN-CLEAN\n");
    return bad;
}
