// backward_samples_san_main.cpp -- TEST-ONLY stand-alone program: the ppg_backward_samples kernel source
// (predpreygrass_amd/csrc/ppg_backward.h) under the CPU wave emulator, built with -fsanitize=address,undefined by
// tests/test_backward_samples_sanitized.py.  Every workgroup gets exactly the LDS the HIP launch declares (ppg::BACKWARD_LDS_BYTES); the
// emulator poisons the bytes behind it, and every tensor is a heap block of exactly its stated size -- [T,B,S] inputs, [horizon,B,S]
// slots, [capacity[s]] values and outputs, [B,2,3] stats -- so a slot word that escaped its range check, or any other access outside
// a tensor, traps.  The outputs are compared bit for bit with a scalar recursion written from the formulas of include/ppg.h.
// Exit status 0 = clean and equal.
#include "wave_emu/san_main.h"

#include "../predpreygrass_amd/csrc/ppg_backward.h"

constexpr uint64_t SEED = 0x2545F4914F6CDD1Dull;

struct Case {
    int T, H, B, S, cp;          // H: the store's horizon (T + 1: one step of slots the call must not read)
    int32_t capacity[2];
    std::vector<double> reward;
    std::vector<double> values[2];
    std::vector<float> values32[2];
    std::vector<int16_t> next_row;
    std::vector<uint8_t> in_use, terminated, truncated;
    std::vector<int32_t> slot;
};

// Rows in use at random (about two thirds), links to random rows in use of the next step, a tenth terminated, a twentieth truncated,
// NaN rewards in rows not in use; bad_links: a quarter of the rows in use get a next_row outside [0, S).  Slots: a running cursor per
// species over the rows in use (step, env, row), cut at 60 % of the prey rows; bad_slots: a fifth of ALL rows get a word that is
// outside the capacity (capacity, capacity + 5, -2, INT32_MAX, INT32_MIN), rows not in use get any word in [-3, capacity + 3).
// Values are NaN at and above the stored count.
static Case make_case(int T, int B, int cp, int cq, bool bad_links, bool bad_slots, bool empty_pred) {
    Case c;
    const int S = cp + cq;
    c.T = T; c.H = T + 1; c.B = B; c.S = S; c.cp = cp;
    const size_t n = (size_t)T * B * S;
    c.reward.resize(n); c.next_row.resize(n); c.in_use.resize(n); c.terminated.resize(n); c.truncated.resize(n);
    c.slot.assign((size_t)c.H * B * S, -1);
    static const int16_t outside[5] = {0, 7, -2, 32767, -32768};   // (the first two are added to S)
    size_t rows[2] = {0, 0};
    for (size_t i = 0; i < n; ++i) {
        c.in_use[i] = below(3) != 0;
        rows[(int)(i % S) >= cp] += c.in_use[i];
    }
    c.capacity[0] = empty_pred ? 0 : (int32_t)rows[0] + 3;
    c.capacity[1] = (int32_t)(rows[1] * 6 / 10);
    int32_t cursor[2] = {0, 0};
    for (int t = 0; t < T; ++t)
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < S; ++r) {
                const size_t i = ((size_t)t * B + b) * S + r;
                const int s = r >= cp;
                const bool used = c.in_use[i] != 0;
                const int pick = below(10);
                c.reward[i] = !used ? NAN : pick == 0 ? -0.0 : pick == 1 ? 0.0 : unit() * 4.0 - 2.0;
                c.terminated[i] = below(10) == 0;
                c.truncated[i] = below(20) == 0;
                int16_t nx = -1;
                if (t + 1 < T && below(8) != 0) {
                    for (int tries = 0; tries < 16 && nx < 0; ++tries) {
                        const int j = below(S);
                        if (c.in_use[((size_t)(t + 1) * B + b) * S + j]) nx = (int16_t)j;
                    }
                }
                if (bad_links && below(4) == 0) {
                    const int k = below(5);
                    nx = k < 2 ? (int16_t)(S + outside[k]) : outside[k];
                }
                c.next_row[i] = used ? nx : (int16_t)(below(S + 2) - 1);
                int32_t k = -1;
                if (used && cursor[s] < c.capacity[s]) k = cursor[s]++;
                if (!used) k = below(c.capacity[s] + 6) - 3;
                if (bad_slots && below(5) == 0) {
                    static const int32_t junk[3] = {-2, INT32_MAX, INT32_MIN};
                    const int w = below(5);
                    k = w == 0 ? c.capacity[s] : w == 1 ? c.capacity[s] + 5 : junk[w - 2];
                }
                c.slot[i] = k;
            }
    for (size_t i = n; i < c.slot.size(); ++i) c.slot[i] = below(cursor[(int)(i % S) >= cp] + 1);
    for (int s = 0; s < 2; ++s) {
        c.values[s].resize((size_t)c.capacity[s]); c.values32[s].resize((size_t)c.capacity[s]);
        for (int32_t k = 0; k < c.capacity[s]; ++k) {
            c.values[s][k] = k < cursor[s] ? unit() * 2.0 - 1.0 : NAN;
            c.values32[s][k] = k < cursor[s] ? (float)(unit() * 2.0 - 1.0) : NAN;
        }
    }
    return c;
}

struct Want {
    std::vector<float> adv[2], ret[2];
    std::vector<double> stats;
};

// the scalar reference: the recursion of include/ppg.h over [T,B,S], then the stores and the sums in the stated order
static void reference(const Case &c, bool f32, bool no_pred_values, double gamma, double lam, Want &w) {
    const int T = c.T, B = c.B, S = c.S;
    const double gl = gamma * lam;
    const size_t n = (size_t)T * B * S;
    std::vector<double> G(n), A(n), V(n);
    std::vector<uint8_t> stored(n);
    for (size_t i = 0; i < n; ++i) {
        const int s = (int)(i % S) >= c.cp;
        const int32_t k = c.slot[i];
        stored[i] = c.in_use[i] && k >= 0 && k < c.capacity[s];
        const bool have = stored[i] && !(s == 0 && no_pred_values);
        V[i] = !have ? 0.0 : f32 ? (double)c.values32[s][k] : c.values[s][k];
    }
    for (int t = T - 1; t >= 0; --t)
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < S; ++r) {
                const size_t i = ((size_t)t * B + b) * S + r;
                const int nx = c.next_row[i];
                const bool used = c.in_use[i] != 0;
                const bool has = t + 1 < T && used && !c.terminated[i] && !c.truncated[i] && nx >= 0 && nx < S;
                const size_t j = has ? ((size_t)(t + 1) * B + b) * S + nx : 0;
                const double g_succ = has ? G[j] : 0.0, a_succ = has ? A[j] : 0.0, v_succ = has ? V[j] : 0.0;
                const double gm = g_succ * gamma, g = c.reward[i] + gm;
                const double vm = v_succ * gamma, boot = c.reward[i] + vm, delta = boot - V[i], am = a_succ * gl, a = delta + am;
                G[i] = used ? g : 0.0;
                A[i] = used ? a : 0.0;
            }
    for (int s = 0; s < 2; ++s) { w.adv[s].assign((size_t)c.capacity[s], 7.0f); w.ret[s].assign((size_t)c.capacity[s], 7.0f); }
    w.stats.assign((size_t)B * 6, 0.0);
    for (int b = 0; b < B; ++b) {
        double acc[2][3][64] = {};
        for (int t = T - 1; t >= 0; --t)
            for (int q = 0; q < S / 64; ++q)
                for (int l = 0; l < 64; ++l) {
                    const int r = 64 * q + l, s = r >= c.cp;
                    const size_t i = ((size_t)t * B + b) * S + r;
                    if (!stored[i]) continue;
                    w.adv[s][c.slot[i]] = (float)A[i];
                    w.ret[s][c.slot[i]] = (float)G[i];
                    acc[s][0][l] = acc[s][0][l] + 1.0;
                    acc[s][1][l] = acc[s][1][l] + A[i];
                    const double p = A[i] * A[i];
                    acc[s][2][l] = acc[s][2][l] + p;
                }
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 3; ++k) {
                for (int m = 1; m < 64; m <<= 1) {
                    double next[64];
                    for (int l = 0; l < 64; ++l) next[l] = acc[s][k][l] + acc[s][k][l ^ m];
                    memcpy(acc[s][k], next, sizeof next);
                }
                w.stats[((size_t)b * 2 + s) * 3 + k] = acc[s][k][0];
            }
    }
}


static bool differ(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() != b.size() || (a.size() && memcmp(a.data(), b.data(), a.size() * 4) != 0);
}

static int run(const Case &c, bool want_g, bool want_a, bool want_stats, bool f32, bool no_pred_values, int prefetch, const char *tag) {
    const double gamma = 0.97, lam = 0.9;
    Want got, want;
    for (int s = 0; s < 2; ++s) {
        got.adv[s].assign(want_a ? (size_t)c.capacity[s] : 0, 7.0f);
        got.ret[s].assign(want_g ? (size_t)c.capacity[s] : 0, 7.0f);
    }
    got.stats.assign(want_stats ? (size_t)c.B * 6 : 0, 7.0);
    static float nothing;   // (an empty vector has no address: a species of capacity 0 is never addressed)
    ppg::BackwardSamplesParams K;
    memset(&K, 0, sizeof K);
    K.batch = c.B; K.S = c.S; K.T = c.T; K.cap_pred = c.cp; K.values_f32 = f32; K.prefetch = prefetch;
    K.reward = c.reward.data(); K.next_row = c.next_row.data();
    K.in_use = c.in_use.data(); K.terminated = c.terminated.data(); K.truncated = c.truncated.data();
    K.slot = c.slot.data();
    for (int s = 0; s < 2; ++s) {
        K.capacity[s] = c.capacity[s];
        const void *v = f32 ? (const void *)c.values32[s].data() : (const void *)c.values[s].data();
        K.values[s] = !want_a || (s == 0 && no_pred_values) ? nullptr : c.capacity[s] ? v : (const void *)&nothing;
        K.advantage[s] = !want_a ? nullptr : c.capacity[s] ? got.adv[s].data() : &nothing;
        K.returns[s] = !want_g ? nullptr : c.capacity[s] ? got.ret[s].data() : &nothing;
    }
    K.gamma = gamma; K.gl = gamma * lam;
    K.stats = want_stats ? got.stats.data() : nullptr;
    run_grid<ppg::BackwardSamplesParams, ppg::backward_samples_main, ppg::BACKWARD_LDS_BYTES>(K, c.B);
    reference(c, f32, no_pred_values, gamma, lam, want);
    int bad = 0;
    for (int s = 0; s < 2; ++s) {
        if (want_g && differ(got.ret[s], want.ret[s])) { fprintf(stderr, "%s: returns[%d] differ\n", tag, s); bad = 1; }
        if (want_a && differ(got.adv[s], want.adv[s])) { fprintf(stderr, "%s: advantage[%d] differ\n", tag, s); bad = 1; }
        for (float x : got.adv[s]) if (x != x) { fprintf(stderr, "%s: NaN in advantage[%d]\n", tag, s); return 1; }
        for (float x : got.ret[s]) if (x != x) { fprintf(stderr, "%s: NaN in returns[%d]\n", tag, s); return 1; }
    }
    if (want_stats && memcmp(got.stats.data(), want.stats.data(), got.stats.size() * 8) != 0) { fprintf(stderr, "%s: stats differ\n", tag); bad = 1; }
    return bad;
}

int main() {
    lcg_seed(SEED);
    int bad = 0;
    char tag[128];
    static const int shapes[3][2] = {{64, 64}, {64, 128}, {128, 256}};
    for (const auto &shape : shapes)
        for (int T : {1, 9})
            for (int wrong = 0; wrong < 3; ++wrong) {   // 1: out-of-range links and slot words; 2: a predator store of capacity 0
                if (wrong == 1 && T == 1) continue;
                const Case c = make_case(T, 2, shape[0], shape[1], wrong == 1, wrong == 1, wrong == 2);
                for (int prefetch = 0; prefetch < 2; ++prefetch) {
                    snprintf(tag, sizeof tag, "S=%d+%d T=%d case=%d prefetch=%d", shape[0], shape[1], T, wrong, prefetch);
                    bad |= run(c, true, true, true, false, false, prefetch, tag);
                    bad |= run(c, true, true, true, true, false, prefetch, tag);
                    bad |= run(c, true, false, false, false, false, prefetch, tag);
                    bad |= run(c, false, true, true, false, false, prefetch, tag);
                    bad |= run(c, true, true, false, false, true, prefetch, tag);
                }
            }
    if (!bad) printf("BACKWARD-SAMPLES-SAN-CLEAN\n");
    return bad;
}
