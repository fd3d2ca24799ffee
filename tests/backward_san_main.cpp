// backward_san_main.cpp -- TEST-ONLY stand-alone program: the ppg_backward kernel source (predpreygrass_amd/csrc/ppg_backward.h)
// under the CPU wave emulator, built with -fsanitize=address,undefined by tests/test_backward_sanitized.py.  Every workgroup gets
// exactly the LDS the HIP launch declares (ppg::BACKWARD_LDS_BYTES); the emulator poisons the bytes behind it, and the tensors are
// heap blocks of exactly [T,B,S] elements, so an access outside either traps.  The outputs are compared bit for bit with a scalar
// recursion written from the formulas of include/ppg.h.  Exit status 0 = clean and equal.
#include "wave_emu/san_main.h"

#include "../predpreygrass_amd/csrc/ppg_backward.h"

constexpr uint64_t SEED = 0x2545F4914F6CDD1Dull;

struct Case {
    int T, B, S;
    std::vector<double> reward, values;
    std::vector<float> values32;
    std::vector<int16_t> next_row;
    std::vector<uint8_t> in_use, terminated, truncated;
};

// Rows in use at random (about two thirds), links to random rows in use of the next step (not injective: the kernel only reads),
// a tenth terminated, a twentieth truncated, NaN reward / values in rows not in use, -0.0 and 0.0 rewards.  bad_links: a quarter
// of the rows in use get a next_row outside [0, S) instead.
static Case make_case(int T, int B, int S, bool bad_links) {
    Case c;
    c.T = T; c.B = B; c.S = S;
    const size_t n = (size_t)T * B * S;
    c.reward.resize(n); c.values.resize(n); c.values32.resize(n); c.next_row.resize(n);
    c.in_use.resize(n); c.terminated.resize(n); c.truncated.resize(n);
    static const int16_t outside[5] = {0, 7, -2, 32767, -32768};   // (the first two are added to S)
    for (size_t i = 0; i < n; ++i) c.in_use[i] = below(3) != 0;
    for (int t = 0; t < T; ++t)
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < S; ++r) {
                const size_t i = ((size_t)t * B + b) * S + r;
                const bool used = c.in_use[i] != 0;
                const int pick = below(10);
                c.reward[i] = !used ? NAN : pick == 0 ? -0.0 : pick == 1 ? 0.0 : unit() * 4.0 - 2.0;
                c.values32[i] = !used ? NAN : (float)(unit() * 2.0 - 1.0);
                c.values[i] = !used ? NAN : unit() * 2.0 - 1.0;
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
            }
    return c;
}

static void reference(const Case &c, bool f32, double gamma, double lam, std::vector<double> &G, std::vector<double> &A) {
    const int T = c.T, B = c.B, S = c.S;
    const double gl = gamma * lam;
    G.assign((size_t)T * B * S, -1.0); A.assign((size_t)T * B * S, -1.0);
    for (int t = T - 1; t >= 0; --t)
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < S; ++r) {
                const size_t i = ((size_t)t * B + b) * S + r;
                const int nx = c.next_row[i];
                const bool used = c.in_use[i] != 0;
                const bool has = t + 1 < T && used && !c.terminated[i] && !c.truncated[i] && nx >= 0 && nx < S;
                const size_t j = has ? ((size_t)(t + 1) * B + b) * S + nx : 0;
                const double g_succ = has ? G[j] : 0.0, a_succ = has ? A[j] : 0.0;
                const double v_succ = has ? (f32 ? (double)c.values32[j] : c.values[j]) : 0.0;
                const double v = f32 ? (double)c.values32[i] : c.values[i];
                const double gm = g_succ * gamma, g = c.reward[i] + gm;
                const double vm = v_succ * gamma, boot = c.reward[i] + vm, delta = boot - v, am = a_succ * gl, a = delta + am;
                G[i] = used ? g : 0.0;
                A[i] = used ? a : 0.0;
            }
}


static int run(const Case &c, bool want_g, bool want_a, bool f32, int prefetch, const char *tag) {
    const double gamma = 0.97, lam = 0.9;
    const size_t n = (size_t)c.T * c.B * c.S;
    std::vector<double> G(want_g ? n : 0, 7.0), A(want_a ? n : 0, 7.0), wantG, wantA;
    ppg::BackwardParams K;
    memset(&K, 0, sizeof K);
    K.batch = c.B; K.S = c.S; K.T = c.T; K.values_f32 = f32; K.prefetch = prefetch;
    K.reward = c.reward.data(); K.next_row = c.next_row.data();
    K.in_use = c.in_use.data(); K.terminated = c.terminated.data(); K.truncated = c.truncated.data();
    K.values = !want_a ? nullptr : f32 ? (const void *)c.values32.data() : (const void *)c.values.data();
    K.gamma = gamma; K.gl = gamma * lam;
    K.returns = want_g ? G.data() : nullptr; K.advantages = want_a ? A.data() : nullptr;
    run_grid<ppg::BackwardParams, ppg::backward_main, ppg::BACKWARD_LDS_BYTES>(K, c.B);
    reference(c, f32, gamma, lam, wantG, wantA);
    int bad = 0;
    if (want_g && memcmp(G.data(), wantG.data(), n * 8) != 0) { fprintf(stderr, "%s: returns differ\n", tag); bad = 1; }
    if (want_a && memcmp(A.data(), wantA.data(), n * 8) != 0) { fprintf(stderr, "%s: advantages differ\n", tag); bad = 1; }
    for (size_t i = 0; i < n; ++i)
        if ((want_g && G[i] != G[i]) || (want_a && A[i] != A[i])) { fprintf(stderr, "%s: NaN in an output\n", tag); return 1; }
    return bad;
}

int main() {
    lcg_seed(SEED);
    int bad = 0;
    char tag[96];
    for (int S : {128, 384})
        for (int T : {1, 9})
            for (int wrong = 0; wrong < 2; ++wrong) {
                if (wrong && T == 1) continue;
                const Case c = make_case(T, 2, S, wrong != 0);
                for (int prefetch = 0; prefetch < 2; ++prefetch) {
                    snprintf(tag, sizeof tag, "S=%d T=%d out-of-range=%d prefetch=%d", S, T, wrong, prefetch);
                    bad |= run(c, true, false, false, prefetch, tag);
                    bad |= run(c, false, true, false, prefetch, tag);
                    bad |= run(c, true, true, false, prefetch, tag);
                    bad |= run(c, true, true, true, prefetch, tag);
                }
            }
    if (!bad) printf("BACKWARD-SAN-CLEAN\n");
    return bad;
}
