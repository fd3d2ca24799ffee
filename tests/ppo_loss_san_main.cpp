// ppo_loss_san_main.cpp -- TEST-ONLY stand-alone program: the ppg_ppo_loss kernel source (predpreygrass_amd/csrc/ppg_ppo.h) under the
// CPU wave emulator, built with -fsanitize=address,undefined by tests/test_ppo_loss_sanitized.py.  Every workgroup gets exactly the LDS
// the HIP launch declares (ppg::PPO_LDS_BYTES; the emulator poisons the bytes behind it), and every tensor is a heap block of exactly
// its stated size -- [M] index, [M,A] logits and gradients, [capacity] columns, [capacity,A] dist, [G,8] partial -- so a slot word or an
// action that escaped its range check, or any other access outside a tensor, traps.  The outputs are compared with a scalar
// restatement of include/ppg.h (this program's libm on both sides: bit for bit).  Shapes: the chunk edges and a partial wave, with
// every kind of invalid row mixed in.  Exit status 0 = clean and equal.
#include "wave_emu/san_main.h"

#include "../predpreygrass_amd/csrc/ppg_ppo.h"

constexpr uint64_t SEED = 0x9E3779B97F4A7C15ull;

struct Case {
    int64_t M, capacity;
    int A;
    bool has_index, has_values, has_dist, has_norm;
    std::vector<int32_t> index;
    std::vector<float> logits, values, logp, dist, advantage, target;
    std::vector<int8_t> action;
    double norm[2];
};

static float gauss() { return (float)((unit() + unit() + unit() + unit() - 2.0) * 1.7); }

// Columns of M + 4 slots (without an index: M), the last four invalid by their columns when there is an index; about a sixth of the
// rows invalid: index -1, INT32_MIN, capacity, INT32_MAX, or a slot whose action is PPG_ACTION_UNSET / A / -1 or whose logp is NaN /
// -inf.  The logits rows of invalid rows and the other columns of invalid slots are NaN.  Some valid rows carry a -inf logit.
static Case make_case(int64_t M, int A, bool has_index, bool has_values, bool has_dist, bool has_norm) {
    Case c;
    c.M = M; c.A = A; c.has_index = has_index; c.has_values = has_values; c.has_dist = has_dist; c.has_norm = has_norm;
    c.capacity = has_index ? M + 4 : M;
    const size_t cap = (size_t)c.capacity;
    c.logits.resize((size_t)M * A); c.values.resize((size_t)M); c.index.resize(has_index ? (size_t)M : 0);
    c.logp.resize(cap); c.dist.resize(cap * A); c.advantage.resize(cap); c.target.resize(cap); c.action.resize(cap);
    for (size_t k = 0; k < cap; ++k) {
        c.action[k] = (int8_t)below(A);
        c.logp[k] = -(float)(unit() * 3.0) - 0.01f;
        c.advantage[k] = gauss();
        c.target[k] = gauss();
        for (int a = 0; a < A; ++a) c.dist[k * A + a] = gauss();
        if (A > 1 && below(9) == 0) c.dist[k * A + below(A)] = -INFINITY;
    }
    auto spoil = [&](size_t k, int kind) {
        if (kind == 0) c.action[k] = PPG_ACTION_UNSET;
        else if (kind == 1) c.action[k] = (int8_t)A;
        else if (kind == 2) c.action[k] = -1;
        else if (kind == 3) c.logp[k] = NAN;
        else c.logp[k] = -INFINITY;
        c.advantage[k] = c.target[k] = NAN;
        for (int a = 0; a < A; ++a) c.dist[k * A + a] = NAN;
    };
    if (has_index) for (int q = 0; q < 4; ++q) spoil((size_t)M + q, q + 1);
    for (int64_t i = 0; i < M; ++i) {
        int64_t k = has_index ? below((int)M) : i;
        bool bad = below(6) == 0;
        if (bad) {
            if (has_index) {
                static const int32_t out[4] = {-1, INT32_MIN, 0, INT32_MAX};
                const int w = below(8);
                k = w < 4 ? (w == 2 ? c.capacity : out[w]) : M + (w - 4);
            } else {
                spoil((size_t)i, below(5));
            }
        }
        if (has_index) c.index[(size_t)i] = (int32_t)k;
        for (int a = 0; a < A; ++a) c.logits[(size_t)i * A + a] = bad ? NAN : (k >= 0 && k < (int64_t)cap ? c.dist[(size_t)k * A + a] : 0.0f) + 0.3f * gauss();
        if (!bad && A > 1 && below(9) == 0) c.logits[(size_t)i * A + below(A)] = -INFINITY;
        c.values[(size_t)i] = bad ? NAN : gauss() * 2.5f;
    }
    c.norm[0] = 0.1; c.norm[1] = 1.3;
    return c;
}

struct Out {
    std::vector<float> gl, gv;
    std::vector<double> partial;
};

static const double CLIP = 0.3, VF_CLIP = 10.0, VF_COEFF = 0.5, ENT = 0.01, KLC = 0.2;

static void softmax_row(const float *row, int A, double *d, double *lp, double *p) {
    double m = -INFINITY;
    for (int c = 0; c < A; ++c) if ((double)row[c] > m) m = (double)row[c];
    double s = 0.0;
    for (int c = 0; c < A; ++c) {
        d[c] = (double)row[c] - m;
        p[c] = d[c] == -INFINITY ? 0.0 : exp(d[c]);
        if (d[c] != -INFINITY) s = s + p[c];
    }
    const double ls = log(s);
    for (int c = 0; c < A; ++c) { lp[c] = d[c] - ls; p[c] = p[c] / s; }
}

// the scalar reference: include/ppg.h row by row, then partial in lane order and through the butterfly
static void reference(const Case &c, Out &w) {
    const int A = c.A;
    const int64_t M = c.M, G = (M + ppg::PPO_CHUNK - 1) / ppg::PPO_CHUNK;
    std::vector<uint8_t> valid((size_t)M);
    std::vector<int64_t> slot((size_t)M);
    double n = 0.0;
    for (int64_t i = 0; i < M; ++i) {
        const int64_t k = c.has_index ? c.index[(size_t)i] : i;
        bool ok = k >= 0 && k < c.capacity;
        if (ok) ok = c.action[(size_t)k] >= 0 && c.action[(size_t)k] < A && std::isfinite(c.logp[(size_t)k]);
        valid[(size_t)i] = ok; slot[(size_t)i] = ok ? k : 0;
        if (ok) n = n + 1.0;
    }
    const double wgt = n > 0.0 ? 1.0 / n : 0.0;
    w.gl.assign((size_t)M * A, 0.0f); w.gv.assign(c.has_values ? (size_t)M : 0, 0.0f); w.partial.assign((size_t)G * 8, 0.0);
    std::vector<double> col((size_t)M * 8, 0.0);
    for (int64_t i = 0; i < M; ++i) {
        if (!valid[(size_t)i]) continue;
        const size_t k = (size_t)slot[(size_t)i];
        const int a = c.action[k];
        double d[32], lp[32], p[32], dq[32], lq[32], q[32];
        softmax_row(&c.logits[(size_t)i * A], A, d, lp, p);
        if (c.has_dist) softmax_row(&c.dist[k * A], A, dq, lq, q);
        double hsum = 0.0, kl = 0.0;
        for (int x = 0; x < A; ++x) {
            if (d[x] != -INFINITY) { const double t = p[x] * lp[x]; hsum = hsum + t; }
            if (c.has_dist && q[x] != 0.0) { const double diff = lq[x] - lp[x]; const double t = q[x] * diff; kl = kl + t; }
        }
        const double H = 0.0 - hsum;
        const double r = exp(lp[a] - (double)c.logp[k]);
        double adv = (double)c.advantage[k];
        if (c.has_norm) { const double centred = adv - c.norm[0]; adv = centred * c.norm[1]; }
        const double lo = 1.0 - CLIP, hi = 1.0 + CLIP;
        const double rc = r < lo ? lo : r > hi ? hi : r;
        const double s1 = adv * r, s2 = adv * rc;
        const bool clipped = s2 < s1;
        const double c1 = clipped ? 0.0 : s1;
        double *o = &col[(size_t)i * 8];
        o[0] = 1.0; o[1] = clipped ? s2 : s1; o[4] = H; o[5] = kl; o[6] = clipped ? 1.0 : 0.0; o[7] = (double)c.logp[k] - lp[a];
        if (c.has_values) {
            const double e = (double)c.values[(size_t)i] - (double)c.target[k];
            const double vf = e * e;
            const bool over = vf > VF_CLIP;
            o[2] = over ? VF_CLIP : vf; o[3] = vf;
            const double e2 = e + e, gv = VF_COEFF * (over ? 0.0 : e2);
            w.gv[(size_t)i] = (float)(wgt * gv);
        }
        for (int x = 0; x < A; ++x) {
            if (d[x] == -INFINITY) continue;
            const double lh = lp[x] + H, plh = p[x] * lh, te = ENT * plh;
            const double delta = (x == a ? 1.0 : 0.0) - p[x], ts = c1 * delta;
            double y = te - ts;
            if (c.has_dist) { const double pq = p[x] - q[x]; const double tk = KLC * pq; y = y + tk; }
            w.gl[(size_t)i * A + x] = (float)(wgt * y);
        }
    }
    for (int64_t g = 0; g < G; ++g)
        for (int x = 0; x < 8; ++x) {
            double acc[64] = {};
            for (int j = 0; j < ppg::PPO_CHUNK / 64; ++j)
                for (int l = 0; l < 64; ++l) {
                    const int64_t i = g * ppg::PPO_CHUNK + 64 * j + l;
                    if (i < M && valid[(size_t)i]) acc[l] = acc[l] + col[(size_t)i * 8 + x];
                }
            for (int m = 1; m < 64; m <<= 1) {
                double next[64];
                for (int l = 0; l < 64; ++l) next[l] = acc[l] + acc[l ^ m];
                memcpy(acc, next, sizeof next);
            }
            w.partial[(size_t)g * 8 + x] = acc[0];
        }
}

static int run(const Case &c, const char *tag) {
    Out got, want;
    const int64_t G = (c.M + ppg::PPO_CHUNK - 1) / ppg::PPO_CHUNK;
    got.gl.assign((size_t)c.M * c.A, 7.0f); got.gv.assign(c.has_values ? (size_t)c.M : 0, 7.0f); got.partial.assign((size_t)G * 8, 7.0);
    ppg::PpoParams K;
    memset(&K, 0, sizeof K);
    K.M = c.M; K.capacity = c.capacity; K.A = c.A; K.G = (int32_t)G;
    K.index = c.has_index ? c.index.data() : nullptr;
    K.logits = c.logits.data();
    K.values = c.has_values ? c.values.data() : nullptr;
    K.action = c.action.data(); K.logp = c.logp.data();
    K.dist = c.has_dist ? c.dist.data() : nullptr;
    K.advantage = c.advantage.data();
    K.value_target = c.has_values ? c.target.data() : nullptr;
    K.adv_norm = c.has_norm ? c.norm : nullptr;
    K.clip_lo = 1.0 - CLIP; K.clip_hi = 1.0 + CLIP; K.vf_clip = VF_CLIP; K.vf_coeff = VF_COEFF; K.ent_coeff = ENT; K.kl_coeff = c.has_dist ? KLC : 0.0;
    K.grad_logits = got.gl.data(); K.grad_values = c.has_values ? got.gv.data() : nullptr; K.partial = got.partial.data();
    run_grid<ppg::PpoParams, ppg::ppo_count_main>(K, (int)G);
    run_grid<ppg::PpoParams, ppg::ppo_rows_main, ppg::PPO_LDS_BYTES>(K, (int)G);
    reference(c, want);
    int bad = 0;
    if (memcmp(got.gl.data(), want.gl.data(), got.gl.size() * 4) != 0) { fprintf(stderr, "%s: grad_logits differ\n", tag); bad = 1; }
    if (got.gv.size() && memcmp(got.gv.data(), want.gv.data(), got.gv.size() * 4) != 0) { fprintf(stderr, "%s: grad_values differ\n", tag); bad = 1; }
    if (memcmp(got.partial.data(), want.partial.data(), got.partial.size() * 8) != 0) { fprintf(stderr, "%s: partial differs\n", tag); bad = 1; }
    double n = 0.0;
    for (int64_t g = 0; g < G; ++g) n += got.partial[(size_t)g * 8];
    if (!(n > 0.0 && n < (double)c.M) && c.M > 8) { fprintf(stderr, "%s: %g of %lld rows valid\n", tag, n, (long long)c.M); bad = 1; }
    return bad;
}

int main() {
    lcg_seed(SEED);
    int bad = 0, q = 0;
    char tag[128];
    for (int64_t M : {1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 7})
        for (int A : {1, 9, 32}) {
            ++q;
            const bool has_index = q % 2 != 0, has_values = q % 3 != 0, has_dist = q % 5 != 0, has_norm = q % 4 < 2;
            snprintf(tag, sizeof tag, "M=%lld A=%d index=%d values=%d dist=%d norm=%d", (long long)M, A, has_index, has_values, has_dist, has_norm);
            bad |= run(make_case(M, A, has_index, has_values, has_dist, has_norm), tag);
        }
    if (!bad) printf("PPO-LOSS-SAN-CLEAN\n");
    return bad;
}
