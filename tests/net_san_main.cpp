// net_san_main.cpp -- TEST-ONLY stand-alone program: the ppg_net_forward / ppg_net_backward kernel source (predpreygrass_amd/csrc/
// ppg_net.h) under the CPU wave emulator, built with -fsanitize=address,undefined by tests/test_net_sanitized.py.  Every workgroup
// (four wavefronts) gets exactly the LDS the HIP launch passes (two buffers of TS samples of the widest layer; the emulator poisons the
// bytes behind it), and every tensor is a heap block of exactly its stated size -- [capacity][C][R][R] observations, [M] index, [M][A]
// out and grad_out, [M][ws_row] workspace, [G][n_params] partial, one block per parameter and per gradient -- so a slot word that
// escaped its range check, a tap outside the image or any other access outside a tensor traps.  The outputs are compared with a scalar
// float64 restatement of the network (measure and bound of tests/net_cases.py: max|x - ref| / max|ref| <= 1e-4 per tensor; rows that
// are selections: +0.0 bits).  The two smallest networks of the cases, the shapes of M around a tile and several tiles per workgroup,
// invalid slots (-1, capacity, INT32_MIN, INT32_MAX) mixed in with NaN in their grad_out rows.  Exit status 0 = clean and within the bound.
#include "wave_emu/san_main.h"

#include "../predpreygrass_amd/csrc/ppg_net.h"

constexpr uint64_t SEED = 0x9E3779B97F4A7C15ull;

struct Net {
    int R, C, hwc, nhwc, A;
    std::vector<int> conv;
};

struct Layout {
    int IH, IW, P, CIN, S, ws_row, n_params, TS;
    std::vector<int> ch, ws_off, p_off;
};

static ppg_policy_spec spec_of(const Net &n) {
    ppg_policy_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.obs_channels = n.C; sp.obs_range = n.R; sp.n_actions = n.A;
    sp.layout = n.hwc ? PPG_POLICY_LAYOUT_HWC : PPG_POLICY_LAYOUT_CHW;
    sp.flatten = n.nhwc ? PPG_POLICY_FLATTEN_NHWC : PPG_POLICY_FLATTEN_NCHW;
    sp.n_conv = (int)n.conv.size();
    for (int l = 0; l < sp.n_conv; ++l) sp.conv_out[l] = n.conv[(size_t)l];
    sp.n_fc = 1; sp.fc_out[0] = n.A;
    return sp;
}

// the geometry the host layer launches with (ppg::net_layout), in the reference's terms
static Layout layout_of(const Net &n) {
    ppg::NetParams K;
    memset(&K, 0, sizeof K);
    ppg::net_layout(spec_of(n), 1, 0, K);
    Layout L;
    L.IH = K.IH; L.IW = K.IW; L.P = K.P; L.CIN = K.conv_c[0]; L.S = K.S; L.ws_row = K.ws_row; L.n_params = K.n_params; L.TS = K.TS;
    for (int l = 0; l <= K.n_conv; ++l) L.ch.push_back(K.conv_c[l]);
    for (int l = 0; l < K.n_conv; ++l) L.ws_off.push_back(K.ws_off[l]);
    for (int q = 0; q <= K.n_seg; ++q) L.p_off.push_back(K.p_off[q]);
    return L;
}

// the network in float64 over the valid rows: out [M][A] and the flat gradients
static void reference(const Net &n, const Layout &L, const std::vector<std::vector<float>> &par, const std::vector<float> &obs, int64_t capacity,
                      const std::vector<int32_t> &index, bool has_index, int64_t M, const std::vector<float> &grad_out, std::vector<double> &out,
                      std::vector<double> &grads) {
    const int P = L.P, IW = L.IW, IH = L.IH, nc = (int)n.conv.size(), flat = L.ch.back() * P;
    out.assign((size_t)M * n.A, 0.0);
    grads.assign((size_t)L.n_params, 0.0);
    for (int64_t i = 0; i < M; ++i) {
        const int64_t k = has_index ? index[(size_t)i] : i;
        if (k < 0 || k >= capacity) continue;
        std::vector<std::vector<double>> act((size_t)nc + 1);
        act[0].resize((size_t)L.CIN * P);
        for (int c = 0; c < L.CIN; ++c)
            for (int p = 0; p < P; ++p)
                act[0][(size_t)c * P + p] = (double)obs[(size_t)k * L.CIN * P + (n.hwc ? (size_t)p * L.CIN + c : (size_t)c * P + p)];
        for (int l = 0; l < nc; ++l) {
            const int ci_n = L.ch[(size_t)l], co_n = L.ch[(size_t)l + 1];
            act[(size_t)l + 1].assign((size_t)co_n * P, 0.0);
            for (int co = 0; co < co_n; ++co)
                for (int h = 0; h < IH; ++h)
                    for (int w = 0; w < IW; ++w) {
                        double a = (double)par[(size_t)2 * l + 1][(size_t)co];
                        for (int ci = 0; ci < ci_n; ++ci)
                            for (int ky = 0; ky < 3; ++ky)
                                for (int kx = 0; kx < 3; ++kx) {
                                    const int hh = h + ky - 1, ww = w + kx - 1;
                                    if (hh < 0 || hh >= IH || ww < 0 || ww >= IW) continue;
                                    a += (double)par[(size_t)2 * l][((size_t)co * ci_n + ci) * 9 + ky * 3 + kx] * act[(size_t)l][(size_t)ci * P + hh * IW + ww];
                                }
                        act[(size_t)l + 1][(size_t)co * P + h * IW + w] = a > 0.0 ? a : 0.0;
                    }
        }
        const int C_last = L.ch.back();
        auto feature = [&](int idx) { return n.nhwc ? (idx % P) * C_last + idx / P : idx; };   // idx = c * P + p
        const std::vector<float> &fw = par[(size_t)2 * nc], &fb = par[(size_t)2 * nc + 1];
        std::vector<double> dflat((size_t)flat, 0.0);
        for (int o = 0; o < n.A; ++o) {
            double a = (double)fb[(size_t)o];
            for (int idx = 0; idx < flat; ++idx) a += (double)fw[(size_t)o * flat + feature(idx)] * act[(size_t)nc][(size_t)idx];
            out[(size_t)i * n.A + o] = a;
            const double g = (double)grad_out[(size_t)i * n.A + o];
            grads[(size_t)L.p_off[(size_t)2 * nc + 1] + o] += g;
            for (int idx = 0; idx < flat; ++idx) {
                grads[(size_t)L.p_off[(size_t)2 * nc] + (size_t)o * flat + feature(idx)] += g * act[(size_t)nc][(size_t)idx];
                dflat[(size_t)idx] += g * (double)fw[(size_t)o * flat + feature(idx)];
            }
        }
        std::vector<double> d = dflat;
        for (int l = nc - 1; l >= 0; --l) {
            const int ci_n = L.ch[(size_t)l], co_n = L.ch[(size_t)l + 1];
            for (size_t e = 0; e < d.size(); ++e)
                if (!(act[(size_t)l + 1][e] > 0.0)) d[e] = 0.0;
            std::vector<double> dx((size_t)ci_n * P, 0.0);
            for (int co = 0; co < co_n; ++co)
                for (int h = 0; h < IH; ++h)
                    for (int w = 0; w < IW; ++w) {
                        const double g = d[(size_t)co * P + h * IW + w];
                        grads[(size_t)L.p_off[(size_t)2 * l + 1] + co] += g;
                        for (int ci = 0; ci < ci_n; ++ci)
                            for (int ky = 0; ky < 3; ++ky)
                                for (int kx = 0; kx < 3; ++kx) {
                                    const int hh = h + ky - 1, ww = w + kx - 1;
                                    if (hh < 0 || hh >= IH || ww < 0 || ww >= IW) continue;
                                    const size_t wi = ((size_t)co * ci_n + ci) * 9 + ky * 3 + kx;
                                    grads[(size_t)L.p_off[(size_t)2 * l] + wi] += g * act[(size_t)l][(size_t)ci * P + hh * IW + ww];
                                    dx[(size_t)ci * P + hh * IW + ww] += g * (double)par[(size_t)2 * l][wi];
                                }
                    }
            d = dx;
        }
    }
}

static int compare(const char *tag, const char *what, const float *got, const double *want, size_t n) {
    double worst = 0.0, top = 0.0;
    for (size_t e = 0; e < n; ++e) {
        const double diff = fabs((double)got[e] - want[e]);
        if (!(diff <= worst)) worst = diff;   // (a NaN sticks)
        if (fabs(want[e]) > top) top = fabs(want[e]);
    }
    if (top == 0.0 ? worst != 0.0 : !(worst / top <= 1e-4)) {
        fprintf(stderr, "%s: %s differs: max|x - ref| = %g, max|ref| = %g\n", tag, what, worst, top);
        return 1;
    }
    return 0;
}

static int run(const Net &n, int64_t M, int groups, bool has_index, bool invalid, const char *tag) {
    const Layout L = layout_of(n);
    const int nc = (int)n.conv.size(), n_seg = 2 * (nc + 1), row = L.CIN * L.P;
    const int64_t capacity = 23;
    std::vector<float> obs((size_t)capacity * row);
    for (float &x : obs) x = below(10) < 3 ? (float)(1 + below(256)) / 64.0f : 0.0f;
    std::vector<std::vector<float>> par((size_t)n_seg), grad((size_t)n_seg);
    for (int q = 0; q < n_seg; ++q) {
        par[(size_t)q].resize((size_t)(L.p_off[(size_t)q + 1] - L.p_off[(size_t)q]));
        grad[(size_t)q].assign(par[(size_t)q].size(), 7.0f);
        for (float &x : par[(size_t)q]) x = uniform(-0.6f, 0.6f);
    }
    if (!has_index && M > capacity) return 0;
    std::vector<int32_t> index(has_index ? (size_t)M : 0);
    std::vector<float> grad_out((size_t)M * n.A);
    for (float &x : grad_out) x = uniform(-1.0f, 1.0f);
    std::vector<uint8_t> bad((size_t)M, 0);
    for (int64_t i = 0; i < M; ++i) {
        if (!has_index) continue;
        index[(size_t)i] = below((int)capacity);
        if (invalid && below(3) == 0) {
            static const int32_t out_of_range[4] = {-1, 0, INT32_MIN, INT32_MAX};
            const int w = below(4);
            index[(size_t)i] = w == 1 ? (int32_t)capacity : out_of_range[w];
            bad[(size_t)i] = 1;
            for (int o = 0; o < n.A; ++o) grad_out[(size_t)i * n.A + o] = NAN;
        }
    }
    ppg::NetParams K;
    memset(&K, 0, sizeof K);
    const size_t lds = (size_t)ppg::net_layout(spec_of(n), M, groups, K);   // geometry, TS, tiles, G and the LDS exactly as the host layer launches
    const int G = K.G;
    std::vector<float> out((size_t)M * n.A, 7.0f), workspace((size_t)M * L.ws_row, 7.0f), partial((size_t)G * L.n_params, NAN);
    K.capacity = capacity; K.obs_dtype = 1;
    K.obs = obs.data(); K.index = has_index ? index.data() : nullptr;
    for (int l = 0; l < nc; ++l) { K.conv_w[l] = par[(size_t)2 * l].data(); K.conv_b[l] = par[(size_t)2 * l + 1].data(); }
    K.fc_w[0] = par[(size_t)2 * nc].data(); K.fc_b[0] = par[(size_t)2 * nc + 1].data();
    K.out = out.data(); K.workspace = workspace.data(); K.grad_out = grad_out.data(); K.partial = partial.data();
    for (int q = 0; q < n_seg; ++q) K.grad[q] = grad[(size_t)q].data();
    for (int b = 0; b < G; ++b)
        wv::run_block([](void *arg) { ppg::net_forward_main(*(const ppg::NetParams *)arg, wv::emu().lds); }, (void *)&K, b, lds, ppg::NET_WAVES);
    for (int b = 0; b < G; ++b)
        wv::run_block([](void *arg) { ppg::net_backward_main(*(const ppg::NetParams *)arg, wv::emu().lds); }, (void *)&K, b, lds, ppg::NET_WAVES);
    for (int b = 0; b < (L.n_params + ppg::NET_THREADS - 1) / ppg::NET_THREADS; ++b)
        wv::run_block([](void *arg) { ppg::net_reduce_main(*(const ppg::NetParams *)arg); }, (void *)&K, b, 16, ppg::NET_WAVES);
    std::vector<double> want_out, want_grads;
    reference(n, L, par, obs, capacity, index, has_index, M, grad_out, want_out, want_grads);
    int fail = compare(tag, "out", out.data(), want_out.data(), out.size());
    for (int q = 0; q < n_seg; ++q) {
        char what[32];
        snprintf(what, sizeof what, "gradient tensor %d", q);
        fail |= compare(tag, what, grad[(size_t)q].data(), want_grads.data() + L.p_off[(size_t)q], grad[(size_t)q].size());
    }
    for (int64_t i = 0; i < M; ++i)
        for (int o = 0; o < n.A && bad[(size_t)i]; ++o) {
            uint32_t bits;
            memcpy(&bits, &out[(size_t)i * n.A + o], 4);
            if (bits != 0) { fprintf(stderr, "%s: out of invalid row %lld is not +0.0\n", tag, (long long)i); fail = 1; }
        }
    return fail;
}

int main() {
    lcg_seed(SEED);
    const Net nets[2] = {{5, 4, 1, 1, 3, {8}}, {5, 5, 0, 0, 9, {8, 16}}};
    int bad = 0;
    char tag[128];
    for (const Net &n : nets) {
        const int TS = layout_of(n).TS;
        const int64_t shapes[6][2] = {{1, 0}, {TS - 1, 0}, {TS, 0}, {TS + 1, 0}, {2 * TS + 3, 0}, {5 * TS + 1, 2}};
        for (const auto &sh : shapes)
            for (int mode = 0; mode < 3; ++mode) {   // no index | a permutation with repeats | invalid slots mixed in
                if (sh[0] < 1) continue;
                snprintf(tag, sizeof tag, "R=%d C=%d convs=%zu A=%d M=%lld groups=%lld mode=%d", n.R, n.C, n.conv.size(), n.A, (long long)sh[0],
                         (long long)sh[1], mode);
                bad |= run(n, sh[0], (int)sh[1], mode > 0, mode == 2, tag);
            }
    }
    if (!bad) printf("NET-SAN-CLEAN\n");
    return bad;
}
