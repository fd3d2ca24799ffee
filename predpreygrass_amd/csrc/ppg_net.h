// ppg_net.h -- ppg_net_forward / ppg_net_backward of include/ppg.h: a float32 forward and backward pass of a PolicyNet (L x [zero pad 1,
// conv 3x3, ReLU], flatten, Linear layers) over a minibatch of rows gathered from a dense [capacity][C][R][R] observation tensor through
// an int32 slot index, with the weights read where the optimiser keeps them (float32, PyTorch layouts, no packed copy).
//
// Three kernels of NET_THREADS = 256 threads (four wavefronts), written against the wave primitives of wave.h (the CPU test build runs
// the same source).  Workgroups are persistent: workgroup g of G takes the tiles g, g + G, ... of TS <= 4 minibatch rows each.
//   net_forward   gathers the tile's rows into LDS (float64 / bfloat16 converted as obs.to(float32) does), runs every layer with the
//                 tile's activations in two LDS buffers (input | output, swapped per layer), stores every post-ReLU activation into
//                 the caller's workspace [M][ws_row] and the last layer's output into out[M][n_out].
//   net_backward  stages grad_out and, layer by layer from the last, the layer's input (workspace, or the gathered rows for the first
//                 convolution) into the two buffers; a thread OWNS the parameters j = t, t + 256, ... of the layer: it forms the tile's
//                 contribution as one fmaf chain (samples ascending, then positions ascending) and adds it to partial[g][j] -- the
//                 first tile of a workgroup stores, later ones add, so `partial` needs no initial value and a row is touched by one
//                 thread only.  Then the input gradient replaces the staged input in place, selected by input > 0 (ReLU).
//   net_reduce    grads[j] = partial[0][j] + partial[1][j] + ... in ascending g, written per tensor in PyTorch layout.
// Inner products are v_fma_f32 chains (fmaf on purpose: the library is built with -ffp-contract=off); the fully connected layers'
// forward chains are split over the 64 lanes of a wavefront (feature f = lane, lane + 64, ...) and combined by an xor butterfly.  No
// atomics: for a given M and G the same bits from run to run.  The per-sample accumulators are a four-element array under a fully
// unrolled loop, indexed by constants only (no scratch); everything indexed at run time lives in LDS or in the parameter block.
// A slot number becomes an address only after 0 <= k < capacity was checked.  A row whose slot is outside is a selection: nothing of
// it is read (not its observation, not its grad_out row), its out row is +0.0, and it takes part in no chain.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "ppg_rows.h"

namespace ppg {

constexpr int NET_WAVES = 4;
constexpr int NET_THREADS = 64 * NET_WAVES;
constexpr int NET_TS_MAX = 4;                  // samples of a tile (the unrolled accumulators)
constexpr int NET_MAX_GROUPS = 1024;           // rows of partial
constexpr int NET_MAX_SEGMENTS = 2 * (PPG_POLICY_MAX_CONV + PPG_POLICY_MAX_FC);   // parameter tensors

struct NetParams {
    int64_t M;                  // 1 .. 2^24 (the host checks)
    int64_t capacity;           // 0 .. INT32_MAX
    int32_t G, TS, n_tiles;     // workgroups, samples per tile, ceil(M / TS)
    int32_t obs_dtype;          // 0 float64, 1 float32, 2 bfloat16
    int32_t hwc, flatten_nhwc;
    int32_t IH, IW, P, n_conv, n_fc;
    int32_t conv_c[PPG_POLICY_MAX_CONV + 1];   // channels: [0] of the image, [l + 1] out of convolution l
    int32_t fc_d[PPG_POLICY_MAX_FC + 1];       // widths: [0] the flattened features, [l + 1] out of linear layer l
    int32_t S;                  // floats of one sample in an LDS buffer: the widest layer
    int32_t ws_row;             // floats of one row of the workspace
    int32_t ws_off[PPG_POLICY_MAX_CONV + PPG_POLICY_MAX_FC];   // convolution l at [l], hidden layer l at [n_conv + l]
    int32_t n_params, n_seg;
    int32_t p_off[NET_MAX_SEGMENTS + 1];       // flat parameter order: conv l weight 2 l, bias 2 l + 1, fc l weight 2 (n_conv + l), bias + 1
    const void *obs;            // [capacity][C][R][R]
    const int32_t *index;       // [M] or NULL: k = i
    const float *conv_w[PPG_POLICY_MAX_CONV], *conv_b[PPG_POLICY_MAX_CONV];
    const float *fc_w[PPG_POLICY_MAX_FC], *fc_b[PPG_POLICY_MAX_FC];
    float *out;                 // [M][n_out]           (forward)
    float *workspace;           // [M][ws_row]
    const float *grad_out;      // [M][n_out]           (backward)
    float *partial;             // [G][n_params]
    float *grad[NET_MAX_SEGMENTS];             // per tensor, in the flat order (reduce)
};

// ---- the geometry a network's shape decides, device-free (the host layer and the stand-alone test program share it) ---------------------
// sp: a spec the shape rules accept (ppg_policy_shape.h); 1 <= M; groups >= 0 (0: automatic).  Fills K's geometry, workspace and parameter
// layout, TS, the tiles and G -- no pointer -- and returns the dynamic LDS bytes of a workgroup: two buffers of TS samples of the widest layer.
static inline int net_layout(const ppg_policy_spec &sp, int64_t M, int32_t groups, NetParams &K) {
    const int R = sp.obs_range, C = sp.obs_channels, hwc = sp.layout == PPG_POLICY_LAYOUT_HWC;
    K.hwc = hwc; K.flatten_nhwc = sp.flatten == PPG_POLICY_FLATTEN_NHWC;
    K.IH = hwc ? C : R; K.IW = R; K.P = K.IH * K.IW;
    K.n_conv = sp.n_conv; K.n_fc = sp.n_fc;
    K.conv_c[0] = hwc ? R : C;
    int S = K.conv_c[0] * K.P, ws = 0, np = 0, seg = 0;
    for (int l = 0; l < sp.n_conv; ++l) {
        K.conv_c[l + 1] = sp.conv_out[l];
        const int n = sp.conv_out[l] * K.P;
        if (n > S) S = n;
        K.ws_off[l] = ws; ws += n;
        K.p_off[seg++] = np; np += sp.conv_out[l] * K.conv_c[l] * 9;
        K.p_off[seg++] = np; np += sp.conv_out[l];
    }
    K.fc_d[0] = K.conv_c[sp.n_conv] * K.P;
    for (int l = 0; l < sp.n_fc; ++l) {
        K.fc_d[l + 1] = sp.fc_out[l];
        if (sp.fc_out[l] > S) S = sp.fc_out[l];
        if (l + 1 < sp.n_fc) { K.ws_off[sp.n_conv + l] = ws; ws += sp.fc_out[l]; }
        K.p_off[seg++] = np; np += sp.fc_out[l] * K.fc_d[l];
        K.p_off[seg++] = np; np += sp.fc_out[l];
    }
    K.p_off[seg] = np;
    K.S = S; K.ws_row = ws; K.n_params = np; K.n_seg = seg;
    // two buffers of TS samples: the largest TS within 80 KB (two workgroups per CU), else one sample in whatever it takes (<= 115 KB)
    const int budget = 80 * 1024;
    K.TS = 2 * 4 * S * 4 <= budget ? 4 : 2 * 2 * S * 4 <= budget ? 2 : 1;
    K.M = M;
    K.n_tiles = (int32_t)((M + K.TS - 1) / K.TS);
    const int g_max = K.n_tiles < NET_MAX_GROUPS ? K.n_tiles : NET_MAX_GROUPS;
    K.G = groups && groups < g_max ? groups : g_max;
    return 2 * K.TS * S * 4;
}

PPG_DEVICE int net_thread() { return wv::wave_index() * 64 + wv::lane(); }

PPG_DEVICE float net_wave_sum(float x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = x + (float)wv::shfl_xor_f64((double)x, m);   // (float -> double -> float: exact)
    return x;
}

// the slot of minibatch row i, or -1: the row is a selection only
template <class KP>
PPG_DEVICE int64_t net_slot(const KP &K, int64_t i) {
    const int64_t k = K.index ? (int64_t)K.index[i] : i;
    return (k < 0 || k >= K.capacity) ? -1 : k;
}

// bit s set: sample s of the tile is a row of the minibatch with a slot inside the store
template <class KP>
PPG_DEVICE int net_tile_mask(const KP &K, int tile) {
    int vmask = 0;
#pragma unroll
    for (int s = 0; s < NET_TS_MAX; ++s) {
        const int64_t i = (int64_t)tile * K.TS + s;
        if (s < K.TS && i < K.M && net_slot(K, i) >= 0) vmask |= 1 << s;
    }
    return vmask;
}

// the tile's observation rows -> X[s][channel][position], converted to float32
template <class KP>
PPG_DEVICE void net_gather(const KP &K, int tile, int vmask, float *X, int t) {
    const int CIN = K.conv_c[0], P = K.P, n = CIN * P;
#pragma unroll
    for (int s = 0; s < NET_TS_MAX; ++s) {
        if (!(vmask >> s & 1)) continue;
        const int64_t k = net_slot(K, (int64_t)tile * K.TS + s);
        const size_t base = (size_t)k * (size_t)n;
        for (int e = t; e < n; e += NET_THREADS) {
            float v;
            if (K.obs_dtype == 0) v = (float)((const double *)K.obs)[base + e];
            else if (K.obs_dtype == 1) v = ((const float *)K.obs)[base + e];
            else {
                const uint32_t bits = (uint32_t)((const uint16_t *)K.obs)[base + e] << 16;
                memcpy(&v, &bits, 4);
            }
            // memory order: channels-last rows are [position][channel], channel-first ones [channel][position]
            const int c = K.hwc ? e % CIN : e / P, p = K.hwc ? e / CIN : e % P;
            X[s * K.S + c * P + p] = v;
        }
    }
}

// bit ky * 3 + kx set: the tap (h + ky - 1, w + kx - 1) lies inside the image
PPG_DEVICE int net_tap_mask(int h, int w, int IH, int IW) {
    int m = 0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int hh = h + ky - 1, ww = w + kx - 1;
            if (hh >= 0 && hh < IH && ww >= 0 && ww < IW) m |= 1 << (ky * 3 + kx);
        }
    return m;
}

// the feature of the first linear layer that element idx = c * P + p of the last convolution's output is
template <class KP>
PPG_DEVICE int net_lds_index(const KP &K, int layer, int f) {
    if (layer != 0 || !K.flatten_nhwc) return f;
    const int C = K.conv_c[K.n_conv];
    return (f % C) * K.P + f / C;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
template <class KP>
PPG_DEVICE void net_forward_main(const KP &K, unsigned char *lds) {
    const int g = PPG_BLOCK_INDEX();
    if (g >= K.G) return;
    const int t = net_thread(), P = K.P, IW = K.IW, IH = K.IH, S = K.S;
    const int n_out = K.fc_d[K.n_fc];
    float *X = (float *)lds, *Y = X + K.TS * S;
    for (int tile = g; tile < K.n_tiles; tile += K.G) {
        const int vmask = net_tile_mask(K, tile);
        const int64_t i0 = (int64_t)tile * K.TS;
        // rows that are selections: +0.0
        for (int e = t; e < K.TS * n_out; e += NET_THREADS) {
            const int s = e / n_out;
            if (i0 + s < K.M && !(vmask >> s & 1)) K.out[(size_t)(i0 + s) * n_out + (e - s * n_out)] = 0.0f;
        }
        net_gather(K, tile, vmask, X, t);
        wv::wg_barrier();
        for (int l = 0; l < K.n_conv; ++l) {
            const int Cin = K.conv_c[l], Cout = K.conv_c[l + 1];
            const float *W = K.conv_w[l], *B = K.conv_b[l];
            for (int item = t; item < Cout * P; item += NET_THREADS) {
                const int co = item / P, p = item - co * P, h = p / IW, w = p - h * IW;
                const int taps = net_tap_mask(h, w, IH, IW);
                const float b = B[co];
                float acc[NET_TS_MAX] = {b, b, b, b};
                const float *wrow = W + (size_t)co * Cin * 9;
                for (int ci = 0; ci < Cin; ++ci) {
                    const int xb = ci * P + p - IW - 1;
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        if (!(taps >> tap & 1)) continue;
                        const float wt = wrow[ci * 9 + tap];
                        const int off = (tap / 3) * IW + tap % 3;
#pragma unroll
                        for (int s = 0; s < NET_TS_MAX; ++s)
                            if (vmask >> s & 1) acc[s] = fmaf(wt, X[s * S + xb + off], acc[s]);
                    }
                }
#pragma unroll
                for (int s = 0; s < NET_TS_MAX; ++s) {
                    if (!(vmask >> s & 1)) continue;
                    const float y = acc[s] > 0.0f ? acc[s] : 0.0f;
                    Y[s * S + item] = y;
                    K.workspace[(size_t)(i0 + s) * K.ws_row + K.ws_off[l] + item] = y;
                }
            }
            wv::wg_barrier();
            float *sw = X; X = Y; Y = sw;
        }
        for (int l = 0; l < K.n_fc; ++l) {
            const int in = K.fc_d[l], out = K.fc_d[l + 1];
            const bool last = l + 1 == K.n_fc;
            const float *W = K.fc_w[l], *B = K.fc_b[l];
            const int ln = wv::lane();
            for (int item = wv::wave_index(); item < K.TS * out; item += NET_WAVES) {   // (wave-uniform: the butterfly is a collective)
                const int s = item / out, o = item - s * out;
                if (!(vmask >> s & 1)) continue;
                float acc = 0.0f;
                for (int f = ln; f < in; f += 64) acc = fmaf(W[(size_t)o * in + f], X[s * S + net_lds_index(K, l, f)], acc);
                acc = net_wave_sum(acc);
                float y = acc + B[o];
                if (!last) y = y > 0.0f ? y : 0.0f;
                if (ln == 0) {
                    Y[s * S + o] = y;
                    if (last) K.out[(size_t)(i0 + s) * n_out + o] = y;
                    else K.workspace[(size_t)(i0 + s) * K.ws_row + K.ws_off[K.n_conv + l] + o] = y;
                }
            }
            wv::wg_barrier();
            float *sw = X; X = Y; Y = sw;
        }
        if ((K.n_conv + K.n_fc) & 1) { float *sw = X; X = Y; Y = sw; }   // (the next tile starts in the first buffer again)
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
// this workgroup's row of partial takes the tile's contribution to parameter j: stored by its first tile, added by the later ones; a
// tile of selections adds nothing (not even +0.0: -0.0 + +0.0 would change a sign bit)
PPG_DEVICE void net_accumulate(float *row, bool first, int vmask, int j, float sum) {
    if (first) row[j] = sum;
    else if (vmask) row[j] = row[j] + sum;
}

// rows of the workspace -> X[s][0 .. n)
template <class KP>
PPG_DEVICE void net_stage(const KP &K, int64_t i0, int vmask, int off, int n, float *X, int t) {
#pragma unroll
    for (int s = 0; s < NET_TS_MAX; ++s) {
        if (!(vmask >> s & 1)) continue;
        const float *src = K.workspace + (size_t)(i0 + s) * K.ws_row + off;
        for (int e = t; e < n; e += NET_THREADS) X[s * K.S + e] = src[e];
    }
}

template <class KP>
PPG_DEVICE void net_backward_main(const KP &K, unsigned char *lds) {
    const int g = PPG_BLOCK_INDEX();
    if (g >= K.G) return;
    const int t = net_thread(), P = K.P, IW = K.IW, IH = K.IH, S = K.S;
    const int n_out = K.fc_d[K.n_fc];
    float *row = K.partial + (size_t)g * K.n_params;
    float *D = (float *)lds, *X = D + K.TS * S;   // the layer's output gradient | its input, then its input gradient
    for (int tile = g; tile < K.n_tiles; tile += K.G) {
        const bool first = tile == g;
        const int vmask = net_tile_mask(K, tile);
        const int64_t i0 = (int64_t)tile * K.TS;
#pragma unroll
        for (int s = 0; s < NET_TS_MAX; ++s)
            if (vmask >> s & 1)
                for (int e = t; e < n_out; e += NET_THREADS) D[s * S + e] = K.grad_out[(size_t)(i0 + s) * n_out + e];
        for (int l = K.n_fc - 1; l >= 0; --l) {
            const int in = K.fc_d[l], out = K.fc_d[l + 1], seg = 2 * (K.n_conv + l);
            const float *W = K.fc_w[l];
            net_stage(K, i0, vmask, l ? K.ws_off[K.n_conv + l - 1] : K.ws_off[K.n_conv - 1], in, X, t);
            wv::wg_barrier();
            for (int j = t; j < out * in; j += NET_THREADS) {
                const int o = j / in, idx = net_lds_index(K, l, j - o * in);
                float sum = 0.0f;
#pragma unroll
                for (int s = 0; s < NET_TS_MAX; ++s)
                    if (vmask >> s & 1) sum = fmaf(D[s * S + o], X[s * S + idx], sum);
                net_accumulate(row, first, vmask, K.p_off[seg] + j, sum);
            }
            for (int o = t; o < out; o += NET_THREADS) {
                float sum = 0.0f;
#pragma unroll
                for (int s = 0; s < NET_TS_MAX; ++s)
                    if (vmask >> s & 1) sum = sum + D[s * S + o];
                net_accumulate(row, first, vmask, K.p_off[seg + 1] + o, sum);
            }
            wv::wg_barrier();
            for (int f = t; f < in; f += NET_THREADS) {
                const int idx = net_lds_index(K, l, f);
                float acc[NET_TS_MAX] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int o = 0; o < out; ++o) {
                    const float wt = W[(size_t)o * in + f];
#pragma unroll
                    for (int s = 0; s < NET_TS_MAX; ++s)
                        if (vmask >> s & 1) acc[s] = fmaf(wt, D[s * S + o], acc[s]);
                }
#pragma unroll
                for (int s = 0; s < NET_TS_MAX; ++s)
                    if (vmask >> s & 1) X[s * S + idx] = X[s * S + idx] > 0.0f ? acc[s] : 0.0f;
            }
            wv::wg_barrier();
            float *sw = D; D = X; X = sw;
        }
        for (int l = K.n_conv - 1; l >= 0; --l) {
            const int Cin = K.conv_c[l], Cout = K.conv_c[l + 1], seg = 2 * l;
            const float *W = K.conv_w[l];
            if (l) net_stage(K, i0, vmask, K.ws_off[l - 1], Cin * P, X, t);
            else net_gather(K, tile, vmask, X, t);
            wv::wg_barrier();
            for (int j = t; j < Cout * Cin * 9; j += NET_THREADS) {
                const int co = j / (Cin * 9), r = j - co * Cin * 9, ci = r / 9, tap = r - ci * 9, ky = tap / 3, kx = tap - ky * 3;
                const int h_lo = ky == 0 ? 1 : 0, h_hi = ky == 2 ? IH - 1 : IH, w_lo = kx == 0 ? 1 : 0, w_hi = kx == 2 ? IW - 1 : IW;
                const int db = co * P, xb = ci * P + (ky - 1) * IW + (kx - 1);
                float sum = 0.0f;
#pragma unroll
                for (int s = 0; s < NET_TS_MAX; ++s) {
                    if (!(vmask >> s & 1)) continue;
                    for (int h = h_lo; h < h_hi; ++h)
                        for (int w = w_lo; w < w_hi; ++w) sum = fmaf(D[s * S + db + h * IW + w], X[s * S + xb + h * IW + w], sum);
                }
                net_accumulate(row, first, vmask, K.p_off[seg] + j, sum);
            }
            for (int co = t; co < Cout; co += NET_THREADS) {
                float sum = 0.0f;
#pragma unroll
                for (int s = 0; s < NET_TS_MAX; ++s) {
                    if (!(vmask >> s & 1)) continue;
                    for (int p = 0; p < P; ++p) sum = sum + D[s * S + co * P + p];
                }
                net_accumulate(row, first, vmask, K.p_off[seg + 1] + co, sum);
            }
            wv::wg_barrier();
            if (l == 0) break;   // (the observation's gradient is nobody's)
            for (int item = t; item < Cin * P; item += NET_THREADS) {
                const int ci = item / P, p = item - ci * P, h = p / IW, w = p - h * IW;
                // output position (h - ky + 1, w - kx + 1) reads this input through tap (ky, kx): inside exactly when the mirrored tap is
                const int taps = net_tap_mask(h, w, IH, IW);
                float acc[NET_TS_MAX] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int co = 0; co < Cout; ++co) {
                    const float *wrow = W + ((size_t)co * Cin + ci) * 9;
                    const int db = co * P + p + IW + 1;
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        if (!(taps >> (8 - tap) & 1)) continue;
                        const float wt = wrow[tap];
                        const int off = (tap / 3) * IW + tap % 3;
#pragma unroll
                        for (int s = 0; s < NET_TS_MAX; ++s)
                            if (vmask >> s & 1) acc[s] = fmaf(wt, D[s * S + db - off], acc[s]);
                    }
                }
#pragma unroll
                for (int s = 0; s < NET_TS_MAX; ++s)
                    if (vmask >> s & 1) X[s * S + item] = X[s * S + item] > 0.0f ? acc[s] : 0.0f;
            }
            wv::wg_barrier();
            float *sw = D; D = X; X = sw;
        }
        if ((K.n_conv + K.n_fc - 1) & 1) { float *sw = D; D = X; X = sw; }
    }
}

// ---- the sum over the workgroups' rows ---------------------------------------------------------------------------------------------------
template <class KP>
PPG_DEVICE void net_reduce_main(const KP &K) {
    const int j = PPG_BLOCK_INDEX() * NET_THREADS + net_thread();
    if (j >= K.n_params) return;
    float sum = K.partial[j];
    for (int g = 1; g < K.G; ++g) sum = sum + K.partial[(size_t)g * K.n_params + j];
    int seg = 0;
    while (seg + 1 < K.n_seg && j >= K.p_off[seg + 1]) ++seg;
    K.grad[seg][j - K.p_off[seg]] = sum;
}

}  // namespace ppg
