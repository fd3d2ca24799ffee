// ppg_policy_pack.h -- the policy weights in the kernels' operand order, device-free (include/ppg.h: ppg_policy_pack, ppg_policy_image,
// ppg_policy_update).  Needs include/ppg.h and the C++ standard library only: plain g++ compiles it (tests/policy_update_san_main.cpp).
//
// ONE statement of the fragment order serves two consumers.  The pack functions below are templates over an EMITTER that says what a
// word of the result is: ppg_emit_values emits the rounded weight itself (what ppg_policy_create_spec uploads), ppg_emit_map emits WHERE
// the weight comes from -- a parameter tensor and an element index, the constant zero, or the bf16 remainder of a convolution bias.  The
// second result is the REPACK MAP of ppg_policy_update: a kernel (ppg_policy.h: ppg_policy_repack) that gathers through it from
// float32 parameters in device memory produces the image of create, bit for bit, because both sides end in the same word function
// (ppg_repack_value / ppg_repack_word: integer rounding, no hardware convert).
//
// THE IMAGE (ppg_policy::dev_weights): the PPG_FRAG_N arrays of ppg_policy_fragments one behind the other, each rounded up to 256 bytes
// with zeros, the float32 bias block behind them (ppg_policy_image_layout).  The slot table is the last array in front of the bias
// block; it is not a weight, no map entry covers it and an update never writes it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/ppg.h"

#if defined(__HIPCC__)
#define PPG_PACK_HD __host__ __device__
#else
#define PPG_PACK_HD
#endif

// MFMA row r of a 32-row tile computes this feature of the tile (ppg_policy.h: ORIENTATION)
static int ppg_row_feature(int r) { return 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3); }

PPG_PACK_HD static inline uint16_t ppg_bf16_bits(float f) {   // round to nearest even; a NaN stays a (quiet) NaN
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// what bf16 rounding leaves of b: the convolutions carry their bias as a bf16 head plus the bf16 of this remainder (ConvW)
PPG_PACK_HD static inline float ppg_bf16_tail(float b) {
    const uint32_t hb = (uint32_t)ppg_bf16_bits(b) << 16;
    float hf;
    __builtin_memcpy(&hf, &hb, 4);
    return b - hf;
}

// ---- sources: the parameter tensors of a spec, numbered ----
enum { PPG_SRC_CONV_W = 0, PPG_SRC_CONV_B = PPG_POLICY_MAX_CONV, PPG_SRC_FC_W = 2 * PPG_POLICY_MAX_CONV,
       PPG_SRC_FC_B = 2 * PPG_POLICY_MAX_CONV + PPG_POLICY_MAX_FC, PPG_SRC_N = 2 * PPG_POLICY_MAX_CONV + 2 * PPG_POLICY_MAX_FC };

struct ppg_policy_sources { const float *t[PPG_SRC_N]; };

static ppg_policy_sources ppg_policy_sources_of(const ppg_policy_spec &sp) {
    ppg_policy_sources S;
    for (int l = 0; l < PPG_POLICY_MAX_CONV; ++l) { S.t[PPG_SRC_CONV_W + l] = sp.conv_w[l]; S.t[PPG_SRC_CONV_B + l] = sp.conv_b[l]; }
    for (int l = 0; l < PPG_POLICY_MAX_FC; ++l) { S.t[PPG_SRC_FC_W + l] = sp.fc_w[l]; S.t[PPG_SRC_FC_B + l] = sp.fc_b[l]; }
    return S;
}

// elements of every parameter tensor of the spec's shape (0: the spec has no such layer)
static void ppg_policy_source_sizes(const ppg_policy_spec &sp, size_t n[PPG_SRC_N]) {
    const int hwc = sp.layout == PPG_POLICY_LAYOUT_HWC;
    const int CIN = hwc ? sp.obs_range : sp.obs_channels, P = (hwc ? sp.obs_channels : sp.obs_range) * sp.obs_range;
    for (int t = 0; t < PPG_SRC_N; ++t) n[t] = 0;
    int ci = CIN;
    for (int l = 0; l < sp.n_conv; ++l) {
        n[PPG_SRC_CONV_W + l] = (size_t)sp.conv_out[l] * ci * 9;
        n[PPG_SRC_CONV_B + l] = (size_t)sp.conv_out[l];
        ci = sp.conv_out[l];
    }
    size_t fi = (size_t)P * ci;
    for (int l = 0; l < sp.n_fc; ++l) {
        n[PPG_SRC_FC_W + l] = (size_t)sp.fc_out[l] * fi;
        n[PPG_SRC_FC_B + l] = (size_t)sp.fc_out[l];
        fi = (size_t)sp.fc_out[l];
    }
}

// ---- a map entry (one int32 per bf16 word of the weight arrays and per float of the bias block; include/ppg.h: PPG_POLICY_IMAGE_MAP) ----
//   0                                            the constant zero
//   (tensor + 1) << 24 | element                 that element of source tensor `tensor` (PPG_SRC_*); element < 2^24
//   ... | PPG_MAP_TAIL                           the bf16 remainder of that element (ppg_bf16_tail)
enum { PPG_MAP_INDEX_BITS = 24, PPG_MAP_TAIL = 1 << 29 };

static inline int32_t ppg_map_entry(int tensor, size_t element) { return (int32_t)(((uint32_t)(tensor + 1) << PPG_MAP_INDEX_BITS) | (uint32_t)element); }

// The value a map entry stands for, in two steps so that a caller can have many gathers in flight before it finishes the first;
// `src[tensor]` is the tensor's first element (a table of PPG_SRC_N pointers: a plain array on the host, the kernel's parameter block
// on the device).  Both the kernel and the CPU path call these and nothing else.
//   fetch:  the element the entry names.  No branch around the loads: the constant zero reads element 0 of tensor 0 -- conv_w[0],
//           which every network has -- and finish drops it.
//   finish: the element itself, what bfloat16 leaves of it, or zero.
template <class Table>
PPG_PACK_HD static inline float ppg_repack_fetch(int32_t e, const Table &src) {
    const int t = e ? ((e >> PPG_MAP_INDEX_BITS) & 31) - 1 : 0;
    return src[t][e & ((1 << PPG_MAP_INDEX_BITS) - 1)];
}
PPG_PACK_HD static inline float ppg_repack_finish(int32_t e, float v) {
    const float r = (e & PPG_MAP_TAIL) ? ppg_bf16_tail(v) : v;
    return e ? r : 0.0f;
}
template <class Table>
PPG_PACK_HD static inline float ppg_repack_value(int32_t e, const Table &src) { return ppg_repack_finish(e, ppg_repack_fetch(e, src)); }
// ... as the bf16 word of a weight array (the bias block takes the value itself)
template <class Table>
PPG_PACK_HD static inline uint16_t ppg_repack_word(int32_t e, const Table &src) { return ppg_bf16_bits(ppg_repack_value(e, src)); }

// ---- emitters: what the pack functions write for "element i of tensor t" ----
struct ppg_emit_values {   // the weight itself: bf16 bits in the arrays, float in the bias block
    typedef uint16_t word;
    typedef float fword;
    const float *const *src;
    word at(int t, size_t i) const { return ppg_bf16_bits(src[t][i]); }
    word tail(int t, size_t i) const { return ppg_bf16_bits(ppg_bf16_tail(src[t][i])); }
    fword f32(int t, size_t i) const { return src[t][i]; }
};
struct ppg_emit_map {      // where it comes from
    typedef int32_t word;
    typedef int32_t fword;
    word at(int t, size_t i) const { return ppg_map_entry(t, i); }
    word tail(int t, size_t i) const { return ppg_map_entry(t, i) | PPG_MAP_TAIL; }
    fword f32(int t, size_t i) const { return ppg_map_entry(t, i); }
};
// (a word no emitter call writes is the value-initialised one: bf16 zero, or the map's "constant zero")

// conv weights [cout][cin][3][3] (tensor tw, bias tensor tb) -> fragments [mt][ks][lane][8]: lane (r = lane & 31, h = lane >> 5) holds,
// for K block q = 2 ks + h = tap * CBIN + cb, the eight input channels 8 cb .. 8 cb + 7 of output channel 32 mt + r at tap (ky, kx)
template <class E>
static void ppg_pack_conv(const E &emit, int tw, int tb, int cout, int cin, int cbin, int mt_n, std::vector<typename E::word> &out) {
    const int Q = 9 * cbin, KS = (Q + 2) / 2;   // (block Q = the bias, ConvW)
    out.assign((size_t)mt_n * KS * 64 * 8, typename E::word());
    for (int mt = 0; mt < mt_n; ++mt)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 31, h = lane >> 5, q = 2 * ks + h, co = 32 * mt + ppg_row_feature(r);
                if (q > Q || co >= cout) continue;
                typename E::word *dst = &out[(((size_t)mt * KS + ks) * 64 + lane) * 8];
                if (q == Q) {   // bias = bf16 head + bf16 remainder
                    dst[0] = emit.at(tb, (size_t)co);
                    dst[1] = emit.tail(tb, (size_t)co);
                    continue;
                }
                const int tap = q / cbin, cb = q % cbin;
                for (int j = 0; j < 8; ++j) {
                    const int ci = 8 * cb + j;
                    if (ci < cin) dst[j] = emit.at(tw, ((size_t)co * cin + ci) * 9 + tap);
                }
            }
}

// conv1 of the pipeline kernels as fragments of v_mfma_f32_16x16x32_bf16 (ppg_policy_pipe.h: Conv1X), [ky][lane][8]: lane (r = lane &
// 15 = output channel, kq = lane >> 4) holds for kernel row ky -- kq < 3: the eight input channels 0-7 at tap (ky, kx = kq); kq = 3: the
// ninth input channel at the taps kx = 0, 1, 2 (elements 0-2; the rest zero).  cin <= 9.
template <class E>
static void ppg_pack_conv1x(const E &emit, int tw, int cout, int cin, std::vector<typename E::word> &out) {
    out.assign((size_t)3 * 64 * 8, typename E::word());
    for (int ky = 0; ky < 3; ++ky)
        for (int lane = 0; lane < 64; ++lane) {
            const int co = lane & 15, kq = lane >> 4;
            if (co >= cout) continue;
            typename E::word *dst = &out[((size_t)ky * 64 + lane) * 8];
            for (int j = 0; j < 8; ++j) {
                const int ci = kq < 3 ? j : 8, kx = kq < 3 ? kq : j;
                if (ci < cin && kx < 3) dst[j] = emit.at(tw, ((size_t)co * cin + ci) * 9 + ky * 3 + kx);
            }
        }
}

// A Linear layer -> fragments [ks][mt][lane][8] of the 32x32x16 MFMA: lane holds output feature o = 32 mt + row feature(lane & 31) and
// inputs k = 16 ks + 8 h + j; `value(o, k)` returns the word of that weight (the value-initialised word for padding)
template <class Word, class Value>
static void ppg_pack_fc(int K, int mt_n, Value value, std::vector<Word> &out) {
    const int KS = K / 16;
    out.assign((size_t)KS * mt_n * 64 * 8, Word());
    for (int ks = 0; ks < KS; ++ks)
        for (int mt = 0; mt < mt_n; ++mt)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 31, h = lane >> 5, o = 32 * mt + ppg_row_feature(r);
                for (int j = 0; j < 8; ++j)
                    out[(((size_t)ks * mt_n + mt) * 64 + lane) * 8 + j] = value(o, 16 * ks + 8 * h + j);
            }
}

// the single Linear head (tensor th) of a network without hidden head layers -> fragments of v_mfma_f32_16x16x32_bf16, [action tile][k-step][lane][8]:
// lane holds action 16 tile + (lane & 15) and the features of area F's elements 32 ks + 8 (lane >> 4) + j; F is [position][flat_c
// channels] (flat_c = the last convolution's channels padded to blocks of 8); `nhwc`: which feature (channel c, position q) is
template <class E>
static void ppg_pack_head(const E &emit, int th, int n_actions, int P, int cout_last, bool nhwc, std::vector<typename E::word> &out) {
    const int flat_c = (cout_last + 7) / 8 * 8, ksteps = (P * flat_c + 31) / 32, head_mt = (n_actions + 15) / 16, flat = P * cout_last;
    out.assign((size_t)head_mt * ksteps * 64 * 8, typename E::word());
    for (int mt = 0; mt < head_mt; ++mt)
        for (int ks = 0; ks < ksteps; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int a = 16 * mt + (lane & 15);
                if (a >= n_actions) continue;
                for (int j = 0; j < 8; ++j) {
                    const int e = 32 * ks + 8 * (lane >> 4) + j, q = e / flat_c, c = e % flat_c;
                    const int ft = (q < P && c < cout_last) ? (nhwc ? q * cout_last + c : c * P + q) : -1;
                    if (ft >= 0) out[(((size_t)mt * ksteps + ks) * 64 + lane) * 8 + j] = emit.at(th, (size_t)a * flat + ft);
                }
            }
}

// The weights of a spec in the kernels' operand order, one vector per device array: the convolutions, then up to three linear layers (a
// direct head: wh, whw), conv1 in the pipeline's form, the pipeline's slot table (ppg_policy_layout::slot_tab: not a weight, uploaded with them)
enum { PPG_FRAG_FC = PPG_POLICY_MAX_CONV, PPG_FRAG_CONV1X = PPG_POLICY_MAX_CONV + 3, PPG_FRAG_SLOTS, PPG_FRAG_N };
enum { PPG_POLICY_BIAS_FLOATS = 256 + 256 + 32 + 16 };
template <class Word, class FWord>
struct ppg_policy_fragments_t {
    std::vector<Word> f[PPG_FRAG_N];
    std::vector<FWord> bias;   // FC chain: b1, b2, b3 at [0], [256], [512]; direct: head bias at [512]; the pipeline's conv1 bias at [544]
};
typedef ppg_policy_fragments_t<uint16_t, float> ppg_policy_fragments;
typedef ppg_policy_fragments_t<int32_t, int32_t> ppg_policy_fragment_map;

// sp: a spec ppg_policy_check_spec accepts (its weight pointers are read by the emitter only); f[PPG_FRAG_SLOTS] stays empty
template <class E>
static void ppg_policy_fragments_of(const ppg_policy_spec &sp, const E &emit, ppg_policy_fragments_t<typename E::word, typename E::fword> &F) {
    typedef typename E::word Word;
    const int hwc = sp.layout == PPG_POLICY_LAYOUT_HWC, n_actions = sp.n_actions;
    const int CIN = hwc ? sp.obs_range : sp.obs_channels, P = (hwc ? sp.obs_channels : sp.obs_range) * sp.obs_range;
    const int cout_last = sp.conv_out[sp.n_conv - 1];
    const int flat = P * cout_last;   // features behind the flatten
    const bool nhwc = sp.flatten == PPG_POLICY_FLATTEN_NHWC;
    std::vector<typename E::fword> &bias = F.bias;
    bias.assign(PPG_POLICY_BIAS_FLOATS, typename E::fword());
    int ci = CIN;
    for (int l = 0; l < sp.n_conv; ++l) {   // input channel blocks: conv1 one or two, then 2, 4, 8; output row tiles: 1, 1, then 2
        ppg_pack_conv(emit, PPG_SRC_CONV_W + l, PPG_SRC_CONV_B + l, sp.conv_out[l], ci, l == 0 ? (CIN > 8 ? 2 : 1) : l == 1 ? 2 : l == 2 ? 4 : 8, l < 2 ? 1 : 2, F.f[l]);
        ci = sp.conv_out[l];
    }
    if (CIN <= 9) {
        ppg_pack_conv1x(emit, PPG_SRC_CONV_W, sp.conv_out[0], CIN, F.f[PPG_FRAG_CONV1X]);
        for (int c = 0; c < sp.conv_out[0] && c < 16; ++c) bias[544 + c] = emit.f32(PPG_SRC_CONV_B, (size_t)c);
    }
    if (sp.n_fc == 1) {
        std::vector<Word> &wh = F.f[PPG_FRAG_FC], &whw = F.f[PPG_FRAG_FC + 1];
        ppg_pack_head(emit, PPG_SRC_FC_W, n_actions, P, cout_last, nhwc, wh);
        for (int a = 0; a < n_actions; ++a) bias[512 + a] = emit.f32(PPG_SRC_FC_B, (size_t)a);
        // whw: wavefront w owns k-steps [w per, (w + 1) per) of action tile 0, its first 18 ride in registers (ppg_policy_direct.h)
        const int ksteps = (P * ((cout_last + 7) / 8 * 8) + 31) / 32, HFR = 18, per = (ksteps + 3) / 4;
        whw.assign((size_t)4 * HFR * 64 * 8, Word());
        for (int w = 0; w < 4; ++w)
            for (int i = 0; i < HFR && i < per; ++i) {
                const int ks = w * per + i;
                if (ks >= ksteps) break;
                for (int k = 0; k < 64 * 8; ++k) whw[((size_t)w * HFR + i) * 64 * 8 + k] = wh[(size_t)ks * 64 * 8 + k];
            }
        return;
    }
    // FC1: the K order is the scratch slot's [row tile of conv3][position][32 channels]; hidden widths are zero-padded to 256
    const int h1 = sp.fc_out[0], h2 = sp.n_fc == 3 ? sp.fc_out[1] : 0;
    // feature index of (channel c, position q) behind the flatten, or -1 for a padding channel
    auto feature = [=](int c, int q) { return c >= cout_last ? -1 : nhwc ? q * cout_last + c : c * P + q; };
    ppg_pack_fc(64 * P, 8, [&](int o, int k) -> Word {
        const int c = 32 * (k / (32 * P)) + k % 32, q = (k % (32 * P)) / 32, ft = feature(c, q);
        return (o < h1 && ft >= 0) ? emit.at(PPG_SRC_FC_W, (size_t)o * flat + ft) : Word(); }, F.f[PPG_FRAG_FC]);
    for (int i = 0; i < h1; ++i) bias[i] = emit.f32(PPG_SRC_FC_B, (size_t)i);
    if (sp.n_fc == 3) {
        ppg_pack_fc(256, 8, [&](int o, int k) -> Word { return (o < h2 && k < h1) ? emit.at(PPG_SRC_FC_W + 1, (size_t)o * h1 + k) : Word(); }, F.f[PPG_FRAG_FC + 1]);
        for (int i = 0; i < h2; ++i) bias[256 + i] = emit.f32(PPG_SRC_FC_B + 1, (size_t)i);
    }
    const int last = sp.n_fc - 1, hl = sp.n_fc == 3 ? h2 : h1;
    ppg_pack_fc(256, 1, [&](int o, int k) -> Word { return (o < n_actions && k < hl) ? emit.at(PPG_SRC_FC_W + last, (size_t)o * hl + k) : Word(); }, F.f[PPG_FRAG_FC + 2]);
    for (int i = 0; i < n_actions; ++i) bias[512 + i] = emit.f32(PPG_SRC_FC_B + last, (size_t)i);
}

// the values: sp's weight pointers are host arrays
static void ppg_policy_fragments_of(const ppg_policy_spec &sp, ppg_policy_fragments &F) {
    const ppg_policy_sources S = ppg_policy_sources_of(sp);
    const ppg_emit_values emit = {S.t};
    ppg_policy_fragments_of(sp, emit, F);
}

// ---- the image: where each array lies in dev_weights (the ONE definition: create, the map and ppg_policy_image use it) ----
struct ppg_policy_image_layout {
    size_t off[PPG_FRAG_N + 1];   // byte offset of array l, a multiple of 256; [PPG_FRAG_N] = the float32 bias block
    size_t words[PPG_FRAG_N];     // bf16 words array l holds (the bytes behind them, up to the next offset, are zero)
    size_t n_bias;                // floats of the bias block
    size_t total;                 // bytes of the image
};

// slot_words: words of the slot table (F.f[PPG_FRAG_SLOTS] is not looked at: only fragments of values could hold it)
template <class Word, class FWord>
static ppg_policy_image_layout ppg_policy_image_layout_of(const ppg_policy_fragments_t<Word, FWord> &F, size_t slot_words) {
    ppg_policy_image_layout L;
    size_t total = 0;
    for (int l = 0; l < PPG_FRAG_N; ++l) {
        L.words[l] = l == PPG_FRAG_SLOTS ? slot_words : F.f[l].size();
        L.off[l] = total;
        total += (L.words[l] * 2 + 255) / 256 * 256;
    }
    L.off[PPG_FRAG_N] = total;
    L.n_bias = F.bias.size();
    L.total = total + L.n_bias * 4;
    return L;
}

// image[L.total] = the arrays of F, `slot_tab` (L.words[PPG_FRAG_SLOTS] words; may be NULL when there are none), zeros between them, the bias block
static void ppg_policy_image_assemble(const ppg_policy_fragments &F, const ppg_policy_image_layout &L, const uint16_t *slot_tab, unsigned char *image) {
    __builtin_memset(image, 0, L.total);
    for (int l = 0; l < PPG_FRAG_N; ++l) {
        const uint16_t *from = l == PPG_FRAG_SLOTS ? slot_tab : F.f[l].data();
        if (L.words[l]) __builtin_memcpy(image + L.off[l], from, L.words[l] * 2);
    }
    __builtin_memcpy(image + L.off[PPG_FRAG_N], F.bias.data(), L.n_bias * 4);
}

// ---- the repack map (include/ppg.h: PPG_POLICY_IMAGE_MAP) ----
// PPG_MAP_HEADER words: [0] PPG_MAP_HEADER, [1] W = bf16 words the map covers = image bytes [0, 2 W) = every array in front of the slot
// table (a multiple of 128), [2] floats of the bias block, [3] bytes of the image, [4] byte offset of the bias block, [5 + l] byte offset
// of array l, [5 + PPG_FRAG_N + l] bf16 words of array l (l < PPG_FRAG_N), the rest zero.  Then W entries, one per bf16 word from image
// byte 0 on (the zeros that pad an array are entries too), then one entry per float of the bias block.
enum { PPG_MAP_HEADER = 32 };
static_assert(5 + 2 * PPG_FRAG_N <= PPG_MAP_HEADER, "the map header holds both per-array tables");

// sp: a spec ppg_policy_check_spec accepts; its weight pointers are not read
static void ppg_policy_map_of(const ppg_policy_spec &sp, size_t slot_words, std::vector<int32_t> &map, ppg_policy_image_layout &L) {
    ppg_policy_fragment_map F;
    ppg_policy_fragments_of(sp, ppg_emit_map(), F);
    L = ppg_policy_image_layout_of(F, slot_words);
    const size_t W = L.off[PPG_FRAG_SLOTS] / 2;
    map.assign(PPG_MAP_HEADER + W + L.n_bias, 0);
    map[0] = PPG_MAP_HEADER; map[1] = (int32_t)W; map[2] = (int32_t)L.n_bias; map[3] = (int32_t)L.total; map[4] = (int32_t)L.off[PPG_FRAG_N];
    for (int l = 0; l < PPG_FRAG_N; ++l) { map[5 + l] = (int32_t)L.off[l]; map[5 + PPG_FRAG_N + l] = (int32_t)L.words[l]; }
    for (int l = 0; l < PPG_FRAG_SLOTS; ++l)
        for (size_t i = 0; i < F.f[l].size(); ++i) map[PPG_MAP_HEADER + L.off[l] / 2 + i] = F.f[l][i];
    for (size_t i = 0; i < L.n_bias; ++i) map[PPG_MAP_HEADER + W + i] = F.bias[i];
}

// What the update kernel does, on the CPU: every word the map covers is written, nothing else is touched.
static void ppg_policy_repack_cpu(const int32_t *map, const float *const *src, unsigned char *image) {
    const size_t W = (size_t)map[1], n_bias = (size_t)map[2], bias_off = (size_t)map[4];
    const int32_t *e = map + map[0];
    for (size_t i = 0; i < W; ++i) {
        const uint16_t w = ppg_repack_word(e[i], src);
        __builtin_memcpy(image + 2 * i, &w, 2);
    }
    for (size_t i = 0; i < n_bias; ++i) {
        const float v = ppg_repack_value(e[W + i], src);
        __builtin_memcpy(image + bias_off + 4 * i, &v, 4);
    }
}
