// policy_update_san_main.cpp -- TEST-ONLY stand-alone program: the repack map and the word function of ppg_policy_update
// (predpreygrass_amd/csrc/ppg_policy_pack.h, the only project header included: it needs no HIP) built with -fsanitize=address,undefined
// by tests/test_policy_update_sanitized.py.  Every parameter tensor is a heap block of exactly its size and so is the image, so a map
// entry whose index leaves its tensor, or a word written outside the image, traps.  For every shape of tests/policy_update_cases.py the
// image is filled with 0xA5, given a slot table (random words: its section must survive untouched), run through the map --
// ppg_policy_repack_cpu, which calls what the kernel calls -- and compared with the image of ppg_policy_fragments_of, byte for byte.
// Exit status 0 = clean and equal.
#include <stdio.h>
#include <string.h>

#include <memory>

#include "../predpreygrass_amd/csrc/ppg_policy_pack.h"

static uint64_t g_lcg = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_lcg >> 33); }
static float gauss() { return (float)(((double)rnd() + rnd() + rnd() + rnd()) / 2147483648.0 - 2.0) * 1.7f; }

struct Shape {
    int hwc, C, R, n_conv, conv[PPG_POLICY_MAX_CONV], n_hidden, hidden[2], nhwc, A;
};

// tests/policy_update_cases.py: SHAPES
static const Shape SHAPES[] = {
    {1, 4, 7, 3, {16, 32, 64}, 0, {0, 0}, 1, 9},
    {1, 4, 9, 3, {16, 32, 64}, 0, {0, 0}, 1, 9},
    {1, 4, 11, 3, {16, 32, 64}, 0, {0, 0}, 1, 9},
    {1, 5, 15, 3, {16, 32, 64}, 0, {0, 0}, 1, 17},
    {1, 1, 3, 1, {5}, 0, {0, 0}, 1, 1},
    {1, 8, 9, 2, {5, 12}, 0, {0, 0}, 0, 25},
    {0, 4, 9, 3, {16, 32, 64}, 0, {0, 0}, 0, 9},
    {0, 5, 7, 3, {5, 12, 40}, 0, {0, 0}, 1, 32},
    {0, 1, 3, 4, {16, 32, 64, 64}, 0, {0, 0}, 0, 9},
    {0, 8, 5, 5, {16, 24, 40, 64, 64}, 0, {0, 0}, 0, 17},
    {1, 4, 7, 6, {8, 16, 32, 64, 64, 64}, 0, {0, 0}, 1, 9},
    {0, 4, 11, 3, {16, 32, 64}, 0, {0, 0}, 1, 25},
    {1, 4, 9, 3, {16, 32, 64}, 2, {256, 256}, 1, 9},
    {1, 4, 7, 3, {16, 32, 64}, 1, {256, 0}, 1, 9},
    {1, 5, 11, 3, {16, 32, 64}, 2, {96, 160}, 0, 17},
    {0, 4, 9, 3, {16, 32, 64}, 2, {256, 256}, 0, 9},
    {0, 4, 15, 3, {16, 32, 64}, 2, {96, 160}, 1, 32},
    {1, 8, 15, 3, {5, 12, 40}, 1, {256, 0}, 1, 25},
    {1, 1, 3, 3, {16, 32, 64}, 2, {256, 256}, 0, 1},
};

static int run(const Shape &s, int q) {
    ppg_policy_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.obs_channels = s.C; sp.obs_range = s.R; sp.n_actions = s.A;
    sp.layout = s.hwc ? PPG_POLICY_LAYOUT_HWC : PPG_POLICY_LAYOUT_CHW;
    sp.flatten = s.nhwc ? PPG_POLICY_FLATTEN_NHWC : PPG_POLICY_FLATTEN_NCHW;
    sp.n_conv = s.n_conv; sp.n_fc = s.n_hidden + 1;
    for (int l = 0; l < s.n_conv; ++l) sp.conv_out[l] = s.conv[l];
    for (int l = 0; l < s.n_hidden; ++l) sp.fc_out[l] = s.hidden[l];
    sp.fc_out[s.n_hidden] = s.A;
    // every tensor a heap block of exactly its size
    size_t n[PPG_SRC_N];
    ppg_policy_source_sizes(sp, n);
    std::unique_ptr<float[]> tensor[PPG_SRC_N];
    const float *src[PPG_SRC_N];
    for (int t = 0; t < PPG_SRC_N; ++t) {
        src[t] = nullptr;
        if (!n[t]) continue;
        tensor[t].reset(new float[n[t]]);
        for (size_t i = 0; i < n[t]; ++i) tensor[t][i] = gauss();
        src[t] = tensor[t].get();
    }
    // the map knows the shape only; the slot table: none, or some words that nothing may touch
    const size_t slot_words = q % 2 ? 0 : 96 + (size_t)q;
    std::vector<uint16_t> slots(slot_words);
    for (size_t i = 0; i < slot_words; ++i) slots[i] = (uint16_t)rnd();
    std::vector<int32_t> map;
    ppg_policy_image_layout L;
    ppg_policy_map_of(sp, slot_words, map, L);
    if (map.size() != (size_t)PPG_MAP_HEADER + L.off[PPG_FRAG_SLOTS] / 2 + L.n_bias) { fprintf(stderr, "shape %d: the map's size\n", q); return 1; }
    std::unique_ptr<unsigned char[]> got(new unsigned char[L.total]);
    memset(got.get(), 0xA5, L.total);
    memset(got.get() + L.off[PPG_FRAG_SLOTS], 0, L.off[PPG_FRAG_N] - L.off[PPG_FRAG_SLOTS]);
    if (slot_words) memcpy(got.get() + L.off[PPG_FRAG_SLOTS], slots.data(), slot_words * 2);
    ppg_policy_repack_cpu(map.data(), src, got.get());
    // the reference: the values path, with the weight pointers in the spec
    for (int l = 0; l < PPG_POLICY_MAX_CONV; ++l) { sp.conv_w[l] = src[PPG_SRC_CONV_W + l]; sp.conv_b[l] = src[PPG_SRC_CONV_B + l]; }
    for (int l = 0; l < PPG_POLICY_MAX_FC; ++l) { sp.fc_w[l] = src[PPG_SRC_FC_W + l]; sp.fc_b[l] = src[PPG_SRC_FC_B + l]; }
    ppg_policy_fragments F;
    ppg_policy_fragments_of(sp, F);
    const ppg_policy_image_layout P = ppg_policy_image_layout_of(F, slot_words);
    if (P.total != L.total || memcmp(P.off, L.off, sizeof P.off) != 0 || memcmp(P.words, L.words, sizeof P.words) != 0) {
        fprintf(stderr, "shape %d: the map and the fragments disagree about the layout\n", q);
        return 1;
    }
    std::unique_ptr<unsigned char[]> want(new unsigned char[P.total]);
    ppg_policy_image_assemble(F, P, slots.data(), want.get());
    if (memcmp(got.get(), want.get(), P.total) != 0) {
        size_t at = 0;
        while (got[at] == want[at]) ++at;
        fprintf(stderr, "shape %d: the images differ at byte %zu of %zu\n", q, at, P.total);
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0, q = 0;
    for (const Shape &s : SHAPES) bad |= run(s, q++);
    if (!bad) printf("POLICY-UPDATE-SAN-CLEAN\n");
    return bad;
}
