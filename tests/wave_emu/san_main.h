// san_main.h -- TEST-ONLY: what the stand-alone sanitizer programs (tests/*_san_main.cpp) share: the emulator with its fiber switch,
// one LCG whose seed each program sets first thing in main(), and the launch of a kernel main over a grid of one-wave workgroups.
#pragma once

#include "wave_emu.h"

#include <math.h>

#include <vector>

#include "ctx_switch.h"

static uint64_t g_lcg;
static void lcg_seed(uint64_t s) { g_lcg = s; }
static uint32_t rnd() {
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_lcg >> 33);
}
static int below(int n) { return (int)(rnd() % (uint32_t)n); }
static double unit() { return (double)rnd() / 2147483648.0; }
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xFFFFFF) / 16777216.0f; }

// `grid` workgroups of Main with exactly LDS bytes each (the emulator poisons the bytes behind them); the second form is for a main
// that takes no LDS (16 bytes, which it never sees)
template <class P, void (*Main)(const P &, unsigned char *), int LDS>
static void run_grid(const P &K, int grid) {
    for (int b = 0; b < grid; ++b)
        wv::run_block([](void *arg) { Main(*(const P *)arg, wv::emu().lds); }, (void *)&K, b, LDS, 1);
}
template <class P, void (*Main)(const P &)>
static void run_grid(const P &K, int grid) {
    for (int b = 0; b < grid; ++b) wv::run_block([](void *arg) { Main(*(const P *)arg); }, (void *)&K, b, 16, 1);
}
